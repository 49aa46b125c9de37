"""Diagnostic: ms per 1920 x 1080 wave of the spot-in-fog scene of tests/test_pointlight_gpu.py (tests/pointlight_model.py::FogSpot: a
homogeneous grey medium, one spot light, a black backdrop, maxdepth 1) on the default kernel and on the per-lane kernel
(VSPG_KERNEL=lane), and of the same scene at the integrator's default depth.

  python scripts/pointlight_timing.py [--rounds 5] [--waves 4] [--out file.json]

One renderer per configuration; the rounds alternate between the configurations, so drift of the machine lands on all of them
alike.  A round times `waves` one-sample waves between two device synchronisations after the warm-up waves; the figure per
configuration is the median over the rounds, with the minimum and the maximum next to it."""
import argparse
import json
import os
import statistics
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import torch

import __graft_entry__ as g

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--waves", type=int, default=4)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()

P = g.load_package()
P.load()
import pointlight_model as M
import test_pointlight_gpu as T

W, H = 1920, 1080
F = M.FogSpot()
F.W, F.H = W, H


def make(kernel, maxdepth):
    if kernel:
        os.environ["VSPG_KERNEL"] = kernel
    try:
        prm = P.app_f_params()
        prm.maxdepth = maxdepth
        r = P.Renderer(T.fog_spot_scene(P, F), prm, W, H)
        for w in range(args.warmup):
            r.render_wave(w, w + 1)
            r.post_process_wave()
        torch.cuda.synchronize()
        return r, r.kernel_name()
    finally:
        os.environ.pop("VSPG_KERNEL", None)


configs = {"default, maxdepth 1": (None, 1), "lane, maxdepth 1": ("lane", 1), "default, maxdepth 5": (None, 5), "lane, maxdepth 5": ("lane", 5)}
renderers = {k: make(*v) for k, v in configs.items()}
times = {k: [] for k in configs}
wave = args.warmup
for rnd in range(args.rounds):
    for k, (kernel, _) in configs.items():
        r = renderers[k][0]
        if kernel:      # (the choice is read at every launch)
            os.environ["VSPG_KERNEL"] = kernel
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for w in range(wave, wave + args.waves):
            r.render_wave(w, w + 1)
        torch.cuda.synchronize()
        times[k].append((time.perf_counter() - t0) / args.waves * 1e3)
        os.environ.pop("VSPG_KERNEL", None)
    wave += args.waves
result = {"workload": "spot in fog 1920x1080", "rounds": args.rounds, "waves_per_round": args.waves, "ms_per_wave": {}}
for k in configs:
    r, name = renderers[k]
    c = r.counters()
    result["ms_per_wave"][k] = {"median": statistics.median(times[k]), "min": min(times[k]), "max": max(times[k]), "kernel": name,
                                "segments_per_path": c["segments"] / max(1, c["paths"]), "shadow_rays_per_path": c["shadow_rays"] / max(1, c["paths"])}
    print("%-20s %-38s median %.3f ms/wave (min %.3f, max %.3f)  seg/path %.2f  shadow/path %.2f" % (
        k, name, result["ms_per_wave"][k]["median"], min(times[k]), max(times[k]), result["ms_per_wave"][k]["segments_per_path"],
        result["ms_per_wave"][k]["shadow_rays_per_path"]))
    r.close()
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
