"""Diagnostic: ms per 1920 x 1080 wave of the projector-in-fog scene of tests/test_imagelight_gpu.py (tests/imagelight_model.py::FogProjector:
a homogeneous grey medium, one projection light with a 2 x 2 slide, a black backdrop, maxdepth 1) on the default kernel and on the
per-lane kernel (VSPG_KERNEL=lane), and beside it, on the same commit, the same scene lit by a spot light of the projection's
bounding cone (same position and axis, cone angle = the angle of the screen window's corner, no falloff band).

  python scripts/imagelight_timing.py [--rounds 5] [--waves 4] [--out profiles/imagelight_timing.json]

One renderer per configuration; the rounds alternate between the configurations, so drift of the machine lands on all of them
alike.  A round times `waves` one-sample waves between two device synchronisations after the warm-up waves; the figure per
configuration is the median over the rounds, with the minimum and the maximum next to it, and segments and shadow rays per path."""
import argparse
import json
import math
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
import imagelight_model as M
import scenes

W, H = 1920, 1080
F = M.FogProjector()
F.W, F.H = W, H


def fog_scene(light):
    s = scenes.empty_scene(W, H, eye=F.eye, look=F.look, up=F.up, fov=F.fov)
    m = s.medium
    m.type = P.MEDIUM_HOMOGENEOUS
    m.sigma_a[:] = (F.sigma_a,) * 3
    m.sigma_s[:] = (F.sigma_s,) * 3
    m.g = F.g
    scenes.add_quad(s, (-6, -6, F.z_wall), (12, 0, 0), (0, 12, 0), kd=(0, 0, 0))
    if light == "projection":
        return s, P.add_projection_light(s, F.I, fov=F.proj_fov, ctm=F.ctm())
    pos, axis, phi, cos_o, cos_e = F.light.bounds()      # the spot of the projection's bounding cone
    mean = F.SLIDE.reshape(-1, 3).mean(axis=0)
    P.add_spot_light(s, [float(a * b) for a, b in zip(F.I, mean)], [float(v) for v in pos], [float(a + b) for a, b in zip(pos, axis)],
                     coneangle=math.degrees(math.acos(float(cos_e))), conedelta=0.0)
    return s, None


def make(light, kernel):
    if kernel:
        os.environ["VSPG_KERNEL"] = kernel
    try:
        prm = P.app_f_params()
        prm.maxdepth = 1
        s, slot = fog_scene(light)
        r = P.Renderer(s, prm, W, H)
        if slot is not None:
            r.set_light_image(slot, F.SLIDE)
        for w in range(args.warmup):
            r.render_wave(w, w + 1)
            r.post_process_wave()
        torch.cuda.synchronize()
        return r, r.kernel_name()
    finally:
        os.environ.pop("VSPG_KERNEL", None)


configs = {"projection, default": ("projection", None), "projection, lane": ("projection", "lane"), "spot, default": ("spot", None), "spot, lane": ("spot", "lane")}
renderers = {k: make(*v) for k, v in configs.items()}
times = {k: [] for k in configs}
wave = args.warmup
for rnd in range(args.rounds):
    for k, (_, kernel) in configs.items():
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
result = {"workload": "projector in fog 1920x1080, maxdepth 1", "rounds": args.rounds, "waves_per_round": args.waves, "ms_per_wave": {}}
for k in configs:
    r, name = renderers[k]
    c = r.counters()
    result["ms_per_wave"][k] = {"median": statistics.median(times[k]), "min": min(times[k]), "max": max(times[k]), "kernel": name,
                                "segments_per_path": c["segments"] / max(1, c["paths"]), "shadow_rays_per_path": c["shadow_rays"] / max(1, c["paths"])}
    print("%-22s %-38s median %.3f ms/wave (min %.3f, max %.3f)  seg/path %.2f  shadow/path %.2f" % (
        k, name, result["ms_per_wave"][k]["median"], min(times[k]), max(times[k]), result["ms_per_wave"][k]["segments_per_path"],
        result["ms_per_wave"][k]["shadow_rays_per_path"]))
    r.close()
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
