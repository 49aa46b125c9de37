"""Diagnostic: ms per 1920 x 1080 wave of the lamp-in-fog scene (a homogeneous grey medium over a floor, one small emissive sphere, the
integrator's App.-F parameters) on the default kernel and on the per-lane kernel (VSPG_KERNEL=lane), next to the same scene with the
lamp replaced by a two-sided emissive rectangle of equal power: Phi_sphere = Pi * 4 Pi r^2 * L, Phi_rect = Pi * 2 * a^2 * L' with
a = 2 r gives L' = (Pi / 2) * L.  The rectangle scene keeps a NON-emissive sphere of the lamp's size, so both run the full-scene
kernels and the difference is the light alone.

  python scripts/spherelight_timing.py [--rounds 5] [--waves 4] [--out file.json]

One renderer per configuration; the rounds alternate between the configurations, so drift of the machine lands on all of them
alike.  A round times `waves` one-sample waves between two device synchronisations after the warm-up waves; the figure per
configuration is the median over the rounds, with the minimum and the maximum next to it.  On a build without sphere lights the
sphere configurations are left out (the rectangle ones are the comparison that build can run)."""
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
import scenes

W, H = 1920, 1080
CENTER, RADIUS, L = (0.3, -0.2, 0.5), 0.4, (5.0, 4.0, 3.0)


def scene(light):
    s = scenes.empty_scene(W, H, eye=(0, 0.3, -3), look=(0, 0, 0))
    m = s.medium
    m.type = P.MEDIUM_HOMOGENEOUS
    m.sigma_a[:] = (0.05, 0.05, 0.05)
    m.sigma_s[:] = (0.4, 0.4, 0.4)
    m.g = 0.3
    scenes.add_quad(s, (-6, -1.25, -6), (0, 0, 12), (12, 0, 0), kd=(0.4, 0.35, 0.3))
    scenes.add_sphere(s, CENTER, RADIUS, kd=(0.2, 0.2, 0.2))
    if light == "sphere":
        P.add_sphere_light(s, 0, L)
    else:      # a two-sided square of side 2 r above the sphere, equal power
        a = 2 * RADIUS
        scenes.add_quad(s, (CENTER[0] - a / 2, CENTER[1] + 1.5 * RADIUS, CENTER[2] - a / 2), (a, 0, 0), (0, 0, a), kd=(0, 0, 0),
                        le=tuple(math.pi / 2 * v for v in L), two_sided=1)
    return s


def make(light, kernel):
    if kernel:
        os.environ["VSPG_KERNEL"] = kernel
    try:
        r = P.Renderer(scene(light), P.app_f_params(), W, H)
        for w in range(args.warmup):
            r.render_wave(w, w + 1)
            r.post_process_wave()
        torch.cuda.synchronize()
        return r, r.kernel_name()
    finally:
        os.environ.pop("VSPG_KERNEL", None)


configs = {"rectangle, default": ("rectangle", None), "rectangle, lane": ("rectangle", "lane")}
if hasattr(P, "add_sphere_light"):
    configs.update({"sphere, default": ("sphere", None), "sphere, lane": ("sphere", "lane")})
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
result = {"workload": "lamp in fog 1920x1080", "rounds": args.rounds, "waves_per_round": args.waves, "ms_per_wave": {}}
for k in configs:
    r, name = renderers[k]
    c = r.counters()
    result["ms_per_wave"][k] = {"median": statistics.median(times[k]), "min": min(times[k]), "max": max(times[k]), "kernel": name,
                                "segments_per_path": c["segments"] / max(1, c["paths"]), "shadow_rays_per_path": c["shadow_rays"] / max(1, c["paths"])}
    print("%-20s %-38s median %.3f ms/wave (min %.3f, max %.3f)  seg/path %.2f  shadow/path %.2f" % (
        k, name, result["ms_per_wave"][k]["median"], min(times[k]), max(times[k]), result["ms_per_wave"][k]["segments_per_path"],
        result["ms_per_wave"][k]["shadow_rays_per_path"]))
    r.close()
if "sphere, default" in configs:
    result["sphere_over_rectangle"] = {k: result["ms_per_wave"]["sphere, " + k]["median"] / result["ms_per_wave"]["rectangle, " + k]["median"] for k in ("default", "lane")}
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
