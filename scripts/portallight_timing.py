"""Diagnostic: ms per 1080p wave of the cloud-scene shape (bench.py --workload cloud-scene) lit by (a) an image sky and (b) the same
image behind a portal -- a 4 x 4 window at height 3 above the cloud, facing up --, at 1024^2 and 4096^2 texels; and, from the probe,
the bisection trip counts of the portal light's SampleLi.

  python scripts/portallight_timing.py [--rounds 5] [--waves 4] [--out profiles/portallight_timing.json]

Each configuration keeps one renderer; the rounds alternate between the configurations (a1024, b1024, a4096, b4096, a1024, ...), so
drift of the machine lands on all of them alike.  A round times `waves` one-sample waves between two device synchronisations after the
renderer's warm-up waves; the figure per configuration is the median over the rounds, with the minimum and the maximum next to it.
The host build time of each portal light (vspg_renderer_set_portal_environment_image, sequential host work) is recorded too."""
import argparse
import json
import os
import statistics
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import torch

import __graft_entry__ as g

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--waves", type=int, default=4)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--probe", type=int, default=1 << 16)
ap.add_argument("--out", default=None)
args = ap.parse_args()

P = g.load_package()
P.load()
import envlight_model as M

W, H = 1920, 1080
SKY, SUN, SUN_DIR = (0.25, 0.35, 0.5), (6.0, 5.5, 5.0), (0.4, 0.8, -0.3)
PORTAL = np.array([[-2, 3, -2], [2, 3, -2], [2, 3, 2], [-2, 3, 2]], np.float32)   # portalFrame z = +y


def image_sky(res):
    img = np.empty((res, res, 3), np.float32)
    img[...] = np.array(SKY, np.float32)
    d = np.array(SUN_DIR, np.float64)
    d = (d / np.linalg.norm(d)).astype(np.float32)[None, :]
    u, v = M.sphere_to_square(d)
    px, py = min(int(u[0] * res), res - 1), min(int(v[0] * res), res - 1)
    img[py, px] += np.array(SUN, np.float32) * np.float32(res * res / (4 * np.pi))
    return img


build_ms = {}


def make(kind):
    res, portal = int(kind.split("^")[0].split()[-1]), kind.startswith("portal")
    scene = P.cloud_scene(W, H, 256)
    scene.n_infinite_lights = 0
    P.add_infinite_light(scene, P.LIGHT_IMAGE_INFINITE, (1.0, 1.0, 1.0))
    r = P.Renderer(scene, P.app_f_params(), W, H)
    t0 = time.perf_counter()
    if portal:
        r.set_portal_environment_image(0, image_sky(res), PORTAL)
    else:
        r.set_environment_image(0, image_sky(res))
    build_ms[kind] = (time.perf_counter() - t0) * 1e3
    for w in range(args.warmup):
        r.render_wave(w, w + 1)
        r.post_process_wave()
    torch.cuda.synchronize()
    r.reset_counters()
    return r


kinds = ["image 1024^2", "portal 1024^2", "image 4096^2", "portal 4096^2"]
renderers = {k: make(k) for k in kinds}
times = {k: [] for k in kinds}
wave = args.warmup
for rnd in range(args.rounds):
    for k in kinds:
        r = renderers[k]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for w in range(wave, wave + args.waves):
            r.render_wave(w, w + 1)
        torch.cuda.synchronize()
        times[k].append((time.perf_counter() - t0) / args.waves * 1e3)
    wave += args.waves
result = {"workload": "cloud-scene 1920x1080, 256^3 grid, one image sky", "rounds": args.rounds, "waves_per_round": args.waves, "ms_per_wave": {},
          "set_call_ms_including_image_generation": build_ms, "bisection_trips": {}}
rng = np.random.default_rng(1)
for k in kinds:
    r = renderers[k]
    c = r.counters()
    result["ms_per_wave"][k] = {"median": statistics.median(times[k]), "min": min(times[k]), "max": max(times[k]), "kernel": r.kernel_name(),
                                "segments_per_path": c["segments"] / max(1, c["paths"]), "shadow_rays_per_path": c["shadow_rays"] / max(1, c["paths"])}
    print("%-14s %-36s median %.3f ms/wave (min %.3f, max %.3f)  seg/path %.2f  shadow/path %.2f" % (
        k, r.kernel_name(), result["ms_per_wave"][k]["median"], min(times[k]), max(times[k]), result["ms_per_wave"][k]["segments_per_path"],
        result["ms_per_wave"][k]["shadow_rays_per_path"]))
    if k.startswith("portal"):   # context points in the cloud's box, as NEE meets them
        n = args.probe
        p = rng.uniform((-0.8, -0.5, -0.8), (0.8, 0.9, 0.8), (n, 3)).astype(np.float32)
        o = r.portallight_batch(0, p, np.tile(np.float32([0, 1, 0]), (n, 1)), rng.uniform(0, 1, (n, 2)).astype(np.float32))
        ok = o[:, 12] == 1
        result["bisection_trips"][k] = {"samples": int(ok.sum()), "of": n, "mean_x": float(o[ok, 24].mean()), "max_x": int(o[ok, 24].max()),
                                        "mean_y": float(o[ok, 25].mean()), "max_y": int(o[ok, 25].max())}
        print("   bisection trips:", result["bisection_trips"][k])
    r.close()
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
