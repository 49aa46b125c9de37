"""Diagnostic: what a camera model costs per 1920 x 1080 wave, against the pinhole on the SAME kernel:
  fog    the App.-F fog box with one small triangle in a corner, so that the pinhole runs the full-scene kernel too
         (k_render_wave_wg2<HomogeneousMedium>; a "power" light sampler would not do it: with one light the pick is trivial and the
         sampler is uniform): pinhole, thin lens (lensradius 0.05, focused on the back wall), orthographic, both spherical mappings
  cloud  the benchmark's 256^3 cloud: the wavefront pipeline, pinhole and thin lens
and, to split a lens's cost into the ray generator and the less coherent first segment, the fog box at maxdepth 0 -- one segment per
path: the camera ray, its free flight and nothing else -- with the lens focused at 1e6 (the generator's arithmetic, rays within
lensradius of the pinhole's: the same coherence) and focused on the back wall (the same arithmetic, defocused rays).

  python scripts/camera_timing.py [--rounds 5] [--waves 4] [--out profiles/camera_timing.json]

One renderer per configuration; the rounds alternate between the configurations, so drift of the machine lands on all of them
alike.  A round times `waves` one-sample waves between two device synchronisations after the warm-up waves; the figure per
configuration is the median over the rounds, with the minimum and the maximum next to it, and segments per path."""
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
ap.add_argument("--out", default=None)
args = ap.parse_args()

P = g.load_package()
P.load()
W, H = 1920, 1080
TRIANGLE = np.array([[[0.9, -0.99, 0.9], [0.9, -0.99, 0.99], [0.99, -0.99, 0.9]]], np.float32)
FOG_VIEW = ((0, 0, -0.95), (0, 0, 0), (0, 1, 0), 60.0)
#          name: (model, lens_radius, focal_distance, screen window)
CAMERAS = {"pinhole": None, "lens 0.05 @ 1.95": (P.CAMERA_PERSPECTIVE, 0.05, 1.95, None), "lens 0.05 @ 1e6": (P.CAMERA_PERSPECTIVE, 0.05, 1e6, None),
           "orthographic": (P.CAMERA_ORTHOGRAPHIC, 0.0, 1e6, (-0.9, 0.9, -0.50625, 0.50625)), "spherical equal-area": (P.CAMERA_SPHERICAL_EQUALAREA, 0.0, 1e6, None),
           "spherical equirectangular": (P.CAMERA_SPHERICAL_EQUIRECT, 0.0, 1e6, None)}


def make(medium, camera, maxdepth):
    s = P.fog_box_scene(W, H) if medium == "fog" else P.cloud_box_scene(W, H)
    if medium == "fog":
        P.set_triangles(s, TRIANGLE.copy(), np.full((1, 3), 0.5, np.float32))
    prm = P.app_f_params()
    if maxdepth is not None:
        prm.maxdepth = maxdepth
    r = P.Renderer(s, prm, W, H)
    if CAMERAS[camera]:
        model, lr, fd, sw = CAMERAS[camera]
        if medium == "fog":
            cam = P.camera_look_at_window(model, *FOG_VIEW, W, H, screen_window=sw)
        else:   # the cloud scene's own view: its frame and origin, and its raster map under the perspective model
            cam = s.camera
        r.set_camera(cam, model, lr, fd)
    for w in range(args.warmup):
        r.render_wave(w, w + 1)
        r.post_process_wave()
    torch.cuda.synchronize()
    return r, r.kernel_name()


configs = {"fog, %s" % c: ("fog", c, None) for c in CAMERAS}
configs.update({"fog maxdepth 0, %s" % c: ("fog", c, 0) for c in ("pinhole", "lens 0.05 @ 1e6", "lens 0.05 @ 1.95")})
configs.update({"cloud, %s" % c: ("cloud", c, None) for c in ("pinhole", "lens 0.05 @ 1.95")})
renderers = {k: make(*v) for k, v in configs.items()}
times = {k: [] for k in configs}
wave = args.warmup
for rnd in range(args.rounds):
    for k in configs:
        r = renderers[k][0]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for w in range(wave, wave + args.waves):
            r.render_wave(w, w + 1)
        torch.cuda.synchronize()
        times[k].append((time.perf_counter() - t0) / args.waves * 1e3)
    wave += args.waves
result = {"workload": "1920x1080, one sample per wave; fog: the fog box with one corner triangle; cloud: the 256^3 cloud box", "rounds": args.rounds,
          "waves_per_round": args.waves, "ms_per_wave": {}}
for k in configs:
    r, name = renderers[k]
    c = r.counters()
    result["ms_per_wave"][k] = {"median": statistics.median(times[k]), "min": min(times[k]), "max": max(times[k]), "kernel": name,
                                "segments_per_path": c["segments"] / max(1, c["paths"])}
    print("%-40s %-40s median %.3f ms/wave (min %.3f, max %.3f)  seg/path %.2f" % (
        k, name, result["ms_per_wave"][k]["median"], min(times[k]), max(times[k]), result["ms_per_wave"][k]["segments_per_path"]))
    r.close()
med = lambda k: result["ms_per_wave"][k]["median"]
result["ratio_to_pinhole"] = {k: med(k) / med(k.split(",")[0] + ", pinhole") for k in configs if not k.endswith("pinhole")}
# maxdepth 0: pinhole -> lens @ 1e6 is the generator's arithmetic; lens @ 1e6 -> lens @ 1.95 is the defocused first segment
result["fog_maxdepth0_generator_ms"] = med("fog maxdepth 0, lens 0.05 @ 1e6") - med("fog maxdepth 0, pinhole")
result["fog_maxdepth0_coherence_ms"] = med("fog maxdepth 0, lens 0.05 @ 1.95") - med("fog maxdepth 0, lens 0.05 @ 1e6")
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
