"""Diagnostic: what an image texture on the diffuse reflectance costs per 1920 x 1080 wave.  A box whose six walls all carry one
bilinear, repeating texture (uscale = vscale = 4) is timed against its constant twin -- the same box with the image's mean colour
as every wall's Kd -- on the same kernel:
  fog    the App.-F fog box with one small triangle (so that the twin is not `simple` either): k_render_wave_wg2<HomogeneousMedium>
  cloud  the benchmark's 256^3 cloud inside the same walls: the wavefront pipeline
for a 64 x 64 and a 4096 x 4096 image (16 KB and 256 MB of float4 texels: one that lives in cache, one that does not).

  python scripts/texture_timing.py [--rounds 5] [--waves 4] [--out profiles/texture_timing.json]

One renderer per configuration; the rounds alternate between the configurations, so drift of the machine lands on all of them
alike.  A round times `waves` one-sample waves between two device synchronisations after the warm-up waves; the figure per
configuration is the median over the rounds, with the minimum and the maximum next to it, and segments and surface hits per path."""
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


def image(res):
    return np.ascontiguousarray(np.random.default_rng(res).uniform(0.05, 0.95, (res, res, 3)).astype(np.float32))


def scene(medium, res):
    """res = 0: the constant twin (Kd = the mean of the 64 x 64 image)."""
    s = P.fog_box_scene(W, H) if medium == "fog" else P.cloud_box_scene(W, H)
    P.set_triangles(s, TRIANGLE.copy(), np.full((1, 3), 0.5, np.float32))
    if res:
        k = P.add_texture(s, image(res), filter="bilinear", wrap="repeat", uscale=4.0, vscale=4.0)
        for i in range(6):
            P.scene_textures(s).quad_texture[i] = k
    else:
        mean = image(64).reshape(-1, 3).mean(axis=0)
        for i in range(6):
            s.quads[i].Kd[:] = [float(v) for v in mean]
    return s


def make(medium, res):
    r = P.Renderer(scene(medium, res), P.app_f_params(), W, H)
    for w in range(args.warmup):
        r.render_wave(w, w + 1)
        r.post_process_wave()
    torch.cuda.synchronize()
    return r, r.kernel_name()


configs = {"%s, %s" % (m, "constant Kd" if not res else "%d^2 texture" % res): (m, res) for m in ("fog", "cloud") for res in (0, 64, 4096)}
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
result = {"workload": "six textured walls 1920x1080, bilinear, repeat, uscale = vscale = 4, texel layout: one float4 per texel", "rounds": args.rounds,
          "waves_per_round": args.waves, "ms_per_wave": {}}
for k in configs:
    r, name = renderers[k]
    c = r.counters()
    result["ms_per_wave"][k] = {"median": statistics.median(times[k]), "min": min(times[k]), "max": max(times[k]), "kernel": name,
                                "segments_per_path": c["segments"] / max(1, c["paths"]), "surface_hits_per_path": c["surface_hits"] / max(1, c["paths"])}
    print("%-26s %-40s median %.3f ms/wave (min %.3f, max %.3f)  seg/path %.2f  surface hits/path %.2f" % (
        k, name, result["ms_per_wave"][k]["median"], min(times[k]), max(times[k]), result["ms_per_wave"][k]["segments_per_path"],
        result["ms_per_wave"][k]["surface_hits_per_path"]))
    r.close()
for m in ("fog", "cloud"):
    base = result["ms_per_wave"]["%s, constant Kd" % m]["median"]
    result["%s_ratio_to_constant" % m] = {str(res): result["ms_per_wave"]["%s, %d^2 texture" % (m, res)]["median"] / base for res in (64, 4096)}
print(json.dumps(result))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
