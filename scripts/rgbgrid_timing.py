#!/usr/bin/env python3
"""ms per 1080p wave of the 256^3 cloud box rendered as an RGB grid medium ("rgbgrid") and as its uniformgrid twin.

The cloud workload's density field d with power-of-two coefficients: the uniformgrid has grey sigma_a = A, sigma_s = S; the rgbgrid
holds the voxels A d_i and S d_i in all three channels -- the same medium bit for bit (tests/test_rgbgrid_gpu.py), so both renderers
walk the same paths; what differs is the fetch -- two 128-byte lines of RGB octets per query against one 32-byte octet -- and the
per-channel arithmetic behind it.  The timer is the host's around whole waves: no per-kernel split is taken.  The
uniformgrid figure is the baseline (the parent's kernel).  Same process, alternating rounds; min, median and max of each are reported.

    python3 scripts/rgbgrid_timing.py [--rounds N] [--waves N] [--grid N] [--out FILE]
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, S = 0.125, 8.0   # sigma_t 8.125, albedo 0.985: the cloud workload's regime, in powers of two


def load_package():
    spec = importlib.util.spec_from_file_location("vspg_pbrt_v4_amd", os.path.join(ROOT, "vspg-pbrt-v4_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["vspg_pbrt_v4_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--waves", type=int, default=8)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgbgrid_timing.json"))
    args = ap.parse_args()
    P = load_package()
    W, H, n = 1920, 1080, args.grid
    uni = P.cloud_box_scene(W, H, n)
    uni.medium.sigma_a[:] = (A,) * 3
    uni.medium.sigma_s[:] = (S,) * 3
    d = uni._density_keepalive.reshape(n, n, n)
    rgb = P.cloud_box_scene(W, H, n)
    m = rgb.medium
    rep = lambda v: np.repeat(v[..., None], 3, axis=-1).astype(np.float32)
    P.set_rgb_grid_medium(rgb, rep(np.float32(A) * d), rep(np.float32(S) * d), None, p0=list(m.bounds_min), p1=list(m.bounds_max), g=m.g, scale=1.0)
    prm = P.app_f_params()
    rs = {"uniformgrid": P.Renderer(uni, prm, W, H), "rgbgrid": P.Renderer(rgb, prm, W, H)}
    names = {k: r.kernel_name() for k, r in rs.items()}
    ms = {k: [] for k in rs}
    wave = 0
    for k, r in rs.items():   # warm-up: allocations, first launches
        r.render_wave(0, 1); r.post_process_wave(); r.counters()
    for _ in range(args.rounds):
        for k, r in rs.items():
            t0 = time.perf_counter()
            for w in range(wave, wave + args.waves):
                r.render_wave(w + 1, w + 2); r.post_process_wave()
            r.counters()   # synchronises
            ms[k].append((time.perf_counter() - t0) * 1e3 / args.waves)
        wave += args.waves
    same = np.array_equal(rs["uniformgrid"].film().view(np.uint32), rs["rgbgrid"].film().view(np.uint32))
    for r in rs.values():
        r.close()
    stat = lambda v: {"min": min(v), "median": float(np.median(v)), "max": max(v), "rounds": v}
    out = {"resolution": [W, H], "grid": n, "waves_per_round": args.waves, "sigma_a": A, "sigma_s": S, "kernels": names, "films_equal_bit_for_bit": bool(same),
           "ms_per_wave": {k: stat(v) for k, v in ms.items()},
           "ratio_of_medians": float(np.median(ms["rgbgrid"]) / np.median(ms["uniformgrid"])),
           "lines_per_query": {"rgbgrid": 2, "uniformgrid": "one 32-byte octet of one line"}, "bytes_per_voxel_and_grid": 128,
           "timer": "host clock around waves_per_round waves and a synchronising read of the counters"}
    print(json.dumps(out, indent=1))
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
