"""What the next frame of a COLOURED volume sequence costs: vspg_renderer_update_rgb_grids on a live "rgbgrid" renderer against the
only route there was before it, vspg_renderer_destroy followed by vspg_renderer_create (whose storage is built on the host).
  * the App.-F cloud box at 1920 x 1080 with both sigma grids (sigma_a = d * (0.6, 0.2, 0.05), sigma_s = d * (0.8, 1.6, 3.2) of the
    procedural cloud density d), 64^3 and 256^3 voxels; two such media alternate, so every call changes every voxel;
  * (a) destroy + create, (b) the update from host arrays, (c) the update from torch tensors on the device: wall clock around calls
    that end in a synchronise, median of the repetitions after a warm-up call of each route; the updated renderer's majorants and
    octets are compared with the re-created one's once per size (faster and different is not faster);
  * (d) k_rgb_octet_build alone next to (e) the per-lane fill variant and a hipMemsetAsync over the same image in the same process
    (scripts/microbench/rgb_octet_fill.hip, device events): the memset is the write-only streaming rate of that machine on that day.
Every GPU step is a child process under its own time limit; a step that fails ends the run.  A record, not a test.
  python scripts/rgbgrid_update_timing.py [--reps 9] [--out profiles/rgbgrid_update_timing.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(R, "vspg-pbrt-v4_amd", "csrc")
FILL_SRC = os.path.join(R, "scripts", "microbench", "rgb_octet_fill.hip")
FILL_EXE = os.path.join(R, "scripts", "microbench", "rgb_octet_fill")
W, H = 1920, 1080
SIZES = (64, 256)
LIMIT = {64: 240, 256: 900}   # seconds per renderer step: create alone builds 2 x 2.35 GB on the host at 256^3


def child(n, reps):
    """One size in one process: prints one JSON line."""
    sys.path.insert(0, R)
    import numpy as np
    import torch  # (first: torch's HIP runtime opens the device only if it does so before the library's)
    if not torch.cuda.is_available():
        raise SystemExit("rgbgrid_update_timing.py needs the GPU: a timing without one says nothing")
    import __graft_entry__ as g
    P = g.load_package()
    P.load()

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    def u32(a):
        return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)

    ca, cs = np.array([0.6, 0.2, 0.05], np.float32), np.array([0.8, 1.6, 3.2], np.float32)
    grids, scenes = [], []
    for seed in (5, 6):
        d = P.procedural_cloud_density(n, seed).reshape(n, n, n)
        a, s = np.ascontiguousarray(d[..., None] * ca), np.ascontiguousarray(d[..., None] * cs)
        grids.append((a.reshape(-1), s.reshape(-1)))
        scenes.append(P.set_rgb_grid_medium(P.fog_box_scene(W, H), a, s, None, p0=(-0.9, -0.9, -0.6), p1=(0.9, 0.8, 0.9), g=0.877, scale=8.0))
    dev = [tuple(torch.from_numpy(v).cuda() for v in pair) for pair in grids]
    prm = P.app_f_params()
    r = [P.Renderer(scenes[0], prm, W, H, seed=1)]
    r[0].update_rgb(*grids[1])
    fresh = P.Renderer(scenes[1], prm, W, H, seed=1)
    mu, mf = r[0].majorant(), fresh.majorant()
    same = bool(np.all((mu == mf) & ((u32(mu) == u32(mf)) | (mf == 0))))
    for which in (0, 1):
        same = same and np.array_equal(u32(r[0].rgb_octets(which)), u32(fresh.rgb_octets(which)))
    fresh.close()
    t = {"destroy_create": [], "update_host": [], "update_device": []}
    for rep in range(reps + 1):   # (repetition 0 warms every route up)
        k = rep % 2
        ms_h = timed(lambda: r[0].update_rgb(*grids[k]))
        ms_d = timed(lambda: r[0].update_rgb(*dev[1 - k]))

        def recreate():
            r[0].close()
            r[0] = P.Renderer(scenes[k], prm, W, H, seed=1)
        ms_c = timed(recreate)
        if rep:
            t["update_host"].append(ms_h)
            t["update_device"].append(ms_d)
            t["destroy_create"].append(ms_c)
    r[0].close()
    out = {"n": n, "film": [W, H], "reps": reps, "device": torch.cuda.get_device_name(0), "updated_equals_recreated": same,
           "source_bytes_per_grid": 12 * n ** 3, "octet_bytes_per_grid": ((n + 8) // 8) ** 3 * 512 * 128}
    for name, x in t.items():
        out[name + "_ms"] = {"median": round(statistics.median(x), 3), "min": round(min(x), 3), "max": round(max(x), 3)}
    print(json.dumps(out), flush=True)
    if not same:
        raise SystemExit("the updated renderer differed from the re-created one")


def step(cmd, limit):
    """A GPU step under its own time limit; its last output line is JSON."""
    print("+ %s" % " ".join(cmd), flush=True)
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    sys.stdout.write(p.stdout)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        raise SystemExit("step ended with status %d: nothing more is started" % p.returncode)
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps)
        return
    if not os.path.exists(FILL_EXE) or os.path.getmtime(FILL_EXE) < os.path.getmtime(FILL_SRC):
        flags = subprocess.check_output(["make", "-s", "--no-print-directory", "-C", CSRC, "print-HIPFLAGS"], text=True).split()
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["-I", CSRC, "-o", FILL_EXE, FILL_SRC])
    record = {"what": "rgbgrid update timing: wall clock around calls that end in a synchronise (renderer), device events (fill); medians", "sizes": []}
    for n in SIZES:
        row = step([sys.executable, os.path.abspath(__file__), "--child", str(n), "--reps", str(a.reps)], LIMIT[n])
        row["fill"] = step([FILL_EXE, str(n), str(a.reps)], 120)
        c = row["destroy_create_ms"]["median"]
        row["ratios"] = {"destroy_create_over_update_host": round(c / row["update_host_ms"]["median"], 2),
                         "destroy_create_over_update_device": round(c / row["update_device_ms"]["median"], 2),
                         "staged_over_memset": round(row["fill"]["staged_ms"] / row["fill"]["memset_ms"], 3),
                         "per_lane_over_staged": round(row["fill"]["per_lane_ms"] / row["fill"]["staged_ms"], 3)}
        record["sizes"].append(row)
    print(json.dumps(record, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
