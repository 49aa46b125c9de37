"""What the next frame of a volume sequence costs: vspg_renderer_update_grid on a live renderer against the only route there was
before it, vspg_renderer_destroy followed by vspg_renderer_create on the same scene.
  * grids of 64^3 and 256^3 samples, GridMedium ("GRID": 16^3 majorant cells) and NanoVDB semantics ("NANOVDB": 64^3 cells), the
    procedural cloud in the App.-F box at 1920x1080 (the per-pixel buffers are part of what a re-creation pays for);
  * the update from a host array (staged on the device, as create stages it) and from a torch tensor on the device (read in place);
  * two densities alternate, so every call changes every voxel.
Both routes end in a synchronise of the device (the update synchronises its stream, create the device), so a host clock around the
call measures the work: median / min / max of the repetitions after a warm-up call of each route.  The majorants and the bricks of
the updated renderer are compared with the re-created one's once per configuration (faster and different is not faster).
A record, not a test.
  python scripts/medium_update_timing.py [--reps 9] [--out profiles/medium_update_timing.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import torch  # noqa: E402  (first: torch's HIP runtime opens the device only if it does so before the library's)

if not torch.cuda.is_available():
    raise SystemExit("medium_update_timing.py needs the GPU: a timing without one says nothing")
import __graft_entry__ as g  # noqa: E402

P = g.load_package()
P.load()
W, H = 1920, 1080


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t) * 1e3


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run(kind, n, reps, emit):
    scenes = [(P.cloud_box_scene if kind == "GRID" else P.nanovdb_box_scene)(W, H, n=n, seed=s) for s in (5, 6)]
    dens = [s._density_keepalive for s in scenes]
    dev = [torch.from_numpy(d).cuda() for d in dens]
    prm = P.app_f_params()
    r = P.Renderer(scenes[0], prm, W, H, seed=1)
    # once: the updated renderer holds what a re-created one holds
    r.update_density(dens[1])
    fresh = P.Renderer(scenes[1], prm, W, H, seed=1)
    same = (np.array_equal(r.majorant(), fresh.majorant()) and r.brick_info() == fresh.brick_info()
            and all(np.array_equal(u32(a), u32(b)) for a, b in zip(r.brick_storage(), fresh.brick_storage())))
    info = fresh.brick_info()
    fresh.close()
    r.update_density(dev[0])
    t = {"update, host source": [], "update, device source": [], "destroy + create": []}
    for rep in range(reps + 1):   # (repetition 0 warms every route up)
        k = (rep + 1) % 2
        _, ms = timed(lambda: r.update_density(dens[k]))
        _, ms2 = timed(lambda: r.update_density(dev[1 - k]))

        def recreate():
            nonlocal r
            r.close()
            r = P.Renderer(scenes[k], prm, W, H, seed=1)
        _, ms3 = timed(recreate)
        if rep:
            t["update, host source"].append(ms)
            t["update, device source"].append(ms2)
            t["destroy + create"].append(ms3)
    r.close()
    emit("== %s %d^3 (%.1f MB of samples; %s bricks: %d of %d stored, %.1f MB of octets), film %d x %d; updated == re-created: %s =="
         % (kind, n, 4 * n ** 3 / 1e6, "indexed" if info["indexed"] else "dense", info["n_stored"], info["bnx"] * info["bny"] * info["bnz"],
            info["octet_bytes"] / 1e6, W, H, "yes" if same else "NO"))
    base = statistics.median(t["destroy + create"])
    for name, x in t.items():
        emit("  %-22s %9.3f ms  (min %.3f, max %.3f, %d repetitions)  %5.1fx" % (name, statistics.median(x), min(x), max(x), len(x), base / statistics.median(x)))
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("medium update timing: %s, wall clock around calls that end in a synchronise, median of %d repetitions after a warm-up;" % (torch.cuda.get_device_name(0), a.reps))
    emit("last column: destroy + create over this route")
    ok = True
    for kind in ("GRID", "NANOVDB"):
        for n in (64, 256):
            ok = run(kind, n, a.reps, emit) and ok
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if not ok:
        raise SystemExit("an updated renderer differed from the re-created one")


if __name__ == "__main__":
    main()
