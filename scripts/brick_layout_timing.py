"""What the two layouts of a grid medium's density cost (csrc/vspg_capi.hip, vspg_renderer_create: every brick in grid order while
they fit 8 GiB, else only the non-empty ones behind an index; VSPG_DENSE_BRICKS=0|1 forces either):
  * the `cloud` workload (256^3 procedural cloud in the box, App.-F options) at 1920x1080 with the index forced and with the
    dense layout: renderer creation (upload, k_brick_flags, slot numbering on the host, k_brick_fill), bytes held
    (vspg_brick_info), ms per one-sample wave;
  * the production-sized sparse grid of tests/test_brick_storage_gpu.py (1160 x 520 x 456, 558 888 bricks: indexed by itself) at
    1920x1080: the same three figures.
Waves are timed between two device events of the HIP runtime the library runs on, after a warm-up repetition; the renderers of a
workload are alternated in one process; median / min / max of the repetitions.  A record, not a test.
  python scripts/brick_layout_timing.py [--waves 16] [--reps 7]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import __graft_entry__ as g  # noqa: E402

P = g.load_package()
P.load()
import brick_model as bm  # noqa: E402  (the sparse density generator only)
import scenes  # noqa: E402

hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
W, H = 1920, 1080


def chk(rc):
    if rc != 0:
        raise RuntimeError("HIP error %d" % rc)


class Timer:
    def __init__(self):
        self.a, self.b = C.c_void_p(), C.c_void_p()
        chk(hip.hipEventCreate(C.byref(self.a)))
        chk(hip.hipEventCreate(C.byref(self.b)))

    def start(self):
        chk(hip.hipDeviceSynchronize())
        chk(hip.hipEventRecord(self.a, None))

    def stop(self):
        chk(hip.hipEventRecord(self.b, None))
        chk(hip.hipEventSynchronize(self.b))
        ms = C.c_float()
        chk(hip.hipEventElapsedTime(C.byref(ms), self.a, self.b))
        return ms.value


def create(scene, layout):
    """(renderer, seconds to create it) under VSPG_DENSE_BRICKS = 0 ("indexed") / 1 ("dense") / unset (None)."""
    old = os.environ.pop("VSPG_DENSE_BRICKS", None)
    if layout is not None:
        os.environ["VSPG_DENSE_BRICKS"] = "0" if layout == "indexed" else "1"
    try:
        chk(hip.hipDeviceSynchronize())
        t = time.perf_counter()
        r = P.Renderer(scene, P.app_f_params(), W, H, spp=1 << 20, seed=1)
        chk(hip.hipDeviceSynchronize())
        return r, time.perf_counter() - t
    finally:
        os.environ.pop("VSPG_DENSE_BRICKS", None)
        if old is not None:
            os.environ["VSPG_DENSE_BRICKS"] = old


def run(name, scene, layouts, waves, reps):
    timer = Timer()
    rs = []
    for layout in layouts:
        create(scene, layout)[0].close()                     # first creation of a process pays for loading the code objects
        secs = []
        for _ in range(3):
            r, s = create(scene, layout)
            secs.append(s)
            if len(secs) < 3:
                r.close()
        rs.append((layout, r, secs))
    print("== %s, %d x %d, kernel %s, %d one-sample waves per repetition ==" % (name, W, H, rs[0][1].kernel_name(), waves))
    times = {layout: [] for layout in layouts}
    w = 0
    for rep in range(reps + 1):
        for layout, r, _ in rs:
            timer.start()
            for k in range(waves):
                r.render_wave(w + k, w + k + 1)
                r.post_process_wave()
            ms = timer.stop() / waves
            if rep:
                times[layout].append(ms)
        w += waves
    for layout, r, secs in rs:
        bi = r.brick_info()
        x = times[layout]
        print("  %-8s %s: %d of %d bricks stored, index %.1f MB, octets %.1f MB; create %.3f s (min %.3f max %.3f of %d); "
              "%.4f ms per wave (min %.4f max %.4f, %d repetitions)"
              % (layout or "auto", "indexed" if bi["indexed"] else "dense", bi["n_stored"], bi["bnx"] * bi["bny"] * bi["bnz"], bi["index_bytes"] / 1e6,
                 bi["octet_bytes"] / 1e6, statistics.median(secs), min(secs), max(secs), len(secs), statistics.median(x), min(x), max(x), len(x)))
        r.close()
    if len(layouts) == 2:
        a, b = (statistics.median(times[k]) for k in layouts)
        print("  %s - %s %+.4f ms per wave (%+.2f %%)" % (layouts[0], layouts[1], a - b, 100 * (a - b) / b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--waves", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    run("cloud (256^3 in the box)", P.cloud_box_scene(W, H), ["indexed", "dense"], a.waves, a.reps)
    big = (1160, 520, 456)
    t = time.perf_counter()
    dens = bm.coarse_blob_density(big)
    print("sparse grid %d x %d x %d generated in %.1f s" % (big + (time.perf_counter() - t,)))
    scene = scenes.grid_scene(dens, big, 0.08, 7.9, g=0.877, bmin=(-0.9, -0.8, -0.5), bmax=(0.9, 0.7, 0.9), W=W, H=H)
    run("sparse grid 1160 x 520 x 456", scene, [None], a.waves, a.reps)


if __name__ == "__main__":
    main()
