"""What getting the image out of the renderer costs: a fog box at 1920x1080 and 3840x2160 with a few waves in the film, three routes
alternated in one process, host clock around calls that each end in a stream synchronise, median of 20 calls after 3 warm-up calls:
  A  film() + the resolve on the host in numpy (sum / weight, the fp16 clamp, astype(float16), the B,G,R scan-line order): what a
     library without vspg_film_resolve leaves to its caller -- 16 bytes per pixel cross to the host;
  B  film_resolve(half=True, layout="scanline"): resolved on the device, 6 bytes per pixel cross, the bytes are the EXR payload;
  C  film_resolve(half=False, layout="scanline"): the same in float32, 12 bytes per pixel.
A's two parts (the film() read, the numpy pass) are timed separately as well.
  python scripts/film_resolve_timing.py            the table
  python scripts/film_resolve_timing.py --child    24 B calls and 24 C calls at 1920x1080: what
                                                   `rocprofv3 --kernel-trace --memory-copy-trace --stats -- python ... --child` watches"""
import os
import statistics
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np  # noqa: E402
import __graft_entry__ as g  # noqa: E402

P = g.load_package()
P.load()
WARM, CALLS = 3, 20


def host_resolve(film):
    rgb, w = film[..., :3], film[..., 3:4]
    with np.errstate(all="ignore"):
        v = np.where(w != 0, rgb / np.where(w != 0, w, np.float32(1)), rgb)
        m = v.max(axis=-1, keepdims=True)
        v = np.where((m > 65504) & (v > 65504), np.float32(65504), v)
        h = v.astype(np.float16)
    return np.ascontiguousarray(h[..., ::-1].transpose(0, 2, 1)), int((m > 65504).sum())


def renderer(w, h):
    r = P.Renderer(P.fog_box_scene(w, h), P.app_f_params(), w, h, spp=64, seed=1)
    for s in range(4):
        r.render_wave(s, s + 1)
        r.post_process_wave()
    r.flush()
    r.film()        # (synchronises: nothing of the render is left to pay for)
    return r


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    if "--child" in sys.argv:
        r = renderer(1920, 1080)
        for _ in range(24):
            r.film_resolve(half=True, layout="scanline")
        for _ in range(24):
            r.film_resolve(half=False, layout="scanline")
        print("child: 24 F16 and 24 F32 scan-line resolves at 1920x1080")
        return
    for w, h in ((1920, 1080), (3840, 2160)):
        r = renderer(w, h)
        routes = {
            "A  film() + numpy resolve, half": lambda: host_resolve(r.film()),
            "A1 film() alone": lambda: r.film(),
            "B  film_resolve F16 scanline": lambda: r.film_resolve(half=True, layout="scanline"),
            "C  film_resolve F32 scanline": lambda: r.film_resolve(half=False, layout="scanline"),
        }
        times = {k: [] for k in routes}
        outs = {}
        for call in range(WARM + CALLS):
            for k, fn in routes.items():      # alternated: every route sees the same machine
                ms, outs[k] = timed(fn)
                if call >= WARM:
                    times[k].append(ms)
        print("%d x %d, kernel %s, %d calls per route after %d warm-up calls, ms per call (host clock, each call ends in a stream synchronise)"
              % (w, h, r.kernel_name(), CALLS, WARM))
        for k, x in times.items():
            print("  %-34s median %9.3f  min %9.3f  max %9.3f" % (k, statistics.median(x), min(x), max(x)))
        a, b, c = (statistics.median(times[k]) for k in list(routes)[:1] + list(routes)[2:])
        a1 = statistics.median(times["A1 film() alone"])
        npix = w * h
        print("  bytes to the host: A %.1f MB, B %.1f MB, C %.1f MB;  A / B %.2f, A1 / B %.2f, C / B %.2f"
              % (npix * 16 / 1e6, npix * 6 / 1e6, npix * 12 / 1e6, a / b, a1 / b, c / b))
        same = np.array_equal(outs["A  film() + numpy resolve, half"][0].view(np.uint16), outs["B  film_resolve F16 scanline"][0].view(np.uint16))
        print("  A's and B's images equal bit for bit: %s; clamped pixels A %d, B %d" % (same, outs["A  film() + numpy resolve, half"][1], outs["B  film_resolve F16 scanline"][1]))
        r.close()


if __name__ == "__main__":
    main()
