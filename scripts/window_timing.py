"""What a pixel window costs: ms per vspg_render_window call at 1920x1080, fog box and 256^3 cloud, one sample index per call and
64 per call, windows of 1/4, 1/16 and 1/256 of the frame at an interior, unaligned origin (and the 1/4 window again at the frame's corner),
next to the full frame.
  python scripts/window_timing.py [fog|cloud ...] [--full-only]     (VSPG_LIB selects another build of the library: with
  --full-only the full-frame lines alone, which is all a library without vspg_render_window can run)
Hot-loop timing between device synchronisations, median of five repetitions after a warm-up repetition; a one-sample call leaves
its samples parked, so successive calls of the same window resolve them in the kernel as a frame's waves do."""
import os
import statistics
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import torch  # noqa: E402  (before the library: tests/conftest.py, gpu_pkg)

torch.cuda.is_available()
import __graft_entry__ as g  # noqa: E402

P = g.load_package()
P.load()
W, H = 1920, 1080
X0, Y0 = 403, 211
# ("1/4c": the same quarter cut from the frame's top-left corner, away from the middle of the picture -- what content costs)
WINDOWS = [("full", (0, 0, W, H)), ("1/4", (X0, Y0, X0 + 960, Y0 + 540)), ("1/4c", (3, 5, 3 + 960, 5 + 540)), ("1/16", (X0, Y0, X0 + 480, Y0 + 270)),
           ("1/256", (X0, Y0, X0 + 120, Y0 + 68))]


def measure(r, win, n_samples, calls, full_only):
    w = [0]

    def call():
        if full_only:
            r.render_wave(w[0], w[0] + n_samples)
        else:
            r.render_window(*win, w[0], w[0] + n_samples)
        w[0] += n_samples
    times = []
    for rep in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        r.flush()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / calls * 1e3)
    return statistics.median(times[1:]), min(times[1:]), max(times[1:])


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    full_only = "--full-only" in sys.argv
    print("library %s%s" % (os.environ.get("VSPG_LIB", "(this tree's)"), "  [full frame only]" if full_only else ""))
    for workload in args or ["fog", "cloud"]:
        scene = P.fog_box_scene(W, H) if workload == "fog" else P.cloud_box_scene(W, H, 256)
        for n_samples in (1, 64):
            full_ms = None
            for name, win in WINDOWS[:1] if full_only else WINDOWS:
                r = P.Renderer(scene, P.app_f_params(), W, H)
                calls = (32 if n_samples == 1 else 2) if workload == "fog" else (8 if n_samples == 1 else 1)
                if name != "full":
                    calls *= 4
                med, lo, hi = measure(r, win, n_samples, calls, full_only)
                kn = r.kernel_name()
                r.close()
                frac = (win[2] - win[0]) * (win[3] - win[1]) / float(W * H)
                if name == "full":
                    full_ms = med
                print("%-5s %2d sample(s)/call  window %-5s %4dx%-4d  %9.4f ms/call (min %.4f max %.4f)  area x this library's full = %9.4f ms  ratio %.2f  %s"
                      % (workload, n_samples, name, win[2] - win[0], win[3] - win[1], med, lo, hi, frac * full_ms, med / (frac * full_ms), kn), flush=True)


if __name__ == "__main__":
    main()
