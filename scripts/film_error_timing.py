"""What the film error per wave costs: 1920x1080 fog box, 64 one-sample waves after warm-up, ms per wave between two device events
recorded on the renderer's stream, three variants alternated in one process:
  A  render_wave + post_process_wave, a flush behind the last wave (what a render without error records runs);
  B  A + film_error_enqueue after every wave, one film_errors() behind the loop (vspg_film_error_enqueue: reduced on the device);
  C  A + film() after every wave + the same six sums in numpy (the only route a library without the entry points offers).
  python scripts/film_error_timing.py            the three variants, median / min / max of five repetitions after a warm-up one
  python scripts/film_error_timing.py --child    variant B once: what `rocprofv3 --kernel-trace --stats -- python ... --child` watches
The events belong to the HIP runtime the library itself runs on (libamdhip64 of the ROCm installation), not to torch's."""
import ctypes as C
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np  # noqa: E402
import __graft_entry__ as g  # noqa: E402

P = g.load_package()
P.load()
hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
W, H, WAVES = 1920, 1080, 64


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


def numpy_sums(film, ref64, den2):
    rgb, w = film[..., :3], film[..., 3:4]
    with np.errstate(all="ignore"):
        v = np.where(w != 0, rgb / w, rgb).astype(np.float64)
        se = (v - ref64) ** 2
        rse = se / den2
        se[np.isinf(se)] = 0
        rse[np.isinf(rse)] = 0
    return se.sum(axis=(0, 1)), rse.sum(axis=(0, 1))


class Variant:
    def __init__(self, name, ref):
        self.name = name
        self.r = P.Renderer(P.fog_box_scene(W, H), P.app_f_params(), W, H, spp=1 << 20, seed=1)
        self.w = 0
        self.ref64 = ref.astype(np.float64)
        self.den2 = (self.ref64 + 0.01) ** 2
        if name == "B":
            self.r.set_reference_image(ref)
        self.last = None

    def run(self, n):
        r = self.r
        for _ in range(n):
            r.render_wave(self.w, self.w + 1)
            r.post_process_wave()
            self.w += 1
            if self.name == "B":
                r.film_error_enqueue(tag=self.w)
            elif self.name == "C":
                self.last = numpy_sums(r.film(), self.ref64, self.den2)
        if self.name == "B":
            self.last = r.film_errors()[-1]
        else:
            r.flush()


def main():
    ref_r = P.Renderer(P.fog_box_scene(W, H), P.app_f_params(), W, H, spp=64, seed=99)
    ref_r.render_wave(0, 64)
    f = ref_r.film()
    ref = (f[..., :3] / f[..., 3:4]).astype(np.float32)
    ref_r.close()
    if "--child" in sys.argv:
        v = Variant("B", ref)
        v.run(8)
        v.run(WAVES)
        print("child: B, %d waves, last record %r" % (WAVES, v.last))
        return
    t = Timer()
    vs = [Variant(n, ref) for n in "ABC"]
    print("kernel %s, %d x %d, %d one-sample waves per repetition" % (vs[0].r.kernel_name(), W, H, WAVES))
    times = {v.name: [] for v in vs}
    for rep in range(6):
        for v in vs:
            t.start()
            v.run(WAVES)
            ms = t.stop() / WAVES
            if rep:
                times[v.name].append(ms)
    for v in vs:
        x = times[v.name]
        print("%s  %9.4f ms per wave (min %.4f max %.4f, %d repetitions)" % (v.name, statistics.median(x), min(x), max(x), len(x)))
    a, b, c = (statistics.median(times[k]) for k in "ABC")
    print("B - A %+.4f ms per wave, C - A %+.4f ms per wave, C / B %.1f" % (b - a, c - a, c / b))
    rec = vs[1].last
    print("B's last record: spp %d mse %.9g mrse %.9g" % (rec.tag, rec.mse(), rec.mrse()))
    se, rse = vs[2].last
    print("C's last sums:   se %r rse %r" % (se.tolist(), rse.tolist()))


if __name__ == "__main__":
    main()
