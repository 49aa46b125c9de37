"""Film error against a reference image (include/vspg.h, VspgFilmError): what can be checked without a device -- the three entry
points are declared, exported and bound; the record's layout is the C layout; NULL arguments are refused; and the host side of the
arithmetic: combine_film_errors adds sums and pixel counts, mse() / mrse() perform the reference's last step
(src/pbrt/util/image.cpp:603-606: per channel Float(sum / (Float(w) * Float(h))); util/image.h:205-210: Average() in Float)."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

NAMES = ["vspg_renderer_set_reference_image", "vspg_film_error_enqueue", "vspg_film_error_read"]
f32 = np.float32


def _sharding():
    spec = importlib.util.spec_from_file_location("vspg_sharding", os.path.join(ROOT, "vspg-pbrt-v4_amd", "sharding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_header_library_and_binding_carry_the_entry_points(pkg):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vspg.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(vspg_[a-z0-9_]+)\s*\(", src))
    lib = pkg.load()
    bound = {n for n, _, _ in pkg.SYMBOLS}
    for n in NAMES:
        assert n in declared, n
        assert hasattr(lib, n), n
        assert n in bound, n
    assert lib.vspg_abi_version() == 7


def test_record_layout_is_the_c_layout(pkg, tmp_path):
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vspg.h"\n'
                    'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(VspgFilmError), offsetof(VspgFilmError, tag),\n'
                    '  offsetof(VspgFilmError, tick_khz), offsetof(VspgFilmError, n_pixels), offsetof(VspgFilmError, device_ticks),\n'
                    '  offsetof(VspgFilmError, sum_se), offsetof(VspgFilmError, sum_rse), VSPG_FILM_ERROR_LOG_RECORDS); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)])
    size, o_tag, o_khz, o_n, o_ticks, o_se, o_rse, log = map(int, subprocess.check_output([str(exe)]).split())
    T = pkg.VspgFilmError
    assert size == 88 == C.sizeof(T)
    assert (o_tag, o_khz, o_n, o_ticks, o_se, o_rse) == (T.tag.offset, T.tick_khz.offset, T.n_pixels.offset, T.device_ticks.offset,
                                                         T.sum_se.offset, T.sum_rse.offset)
    assert log == pkg.FILM_ERROR_LOG_RECORDS == 4096


def test_null_arguments_are_refused(pkg):
    lib = pkg.load()
    img = (C.c_float * 3)()
    assert lib.vspg_renderer_set_reference_image(None, img, None) == pkg.VSPG_EINVAL
    assert lib.vspg_renderer_set_reference_image(None, None, None) == pkg.VSPG_EINVAL
    assert lib.vspg_film_error_enqueue(None, 0, 0, 1, 1, 0, None) == pkg.VSPG_EINVAL
    rec = (pkg.VspgFilmError * 1)()
    n = C.c_size_t(7)
    assert lib.vspg_film_error_read(None, rec, 1, C.byref(n), None) == pkg.VSPG_EINVAL
    assert lib.vspg_film_error_read(None, None, 0, None, None) == pkg.VSPG_EINVAL
    assert lib.vspg_last_error()


def _rec(pkg, win, se, rse, tag=0, ticks=0):
    x0, y0, x1, y1 = win
    return pkg.FilmError(x0, y0, x1, y1, tag, 100000, (x1 - x0) * (y1 - y0), ticks, se, rse)


def test_combine_adds_sums_and_pixel_counts(pkg):
    sh = _sharding()
    a = _rec(pkg, (0, 0, 100, 24), [1.5, 2.25, 1e-3], [10.0, 20.0, 30.0], tag=4, ticks=50)
    b = _rec(pkg, (0, 24, 100, 48), [0.5, 1e-17, 2.0], [1.0, 2.0, 3.0], tag=4, ticks=70)
    c = _rec(pkg, (0, 48, 100, 76), [3.0, 4.0, 5.0], [0.125, 0.25, 0.5], tag=4, ticks=60)
    u = sh.combine_film_errors([a, b, c])
    for k in range(3):
        assert u.sum_se[k] == (a.sum_se[k] + b.sum_se[k]) + c.sum_se[k]      # added in the order given, in double
        assert u.sum_rse[k] == (a.sum_rse[k] + b.sum_rse[k]) + c.sum_rse[k]
    assert u.n_pixels == 100 * 76 and u.window() == (0, 0, 100, 76)
    assert u.tag == 4 and u.device_ticks == 70
    assert a.n_pixels == 2400 and a.sum_se == [1.5, 2.25, 1e-3]             # the inputs are left alone
    # a NaN poisons its channel only
    d = _rec(pkg, (0, 76, 100, 80), [float("nan"), 1.0, 1.0], [1.0, 1.0, 1.0])
    v = sh.combine_film_errors([u, d])
    assert np.isnan(v.sum_se[0]) and v.sum_se[1] == u.sum_se[1] + 1.0 and v.n_pixels == 8000
    assert sh.combine_film_errors([a]).sum_se == a.sum_se


def test_mse_and_mrse_reproduce_the_float_steps(pkg):
    # sums chosen so that every rounding matters: the per-channel quotient is rounded to Float before the average, and the
    # average itself adds and divides in Float
    se = [1234.56789012345, 0.000123456789012345, 98765.4321098765]
    rse = [3.3333333333333335, 7.777777777777778e5, 1.1111111111111112e-7]
    r = _rec(pkg, (13, 5, 77, 50), se, rse)

    def expect(sums, div):
        ch = [f32(np.float64(s) / np.float64(div)) for s in sums]       # image.cpp:605: double / Float -> Float
        acc = f32(0)
        for v in ch:                                                     # image.h:205-210
            acc = f32(acc + v)
        return float(f32(acc / f32(3)))
    div = f32(77 - 13) * f32(50 - 5)                                     # Float(Resolution().x) * Float(Resolution().y)
    assert r.mse() == expect(se, div) and r.mrse() == expect(rse, div)
    # ... and differ from the same steps taken in double (the check can tell the two apart)
    assert r.mse() != sum(s / float(div) for s in se) / 3
    # a union of windows is no rectangle: the divisor is Float(n_pixels)
    sh = _sharding()
    u = sh.combine_film_errors([_rec(pkg, (0, 0, 10, 8), se, rse), _rec(pkg, (20, 8, 30, 16), se, rse)])
    assert u.n_pixels == 160 and u.mse() == expect([2 * s for s in se], f32(160))
    # a frame whose pixel count is no Float: the product of the two Floats is what the reference divides by
    big = _rec(pkg, (0, 0, 4099, 4097), se, rse)
    assert big.mse() == expect(se, f32(4099) * f32(4097))
