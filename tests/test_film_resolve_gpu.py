"""vspg_film_resolve: the film resolved to pixel values on the device (include/vspg.h, csrc/vspg_film_resolve.h) against a NumPy model
of RGBFilm::GetPixelRGB + the fp16 clamp of RGBFilm::GetImage + Half(float).  A fog box at 67 x 41 (both dimensions odd: in the
scan-line layout the channel planes of a row then start at odd element offsets); bits and counts only, no tolerance."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exr_model as X  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 67, 41
WINDOWS = [(0, 0, 67, 41),      # the frame
           (13, 5, 60, 40),     # an interior window, odd width, odd x0
           (66, 40, 67, 41),    # the last pixel
           (1, 0, 4, 41),       # a column strip: 3 wide, odd x0
           (0, 7, 67, 8)]       # one row


def fbits(*words):
    return np.array(words, dtype=np.uint32).view(np.float32)


def synthetic_film():
    """(H, W, 4) float32: every value at which the resolve can go wrong, in every channel position, with weight 1 (the division is
    exact), weight 0 (the sums pass through) and weight 4 (a real division, exact too: a power of two), cycled over the whole frame
    so that every window above holds many of them."""
    qnan, nqnan = fbits(0x7fc00000)[0], fbits(0xffc00000)[0]
    f = np.float32
    vals = [f(0.0), f(-0.0),
            f(6e-8), f(2.0 ** -24), f(2.0 ** -25), fbits(0x33000001)[0], f(1.5 * 2.0 ** -24), f(2.5 * 2.0 ** -24), f(1e-6), f(6e-5), f(6.1e-5),
            f(2.0 ** -14), fbits(0x387fffff)[0], f(-6e-8), f(-6e-5),                                      # half subnormals and their edges
            f(1 + 2.0 ** -11), f(1 + 3 * 2.0 ** -11), f(2049.0), f(2051.0), fbits(0x3f801001)[0], f(-2049.0),  # exact ties, both parities; just past one
            f(65504.0), f(65505.0), f(65519.996), f(65520.0), f(1e9), f(np.inf), f(-70000.0), f(-np.inf), f(-65519.996), f(-65520.0),
            qnan, nqnan, f(0.1), f(3.0)]
    pixels = []
    for v in vals:
        for c in range(3):          # the value in each channel position, beside two ordinary ones
            p = [f(1.0), f(0.25), f(100.0)]
            p[c] = v
            pixels.append(p)
    import itertools
    for trio in [(qnan, f(70000.0), f(1.0)), (nqnan, f(1e9), f(70000.0)), (qnan, nqnan, f(70000.0)), (f(65504.0), f(65505.0), f(2.0)),
                 (f(70000.0), f(70000.0), f(70000.0)), (f(np.inf), f(-np.inf), qnan), (f(-70000.0), f(65503.0), f(1.0))]:
        pixels += [list(p) for p in itertools.permutations(trio)]     # both orders around a NaN: (NaN,70000,1) stays, (70000,NaN,1) clamps r
    n = len(pixels)
    assert n % W != 0
    film = np.zeros((H * W, 4), dtype=np.float32)
    idx = np.arange(H * W)
    film[:, :3] = np.array(pixels, dtype=np.float32)[idx % n]
    lap = idx // n                                    # successive laps over the list: weight 1, 0, 4, 1, ...
    film[:, 3] = np.array([1.0, 0.0, 4.0], dtype=np.float32)[lap % 3]
    film[lap % 3 == 2, :3] *= np.float32(4.0)         # (value * 4 / 4: exact unless it overflows, and then the model says what comes out)
    return film.reshape(H, W, 4)


def model(film, win, half, layout):
    """Section by section what include/vspg.h says of vspg_film_resolve.  -> (bits in the layout's shape, n_clamped)"""
    x0, y0, x1, y1 = win
    f = np.ascontiguousarray(film[y0:y1, x0:x1], dtype=np.float32)
    w = f[..., 3:4]
    with np.errstate(all="ignore"):
        v = np.where(w != 0, f[..., :3] / np.where(w != 0, w, np.float32(1)), f[..., :3]).astype(np.float32)   # one float division
    n = 0
    if half:
        r, g, b = v[..., 0], v[..., 1], v[..., 2]
        with np.errstate(invalid="ignore"):
            m = r.copy()
            m = np.where(m < g, g, m)
            m = np.where(m < b, b, m)
            clamp = m > np.float32(65504)
            v = np.where(clamp[..., None] & (v > np.float32(65504)), np.float32(65504), v)
        n = int(clamp.sum())
        bits = X.half_bits(v)
    else:
        bits = v.view(np.uint32)
    if layout == "scanline":
        bits = np.ascontiguousarray(bits[..., ::-1].transpose(0, 2, 1))    # (h, 3, w): B, G, R planes per row
    return bits, n


def as_bits(a):
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def write_film(r, film):
    import torch
    ptr, n = r.film_ptr()
    assert n == film.size

    class Dev:
        __cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (ptr, False), "version": 2}
    t = torch.as_tensor(Dev(), device="cuda:0")
    t.copy_(torch.from_numpy(np.ascontiguousarray(film).view(np.int32).ravel().copy()).view(torch.float32))   # (through int32: no NaN is touched)
    torch.cuda.synchronize()


def renderer(P, seed=3, **kw):
    return P.Renderer(P.fog_box_scene(W, H), P.app_f_params(), W, H, seed=seed, **kw)


@pytest.fixture(scope="module")
def synthetic(gpu_pkg):
    r = renderer(gpu_pkg)
    film = synthetic_film()
    write_film(r, film)
    back = r.film()
    assert np.array_equal(back.view(np.uint32), film.view(np.uint32)), "the film did not take the test's values"
    yield r, film
    r.close()


@pytest.mark.parametrize("layout", ["rgb", "scanline"])
@pytest.mark.parametrize("half", [True, False], ids=["f16", "f32"])
@pytest.mark.parametrize("win", WINDOWS, ids=["%d-%d-%d-%d" % w for w in WINDOWS])
def test_synthetic_film(synthetic, win, half, layout):
    r, film = synthetic
    out, n = r.film_resolve(win, half=half, layout=layout)
    x0, y0, x1, y1 = win
    assert out.shape == ((y1 - y0, x1 - x0, 3) if layout == "rgb" else (y1 - y0, 3, x1 - x0))
    assert out.dtype == (np.float16 if half else np.float32)
    want, n_want = model(film, win, half, layout)
    got = as_bits(out)
    bad = got != want
    print("window %s %s %s: %d values, %d differ; clamped %d, model %d" % (win, "f16" if half else "f32", layout, got.size, int(bad.sum()), n, n_want))
    assert not bad.any(), [(tuple(i), hex(got[tuple(i)]), hex(want[tuple(i)])) for i in np.argwhere(bad)[:8]]
    assert n == n_want
    if half and (x1 - x0) * (y1 - y0) > 200:
        assert n_want > 0 and (want == 0x7e00).any() and (want == 0xfe00).any() and (want == 0xfc00).any() and (want == 0x7bff).any()


def test_rendered_film_is_complete(gpu_pkg):
    """Three one-sample waves of the default kernel leave parked samples and suspended paths; film_resolve comes before any other
    accessor and must show the COMPLETE film."""
    P = gpu_pkg
    assert os.environ.get("VSPG_WG3_CARRY", "1") != "0"
    r = renderer(P, seed=7)
    assert r.kernel_name().startswith("k_render_wave_wg3<"), r.kernel_name()
    for s in range(3):
        r.render_wave(s, s + 1)
    res = r.lib.vspg_debug_carry_resumes
    res.restype, res.argtypes = C.c_longlong, [C.c_void_p]
    assert int(res(r.h)) > 0, "no launch resumed carried paths: the test would show nothing"
    first = {(h, l): r.film_resolve(half=h, layout=l) for h, l in [(True, "scanline")]}     # before any other accessor
    film = r.film()
    assert r.counters()["paths"] == W * H * 3 and (film[..., 3] == 3).all()
    r.flush()
    for half in (True, False):
        for layout in ("rgb", "scanline"):
            out, n = r.film_resolve(half=half, layout=layout)
            want, n_want = model(film, (0, 0, W, H), half, layout)
            assert np.array_equal(as_bits(out), want) and n == n_want == 0
            if (half, layout) in first:
                assert np.array_equal(as_bits(first[(half, layout)][0]), want) and first[(half, layout)][1] == 0
    # and over a window of a film that only a window was rendered into: the w == 0 branch beside rendered pixels
    r.film_clear()
    r.render_window(13, 5, 60, 40, 0, 1)
    out, n = r.film_resolve((10, 3, 64, 41), half=True, layout="scanline")
    film = r.film()
    want, _ = model(film, (10, 3, 64, 41), True, "scanline")
    assert np.array_equal(as_bits(out), want) and (film[..., 3] == 0).any() and (film[..., 3] == 1).any()
    r.close()


def test_argument_errors_leave_the_buffer_untouched(gpu_pkg):
    P = gpu_pkg
    r = renderer(P)
    r.render_wave(0, 1)
    lib = r.lib
    buf = np.full(W * H * 3 + 8, 0x5a5a, dtype=np.uint16)
    n = C.c_uint64(77)

    def call(x0, y0, x1, y1, fmt, layout, nbytes):
        return lib.vspg_film_resolve(r.h, x0, y0, x1, y1, fmt, layout, buf.ctypes.data_as(C.c_void_p), nbytes, C.byref(n), None)
    full = W * H * 3 * 2
    cases = [(0, 0, W, H, 1, 0, full - 2), (0, 0, W, H, 1, 0, full + 2), (0, 0, W, H, 1, 0, full * 2), (0, 0, W, H, 0, 0, full), (0, 0, W, H, 1, 0, 0),
             (5, 5, 5, 9, 1, 0, 0), (9, 5, 5, 9, 1, 0, 4 * 4 * 6), (0, 0, W + 1, H, 1, 0, (W + 1) * H * 6), (0, 0, W, H + 1, 1, 1, W * (H + 1) * 6),
             (-1, 0, W, H, 1, 0, (W + 1) * H * 6), (0, -1, W, H, 1, 0, W * (H + 1) * 6),
             (0, 0, W, H, 2, 0, full), (0, 0, W, H, -1, 0, full), (0, 0, W, H, 1, 2, full), (0, 0, W, H, 1, -1, full)]
    for c in cases:
        rc = call(*c)
        assert rc == -1, (c, rc)      # VSPG_EINVAL
        assert lib.vspg_last_error(), c
        assert (buf == 0x5a5a).all() and n.value == 77, c
    assert lib.vspg_film_resolve(None, 0, 0, W, H, 1, 0, buf.ctypes.data_as(C.c_void_p), full, None, None) == -1
    assert lib.vspg_film_resolve(r.h, 0, 0, W, H, 1, 0, None, full, None, None) == -1
    # the Python wrapper raises the same error
    with pytest.raises(P.VspgError) as e:
        r.film_resolve((0, 0, W + 1, H))
    assert e.value.code == -1
    # a right call still works afterwards, n_clamped may be NULL, and nothing is written past out_bytes
    assert lib.vspg_film_resolve(r.h, 0, 0, W, H, 1, 0, buf.ctypes.data_as(C.c_void_p), full, None, None) == 0
    assert (buf[W * H * 3:] == 0x5a5a).all() and not (buf[:W * H * 3] == 0x5a5a).all()
    out, _ = r.film_resolve(half=True)
    assert np.array_equal(buf[:W * H * 3], out.view(np.uint16).ravel())
    r.close()
