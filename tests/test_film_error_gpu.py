"""Film error against a reference image, reduced on the device (vspg_film_error_enqueue, csrc/vspg_film_error.h).

The checker is numpy on the film the renderer itself returns: v = where(w != 0, rgb / w, rgb) in float32 (RGBFilm::GetPixelRGB,
film.h:269-287), the terms of Image::MSE / Image::MRSE (src/pbrt/util/image.cpp:594, :626) in float64, a term that is infinite left
out (:595-597, :627-629), math.fsum per channel as the exact sum S.

The bound on a sum is the textbook one for ANY order of adding n non-negative doubles: |computed - S| <= gamma * S with
gamma = (n - 1) u / (1 - (n - 1) u), u = 2^-53, n the window's pixel count (8.4e-13 for 100 x 76, 2.3e-10 at 1080p).  It needs no
measurement and leaves the kernel free in its tree.

One point where the reference's formula and a plain reading of "an infinite reference pixel is skipped" part: for ref_c = +inf the
squared error is +inf and is skipped, but the RELATIVE term is inf / Sqr(inf + 0.01) = NaN, which IsInf does not catch
(image.cpp:626-629), so that channel's sum_rse is NaN in the reference and here; the three sum_se stay finite.  The skip test
asserts exactly that, against the numpy checker, which restates the same formula."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_window_gpu import SHAPES, H, W

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
U = 2.0 ** -53


def gamma(n):
    return (n - 1) * U / (1 - (n - 1) * U)


def normalised(film):
    rgb, w = film[..., :3], film[..., 3:4]
    with np.errstate(all="ignore"):
        v = np.where(w != 0, rgb / w, rgb)
    assert v.dtype == np.float32
    return v


def exact_sums(film, ref, win):
    """-> [S_se[0..2], S_rse[0..2]]: math.fsum of the terms that are not infinite"""
    x0, y0, x1, y1 = win
    v = normalised(film)[y0:y1, x0:x1].astype(f64)
    q = np.asarray(ref, dtype=f32)[y0:y1, x0:x1].astype(f64)
    with np.errstate(all="ignore"):
        se = (v - q) ** 2
        rse = (v - q) ** 2 / (q + 0.01) ** 2
    out = []
    for terms in (se, rse):
        for c in range(3):
            t = terms[..., c].ravel()
            t = t[~np.isinf(t)]
            out.append(float("nan") if np.isnan(t).any() else math.fsum(t.tolist()))
    return out


def six(rec):
    return list(rec.sum_se) + list(rec.sum_rse)


def bits(rec):
    return struct.pack("<6d", *six(rec))


def check_sums(rec, film, ref, win, label, slack=1.0):
    n = (win[2] - win[0]) * (win[3] - win[1])
    assert rec.window() == tuple(win) and rec.n_pixels == n
    S = exact_sums(film, ref, win)
    g = slack * gamma(n)
    for k, (got, want) in enumerate(zip(six(rec), S)):
        rel = abs(got - want) / want if want else abs(got - want)
        print("%-30s sum[%d] = %.17g  exact %.17g  rel.err %.3e  bound %.3e" % (label, k, got, want, rel, g))
        assert math.isfinite(got) and got >= 0
        assert abs(got - want) <= g * want, (label, k, got, want)


def waves(r, w0, w1):
    for w in range(w0, w1):
        r.render_wave(w, w + 1)
        r.post_process_wave()


def fog_renderer(P, w=W, h=H, seed=0, spp=64):
    r = P.Renderer(P.fog_box_scene(w, h), P.app_f_params(), w, h, spp=spp, seed=seed)
    assert r.kernel_name().startswith("k_render_wave_wg3<"), r.kernel_name()
    return r


_REF = {}


def reference_image(P, w=W, h=H):
    """the normalised film of an independently seeded 64-wave render"""
    if (w, h) not in _REF:
        r = fog_renderer(P, w, h, seed=1234)
        waves(r, 0, 64)
        _REF[(w, h)] = normalised(r.film()).copy()
        r.close()
    return _REF[(w, h)]


def test_sums_after_one_and_four_waves_for_every_window_shape(gpu_pkg):
    P = gpu_pkg
    ref = reference_image(P)
    r = fog_renderer(P, seed=3)
    r.set_reference_image(ref)
    films = []
    for n_before, n_after in ((0, 1), (1, 4)):
        waves(r, n_before, n_after)
        for win in SHAPES:
            r.film_error_enqueue(win, tag=n_after)
        films.append(r.film())
    recs = r.film_errors()
    assert len(recs) == 2 * len(SHAPES)
    for i, rec in enumerate(recs):
        win, film = SHAPES[i % len(SHAPES)], films[i // len(SHAPES)]
        assert rec.tag == (1, 4)[i // len(SHAPES)]
        check_sums(rec, film, ref, win, "%d waves %r" % (rec.tag, win))
    assert recs[-1].tick_khz > 0
    r.close()


def test_reference_equal_to_the_film_gives_exact_zeros(gpu_pkg):
    """pins the pixel value to ONE correctly rounded float division: a reciprocal multiply or a double division leaves residues"""
    P = gpu_pkg
    r = fog_renderer(P, seed=5)
    waves(r, 0, 3)
    film = r.film()
    assert (film[..., 3] > 0).all() and len(np.unique(film[..., 0] / film[..., 3])) > 1000   # (a real image, no trivial quotients)
    r.set_reference_image(normalised(film))
    r.film_error_enqueue()
    r.film_error_enqueue((13, 5, 77, 50))
    for rec in r.film_errors():
        assert bits(rec) == struct.pack("<6d", *([0.0] * 6)), six(rec)
    r.close()


def test_same_state_gives_the_same_bits(gpu_pkg):
    P = gpu_pkg
    ref = reference_image(P)
    seen = []
    for attempt in range(2):
        r = fog_renderer(P, seed=9)
        r.set_reference_image(ref)
        waves(r, 0, 2)
        for win in (SHAPES[0], SHAPES[-1], SHAPES[0], SHAPES[-1]):
            r.film_error_enqueue(win)
        waves(r, 2, 5)
        r.film_error_enqueue()
        r.film_error_enqueue()
        recs = r.film_errors()
        assert bits(recs[0]) == bits(recs[2]) and bits(recs[1]) == bits(recs[3]) and bits(recs[4]) == bits(recs[5])
        assert bits(recs[0]) != bits(recs[1]) != bits(recs[4])
        seen.append([bits(x) for x in recs])
        r.close()
    assert seen[0] == seen[1]


def test_record_is_of_the_complete_film_on_the_headline_configuration(gpu_pkg):
    """k_render_wave_wg3, one-sample waves, carry enabled: enqueue directly behind render_wave, no flush in between"""
    import ctypes as C
    P = gpu_pkg
    assert os.environ.get("VSPG_WG3_CARRY", "1") != "0" and os.environ.get("VSPG_WG2_DEFER", "1") != "0"
    w, h, n = 160, 96, 7
    ref = reference_image(P, w, h)
    r = fog_renderer(P, w, h, seed=11)
    r.set_reference_image(ref)
    for s in range(n):          # (no post-processing: no buffer update drains anything)
        r.render_wave(s, s + 1)
    f = r.lib.vspg_debug_carry_resumes
    f.restype, f.argtypes = C.c_longlong, [C.c_void_p]
    assert int(f(r.h)) > 0, "no launch resumed carried paths: the test would show nothing"
    r.film_error_enqueue(tag=n)
    film = r.film()
    assert r.counters()["paths"] == w * h * n
    assert (film[..., 3] > 0).all()
    (rec,) = r.film_errors()
    check_sums(rec, film, ref, (0, 0, w, h), "headline, carried")
    r.close()


def test_infinite_terms_are_skipped_nan_terms_poison_and_unrendered_pixels_take_the_w0_branch(gpu_pkg):
    P = gpu_pkg
    ref = reference_image(P)
    r = fog_renderer(P, seed=13)
    r.render_window(*SHAPES[0], 0, 1)       # the interior window only: every other pixel keeps weight 0
    film = r.film()
    assert (film[..., 3] == 0).sum() == W * H - (77 - 13) * (50 - 5)
    full = (0, 0, W, H)
    # (a) weight 0 outside the window: v = rgbSum = 0 there
    r.set_reference_image(ref)
    r.film_error_enqueue(full)
    # (b) +inf in channel 1 of some pixels, inside and outside the rendered window
    inf_ref = ref.copy()
    inf_ref[7, 3, 1] = inf_ref[20, 40, 1] = inf_ref[49, 76, 1] = np.inf
    r.set_reference_image(inf_ref)
    r.film_error_enqueue(full)
    # (c) a NaN in channel 2
    nan_ref = ref.copy()
    nan_ref[30, 30, 2] = np.nan
    r.set_reference_image(nan_ref)
    r.film_error_enqueue(full)
    a, b, c = r.film_errors()
    check_sums(a, film, ref, full, "partly rendered")
    # (b): the three squared-error sums are finite and are the numpy sums with those terms left out; so are the relative sums of
    # channels 0 and 2; channel 1's relative sum is NaN, as image.cpp:626-629 makes it (module docstring)
    S = exact_sums(film, inf_ref, full)
    Sa = exact_sums(film, ref, full)
    g = gamma(W * H)
    print("inf:", six(b), S)
    assert S[1] < Sa[1] and math.isfinite(S[1])            # the checker did leave terms out
    for k in (0, 1, 2, 3, 5):
        assert math.isfinite(b.sum_se[k] if k < 3 else b.sum_rse[k - 3])
        assert abs(six(b)[k] - S[k]) <= g * S[k], (k, six(b)[k], S[k])
    assert math.isnan(S[4]) and math.isnan(b.sum_rse[1])
    # (c): that channel's two sums are NaN, the others as ever
    S = exact_sums(film, nan_ref, full)
    print("nan:", six(c), S)
    assert math.isnan(c.sum_se[2]) and math.isnan(c.sum_rse[2]) and math.isnan(S[2]) and math.isnan(S[5])
    for k in (0, 1, 3, 4):
        assert abs(six(c)[k] - S[k]) <= g * S[k], (k, six(c)[k], S[k])
    r.close()


def test_windows_add_up(gpu_pkg):
    import importlib.util
    spec = importlib.util.spec_from_file_location("vspg_sharding", os.path.join(ROOT, "vspg-pbrt-v4_amd", "sharding.py"))
    sh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sh)
    P = gpu_pkg
    ref = reference_image(P)
    r = fog_renderer(P, seed=17)
    r.set_reference_image(ref)
    waves(r, 0, 4)
    bands = sh.window_bands(H, 3)
    assert bands[0][0] == 0 and bands[-1][1] == H
    for rank in range(3):
        sh.BandShard(r, W, H, rank, 3).film_error_enqueue(tag=4)
    r.film_error_enqueue(tag=4)
    *parts, whole = r.film_errors()
    assert [p.window() for p in parts] == [(0, y0, W, y1) for y0, y1 in bands]
    u = sh.combine_film_errors(parts)
    assert u.n_pixels == whole.n_pixels == W * H and u.window() == whole.window()
    g = 2 * gamma(W * H)
    for k, (a, b) in enumerate(zip(six(u), six(whole))):
        print("bands vs frame sum[%d]: %.17g %.17g rel %.3e bound %.3e" % (k, a, b, abs(a - b) / b, g))
        assert abs(a - b) <= g * b
    check_sums(u, r.film(), ref, (0, 0, W, H), "combined bands")
    assert abs(u.mse() - whole.mse()) <= abs(float(np.spacing(f32(whole.mse()))))
    r.close()


def test_log_order_ticks_emptying_and_overflow(gpu_pkg):
    P = gpu_pkg
    ref = reference_image(P)
    r = fog_renderer(P, seed=19)
    with pytest.raises(P.VspgError) as e:
        r.film_error_enqueue()
    assert e.value.code == P.VSPG_EINVAL and "reference image" in str(e.value)
    assert r.film_errors() == []
    r.set_reference_image(ref)
    with pytest.raises(P.VspgError) as e:        # window rules are vspg_render_window's
        r.film_error_enqueue((0, 0, W + 1, H))
    assert e.value.code == P.VSPG_EINVAL
    with pytest.raises(P.VspgError):
        r.film_error_enqueue((5, 5, 5, 9))
    tags = [7, 3, 11, 0, -2]
    for k, t in enumerate(tags):
        waves(r, k, k + 1)
        r.film_error_enqueue(tag=t)
    recs = r.film_errors()
    assert [x.tag for x in recs] == tags
    ticks = [x.device_ticks for x in recs]
    assert ticks == sorted(ticks) and ticks[0] > 0 and ticks[-1] > ticks[0]
    assert all(x.tick_khz == recs[0].tick_khz and x.tick_khz > 0 for x in recs)
    assert r.film_errors() == []                                     # reading empties the log
    # too little room: VSPG_EINVAL, log untouched
    import ctypes as C
    r.film_error_enqueue(tag=21)
    r.film_error_enqueue(tag=22)
    buf, n = (P.VspgFilmError * 1)(), C.c_size_t()
    assert r.lib.vspg_film_error_read(r.h, buf, 1, C.byref(n), None) == P.VSPG_EINVAL
    assert [x.tag for x in r.film_errors()] == [21, 22]
    # fill it; one more is refused, nothing is lost
    N = P.FILM_ERROR_LOG_RECORDS
    one_pixel = (37, 41, 38, 42)
    for k in range(N):
        r.film_error_enqueue(one_pixel if k else None, tag=k)
    with pytest.raises(P.VspgError) as e:
        r.film_error_enqueue(tag=N)
    assert e.value.code == P.VSPG_EINVAL and "full" in str(e.value)
    recs = r.film_errors()
    assert [x.tag for x in recs] == list(range(N))
    assert recs[0].n_pixels == W * H and all(x.n_pixels == 1 for x in recs[1:])
    assert all(bits(x) == bits(recs[1]) for x in recs[1:])
    ticks = [x.device_ticks for x in recs]
    assert ticks == sorted(ticks)
    check_sums(recs[0], r.film(), ref, (0, 0, W, H), "first of a full log")
    r.film_error_enqueue(tag=5)                                      # and the log takes records again
    assert [x.tag for x in r.film_errors()] == [5]
    r.close()


def test_wavefront_pipeline_boundary_scene_over_a_grid_medium(gpu_pkg):
    import scenes
    P = gpu_pkg
    scene = scenes.cloud_scene(W, H, scenes.cloud_density(24), 24)
    ref_r = P.Renderer(scene, P.app_f_params(), W, H, spp=16, seed=77)
    assert ref_r.kernel_name().startswith("k_wf_walk<GridMedium"), ref_r.kernel_name()
    ref_r.render_wave(0, 16)
    ref = normalised(ref_r.film()).copy()
    ref_r.close()
    r = P.Renderer(scene, P.app_f_params(), W, H, spp=16, seed=3)
    r.set_reference_image(ref)
    waves(r, 0, 1)
    r.film_error_enqueue(tag=1)
    r.film_error_enqueue(SHAPES[0], tag=1)
    film = r.film()
    a, b = r.film_errors()
    check_sums(a, film, ref, (0, 0, W, H), "cloud_scene frame")
    check_sums(b, film, ref, SHAPES[0], "cloud_scene interior")
    r.close()


def test_full_size_frame(gpu_pkg):
    P = gpu_pkg
    w, h = 1920, 1080
    ref = reference_image(P, w, h)
    r = fog_renderer(P, w, h, seed=23)
    r.set_reference_image(ref)
    waves(r, 0, 2)
    r.film_error_enqueue(tag=2)
    (rec,) = r.film_errors()
    assert rec.n_pixels == 2073600
    check_sums(rec, r.film(), ref, (0, 0, w, h), "1920 x 1080")
    r.close()


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = map(int, f.readline().split())
        assert float(f.readline()) < 0
        return np.frombuffer(f.read(), dtype="<f4").reshape(h, w, 3)[::-1].copy()


def image_mse_average(img, ref):
    """Image::MSE(...).Average() (image.cpp:575-607, image.h:205-210) of two float images, the sums exact"""
    h, w, _ = img.shape
    d = (img.astype(f64) - ref.astype(f64)) ** 2
    acc = f32(0)
    for c in range(3):
        t = d[..., c].ravel()
        acc = f32(acc + f32(f64(math.fsum(t[~np.isinf(t)].tolist())) / f64(f32(w) * f32(h))))
    return f32(acc / f32(3))


@pytest.mark.parametrize("bounds", [None, (13, 60, 5, 40)])
def test_vspg_pbrt_writes_one_line_per_wave(gpu_pkg, tmp_path, bounds):
    host = os.path.join(ROOT, "vspg-pbrt-v4_amd", "host")
    subprocess.check_call(["make", "-C", host])
    exe, scene = os.path.join(host, "vspg_pbrt"), os.path.join(ROOT, "tests", "scenes", "fog_box.pbrt")
    ref_pfm, out_pfm, m = tmp_path / "ref.pfm", tmp_path / "out.pfm", tmp_path / "m.txt"
    a = subprocess.run([exe, scene, "--spp", "48", "--seed", "5", "--outfile", str(ref_pfm)], capture_output=True, text=True, timeout=300)
    assert a.returncode == 0, a.stdout + a.stderr
    args = [exe, scene, "--spp", "8", "--mse-reference-image", str(ref_pfm), "--mse-reference-out", str(m), "--outfile", str(out_pfm)]
    if bounds:
        args += ["--pixelbounds", ",".join(map(str, bounds))]
    b = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    lines = [ln.split(", ") for ln in m.read_text().splitlines()]
    assert [int(x[0]) for x in lines] == list(range(1, 9))
    vals = [f32(x[1]) for x in lines]
    assert all(np.isfinite(v) and v > 0 for v in vals)
    ref, out = read_pfm(str(ref_pfm)), read_pfm(str(out_pfm))
    if bounds:
        x0, x1, y0, y1 = bounds
        ref = ref[y0:y1, x0:x1]
    assert out.shape == ref.shape
    want = image_mse_average(out, ref)
    print("mse lines:", [float(v) for v in vals], "numpy on the written images:", float(want))
    assert abs(f64(vals[-1]) - f64(want)) <= f64(np.spacing(want)), (vals[-1], want)
    # --wave-log lines gain mse / mrse / device_ms with a reference image, and only then
    import json
    log = tmp_path / "w.jsonl"
    c = subprocess.run(args + ["--wave-log", str(log)], capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stdout + c.stderr
    rows = [json.loads(ln) for ln in log.read_text().splitlines()]
    assert len(rows) == 8 and all({"mse", "mrse", "device_ms"} <= set(x) for x in rows)
    assert [f32(x["mse"]) for x in rows] == [f32(ln.split(", ")[1]) for ln in m.read_text().splitlines()] == vals
    ms = [x["device_ms"] for x in rows]
    assert ms[0] == 0 and ms == sorted(ms) and ms[-1] > 0
    d = subprocess.run(args[:4] + ["--outfile", str(out_pfm), "--wave-log", str(log)], capture_output=True, text=True, timeout=300)
    assert d.returncode == 0, d.stdout + d.stderr
    assert all(set(json.loads(ln)) == {"wave", "ms", "paths", "segments", "density_queries", "kernel"} for ln in log.read_text().splitlines())
