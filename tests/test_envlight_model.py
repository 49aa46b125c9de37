"""The image infinite light's model (tests/envlight_model.py) held to the reference's own conditions, to the float64 statement of the
mathematics, to answers derived by hand, and shown to catch planted errors; and the C-ABI additions that need no device.  The device is
compared with the float32 mirror bit for bit in tests/test_envlight_gpu.py.

PDF(Sample(u)) == the pdf Sample returned, EXACTLY: PiecewiseConstant2D::Sample returns (func / rowInt) * (rowInt / integral) and PDF
returns func / integral -- three roundings against one, so in float32 the two differ in the last bits on a general image (the
reference's own test allows 1e-3 relative).  The equality is exact where the arithmetic is: `test_pdf_of_sample_is_sample_pdf` asserts
bit equality on an image of powers of two (every sum and quotient exact), and on the seeded images that PDF reads the very table entry
Sample chose, with the two values within the three roundings."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import envlight_model as M
from conftest import ROOT

f32 = np.float32
EPS = 2.0 ** -24
KINDS = ("peaked", "banded", "equal")
RESES = (1, 2, 3, 16, 64)


def rotation(scale=(1, 1, 1)):
    """A rotation about (1, 2, 3) by 0.7 rad times a scale, as a 3 x 4 float32 matrix."""
    a = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + math.sin(0.7) * K + (1 - math.cos(0.7)) * K @ K
    m = np.zeros((3, 4), f32)
    m[:, :3] = (R @ np.diag(scale)).astype(f32)
    return m


def unit_dirs(n, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)


# ---- mapping ---------------------------------------------------------------------------------------------------------------
def test_round_trip_satisfies_the_references_equal_area_conditions():
    """util/math_test.cpp, EqualArea.Randoms: 0.9999 < |v'| < 1.0001 and Dot(v, v') > 0.9999."""
    d = unit_dirs(10000, 1)
    u, v = M.sphere_to_square(d)
    assert np.all((u >= 0) & (u <= 1) & (v >= 0) & (v <= 1))
    w = M.square_to_sphere(u, v).astype(np.float64)
    l = np.linalg.norm(w, axis=1)
    assert np.all((l > 0.9999) & (l < 1.0001)), (l.min(), l.max())
    assert np.all((w * d).sum(axis=1) > 0.9999)


def test_mirror_against_the_exact_map():
    """|uv_mirror - uv_exact| <= 0.5 * (t1 + 13 eps) + eps, eps = 2^-24.
    The polynomial is the degree-6 MINIMAX fit of atan(b) * 2 / pi on [0, 1]: its error equioscillates, and at b = 0 it is the constant
    term t1 = 4.0676e-6 (atan(0) = 0), so |P - A| <= t1.  Float roundings on top, all on values <= 1 (absolute error <= eps each):
    b = min / max (1, and A' <= 2 / pi < 1), six fma of the Horner chain (6), `1 - phi` (1): |phi| off by t1 + 8 eps; r = sqrt(1 - |z|) (1);
    v = phi * r: (t1 + 8 eps) + eps (r) + eps (product) = t1 + 10 eps; u = r - v: + eps (r) + eps = t1 + 12 eps; the southern mirror
    1 - u: + eps = t1 + 13 eps; the result 0.5 * (u + 1): half of that plus the rounding of u + 1 in [1, 2], eps, halved -- taken whole."""
    d = unit_dirs(10000, 2)
    u, v = M.sphere_to_square(d)
    e = M.sphere_to_square_exact(d.astype(np.float64))
    bound = 0.5 * (float(M.T_COEF[0]) + 13 * EPS) + EPS
    err = np.abs(np.stack([u, v], axis=1).astype(np.float64) - e).max()
    print("mirror vs exact map: max error %.3e, bound %.3e" % (err, bound))
    assert err <= bound
    # and the exact pair is an inverse pair
    dn = d.astype(np.float64) / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)
    assert np.abs(M.square_to_sphere_exact(M.sphere_to_square_exact(dn)) - dn).max() < 1e-12


# ---- distribution ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("res", RESES)
def test_pdf_integrates_to_one(kind, res):
    light = M.EnvLight(M.make_image(kind, res, 11))
    p = M.pdf_exact(light.func)
    assert abs(p.mean() - 1.0) < 1e-12                       # the float64 statement: the step function over the unit square
    # the mirror's PDF at the texel centres: func / integral, the integral a sequential float sum of res terms per row and res rows,
    # each sum's relative error <= (terms + 1) eps, the quotient's eps: (2 res + 3) eps in all
    c = ((np.arange(res) + 0.5) / res).astype(f32)
    uu, vv = np.meshgrid(c, c)
    q = light.pdf_uv(uu.reshape(-1), vv.reshape(-1)).astype(np.float64)
    assert abs(q.mean() - 1.0) <= (2 * res + 3) * EPS, q.mean() - 1.0
    # over the sphere: pdf_li * 4 pi is that pdf (an equal-area map)
    d = M.square_to_sphere(uu.reshape(-1), vv.reshape(-1))
    s = light.pdf_li(d).astype(np.float64) * 4 * math.pi
    assert abs(s.mean() - 1.0) <= (2 * res + 6) * EPS, s.mean() - 1.0


def test_pdf_of_sample_is_sample_pdf():
    rng = np.random.default_rng(5)
    u = rng.random((2000, 2)).astype(f32)
    # powers of two, res a power of two: every product, sum and quotient of the builders and of Sample / PDF is exact
    img = np.exp2(rng.integers(-3, 4, (8, 8))).astype(f32)[..., None].repeat(3, axis=2)
    img[2] = 0
    light = M.EnvLight(img, plant=("uncompensated",))        # (the compensated function of such an image is not dyadic)
    uv, pdf, off = light.sample_uv(u)
    assert np.array_equal(light.pdf_uv(uv[:, 0], uv[:, 1]), pdf)
    assert np.all(pdf > 0) and not np.any(off[:, 1] == 2)
    for kind in KINDS:
        for res in RESES:
            light = M.EnvLight(M.make_image(kind, res, 11))
            uv, pdf, off = light.sample_uv(u)
            inside = (np.trunc(uv * f32(res)).astype(int) == off).all(axis=1)   # (o + du) / n rounds up to the next texel when du -> 1
            assert inside.mean() > 0.999
            table = (light.func[off[:, 1], off[:, 0]] / light.integral).astype(f32)
            assert np.array_equal(light.pdf_uv(uv[:, 0], uv[:, 1])[inside], table[inside])
            assert np.all(np.abs(table.astype(np.float64) - pdf) <= 3 * EPS * table)


# ---- known answers -----------------------------------------------------------------------------------------------------------
def test_one_by_one_image():
    light = M.EnvLight(np.full((1, 1, 3), 0.25, f32), L=(2, 4, 8))
    assert light.func.tolist() == [[1.0]] and light.cdf.tolist() == [[0.0, 1.0]] and light.mcdf.tolist() == [0.0, 1.0] and light.integral == 1
    d, u = unit_dirs(500, 3), np.random.default_rng(3).random((500, 2)).astype(f32)
    valid, uv, wi, pdf, L, _ = light.sample_li(u)
    assert valid.all() and np.array_equal(uv, u)
    assert np.all(pdf == f32(1) / f32(f32(4) * M.PI)) and abs(float(pdf[0]) - 1 / (4 * math.pi)) < 1e-8
    assert np.all(light.pdf_li(d) == pdf[0])
    assert np.all(L == np.array([0.5, 1.0, 2.0], f32)) and np.all(light.Le(d)[0] == np.array([0.5, 1.0, 2.0], f32))


def test_two_by_two_image_with_one_bright_texel():
    """d = [[1, 5], [1, 1]], average 2, compensated [[0, 3], [0, 0]].  Row 0: cdf 0, 0 + 0 / 2, 0 + 3 / 2 -> integral 1.5, cdf 0 0 1.
    Row 1: integral 0 -> the linear cdf 0 .5 1.  Marginal over (1.5, 0): 0, .75, .75 -> integral .75, cdf 0 1 1."""
    img = np.ones((2, 2, 3), f32)
    img[0, 1] = 5
    light = M.EnvLight(img)
    assert light.func.tolist() == [[0, 3], [0, 0]]
    assert light.cdf.tolist() == [[0, 0, 1], [0, 0.5, 1]]
    assert light.mfunc.tolist() == [1.5, 0] and light.mcdf.tolist() == [0, 1, 1] and light.integral == 0.75
    valid, uv, wi, pdf, L, _ = light.sample_li(np.array([[0.25, 0.5]], f32))
    # marginal: o = 0, du = .5, pdf 1.5 / .75 = 2, v = .25; row 0: o = 1, du = .25, pdf 3 / 1.5 = 2, u = (1 + .25) / 2
    assert valid[0] and uv.tolist() == [[0.625, 0.25]] and pdf[0] == f32(4) / f32(f32(4) * M.PI) and L.tolist() == [[5, 5, 5]]
    assert light.pdf_uv([0.625], [0.25])[0] == 4 and light.pdf_uv([0.2], [0.25])[0] == 0 and light.pdf_uv([0.7], [0.9])[0] == 0
    # the wrap, by hand.  The south pole is (u, v) = (1, 1): texel index (2, 2) -> mirrored across u = 1 to (1, -1) -> across v = 0 to (0, 1)
    le, luv = light.Le(np.array([[0, 0, -1]], f32))
    assert luv.tolist() == [[1.0, 1.0]] and le.tolist() == [[1, 1, 1]]
    # next to it along +x, u rounds to exactly 1 and v = 0.99965: index (2, 1) -> mirrored across u = 1 to 1, v FLIPPED to 2 - 1 - 1 = 0
    le, luv = light.Le(np.array([[1e-3, 0, -0.9999995]], f32))
    assert luv[0, 0] == 1.0 and 0.999 < luv[0, 1] < 1 and le.tolist() == [[5, 5, 5]]


def test_average_is_rounded_to_float_before_it_is_subtracted():
    """lights.cpp:1105-1107: `Float average = std::accumulate(d.begin(), d.end(), 0.) / d.size()` -- the double quotient becomes a float
    -- and `std::max<Float>(v - average, 0)` subtracts floats.  envlight_model.rounded_average_image() tells that from a double average:
    mean 1 + 3 * 2^-24 rounds (to even) to 1 + 2^-22, so only the last texel stays: 2^-22.  Row 0: integral 0, the linear cdf.  Row 1: cdf 0,
    0, 2^-22 / 2 -> integral 2^-23, cdf 0 0 1.  Marginal over (0, 2^-23): 0, 0, 2^-24 -> integral 2^-24, cdf 0 0 1."""
    img = M.rounded_average_image()
    assert M.sampling_function(img, compensated=False).tolist() == [[1, 1], [1 + 2.0 ** -22, 1 + 2.0 ** -21]]
    light = M.EnvLight(img)
    assert light.func.tolist() == [[0, 0], [0, 2.0 ** -22]]
    assert light.cdf.tolist() == [[0, 0.5, 1], [0, 0, 1]]
    assert light.mfunc.tolist() == [0, 2.0 ** -23] and light.mcdf.tolist() == [0, 0, 1] and light.integral == 2.0 ** -24
    assert light.pdf_uv([0.25, 0.75], [0.75, 0.75]).tolist() == [0, 4]         # texel (row 1, column 0) is NOT samplable
    u = np.random.default_rng(4).random((64, 2)).astype(f32)
    uv, pdf, off = light.sample_uv(u)
    assert np.all(off == 1) and np.all(pdf == 4)


def test_phi_in_the_references_order():
    """lights.cpp:1141 by hand on a 2 x 2 image: sumL = (1 + 5) + 1 + 1 = 8 per channel (negative texels clamp to 0), scene radius 2, scale
    (1, 0.5, 0.25): 4 pi^2 * 4 * scale * 8 / 4."""
    img = np.ones((2, 2, 3), f32)
    img[0, 1] = 5
    img[1, 1, 2] = -3
    light = M.EnvLight(img, L=(1, 0.5, 0.25))
    k = f32(f32(f32(f32(4) * M.PI) * M.PI) * f32(4))
    want = [f32(f32(f32(k * f32(s)) * f32(t)) / f32(4)) for s, t in ((1, 8), (0.5, 8), (0.25, 7))]
    assert light.phi(2.0).tolist() == [float(x) for x in want]
    assert abs(float(want[0]) - 4 * math.pi ** 2 * 4 * 8 / 4) < 1e-3


def test_all_equal_image_fills_with_ones():
    light = M.EnvLight(np.full((3, 3, 3), 0.75, f32))
    assert np.all(light.func == 1)
    third = f32(1) / f32(3)
    raw = [f32(0), third, f32(third + third), f32(f32(third + third) + third)]
    assert light.mfunc.tolist() == [float(raw[3])] * 3
    assert light.cdf[1].tolist() == [float(f32(x / raw[3])) for x in raw]
    assert abs(float(light.integral) - 1) <= 4 * EPS
    assert np.all(np.abs(light.pdf_li(unit_dirs(100, 4)).astype(np.float64) * 4 * math.pi - 1) <= 8 * EPS)


def test_zero_rows_get_the_linear_cdf_and_are_never_sampled():
    light = M.EnvLight(M.make_image("banded", 16, 11))
    zero = [v for v in range(16) if light.mfunc[v] == 0]
    assert len(zero) >= 8
    for v in zero:
        assert light.cdf[v].tolist() == [float(f32(i) / f32(16)) for i in range(17)]
    u = np.random.default_rng(6).random((4096, 2)).astype(f32)
    uv, pdf, off = light.sample_uv(u)
    assert not np.isin(off[:, 1], zero).any() and np.all(pdf > 0)


# ---- what the fixtures reach ----------------------------------------------------------------------------------------------------
def test_fixtures_reach_every_branch():
    light = M.EnvLight(M.make_image("banded", 16, 11))
    d, u = M.make_queries(light, 4096, 3)
    octant = (d[:, 0] < 0) * 4 + (d[:, 1] < 0) * 2 + (d[:, 2] < 0) * 1
    generic = np.all(d != 0, axis=1)
    for o in range(8):
        assert np.sum(generic & (octant == o)) >= 100, o
    x, y, z = np.abs(d[:, 0]), np.abs(d[:, 1]), np.abs(d[:, 2])
    assert np.sum(x < y) >= 100 and np.sum(x >= y) >= 100 and np.sum(d[:, 2] < 0) >= 100
    assert np.sum(f32(1) - z == 0) >= 2                     # r == 0: the poles
    assert np.sum(np.maximum(x, y) == 0) >= 2               # a == 0
    uu, vv = M.sphere_to_square(d)
    assert np.sum(uu == 1) >= 1 and np.sum(vv == 1) >= 1 and np.sum(uu == 0) >= 1 and np.sum(vv == 0) >= 1
    assert np.sum(np.trunc(uu * f32(16)) == 16) >= 1 and np.sum(np.trunc(vv * f32(16)) == 16) >= 1    # the wrap that follows
    on_marginal = np.isin(u[:, 1], light.mcdf)
    on_row = np.array([u[i, 0] in light.cdf[M.find_interval(light.mcdf, u[i, 1])] for i in range(64)])
    assert on_marginal.sum() >= 2 and on_row.sum() >= 2
    flat = 0
    for i in range(64):                                      # cdf[o + 1] == cdf[o]
        o = M.find_interval(light.mcdf, u[i, 1])
        flat += light.mcdf[o + 1] == light.mcdf[o]
        o0 = M.find_interval(light.cdf[o], u[i, 0])
        flat += light.cdf[o][o0 + 1] == light.cdf[o][o0]
    assert flat >= 1
    valid = light.sample_li(u)[0]
    assert (~valid).sum() >= 1 and valid.sum() >= 4000     # mapPDF == 0 is reached, and is the exception


# ---- planted errors ----------------------------------------------------------------------------------------------------------------
def comparisons(light_of):
    """The named comparisons a wrong light has to fail; light_of(image, m34) builds the light under test."""
    out = {}
    img = np.random.default_rng(12).uniform(0.2, 1.0, (16, 16, 3)).astype(f32)     # no peak: about half the texels stay above the average
    c = ((np.arange(16) + 0.5) / 16).astype(f32)
    uu, vv = np.meshgrid(c, c)
    centres = M.square_to_sphere(uu.reshape(-1), vv.reshape(-1))
    light = light_of(img, None)
    # 1. the solid-angle pdf integrates to one over the sphere
    out["pdf_integrates_to_one_over_the_sphere"] = abs((light.pdf_li(centres).astype(np.float64) * 4 * math.pi).mean() - 1) < 1e-4
    # 2. the sampled function is the compensated one, derived here in float64
    d = img.astype(np.float64).mean(axis=2)
    want = np.maximum(d - d.mean(), 0)
    out["function_is_the_compensated_one"] = np.allclose(M.pdf_exact(light.func), M.pdf_exact(want), rtol=1e-5, atol=1e-7)
    # 3. u[1] picks the row (the marginal), u[0] the column
    u = np.random.default_rng(8).random((512, 2)).astype(f32)
    uv, _, off = light.sample_uv(u)
    rows = np.searchsorted(light.mcdf.astype(np.float64), u[:, 1].astype(np.float64), side="right") - 1
    out["marginal_takes_the_second_variate"] = np.array_equal(off[:, 1], rows)
    # 4. the wrap of u == 1 flips v (derived by hand in test_two_by_two_image_with_one_bright_texel)
    two = np.ones((2, 2, 3), f32)
    two[0, 1] = 5
    out["wrap_flips_v"] = light_of(two, None).Le(np.array([[1e-3, 0, -0.9999995]], f32))[0].tolist() == [[5, 5, 5]]
    # 5. PDF_Li maps the UNNORMALISED ApplyInverse(w) (lights.cpp:1115): under a scale of 2 the float64 map of w / 2
    m = rotation((2, 2, 2))
    sl = light_of(img, m)
    w = unit_dirs(512, 9)
    wl = (np.linalg.inv(m[:, :3].astype(np.float64)) @ w.astype(np.float64).T).T
    e = M.sphere_to_square_exact(wl)      # (it does not normalise either)
    texel = np.floor(e * 16)
    clear = np.all(np.abs(e * 16 - np.round(e * 16)) > 1e-3, axis=1)      # away from texel borders: the float32 index is the exact one
    want_pdf = M.pdf_exact(sl.func)[np.clip(texel[:, 1], 0, 15).astype(int), np.clip(texel[:, 0], 0, 15).astype(int)]
    got = sl.pdf_li(w).astype(np.float64)
    got = got / got.max() * want_pdf.max()                                # (which texel, not the scale: comparison 1 has the scale)
    out["pdf_li_does_not_normalise"] = clear.sum() > 400 and np.allclose(got[clear], want_pdf[clear], rtol=1e-4, atol=1e-9)
    return out


def test_the_comparisons_hold_for_the_mirror():
    got = comparisons(lambda img, m: M.EnvLight(img, m34=m))
    assert all(got.values()), got


@pytest.mark.parametrize("plant,comparison", [("no_4pi", "pdf_integrates_to_one_over_the_sphere"), ("uncompensated", "function_is_the_compensated_one"),
                                              ("swap_variates", "marginal_takes_the_second_variate"), ("no_v_flip", "wrap_flips_v"),
                                              ("normalize_in_pdf", "pdf_li_does_not_normalise")])
def test_planted_errors_fail_their_comparison(plant, comparison):
    got = comparisons(lambda img, m: M.EnvLight(img, m34=m, plant=(plant,)))
    assert not got[comparison], (plant, got)
    assert all(v for k, v in got.items() if k != comparison), (plant, got)       # and only that one


def test_planted_errors_shift_the_estimators_expectation():
    """How the GPU unbiasedness test's sky was chosen: envlight_model.unbiased_sky(), the 16^2 'peaked' image of seed 11 with a peak
    factor of 30.  The model problem: one vertex with an isotropic phase function f = p_s = 1 / (4 pi) under the sky.  Arm A (NEE on): one
    NEE sample plus one phase-sampled escaping ray, weighed by the balance heuristic as the integrator weighs them -- NEE draws texel t
    with probability P_t and scores Le_t f / (p_l + p_s) = Le_t / (1 + pdf_t) (pdf per unit square), the escaping ray hits t with
    probability 1 / n and scores the same.  Arm B (usenee false): the escaping ray alone, scoring Le_t.  With the sampler's P and the
    evaluated pdf consistent arm A's expectation is the sphere mean of Le whatever the distribution, which is arm B's; a planted error
    breaks that.  Welch's statistic on 32 + 32 means of 48 x 32 pixels allows a difference of 4.5 * sqrt((Var_A + Var_B) / (32 * 1536))
    when every pixel is as noisy as the model problem's single estimate; both planted errors move arm A by more than ten times that.
    (With the 1e3 peak of the batch tests' images arm B's variance alone allows 0.43 on a mean of 1.9, and the uncompensated sampler's
    shift of 0.14 would pass: that sky cannot tell.)"""
    img = M.unbiased_sky()
    good = M.EnvLight(img)
    mean = M.expected_radiance_exact(img, (1, 1, 1))[0]
    le = np.maximum(img[..., 0].astype(np.float64), 0)

    def moments(sampler_func, pdf_func, pdf_scale=1.0):
        P = M.pdf_exact(sampler_func) / sampler_func.size            # probability of each texel
        score = le / (1.0 + pdf_scale * M.pdf_exact(pdf_func))
        m_nee, m_esc = (P * score).sum(), score.mean()
        var = (P * score ** 2).sum() - m_nee ** 2 + (score ** 2).mean() - m_esc ** 2
        return m_nee + m_esc, var

    comp = good.func.astype(np.float64)
    right, var_a = moments(comp, comp)
    assert abs(right - mean) < 1e-9 * mean
    var_b = (le ** 2).mean() - mean ** 2
    allowed = 4.5 * math.sqrt((var_a + var_b) / (32 * 1536))
    unc = M.sampling_function(img, compensated=False).astype(np.float64)
    for name, (wrong, _) in (("uncompensated", moments(unc, comp)), ("no_4pi", moments(comp, comp, 4 * math.pi))):
        print("%s: expectation %.4f against %.4f, allowed %.4f" % (name, wrong, mean, allowed))
        assert abs(wrong - mean) > 10 * allowed, (name, wrong, mean, allowed)


# ---- C-ABI additions -----------------------------------------------------------------------------------------------------------
def header():
    return open(os.path.join(ROOT, "include", "vspg.h")).read()


def params_of(name):
    m = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, header())
    assert m, name
    return [re.sub(r"/\*.*?\*/", "", a).strip().split()[-1].lstrip("*") for a in m.group(1).split(",")]


def test_header_declares_the_light_and_both_functions():
    h = header()
    assert "VSPG_LIGHT_IMAGE_INFINITE = 2" in h and "#define VSPG_ABI_VERSION 7" in h
    assert "#define VSPG_ENV_MAX_RES 4096" in h and "#define VSPG_ENVLIGHT_OUT 16" in h
    assert params_of("vspg_renderer_set_environment_image") == ["r", "infinite_light_index", "host_rgb", "res", "render_from_light", "stream"]
    assert params_of("vspg_envlight_batch") == ["r", "infinite_light_index", "n", "dirs", "u", "out", "stream"]
    doc = " ".join(h[h.index("The image of an image infinite light"):h.index("int vspg_renderer_set_environment_image")].replace(" * ", " ").split())
    for words in ("allowIncompletePDF = true", "Only the compensated distribution exists on the device", "top row first", "VSPG_ENV_MAX_RES (4096)",
                  "NaN or infinite", "singular", "film, VSP buffer, guiding fields and training state, counters and the error log persist"):
        assert words in doc, words


def test_symbols_list_them_and_the_library_exports_them(pkg):
    by_name = {name: (res, args) for name, res, args in pkg.SYMBOLS}
    res, args = by_name["vspg_renderer_set_environment_image"]
    assert res is C.c_int and len(args) == 6
    res, args = by_name["vspg_envlight_batch"]
    assert res is C.c_int and len(args) == 7
    lib = pkg.load()
    assert hasattr(lib, "vspg_renderer_set_environment_image") and hasattr(lib, "vspg_envlight_batch")
    assert lib.vspg_abi_version() == 7
    assert (pkg.LIGHT_UNIFORM_INFINITE, pkg.LIGHT_DISTANT, pkg.LIGHT_IMAGE_INFINITE, pkg.ENV_MAX_RES, pkg.ENVLIGHT_OUT) == (0, 1, 2, 4096, 16)
    s = pkg.add_infinite_light(pkg.VspgScene(), pkg.LIGHT_IMAGE_INFINITE, (1, 2, 3))
    assert s.n_infinite_lights == 1 and s.infinite_lights[0].type == 2 and list(s.infinite_lights[0].L) == [1, 2, 3]


def test_null_arguments_are_refused(pkg):
    lib = pkg.load()
    v = np.zeros(3, dtype=np.float32)
    fp = C.POINTER(C.c_float)
    assert lib.vspg_renderer_set_environment_image(None, 0, v.ctypes.data_as(fp), 1, None, None) == pkg.VSPG_EINVAL
    assert b"null argument" in lib.vspg_last_error()
    assert lib.vspg_envlight_batch(None, 0, 1, v.ctypes.data_as(fp), v.ctypes.data_as(fp), v.ctypes.data_as(fp), None) == pkg.VSPG_EINVAL
    assert b"null argument" in lib.vspg_last_error()


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s): the wrapper must refuse first" % name)


def test_wrapper_refuses_bad_images_before_the_library(pkg):
    r = pkg.Renderer.__new__(pkg.Renderer)
    r.lib, r.h = NoLibrary(), None
    good = np.zeros((4, 4, 3), dtype=np.float32)
    for bad, what in ((good.astype(np.float64), "float32"), (good.astype(np.float16), "float32"), (np.zeros((4, 4), np.float32), "shape"),
                      (np.zeros((4, 4, 4), np.float32), "shape"), (np.zeros((4, 5, 3), np.float32), "square"), (np.zeros((0, 0, 3), np.float32), "resolution"),
                      (np.zeros((4, 8, 3), np.float32)[:, ::2], "contiguous"), ([[[0.0] * 3] * 4] * 4, "NumPy array")):
        with pytest.raises(ValueError) as e:
            r.set_environment_image(0, bad)
        assert what in str(e.value), (what, str(e.value))
    with pytest.raises(ValueError) as e:
        r.set_environment_image(0, good, render_from_light=np.eye(4))
    assert "3 x 4" in str(e.value)
    with pytest.raises(ValueError):
        r.envlight_batch(0, np.zeros((3, 3), np.float32), np.zeros((2, 2), np.float32))
    with pytest.raises(AssertionError):     # a good image does reach the library
        r.set_environment_image(0, good, render_from_light=np.eye(3, 4))
