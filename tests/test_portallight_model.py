"""The portal image infinite light on the CPU: the float32 mirror of tests/portallight_model.py against hand-derived answers and its
float64 statement, the project's tan / atan2 against float64 over a dense sweep, five planted errors, the C-ABI additions, the wrapper's
refusals, and the host builder together with the host build of the sampling code under sanitizers
(tests/portallight_build_check.cpp, a stand-alone program fed with case files and compared with the mirror bit for bit)."""
import ctypes as C
import math
import os
import shlex
import subprocess

import numpy as np
import pytest

import portallight_model as M
from conftest import ROOT

f32 = np.float32
HEADER = os.path.join(ROOT, "include", "vspg.h")
CSRC = os.path.join(ROOT, "vspg-pbrt-v4_amd", "csrc")
# |portal_atan2f - atan| <= 2.4e-7 (absolute, radians) and |portal_tanf / tan - 1| <= 3 * 2^-24 (sin and cos within
# 2^-24 each -- they are double polynomials rounded once --, one division)
ATAN_BOUND = 2.4e-7
TAN_REL_BOUND = 3 * 2.0 ** -24


def u32(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


CASES, L_RGB, RADIUS, N_QUERIES, make_light, rotated = M.CASES, M.L_RGB, M.RADIUS, M.N_QUERIES, M.make_light, M.rotated


@pytest.fixture(scope="module")
def lights():
    return {c[0]: make_light(c) for c in CASES}


@pytest.fixture(scope="module")
def batches(lights):
    out = {}
    for c in CASES:
        p, d, u = M.make_queries(lights[c[0]], N_QUERIES, 100 + c[3])
        out[c[0]] = (p, d, u, lights[c[0]].batch(p, d, u))
    return out


# ---- 1. the project's tan and atan2 -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("portalshim") / "portallight_shim.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "portallight_shim.cpp")])
    lib = C.CDLL(so)
    fp = C.POINTER(C.c_float)
    lib.portal_tanf.argtypes = lib.portal_atanf.argtypes = [C.c_int, fp, fp]
    lib.portal_atan2f.argtypes = [C.c_int, fp, fp, fp]

    def call1(fn, x):
        x = np.ascontiguousarray(x, f32)
        y = np.empty_like(x)
        fn(x.size, x.ctypes.data_as(fp), y.ctypes.data_as(fp))
        return y
    return lib, call1


def test_tan_and_atan_stay_inside_the_derived_bounds(shim):
    """A dense sweep on the CPU: 2^22 arguments of atan over [-2^12, 2^12] (log-spaced magnitudes, every branch of the reduction and
    both thresholds' neighbourhoods) and 2^22 angles of tan over the closed range RenderFromImage produces, ends included."""
    lib, call1 = shim
    mag = np.concatenate([np.logspace(-12, 3.7, 1 << 21), np.nextafter(f32(2.414213562373095), f32([0, 9] * 8)), np.nextafter(f32(0.4142135623730950), f32([0, 9] * 8))]).astype(f32)
    t = np.concatenate([mag, -mag, f32([0.0, np.inf, -np.inf])])
    got = call1(lib.portal_atanf, t)
    err = np.abs(got.astype(np.float64) - np.arctan(t.astype(np.float64)))
    print("atan: max abs error %.3e rad over %d arguments (bound %.1e)" % (err.max(), t.size, ATAN_BOUND))
    assert err.max() <= ATAN_BOUND
    assert got[-2] == f32(math.pi / 2) and got[-1] == -f32(math.pi / 2) and got[-3] == 0
    sel = np.linspace(0, t.size - 1, 3000).astype(np.int64)
    assert np.array_equal(u32(got[sel]), u32(M.atanf(t[sel]))), "the NumPy mirror of atan differs from the C text"
    uv = np.linspace(0, 1, 1 << 22).astype(f32)
    a = (-M.PI_OVER_2 + (uv * M.PI).astype(f32)).astype(f32)
    got = call1(lib.portal_tanf, a)
    assert np.all(np.isfinite(got)), "tan must be finite for every uv in [0, 1], ends included"
    ref = np.tan(a.astype(np.float64))
    rel = np.abs(got.astype(np.float64) / ref - 1)[ref != 0]
    print("tan: max relative error %.3e over %d angles (bound %.3e); tan at uv = 0, 1: %g, %g" % (rel.max(), a.size, TAN_REL_BOUND, got[0], got[-1]))
    assert rel.max() <= TAN_REL_BOUND
    sel = np.linspace(0, a.size - 1, 3000).astype(np.int64)
    assert np.array_equal(u32(got[sel]), u32(M.tanf(a[sel]))), "the NumPy mirror of tan differs from the C text"


def test_image_from_render_inverts_render_from_image(lights):
    """ImageFromRender(RenderFromImage(uv)) is the identity inside the clamp, within the two functions' bounds: d(uv) <= (atan's
    bound + tan's relative bound * |sin cos|) / pi plus the roundings of Normalize and the frame (a few 2^-24)."""
    for name in ("16 peaked", "16 banded rot oblique"):
        light = lights[name]
        rng = np.random.default_rng(5)
        uv = np.concatenate([rng.uniform(0.002, 0.998, (4000, 2)), [[0.5, 0.5]]]).astype(f32)
        w, jac = light.render_from_image(uv[:, 0], uv[:, 1])
        ok, u, v, jac2 = light.image_from_render(w)
        assert ok.all() and np.all((u >= 0) & (u <= 1) & (v >= 0) & (v <= 1))
        # the map's own conditioning: alpha = atan2(x, z) moves by |dw| / hypot(x, z) when w moves by dw, and the components of w carry
        # the roundings of Normalize and of the frame there and back (3 products and 2 sums each way: <= 8 * 2^-24 absolute)
        wl = np.stack([w.astype(np.float64) @ light.fx.astype(np.float64), w.astype(np.float64) @ light.fy.astype(np.float64), w.astype(np.float64) @ light.fz.astype(np.float64)], axis=1)
        bu = (ATAN_BOUND + 8 * 2.0 ** -24 / np.hypot(wl[:, 0], wl[:, 2]) + 2 * 2.0 ** -24) / math.pi
        bv = (ATAN_BOUND + 8 * 2.0 ** -24 / np.hypot(wl[:, 1], wl[:, 2]) + 2 * 2.0 ** -24) / math.pi
        eu, ev = np.abs(u.astype(np.float64) - uv[:, 0]), np.abs(v.astype(np.float64) - uv[:, 1])
        print(name, "round trip: max |d uv| %.3e, worst error / bound %.3f" % (max(eu.max(), ev.max()), max((eu / bu).max(), (ev / bv).max())))
        assert np.all(eu <= bu) and np.all(ev <= bv)
        # the float64 statement of the same map and its Jacobian
        ue, ve, je = M.image_from_local_exact(wl)
        assert np.all(np.abs(ue - u) <= bu) and np.all(np.abs(ve - v) <= bv)
        assert np.all(np.abs(jac2 / je - 1) <= 1e-4 + 32 * 2.0 ** -24 / np.minimum(1 - wl[:, 0] ** 2, 1 - wl[:, 1] ** 2))


# ---- 2. hand-derived answers ---------------------------------------------------------------------------------------------------------
def test_tables_of_1x1_and_2x2_images():
    one = make_light(CASES[0])
    j = one.centre_jac[0, 0]
    # the 1 x 1 rectified image is the one texel; d = 0.75 * duv_dw(0.5, 0.5) = 0.75 * pi^2 (w = (0, 0, 1)); the table is d
    assert np.array_equal(one.image.reshape(-1), f32([0.75] * 3)) and j == f32(M.PI * M.PI)
    assert one.func[0, 0] == f32(f32(f32(2.25) / f32(3)) * j) and one.table[0, 0] == one.func[0, 0]
    two = M.PortalLight(M.make_image("random", 2, 1), M.AXIS_PORTAL)
    f = two.func.astype(np.float64)
    want = [[f[0, 0], f[0, 0] + f[0, 1]], [f[1, 0] + f[0, 0], ((f[1, 1] + (f[1, 0] + f[0, 0])) + (f[0, 0] + f[0, 1])) - f[0, 0]]]
    assert np.array_equal(u32(two.table), u32(np.array(want).astype(f32)))


def test_integral_of_whole_half_texel_and_empty_windows():
    light = M.PortalLight(M.make_image("random", 2, 1), M.AXIS_PORTAL)
    f = light.func.astype(np.float64)
    whole = light.integral(f32([[0, 0, 1, 1]]))[0]
    assert whole == f32(np.float64(light.table[1, 1]) / 4)                       # the last table entry over nx * ny
    assert abs(whole - f.sum() / 4) <= 2.0 ** -23 * f.sum() / 4
    half = light.integral(f32([[0, 0, 0.25, 0.5]]))[0]                           # half of texel (0, 0) in x, all of it in y
    assert half == f32(np.float64(f32(f32(0.5) * light.table[0, 0])) / 4)
    assert light.integral(f32([[0.3, 0.2, 0.3, 0.9]]))[0] == 0                   # an empty window
    assert light.integral(f32([[0.75, 0.25, 0.25, 0.75]]))[0] == 0               # an inverted one: max(., 0)
    assert M.window_integral_exact(f, (0, 0, 0.25, 0.5)) == f[0, 0] / 8


def test_bcond_equal_ends_case():
    """p.x on a texel edge: floor and ceil coincide and the column is [p.x, p.x + 1/nx]."""
    light = M.PortalLight(M.make_image("constant", 4, 0), M.AXIS_PORTAL)
    # a constant function... is not constant after the Jacobian, but it is symmetric: u0 = 0.5 over the symmetric window samples x = 0.5
    s = light.sample_uv(f32([[0.25, 0.25, 0.75, 0.75]]), f32([[0.5, 0.5]]))
    assert s["why"][0] == 0 and s["u"][0] == f32(0.5) and s["v"][0] == f32(0.5)
    assert s["cond"][0, 0] == f32(0.5) and s["cond"][0, 2] == f32(0.75)


def test_image_bounds_of_a_point_on_the_axis_are_symmetric(lights):
    for name in ("16 peaked", "64 random oblique"):
        light = lights[name]
        c = light.portal.astype(np.float64).mean(axis=0)
        p = (c[None, :] - np.array([[0.5], [1.0], [2.5]]) * light.fz.astype(np.float64)[None, :]).astype(f32)
        ok, b = light.image_bounds(p)
        assert ok.all()
        tol = 2 * ATAN_BOUND / math.pi + 16 * 2.0 ** -24
        assert np.all(np.abs(b[:, 0] + b[:, 2] - 1) <= tol) and np.all(np.abs(b[:, 1] + b[:, 3] - 1) <= tol)
        assert np.all(b[:, 2] > b[:, 0]) and np.all(b[:, 3] > b[:, 1])
        # closed form: the half-angles are atan(half-extent / distance)
        q = light.portal.astype(np.float64)
        hx, hy = np.linalg.norm(q[3] - q[0]) / 2, np.linalg.norm(q[1] - q[0]) / 2
        for i, h in enumerate((0.5, 1.0, 2.5)):
            assert abs(b[i, 2] - (math.atan(hx / h) + math.pi / 2) / math.pi) <= tol and abs(b[i, 3] - (math.atan(hy / h) + math.pi / 2) / math.pi) <= tol


# ---- 3. mirror against the float64 statement --------------------------------------------------------------------------------------
def test_density_over_a_window_sums_to_one(lights):
    for name in ("16 peaked", "16 half zero", "3 random rot"):
        light = lights[name]
        f = light.func.astype(np.float64)
        b = (0.21, 0.3, 0.77, 0.93)
        n = 240
        xs, ys = b[0] + (np.arange(n) + 0.5) * (b[2] - b[0]) / n, b[1] + (np.arange(n) + 0.5) * (b[3] - b[1]) / n
        bb = np.tile(f32(b), (n * n, 1))
        fint = light.integral(bb[:1])[0]
        dens = light.eval(np.tile(xs, n).astype(f32), np.repeat(ys, n).astype(f32)).astype(np.float64) / float(fint)
        total = dens.sum() * (b[2] - b[0]) * (b[3] - b[1]) / (n * n)
        exact = M.window_integral_exact(f, b)
        print(name, "window integral %.7g (exact %.7g), density sums to %.5f" % (fint, exact, total))
        assert abs(fint / exact - 1) <= 64 * 2.0 ** -24   # four lookups of <= 2^-24-rounded table entries, the double subtraction exact
        assert abs(total - 1) <= 0.02                     # midpoint rule on a step function: the cells the texel edges cut


def test_pdf_of_a_sample_is_the_pdf_sample_returned(lights, batches):
    """PDF_Li(wi) against the pdf SampleLi returned: bit for bit on a power-of-two image under the identity (uv -> wi -> uv may move
    (u, v) by the map's bound, which matters only next to a texel edge); elsewhere the same texel within the stated roundings."""
    for c in CASES:
        light = lights[c[0]]
        p, d, u, o = batches[c[0]]
        ok = o[:, 12] == 1
        if not ok.any():
            continue
        back = light.pdf_li(p[ok], o[ok, 17:20])
        uu, vv = o[ok, 13].astype(np.float64) * light.res, o[ok, 14].astype(np.float64) * light.res
        edge = np.minimum(np.abs(uu - np.round(uu)), np.abs(vv - np.round(vv))) * math.pi / light.res < (ATAN_BOUND + TAN_REL_BOUND)
        rel = np.abs(back.astype(np.float64) / o[ok, 20] - 1)
        far = ~edge & (back > 0)
        print(c[0], "pdf round trip: %d samples, %d near an edge, max rel %.2e" % (ok.sum(), edge.sum(), rel[far].max() if far.any() else 0))
        assert np.all(back[~edge] > 0)
        if not c[4] and not c[5] and light.res & (light.res - 1) == 0:   # identity, axis-aligned frame, power-of-two image
            assert np.array_equal(u32(back[~edge]), u32(o[ok, 20][~edge])), c[0]
        assert rel[far].max() <= 1e-5  # the Jacobian evaluated at w and at the re-derived w: a few ulp of (1 - x^2)


def test_px_brackets_u0_within_one_texel_mass(lights, batches):
    for name in ("16 peaked", "64 random oblique", "3 random rot"):
        light = lights[name]
        p, d, u, o = batches[name]
        f = light.func.astype(np.float64)
        worst = 0.0
        for i in np.nonzero(o[:, 12] == 1)[0][:60]:
            b = o[i, 1:5].astype(np.float64)
            cdf = M.window_cdf_x_exact(f, b, float(o[i, 13]))
            col = int(min(o[i, 13] * light.res, light.res - 1))
            mass = M.window_integral_exact(f, (max(b[0], col / light.res), b[1], min(b[2], (col + 1) / light.res), b[3])) / M.window_integral_exact(f, b)
            worst = max(worst, abs(cdf - u[i, 0]) - mass)
            assert abs(cdf - u[i, 0]) <= mass + 1e-4
        print(name, "Px(p.x) - u0 beyond one texel's mass: %.2e" % worst)


def test_fixtures_reach_every_branch_and_stay_below_the_cap(lights, batches):
    why = np.concatenate([batches[c[0]][3][:, 26] for c in CASES]).astype(int)
    trips = np.concatenate([batches[c[0]][3][:, 24:26] for c in CASES])
    print("why histogram:", np.bincount(why, minlength=6), "max trips", trips.max(), "cap", M.BISECT_CAP)
    assert (why == M.WHY_OK).sum() > 0.5 * why.size
    assert (why == M.WHY_NO_BOUNDS).any(), "a point behind the portal plane"
    assert trips.max() < M.BISECT_CAP, "a bisection reached the cap"
    assert (why == M.WHY_BAD_T).sum() == 0, "no fixture may lose a sample to a non-finite interpolation parameter"
    # duv_dw == 0 (WHY_ZERO_JACOBIAN) IS reachable in float32, exactly on the image's edge: at u = 0 the tangent is -+2.29e7, Normalize
    # gives w.x = -+1 exactly (len == |x| in float) and 1 - w.x^2 = 0.  A sample lands there only with a window that starts at the
    # clamped u = 0 and the variate u0 = 0 (t = 0); no context point of the fixtures produces such a window (w.z would have to
    # underflow), so it is reached at the level of Sample, on the mirror: the sample is (0, v), its Jacobian 0, no light sample.
    light = lights["16 peaked"]
    s0 = light.sample_uv(f32([[0, 0.2, 0.5, 0.8]]), f32([[0, 0.5]]))
    _, jac = light.render_from_image(s0["u"], s0["v"])
    _, corner = light.render_from_image(f32([0, 1]), f32([0, 1]))
    print("sample on the edge:", s0["why"], s0["u"], s0["v"], "duv_dw", jac, "at the corners", corner)
    assert s0["why"][0] == M.WHY_OK and s0["u"][0] == 0 and jac[0] == 0 and np.all(np.isfinite(corner))
    assert (why == M.WHY_ZERO_JACOBIAN).sum() == 0
    # the zero window and the zero conditional column, from the half-zero image directly (windows inside / across the zero half)
    assert (why == M.WHY_ZERO_WINDOW).any() and (why == M.WHY_ZERO_COLUMN).any(), "the half-zero images reach both zero integrals"
    # ... and on a hand-made function (rows 0..7 zero): a window inside the zero half, one across it
    z = M.PortalLight(M.make_image("constant", 16, 0), M.AXIS_PORTAL)
    z.func = z.func.copy()
    z.func[:8] = 0
    z.table = z._summed_area(z.func)
    s = z.sample_uv(f32([[0.1, 0.05, 0.9, 0.4], [0.1, 0.05, 0.9, 0.95]]), f32([[0.3, 0.6], [0.3, 0.6]]))
    print("zero window:", s["why"])
    assert s["why"][0] == M.WHY_ZERO_WINDOW and s["why"][1] == M.WHY_OK and s["v"][1] >= 0.5
    # the non-power-of-two path ran (res 3), and context points keep away from the portal's vertices
    assert lights["3 random rot"].res == 3 and (batches["3 random rot"][3][:, 12] == 1).any()
    for c in CASES:
        p = batches[c[0]][0].astype(np.float64)
        dist = np.linalg.norm(p[:, None, :] - lights[c[0]].portal.astype(np.float64)[None, :, :], axis=2).min()
        assert dist > 0.1, (c[0], dist)


# ---- 4. planted errors --------------------------------------------------------------------------------------------------------------
def _comparisons(light):
    """name -> passes?  Each looks at one property of the light against the float64 statement or a hand-derived fact."""
    res = light.res
    out = {}
    f = light.func.astype(np.float64)
    exact = np.cumsum(np.cumsum(f, axis=0), axis=1)
    out["table against the exact sums"] = bool(np.all(np.abs(light.table / exact - 1) <= 2.0 ** -23))
    c = light.portal.astype(np.float64).mean(axis=0)
    p = (c - 1.3 * light.fz.astype(np.float64)).astype(f32).reshape(1, 3)
    ok, b = light.image_bounds(p)
    w, _ = light.render_from_image(b[:, 2], b[:, 3])
    # ImageFromRender of that direction may round either way: take the direction whose (u, v) IS the top corner, if there is one
    okk, u, v, _ = light.image_from_render(w)
    corner = bool(okk[0] and u[0] == b[0, 2] and v[0] == b[0, 3])
    inside = light.Le(p, w)[0][0]
    out["Le on the top edge of the bounds"] = (not corner) or bool(inside)
    xs = ((np.arange(res) + 0.5) / res)
    wl = M.local_from_image_exact(np.tile(xs, res), np.repeat(xs, res))
    je = (math.pi ** 2 * (1 - wl[:, 0] ** 2) * (1 - wl[:, 1] ** 2) / wl[:, 2]).reshape(res, res)
    avg = light.image.astype(np.float64).sum(axis=2) / 3
    # (1 - x^2 cancels towards the image's edge: its float32 value carries 4 * 2^-24 absolute)
    tol = 1e-5 + 8 * 2.0 ** -24 * (1 / (1 - wl[:, 0] ** 2) + 1 / (1 - wl[:, 1] ** 2)).reshape(res, res)
    out["d carries the Jacobian"] = bool(np.all(np.abs(f - avg * je) <= tol * np.abs(avg * je) + 1e-12))
    out["bounds of an axis point are symmetric"] = bool(ok[0] and abs(b[0, 0] + b[0, 2] - 1) <= 1e-5 and abs(b[0, 1] + b[0, 3] - 1) <= 1e-5
                                                        and b[0, 2] - b[0, 0] > 0.05 and b[0, 3] - b[0, 1] > 0.05)
    rng = np.random.default_rng(3)
    uv = (b[0, :2] + rng.uniform(0.1, 0.9, (50, 2)) * (b[0, 2:] - b[0, :2])).astype(f32)
    wq, _ = light.render_from_image(uv[:, 0], uv[:, 1])
    pdf = light.pdf_li(np.repeat(p, 50, axis=0), wq).astype(np.float64)
    wloc = np.stack([wq.astype(np.float64) @ light.fx.astype(np.float64), wq.astype(np.float64) @ light.fy.astype(np.float64), wq.astype(np.float64) @ light.fz.astype(np.float64)], axis=1)
    _, _, jq = M.image_from_local_exact(wloc)
    if M.window_integral_exact(f, b[0].astype(np.float64)) > 0:
        want = np.array([M.window_pdf_exact(f, b[0].astype(np.float64), float(uv[i, 0]), float(uv[i, 1])) for i in range(50)]) / jq
        out["PDF_Li is the window density over the Jacobian"] = bool(np.all(np.abs(pdf - want) <= 2e-3 * want))
    else:  # (an empty window has no density to compare)
        out["PDF_Li is the window density over the Jacobian"] = bool(np.all(pdf == 0))
    return out


PLANTED = {"float_table": "table against the exact sums", "exclusive_top": "Le on the top edge of the bounds",
           "no_jacobian_in_d": "d carries the Jacobian", "portal1": "bounds of an axis point are symmetric",
           "multiply_jacobian": "PDF_Li is the window density over the Jacobian"}


def test_the_unplanted_mirror_passes_every_comparison():
    got = _comparisons(make_light(CASES[6]))
    assert all(got.values()), got


@pytest.mark.parametrize("plant", sorted(PLANTED))
def test_planted_errors_fail_their_comparison_and_no_other(plant):
    got = _comparisons(make_light(CASES[6], plant=(plant,)))
    failed = sorted(k for k, v in got.items() if not v)
    assert failed == [PLANTED[plant]], (plant, got)


# ---- 5. the C-ABI additions, the wrapper's refusals ----------------------------------------------------------------------------------
def test_header_compiles_as_c99_with_the_new_declarations(pkg, tmp_path):
    src = tmp_path / "decl.c"
    src.write_text('#include <stdio.h>\n#include "vspg.h"\n'
                   'int (*a)(VspgRenderer *, int, const float *, int, const float *, const float *, void *) = vspg_renderer_set_portal_environment_image;\n'
                   'int (*b)(VspgRenderer *, int, int, const float *, const float *, const float *, float *, void *) = vspg_portallight_batch;\n'
                   'int (*c)(VspgRenderer *, int, int *, float *, float *, float *, float *, void *) = vspg_portallight_read;\n'
                   'int main(void) { printf("%zu %zu %d %d\\n", sizeof(VspgScene), sizeof(VspgMedium), VSPG_ABI_VERSION, VSPG_PORTALLIGHT_OUT); return a == 0 || b == 0 || c == 0; }\n')
    obj = tmp_path / "decl.o"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), "-c", "-o", str(obj), str(src)])
    src2 = tmp_path / "sizes.c"
    src2.write_text('#include <stdio.h>\n#include "vspg.h"\nint main(void) { printf("%zu %zu %d %d\\n", sizeof(VspgScene), sizeof(VspgMedium), VSPG_ABI_VERSION, VSPG_PORTALLIGHT_OUT); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src2)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["4392", "312", "7", "32"]
    assert C.sizeof(pkg.VspgScene) == 4392 and pkg.PORTALLIGHT_OUT == 32
    names = {s[0] for s in pkg.SYMBOLS}
    assert {"vspg_renderer_set_portal_environment_image", "vspg_portallight_batch", "vspg_portallight_read"} <= names
    assert pkg.load().vspg_abi_version() == 7


def test_refusals_that_need_no_renderer(pkg):
    lib = pkg.load()
    img = np.ones((2, 2, 3), f32)
    fp = C.POINTER(C.c_float)
    q = np.ascontiguousarray(M.AXIS_PORTAL)
    assert lib.vspg_renderer_set_portal_environment_image(None, 0, img.ctypes.data_as(fp), 2, None, q.ctypes.data_as(fp), None) == pkg.VSPG_EINVAL
    assert b"null" in lib.vspg_last_error()
    out = np.zeros(32, f32)
    assert lib.vspg_portallight_batch(None, 0, 1, out.ctypes.data_as(fp), out.ctypes.data_as(fp), out.ctypes.data_as(fp), out.ctypes.data_as(fp), None) == pkg.VSPG_EINVAL
    res = C.c_int(0)
    assert lib.vspg_portallight_read(None, 0, C.byref(res), None, None, None, None, None) == pkg.VSPG_EINVAL


def test_wrapper_refusals(pkg):
    for bad in (None, np.zeros((3, 3), f32), np.zeros(11, f32), "portal", [[0, 0, 0]] * 5):
        with pytest.raises(ValueError):
            pkg.portal_source(bad)
    q = pkg.portal_source(M.AXIS_PORTAL.astype(np.float64).tolist())
    assert q.dtype == f32 and q.shape == (4, 3) and q.flags["C_CONTIGUOUS"]
    with pytest.raises(ValueError):
        pkg.environment_image_source(np.ones((2, 3, 3), f32))


def test_the_quadrilateral_tests_of_the_model():
    assert M.portal_checks(M.AXIS_PORTAL) is None and M.portal_checks(M.oblique_portal()) is None
    skew = M.AXIS_PORTAL.copy()
    skew[2] += f32([0.3, 0, 0])
    assert M.portal_checks(skew) is not None
    para = M.AXIS_PORTAL.copy()
    para[2:] += f32([0.4, 0, 0])   # a parallelogram: opposite edges parallel, sides not perpendicular
    assert M.portal_checks(para) == "not perpendicular"
    deg = M.AXIS_PORTAL.copy()
    deg[1] = deg[0]
    assert M.portal_checks(deg) == "degenerate"
    nan = M.AXIS_PORTAL.copy()
    nan[3, 1] = np.nan
    assert M.portal_checks(nan) == "not finite"


# ---- 6. the host builder and the host build of the sampling code, under sanitizers ---------------------------------------------------
def write_case(path, case, light, p, d, u, portal=None):
    m34 = rotated() if case[4] else np.eye(3, 4, dtype=f32)
    with open(path, "wb") as f:
        f.write(np.array([light.res, p.shape[0]], np.int32).tobytes())
        for a in (m34, light.portal if portal is None else portal, f32(L_RGB), f32([RADIUS]), light.src, p, d, u):
            f.write(np.ascontiguousarray(a, f32).tobytes())


def read_out(path, res, n):
    raw = open(path, "rb").read()
    if np.frombuffer(raw[:4], np.int32)[0]:
        return None
    a = np.frombuffer(raw[4:], f32)
    npx = res * res
    o, parts = 0, {}
    for name, cnt in (("rec", 20), ("image", npx * 3), ("func", npx), ("table", npx), ("phi", 3), ("out", 32 * n)):
        parts[name] = a[o:o + cnt]
        o += cnt
    assert o == a.size
    return parts


def test_host_builder_and_sampling_equal_the_mirror_under_sanitizers(tmp_path, lights, batches):
    """tests/portallight_build_check.cpp with the two host-only units, compiled with the library's flags plus AddressSanitizer and
    UndefinedBehaviorSanitizer on the host side, linked without the HIP runtime and run directly: the rectified image, func, the float
    table, frame, Area, Phi's sums and Phi, and all 32 outputs per query -- trip counts included -- equal the mirror bit for bit."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    hipcc, clangxx = os.path.join(rocm, "bin", "hipcc"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")
    for tool in (hipcc, clangxx):
        if not os.path.exists(tool):
            pytest.fail("%s not found (ROCm)" % tool)
    args = []
    for i, c in enumerate(CASES):
        p, d, u, _ = batches[c[0]]
        write_case(str(tmp_path / ("case%d.bin" % i)), c, lights[c[0]], p, d, u)
        args += [str(tmp_path / ("case%d.bin" % i)), str(tmp_path / ("out%d.bin" % i))]
    bad = M.AXIS_PORTAL.copy()
    bad[2] += f32([0.3, 0, 0])
    write_case(str(tmp_path / "bad.bin"), CASES[0], lights[CASES[0][0]], *batches[CASES[0][0]][:3], portal=bad)
    args += [str(tmp_path / "bad.bin"), str(tmp_path / "bad.out")]
    flags = shlex.split(subprocess.check_output(["make", "-s", "--no-print-directory", "-C", CSRC, "print-HIPFLAGS"], text=True))
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    host = [a for s in sanitize for a in ("-Xarch_host", s)]
    jobs = [(os.path.join(CSRC, u + ".hip"), []) for u in ("vspg_scene_build", "vspg_scene_api")] + \
           [(os.path.join(ROOT, "tests", "portallight_build_check.cpp"), ["-x", "hip", "-I", CSRC])]
    procs, objs = [], []
    for src, extra in jobs:
        obj = str(tmp_path / (os.path.splitext(os.path.basename(src))[0] + ".o"))
        objs.append(obj)
        cmd = [hipcc] + flags + host + ["-g"] + extra + ["-c", "-o", obj, src]
        procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for cmd, pr in procs:
        out = pr.communicate()[0]
        assert pr.returncode == 0, "%s\n%s" % (" ".join(cmd), out)
    exe = str(tmp_path / "portallight_build_check")
    subprocess.check_call([clangxx] + sanitize + ["-o", exe] + objs)
    pr = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    print(pr.stdout)
    assert pr.returncode == 0, "exit status %d\n%s\n%s" % (pr.returncode, pr.stdout, pr.stderr)
    assert read_out(str(tmp_path / "bad.out"), 1, N_QUERIES) is None, "the skewed quadrilateral must be refused"
    for i, c in enumerate(CASES):
        light = lights[c[0]]
        got = read_out(str(tmp_path / ("out%d.bin" % i)), light.res, N_QUERIES)
        assert got is not None, c[0]
        rec = np.concatenate([light.p0, light.p2, light.fx, light.fy, light.fz, [light.area], light.sum_phi, [0]]).astype(f32)
        for name, want in (("rec", rec), ("image", light.image), ("func", light.func), ("table", light.table), ("phi", light.phi())):
            w = np.ascontiguousarray(want, f32).reshape(-1)
            neq = u32(got[name]) != u32(w)
            assert not neq.any(), "%s: %s differs at %d of %d (first %d: %r != %r)" % (c[0], name, neq.sum(), w.size, np.argmax(neq), got[name][np.argmax(neq)], w[np.argmax(neq)])
        want = batches[c[0]][3]
        g = got["out"].reshape(-1, 32)
        neq = u32(g) != u32(want)
        cols = sorted(set(np.nonzero(neq)[1].tolist()))
        assert not neq.any(), "%s: batch differs in %d elements, columns %s; first row %d\n got %r\nwant %r" % (
            c[0], neq.any(axis=1).sum(), cols, np.argmax(neq.any(axis=1)), g[np.argmax(neq.any(axis=1))], want[np.argmax(neq.any(axis=1))])
