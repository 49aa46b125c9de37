"""Thin-lens, orthographic and spherical cameras without a GPU: the float32 mirror (tests/camera_model.py) against the float64 statement
inside a derived bound and against hand answers, five planted errors that those checks must see, vspg_camera_look_at_window, the
C-ABI (symbols, sizes, the new record's layout), choose_kernel under `camera_general`, the host's camera code under sanitizers
(tests/camera_build_check.cpp, a stand-alone program), the scene-file forms, and the conditions the statistical GPU tests rest on.

THE BOUND (u = 2^-24, the unit roundoff of float32; every count is of roundings of magnitude <= u relative to the operand):
  raster map      c = s * p + o: two roundings, |dc| <= u (|s p| + |c|) <= 2 u C, with C = |s p| + |o|
  normalise       three squares, two sums, a square root, three divisions: the length carries <= 3 u relative (2.5 u of the sum, half of
                  it through the root, 1 u of the root, rounded up), each component one more: <= 4 u relative, plus the inputs' error
  pinhole         direction: 2 u C + 4 u                                                                          (|d| = 1)
  lens            ft = F / d.z: the division's u plus d.z's relative error (2 u C + 4 u) / d.z.  pFocus = o + d ft: product and sum, and
                  the errors of d and ft scaled by ft: |dpFocus| <= (2 (2 u C + 4 u) / d.z + 2 u) |pFocus| + (2 u C for o).
                  pLens = R disk: the disk's quotient, product with Pi/4, the subtraction from Pi/2 (absolute u Pi / 2 on theta), sin / cos
                  within 1 ulp, two products: <= 6 u R.  The difference adds u |pFocus - pLens|; normalising divides every absolute
                  error by |pFocus - pLens| and adds 4 u.
  frame           three products and two sums per component of a vector of length L: <= 3 u sqrt(3) L <= 6 u L (right, up, fwd are
                  unit vectors); the origin's sum one more rounding of |ro|.
  spherical       uv: one division (u relative); the angles 2 Pi uv[0] and Pi uv[1]: float Pi is 0.47 u off Pi, the product rounds once:
                  absolute <= 2 Pi (1 + 1.5) u = 15.8 u on phi; sin and cos within 1 ulp, one product: <= 18 u per component; the
                  equal-area map is held to its exact form by tests/test_envlight_model.py within the same order.  24 u covers both.
`direction_bound` and `origin_bound` below evaluate these expressions per ray from the float64 statement; nothing is fitted."""
import ctypes as C
import json
import os
import shlex
import subprocess

import numpy as np
import pytest

import camera_model as M
from conftest import ROOT

f32 = np.float32
U = 2.0 ** -24
CSRC = os.path.join(ROOT, "vspg-pbrt-v4_amd", "csrc")
HOST = os.path.join(ROOT, "vspg-pbrt-v4_amd", "host")
W, H = 33, 17      # no power of two: the uv division shows
EYE, LOOK, UP = (0.3, 0.2, -0.95), (0.0, 0.1, 0.0), (0.1, 1.0, 0.05)


def look_at(pkg, model, xres=W, yres=H, fov=60.0, **kw):
    return pkg.camera_look_at_window(model, EYE, LOOK, UP, fov, xres, yres, **kw)


def make(pkg, model, lens_radius=0.0, focal_distance=1e6, xres=W, yres=H, **kw):
    return M.Camera.from_c(look_at(pkg, model, xres, yres, **kw), model, xres, yres, lens_radius, focal_distance)


def axis_camera(model, lens_radius=0.0, focal_distance=1e6, xres=32, yres=16, origin=(1.0, 2.0, 3.0)):
    """The identity frame at `origin`, the raster map x -> x / 16 - 1, y -> 0.5 - y / 16: exact in float32, the centre is (0, 0)."""
    return M.Camera(origin, (1, 0, 0), (0, 1, 0), (0, 0, 1), 0.0625, -1.0, -0.0625, 0.5, model, xres, yres, lens_radius, focal_distance)


def sample_grid(n, seed, w=W, h=H):
    rng = np.random.default_rng(seed)
    pix = np.stack([rng.integers(0, w, n), rng.integers(0, h, n)], axis=1)
    u = rng.random((n, 4)).astype(f32)
    u[:8] = [[0, 0, 0, 0], [0, 0, 0.5, 0.5], [np.nextafter(f32(1), f32(0))] * 4, [0.5, 0.5, 0.75, 0.25], [0.5, 0.5, 0.25, 0.75], [0.1, 0.9, 0.8, 0.8],
             [0.9, 0.1, 0.5, 0.9], [0.3, 0.3, 0.9, 0.5]]
    pix[:4] = [[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]]
    return pix, u


def bounds(cam, pfx, pfy, ulx, uly):
    """(origin bound, direction bound) per ray from the float64 statement, as the module docstring derives them."""
    o, d = M.camera_space_ray64(cam, pfx, pfy, ulx, uly)
    n = o.shape[0]
    if cam.model >= M.SPHERICAL_EQUALAREA:
        return np.full(n, U * np.abs(cam.origin).max() + 1e-300), np.full(n, (24 + 6) * U)
    Cm = np.abs(float(cam.sx) * np.asarray(pfx, np.float64)) + abs(float(cam.ox)) + np.abs(float(cam.sy) * np.asarray(pfy, np.float64)) + abs(float(cam.oy))
    pin = 2 * U * Cm + 4 * U                     # the direction before the lens (orthographic: (0, 0, 1), exact)
    if not cam.has_lens:
        d_err = pin if cam.model == M.PERSPECTIVE else np.zeros(n)
        o_len = np.linalg.norm(o, axis=1)
        return U * (np.abs(cam.origin).max() + 2 * o_len) + 6 * U * o_len + 2 * U * Cm, d_err + 6 * U
    R, F = float(cam.lens_radius), float(cam.focal_distance)
    nolens = M.Camera(cam.origin, cam.right, cam.up, cam.fwd, cam.sx, cam.ox, cam.sy, cam.oy, cam.model, cam.xres, cam.yres)
    o0, d0 = M.camera_space_ray64(nolens, pfx, pfy, ulx, uly)
    dz = d0[:, 2]
    focus = o0 + d0 * (F / dz)[:, None]
    fl, sep = np.linalg.norm(focus, axis=1), np.linalg.norm(focus - o, axis=1)
    d_focus = (2 * pin / dz + 2 * U) * fl + 2 * U * Cm
    d_err = (d_focus + 6 * U * R + U * sep) / sep + 4 * U
    o_len = np.linalg.norm(o, axis=1)
    return U * (np.abs(cam.origin).max() + 2 * o_len) + 6 * U * o_len + 6 * U * R, d_err + 6 * U


def mirror_against_statement(cam, pix, u, plant=()):
    """max over the rays of |mirror - statement| / bound, for the origin and for the direction."""
    pfx, pfy = M.raster_point(pix[:, 0], pix[:, 1], u[:, 0], u[:, 1])
    ro, rd = M.generate_ray(cam, pfx, pfy, u[:, 2], u[:, 3], plant)
    ro64, rd64 = M.generate_ray64(cam, pfx, pfy, u[:, 2], u[:, 3])
    bo, bd = bounds(cam, pfx, pfy, u[:, 2], u[:, 3])
    return float((np.abs(ro - ro64).max(axis=1) / bo).max()), float((np.abs(rd - rd64).max(axis=1) / bd).max())


LENS_CASES = [(M.PERSPECTIVE, 0.0, 1e6), (M.PERSPECTIVE, 0.05, 1.95), (M.PERSPECTIVE, 0.3, 0.7), (M.ORTHOGRAPHIC, 0.0, 1e6), (M.ORTHOGRAPHIC, 0.05, 1.95),
              (M.ORTHOGRAPHIC, 0.4, 0.6), (M.SPHERICAL_EQUALAREA, 0.0, 1e6), (M.SPHERICAL_EQUIRECT, 0.0, 1e6)]


@pytest.mark.parametrize("model,R,F", LENS_CASES)
def test_mirror_against_the_float64_statement(pkg, model, R, F):
    cam = make(pkg, model, R, F)
    pix, u = sample_grid(600, 11 + model)
    eo, ed = mirror_against_statement(cam, pix, u)
    print("model %d R %g F %g: origin error / bound %.3f, direction error / bound %.3f" % (model, R, F, eo, ed))
    assert eo <= 1 and ed <= 1, (eo, ed)


# ---- known answers by hand ---------------------------------------------------------------------------------------------------------
def ray1(cam, pfx, pfy, ulx=0.5, uly=0.5, plant=()):
    ro, rd = M.generate_ray(cam, [pfx], [pfy], [ulx], [uly], plant)
    return ro[0], rd[0]


def hand_answers(plant=()):
    """Every hand answer as (name, got, want, tolerance); tolerance 0 = bit for bit."""
    out = []
    o3 = np.array([1, 2, 3], f32)
    # the centre pixel of each model (raster (16, 8) of the 32 x 16 axis camera)
    ro, rd = ray1(axis_camera(M.PERSPECTIVE), 16, 8, plant=plant)
    out += [("perspective centre o", ro, o3, 0), ("perspective centre d", rd, [0, 0, 1], 0)]
    ro, rd = ray1(axis_camera(M.ORTHOGRAPHIC), 16, 8, plant=plant)
    out += [("orthographic centre o", ro, o3, 0), ("orthographic centre d", rd, [0, 0, 1], 0)]
    ro, rd = ray1(axis_camera(M.ORTHOGRAPHIC), 24, 4, plant=plant)          # (0.5, 0.25, 0) in camera space
    out += [("orthographic off-centre o", ro, [1.5, 2.25, 3], 0), ("orthographic off-centre d", rd, [0, 0, 1], 0)]
    ro, rd = ray1(axis_camera(M.SPHERICAL_EQUALAREA), 16, 8, plant=plant)   # uv (.5, .5): the map's north pole (0, 0, 1), swapped to +y
    out += [("equal-area centre o", ro, o3, 0), ("equal-area centre d", rd, [0, 1, 0], 0)]
    ro, rd = ray1(axis_camera(M.SPHERICAL_EQUIRECT), 16, 8, plant=plant)    # theta = Pi / 2, phi = Pi: (-1, 0, 0)
    out += [("equirectangular centre d", rd, [-1, 0, 0], 4 * U * np.pi)]
    # poles and seams.  equirectangular: uv[1] = 0 is theta = 0, the direction (0, 0, 1) swapped to +y whatever phi is; uv[0] = 0 is
    # phi = 0, at mid-height (1, 0, 0)
    _, rd = ray1(axis_camera(M.SPHERICAL_EQUIRECT), 11, 0, plant=plant)
    out += [("equirectangular pole", rd, [0, 1, 0], 0)]
    _, rd = ray1(axis_camera(M.SPHERICAL_EQUIRECT), 0, 8, plant=plant)
    out += [("equirectangular seam", rd, [1, 0, 0], 4 * U * np.pi)]
    # equal-area: the corner uv (0, 0) is the south pole (0, 0, -1), swapped to -y; the edge midpoint uv (0, .5) is (-1, 0, 0)
    _, rd = ray1(axis_camera(M.SPHERICAL_EQUALAREA), 0, 0, plant=plant)
    out += [("equal-area pole", rd, [0, -1, 0], 0)]
    _, rd = ray1(axis_camera(M.SPHERICAL_EQUALAREA), 0, 8, plant=plant)
    out += [("equal-area seam", rd, [-1, 0, 0], 0)]
    # uv by division: at 33 x 17 the raster point (19, 8.5) is uv (19/33, 1/2), and float32 19 * (1 / 33) is not float32 19 / 33;
    # equirectangular theta = Pi / 2 (sinf gives exactly 1), phi = 2 Pi * (19 / 33): (cos phi, sin phi) bit for bit
    cam = axis_camera(M.SPHERICAL_EQUIRECT, xres=33, yres=17)
    phi = f32(f32(2) * M.PI) * (f32(19) / f32(33))
    _, rd = ray1(cam, 19, 8.5, plant=plant)
    out += [("uv by division", rd[[0, 2]], [M.EM.cosf(phi)[0], M.EM.sinf(phi)[0]], 0)]
    # the degenerate disk sample: the pinhole's ray -- the origin bit for bit, the direction inside one more normalisation
    for model in (M.PERSPECTIVE, M.ORTHOGRAPHIC):
        pin, lens = axis_camera(model), axis_camera(model, 0.25, 2.0)
        ro0, rd0 = ray1(pin, 21.25, 3.5, plant=plant)
        ro1, rd1 = ray1(lens, 21.25, 3.5, 0.5, 0.5, plant=plant)
        if model == M.PERSPECTIVE:
            out += [("uLens (.5, .5) o, perspective", ro1, ro0, 0), ("uLens (.5, .5) d, perspective", rd1, rd0, 12 * U)]
        else:   # the reference's orthographic lens starts at the LENS point, the centre of the lens here: the camera origin
            out += [("uLens (.5, .5) o, orthographic", ro1, o3, 0)]
        # a lens ray at camera depth F meets the pinhole ray's point there
        ro2, rd2 = ray1(lens, 21.25, 3.5, 0.9, 0.3, plant=plant)
        F = 2.0
        p_lens = ro2.astype(np.float64) + rd2.astype(np.float64) * ((3 + F - float(ro2[2])) / float(rd2[2]))
        p_pin = ro0.astype(np.float64) + rd0.astype(np.float64) * (F / float(rd0[2]))
        out += [("focus point, model %d" % model, p_lens, p_pin, 40 * U * F)]
    # the reference's orthographic quirk: the lens ray starts at the lens point l, not at pCamera + l, so the point seen at depth Z is
    # X Z / F + l (1 - Z / F).  X = (0.5, 0.25); uLens (1, .5) is the disk point (1, 0), R = 0.2: l = (0.2, 0); F = 2, Z = 1:
    # (0.25 + 0.1, 0.125 + 0) = (0.35, 0.125)
    lens = axis_camera(M.ORTHOGRAPHIC, 0.2, 2.0)
    ro, rd = ray1(lens, 24, 4, 1.0, 0.5, plant=plant)
    out += [("orthographic lens o", ro, [1.2, 2, 3], 2 * U * 3)]
    p = ro.astype(np.float64) + rd.astype(np.float64) * (1.0 / float(rd[2]))
    out += [("orthographic quirk", p, [1.35, 2.125, 4.0], 16 * U * 4)]
    return out


def failed(answers):
    bad = []
    for name, got, want, tol in answers:
        got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
        ok = np.array_equal(got, want) if tol == 0 else bool(np.all(np.abs(got - want) <= tol))
        if not ok:
            bad.append((name, got.tolist(), want.tolist()))
    return bad


def test_hand_answers():
    assert failed(hand_answers()) == []


def golden_sampler_cases():
    G = json.load(open(os.path.join(ROOT, "tests", "golden", "primitives.json")))
    return [c for c in G["independent_sampler"] if len(c["f"]) >= 6]


def sampler_dimensions_ok(oracle, plant=()):
    """The lens variates are dimensions 4 and 5 of the pixel sample, the filter's 1 and 2: against the golden vectors of the
    reference's own IndependentSampler (tests/golden/primitives.json)."""
    cases = golden_sampler_cases()
    assert cases
    for c in cases:
        got = M.sampler_variates(oracle, [[c["px"], c["py"]]], [c["sample"]], seed=c["seed"], plant=plant)[0]
        want = np.array([float.fromhex(c["f"][k]) for k in (1, 2, 4, 5)], f32)
        if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
            return False
    return True


def test_sampler_dimensions(oracle):
    assert sampler_dimensions_ok(oracle)


@pytest.mark.parametrize("plant", ["lens_plus_pcamera", "ft_no_divide", "no_yz_swap", "uv_reciprocal", "wrong_dims"])
def test_planted_errors_fail(pkg, oracle, plant):
    """Each planted error is seen by a check that passes without it: the hand answers, the mirror against the statement, or the
    sampler's golden vectors."""
    seen = []
    if failed(hand_answers((plant,))):
        seen.append("hand answers")
    for model, R, F in LENS_CASES:
        eo, ed = mirror_against_statement(make(pkg, model, R, F), *sample_grid(300, 5), plant=(plant,))
        if eo > 1 or ed > 1:
            seen.append("statement, model %d R %g" % (model, R))
    if not sampler_dimensions_ok(oracle, (plant,)):
        seen.append("sampler")
    print(plant, "seen by", seen)
    assert seen, plant
    if plant == "uv_reciprocal":   # it shows at a resolution that is no power of two, and only there
        pix, u = sample_grid(300, 5, 32, 16)
        cam = make(pkg, M.SPHERICAL_EQUIRECT, xres=32, yres=16)
        a = M.rays_of_samples(cam, pix, u)[1]
        b = M.rays_of_samples(cam, pix, u, plant=(plant,))[1]
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        cam = make(pkg, M.SPHERICAL_EQUIRECT)
        pix, u = sample_grid(300, 5)
        assert not np.array_equal(M.rays_of_samples(cam, pix, u)[1].view(np.uint32), M.rays_of_samples(cam, pix, u, plant=(plant,))[1].view(np.uint32))


# ---- vspg_camera_look_at_window ---------------------------------------------------------------------------------------------------------
def cam_bytes(c):
    return bytes(memoryview(c))


@pytest.mark.parametrize("xres,yres,fov", [(33, 17, 60.0), (17, 33, 37.5), (64, 64, 90.0), (1920, 1080, 45.0)])
def test_look_at_window_default_equals_look_at(pkg, xres, yres, fov):
    lib = pkg.load()
    a = pkg.VspgCamera()
    assert lib.vspg_camera_look_at(C.byref(a), pkg.f3(*EYE), pkg.f3(*LOOK), pkg.f3(*UP), fov, xres, yres) == 0
    b = pkg.camera_look_at_window(pkg.CAMERA_PERSPECTIVE, EYE, LOOK, UP, fov, xres, yres)
    assert cam_bytes(a) == cam_bytes(b)
    assert cam_bytes(pkg.fog_box_scene(xres, yres).camera) == cam_bytes(pkg.camera_look_at_window(0, (0, 0, -0.95), (0, 0, 0), (0, 1, 0), 60.0, xres, yres))


def test_look_at_window_hand_answers(pkg):
    raster = lambda c: (c.sx, c.ox, c.sy, c.oy)
    o = pkg.CAMERA_ORTHOGRAPHIC
    assert raster(look_at(pkg, o, 32, 16, screen_window=(-2, 6, -1, 3))) == (0.25, -2.0, -0.25, 3.0)
    assert raster(look_at(pkg, o, 32, 16, frame_aspect=2.0)) == (0.125, -2.0, -0.125, 1.0)      # [-2, 2] x [-1, 1]
    assert raster(look_at(pkg, o, 32, 16, frame_aspect=0.5)) == (0.0625, -1.0, -0.25, 2.0)      # [-1, 1] x [-2, 2]
    assert raster(look_at(pkg, o, 32, 16)) == (0.125, -2.0, -0.125, 1.0)                        # the film's own aspect, 2
    assert raster(look_at(pkg, o, 16, 32)) == (0.125, -1.0, -0.125, 2.0)                        # ... and 1/2: [-1, 1] x [-2, 2]
    p = raster(look_at(pkg, pkg.CAMERA_PERSPECTIVE, 32, 16, fov=90.0, screen_window=(-2, 6, -1, 3)))   # tan(45 degrees) = 1 within an ulp of double
    assert np.allclose(p, (0.25, -2.0, -0.25, 3.0), rtol=2e-7, atol=0)
    t = np.tan(np.radians(30.0))
    p = raster(look_at(pkg, pkg.CAMERA_PERSPECTIVE, 32, 16, fov=60.0, frame_aspect=0.5))
    assert np.allclose(p, (2 * t / 32, -t, -4 * t / 16, 2 * t), rtol=2e-7, atol=0)
    s = look_at(pkg, pkg.CAMERA_SPHERICAL_EQUIRECT, 32, 16, screen_window=(-2, 6, -1, 3))
    assert raster(s) == (0, 0, 0, 0) and list(s.fwd) == list(look_at(pkg, o, 32, 16).fwd) and list(s.origin) == [f32(v) for v in EYE]
    for kw in (dict(frame_aspect=-1.0), dict(frame_aspect=float("nan")), dict(screen_window=(0, 1, float("inf"), 1))):
        with pytest.raises(pkg.VspgError):
            look_at(pkg, o, **kw)
    with pytest.raises(pkg.VspgError):
        look_at(pkg, 4)


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------------------
def test_symbols_sizes_and_layout(pkg, tmp_path):
    by_name = {name: (res, args) for name, res, args in pkg.SYMBOLS}
    assert len(by_name["vspg_renderer_set_camera"][1]) == 4 and len(by_name["vspg_camera_look_at_window"][1]) == 10 and len(by_name["vspg_camera_ray_batch"][1]) == 8
    lib = pkg.load()
    for n in ("vspg_renderer_set_camera", "vspg_camera_look_at_window", "vspg_camera_ray_batch"):
        assert hasattr(lib, n), n
    assert lib.vspg_abi_version() == 7 and C.sizeof(pkg.VspgScene) == 4392
    assert (pkg.CAMERA_PERSPECTIVE, pkg.CAMERA_ORTHOGRAPHIC, pkg.CAMERA_SPHERICAL_EQUALAREA, pkg.CAMERA_SPHERICAL_EQUIRECT) == (0, 1, 2, 3)
    fields = [n for n, _ in pkg.VspgCameraModel._fields_]
    assert fields == ["model", "lens_radius", "focal_distance"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vspg.h"', "int main(void) {",
             'printf("%zu %zu %zu %d\\n", sizeof(VspgCameraModel), sizeof(VspgCamera), sizeof(VspgScene), VSPG_ABI_VERSION);']
    lines += ['printf("%%zu\\n", offsetof(VspgCameraModel, %s));' % f for f in fields]
    lines += ['printf("%d %d %d %d\\n", VSPG_CAMERA_PERSPECTIVE, VSPG_CAMERA_ORTHOGRAPHIC, VSPG_CAMERA_SPHERICAL_EQUALAREA, VSPG_CAMERA_SPHERICAL_EQUIRECT);', "return 0; }"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(tmp_path / "layout.c")])
    out = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    assert out[:4] == [C.sizeof(pkg.VspgCameraModel), C.sizeof(pkg.VspgCamera), 4392, 7] and out[0] == 12
    assert out[4:7] == [getattr(pkg.VspgCameraModel, f).offset for f in fields] and out[7:] == [0, 1, 2, 3]
    z = pkg.VspgCameraModel()
    assert (z.model, z.lens_radius, z.focal_distance) == (0, 0.0, 0.0)
    # the refusals that need no renderer
    cam = look_at(pkg, 0)
    assert lib.vspg_renderer_set_camera(None, C.byref(cam), None, None) == pkg.VSPG_EINVAL and b"null renderer" in lib.vspg_last_error()
    v = np.zeros(4, f32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    assert lib.vspg_camera_ray_batch(None, 1, np.zeros(2, np.int32).ctypes.data_as(ip), np.zeros(1, np.int32).ctypes.data_as(ip), None, v.ctypes.data_as(fp),
                                     v.ctypes.data_as(fp), None) == pkg.VSPG_EINVAL
    h = open(os.path.join(ROOT, "include", "vspg.h")).read()
    doc = " ".join(h.replace(" * ", " ").split())
    for words in ("CLEARS NOTHING", "vspg_film_clear and its peers are the caller's business", "vspg_renderer_set_camera, the buffer setters", "zeroed = today's pinhole"):
        assert words in doc, words


# ---- choose_kernel ------------------------------------------------------------------------------------------------------------------------
CHOICE_PROGRAM = r"""
#include <cstdio>
#include "vspg_kernel_choice.h"
using namespace vspg_choice;
int main() {
    const int media[] = {VSPG_MEDIUM_HOMOGENEOUS, VSPG_MEDIUM_GRID, VSPG_MEDIUM_NANOVDB, VSPG_MEDIUM_RGBGRID};
    const char *const kernels[] = {"", "lane", "wg", "wf"};
    for (int cam = 0; cam < 2; ++cam)
        for (int m = 0; m < 4; ++m)
            for (int guided = 0; guided < 2; ++guided)
                for (int k = 0; k < 4; ++k) {
                    ChoiceFacts f;  // a grey fog box: the headline configuration under the pinhole
                    f.medium_type = media[m];
                    f.medium_grey = f.surfaces_grey = f.null_zero = true;
                    f.guided = guided, f.training = guided;
                    f.camera_general = cam;
                    ChoiceEnv e;
                    e.kernel = kernels[k];
                    const KernelChoice c = choose_kernel(f, e);
                    std::printf("%d %d %d %s| %s %d\n", cam, media[m], guided, kernels[k], kernel_name(c).c_str(), c.arith_covered ? 1 : 0);
                }
    std::printf("default %d\n", ChoiceFacts().camera_general ? 1 : 0);
    return 0;
}
"""


def test_choose_kernel_under_camera_general(tmp_path):
    (tmp_path / "choice.cpp").write_text(CHOICE_PROGRAM)
    exe = str(tmp_path / "choice")
    subprocess.check_call(["c++", "-std=c++17", "-I", CSRC, "-o", exe, str(tmp_path / "choice.cpp")])
    lines = subprocess.check_output([exe], text=True).splitlines()
    assert lines[-1] == "default 0"
    got = {}
    for l in lines[:-1]:
        key, val = l.split("| ")
        cam, m, g, k = (key.split(" ") + [""])[:4]
        got[(int(cam), int(m), int(g), k)] = tuple(val.split(" "))
    HOM, GRID, NVDB, RGB = 1, 2, 3, 4
    # the pinhole: the table as it was
    assert got[(0, HOM, 0, "")] == ("k_render_wave_wg3<HomogeneousMediumT<2,true>>", "1")
    assert got[(0, HOM, 1, "")][0] == "k_render_wave_wg2<HomogeneousMediumT<2,true>,guided,train>"
    assert got[(0, HOM, 1, "lane")][0] == "k_render_wave<HomogeneousMediumT<2,true>,guided,train>"
    assert got[(0, GRID, 0, "wg")][0] == "k_render_wave_wg<GridMediumGrey>" or got[(0, GRID, 0, "wg")][0].startswith("k_render_wave_wg<GridMedium")
    # another camera over fog: the full-scene workgroup kernel; guided: the per-lane kernel; VSPG_KERNEL=lane: the per-lane kernel
    assert got[(1, HOM, 0, "")] == ("k_render_wave_wg2<HomogeneousMedium>", "0")
    assert got[(1, HOM, 0, "wg")][0] == "k_render_wave_wg2<HomogeneousMedium>"
    assert got[(1, HOM, 0, "lane")][0] == "k_render_wave<HomogeneousMedium>"
    assert got[(1, HOM, 1, "")][0] == "k_render_wave<HomogeneousMedium,guided,train>"
    assert got[(1, HOM, 1, "lane")][0] == "k_render_wave<HomogeneousMedium,guided,train>"
    # grid, NanoVDB and RGB grid: the pipeline, as under the pinhole; lane: the per-lane kernel; no rectangle-scene workgroup kernel
    for m in (GRID, NVDB, RGB):
        for g in (0, 1):
            for k in ("", "wf"):
                assert got[(1, m, g, k)] == got[(0, m, g, k)] and got[(1, m, g, k)][0].startswith("k_wf_"), (m, g, k)
            assert got[(1, m, g, "lane")][0].startswith("k_render_wave<") and got[(1, m, g, "lane")] == got[(0, m, g, "lane")]
            assert got[(1, m, g, "wg")][0].startswith("k_render_wave<"), got[(1, m, g, "wg")]
    # no row under another camera names a rectangle-scene instantiation or k_render_wave_wg3
    for key, (name, _) in got.items():
        if key[0] == 1:
            assert "wg3" not in name and "MediumT<" not in name, (key, name)


# ---- the host's camera code under sanitizers: a stand-alone program -----------------------------------------------------------------------
def test_host_camera_code_under_sanitizers(tmp_path):
    """tests/camera_build_check.cpp with the two host-only units, compiled with the library's flags plus AddressSanitizer and
    UndefinedBehaviorSanitizer on the host side, linked without the HIP runtime and run directly."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    hipcc, clangxx = os.path.join(rocm, "bin", "hipcc"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")
    for tool in (hipcc, clangxx):
        if not os.path.exists(tool):
            pytest.fail("%s not found (ROCm)" % tool)
    flags = shlex.split(subprocess.check_output(["make", "-s", "--no-print-directory", "-C", CSRC, "print-HIPFLAGS"], text=True))
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    host = [a for s in sanitize for a in ("-Xarch_host", s)]
    jobs = [(os.path.join(CSRC, u + ".hip"), []) for u in ("vspg_scene_build", "vspg_scene_api")] + \
           [(os.path.join(ROOT, "tests", "camera_build_check.cpp"), ["-x", "hip", "-I", CSRC])]
    procs, objs = [], []
    for src, extra in jobs:
        obj = str(tmp_path / (os.path.splitext(os.path.basename(src))[0] + ".o"))
        objs.append(obj)
        cmd = [hipcc] + flags + host + ["-g"] + extra + ["-c", "-o", obj, src]
        procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for cmd, p in procs:
        out = p.communicate()[0]
        assert p.returncode == 0, "%s\n%s" % (" ".join(cmd), out)
    exe = str(tmp_path / "camera_build_check")
    subprocess.check_call([clangxx] + sanitize + ["-o", exe] + objs)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, "exit status %d\n%s\n%s" % (p.returncode, p.stdout, p.stderr)
    assert p.stderr.strip() == "", p.stderr
    assert "camera_build_check: ok" in p.stdout


# ---- scene files ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vspg_pbrt():
    exe = os.path.join(HOST, "vspg_pbrt")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", CSRC, "libvspg_hip.so"])
        subprocess.check_call(["make", "-C", HOST])
    return exe


SCENE = """LookAt 0 0 -0.95   0 0 0   0 1 0
MediumInterface "" "fog"
Camera %(camera)s
Sampler "independent" "integer pixelsamples" 4
Film "rgb" "integer xresolution" 32 "integer yresolution" 16 "string filename" "%(out)s"
Integrator "guidedvolpathvspg" "integer maxdepth" 5 "bool vspguiding" true "bool surfaceguiding" false
    "bool volumeguiding" false "bool vspsecondaryguiding" false
WorldBegin
MakeNamedMedium "fog" "string type" "homogeneous" "rgb sigma_a" [ .05 .05 .05 ] "rgb sigma_s" [ .45 .45 .45 ] "float g" 0
MediumInterface "fog" "fog"
Material "diffuse" "rgb reflectance" [ .73 .73 .73 ]
Shape "bilinearmesh" "point3 P" [ -1 -1 1    -1 1 1     1 -1 1     1 1 1 ]
AttributeBegin
  Material "diffuse" "rgb reflectance" [ 0 0 0 ]
  AreaLightSource "diffuse" "rgb L" [ 17 12 4 ]
  Shape "bilinearmesh" "point3 P" [ -0.25 0.999 -0.25   0.25 0.999 -0.25   -0.25 0.999 0.25   0.25 0.999 0.25 ]
AttributeEnd
"""


def parse_camera(exe, tmp_path, camera):
    (tmp_path / "scene.pbrt").write_text(SCENE % {"camera": camera, "out": "x.pfm"})
    return subprocess.run([exe, str(tmp_path / "scene.pbrt"), "--parse-only"], capture_output=True, text=True)


def camera_line(r):
    return [l for l in r.stdout.splitlines() if l.startswith("camera: ")][0]


def test_scene_file_camera_forms(vspg_pbrt, tmp_path):
    t = np.tan(np.radians(30.0))
    fmt = lambda v: "%.9g" % f32(v)
    cases = [
        ('"perspective" "float fov" 60', "model 0 lens_radius 0 focal_distance 0 raster (%s, %s, %s, %s)" % (fmt(4 * t / 32), fmt(-2 * t), fmt(-2 * t / 16), fmt(t))),
        ('"perspective" "float fov" 60 "float lensradius" 0.05 "float focaldistance" 1.95', "model 0 lens_radius 0.0500000007 focal_distance 1.95000005 raster"),
        ('"perspective" "float fov" 90 "float lensradius" 0.125', "model 0 lens_radius 0.125 focal_distance 1000000 raster"),
        ('"perspective" "float fov" 60 "float focaldistance" 3', "model 0 lens_radius 0 focal_distance 0 raster"),
        ('"orthographic"', "model 1 lens_radius 0 focal_distance 0 raster (0.125, -2, -0.125, 1)"),
        ('"orthographic" "float screenwindow" [ -2 6 -1 3 ] "float lensradius" 0.25 "float focaldistance" 2', "model 1 lens_radius 0.25 focal_distance 2 raster (0.25, -2, -0.25, 3)"),
        ('"orthographic" "float frameaspectratio" 0.5', "model 1 lens_radius 0 focal_distance 0 raster (0.0625, -1, -0.25, 2)"),
        ('"spherical"', "model 2 lens_radius 0 focal_distance 0 raster (0, 0, 0, 0)"),
        ('"spherical" "string mapping" "equalarea"', "model 2 lens_radius 0"),
        ('"spherical" "string mapping" "equirectangular" "float lensradius" 3 "float focaldistance" 7 "float screenwindow" [ -1 1 -1 1 ] "float frameaspectratio" 2',
         "model 3 lens_radius 0 focal_distance 0 raster (0, 0, 0, 0)"),
    ]
    for camera, want in cases:
        r = parse_camera(vspg_pbrt, tmp_path, camera)
        assert r.returncode == 0, (camera, r.stdout + r.stderr)
        assert want in camera_line(r), (camera, camera_line(r), want)


def test_scene_file_camera_refusals_by_name(vspg_pbrt, tmp_path):
    cases = [('"spherical" "string mapping" "fisheye"', 'unknown mapping "fisheye"'),
             ('"orthographic" "float screenwindow" [ -1 1 -1 ]', '"screenwindow" should have four values'),
             ('"perspective" "float fov" 60 "float screenwindow" [ -1 1 ]', '"screenwindow" should have four values'),
             ('"realistic" "string lensfile" "wide.dat"', 'Camera "realistic"'),
             ('"fisheye"', 'Camera "fisheye"'),
             ('"perspective" "float lensradius" -1', '"lensradius"'),
             ('"orthographic" "float lensradius" 0.1 "float focaldistance" 0', '"focaldistance"'),
             ('"perspective" "float fov" 60 "float lensradus" 0.1', "lensradus"),
             ('"orthographic" "float fov" 60', "fov")]
    for camera, needle in cases:
        r = parse_camera(vspg_pbrt, tmp_path, camera)
        assert r.returncode != 0 and needle in r.stderr, (camera, needle, r.stdout + r.stderr)


def test_fog_box_dof_scene_parses(vspg_pbrt):
    """tests/scenes/fog_box_dof.pbrt is fog_box.pbrt through a thin lens; before cameras had a lens it was refused."""
    r = subprocess.run([vspg_pbrt, os.path.join(ROOT, "tests", "scenes", "fog_box_dof.pbrt"), "--parse-only"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "7 rectangles" in r.stdout and "model 0 lens_radius 0.0500000007 focal_distance 1.95000005" in camera_line(r)
    a = open(os.path.join(ROOT, "tests", "scenes", "fog_box.pbrt")).read().splitlines()
    b = open(os.path.join(ROOT, "tests", "scenes", "fog_box_dof.pbrt")).read().splitlines()
    changed = [(x, y) for x, y in zip(a, b) if x != y]
    assert len(a) == len(b) and len(changed) == 3 and any("lensradius" in y and "focaldistance" in y for _, y in changed)


# ---- the conditions the statistical GPU tests rest on -------------------------------------------------------------------------------------
def test_depth_of_field_geometry_conditions():
    """tests/test_camera_gpu.py photographs an emissive half-plane's edge through a lens.  For its geometry every tested pixel's hit
    probability lies in [0.1, 0.9], for both cameras, and the closed form it integrates agrees with a brute-force count of lens
    points on the bright side under the float64 statement."""
    import camera_dof as D
    for model in (M.PERSPECTIVE, M.ORTHOGRAPHIC):
        g = D.geometry(model)
        P = D.hit_probability(g)
        assert P.shape == (len(g.pixels),) and len(g.pixels) == 32
        assert P.min() >= 0.1 and P.max() <= 0.9, (model, P.min(), P.max())
        assert np.all(np.diff(P) > 0)          # the blur rises monotonically across the row
        mc = D.hit_probability_by_statement(g, n=40000, seed=3)
        sigma = np.sqrt(P * (1 - P) / 40000)
        assert np.all(np.abs(mc - P) <= 5 * sigma), (model, np.abs(mc - P).max(), sigma.max())
