"""Point and spot lights on the CPU: the float32 mirror of tests/pointlight_model.py against its float64 statement, the closed forms
it restates (SmoothStep, Phi, Bounds), the planted errors those checks must catch, the C-ABI additions (record layout, refusals,
vspg_spot_light_look_at / vspg_point_light_at bit for bit), LightSource "point" in scene files, and the conditions the statistical
GPU test of a spot in fog rests on."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import pointlight_model as M
from conftest import ROOT

f32 = np.float32
EPS = 2.0 ** -24          # half an ulp of 1: the relative error of one float32 operation
HEADER = os.path.join(ROOT, "include", "vspg.h")
HOST = os.path.join(ROOT, "vspg-pbrt-v4_amd", "host")


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ctm_oblique():
    """A CTM with rotation and translation: Translate(0.3, -0.2, 0.5) * Rotate(37, (1, 2, 3))."""
    return M.mat4_mul(M.translate((0.3, -0.2, 0.5)), M.rotate(37.0, (1, 2, 3)))


def the_spot(ctm=True):
    return M.spot_light((3.0, 2.0, 1.0), (0.4, 1.5, -0.3), (-0.2, 0.1, 0.6), 30.0, 5.0, ctm=ctm_oblique() if ctm else None)


def contexts(light, n, seed):
    """Points 0.05 .. 20 units from the light in every direction."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.exp(rng.uniform(math.log(0.05), math.log(20.0), n))
    return (light.pos.astype(np.float64) + d * r[:, None]).astype(f32)


# ---- 1. the mirror against the float64 statement -------------------------------------------------------------------------------------
def mirror_error(light, p, planted=None):
    """Per context: max |wi - wi64|, and max |L - L64| over the channels relative to I / d^2 (the unattenuated radiance there)."""
    valid, wi, L, pdf, pl, delta = light.sample_li(p, planted)
    wi64, L64 = light.sample_li64(p)
    d2 = ((light.pos.astype(np.float64) - p.astype(np.float64)) ** 2).sum(axis=1)
    scale = light.I.astype(np.float64)[None, :] / d2[:, None]
    return np.abs(wi - wi64).max(axis=1), (np.abs(np.where(valid[:, None], L, 0) - L64) / scale).max(axis=1)


def bounds_for(light):
    """Bounds on the mirror's rounding error, derived from float32 rounding (EPS per operation, first order), not from what is observed.
      d = pos - p          one rounding per component                                            1 EPS (relative, per component)
      |d|^2                three squares (2 + 1 EPS each), two additions                         5 EPS
      |d|                  a square root halves that and adds its own rounding                   3.5 EPS
      wi = d / |d|         1 + 3.5 + 1 relative to a component no larger than 1                  5.5 EPS absolute  -> 6 EPS
      I / |d|^2 (point)    5 + 1                                                                 6 EPS relative    -> 7 EPS
    Spot lights: the linear part of mInv is a rotation (rows of length 1: |row|_1 <= sqrt 3), so v = mInv(-wi) has an absolute error of
    sqrt(3) * 5.5 + 3 EPS per component (three products and two sums of terms below 1), Normalize adds 5.5 more: cos(theta) is off by
    at most 18.1 EPS -> 19.  t = (cos - a) / (b - a) divides that by (b - a) and adds 3 EPS of its own (t <= 1); SmoothStep's slope is at
    most 1.5, and its three products and one difference add 5 EPS.  The falloff factor s is then off by 1.5 * (19 / (b - a) + 3) + 5
    EPS absolute; L = (I s) / |d|^2 by that plus 7 EPS of relative error in the scale of I / |d|^2."""
    wi_bound = 6 * EPS
    if light.kind == M.LIGHT_POINT:
        return wi_bound, 7 * EPS
    width = float(light.cos_start) - float(light.cos_end)
    return wi_bound, (1.5 * (19 / width + 3) + 5 + 7) * EPS


@pytest.mark.parametrize("which", ["point", "spot", "spot_ctm", "spot_wide"])
def test_mirror_agrees_with_the_float64_statement(which):
    light = {"point": lambda: M.point_light((3, 2, 1), (0.4, 1.5, -0.3), ctm=ctm_oblique()), "spot": lambda: the_spot(False),
             "spot_ctm": lambda: the_spot(True), "spot_wide": lambda: M.spot_light((1, 1, 1), (0, 0, 0), (0, -1, 0), 80.0, 40.0)}[which]()
    p = contexts(light, 20000, 5)
    e_wi, e_L = mirror_error(light, p)
    b_wi, b_L = bounds_for(light)
    print(which, "wi error %.3g (bound %.3g), L error %.3g (bound %.3g)" % (e_wi.max(), b_wi, e_L.max(), b_L))
    assert e_wi.max() <= b_wi and e_L.max() <= b_L
    if light.kind == M.LIGHT_SPOT:       # the three regimes are all among the contexts
        valid, wi, L, *_ = light.sample_li(p)
        full = np.all(L == (light.I[None, :] / ((light.pos[None, :] - p) ** 2).sum(axis=1, dtype=f32)[:, None]), axis=1)
        assert (~valid).sum() > 1000 and full.sum() > 100 and (valid & ~full).sum() > 100


@pytest.mark.parametrize("planted", M.PLANTED)
def test_planted_errors_break_the_bound(planted):
    """Each planted error puts the mirror outside the bound the honest mirror keeps (a point light has no falloff to get wrong: the
    falloff errors are shown on the spot, the missing 1 / d^2 on both)."""
    lights = [the_spot(True)] + ([M.point_light((3, 2, 1), (0.4, 1.5, -0.3))] if planted == "no_d2" else [])
    for light in lights:
        p = contexts(light, 20000, 6)
        e_wi, e_L = mirror_error(light, p, planted)
        assert e_L.max() > 100 * bounds_for(light)[1], (planted, e_L.max())


def test_smoothstep_known_answers():
    a, b = f32(0.25), f32(0.75)
    x = np.array([a, b, f32(0.5), f32(0.0), f32(1.0), np.nextafter(a, f32(-1)), np.nextafter(b, f32(2))], f32)
    assert M.smooth_step(x, a, b).tolist() == [0.0, 1.0, 0.5, 0.0, 1.0, 0.0, 1.0]
    assert M.smooth_step(np.array([0.2, 0.25, 0.3], f32), a, a).tolist() == [0.0, 1.0, 1.0]      # a == b: the step (math.h:269-270)
    light = the_spot(False)      # ... and through SampleLi: on the cone's rim nothing, on the falloff's inner rim everything
    ce, cs = float(light.cos_end), float(light.cos_start)
    assert light.intensity64(np.array([[math.sqrt(1 - c * c), 0, c] for c in (ce, cs, (ce + cs) / 2, ce - 0.01, 1.0)])).tolist() == [0, 1, 0.5, 0, 1]


def test_spot_phi_is_the_integral_of_its_intensity():
    """Phi = int I(w) dw = 2 pi I int SmoothStep(c) dc over c = cos(theta) in [-1, 1]: the full cone gives (1 - cosStart), and the
    cubic integrates to (cosStart - cosEnd) / 2 exactly -- Gauss-Legendre with 8 nodes is exact for it.  The mirror's Phi has five
    float32 operations on it: 6 EPS relative."""
    for angle, delta in ((30.0, 5.0), (25.0, 8.0), (80.0, 40.0), (10.0, 0.0)):
        light = M.spot_light((3.0, 2.0, 1.0), (0, 0, 0), (0, 0, 1), angle, delta)
        ce, cs = float(light.cos_end), float(light.cos_start)
        x, w = np.polynomial.legendre.leggauss(8)
        c = 0.5 * (cs - ce) * x + 0.5 * (cs + ce)
        band = 0.5 * (cs - ce) * (w * light.intensity64(np.stack([np.sqrt(1 - c * c), 0 * c, c], axis=1))).sum() if cs > ce else 0.0
        assert abs(band - (cs - ce) / 2) <= 1e-15
        want = 2 * math.pi * light.I.astype(np.float64) * ((1 - cs) + band)
        assert np.all(np.abs(light.phi() - want) <= 6 * EPS * want), (angle, delta)
    pl = M.point_light((3.0, 2.0, 1.0), (0, 0, 0))
    assert np.all(np.abs(pl.phi() - 4 * math.pi * pl.I.astype(np.float64)) <= 3 * EPS * 4 * math.pi * pl.I)


def test_light_bounds_contain_every_lit_direction():
    """LightBounds says: no light leaves at more than theta_o + theta_e from w.  10^4 random directions: wherever the spot's I(w) > 0 the
    angle to the axis is within that, and the point light's bound (theta_o = pi) admits every direction."""
    rng = np.random.default_rng(3)
    w = rng.normal(size=(10000, 3))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    for angle, delta in ((30.0, 5.0), (25.0, 8.0), (80.0, 40.0)):
        light = M.spot_light((3.0, 2.0, 1.0), (0, 0, 0), (0.3, -0.5, 0.8), angle, delta)
        p, axis, phi, cos_o, cos_e = light.bounds()
        R = light.mi[:3, :3].astype(np.float64)
        lit = light.intensity64(w @ R.T) > 0
        ang = np.arccos(np.clip(w @ axis.astype(np.float64), -1, 1))
        assert lit.sum() > 50 and np.all(ang[lit] <= math.acos(float(cos_o)) + math.acos(float(cos_e)) + 1e-6)
        assert np.array_equal(p, light.pos) and phi == f32(3.0) * f32(4) * M.PI
    p, axis, phi, cos_o, cos_e = M.point_light((1, 2, 3), (0.5, 0.5, 0.5)).bounds()
    assert math.acos(float(cos_o)) + math.acos(float(cos_e)) >= math.pi and axis.tolist() == [0, 0, 1] and phi == (f32(4) * M.PI) * f32(3)


# ---- 2. the C-ABI additions -----------------------------------------------------------------------------------------------------------
def test_header_declares_the_additions():
    h = open(HEADER).read()
    assert re.search(r"#define VSPG_ABI_VERSION 7\b", h)
    assert re.search(r"enum \{ VSPG_LIGHT_POINT = 3, VSPG_LIGHT_SPOT = 4 \};", h) and re.search(r"#define VSPG_MAX_POINT_LIGHTS 8\b", h)
    for name in ("typedef struct VspgPointLight", "int vspg_spot_light_look_at(", "int vspg_point_light_at(", "int vspg_light_sample_batch(",
                 "int32_t n_point_lights;", "VspgPointLight point_lights[VSPG_MAX_POINT_LIGHTS];"):
        assert name in h, name
    assert h.index("int32_t camera_outside_medium;") < h.index("int32_t n_point_lights;") < h.index("} VspgScene;")     # at the tail


def test_binding_layout_equals_the_headers(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vspg.h"\nint main(void) { printf("%zu %zu %zu %zu %d\\n", '
                   'sizeof(VspgPointLight), sizeof(VspgScene), offsetof(VspgScene, n_point_lights), offsetof(VspgScene, point_lights), '
                   'VSPG_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(pkg.VspgPointLight), C.sizeof(pkg.VspgScene), pkg.VspgScene.n_point_lights.offset, pkg.VspgScene.point_lights.offset, 7]
    assert (pkg.LIGHT_POINT, pkg.LIGHT_SPOT, pkg.VSPG_MAX_POINT_LIGHTS) == (3, 4, 8)
    names = [s[0] for s in pkg.SYMBOLS]
    assert {"vspg_spot_light_look_at", "vspg_point_light_at", "vspg_light_sample_batch"} <= set(names)
    assert pkg.load().vspg_abi_version() == 7


def lit_scene(pkg):
    s = pkg.fog_box_scene(16, 16)
    pkg.add_point_light(s, (1, 1, 1), (0, 0.5, 0))
    pkg.add_spot_light(s, (1, 1, 1), (0, 0.5, 0), (0, 0, 0))
    return s


REFUSALS = [
    ("n_point_lights out of range", lambda s: setattr(s, "n_point_lights", 9)),
    ("n_point_lights out of range", lambda s: setattr(s, "n_point_lights", -1)),
    ("unknown point light type", lambda s: setattr(s.point_lights[0], "type", 2)),
    ("must be affine", lambda s: s.point_lights[0].render_from_light.__setitem__(12, 0.5)),
    ("must be affine", lambda s: s.point_lights[1].light_from_render.__setitem__(15, 2.0)),
    ("renderFromLight is not finite", lambda s: s.point_lights[0].render_from_light.__setitem__(3, float("nan"))),
    ("renderFromLight is not finite", lambda s: s.point_lights[1].light_from_render.__setitem__(0, float("inf"))),
    ("I is not finite", lambda s: s.point_lights[0].I.__setitem__(1, float("nan"))),
    ("I is not finite", lambda s: s.point_lights[1].I.__setitem__(2, float("inf"))),
    ("cone_delta_deg must be >= 0", lambda s: setattr(s.point_lights[1], "cone_delta_deg", -1.0)),
    ("cone_delta_deg exceeds cone_angle_deg", lambda s: setattr(s.point_lights[1], "cone_delta_deg", 31.0)),
    ("cone_angle_deg must be in (0, 180]", lambda s: setattr(s.point_lights[1], "cone_angle_deg", 0.0)),
    ("cone_angle_deg must be in (0, 180]", lambda s: setattr(s.point_lights[1], "cone_angle_deg", 181.0)),
    ("cone_angle_deg must be in (0, 180]", lambda s: setattr(s.point_lights[1], "cone_angle_deg", float("nan"))),
]


@pytest.mark.parametrize("needle,spoil", REFUSALS, ids=[("%02d " % i) + r[0][:24] for i, r in enumerate(REFUSALS)])
def test_create_refuses_bad_point_lights(pkg, needle, spoil):
    """The argument checks come before the device is opened: VSPG_EINVAL with a named message and nothing created, GPU or not."""
    lib = pkg.load()
    s = lit_scene(pkg)
    spoil(s)
    prm, cfg, h = pkg.app_f_params(), pkg.VspgRenderConfig(16, 16, 1, 0, 0, 1, 0), C.c_void_p()
    rc = lib.vspg_renderer_create(C.byref(s), C.byref(prm), C.byref(cfg), C.byref(h))
    assert rc == pkg.VSPG_EINVAL and not h.value and needle in lib.vspg_last_error().decode(), lib.vspg_last_error()


def test_a_point_light_ignores_the_cone_fields(pkg):
    """... which only a spot light reads: garbage there is no reason to refuse a point light (the scene passes validation; without a
    device the call then fails with VSPG_ENODEVICE, with one it succeeds)."""
    lib = pkg.load()
    s = lit_scene(pkg)
    s.point_lights[0].cone_angle_deg, s.point_lights[0].cone_delta_deg = -5.0, 400.0
    prm, cfg, h = pkg.app_f_params(), pkg.VspgRenderConfig(16, 16, 1, 0, 0, 1, 0), C.c_void_p()
    rc = lib.vspg_renderer_create(C.byref(s), C.byref(prm), C.byref(cfg), C.byref(h))
    assert rc in (0, pkg.VSPG_ENODEVICE), lib.vspg_last_error()
    if rc == 0:
        lib.vspg_renderer_destroy(h)


LOOK_AT = [((0, 0, 0), (0, 0, 1)), ((0, 0, 0), (0, 0, -1)), ((1, 2, 3), (1, 2, 3.5)), ((1, 2, 3), (1, 2, -7)),      # along +-z: both branches of copysign
           ((0, 0, 0), (1, 0, 0)), ((0, 1.5, 0), (0, 0, 0)), ((0.5, -0.25, 2), (0.5, 4, 2)),                            # axis-aligned
           ((0.4, 1.5, -0.3), (-0.2, 0.1, 0.6)), ((3, -2, 1), (-1, 0.5, -4)), ((0.1, 0.2, 0.3), (0.1000001, 0.2, 0.9))]  # oblique


@pytest.mark.parametrize("with_ctm", [False, True])
def test_look_at_equals_the_mirror(pkg, with_ctm):
    lib = pkg.load()
    ctm = ctm_oblique() if with_ctm else None
    cp = None if ctm is None else np.ascontiguousarray(ctm.reshape(16)).ctypes.data_as(C.POINTER(C.c_float))
    for fr, to in LOOK_AT:
        l = pkg.VspgPointLight()
        assert lib.vspg_spot_light_look_at(C.byref(l), pkg.f3(*fr), pkg.f3(*to), cp) == 0, lib.vspg_last_error()
        m, mi = M.spot_transform(fr, to, ctm)
        assert np.array_equal(u32(np.array(l.render_from_light[:], f32)), u32(m.reshape(16))), (fr, to, "m")
        assert np.array_equal(u32(np.array(l.light_from_render[:], f32)), u32(mi.reshape(16))), (fr, to, "mInv")
        # what the matrices mean: the light sits at ctm(from) and shines along ctm(to - from)
        c64 = np.eye(4) if ctm is None else ctm.astype(np.float64)
        assert np.allclose(m[:3, 3], (c64 @ np.array([*fr, 1.0]))[:3], atol=1e-5)
        axis = c64[:3, :3] @ (np.subtract(to, fr) / np.linalg.norm(np.subtract(to, fr)))
        assert np.allclose(m[:3, 2], axis, atol=1e-5) and np.allclose(m.astype(np.float64) @ mi.astype(np.float64), np.eye(4), atol=1e-5)
        l = pkg.VspgPointLight()
        assert lib.vspg_point_light_at(C.byref(l), pkg.f3(*fr), cp) == 0
        m, mi = M.point_transform(fr, ctm)
        assert np.array_equal(u32(np.array(l.render_from_light[:], f32)), u32(m.reshape(16))) and np.array_equal(u32(np.array(l.light_from_render[:], f32)), u32(mi.reshape(16)))
    l = pkg.VspgPointLight()
    assert lib.vspg_spot_light_look_at(C.byref(l), pkg.f3(1, 2, 3), pkg.f3(1, 2, 3), cp) == pkg.VSPG_EINVAL and b"from == to" in lib.vspg_last_error()
    bad = (C.c_float * 16)(*([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0.5, 1]))
    assert lib.vspg_point_light_at(C.byref(l), pkg.f3(1, 2, 3), bad) == pkg.VSPG_EINVAL


def test_binding_helpers_fill_the_record(pkg):
    s = pkg.fog_box_scene(16, 16)
    assert pkg.add_point_light(s, (2, 4, 8), (1, 2, 3), scale=0.5, power=10.0) == 0
    assert pkg.add_spot_light(s, (3, 2, 1), (0, 1.5, 0), (0, 0, 0), coneangle=25, conedelta=8, scale=2.0, ctm=ctm_oblique()) == 1
    want = M.point_light((2, 4, 8), (1, 2, 3), scale=0.5, power=10.0)
    p, q = s.point_lights[0], s.point_lights[1]
    assert s.n_point_lights == 2 and p.type == pkg.LIGHT_POINT and q.type == pkg.LIGHT_SPOT
    assert np.array_equal(u32(np.array(p.I[:], f32)), u32(want.I)) and np.array_equal(u32(np.array(p.render_from_light[:], f32)), u32(want.m.reshape(16)))
    want = M.spot_light((3, 2, 1), (0, 1.5, 0), (0, 0, 0), 25, 8, scale=2.0, ctm=ctm_oblique())
    assert np.array_equal(u32(np.array(q.I[:], f32)), u32(want.I)) and (q.cone_angle_deg, q.cone_delta_deg) == (25.0, 8.0)
    assert np.array_equal(u32(np.array(q.light_from_render[:], f32)), u32(want.mi.reshape(16)))
    # "power": the light's Phi becomes the requested one (lights.cpp:234-238, :1540-1547), to the rounding of its handful of operations
    s2 = pkg.fog_box_scene(16, 16)
    pkg.add_spot_light(s2, (1, 1, 1), (0, 0, 0), (0, 0, 1), coneangle=40, conedelta=10, power=7.0)
    l = M.Light(M.LIGHT_SPOT, np.array(s2.point_lights[0].I[:], f32), np.eye(4), np.eye(4), 40, 10)
    assert np.all(np.abs(l.phi() - 7.0) <= 7.0 * 16 * EPS)


# ---- 3. scene files ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vspg_pbrt():
    exe = os.path.join(HOST, "vspg_pbrt")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "vspg-pbrt-v4_amd", "csrc"), "libvspg_hip.so"])
        subprocess.check_call(["make", "-C", HOST])
    return exe


POINT_SCENE = '''LookAt 0 0 -3  0 0 0  0 1 0
Camera "perspective" "float fov" 40
Sampler "independent" "integer pixelsamples" 2
Film "rgb" "integer xresolution" 32 "integer yresolution" 24 "string filename" "%(out)s"
Integrator "guidedvolpathvspg" "integer maxdepth" 3 "bool surfaceguiding" false "bool volumeguiding" false "bool vspguiding" false
WorldBegin
MakeNamedMedium "fog" "string type" "homogeneous" "rgb sigma_a" [ .05 .05 .05 ] "rgb sigma_s" [ .4 .4 .4 ] "float g" 0.3
MediumInterface "fog" "fog"
AttributeBegin
  Translate 0.3 -0.2 0.5
  Rotate 37 1 2 3
  LightSource "point" "rgb I" [ 2 4 8 ] "float scale" 0.5 "float power" 10 "point3 from" [ 0.25 1.0 -0.5 ]%(extra)s
AttributeEnd
Material "diffuse" "rgb reflectance" [ .5 .25 .75 ]
Shape "bilinearmesh" "point3 P" [ -4 -1 -4  4 -1 -4  -4 -1 4  4 -1 4 ]
'''


def test_scene_file_point_light(vspg_pbrt, tmp_path):
    (tmp_path / "scene.pbrt").write_text(POINT_SCENE % {"out": "x.pfm", "extra": ""})
    r = subprocess.run([vspg_pbrt, str(tmp_path / "scene.pbrt"), "--parse-only"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    want = M.point_light((2, 4, 8), (0.25, 1.0, -0.5), scale=0.5, power=10.0, ctm=ctm_oblique())
    m = re.search(r"point light 0: type 3 at \((\S+), (\S+), (\S+)\) I \((\S+), (\S+), (\S+)\)", r.stdout)
    assert m, r.stdout
    got = np.array([float(v) for v in m.groups()], f32)
    assert np.array_equal(u32(got[:3]), u32(want.pos)) and np.array_equal(u32(got[3:]), u32(want.I)), (got, want.pos, want.I)
    assert "1 rectangles, 0 triangles, 0 infinite lights" in r.stdout
    (tmp_path / "bad.pbrt").write_text(POINT_SCENE % {"out": "x.pfm", "extra": ' "float bogus" 1'})
    r = subprocess.run([vspg_pbrt, str(tmp_path / "bad.pbrt"), "--parse-only"], capture_output=True, text=True)
    assert r.returncode != 0 and "bogus" in r.stderr, r.stdout + r.stderr
    (tmp_path / "spot.pbrt").write_text(POINT_SCENE.replace('LightSource "point"', 'LightSource "spot"') % {"out": "x.pfm", "extra": ""})
    r = subprocess.run([vspg_pbrt, str(tmp_path / "spot.pbrt"), "--parse-only"], capture_output=True, text=True)
    assert r.returncode != 0 and 'LightSource "spot"' in r.stderr and "vspg_spot_light_look_at" in r.stderr, r.stdout + r.stderr


# ---- 4. the conditions the statistical test of a spot in fog rests on (tests/test_pointlight_gpu.py) ---------------------------------
@pytest.fixture(scope="module")
def fog():
    F = M.FogSpot()
    coarse, fine = F.quadrant_means(F.pixel_means(4, 256)), F.quadrant_means(F.pixel_means(8, 512))
    mc = F.monte_carlo_waves(F.WAVES, seed=1)
    return F, coarse, fine, mc.mean(axis=0), mc.std(axis=0, ddof=1) / math.sqrt(F.WAVES)


def test_fog_model_quadrature_is_finer_than_the_statistic(fog):
    """Halving both step sizes moves no quadrant mean by a tenth of the standard error a 32-wave run has (sized by a NumPy Monte Carlo
    of the same estimator), and that Monte Carlo agrees with the quadrature itself."""
    F, coarse, fine, mc_mean, se = fog
    print("quadrant means", fine, "standard errors", se, "step-halving moves them by", np.abs(coarse - fine))
    assert np.all(fine > 0) and np.all(np.abs(coarse - fine) < 0.1 * se)
    assert np.all(np.abs(mc_mean - fine) <= 4.5 * se)


@pytest.mark.parametrize("planted", M.PLANTED)
def test_fog_statistic_sees_each_planted_error(fog, planted):
    """Each planted error moves some quadrant mean by more than ten standard errors of a 32-wave run, the standard error sized by the
    model's Monte Carlo.  Measured with this view: swapped cosines 15 558, wi for -wi and m for mInv 31.4, a linear falloff 14.5
    (the right-hand quadrants, which see the band's outer half alone), no 1 / d^2 278.  (The renderer's own spread over its 32 waves came
    out 1.4 to 2.5 times the model's -- it decides scattering with the VSP machinery, the model by plain free flight --, at which the
    linear falloff still sits 10 of the renderer's standard errors out.)"""
    F, coarse, fine, mc_mean, se = fog
    z = (F.quadrant_means(F.pixel_means(4, 256, planted=planted)) - coarse) / se
    print(planted, "moves the quadrant means by", z, "standard errors")
    assert np.abs(z).max() > 10


def test_fog_camera_rays_keep_away_from_the_light(fog):
    F = fog[0]
    assert F.min_distance_to_light() >= 0.5
    d = F.rays(np.array([0.0, F.W, 0.0, F.W]), np.array([0.0, 0.0, F.H, F.H]))      # the film's corners end on the backdrop quad
    hit = F.cam[0] + d * F.t_wall(d)[:, None]
    assert np.all(np.abs(hit[:, :2]) < 6.0)
