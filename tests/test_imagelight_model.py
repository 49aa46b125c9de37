"""Projection and goniometric lights on the CPU: the float32 mirror of tests/imagelight_model.py against its float64 statement, known
answers worked out by hand, five planted errors, the C-ABI additions (record layout, refusals, the two transform helpers bit for bit),
and the host's table builder under sanitizers (tests/imagelight_build_check.cpp, a stand-alone program fed with the model's bytes)."""
import ctypes as C
import math
import os
import shlex
import struct
import subprocess

import numpy as np
import pytest

import imagelight_model as M
import pointlight_model as PM
from conftest import ROOT

f32 = np.float32
EPS = 2.0 ** -24          # half an ulp of 1: the relative error of one float32 operation
HEADER = os.path.join(ROOT, "include", "vspg.h")
CSRC = os.path.join(ROOT, "vspg-pbrt-v4_amd", "csrc")
CAP = 0.01                # at most 1 % of a fixture's contexts may show another texel in float32 than in float64


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ctm_oblique():
    return PM.mat4_mul(PM.translate((0.3, -0.2, 0.5)), PM.rotate(37.0, (1, 2, 3)))


FIXTURES = {
    "slide 8x6": lambda: M.projection_light((3, 2, 1), M.slide(8, 6, 1), fov=70.0, ctm=ctm_oblique()),
    "slide 6x8": lambda: M.projection_light((1, 2, 3), M.slide(6, 8, 2), fov=40.0, ctm=ctm_oblique()),
    "slide 1x1": lambda: M.projection_light((1, 1, 1), np.ones((1, 1, 3), f32), fov=90.0, ctm=ctm_oblique()),
    "map 5x5": lambda: M.goniometric_light((3, 2, 1), M.gonio_map(5, 3), ctm=ctm_oblique()),
    "map 64x64": lambda: M.goniometric_light((1, 2, 3), M.gonio_map(64, 4), scale=0.5, ctm=ctm_oblique()),
}


# ---- 1. the mirror against the float64 statement -------------------------------------------------------------------------------------
def mirror_error(light, p, planted=None):
    """Per context: max |wi - wi64|; max |L - L64| over the channels relative to I * max texel / d^2; and whether float32 and float64
    name another texel (or disagree on whether there is one)."""
    valid, wi, L, pdf, pl, delta = light.sample_li(p, planted)
    wi64, L64 = light.sample_li64(p)
    in32, ix, iy, *_ = light.texel_index(p, planted)
    in64, jx, jy = light.texel_index64(p)
    other = (in32 != in64) | (in32 & ((ix != jx) | (iy != jy)))
    d2 = ((light.pos.astype(np.float64) - p.astype(np.float64)) ** 2).sum(axis=1)
    scale = light.I.astype(np.float64)[None, :] * float(np.abs(light.texels).max()) / d2[:, None]
    return np.abs(wi - wi64).max(axis=1), (np.abs(np.where(valid[:, None], L, 0) - L64) / scale).max(axis=1), other


@pytest.mark.parametrize("which", list(FIXTURES))
def test_mirror_agrees_with_the_float64_statement(which):
    """Where both name the same texel, the error is a point light's (tests/test_pointlight_model.py: bounds_for) plus one product:
      wi = d / |d|                6 EPS absolute
      L = (I * texel) / |d|^2     1 (the product) + 5 (|d|^2) + 1 (the quotient) = 7 EPS relative -> 8 EPS of I * max texel / |d|^2
    Contexts whose texel differs between float32 and float64 sit within rounding of a texel or screen edge; the fixture puts an eighth
    (224 of 4096 contexts per edge regime) within 1e-6 of one on purpose, of which about 1e-7 / 1e-6 ~ a tenth can
    flip: they are set aside, and may be at most 1 % of the fixture (the GPU test's contexts are these)."""
    light = FIXTURES[which]()
    p, nn, u, labels = M.contexts_around(light, 4096, 21)
    e_wi, e_L, other = mirror_error(light, p)
    print(which, "wi error %.3g EPS, L error %.3g EPS, other texel %d of %d" % (e_wi.max() / EPS, e_L[~other].max() / EPS, other.sum(), len(p)))
    assert other.mean() <= CAP
    assert e_wi.max() <= 6 * EPS and e_L[~other].max() <= 8 * EPS
    counts = np.bincount(labels, minlength=8)
    if light.kind == M.LIGHT_PROJECTION:      # every regime is there, as the GPU test asserts of the same contexts
        assert np.all(counts > 200), counts
        valid = light.sample_li(p)[0]
        if which != "slide 1x1":
            assert valid[labels == 0].mean() > 0.9 and not valid[(labels >= 1) & (labels <= 4)].any()
        assert valid[labels == 5].sum() == 0
    else:
        assert counts[0] > 200 and counts[6] > 200
    dist = np.linalg.norm(p.astype(np.float64) - light.pos, axis=1)
    assert (dist < 2e-3).sum() > 200 and (dist > 500).sum() > 200


def test_known_answers_of_a_2x2_slide():
    """fov 90 (tan 45 degrees = 1: the screen window [-1, 1]^2 is the plane z = 1), the light at the origin under no CTM: renderFromLight =
    Scale(1, -1, 1), so a point (x, y, z) lies at screen (x / z, -y / z) and the slide's TOP row (v < 0.5) shows upwards."""
    img = np.array([[[1, 0, 0], [0, 1, 0]], [[0, 0, 1], [1, 1, 0]]], f32)      # top: red, green; bottom: blue, yellow
    light = M.projection_light((2, 2, 2), img, fov=90.0)
    assert light.persp.inv_tan == 1 and light.sb.tolist() == [-1, -1, 1, 1] and light.A == 4
    p = np.array([[-0.5, 0.5, 1], [0.5, 0.5, 1], [-0.5, -0.5, 1], [0.5, -0.5, 1]], f32) * f32(2)
    valid, wi, L, pdf, pl, delta = light.sample_li(p)
    d2 = f32(6)      # |2 * (0.5, 0.5, 1)|^2
    assert valid.all() and np.array_equal(L, f32(2) * img.reshape(4, 3) / d2) and np.all(pdf == 1) and np.all(pl == 0)
    # the screen edge is inclusive and shows the last texel; one float further out there is no light
    edge = np.array([[1, 0.25, 1], [np.nextafter(f32(1), f32(2)), 0.25, 1], [-1, -1, 1], [0.25, np.nextafter(f32(-1), f32(-2)), 1]], f32)
    valid, wi, L, *_ = light.sample_li(edge)
    inside, ix, iy, *_ = light.texel_index(edge)
    # (the direction is normalised and projected again: the point on the edge must come back as exactly 1 for this to say anything)
    wl = light.texel_index(edge)[3]
    assert (wl[0, 0] / wl[0, 2] == 1) and valid.tolist()[0] and (ix[0], iy[0]) == (1, 0)
    assert valid.tolist() == [True, False, True, False] and (ix[2], iy[2]) == (0, 1)
    # behind the light: nothing (without the hither test the slide would show mirrored through the origin)
    behind = np.array([[0.5, 0.5, -1], [0, 0, -3]], f32)
    assert not light.sample_li(behind)[0].any() and light.sample_li(behind, "no_hither")[0].all()
    # wl.z on either side of hither: under a uniform scale s of the CTM wl = -wi / s is not a unit vector.  1 / 1000 rounds to hither
    # itself (not below it: lit); 1 / 1001 lies below (dark)
    axis = np.array([[0, 0, 5]], f32)
    for s, lit in ((1000.0, True), (1001.0, False), (999.0, True)):
        l2 = M.projection_light((1, 1, 1), img, fov=90.0, ctm=np.diag([s, s, s, 1]).astype(f32))
        assert l2.texel_index(axis)[3][0, 2] == f32(1 / s)
        assert bool(l2.sample_li(axis)[0][0]) is lit, s


def test_screen_window_and_area_of_both_aspects():
    wide = M.projection_light((1, 1, 1), M.slide(8, 6), fov=90.0)
    a = f32(8) / f32(6)
    assert wide.sb.tolist() == [-a, -1, a, 1] and wide.A == f32(4) * a
    tall = M.projection_light((1, 1, 1), M.slide(6, 8), fov=90.0)
    a = f32(6) / f32(8)
    assert a == 0.75 and tall.sb.tolist() == [-1, f32(-1) / a, 1, f32(1) / a] and tall.A == f32(4) * (f32(1) / a)
    narrow = M.projection_light((1, 1, 1), M.slide(4, 4), fov=60.0)
    assert abs(float(narrow.A) - 4 * math.tan(math.radians(30)) ** 2) <= 8 * EPS * float(narrow.A) and narrow.sb.tolist() == [-1, -1, 1, 1]
    # the slide's corner texel is reached through the window's corner, whatever the aspect
    for light in (wide, tall):
        t = 1.0 / math.tan(math.radians(45))
        c = np.array([[light.sb[2] * 0.999 / t, -light.sb[3] * 0.999 / t, 1.0]], f32)      # (+x, +y on the screen = -y in render space)
        inside, ix, iy, *_ = light.texel_index(c)
        assert inside[0] and (ix[0], iy[0]) == (light.xres - 1, light.yres - 1)


def test_goniometric_light_with_the_1x1_image_is_a_point_light():
    """Bit for bit: SampleLi's rows, Phi and the LightBounds, under a CTM (I * 1 / d^2 = I / d^2; I * 4 * Pi * 1 / 1 = 4 Pi I)."""
    ctm = ctm_oblique()
    g = M.goniometric_light((3, 2, 1), None, scale=0.5, power=7.0, ctm=ctm)
    pt = PM.point_light((3, 2, 1), (0, 0, 0), scale=0.5, power=7.0, ctm=ctm)
    assert np.array_equal(u32(g.I), u32(pt.I)) and np.array_equal(u32(g.pos), u32(pt.pos))
    p, *_ = M.contexts_around(g, 2048, 5)
    for a, b in zip(g.sample_li(p), pt.sample_li(p)):
        assert np.array_equal(u32(np.asarray(a, f32)), u32(np.asarray(b, f32)))
    assert np.array_equal(u32(g.phi()), u32(pt.phi()))
    for a, b in zip(g.bounds(), pt.bounds()):
        assert np.array_equal(u32(np.asarray(a, f32)), u32(np.asarray(b, f32)))


def test_known_answers_of_a_goniometric_map():
    """No CTM: renderFromLight = swapYZ, so a context at p sees the map's direction (p.x, p.z, p.y) / |p|: render +y is the map's pole.
    On the diagonals |x| = |y| the mapping's angle is a half, so with r = sqrt(1 - 1 / sqrt 3) = 0.650 the octant (+, +, +) lies at
    uv = 0.5 + r / 4 = 0.6625 in both, (-, -, +) at 0.3375, (+, -, +) at (0.6625, 0.3375) and the southern (+, +, -) at 0.5 + (1 - r / 2) / 2
    = 0.8375: texels 2, 1, (2, 1) and 3 of a 4 x 4 map.  Straight above the light (the pole) is the map's centre, uv = 0.5: texel (2, 2)."""
    img = M.gonio_map(4, 7)
    light = M.goniometric_light((1, 1, 1), img)
    p = np.array([[2, 2, 2], [-2, 2, -2], [2, 2, -2], [2, -2, 2], [0, 3, 0]], f32)
    inside, ix, iy, *_ = light.texel_index(p)
    assert list(zip(ix.tolist(), iy.tolist())) == [(2, 2), (1, 1), (2, 1), (3, 3), (2, 2)]
    L = light.sample_li(p)[2]
    assert np.array_equal(L[:, 0], np.array([img[2, 2], img[1, 1], img[1, 2], img[3, 3], img[2, 2]], f32) / np.array([12, 12, 12, 12, 9], f32))
    # a negative texel stays negative (no ClampZero in GoniometricLight::I) and the sample is still returned
    neg = M.goniometric_light((1, 1, 1), -img)
    valid, wi, L2, *_ = neg.sample_li(p)
    assert valid.all() and np.array_equal(L2, -L)


def test_phi_of_a_uniform_slide_is_the_solid_angle_of_its_beam():
    """Phi = I * int cos^3(theta) dA over the screen window on the plane z = 1 = I * the beam's solid angle, 4 atan(a b / sqrt(1 + a^2 +
    b^2)) for half extents a, b; a float64 quadrature of cos^3 agrees with that closed form to 1e-9.  The mirror's Phi is the midpoint
    rule at the slide's resolution, h = 2 a / xres: its error is at most area * h^2 / 24 * (|f_xx| + |f_yy|) with |f_xx| <= 3 for f =
    (1 + x^2 + y^2)^(-3/2), and its xres * yres sequential float32 additions add at most xres * yres * EPS relative."""
    for (xres, yres, fov) in ((64, 64, 90.0), (48, 64, 60.0), (64, 32, 100.0)):
        light = M.projection_light((3, 2, 1), np.ones((yres, xres, 3), f32), fov=fov)
        a, b = float(light.sb[2]) * math.tan(math.radians(fov) / 2), float(light.sb[3]) * math.tan(math.radians(fov) / 2)
        omega = 4 * math.atan(a * b / math.sqrt(1 + a * a + b * b))
        n = 2000
        x, y = ((np.arange(n) + 0.5) / n * 2 - 1) * a, ((np.arange(n) + 0.5) / n * 2 - 1) * b
        quad = ((1 + x[None, :] ** 2 + y[:, None] ** 2) ** -1.5).sum() * (2 * a / n) * (2 * b / n)
        assert abs(quad - omega) <= 1e-6 * omega
        h2 = max(2 * a / xres, 2 * b / yres) ** 2
        bound = 4 * a * b * h2 / 24 * 6 + (xres * yres + 8) * EPS * omega
        got = light.phi().astype(np.float64) / light.I
        print(xres, yres, fov, "solid angle %.6f, mirror %.6f, bound %.2g" % (omega, got[0], bound))
        assert np.all(np.abs(got - omega) <= bound)
    g = M.goniometric_light((3, 2, 1), np.full((8, 8), 0.25, f32))
    assert np.all(np.abs(g.phi() - math.pi * g.I.astype(np.float64)) <= 70 * EPS * math.pi * g.I)


@pytest.mark.parametrize("which", ["slide 8x6", "slide 6x8", "slide 1x1"])
def test_light_bounds_contain_every_lit_direction(which):
    """LightBounds says: no light leaves at more than theta_o + theta_e from w, here theta_o = 0 and theta_e the angle of the window's
    corner.  Wherever the slide lights a context, the direction to it is within that (to 1e-6 radians of rounding)."""
    light = FIXTURES[which]()
    p, *_ = M.contexts_around(light, 4096, 9)
    valid = light.sample_li(p)[0]
    pos, w, phi, cos_o, cos_e = light.bounds()
    d = p[valid].astype(np.float64) - pos
    ang = np.arccos(np.clip((d / np.linalg.norm(d, axis=1, keepdims=True)) @ w.astype(np.float64), -1, 1))
    assert valid.sum() > 500 and cos_o == 1 and np.all(ang <= math.acos(float(cos_e)) + 1e-6)
    assert ang.max() > 0.9 * math.acos(float(cos_e))      # (the cone is no wider than it must be: contexts reach its rim)
    raw = light.raw.reshape(-1, 3).max(axis=1).astype(np.float64).sum() / (light.xres * light.yres)
    assert abs(float(phi) - float(max(light.I)) * raw) <= (light.xres * light.yres + 4) * EPS * abs(float(phi))
    # the goniometric light is bounded as an isotropic point light: every direction is admitted
    g = FIXTURES["map 5x5"]()
    pos, w, phi, cos_o, cos_e = g.bounds()
    assert math.acos(float(cos_o)) + math.acos(float(cos_e)) >= math.pi and w.tolist() == [0, 0, 1]


# ---- 2. five planted errors ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planted", M.PLANTED)
def test_planted_errors_are_caught(planted):
    """Each planted error leaves the bound the honest mirror keeps on far more contexts than the 1 % that may be set aside."""
    if planted == "octa":
        # the octahedral wrap differs from the clamp where an index leaves the image, u * res == res: the southern pole, where r = sqrt(1 -
        # |z|) is 0 and u = v = 1 - 0.  Contexts straight below the light (the map's -z is render -y), a hair into the octant (+, +) so
        # that no sign of a zero decides: the clamp shows the corner texel (3, 3), the wrap would mirror twice and show (0, 1).
        light = M.goniometric_light((1, 1, 1), M.gonio_map(4, 7))
        r = np.array([0.25, 0.5, 1, 2, 4, 8], f32)
        p = np.stack([r * f32(1e-6), -r, r * f32(1e-6)], axis=1).astype(f32)
        inside, ix, iy, *_ = light.texel_index(p)
        assert np.all(ix == 3) and np.all(iy == 3)
        inside, ix, iy, *_ = light.texel_index(p, planted)
        assert np.all(ix == 0) and np.all(iy == 1)
        honest, wrong = light.sample_li(p)[2], light.sample_li(p, planted)[2]
        assert np.all(honest != wrong) and np.array_equal(honest[:, 0], light.texels[3, 3] / (r * r))
        return
    light = FIXTURES["map 64x64" if planted == "round" else "slide 8x6"]()
    p, *_ = M.contexts_around(light, 4096, 21)
    e_wi, e_L, other = mirror_error(light, p, planted)
    lit = light.sample_li(p)[0] | light.sample_li(p, planted)[0]
    off = (e_L > 8 * EPS) & lit
    print(planted, "outside the bound: %d of %d lit contexts" % (off.sum(), lit.sum()))
    assert off.sum() > 5 * CAP * len(p)
    if planted == "round":      # ... and on the slide as well
        light = FIXTURES["slide 8x6"]()
        p, *_ = M.contexts_around(light, 4096, 21)
        assert (mirror_error(light, p, planted)[1] > 8 * EPS).sum() > 5 * CAP * len(p)


# ---- 3. the C-ABI additions -----------------------------------------------------------------------------------------------------------
SCENE_FIELDS = ["n_quads", "quads", "camera", "medium", "n_triangles", "tri_p", "tri_kd", "n_infinite_lights", "infinite_lights", "tri_flags",
                "n_spheres", "spheres", "camera_outside_medium", "n_point_lights", "point_lights", "sphere_Le", "sphere_two_sided",
                "rgb_sigma_a", "rgb_sigma_s", "rgb_Le", "rgb_sigma_scale", "rgb_le_scale"]
POINT_LIGHT_FIELDS = ["type", "I", "render_from_light", "light_from_render", "cone_angle_deg", "cone_delta_deg"]


def test_binding_layout_equals_the_headers(pkg, tmp_path):
    """A C program compiled with the header prints every field's offset: the binding's are the same, and the records keep the sizes
    they had -- a projection light's field of view travels in its slot's cone_angle_deg, so VspgScene gained no field and nothing
    moved (4392 bytes, the size tests/test_rgbgrid_model.py pins; VspgPointLight 152)."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vspg.h"\nint main(void) {\n'
                   + "".join('  printf("%%zu\\n", offsetof(VspgScene, %s));\n' % f for f in SCENE_FIELDS)
                   + "".join('  printf("%%zu\\n", offsetof(VspgPointLight, %s));\n' % f for f in POINT_LIGHT_FIELDS)
                   + '  printf("%zu %zu %d %d %d %d\\n", sizeof(VspgScene), sizeof(VspgPointLight), VSPG_ABI_VERSION, VSPG_LIGHT_PROJECTION, '
                     'VSPG_LIGHT_GONIOMETRIC, VSPG_LIGHT_IMAGE_MAX_RES);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    n = len(SCENE_FIELDS)
    offs, ploffs, (size, plsize, abi, proj, gonio, maxres) = got[:n], got[n:n + len(POINT_LIGHT_FIELDS)], got[n + len(POINT_LIGHT_FIELDS):]
    assert offs == [getattr(pkg.VspgScene, f).offset for f in SCENE_FIELDS]
    assert [f[0] for f in pkg.VspgScene._fields_] == SCENE_FIELDS and [f[0] for f in pkg.VspgPointLight._fields_] == POINT_LIGHT_FIELDS
    assert ploffs == [getattr(pkg.VspgPointLight, f).offset for f in POINT_LIGHT_FIELDS] == [0, 4, 16, 80, 144, 148]
    assert size == C.sizeof(pkg.VspgScene) == 4392 and plsize == C.sizeof(pkg.VspgPointLight) == 4 + 12 + 64 + 64 + 8
    assert offs[-1] + 4 == size      # rgb_le_scale is still the record's last field
    assert (abi, proj, gonio, maxres) == (7, pkg.LIGHT_PROJECTION, pkg.LIGHT_GONIOMETRIC, pkg.LIGHT_IMAGE_MAX_RES) == (7, 5, 6, 4096)
    names = [s[0] for s in pkg.SYMBOLS]
    assert {"vspg_projection_light_at", "vspg_goniometric_light_at", "vspg_renderer_set_light_image"} <= set(names)
    assert pkg.load().vspg_abi_version() == 7


def lit_scene(pkg):
    s = pkg.fog_box_scene(16, 16)
    pkg.add_projection_light(s, (1, 1, 1), fov=60, ctm=PM.translate((0, 0.5, 0)))
    pkg.add_goniometric_light(s, (1, 1, 1), ctm=ctm_oblique())
    return s


def skew(s):
    s.point_lights[1].light_from_render[0] = s.point_lights[1].light_from_render[0] + 0.01


REFUSALS = [
    ("field of view (cone_angle_deg) must be in (0, 180)", "EINVAL", lambda s: setattr(s.point_lights[0], "cone_angle_deg", 0.0)),
    ("field of view (cone_angle_deg) must be in (0, 180)", "EINVAL", lambda s: setattr(s.point_lights[0], "cone_angle_deg", 180.0)),
    ("field of view (cone_angle_deg) must be in (0, 180)", "EINVAL", lambda s: setattr(s.point_lights[0], "cone_angle_deg", float("nan"))),
    ("field of view (cone_angle_deg) must be in (0, 180)", "EINVAL", lambda s: setattr(s.point_lights[0], "cone_angle_deg", -45.0)),
    ("must be orthonormal", "ESCOPE", skew),
    ("must be orthonormal", "ESCOPE", lambda s: [s.point_lights[1].light_from_render.__setitem__(k, 2 * s.point_lights[1].light_from_render[k]) for k in range(12)]),
    ("unknown point light type", "EINVAL", lambda s: setattr(s.point_lights[0], "type", 7)),
    ("I is not finite", "EINVAL", lambda s: s.point_lights[0].I.__setitem__(1, float("nan"))),
    ("must be affine", "EINVAL", lambda s: s.point_lights[1].render_from_light.__setitem__(12, 0.5)),
]


@pytest.mark.parametrize("needle,code,spoil", REFUSALS, ids=[("%02d " % i) + r[0][:24] for i, r in enumerate(REFUSALS)])
def test_create_refuses_bad_image_lights(pkg, needle, code, spoil):
    """The argument checks come before the device is opened: a named message and nothing created, GPU or not."""
    lib = pkg.load()
    s = lit_scene(pkg)
    spoil(s)
    prm, cfg, h = pkg.app_f_params(), pkg.VspgRenderConfig(16, 16, 1, 0, 0, 1, 0), C.c_void_p()
    rc = lib.vspg_renderer_create(C.byref(s), C.byref(prm), C.byref(cfg), C.byref(h))
    assert rc == getattr(pkg, "VSPG_" + code) and not h.value and needle in lib.vspg_last_error().decode(), lib.vspg_last_error()


def test_valid_image_lights_pass_validation(pkg):
    """... and the untouched scene passes it (without a device the call then fails with VSPG_ENODEVICE); a goniometric slot's cone fields and a
    projection slot's cone_delta_deg are read by nothing."""
    lib = pkg.load()
    s = lit_scene(pkg)
    s.point_lights[1].cone_angle_deg = s.point_lights[1].cone_delta_deg = float("nan")
    s.point_lights[0].cone_delta_deg = -5.0
    prm, cfg, h = pkg.app_f_params(), pkg.VspgRenderConfig(16, 16, 1, 0, 0, 1, 0), C.c_void_p()
    rc = lib.vspg_renderer_create(C.byref(s), C.byref(prm), C.byref(cfg), C.byref(h))
    assert rc in (0, pkg.VSPG_ENODEVICE), lib.vspg_last_error()
    if rc == 0:
        lib.vspg_renderer_destroy(h)


@pytest.mark.parametrize("with_ctm", [False, True])
def test_transform_helpers_equal_the_mirror(pkg, with_ctm):
    lib = pkg.load()
    ctm = ctm_oblique() if with_ctm else None
    cp = None if ctm is None else np.ascontiguousarray(ctm.reshape(16)).ctypes.data_as(C.POINTER(C.c_float))
    for fn, mirror in ((lib.vspg_projection_light_at, M.projection_transform), (lib.vspg_goniometric_light_at, M.goniometric_transform)):
        l = pkg.VspgPointLight()
        assert fn(C.byref(l), cp) == 0, lib.vspg_last_error()
        m, mi = mirror(ctm)
        assert np.array_equal(u32(np.array(l.render_from_light[:], f32)), u32(m.reshape(16)))
        assert np.array_equal(u32(np.array(l.light_from_render[:], f32)), u32(mi.reshape(16)))
        assert np.allclose(m.astype(np.float64) @ mi.astype(np.float64), np.eye(4), atol=1e-6)
        assert fn(None, cp) == pkg.VSPG_EINVAL
        bad = (C.c_float * 16)(*([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0.5, 1]))
        assert fn(C.byref(l), bad) == pkg.VSPG_EINVAL
    # what they mean: the projector's image is upright (+y of the slide's frame is render -y), the map's pole is render +y
    m, _ = M.projection_transform(None)
    assert m[1, 1] == -1 and m[0, 0] == m[2, 2] == 1
    m, _ = M.goniometric_transform(None)
    assert (m[:3, :3] @ np.array([0, 0, 1], f32)).tolist() == [0, 1, 0]


def test_binding_helpers_fill_the_record(pkg):
    s = pkg.fog_box_scene(16, 16)
    assert pkg.add_projection_light(s, (2, 4, 8), fov=55, ctm=ctm_oblique()) == 0
    img = M.gonio_map(4, 1)
    assert pkg.add_goniometric_light(s, (3, 2, 1), scale=0.5, power=7.0, ctm=ctm_oblique(), image=img) == 1
    assert pkg.add_goniometric_light(s, (3, 2, 1), scale=0.5, power=7.0) == 2
    p, q, r = s.point_lights[0], s.point_lights[1], s.point_lights[2]
    assert s.n_point_lights == 3 and (p.type, q.type, r.type) == (pkg.LIGHT_PROJECTION, pkg.LIGHT_GONIOMETRIC, pkg.LIGHT_GONIOMETRIC)
    assert p.cone_angle_deg == 55 and q.cone_angle_deg == 0      # a projection slot's field of view
    want = M.projection_light((2, 4, 8), np.ones((1, 1, 3), f32), 55, ctm_oblique())
    assert np.array_equal(u32(np.array(p.I[:], f32)), u32(want.I)) and np.array_equal(u32(np.array(p.light_from_render[:], f32)), u32(want.mi.reshape(16)))
    want = M.goniometric_light((3, 2, 1), img, scale=0.5, power=7.0, ctm=ctm_oblique())
    assert np.array_equal(u32(np.array(q.I[:], f32)), u32(want.I)) and np.array_equal(u32(np.array(q.render_from_light[:], f32)), u32(want.m.reshape(16)))
    # "power": Phi of a grey light becomes the requested one (lights.cpp:714-722), to the rounding of its handful of operations and sums
    s2 = pkg.fog_box_scene(16, 16)
    pkg.add_goniometric_light(s2, (1, 1, 1), power=7.0, image=img)
    l = M.ImageLight(M.LIGHT_GONIOMETRIC, np.array(s2.point_lights[0].I[:], f32), np.eye(4), np.eye(4), img)
    assert np.all(np.abs(l.phi() - 7.0) <= 7.0 * 24 * EPS)
    want = M.goniometric_light((3, 2, 1), None, scale=0.5, power=7.0)
    assert np.array_equal(u32(np.array(r.I[:], f32)), u32(want.I))


# ---- 3b. scene files ----------------------------------------------------------------------------------------------------------------
HOST = os.path.join(ROOT, "vspg-pbrt-v4_amd", "host")


@pytest.fixture(scope="module")
def vspg_pbrt():
    exe = os.path.join(HOST, "vspg_pbrt")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", CSRC, "libvspg_hip.so"])
        subprocess.check_call(["make", "-C", HOST])
    return exe


LIGHT_SCENE = '''LookAt 0 0 -3  0 0 0  0 1 0
Camera "perspective" "float fov" 40
Sampler "independent" "integer pixelsamples" 2
Film "rgb" "integer xresolution" 32 "integer yresolution" 24 "string filename" "x.pfm"
Integrator "guidedvolpathvspg" "integer maxdepth" 3 "bool surfaceguiding" false "bool volumeguiding" false "bool vspguiding" false
WorldBegin
MakeNamedMedium "fog" "string type" "homogeneous" "rgb sigma_a" [ .05 .05 .05 ] "rgb sigma_s" [ .4 .4 .4 ] "float g" 0.3
MediumInterface "fog" "fog"
AttributeBegin
  Translate 0.3 -0.2 0.5
  Rotate 37 1 2 3
  %(lights)s
AttributeEnd
Material "diffuse" "rgb reflectance" [ .5 .25 .75 ]
Shape "bilinearmesh" "point3 P" [ -4 -1 -4  4 -1 -4  -4 -1 4  4 -1 4 ]
'''
BOTH = ('LightSource "projection" "float scale" 2.5 "float fov" 55 "string filename" "slide.pfm"\n'
        '  LightSource "goniometric" "rgb I" [ 2 4 8 ] "float scale" 0.5 "float power" 10 "string filename" "map.pfm"')


def parse(exe, tmp_path, lights, name="scene.pbrt"):
    (tmp_path / name).write_text(LIGHT_SCENE % {"lights": lights})
    return subprocess.run([exe, str(tmp_path / name), "--parse-only"], capture_output=True, text=True)


def test_scene_file_image_lights(vspg_pbrt, tmp_path):
    """Both directives under a Translate / Rotate CTM, parsed into the records the binding's helpers and the mirror give: position, I (the
    projection's scale; the goniometric I * scale with "power" folded in over the map's own sum), image size, fov."""
    import exr_model as X
    import re
    slide, gmap = M.slide(8, 6, 1), M.gonio_map(5, 3)
    X.write_pfm(str(tmp_path / "slide.pfm"), slide)
    X.write_pfm(str(tmp_path / "map.pfm"), gmap)      # one channel: "Y", taken as it is
    r = parse(vspg_pbrt, tmp_path, BOTH)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = re.findall(r"point light (\d): type (\d) at \((\S+), (\S+), (\S+)\) I \((\S+), (\S+), (\S+)\) (\w+) image (\d+) x (\d+)(?: fov (\S+))?", r.stdout)
    assert len(lines) == 2, r.stdout
    proj = M.projection_light((2.5, 2.5, 2.5), slide, 55.0, ctm_oblique())
    gon = M.goniometric_light((2, 4, 8), gmap, scale=0.5, power=10.0, ctm=ctm_oblique())
    for got, want, kind, size, fov in ((lines[0], proj, "projection", (8, 6), "55"), (lines[1], gon, "goniometric", (5, 5), "")):
        v = np.array([float(x) for x in got[2:8]], f32)
        assert int(got[1]) == want.kind and got[8] == kind and (int(got[9]), int(got[10])) == size and got[11] == fov
        assert np.array_equal(u32(v[:3]), u32(want.pos)) and np.array_equal(u32(v[3:]), u32(want.I)), (v, want.pos, want.I)
    # an RGB map is averaged to Y: the same "power" scale as the map of the averages
    rgb = np.stack([gmap * f32(0.5), gmap, gmap * f32(1.5)], axis=-1).astype(f32)
    X.write_pfm(str(tmp_path / "map.pfm"), rgb)
    r = parse(vspg_pbrt, tmp_path, BOTH)
    avg = ((rgb[..., 0] + rgb[..., 1]) + rgb[..., 2]) / f32(3)
    want = M.goniometric_light((2, 4, 8), avg, scale=0.5, power=10.0, ctm=ctm_oblique())
    got = re.search(r"point light 1: type 6 at \(\S+, \S+, \S+\) I \((\S+), (\S+), (\S+)\)", r.stdout)
    assert r.returncode == 0 and got and np.array_equal(u32(np.array([float(x) for x in got.groups()], f32)), u32(want.I)), r.stdout + r.stderr
    # no filename on a goniometric light: a warning, and the 1 x 1 image (a point light of I * scale)
    r = parse(vspg_pbrt, tmp_path, 'LightSource "goniometric" "rgb I" [ 2 4 8 ] "float scale" 0.5')
    assert r.returncode == 0 and "No \"filename\" parameter provided for goniometric light" in r.stderr and "goniometric image 1 x 1" in r.stdout, r.stdout + r.stderr
    # the committed example parses
    r = subprocess.run([vspg_pbrt, os.path.join(ROOT, "tests", "scenes", "projector_fog.pbrt"), "--parse-only"], capture_output=True, text=True)
    assert r.returncode == 0 and "type 5" in r.stdout and "projection image 4 x 3 fov 40" in r.stdout, r.stdout + r.stderr


def test_scene_file_image_light_refusals(vspg_pbrt, tmp_path):
    import exr_model as X
    X.write_pfm(str(tmp_path / "slide.pfm"), M.slide(8, 6, 1))
    X.write_pfm(str(tmp_path / "map.pfm"), M.gonio_map(5, 3))
    X.write_pfm(str(tmp_path / "wide.pfm"), M.slide(8, 6, 1)[..., 0].copy())
    proj, gon = 'LightSource "projection" "string filename" "slide.pfm"', 'LightSource "goniometric" "string filename" "map.pfm"'
    for lights, needle in ((proj + ' "float power" 100', '"power" is outside this build\'s scope'),
                           ('LightSource "goniometric" "string filename" "wide.pfm"', "non-square"),
                           ('LightSource "projection" "string filename" "missing.pfm"', "missing.pfm"),
                           ('LightSource "goniometric" "string filename" "missing.pfm"', "missing.pfm"),
                           (proj + ' "float bogus" 1', "bogus"), (gon + ' "float fov" 30', "fov"),
                           ('LightSource "projection" "float fov" 40', 'Must provide "filename"'),
                           ('LightSource "projection" "string filename" "map.pfm"', "must have R, G, and B channels"),
                           (proj + ' "float fov" 180', '"fov" must lie in (0, 180)')):
        r = parse(vspg_pbrt, tmp_path, lights)
        assert r.returncode != 0 and needle in r.stderr, (lights, r.stdout + r.stderr)
    # "spot" stays refused exactly as it was
    r = parse(vspg_pbrt, tmp_path, 'LightSource "spot"')
    assert r.returncode != 0 and 'LightSource "spot"' in r.stderr and "vspg_spot_light_look_at" in r.stderr


# ---- 4. the host's table builder under sanitizers: a stand-alone program -------------------------------------------------------------
def write_case(path, light):
    pos, w, phi, cos_o, cos_e = light.bounds()
    dev = light.device_image().reshape(-1)
    with open(path, "wb") as f:
        f.write(struct.pack("<iiif", light.kind, light.xres, light.yres, float(getattr(light, "fov", 0.0))))
        f.write(np.ascontiguousarray(light.raw, f32).tobytes())
        f.write(struct.pack("<i", dev.size))
        f.write(dev.tobytes())
        tail = np.zeros(23, f32)
        if light.kind == M.LIGHT_PROJECTION:
            tail[0:4] = light.sb
            tail[4:16] = light.persp.m[[0, 1, 3]].reshape(12)
            tail[16] = light.A
            tail[17:20], tail[20] = light._sums()
            tail[21] = light.cos_total_width()
        else:
            tail[17] = tail[20] = light._sum_y()
        tail[22] = phi
        f.write(tail.tobytes())


def test_image_light_tables_under_sanitizers(tmp_path):
    """tests/imagelight_build_check.cpp with the two host-only units, compiled with the library's flags plus AddressSanitizer and
    UndefinedBehaviorSanitizer on the host side, linked without the HIP runtime and run directly on case files written from the model:
    1 x 1, 1 x 7, 7 x 1, 8 x 6, 6 x 8 and 64 x 64 slides, 1 x 1, 5 x 5 and 64 x 64 maps.  I = (0.5, 2, 1) as the program's scenes have it."""
    cases = []
    for k, (xres, yres, fov) in enumerate(((1, 1, 90.0), (1, 7, 35.0), (7, 1, 120.0), (8, 6, 70.0), (6, 8, 40.0), (64, 64, 90.0))):
        light = M.projection_light((0.5, 2, 1), M.slide(xres, yres, k), fov=fov)
        cases.append(str(tmp_path / ("slide%d.bin" % k)))
        write_case(cases[-1], light)
    for k, res in enumerate((1, 5, 64)):
        light = M.goniometric_light((0.5, 2, 1), M.gonio_map(res, k))
        cases.append(str(tmp_path / ("map%d.bin" % k)))
        write_case(cases[-1], light)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    hipcc, clangxx = os.path.join(rocm, "bin", "hipcc"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")
    for tool in (hipcc, clangxx):
        if not os.path.exists(tool):
            pytest.fail("%s not found (ROCm)" % tool)
    flags = shlex.split(subprocess.check_output(["make", "-s", "--no-print-directory", "-C", CSRC, "print-HIPFLAGS"], text=True))
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    host = [a for s in sanitize for a in ("-Xarch_host", s)]
    jobs = [(os.path.join(CSRC, u + ".hip"), []) for u in ("vspg_scene_build", "vspg_scene_api")] + \
           [(os.path.join(ROOT, "tests", "imagelight_build_check.cpp"), ["-x", "hip", "-I", CSRC])]
    procs, objs = [], []
    for src, extra in jobs:
        obj = str(tmp_path / (os.path.splitext(os.path.basename(src))[0] + ".o"))
        objs.append(obj)
        cmd = [hipcc] + flags + host + ["-g"] + extra + ["-c", "-o", obj, src]
        procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for cmd, p in procs:
        out = p.communicate()[0]
        assert p.returncode == 0, "%s\n%s" % (" ".join(cmd), out)
    exe = str(tmp_path / "imagelight_build_check")
    subprocess.check_call([clangxx] + sanitize + ["-o", exe] + objs)
    p = subprocess.run([exe] + cases, capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, "exit status %d\n%s\n%s" % (p.returncode, p.stdout, p.stderr)
    assert p.stderr.strip() == "", p.stderr
    assert "%d case files" % len(cases) in p.stdout


# ---- 5. the conditions the statistical test of a projector in fog rests on (tests/test_imagelight_gpu.py) ----------------------------
@pytest.fixture(scope="module")
def fog():
    F = M.FogProjector()
    coarse, fine = F.quadrant_means(F.pixel_means(4, 256)), F.quadrant_means(F.pixel_means(8, 512))
    mc = F.monte_carlo_waves(F.WAVES, seed=1)
    return F, coarse, fine, mc.mean(axis=0), mc.std(axis=0, ddof=1) / math.sqrt(F.WAVES)


def test_fog_model_quadrature_is_finer_than_the_statistic(fog):
    """Halving both step sizes moves no quadrant mean by a tenth of the standard error a 32-wave run has (sized by a NumPy Monte Carlo
    of the same estimator) -- the integrand jumps at the texel and frustum edges, so this is a condition on the view, not a given --,
    and that Monte Carlo agrees with the quadrature itself."""
    F, coarse, fine, mc_mean, se = fog
    print("quadrant means", fine, "standard errors", se, "step-halving moves them by", np.abs(coarse - fine))
    assert np.all(fine > 0) and np.all(np.abs(coarse - fine) < 0.1 * se)
    assert np.all(np.abs(mc_mean - fine) <= 4.5 * se)


@pytest.mark.parametrize("planted", ["no_flip", "use_m"])
def test_fog_statistic_sees_each_planted_error(fog, planted):
    """Without the y flip the tilt points the beam up and out of the view; with m for mInv the slide is rolled the other way round.
    Each moves some quadrant mean by more than ten standard errors of a 32-wave run."""
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
