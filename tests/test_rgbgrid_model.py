"""RGBGridMedium ("rgbgrid") without a device: the float32 mirror of tests/rgbgrid_model.py against the float64 statement of the same
mathematics, hand-derived known answers, five planted errors that the fixtures must each expose, the scene record's layout against
a C program compiled with the header, the refusals of create, the host-side build as a stand-alone program under sanitizers, and the
precondition of the GPU tests' equivalence: for power-of-two coefficients the rgbgrid mirror equals the models of the uniformgrid
(tests/brick_model.py, tests/majorant_model.py) in every bit."""
import ctypes as C
import os
import shlex
import subprocess

import numpy as np
import pytest

import brick_model
import majorant_model
import rgbgrid_model as M

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vspg-pbrt-v4_amd", "csrc")
FIXTURES = M.fixtures()


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. mirror against statement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_mirror_stays_within_the_derived_bound_of_the_statement(name):
    """Both are given the same MEDIUM-space float32 points (the transform has its own test in the GPU suite's placed fixture, where the
    device must equal the mirror bit for bit).  The bound is rgbgrid_model.lookup_bound's, derived there from the operation count."""
    med = FIXTURES[name]
    pm = M.to_medium32(med, M.probe_points(med))
    keep = np.all((M.offset32(med, pm) >= -1) & (M.offset32(med, pm) <= 2), axis=1)   # the bound's range of coordinates
    pm = pm[keep]
    flat = M.RgbGrid(med.sigma_a, med.sigma_s, med.Le, p0=med.p0, p1=med.p1, g=med.g, scale=med.scale, Lescale=med.Lescale)
    got = M.sample_point32(flat, pm)
    want = M.sample_point64(flat, pm)
    for which, grid, scale in (("sigma_a", med.sigma_a, med.scale), ("sigma_s", med.sigma_s, med.scale), ("Le", med.Le, med.Lescale)):
        g, w = got[("sigma_a", "sigma_s", "Le").index(which)], want[("sigma_a", "sigma_s", "Le").index(which)]
        if grid is None:
            assert np.array_equal(g, w.astype(f32))   # the constant: scale * 1 (or no emission), exact
            continue
        bound = M.lookup_bound(med, grid) * (float(scale) / float(med.scale))
        err = np.abs(g.astype(np.float64) - w).max()
        print("%s %s: max error %.3g, bound %.3g" % (name, which, err, bound))
        assert err <= bound
    m32, m64 = M.majorant32(med), M.majorant64(med)
    assert np.all(np.abs(m32.astype(np.float64) - m64) <= 2.01 * M.U * m64)   # a sum and a product: two roundings


# ---- 2. known answers ----------------------------------------------------------------------------------------------------------------
def test_known_answers():
    # the 1^3 tent against the zero background: at the centre the voxel itself, at a corner of the bounds 1/8 of it (each axis
    # interpolates half way between the voxel and the background), on a face centre 1/2
    a, s = np.array([[[[1.0, 2.0, 4.0]]]], f32), np.array([[[[8.0, 0.5, 0.25]]]], f32)
    tent = M.RgbGrid(a, s, p0=(-1, -1, -1), p1=(1, 1, 1), scale=2.0)
    sa, ss, le = M.sample_point32(tent, np.array([[0, 0, 0], [1, 1, 1], [-1, -1, -1], [1, 0, 0], [3, 0, 0]], f32))
    assert sa.tolist() == [[2, 4, 8], [0.25, 0.5, 1], [0.25, 0.5, 1], [1, 2, 4], [0, 0, 0]]
    assert ss.tolist() == [[16, 1, 0.5], [2, 0.125, 0.0625], [2, 0.125, 0.0625], [8, 0.5, 0.25], [0, 0, 0]]
    assert not le.any()
    assert np.all(M.majorant32(tent) == f32(2 * (4 + 8)))
    # a two-voxel majorant (the same numbers as tests/rgbgrid_build_check.cpp): cells 0..11 along x see voxel 0 (alone or with voxel
    # 1), cells 12..15 voxel 1 alone; the maximum over voxels AND channels per grid, then the sum, then the scale
    two = M.RgbGrid(np.array([[[[1, 5, 2], [3, 0, 4]]]], f32), np.array([[[[7, 1, 1], [2, 2, 6]]]], f32), scale=2.0)
    maj = M.majorant32(two)
    assert np.all(maj[:, :, :12] == 24) and np.all(maj[:, :, 12:] == 20)
    # the absent grid is the constant 1 in both places
    only_s = M.RgbGrid(sigma_s=np.array([[[[7, 1, 1], [2, 2, 6]]]], f32), scale=2.0)
    sa, ss, _ = M.sample_point32(only_s, np.array([[0.25, 0.5, 0.5], [5, 5, 5]], f32))
    assert sa.tolist() == [[2, 2, 2], [2, 2, 2]] and ss.tolist() == [[14, 2, 2], [0, 0, 0]]   # (sigma_a = scale * 1 even outside the bounds, media.h:424-426)
    maj = M.majorant32(only_s)
    assert np.all(maj[:, :, :12] == 16) and np.all(maj[:, :, 12:] == 14)
    # emission: Lescale * Lookup(Le); none without a grid or with a scale that is not positive
    glow = M.RgbGrid(a, s, Le=np.array([[[[1, 2, 3]]]], f32), p0=(-1, -1, -1), p1=(1, 1, 1), Lescale=0.5)
    assert M.sample_point32(glow, np.zeros((1, 3), f32))[2].tolist() == [[0.5, 1, 1.5]]
    glow.Lescale = f32(0)
    assert not M.sample_point32(glow, np.zeros((1, 3), f32))[2].any()


# ---- 3. planted errors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planted", M.PLANTED)
def test_every_planted_error_fails_on_the_fixtures(planted):
    """Each error changes the mirror's bits on at least one fixture: a device that made it would fail the GPU comparison."""
    exposed = []
    for name, med in FIXTURES.items():
        p = M.probe_points(med, n_random=600)
        truth = np.concatenate(M.sample_point32(med, p), axis=1)
        wrong = np.concatenate(M.sample_point32(med, p, planted=(planted,)), axis=1)
        if not np.array_equal(u32(truth), u32(wrong)) or not np.array_equal(M.majorant32(med), M.majorant32(med, planted=(planted,))):
            exposed.append(name)
    print(planted, "exposed by", exposed)
    assert exposed, planted
    if planted == "absent_zero":
        assert set(exposed) == {"only-a", "only-s"}


# ---- 4. the scene record's layout ----------------------------------------------------------------------------------------------------
LAYOUT_PROGRAM = r"""
#include <stdio.h>
#include <stddef.h>
#include "vspg.h"
int main(void) {
    printf("%zu %zu %d %d", sizeof(VspgMedium), sizeof(VspgScene), VSPG_ABI_VERSION, VSPG_MEDIUM_RGBGRID);
#define F(f) printf(" %zu", offsetof(VspgScene, f))
    F(medium); F(n_triangles); F(camera_outside_medium); F(n_point_lights); F(sphere_Le); F(sphere_two_sided);
    F(rgb_sigma_a); F(rgb_sigma_s); F(rgb_Le); F(rgb_sigma_scale); F(rgb_le_scale);
    printf("\n");
    return 0;
}
"""


def test_record_layout_against_the_header(pkg, tmp_path):
    """Sizes and offsets as a C compiler sees the header, against the binding and against the record before this tail (numbers printed
    from the parent's header): VspgMedium keeps its 312 bytes, nothing in front of the tail moved, the tail starts where the record ended."""
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_PROGRAM)
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    v = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    S = pkg.VspgScene
    assert v[:4] == [312, 4392, 7, 4] and pkg.MEDIUM_RGBGRID == 4
    assert v[0] == C.sizeof(pkg.VspgMedium) and v[1] == C.sizeof(S)
    names = ["medium", "n_triangles", "camera_outside_medium", "n_point_lights", "sphere_Le", "sphere_two_sided", "rgb_sigma_a", "rgb_sigma_s", "rgb_Le",
             "rgb_sigma_scale", "rgb_le_scale"]
    assert v[4:] == [getattr(S, n).offset for n in names]
    assert v[4:10] == [1288, 1600, 3004, 3008, 4228, 4324]          # the parent's offsets
    assert v[10] == 4360                                             # the parent's sizeof(VspgScene): the tail begins where the record ended
    s = S()
    assert not s.rgb_sigma_a and not s.rgb_sigma_s and not s.rgb_Le and s.rgb_sigma_scale == 0   # a zeroed record holds no RGB grid


# ---- 5. refusals of create, before the device is opened ------------------------------------------------------------------------------
def good_scene(pkg):
    s = pkg.fog_box_scene(16, 16)
    med = FIXTURES["both-2x3x5"]
    le = M.coloured(med.n, 99, hi=0.5)
    return pkg.set_rgb_grid_medium(s, med.sigma_a.copy(), med.sigma_s.copy(), le, p0=(-0.5,) * 3, p1=(0.5,) * 3, scale=1.5, Lescale=2.0)


def _null(s, *names):
    for n in names:
        setattr(s, n, C.POINTER(C.c_float)())


def _poke(name, value):
    def spoil(s):
        s._rgb_keepalive[name][4, 2, 1, 1] = value
    return spoil


REFUSALS = [
    ("requires \"sigma_a\" and/or \"sigma_s\"", lambda s: _null(s, "rgb_sigma_a", "rgb_sigma_s", "rgb_Le")),
    ("requires \"sigma_a\" if \"Le\"", lambda s: _null(s, "rgb_sigma_a")),
    ("negative or not finite", _poke("sigma_a", -1.0)), ("negative or not finite", _poke("sigma_s", float("nan"))),
    ("negative or not finite", _poke("Le", float("inf"))), ("negative or not finite", _poke("sigma_s", -0.5)),
    ("nx, ny, nz > 0", lambda s: setattr(s.medium, "ny", 0)), ("nx, ny, nz > 0", lambda s: setattr(s.medium, "nx", -2)),
    ("is not finite", lambda s: setattr(s, "rgb_sigma_scale", float("inf"))), ("is not finite", lambda s: setattr(s, "rgb_le_scale", float("nan"))),
    ("no temperature grid", lambda s: setattr(s.medium, "temperature", s.rgb_sigma_a)),
]


@pytest.mark.parametrize("needle,spoil", REFUSALS, ids=["%d %s" % (i, r[0][:18]) for i, r in enumerate(REFUSALS)])
def test_create_refuses(pkg, needle, spoil):
    lib = pkg.load()
    s = good_scene(pkg)
    spoil(s)
    prm, cfg, h = pkg.app_f_params(), pkg.VspgRenderConfig(16, 16, 1, 0, 0, 1, 0), C.c_void_p()
    rc = lib.vspg_renderer_create(C.byref(s), C.byref(prm), C.byref(cfg), C.byref(h))
    assert rc == pkg.VSPG_EINVAL and not h.value and needle in lib.vspg_last_error().decode(), lib.vspg_last_error()


def test_good_scene_and_absent_grids_pass_validation(pkg):
    """(Without a device: VSPG_ENODEVICE after validation.)"""
    lib = pkg.load()
    for drop in ((), ("rgb_sigma_s",), ("rgb_sigma_a", "rgb_Le"), ("rgb_Le",)):
        s = good_scene(pkg)
        _null(s, *drop)
        prm, cfg, h = pkg.app_f_params(), pkg.VspgRenderConfig(16, 16, 1, 0, 0, 1, 0), C.c_void_p()
        rc = lib.vspg_renderer_create(C.byref(s), C.byref(prm), C.byref(cfg), C.byref(h))
        assert rc in (0, pkg.VSPG_ENODEVICE), (drop, lib.vspg_last_error())
        if rc == 0:
            lib.vspg_renderer_destroy(h)


def test_binding_helper(pkg):
    s = good_scene(pkg)
    m = s.medium
    assert m.type == pkg.MEDIUM_RGBGRID and (m.nx, m.ny, m.nz) == (2, 3, 5) and s.rgb_sigma_scale == 1.5 and s.rgb_le_scale == 2.0
    assert s.rgb_sigma_a[3 * (2 * (3 * 4 + 2) + 1) + 1] == s._rgb_keepalive["sigma_a"][4, 2, 1, 1]   # voxel-major, x fastest, R G B per voxel
    with pytest.raises(ValueError):
        pkg.set_rgb_grid_medium(pkg.fog_box_scene(16, 16), np.zeros((2, 2, 2, 3), f32), np.zeros((2, 2, 3, 3), f32))
    with pytest.raises(ValueError):
        pkg.set_rgb_grid_medium(pkg.fog_box_scene(16, 16), np.zeros((2, 2, 2), f32))


# ---- 6. the host-side build under sanitizers: a stand-alone program ------------------------------------------------------------------
def test_rgb_grid_scene_build_under_sanitizers(tmp_path):
    """tests/rgbgrid_build_check.cpp with the two host-only units, compiled with the library's flags plus AddressSanitizer and
    UndefinedBehaviorSanitizer on the host side, linked without the HIP runtime and run directly (as tests/test_spherelight_model.py does)."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    hipcc, clangxx = os.path.join(rocm, "bin", "hipcc"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")
    for tool in (hipcc, clangxx):
        if not os.path.exists(tool):
            pytest.fail("%s not found (ROCm)" % tool)
    flags = shlex.split(subprocess.check_output(["make", "-s", "--no-print-directory", "-C", CSRC, "print-HIPFLAGS"], text=True))
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    host = [a for s in sanitize for a in ("-Xarch_host", s)]
    jobs = [(os.path.join(CSRC, u + ".hip"), []) for u in ("vspg_scene_build", "vspg_scene_api")] + \
           [(os.path.join(ROOT, "tests", "rgbgrid_build_check.cpp"), ["-x", "hip", "-I", CSRC])]
    procs, objs = [], []
    for src, extra in jobs:
        obj = str(tmp_path / (os.path.splitext(os.path.basename(src))[0] + ".o"))
        objs.append(obj)
        cmd = [hipcc] + flags + host + ["-g"] + extra + ["-c", "-o", obj, src]
        procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for cmd, p in procs:
        out = p.communicate()[0]
        assert p.returncode == 0, "%s\n%s" % (" ".join(cmd), out)
    exe = str(tmp_path / "rgbgrid_build_check")
    subprocess.check_call([clangxx] + sanitize + ["-o", exe] + objs)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, "exit status %d\n%s\n%s" % (p.returncode, p.stdout, p.stderr)


# ---- 7. the equivalence's precondition -----------------------------------------------------------------------------------------------
POW2 = [(0.25, 1.0, 2.0), (1.0, 0.25, 0.25), (2.0, 2.0, 1.0)]   # a, s, k


@pytest.mark.parametrize("n", M.SHAPES, ids=lambda n: "%dx%dx%d" % n)
def test_grey_twin_equals_the_uniformgrid_models_in_every_bit(n):
    """uniformgrid: sigma_a = (a k) Lookup(d), sigma_s = (s k) Lookup(d), majorant (a k + s k) MaxValue(d) -- the arithmetic of
    GridMediumT (sigma * d, sigma_t * majorant) over tests/brick_model.py's Lookup and tests/majorant_model.py's grid.  The rgbgrid
    with voxels a d_i, s d_i and scale k: multiplication by a power of two commutes with every rounding of the lerps, and
    fl(a m + s m) = fl((a + s) m).  The same for the emissive pair."""
    rng = np.random.default_rng(5)
    d = rng.uniform(0.2, 3.0, size=n[0] * n[1] * n[2]).astype(f32)
    d[rng.random(d.size) < 0.25] = 0
    sc = rng.uniform(0.0, 2.0, size=d.size).astype(f32)
    le, Lescale = np.array([2.0, 1.0, 0.5], f32), 4.0
    for a, s, k in POW2:
        med = M.grey_twin(d, n, a, s, k, le=le, le_scale=sc, Lescale=Lescale, p0=(-0.7, -0.8, -0.5), p1=(0.8, 0.7, 0.9))
        p = M.probe_points(med, n_random=800)
        o = M.offset32(med, p)
        sa, ss, Le = M.sample_point32(med, p)
        lookup = lambda dens: brick_model.lerp_grid(o, n, lambda ix, iy, iz: brick_model.raw_octet(dens, n, ix, iy, iz))
        dl, scl = lookup(d), lookup(sc)
        ua, us = f32(a) * f32(k), f32(s) * f32(k)   # the scene record's sigma_a / sigma_s: "already multiplied by scale"
        for c in range(3):
            assert np.array_equal(u32(sa[:, c]), u32(ua * dl)) and np.array_equal(u32(ss[:, c]), u32(us * dl))
            assert np.array_equal(u32(Le[:, c]), u32(np.where(scl > 0, le[c] * scl, f32(0))))
        assert majorant_model.same_majorants(M.majorant32(med), (ua + us) * majorant_model.majorant_grid(d, n))


# ---- 8. what the statistical GPU test rests on ---------------------------------------------------------------------------------------
def test_proportional_fixture_separates_its_channels():
    """The Welch test of tests/test_rgbgrid_gpu.py compares the rgbgrid with the chromatic uniformgrid channel by channel; a channel
    swap must not be able to pass it.  What can be shown without a device: the red and the blue channel are different media -- single-
    scattering albedo 0.571 against 0.985, extinction 1.4 d against 3.25 d -- so their films differ by a large factor of the mean, not by
    noise.  That the difference is many STANDARD ERRORS needs rendered waves: the GPU test asserts it on its own means (|z| > 10)
    before it compares anything."""
    a, s = np.array(M.PROPORTIONAL_A), np.array(M.PROPORTIONAL_S)
    albedo = s / (a + s)
    assert albedo[0] < 0.6 and albedo[2] > 0.98 and (a + s)[2] / (a + s)[0] > 2
    assert a[0] / a[2] > 11.9 and s[2] / s[0] > 3.9
    # ... and the rgbgrid's scalar majorant differs from the uniformgrid's per-channel one: the two renderers do not walk the same paths
    d = np.array([[[[1.0]]]], f32)
    med = M.RgbGrid(d * np.array(M.PROPORTIONAL_A, f32), d * np.array(M.PROPORTIONAL_S, f32))
    assert np.all(M.majorant32(med) == f32(0.6) + f32(3.2)) and not np.any(np.isclose(a + s, 3.8))
