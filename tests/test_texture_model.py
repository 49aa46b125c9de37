"""Image textures on diffuse reflectance, without a GPU: the float32 mirror (tests/texture_model.py) against the float64 statement of
the mathematics and against hand-derived answers, five planted errors that those checks must see, the record layout against the
header, vspg_renderer_create's refusals as far as they come before the device is asked for, choose_kernel for textured scenes, the
scene-file directives parsed into the expected record with each refusal by name, and the host's validation and image builder under
sanitizers (tests/texture_build_check.cpp, a stand-alone program)."""
import ctypes as C
import os
import re
import shlex
import struct
import subprocess

import numpy as np
import pytest

import texture_model as M
import texture_scenes as TS
from conftest import ROOT

f32 = np.float32
CSRC = os.path.join(ROOT, "vspg-pbrt-v4_amd", "csrc")


def u32(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


# ---- 1. the mirror against the statement ---------------------------------------------------------------------------------------------
def sweep_coordinates(xres, yres):
    """(u, v) from -2.5 to 3.5: a regular lattice of sixteenths of a texel -- exact texel centres and exact texel edges among them, all of
    them exact in float, st of exactly 0 and 1 included -- and seeded irregular points."""
    k = np.arange(-40 * 16, 56 * 16 + 1)                      # sixteenths of a texel of a 16-texel image: -2.5 .. 3.5
    reg = (k / 256.0).astype(f32)
    rng = np.random.default_rng(11)
    ua = np.concatenate([reg, np.array([0.0, 1.0, -2.5, 3.5], f32), rng.uniform(-2.5, 3.5, 3000).astype(f32)])
    va = np.concatenate([reg[::-1], np.array([1.0, 0.0, 3.5, -2.5], f32), rng.uniform(-2.5, 3.5, 3000).astype(f32)])
    return ua, va


SWEEP_TEXTURES = [(xres, yres, wrap, filt) for (xres, yres) in ((2, 2), (4, 1), (8, 4), (16, 16)) for wrap in TS.WRAPS for filt in TS.FILTERS]


def statement_failures(lookup):
    """The mirror (or a planted variant of it) against the statement over the sweep: the list of cases that miss the bound."""
    bad = []
    for xres, yres, wrap, filt in SWEEP_TEXTURES:
        for variant, kw in enumerate((dict(), dict(scale=1.5, invert=True, su=2.0, sv=0.5, du=0.25, dv=-0.75))):
            tex = M.Texture(TS.coloured_image(xres, yres, seed=xres + yres), filter=TS.FILTERS[filt], wrap=TS.WRAPS[wrap], **kw)
            u, v = sweep_coordinates(xres, yres)
            s, t, R, lobes = lookup(tex, u, v)
            want, edge = M.statement(tex, u, v)
            bound = M.error_bound(tex, u, v)
            err = np.abs(R.astype(np.float64) - want).max(axis=1)
            # the point filter jumps at texel edges: a point within the coordinate's own error of an edge may land on either side, EXCEPT
            # where the arithmetic is exact (the regular lattice under the plain mapping: powers of two throughout) -- there the half-away rule decides
            judged = np.ones(len(u), bool)
            if filt == "point":
                exact = (variant == 0) & (np.arange(len(u)) < len(u) - 3000)
                judged = exact | (edge > 1e-3)
            miss = judged & (err > bound)
            if miss.any():
                i = int(np.argmax(miss))
                bad.append((xres, yres, wrap, filt, variant, int(miss.sum()), float(u[i]), float(v[i]), R[i].tolist(), want[i].tolist(), float(bound[i])))
    return bad


def test_mirror_matches_the_statement():
    """Every element of the sweep lies within error_bound (derived there from the operation count: a few hundred EPS times the
    texels' range at these resolutions and coordinates)."""
    bad = statement_failures(M.lookup)
    assert not bad, bad[:3]
    tex = M.Texture(TS.coloured_image(16, 16), su=2.0, du=0.25)
    u, v = sweep_coordinates(16, 16)
    b = M.error_bound(tex, u, v)
    print("largest bound of the 16 x 16 sweep: %.3g (%.0f EPS)" % (b.max(), b.max() / M.EPS))
    assert b.max() < 2e-4


# ---- 2. hand-derived answers -----------------------------------------------------------------------------------------------------------
A, B, Cc, D = (0.125, 0.25, 0.5), (0.75, 0.0625, 0.375), (0.3125, 0.875, 0.1875), (0.625, 0.4375, 0.9375)
IMG22 = np.array([[A, B], [Cc, D]], f32)                       # top row A B, bottom row C D
IMG41 = np.array([[(0.5, 0.25, 0.125), (0.25, 0.25, 0.25), (0.75, 0.5, 0.25), (0.125, 0.375, 0.625)]], f32)


def known_answer_failures(lookup):
    bad = []

    def expect(name, tex, u, v, R, lobes=None, bits=True):
        s, t, got, gl = lookup(tex, [u], [v])
        R = np.asarray(R, f32)
        ok = np.array_equal(u32(got[0]), u32(R)) if bits else np.allclose(got[0], R, atol=1e-6)
        if not ok or (lobes is not None and bool(gl[0]) != lobes):
            bad.append((name, got[0].tolist(), R.tolist(), bool(gl[0])))

    for wrap in (M.REPEAT, M.CLAMP, M.BLACK):
        for filt in (M.POINT, M.BILINEAR):
            tex = M.Texture(IMG22, filter=filt, wrap=wrap)
            # a texel centre returns the texel bit for bit; t is flipped: v = 0.75 is the TOP row (t = 0.25)
            expect("centre A", tex, 0.25, 0.75, A)
            expect("centre B", tex, 0.75, 0.75, B)
            expect("centre C", tex, 0.25, 0.25, Cc)
            expect("centre D", tex, 0.75, 0.25, D)
    # st[0] = 0 on the 4 x 1 image, bilinear: x = -0.5, xi = -1, dx = 0.5: texels -1 and 0 at weight 0.5 each (the one row twice: yi and yi + 1
    # both wrap / clamp to row 0 at v = 0.5, weights dy = 0 and 1 - dy = 1 -- under black row -1 ... is not read at dy = 0: v = 0.5 -> y = 0)
    first, last = IMG41[0, 0], IMG41[0, 3]
    expect("st 0 repeat", M.Texture(IMG41, wrap=M.REPEAT), 0.0, 0.5, f32(0.5) * last + f32(0.5) * first)
    expect("st 0 clamp", M.Texture(IMG41, wrap=M.CLAMP), 0.0, 0.5, first)
    expect("st 0 black", M.Texture(IMG41, wrap=M.BLACK), 0.0, 0.5, f32(0.5) * first)
    expect("st 1 repeat", M.Texture(IMG41, wrap=M.REPEAT), 1.0, 0.5, f32(0.5) * last + f32(0.5) * first)
    # negative coordinates under repeat: u = -0.875 is texel centre 0.125 - 1 -> texel 0; u = -0.125 -> texel 3
    expect("repeat below zero, texel 0", M.Texture(IMG41, wrap=M.REPEAT), -0.875, 0.5, first)
    expect("repeat below zero, texel 3", M.Texture(IMG41, wrap=M.REPEAT), -0.125, 0.5, last)
    expect("repeat below zero, point", M.Texture(IMG41, wrap=M.REPEAT, filter=M.POINT), -0.125, 0.5, last)
    # between texel centres 0 and 1 at a quarter: x = 0.25 -> 0.75 first + 0.25 second
    expect("quarter", M.Texture(IMG41, wrap=M.CLAMP), 0.1875, 0.5, f32(0.75) * first + f32(0.25) * IMG41[0, 1])
    # the same a period to the left: floor, not truncation, for negative x (x = -3.75: xi = -4, dx = 0.25)
    expect("quarter, a period left", M.Texture(IMG41, wrap=M.REPEAT), 0.1875 - 1.0, 0.5, f32(0.75) * first + f32(0.25) * IMG41[0, 1])
    # invert with scale: 1 - scale * texel, not scale * (1 - texel)
    expect("invert with scale", M.Texture(IMG22, filter=M.POINT, scale=0.5, invert=True), 0.25, 0.75, f32(1) - f32(0.5) * np.asarray(A, f32))
    # a value above 1 clamps to 1, per channel
    expect("above one", M.Texture(IMG22, filter=M.POINT, scale=4.0), 0.25, 0.75, np.minimum(f32(4) * np.asarray(A, f32), f32(1)), lobes=True)
    # a negative scale gives black and no lobes
    expect("negative scale", M.Texture(IMG22, filter=M.POINT, scale=-1.0), 0.25, 0.75, (0, 0, 0), lobes=False)
    expect("black outside", M.Texture(IMG22, filter=M.POINT, wrap=M.BLACK), 1.25, 0.75, (0, 0, 0), lobes=False)
    # a one-channel image broadcasts to grey
    expect("grey", M.Texture(np.array([[0.25, 0.5]], f32), filter=M.POINT), 0.75, 0.5, (0.5, 0.5, 0.5), lobes=True)
    # the mapping: uscale / udelta move the lookup: u = 0.25 under su = 2, du = 0.25 is s = 0.75
    expect("mapping", M.Texture(IMG22, filter=M.POINT, su=2.0, du=0.25), 0.25, 0.75, B)
    # a coordinate beyond the range of int is held to 1e9 texels before the conversion: clamp reads the last texel, black reads nothing
    expect("huge coordinate, clamp", M.Texture(IMG41, wrap=M.CLAMP, su=1e30), 1.0, 0.5, last)
    expect("huge coordinate, clamp, point", M.Texture(IMG41, wrap=M.CLAMP, filter=M.POINT, su=-1e30), 1.0, 0.5, first)
    expect("huge coordinate, black", M.Texture(IMG41, wrap=M.BLACK, su=1e30), 1.0, 0.5, (0, 0, 0), lobes=False)
    return bad


def test_known_answers():
    bad = known_answer_failures(M.lookup)
    assert not bad, bad


def test_uv_functions():
    """The rectangle's (u, v) at its corners and centre, exactly; the triangle's at its vertices, with the default and a given uv."""
    p00, e1, e2 = (-1, -1, 1), (0, 2, 0), (2, 0, 0)   # the fog box's back wall: u runs up, v to the right
    u, v = M.uv_quad(p00, e1, e2, [(-1, -1, 1), (-1, 1, 1), (1, -1, 1), (0, 0, 1), (0.5, -0.5, 1)])
    assert u.tolist() == [0, 1, 0, 0.5, 0.25] and v.tolist() == [0, 0, 1, 0.5, 0.75]
    b = np.eye(3, dtype=f32)
    u, v = M.uv_tri(M.DEFAULT_TRI_UV, b)
    assert u.tolist() == [0, 1, 1] and v.tolist() == [0, 0, 1]
    u, v = M.uv_tri([0.25, 0.5, 2, -1, 0.75, 3], [(0.5, 0.25, 0.25)])
    assert u.tolist() == [0.125 + 0.5 + 0.1875] and v.tolist() == [0.25 - 0.25 + 0.75]


@pytest.mark.parametrize("planted", M.PLANTED)
def test_each_planted_error_is_seen(planted):
    """No t flip, the -0.5 omitted, truncation for floor, C's % for Mod, scale applied after invert: each fails a known answer or the
    sweep against the statement."""
    def wrong(tex, u, v):
        return M.lookup(tex, u, v, planted=planted)
    known, sweep = known_answer_failures(wrong), statement_failures(wrong)
    print(planted, "fails", [k[0] for k in known], "and", len(sweep), "sweep cases")
    assert known or sweep


# ---- 3. the C-ABI: header, record layout, bindings --------------------------------------------------------------------------------------
def header():
    return open(os.path.join(ROOT, "include", "vspg.h")).read()


def params_of(name):
    m = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, header())
    assert m, name
    return [re.sub(r"/\*.*?\*/", "", a).strip().split()[-1].lstrip("*") for a in m.group(1).split(",")]


def test_header_declares_the_record_and_both_functions():
    h = header()
    assert "#define VSPG_ABI_VERSION 7" in h and "#define VSPG_MAX_TEXTURES 8" in h and "#define VSPG_TEXTURE_MAX_RES 4096" in h
    assert "VSPG_TEXWRAP_REPEAT = 0, VSPG_TEXWRAP_CLAMP = 1, VSPG_TEXWRAP_BLACK = 2" in h
    assert "VSPG_TEXFILTER_POINT = 0, VSPG_TEXFILTER_BILINEAR = 1" in h and "#define VSPG_TEXTURE_EVAL_OUT 8" in h
    assert params_of("vspg_renderer_set_texture_image") == ["r", "texture_index", "host_pixels", "xres", "yres", "channels", "stream"]
    assert params_of("vspg_texture_eval_batch") == ["r", "n", "prim", "hit", "out", "stream"]
    assert params_of("vspg_renderer_create_textured") == ["scene", "textures", "params", "cfg", "out"]
    doc = " ".join(h.replace(" * ", " ").split())
    for words in ("Out of scope: filtered lookups", "no power of two", "spheres", "A zeroed record holds no texture"):
        assert words in doc, words


def test_record_layout_matches_the_header(pkg, tmp_path):
    """sizeof and offsetof of the new records as a C compiler sees the header, against the ctypes declarations; VspgScene keeps the
    size it had (the textures travel in a record beside it)."""
    src = tmp_path / "layout.c"
    fields_t = [n for n, _ in pkg.VspgTexture._fields_]
    fields_s = [n for n, _ in pkg.VspgSceneTextures._fields_]
    assert fields_s == ["n_textures", "textures", "quad_texture", "tri_texture", "tri_uv"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vspg.h"', "int main(void) {",
             'printf("%zu %zu %zu\\n", sizeof(VspgTexture), sizeof(VspgSceneTextures), sizeof(VspgScene));']
    lines += ['printf("%%zu\\n", offsetof(VspgTexture, %s));' % f for f in fields_t]
    lines += ['printf("%%zu\\n", offsetof(VspgSceneTextures, %s));' % f for f in fields_s]
    lines += ["return 0; }"]
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    out = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    assert out[:3] == [C.sizeof(pkg.VspgTexture), C.sizeof(pkg.VspgSceneTextures), C.sizeof(pkg.VspgScene)] and out[2] == 4392
    want = [getattr(pkg.VspgTexture, f).offset for f in fields_t] + [getattr(pkg.VspgSceneTextures, f).offset for f in fields_s]
    assert out[3:] == want
    z = pkg.VspgSceneTextures()
    assert z.n_textures == 0 and not any(z.quad_texture) and not z.tri_texture and not z.tri_uv


def test_symbols_and_constants(pkg):
    by_name = {name: (res, args) for name, res, args in pkg.SYMBOLS}
    assert len(by_name["vspg_renderer_set_texture_image"][1]) == 7 and len(by_name["vspg_texture_eval_batch"][1]) == 6 and len(by_name["vspg_renderer_create_textured"][1]) == 5
    lib = pkg.load()
    assert hasattr(lib, "vspg_renderer_create_textured") and hasattr(lib, "vspg_renderer_set_texture_image") and hasattr(lib, "vspg_texture_eval_batch") and lib.vspg_abi_version() == 7
    assert (pkg.VSPG_MAX_TEXTURES, pkg.TEXTURE_MAX_RES, pkg.TEXTURE_EVAL_OUT) == (8, 4096, 8)
    assert (pkg.TEXWRAP_REPEAT, pkg.TEXWRAP_CLAMP, pkg.TEXWRAP_BLACK, pkg.TEXFILTER_POINT, pkg.TEXFILTER_BILINEAR) == (0, 1, 2, 0, 1)
    v = np.zeros(12, f32)
    fp = C.POINTER(C.c_float)
    assert lib.vspg_renderer_set_texture_image(None, 0, v.ctypes.data_as(fp), 2, 2, 3, None) == pkg.VSPG_EINVAL
    assert b"null argument" in lib.vspg_last_error()
    assert lib.vspg_texture_eval_batch(None, 1, None, v.ctypes.data_as(fp), v.ctypes.data_as(fp), None) == pkg.VSPG_EINVAL
    s = pkg.VspgScene()
    k = pkg.add_texture(s, TS.coloured_image(4, 2), filter="ewa", wrap="black", scale=2, invert=True, uscale=3, vscale=4, udelta=5, vdelta=6)
    t = pkg.scene_textures(s).textures[0]
    assert k == 1 and pkg.scene_textures(s).n_textures == 1 and (t.xres, t.yres, t.channels, t.wrap, t.filter, t.invert) == (4, 2, 3, 2, 1, 1)
    assert (t.scale, t.su, t.sv, t.du, t.dv) == (2, 3, 4, 5, 6)
    for bad, what in ((np.zeros((2, 2, 3), np.float64), "float32"), (np.zeros((2, 2, 2), f32), "shape"), (np.zeros((2, 4, 3), f32)[:, ::2], "contiguous"),
                      ([[0.0]], "NumPy array")):
        with pytest.raises(ValueError) as e:
            pkg.texture_image_source(bad)
        assert what in str(e.value)


def create_code(pkg, scene):
    """vspg_renderer_create_textured's return code and message (validation comes before the device is asked for)."""
    lib = pkg.load()
    prm = pkg.app_f_params()
    cfg = pkg.VspgRenderConfig(16, 16, 1, 0, 0, 1, 0)
    h = C.c_void_p()
    rc = lib.vspg_renderer_create_textured(C.byref(scene), C.byref(pkg.scene_textures(scene)), C.byref(prm), C.byref(cfg), C.byref(h))
    msg = (lib.vspg_last_error() or b"").decode()
    if rc == 0:
        lib.vspg_renderer_destroy(h)
    return rc, msg


def textured_box(pkg, image=None, **kw):
    s = TS.fog_box(16, 16, triangle=True)
    k = pkg.add_texture(s, TS.coloured_image(4, 4) if image is None else image, **kw)
    pkg.scene_textures(s).quad_texture[TS.BACK] = k
    return s


def test_create_refuses_bad_textures(pkg):
    E, S = pkg.VSPG_EINVAL, pkg.VSPG_ESCOPE
    cases = []
    s = textured_box(pkg); pkg.scene_textures(s).quad_texture[TS.FLOOR] = 2; cases.append((s, E, "names no texture"))
    s = textured_box(pkg); pkg.scene_textures(s).quad_texture[TS.FLOOR] = -1; cases.append((s, E, "names no texture"))
    s = textured_box(pkg); pkg.scene_textures(s).n_textures = 9; cases.append((s, E, "n_textures"))
    s = textured_box(pkg); s.quads[TS.BACK].material = pkg.MATERIAL_INTERFACE; cases.append((s, E, "interface"))
    s = textured_box(pkg); pkg.set_triangle_textures(s, [2]); cases.append((s, E, "triangle's texture index"))
    s = textured_box(pkg); pkg.set_triangle_textures(s, [1], np.full((1, 3, 2), np.nan, f32)); cases.append((s, E, "uv"))
    img = TS.coloured_image(4, 4); img[1, 2, 0] = np.nan; cases.append((textured_box(pkg, img), E, "not-a-number or infinite"))
    img = TS.coloured_image(4, 4); img[3, 3, 2] = np.inf; cases.append((textured_box(pkg, img), E, "not-a-number or infinite"))
    cases.append((textured_box(pkg, scale=float("nan")), E, "not finite"))
    cases.append((textured_box(pkg, udelta=float("inf")), E, "not finite"))
    s = textured_box(pkg); pkg.scene_textures(s).textures[0].xres = 0; cases.append((s, E, "resolution outside"))
    s = textured_box(pkg); pkg.scene_textures(s).textures[0].yres = 8192; cases.append((s, E, "resolution outside"))
    s = textured_box(pkg); pkg.scene_textures(s).textures[0].channels = 2; cases.append((s, E, "1 or 3 channels"))
    s = textured_box(pkg); pkg.scene_textures(s).textures[0].wrap = 3; cases.append((s, E, "wrap"))
    s = textured_box(pkg); pkg.scene_textures(s).textures[0].filter = 2; cases.append((s, E, "filter"))
    s = textured_box(pkg); pkg.scene_textures(s).textures[0].invert = 2; cases.append((s, E, "invert"))
    s = textured_box(pkg); pkg.scene_textures(s).textures[0].pixels = None; cases.append((s, E, "null pixels"))
    cases.append((textured_box(pkg, TS.coloured_image(6, 4)), S, "power of two"))
    cases.append((textured_box(pkg, TS.coloured_image(4, 3)), S, "power of two"))
    for scene, code, needle in cases:
        rc, msg = create_code(pkg, scene)
        assert rc == code and needle in msg, (needle, rc, msg)
    rc, msg = create_code(pkg, textured_box(pkg))   # a good one passes validation: success, or no device
    assert rc in (0, pkg.VSPG_ENODEVICE), (rc, msg)


# ---- 4. choose_kernel for textured scenes ------------------------------------------------------------------------------------------------
CHOICE_PROGRAM = r"""
#include <cstdio>
#include "vspg_kernel_choice.h"
using namespace vspg_choice;
int main() {
    const int media[] = {VSPG_MEDIUM_HOMOGENEOUS, VSPG_MEDIUM_GRID, VSPG_MEDIUM_NANOVDB, VSPG_MEDIUM_RGBGRID};
    for (int textured = 0; textured < 2; ++textured)
        for (int m = 0; m < 4; ++m)
            for (int guided = 0; guided < 2; ++guided) {
                ChoiceFacts f;  // a grey fog box: the headline configuration when nothing is textured
                f.medium_type = media[m];
                f.medium_grey = true, f.surfaces_grey = !textured, f.null_zero = true;
                f.n_textured = textured;
                f.guided = guided, f.training = guided;
                std::printf("%d %d %d %s\n", textured, media[m], guided, kernel_name(choose_kernel(f, ChoiceEnv())).c_str());
            }
    ChoiceEnv lane;
    lane.kernel = "lane";
    ChoiceFacts f;
    f.medium_type = VSPG_MEDIUM_HOMOGENEOUS, f.n_textured = 1;
    std::printf("lane %s\n", kernel_name(choose_kernel(f, lane)).c_str());
    return 0;
}
"""


def test_choose_kernel_for_textured_scenes(tmp_path):
    (tmp_path / "choice.cpp").write_text(CHOICE_PROGRAM)
    exe = str(tmp_path / "choice")
    subprocess.check_call(["c++", "-std=c++17", "-I", CSRC, "-o", exe, str(tmp_path / "choice.cpp")])
    rows = [l.split(" ", 3) for l in subprocess.check_output([exe], text=True).splitlines()]
    got = {(r[0], int(r[1]), int(r[2])): r[3] for r in rows if r[0] != "lane"}
    HOM, GRID, NVDB, RGB = 1, 2, 3, 4
    # untextured: the kernels they were
    assert got[("0", HOM, 0)] == "k_render_wave_wg3<HomogeneousMediumT<2,true>>"
    assert got[("0", HOM, 1)] == "k_render_wave_wg2<HomogeneousMediumT<2,true>,guided,train>"
    # textured over fog: the full-scene workgroup kernel, or the per-lane kernel when guided
    assert got[("1", HOM, 0)] == "k_render_wave_wg2<HomogeneousMedium>"
    assert got[("1", HOM, 1)] == "k_render_wave<HomogeneousMedium,guided,train>"
    # over grid, NanoVDB and RGB grid media: the pipeline, as without a texture
    for m in (GRID, NVDB, RGB):
        for g in (0, 1):
            assert got[("1", m, g)] == got[("0", m, g)] and got[("1", m, g)].startswith("k_wf_"), (m, g, got[("1", m, g)])
    assert [r for r in rows if r[0] == "lane"][0][1:] == ["k_render_wave<HomogeneousMedium>"]


# ---- 5. the host's validation and image builder under sanitizers: a stand-alone program --------------------------------------------------
def test_host_texture_code_under_sanitizers(tmp_path):
    """tests/texture_build_check.cpp with the two host-only units, compiled with the library's flags plus AddressSanitizer and
    UndefinedBehaviorSanitizer on the host side, linked without the HIP runtime and run directly on case files written from the model:
    1 x 1, 2 x 2, 8 x 4 and 64 x 64 images with 1 and 3 channels."""
    cases = []
    for k, (xres, yres, ch) in enumerate(((1, 1, 3), (2, 2, 3), (8, 4, 1), (4, 8, 3), (64, 64, 3), (64, 64, 1))):
        img = TS.coloured_image(xres, yres, seed=k, channels=ch)
        dev = M.Texture(img).device_image().reshape(-1)
        path = str(tmp_path / ("tex%d.bin" % k))
        with open(path, "wb") as f:
            f.write(struct.pack("<iii", xres, yres, ch))
            f.write(img.tobytes())
            f.write(dev.tobytes())
        cases.append(path)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    hipcc, clangxx = os.path.join(rocm, "bin", "hipcc"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")
    for tool in (hipcc, clangxx):
        if not os.path.exists(tool):
            pytest.fail("%s not found (ROCm)" % tool)
    flags = shlex.split(subprocess.check_output(["make", "-s", "--no-print-directory", "-C", CSRC, "print-HIPFLAGS"], text=True))
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    host = [a for s in sanitize for a in ("-Xarch_host", s)]
    jobs = [(os.path.join(CSRC, u + ".hip"), []) for u in ("vspg_scene_build", "vspg_scene_api")] + \
           [(os.path.join(ROOT, "tests", "texture_build_check.cpp"), ["-x", "hip", "-I", CSRC])]
    procs, objs = [], []
    for src, extra in jobs:
        obj = str(tmp_path / (os.path.splitext(os.path.basename(src))[0] + ".o"))
        objs.append(obj)
        cmd = [hipcc] + flags + host + ["-g"] + extra + ["-c", "-o", obj, src]
        procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for cmd, p in procs:
        out = p.communicate()[0]
        assert p.returncode == 0, "%s\n%s" % (" ".join(cmd), out)
    exe = str(tmp_path / "texture_build_check")
    subprocess.check_call([clangxx] + sanitize + ["-o", exe] + objs)
    p = subprocess.run([exe] + cases, capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, "exit status %d\n%s\n%s" % (p.returncode, p.stdout, p.stderr)
    assert p.stderr.strip() == "", p.stderr
    assert "%d case files" % len(cases) in p.stdout


# ---- 6. the scene-file route: directives into the record, refusals by name -----------------------------------------------------------
HOST = os.path.join(ROOT, "vspg-pbrt-v4_amd", "host")


@pytest.fixture(scope="module")
def vspg_pbrt():
    exe = os.path.join(HOST, "vspg_pbrt")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", CSRC, "libvspg_hip.so"])
        subprocess.check_call(["make", "-C", HOST])
    return exe


TEX_SCENE = '''LookAt 0 0 -3  0 0 0  0 1 0
Camera "perspective" "float fov" 40
Sampler "independent" "integer pixelsamples" 2
Film "rgb" "integer xresolution" 32 "integer yresolution" 24 "string filename" "x.pfm"
Integrator "guidedvolpathvspg" "integer maxdepth" 3 "bool surfaceguiding" false "bool volumeguiding" false "bool vspguiding" false
%(options)s
WorldBegin
%(textures)s
AttributeBegin
  AreaLightSource "diffuse" "rgb L" [ 5 5 5 ]
  Shape "bilinearmesh" "point3 P" [ -0.5 2 -0.5   0.5 2 -0.5   -0.5 2 0.5   0.5 2 0.5 ]
AttributeEnd
%(material)s
%(shapes)s
'''
TEX = 'Texture "wood" "spectrum" "imagemap" "string filename" "img.pfm"'
MAT = 'Material "diffuse" "texture reflectance" "wood"'
QUAD = 'Shape "bilinearmesh" "point3 P" [ -1 -1 -1   -1 -1 1    1 -1 -1    1 -1 1 ]'
MESH = 'Shape "trianglemesh" "point3 P" [ 0 0 0  1 0 0  1 1 0  0 1 0 ] "integer indices" [ 0 1 2  0 2 3 ]'
OPTION = 'Option "bool disabletexturefiltering" true'


def parse_scene(exe, tmp_path, textures=TEX, material=MAT, shapes=QUAD, options=OPTION):
    TS.write_pfm(str(tmp_path / "img.pfm"), TS.coloured_image(8, 4, seed=9))
    with open(tmp_path / "grey.pfm", "wb") as f:      # a one-channel PFM: "Y"
        f.write(b"Pf\n2 2\n-1.0\n" + np.array([0.25, 0.5, 0.75, 1.0], "<f4").tobytes())
    (tmp_path / "scene.pbrt").write_text(TEX_SCENE % dict(textures=textures, material=material, shapes=shapes, options=options))
    return subprocess.run([exe, str(tmp_path / "scene.pbrt"), "--parse-only"], capture_output=True, text=True)


def test_scene_file_directives_become_the_record(vspg_pbrt, tmp_path):
    """Texture with every parameter, the defaults, a one-channel image, "texture reflectance" through Material and through a named
    material, "uv" on a trianglemesh and its default, the default uv on a bilinearmesh, a non-planar patch split into two textured
    triangles, and the warning without the option."""
    full = ('Texture "a" "spectrum" "imagemap" "string filename" "img.pfm" "string filter" "point" "string wrap" "black" "float scale" 0.5 '
            '"bool invert" true "string mapping" "uv" "float uscale" 2 "float vscale" 3 "float udelta" 0.25 "float vdelta" -0.5 '
            '"float maxanisotropy" 16 "string encoding" "sRGB"\n'
            'Texture "b" "spectrum" "imagemap" "string filename" "grey.pfm" "string filter" "ewa" "string wrap" "clamp"\n'
            'Texture "c" "spectrum" "imagemap" "string filename" "img.pfm" "string filter" "trilinear"\n'
            'MakeNamedMaterial "named" "string type" "diffuse" "texture reflectance" "c"')
    shapes = "\n".join([
        'Material "diffuse" "texture reflectance" "a"', QUAD + ' "point2 uv" [ 0 0  1 0  0 1  1 1 ]',
        'Material "diffuse" "texture reflectance" "b"', MESH + ' "point2 uv" [ 0 0  2 0  2 1.5  0 1.5 ]',
        'NamedMaterial "named"', MESH,
        'Shape "bilinearmesh" "point3 P" [ -1 -1 -1   -1 -1 1    1 -1 -1    1 0 1 ]',
        'Material "diffuse" "rgb reflectance" [ .2 .3 .4 ]', QUAD])
    r = parse_scene(vspg_pbrt, tmp_path, textures=full, material="", shapes=shapes)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    assert "texture 0: 8 x 4 x 3 wrap 2 filter 0 invert 1 scale 0.5 mapping (2, 3, 0.25, -0.5)" in out, out
    assert "texture 1: 2 x 2 x 1 wrap 1 filter 1 invert 0 scale 1 mapping (1, 1, 0, 0)" in out, out
    assert "texture 2: 8 x 4 x 3 wrap 0 filter 1 invert 0 scale 1 mapping (1, 1, 0, 0)" in out, out
    assert re.findall(r"rectangle (\d+): texture (\d+)", out) == [("1", "0")], out          # (rectangle 0 is the light; the last one has no texture)
    tris = re.findall(r"triangle (\d+): texture (\d+) uv (.*)", out)
    assert [(t[0], t[1]) for t in tris] == [("0", "1"), ("1", "1"), ("2", "2"), ("3", "2"), ("4", "2"), ("5", "2")], out
    assert tris[0][2] == "(0, 0) (2, 0) (2, 1.5)" and tris[1][2] == "(0, 0) (2, 1.5) (0, 1.5)"       # the mesh's uv, per index
    assert tris[2][2] == "(0, 0) (1, 0) (1, 1)" == tris[3][2]                                          # pbrt's default
    assert tris[4][2] == "(0, 0) (1, 0) (1, 1)" and tris[5][2] == "(0, 0) (1, 1) (0, 1)"             # the patch's corners
    assert "level 0" not in r.stderr
    r = parse_scene(vspg_pbrt, tmp_path, options="")
    assert r.returncode == 0 and "textures are evaluated at level 0" in r.stderr, r.stdout + r.stderr
    r = parse_scene(vspg_pbrt, tmp_path, options='Option "bool disabletexturefiltering" false')
    assert r.returncode == 0 and "textures are evaluated at level 0" in r.stderr
    r = subprocess.run([vspg_pbrt, os.path.join(ROOT, "tests", "scenes", "textured_floor.pbrt"), "--parse-only"], capture_output=True, text=True)
    assert r.returncode == 0 and "rectangle 0: texture 0" in r.stdout and "triangle 1: texture 1 uv (0, 0) (2, 1.5) (2, 0)" in r.stdout, r.stdout + r.stderr
    assert "level 0" not in r.stderr


def test_scene_file_refusals_by_name(vspg_pbrt, tmp_path):
    sphere = 'Shape "sphere" "float radius" 0.3'
    cases = [
        (dict(textures='Texture "wood" "spectrum" "checkerboard"'), '"checkerboard"'),
        (dict(textures='Texture "wood" "spectrum" "scale" "float scale" 2'), '"scale"'),
        (dict(textures='Texture "wood" "float" "imagemap" "string filename" "img.pfm"', material=""), '"float" textures'),
        (dict(textures=TEX + ' "string mapping" "spherical"'), 'mapping "spherical"'),
        (dict(textures=TEX + ' "string mapping" "planar"'), 'mapping "planar"'),
        (dict(textures=TEX + ' "string wrap" "octahedralsphere"'), '"octahedralsphere"'),
        (dict(textures=TEX + ' "string filter" "gaussian"'), '"gaussian"'),
        (dict(textures=TEX + ' "float bogus" 1'), "bogus"),
        (dict(textures='Texture "wood" "spectrum" "imagemap"'), '"filename"'),
        (dict(textures='Texture "wood" "spectrum" "imagemap" "string filename" "img.png"'), "8-bit images"),
        (dict(textures='Texture "wood" "spectrum" "imagemap" "string filename" "missing.pfm"'), "missing.pfm"),
        (dict(material='Material "diffuse" "texture reflectance" "marble"'), '"marble" is not defined'),
        (dict(shapes=sphere), 'Shape "sphere" with a textured material'),
        (dict(shapes=MESH + ' "normal3 N" [ 0 0 1  0 0 1  0 0 1  0 0 1 ]'), '"N"'),
        (dict(shapes=MESH + ' "vector3 S" [ 1 0 0  1 0 0  1 0 0  1 0 0 ]'), '"S"'),
        (dict(shapes=MESH + ' "point2 uv" [ 0 0  1 0  1 1 ]'), "one pair per vertex"),
        (dict(shapes=QUAD + ' "point2 uv" [ 0 0  2 0  0 2  2 2 ]'), "only the default"),
    ]
    for kw, needle in cases:
        r = parse_scene(vspg_pbrt, tmp_path, **kw)
        assert r.returncode != 0 and needle in r.stderr, (needle, r.stdout + r.stderr)
    # an untextured sphere beside a textured rectangle is fine
    r = parse_scene(vspg_pbrt, tmp_path, shapes=QUAD + '\nMaterial "diffuse"\n' + sphere)
    assert r.returncode == 0, r.stdout + r.stderr
