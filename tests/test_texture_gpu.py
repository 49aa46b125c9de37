"""Image textures on diffuse reflectance on the device: vspg_texture_eval_batch against the float32 mirror of tests/texture_model.py bit
for bit, constant textures against constant Kd, a known answer without a tolerance, kernel families against each other, a
statistical comparison against a wall built from two rectangles, vspg_renderer_set_texture_image on a live renderer, refusals and
kernel names, and the scene-file route.  Films are 48 x 32 or smaller; images are 1 x 1, 2 x 2, 8 x 4 and 64 x 64."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import texture_model as M
import texture_scenes as TS
from conftest import ROOT

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 48, 32


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def with_kernel(kernel, fn):
    if kernel:
        os.environ["VSPG_KERNEL"] = kernel
    try:
        return fn()
    finally:
        os.environ.pop("VSPG_KERNEL", None)


TRACE_PIXELS = np.array([(x, y) for y in (3, 11, 16, 27) for x in (2, 13, 24, 35, 46)], np.int32)


def run(P, scene, prm, waves=2, kernel=None, post=True, trace=False, w=W, h=H, seed=0):
    """Render `waves` one-sample waves; returns (kernel name, film, counters, replayed paths or None)."""
    def go():
        r = P.Renderer(scene, prm, w, h, seed=seed)
        name = r.kernel_name()
        for k in range(waves):
            r.render_wave(k, k + 1)
            if post:
                r.post_process_wave()
        film, cnt = r.film(), r.counters()
        paths = r.trace_paths(TRACE_PIXELS, np.zeros(len(TRACE_PIXELS), np.int32)) if trace else None
        r.close()
        return name, film, cnt, paths
    return with_kernel(kernel, go)


# ---- 1. the batch against the mirror, bit for bit ------------------------------------------------------------------------------------
QUADS = [((-1.0, -1.0, 1.0), (0.0, 2.0, 0.0), (2.0, 0.0, 0.0)),          # normal along z
         ((-1.0, -1.0, -1.0), (0.0, 0.0, 2.0), (1.5, 0.0, 0.0)),         # normal along y
         ((1.0, -1.0, -1.0), (0.0, 0.0, 0.75), (0.0, 3.0, 0.0)),         # normal along x
         ((-0.3, 0.1, 0.2), (0.6, 0.3, -0.2), (0.1, 0.4, 0.9))]          # oblique: e1 . e2 = 0.06 + 0.12 - 0.18 = 0
BATCH_TRIS = np.array([[(-0.5, -0.5, 0.0), (0.5, -0.5, 0.1), (0.0, 0.5, 0.3)], [(0.2, 0.1, -0.4), (0.7, 0.3, -0.5), (0.1, 0.8, -0.2)]], f32)
BATCH_UV = np.array([[(0.25, 0.5), (2.0, -1.0), (0.75, 3.0)], [(-1.5, -0.25), (0.5, 1.75), (1.25, 0.5)]], f32)
# (image, mapping): the mappings push st outside [0, 1] and below 0
TEX_SPECS = [((1, 1), dict(su=1.0, sv=1.0, du=0.0, dv=0.0)), ((2, 2), dict(su=3.0, sv=-2.0, du=-1.25, dv=0.5)), ((8, 4), dict(su=-1.5, sv=2.5, du=0.75, dv=-1.0)),
             ((64, 64), dict(su=2.0, sv=3.0, du=-0.5, dv=-1.5)), ((8, 4), dict(su=0.5, sv=0.5, du=0.25, dv=0.25, scale=1.75, invert=True)),
             ((2, 2), dict(su=4.0, sv=4.0, du=-2.0, dv=-2.0, scale=-1.0))]
COMBOS = [(w, f) for w in ("repeat", "clamp", "black") for f in ("point", "bilinear")]


@pytest.mark.parametrize("shift,with_uv", [(0, True), (1, False), (2, True), (3, False), (4, True), (5, False)])
def test_eval_batch_equals_the_mirror(gpu_pkg, shift, with_uv):
    """Six textures -- every wrap with both filters, rotated over the six image / mapping pairs by `shift` -- on four rectangles (one
    per axis and an oblique one) and two triangles, with the mesh's uv and with the default; a fifth rectangle without a texture.
    4099 elements, none left out: every output of every element equals the mirror's bits."""
    P = gpu_pkg
    s = TS.fog_box(16, 16, triangle=False)
    s.n_quads = 0
    for p00, e1, e2 in QUADS:
        P.add_quad(s, p00, e1, e2, kd=(0.5, 0.5, 0.5))
    P.add_quad(s, (-1, 1, -1), (2, 0, 0), (0, 0, 2), kd=(0.25, 1.5, 0.0))     # untextured: Kd clamps to (0.25, 1, 0)
    P.set_triangles(s, BATCH_TRIS.copy(), np.full((2, 3), 0.5, f32))
    mirrors = []
    for k, (wrap, filt) in enumerate(COMBOS):
        (xres, yres), kw = TEX_SPECS[(k + shift) % 6]
        img = TS.coloured_image(xres, yres, seed=k, channels=1 if k == 2 else 3)
        pk = dict(kw)
        pk = dict(uscale=pk.pop("su"), vscale=pk.pop("sv"), udelta=pk.pop("du"), vdelta=pk.pop("dv"), **pk)
        assert P.add_texture(s, img, filter=filt, wrap=wrap, **pk) == k + 1
        mirrors.append(M.Texture(img, filter=TS.FILTERS[filt], wrap=TS.WRAPS[wrap], **kw))
    for i in range(4):
        P.scene_textures(s).quad_texture[i] = 1 + (i + shift) % 6
    tri_tex = [1 + (4 + shift) % 6, 1 + (5 + shift) % 6]
    P.set_triangle_textures(s, tri_tex, BATCH_UV if with_uv else None)
    n = 4099
    rng = np.random.default_rng(7 + shift)
    prims = np.array([0, 1, 2, 3, -2, -3, 4], np.int32)[np.arange(n) % 7]
    ab = rng.uniform(-0.3, 1.3, (n, 2)).astype(f32)
    ab[:64] = rng.integers(0, 9, (64, 2)).astype(f32) / f32(8)              # exact edges and corners among them
    hit = np.zeros((n, 3), f32)
    for i, (p00, e1, e2) in enumerate(QUADS + [((-1, 1, -1), (2, 0, 0), (0, 0, 2))]):
        sel = prims == i
        hit[sel] = np.asarray(p00, f32) + ab[sel, :1] * np.asarray(e1, f32) + ab[sel, 1:] * np.asarray(e2, f32)
    bary = rng.dirichlet((1, 1, 1), n).astype(f32)
    bary[:64] = np.eye(3, dtype=f32)[np.arange(64) % 3]
    hit[prims < 0] = bary[prims < 0]
    r = P.Renderer(s, P.app_f_params(), 16, 16)
    got = r.texture_eval_batch(prims, hit)
    r.close()
    want = np.zeros((n, 8), f32)
    all_quads = QUADS + [((-1, 1, -1), (2, 0, 0), (0, 0, 2))]
    for i in range(5):
        sel = prims == i
        u, v = M.uv_quad(*all_quads[i], hit[sel])
        if i < 4:
            st_s, st_t, R, lobes = M.lookup(mirrors[P.scene_textures(s).quad_texture[i] - 1], u, v)
            want[sel] = np.column_stack([u, v, st_s, st_t, R, lobes.astype(f32)])
        else:
            want[sel] = np.column_stack([u, v, np.zeros_like(u), np.zeros_like(u), np.tile(np.array([0.25, 1, 0], f32), (len(u), 1)), np.ones_like(u)])
    for j in range(2):
        sel = prims == -2 - j
        u, v = M.uv_tri(BATCH_UV[j] if with_uv else M.DEFAULT_TRI_UV, hit[sel])
        st_s, st_t, R, lobes = M.lookup(mirrors[tri_tex[j] - 1], u, v)
        want[sel] = np.column_stack([u, v, st_s, st_t, R, lobes.astype(f32)])
    names = ["u", "v", "s", "t", "R.r", "R.g", "R.b", "has_lobes"]
    for c in range(8):
        bad = np.flatnonzero(u32(got[:, c]) != u32(want[:, c]))
        assert bad.size == 0, (names[c], len(bad), "first element", int(bad[0]), int(prims[bad[0]]), got[bad[0]], want[bad[0]])
    assert (want[:, 7] == 0).any() and (want[:, 7] == 1).any() and np.unique(want[:, 4]).size > 100


# ---- scenes of the path tests ------------------------------------------------------------------------------------------------------------
SAFE = dict(uscale=0.5, vscale=0.5, udelta=0.25, vdelta=0.25)   # st stays in [0.25, 0.75]: no wrap decides, whatever the image


def box(P, medium, textures=(), back=0, floor=0, tri=0, back_kd=None, floor_kd=None, tri_kd=(0.5, 0.5, 0.5)):
    """The fog box with its corner triangle (never `simple`), over fog or a 2^3 grid medium; `textures`: add_texture argument pairs."""
    s = TS.fog_box(W, H, triangle=False)
    P.set_triangles(s, TS.CORNER_TRIANGLE.copy(), np.asarray([tri_kd], f32))
    if medium == "grid":
        TS.small_grid_medium(P, s)
    for img, kw in textures:
        P.add_texture(s, img, **kw)
    P.scene_textures(s).quad_texture[TS.BACK], P.scene_textures(s).quad_texture[TS.FLOOR] = back, floor
    if tri:
        P.set_triangle_textures(s, [tri])
    if back_kd is not None:
        s.quads[TS.BACK].Kd[:] = back_kd
    if floor_kd is not None:
        s.quads[TS.FLOOR].Kd[:] = floor_kd
    return s


def guided_params(P):
    prm = P.default_params()
    prm.guide_num_training_waves = 2
    return prm


# ---- 2. constant twins ---------------------------------------------------------------------------------------------------------------------
TWIN_CONSTANTS = [((0.6, 0.3, 0.15), (8, 4), "repeat"), ((0.0, 0.0, 0.0), (1, 1), "clamp"), ((1.0, 1.0, 1.0), (2, 2), "black")]


def trained_state(P, scene, prm, kernel=None):
    """Two training waves of `scene` with the field updated in the loop; returns what a renderer needs to continue from there: both
    fields and the VSP buffer."""
    def go():
        t = P.Renderer(scene, prm, W, H)
        assert "train" in t.kernel_name()
        for w in range(2):
            t.render_wave(w, w + 1)
            t.post_process_wave()
        assert t.training_stats()["iteration"] >= 1
        fields = []
        for vol in (0, 1):
            nodes, regs, nn, nr = t.get_guiding_field(vol)
            fields.append(P.Field(list(nodes)[:nn], list(regs)[:nr]))
        vsp, ready = t.vsp_buffer()
        t.close()
        return fields, vsp, ready
    return with_kernel(kernel, go)


def guided_wave(P, scene, prm, state, kernel=None, wave=2):
    """Wave `wave` of a renderer that starts from `state`: (kernel name, film, counters, replayed paths)."""
    fields, vsp, ready = state

    def go():
        r = P.Renderer(scene, prm, W, H)
        r.set_guiding_field(fields[0], fields[1])
        if ready:
            r.load_vsp_buffer(vsp)
        r.render_wave(wave, wave + 1)
        out = r.kernel_name(), r.film(), r.counters(), r.trace_paths(TRACE_PIXELS, np.full(len(TRACE_PIXELS), wave, np.int32))
        r.close()
        return out
    return with_kernel(kernel, go)


def assert_twins_equal(a, b, family, what):
    assert a[0] == b[0] and a[0].startswith(family), (a[0], b[0])
    assert np.isfinite(a[1]).all() and a[1][..., :3].max() > 0
    assert np.array_equal(u32(a[1]), u32(b[1])), "films differ: %s" % (what,)
    assert a[2] == b[2], (what, a[2], b[2])
    assert np.array_equal(u32(a[3][0]), u32(b[3][0])) and np.array_equal(a[3][1], b[3][1]), "replayed paths differ: %s" % (what,)


# (guided over fog there is one kernel, the per-lane one, whatever VSPG_KERNEL says: it is run once)
@pytest.mark.parametrize("medium,kernel,family,guided", [("fog", None, "k_render_wave_wg2<HomogeneousMedium>", False), ("fog", "lane", "k_render_wave<HomogeneousMedium", False),
                                                         ("grid", None, "k_wf_", False), ("fog", None, "k_render_wave<HomogeneousMedium,guided", True),
                                                         ("grid", None, "k_wf_", True)])
def test_constant_texture_equals_constant_kd(gpu_pkg, medium, kernel, family, guided):
    """A texture that is one constant under "point", on the back wall, the floor and the triangle, against that constant as their Kd:
    films, counters and replayed paths bit for bit, on the same kernel (both scenes hold a triangle: neither is `simple`).
    Guided (over fog a guided textured scene runs the per-lane kernel): the field trains in the loop.  Two renderers that each train
    their own field cannot be compared past the first update: measured on the MI355X, two runs of the SAME untextured scene on
    k_render_wave<HomogeneousMedium,guided,train> agree bit for bit after wave 0 and differ after wave 1
    (test_in_loop_training_is_not_reproducible_run_to_run below records that).  So the twins are compared (a) over the first training wave, each
    recording its own samples, and (b) over a guided wave that both start from ONE state trained in the loop on the textured
    scene -- its two fields and its VSP buffer, read back after two training waves and loaded into both."""
    P = gpu_pkg
    prm = guided_params(P) if guided else P.app_f_params()
    for colour, (xres, yres), wrap in TWIN_CONSTANTS:
        tex = [(TS.constant_image(xres, yres, colour), dict(filter="point", wrap=wrap, **SAFE))]

        def textured():
            return box(P, medium, tex, back=1, floor=1, tri=1)

        def constant():
            return box(P, medium, (), back_kd=colour, floor_kd=colour, tri_kd=colour)
        waves = 1 if guided else 3
        # (guided: the replay comes before the first update, which is where two renderers' fields part)
        a = run(P, textured(), prm, waves=waves, kernel=kernel, trace=True, post=not guided)
        b = run(P, constant(), prm, waves=waves, kernel=kernel, trace=True, post=not guided)
        print(medium, kernel, guided, colour, a[0], a[2])
        assert_twins_equal(a, b, family, (colour, "waves from a fresh renderer"))
        if guided:
            state = trained_state(P, textured(), prm, kernel)
            a = guided_wave(P, textured(), prm, state, kernel)
            b = guided_wave(P, constant(), prm, state, kernel)
            assert_twins_equal(a, b, family, (colour, "a guided wave from the state trained in the loop"))


def test_in_loop_training_is_not_reproducible_run_to_run(gpu_pkg):
    """Why the guided twins above share one trained state: two renderers of the SAME untextured scene, each training its own field,
    agree bit for bit over the first training wave.  Past the first field update they are not held to agree (measured on the MI355X:
    they differ after wave 1); the film after two waves is only required to be finite, and whether it agreed is printed."""
    P = gpu_pkg
    prm = guided_params(P)
    a = run(P, box(P, "fog", ()), prm, waves=1)
    b = run(P, box(P, "fog", ()), prm, waves=1)
    assert a[0] == b[0] == "k_render_wave<HomogeneousMedium,guided,train>" and np.array_equal(u32(a[1]), u32(b[1])) and a[2] == b[2]
    a2, b2 = run(P, box(P, "fog", ()), prm, waves=2), run(P, box(P, "fog", ()), prm, waves=2)
    print("two in-loop training runs of one scene agree after two waves:", bool(np.array_equal(u32(a2[1]), u32(b2[1]))))
    assert np.isfinite(a2[1]).all() and np.isfinite(b2[1]).all()


# ---- 3. a known answer without a tolerance -------------------------------------------------------------------------------------------------
FOUR = [(0.9, 0.2, 0.1), (0.15, 0.8, 0.25), (0.2, 0.3, 0.95), (0.7, 0.65, 0.05)]


def test_four_colour_wall_equals_one_of_four_twins(gpu_pkg):
    """The back wall carries a 2 x 2 point-filtered texture of four colours; 1 spp, maxdepth 1: the first vertex still gathers direct
    light (`depth++ >= maxDepth` is false for depth 0) and every later vertex, surface or volume, ends the path at that test before its
    BSDF or NEE -- only emission is added there, scaled by the throughput the first vertex left.  So a path looks the texture up at most
    once, and a path that does runs exactly as in the twin whose wall has that texel's colour as Kd; every other path is the same in
    all four twins.  Every pixel equals one twin's pixel, exactly one where they differ, and each twin claims its share."""
    P = gpu_pkg
    prm = P.app_f_params()
    prm.maxdepth = 1
    img = np.array([[FOUR[0], FOUR[1]], [FOUR[2], FOUR[3]]], f32)
    name, film, _, _ = run(P, box(P, "fog", [(img, dict(filter="point", wrap="clamp"))], back=1), prm, waves=1, post=False)
    twins = []
    for c in FOUR:
        n2, f2, _, _ = run(P, box(P, "fog", (), back_kd=c), prm, waves=1, post=False)
        assert n2 == name == "k_render_wave_wg2<HomogeneousMedium>"
        twins.append(f2)
    eq = np.stack([np.all(u32(film) == u32(t), axis=-1) for t in twins])          # [4, H, W]
    differ = ~np.all(np.stack([np.all(u32(twins[0]) == u32(t), axis=-1) for t in twins[1:]]), axis=0)
    assert eq.any(axis=0).all(), "%d pixels equal none of the four twins" % int((~eq.any(axis=0)).sum())
    assert np.all(eq[:, ~differ]), "where the twins agree the film agrees with all of them"
    # where the twins differ they differ pairwise (four distinct colours scale the same non-zero light), so a pixel equals one only
    assert np.all(eq[:, differ].sum(axis=0) == 1)
    share = eq[:, differ].mean(axis=1)
    print("pixels at which the twins differ: %d of %d; shares %s" % (int(differ.sum()), differ.size, share))
    assert differ.sum() >= 100 and np.all(share >= 0.10), share


# ---- 4. kernel families against each other -------------------------------------------------------------------------------------------------
PLATFORM = np.array([[(-0.6, -0.7, 0.2), (-0.6, -0.7, 0.8), (0.6, -0.7, 0.8)], [(-0.6, -0.7, 0.2), (0.6, -0.7, 0.8), (0.6, -0.7, 0.2)]], f32)   # faces +y
PLATFORM_UV = np.array([[(0, 0), (0, 1.5), (2, 1.5)], [(0, 0), (2, 1.5), (2, 0)]], f32)


def family_scene(P, medium):
    s = TS.fog_box(W, H, triangle=False)
    if medium == "grid":
        TS.small_grid_medium(P, s)
    P.set_triangles(s, PLATFORM.copy(), np.full((2, 3), 0.5, f32))
    k = P.add_texture(s, TS.coloured_image(64, 64, seed=3), filter="bilinear", wrap="repeat", uscale=1.5, vscale=2.0, udelta=0.1, vdelta=-0.2)
    P.scene_textures(s).quad_texture[TS.BACK] = k
    P.set_triangle_textures(s, [k, k], PLATFORM_UV)
    return s


@pytest.mark.parametrize("medium,default", [("fog", "k_render_wave_wg2<HomogeneousMedium>"), ("grid", "k_wf_")])
def test_kernel_families_agree(gpu_pkg, medium, default):
    """A coloured 64 x 64 bilinear texture on the back wall and on a two-triangle platform with its own uv: the default kernel
    (the full-scene workgroup kernel over fog, the pipeline over the grid) against the per-lane kernel, films and counters bit for bit."""
    P = gpu_pkg
    a = run(P, family_scene(P, medium), P.app_f_params(), waves=3)
    b = run(P, family_scene(P, medium), P.app_f_params(), waves=3, kernel="lane")
    print(medium, a[0], "|", b[0], a[2])
    assert a[0].startswith(default) and b[0].startswith("k_render_wave<") and a[0] != b[0]
    assert np.isfinite(a[1]).all() and a[1][..., :3].max() > 0
    assert np.array_equal(u32(a[1]), u32(b[1])) and a[2] == b[2]
    plain = run(P, TS.fog_box(W, H), P.app_f_params(), waves=3)[1] if medium == "fog" else None
    assert plain is None or not np.array_equal(u32(plain), u32(a[1]))     # ... and the texture is in it


def test_guided_kernel_families_agree(gpu_pkg):
    """Guided.  Over fog a guided textured scene has ONE kernel, the per-lane one (the guided workgroup kernel serves `simple` scenes
    only), so the comparison is over the grid: the field trains in the loop for two waves on the pipeline; with that field and that
    VSP buffer loaded, wave 2 on the pipeline and on the per-lane kernel agree bit for bit (two in-loop training runs are not
    comparable past the first update: test_in_loop_training_is_not_reproducible_run_to_run)."""
    P = gpu_pkg
    prm = guided_params(P)
    fog = P.Renderer(family_scene(P, "fog"), prm, W, H)
    assert fog.kernel_name() == "k_render_wave<HomogeneousMedium,guided,train>" == with_kernel("wg", fog.kernel_name)
    fog.close()
    scene = family_scene(P, "grid")
    state = trained_state(P, scene, prm)
    out = {}
    for kernel in (None, "lane"):
        name, film, cnt, _ = guided_wave(P, scene, prm, state, kernel)
        out[name] = (film, cnt)
    print("guided kernels compared:", sorted(out))
    assert len(out) == 2 and any(n.startswith("k_render_wave<") for n in out) and any(n.startswith("k_wf_") for n in out)
    (fa, ca), (fb, cb) = out.values()
    assert np.isfinite(fa).all() and fa[..., :3].max() > 0
    assert np.array_equal(u32(fa), u32(fb)) and ca == cb


# ---- 5. statistical: a two-texel wall against two rectangles -------------------------------------------------------------------------------
KA, KB = (0.9, 0.3, 0.1), (0.1, 0.4, 0.9)
BLOCKS = [(x0, y0, x0 + 12, y0 + 8) for y0 in (0, 8, 16, 24) for x0 in (0, 12, 24, 36)]     # sixteen 12 x 8 blocks tile the film


def test_two_texel_wall_against_two_rectangles(gpu_pkg):
    """The back wall with a 2 x 1 point-filtered texture (a | b along u, which runs up the wall) in fog at the default maxdepth,
    against the wall built from two rectangles of Kd a (lower half) and b (upper half).  The two run under different seeds, so they
    are independent; per block and channel the means over 48 separately cleared one-sample waves are compared by Welch's statistic,
    |z| <= 4.5 (the threshold of test_pointlight_gpu.py).  What it can see: printed below as 4.5 standard errors of the difference
    relative to the block mean -- measured on the MI355X at these 48 waves: 16 % of a block's channel at the median, 25 % at worst
    (largest |z| 2.8).  Swapping the two texels, or moving their edge by a quarter of the wall, changes the red and blue channels of
    the blocks that look at the wall by far more than that (Kd 0.9 against 0.1); an error of a few percent it does not see."""
    P = gpu_pkg
    prm = P.app_f_params()
    waves = 48
    tex = box(P, "fog", [(np.array([[KA, KB]], f32), dict(filter="point", wrap="clamp"))], back=1)
    two = box(P, "fog", ())
    q = two.quads[TS.BACK]
    q.p00[:], q.e1[:], q.e2[:], q.Kd[:] = (-1, -1, 1), (0, 1, 0), (2, 0, 0), KA
    P.add_quad(two, (-1, 0, 1), (0, 1, 0), (2, 0, 0), kd=KB)
    means = []
    for scene, seed in ((tex, 0), (two, 1)):
        r = P.Renderer(scene, prm, W, H, seed=seed)
        assert r.kernel_name() == "k_render_wave_wg2<HomogeneousMedium>"
        rows = []
        for w in range(waves):
            r.film_clear()
            r.render_wave(w, w + 1)
            f = r.film()[..., :3].astype(np.float64)
            rows.append([f[y0:y1, x0:x1].mean(axis=(0, 1)) for x0, y0, x1, y1 in BLOCKS])
        r.close()
        means.append(np.array(rows))          # [waves, blocks, 3]
    a, b = means
    se = np.sqrt(a.var(axis=0, ddof=1) / waves + b.var(axis=0, ddof=1) / waves)
    z = (a.mean(axis=0) - b.mean(axis=0)) / se
    visible = 4.5 * se / np.maximum(a.mean(axis=0), 1e-12)
    print("largest |z| %.2f; smallest visible relative effect per block and channel: median %.3f, worst %.3f" % (np.abs(z).max(), np.median(visible), visible.max()))
    assert np.all(se > 0) and np.all(np.abs(z) <= 4.5), z


# ---- 6. vspg_renderer_set_texture_image on a live renderer ---------------------------------------------------------------------------------
def probe(r):
    rng = np.random.default_rng(5)
    n = 515
    hit = np.column_stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), np.ones(n)]).astype(f32)
    return r.texture_eval_batch(np.full(n, TS.BACK, np.int32), hit)


def test_set_texture_image_on_a_live_renderer(gpu_pkg):
    P = gpu_pkg
    first, same_res, other_res = TS.coloured_image(8, 4, seed=1), TS.coloured_image(8, 4, seed=2), TS.coloured_image(64, 64, seed=3, channels=1)
    kw = dict(filter="bilinear", wrap="repeat", uscale=2.0, vscale=1.5)
    prm = P.app_f_params()

    def fresh(img):
        return P.Renderer(box(P, "fog", [(img, kw)], back=1), prm, W, H)
    live = fresh(first)
    live.render_wave(0, 1)
    for step, img in enumerate((same_res, other_res)):
        film0, cnt0 = live.film(), live.counters()
        live.set_texture_image(0, img)
        assert np.array_equal(u32(live.film()), u32(film0)) and live.counters() == cnt0          # the film and the counters persist
        ref = fresh(img)
        assert np.array_equal(u32(probe(live)), u32(probe(ref)))
        live.film_clear()
        live.render_wave(1 + step, 2 + step)
        ref.render_wave(1 + step, 2 + step)
        assert ref.film()[..., :3].max() > 0 and np.array_equal(u32(live.film()), u32(ref.film()))
        ref.close()
    # a torch tensor on the device is accepted
    import torch
    live.set_texture_image(0, torch.from_numpy(first).to("cuda:0"))
    ref = fresh(first)
    assert np.array_equal(u32(probe(live)), u32(probe(ref)))
    ref.close()
    # refusals leave the renderer unchanged
    before, film0 = probe(live), live.film()
    nan = first.copy(); nan[2, 3, 1] = np.nan
    for bad_index, img, code, needle in ((0, nan, P.VSPG_EINVAL, "not-a-number or infinite"), (1, first, P.VSPG_EINVAL, "names no texture"),
                                         (-1, first, P.VSPG_EINVAL, "names no texture"), (0, TS.coloured_image(6, 4), P.VSPG_ESCOPE, "power of two"),
                                         (0, np.zeros((4, 8192, 1), f32), P.VSPG_EINVAL, "resolution outside")):
        with pytest.raises(P.VspgError) as e:
            live.set_texture_image(bad_index, img)
        assert e.value.code == code and needle in str(e.value), str(e.value)
    assert np.array_equal(u32(probe(live)), u32(before)) and np.array_equal(u32(live.film()), u32(film0))
    live.close()


def test_set_texture_image_keeps_the_guiding_field(gpu_pkg):
    P = gpu_pkg
    kw = dict(filter="bilinear", wrap="repeat")
    r = P.Renderer(box(P, "fog", [(TS.coloured_image(8, 4, seed=1), kw)], back=1), guided_params(P), W, H)
    for w in range(2):
        r.render_wave(w, w + 1)
        r.post_process_wave()

    def state():
        out = [r.training_stats()]
        for vol in (0, 1):
            nodes, regs, nn, nr = r.get_guiding_field(vol)
            out.append((nn, nr, bytes(nodes)[:nn * C.sizeof(P.VspgKdNode)], bytes(regs)[:nr * C.sizeof(P.VspgFieldRegion)]))
        return out, r.vsp_buffer()[0].tobytes()
    before = state()
    assert before[0][0]["iteration"] >= 1
    r.set_texture_image(0, TS.coloured_image(2, 2, seed=4))
    assert state() == before
    r.render_wave(2, 3)
    assert np.isfinite(r.film()).all()
    r.close()


# ---- 7. refusals and kernel names ----------------------------------------------------------------------------------------------------------
def test_kernel_names_and_refusals_on_the_device(gpu_pkg):
    P = gpu_pkg
    img, kw = TS.coloured_image(8, 4), dict(filter="bilinear", wrap="repeat")

    def name(scene, prm):
        r = P.Renderer(scene, prm, 16, 16)
        n = r.kernel_name()
        r.close()
        return n
    plain = TS.fog_box(16, 16, triangle=False)
    headline = name(plain, P.app_f_params())
    assert headline.startswith("k_render_wave_wg3<")
    unbound = TS.fog_box(16, 16, triangle=False)
    P.add_texture(unbound, img, **kw)                      # a texture no surface uses: the scene's kernel is the one it was
    assert name(unbound, P.app_f_params()) == headline
    bound = TS.fog_box(16, 16, triangle=False)
    P.scene_textures(bound).quad_texture[TS.FLOOR] = P.add_texture(bound, img, **kw)
    assert name(bound, P.app_f_params()) == "k_render_wave_wg2<HomogeneousMedium>"
    assert name(bound, guided_params(P)) == "k_render_wave<HomogeneousMedium,guided,train>"
    grid = TS.small_grid_medium(P, TS.fog_box(16, 16, triangle=False))
    grid_name = name(grid, P.app_f_params())
    P.scene_textures(grid).quad_texture[TS.FLOOR] = P.add_texture(grid, img, **kw)
    assert name(grid, P.app_f_params()) == grid_name and grid_name.startswith("k_wf_")
    # refusals at create with a device present: the same codes, and nothing is left behind that stops the next renderer
    for mutate, code in ((lambda s: setattr(P.scene_textures(s).textures[0], "xres", 6), P.VSPG_ESCOPE), (lambda s: P.scene_textures(s).quad_texture.__setitem__(1, 5), P.VSPG_EINVAL),
                         (lambda s: setattr(P.scene_textures(s).textures[0], "wrap", 7), P.VSPG_EINVAL)):
        s = TS.fog_box(16, 16, triangle=False)
        P.scene_textures(s).quad_texture[TS.FLOOR] = P.add_texture(s, img, **kw)
        mutate(s)
        with pytest.raises(P.VspgError) as e:
            P.Renderer(s, P.app_f_params(), 16, 16)
        assert e.value.code == code, str(e.value)
    # the batch refuses primitives it has no answer for: a sphere, a rectangle or a triangle that is not there
    s = TS.fog_box(16, 16, triangle=True)
    P.add_sphere(s, (0, 0, 0), 0.2)
    P.scene_textures(s).quad_texture[TS.FLOOR] = P.add_texture(s, img, **kw)
    r = P.Renderer(s, P.app_f_params(), 16, 16)
    for prim in (32, 7, -1, -3):
        with pytest.raises(P.VspgError) as e:
            r.texture_eval_batch([prim], [(0, 0, 0)])
        assert e.value.code == P.VSPG_EINVAL
    assert r.texture_eval_batch([0, -2], [(0, -1, 0), (1, 0, 0)]).shape == (2, 8)
    r.close()


def test_coordinates_beyond_the_range_of_int(gpu_pkg):
    """uscale = +-1e30 is finite and passes validation: the texel coordinate is held to +-1e9 before it becomes an integer, on the device
    as in the mirror -- every output equals the mirror's bits, for both filters under clamp and black."""
    P = gpu_pkg
    rng = np.random.default_rng(3)
    hit = np.column_stack([rng.uniform(-1, 1, 257), -np.ones(257), rng.uniform(-1, 1, 257)]).astype(f32)
    floor = ((-1, -1, -1), (0, 0, 2), (2, 0, 0))
    for filt in ("point", "bilinear"):
        for wrap in ("clamp", "black", "repeat"):
            for su in (1e30, -1e30):
                s = TS.fog_box(16, 16, triangle=False)
                img = TS.coloured_image(8, 4, seed=5)
                P.scene_textures(s).quad_texture[TS.FLOOR] = P.add_texture(s, img, filter=filt, wrap=wrap, uscale=su, vscale=-su)
                r = P.Renderer(s, P.app_f_params(), 16, 16)
                got = r.texture_eval_batch(np.full(257, TS.FLOOR, np.int32), hit)
                r.close()
                u, v = M.uv_quad(*floor, hit)
                st_s, st_t, R, lobes = M.lookup(M.Texture(img, filter=TS.FILTERS[filt], wrap=TS.WRAPS[wrap], su=su, sv=-su), u, v)
                want = np.column_stack([u, v, st_s, st_t, R, lobes.astype(f32)])
                assert np.array_equal(u32(got), u32(want)), (filt, wrap, su)


# ---- 8. the scene-file route ---------------------------------------------------------------------------------------------------------------
def test_scene_file_equals_the_c_abi(gpu_pkg, tmp_path):
    """vspg_pbrt tests/scenes/textured_floor.pbrt -- a bilinear repeating texture with a scaled and shifted mapping on the floor, an
    inverted point-filtered clamped one on a two-triangle platform with its own uv -- against the same scene built through the binding:
    the films are equal bit for bit, and the textures are in it."""
    import exr_model as X
    P = gpu_pkg
    exe = os.path.join(ROOT, "vspg-pbrt-v4_amd", "host", "vspg_pbrt")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    out = tmp_path / "textured_floor.pfm"
    a = subprocess.run([exe, os.path.join(ROOT, "tests", "scenes", "textured_floor.pbrt"), "--outfile", str(out), "--spp", "3"], capture_output=True, text=True, timeout=120)
    assert a.returncode == 0, a.stdout + a.stderr
    got = X.read_pfm(str(out))
    img = np.ascontiguousarray(X.read_pfm(os.path.join(ROOT, "tests", "golden", "texture_floor.pfm")), f32)
    assert img.shape == (4, 8, 3)
    s = P.fog_box_scene(64, 48)
    s.quads[TS.FLOOR].Kd[:] = (0.5, 0.5, 0.5)
    P.scene_textures(s).quad_texture[TS.FLOOR] = P.add_texture(s, img, filter="bilinear", wrap="repeat", scale=1.1, uscale=2, vscale=3, udelta=0.125, vdelta=-0.25)
    k2 = P.add_texture(s, img, filter="point", wrap="clamp", invert=True)
    v = np.array([(-0.6, -0.7, 0.2), (-0.6, -0.7, 0.8), (0.6, -0.7, 0.8), (0.6, -0.7, 0.2)], f32)
    uv = np.array([(0, 0), (0, 1.5), (2, 1.5), (2, 0)], f32)
    P.set_triangles(s, np.stack([v[[0, 1, 2]], v[[0, 2, 3]]]), np.full((2, 3), 0.5, f32))
    P.set_triangle_textures(s, [k2, k2], np.stack([uv[[0, 1, 2]], uv[[0, 2, 3]]]))
    r = P.Renderer(s, P.app_f_params(), 64, 48)
    for w in range(3):
        r.render_wave(w, w + 1)
        r.post_process_wave()
    f = r.film()
    r.close()
    want = (f[..., :3] / f[..., 3:4]).astype(f32)
    assert want.max() > 0 and np.array_equal(u32(got), u32(want))
    plain = P.Renderer(P.fog_box_scene(64, 48), P.app_f_params(), 64, 48)
    for w in range(3):
        plain.render_wave(w, w + 1)
        plain.post_process_wave()
    assert not np.array_equal(u32(plain.film()), u32(f))
    plain.close()
