"""Projection and goniometric lights on the device: vspg_light_sample_batch against the float32 mirror of tests/imagelight_model.py bit
for bit, the three light samplers over a scene with every light kind, vspg_renderer_set_light_image on a live renderer, and the
lights through whole paths -- a goniometric light with the 1 x 1 image against a point light, kernel families against each other, a
deterministic known answer, guided renders.  Light list of the five-light scene: 0 the emissive rectangle, 1 the distant light, 2 the
point light, 3 the projection light, 4 the goniometric light."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import imagelight_model as M
import pointlight_model as PM
import scenes

pytestmark = pytest.mark.gpu

f32 = np.float32
EPS = 2.0 ** -24
W, H = 32, 24
COLS = {"index": 0, "pmf": 1, "PMF": 2, "valid": 3, "wi": slice(4, 7), "L": slice(7, 10), "pdf": 10, "pLight": slice(11, 14), "delta": 14, "zero": 15}
SAMPLERS = ["uniform", "power", "bvh"]

POINT_I, POINT_FROM = (3.0, 2.0, 1.0), (0.2, 0.3, -0.1)
PROJ_I, PROJ_FOV = (6.0, 5.0, 4.0), 50.0
GONIO_I = (2.0, 3.0, 4.0)
QUAD_LE, SUN_L, SUN_W = (4.0, 3.0, 2.0), (3.0, 2.5, 2.0), (0.4, 0.8, -0.3)


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ctm_oblique():
    return PM.mat4_mul(PM.translate((0.3, -0.2, 0.5)), PM.rotate(37.0, (1, 2, 3)))


def ctm_down(at=(0.4, 1.5, -0.3)):
    """At `at`, the light's +z pointing down and a little forward: Translate * Rotate(100 degrees about x) sends +z to (0, -0.98, -0.17)."""
    return PM.mat4_mul(PM.translate(at), PM.rotate(100.0, (1, 0, 0)))


def with_kernel(kernel, fn):
    if kernel:
        os.environ["VSPG_KERNEL"] = kernel
    try:
        return fn()
    finally:
        os.environ.pop("VSPG_KERNEL", None)


def sampler_params(P, sampler, prm=None):
    prm = prm or P.app_f_params()
    prm.lightsampler = {"uniform": P.LIGHTSAMPLER_UNIFORM, "power": P.LIGHTSAMPLER_POWER, "bvh": P.LIGHTSAMPLER_BVH}[sampler]
    return prm


def vacuum_scene(P):
    s = scenes.empty_scene(W, H, eye=(0, 0.2, -3), look=(0, 0, 0))
    s.medium.type = P.MEDIUM_NONE
    s.camera_outside_medium = 1
    return s


SLIDE, MAP = M.slide(8, 6, 1), M.gonio_map(5, 3)


def add_image_lights(P, s, proj_ctm, gonio_ctm):
    """The projection and the goniometric light of this file; returns their point-light slots and their mirrors (holding the 1 x 1 image
    of ones, as a fresh renderer does)."""
    kp = P.add_projection_light(s, PROJ_I, fov=PROJ_FOV, ctm=proj_ctm)
    kg = P.add_goniometric_light(s, GONIO_I, ctm=gonio_ctm)
    return (kp, kg), (M.projection_light(PROJ_I, np.ones((1, 1, 3), f32), PROJ_FOV, proj_ctm), M.goniometric_light(GONIO_I, None, ctm=gonio_ctm))


def give_images(r, slots, mirrors, slide=SLIDE, gmap=MAP):
    r.set_light_image(slots[0], slide)
    r.set_light_image(slots[1], gmap)
    mirrors[0].set_image(slide)
    mirrors[1].set_image(gmap)


def five_light_scene(P, medium="none"):
    """An emissive rectangle over a floor, a distant light, a point light, the projector (above, shining down) and the goniometric light."""
    if medium == "grid":
        s = scenes.empty_scene(W, H, eye=(0.0, 0.6, -4.2), look=(0, 0.15, 0), fov=38.0)
        dens = np.array([0.2, 1, 0.7, 0.1, 0.9, 0.4, 1, 0.6], f32)
        m = s.medium
        m.type = P.MEDIUM_GRID
        m.sigma_a[:] = (0.03,) * 3
        m.sigma_s[:] = (2.97,) * 3
        m.g = 0.6
        m.nx = m.ny = m.nz = 2
        m.bounds_min[:] = (-0.8, -0.5, -0.8)
        m.bounds_max[:] = (0.8, 0.9, 0.8)
        m.density = dens.ctypes.data_as(C.POINTER(C.c_float))
        s._density_keepalive = dens
    else:
        s = vacuum_scene(P)
    scenes.add_quad(s, (-6, -1.25, -6), (0, 0, 12), (12, 0, 0), kd=(0.4, 0.35, 0.3))                 # floor, n = +y
    scenes.add_quad(s, (-1.5, 2.0, 0.5), (0.5, 0, 0), (0, 0, 0.5), kd=(0, 0, 0), le=QUAD_LE)         # emitter, n = -y, area 0.25
    P.add_infinite_light(s, P.LIGHT_DISTANT, SUN_L, SUN_W)
    P.add_point_light(s, POINT_I, POINT_FROM)
    slots, mirrors = add_image_lights(P, s, ctm_down(), ctm_oblique())
    return s, slots, mirrors


# ---- 1. the batch against the mirror, bit for bit ----------------------------------------------------------------------------------
def mirror_rows(got, p, lights_by_index):
    """The mirror's rows [3:16] for the lights the device picked; rows of other lights are copied from the device and not judged."""
    want = got.copy()
    idx = got[:, 0].astype(int)
    for li, light in lights_by_index.items():
        sel = idx == li
        valid, wi, L, pdf, pl, delta = light.sample_li(p[sel])
        rows = np.zeros((sel.sum(), 13), f32)
        rows[:, 0], rows[:, 1:4], rows[:, 4:7], rows[:, 7], rows[:, 8:11], rows[:, 11] = valid, wi, L, pdf, pl, delta
        rows[~valid] = 0
        want[sel, 3:] = rows
    return want


def assert_rows_equal(got, want, what):
    for name, c in COLS.items():
        bad = np.argwhere(u32(got[:, c]) != u32(want[:, c]))
        assert bad.size == 0, (what, name, len(bad), "first query", int(bad[0, 0]), got[bad[0, 0]], want[bad[0, 0]])


BATCH_LIGHTS = {
    "slide 8x6": lambda: M.projection_light((3, 2, 1), M.slide(8, 6, 1), fov=70.0, ctm=ctm_oblique()),
    "slide 6x8": lambda: M.projection_light((1, 2, 3), M.slide(6, 8, 2), fov=40.0, ctm=ctm_oblique()),
    "slide 1x1": lambda: M.projection_light((1, 1, 1), np.ones((1, 1, 3), f32), fov=90.0, ctm=ctm_oblique()),
    "map 5x5": lambda: M.goniometric_light((3, 2, 1), M.gonio_map(5, 3), ctm=ctm_oblique()),
    "map 64x64": lambda: M.goniometric_light((1, 2, 3), M.gonio_map(64, 4), scale=0.5, ctm=ctm_oblique()),
}


@pytest.mark.parametrize("which", list(BATCH_LIGHTS))
def test_batch_equals_the_mirror(gpu_pkg, which):
    """4096 contexts around one light (tests/imagelight_model.py::contexts_around: medium and surface contexts; inside the frustum, outside
    it on each side, behind the light, within 1e-6 of a texel edge and of the screen edge; 1e-3 and 1e3 units away).  The device's rows
    equal the float32 mirror's in every bit -- no context is set aside here: the mirror rounds where the device rounds."""
    P = gpu_pkg
    light = BATCH_LIGHTS[which]()
    s = vacuum_scene(P)
    if light.kind == M.LIGHT_PROJECTION:
        slot = P.add_projection_light(s, light.I, fov=light.fov, ctm=ctm_oblique())
    else:
        slot = P.add_goniometric_light(s, light.I, ctm=ctm_oblique())
    r = P.Renderer(s, P.app_f_params(), W, H)
    if which != "slide 1x1":      # (the 1 x 1 slide of ones is what a fresh renderer holds)
        r.set_light_image(slot, light.raw)
    p, nn, u, labels = M.contexts_around(light, 4096, 21)
    got = r.light_sample_batch(p, nn, u)
    r.close()
    assert np.all(got[:, 0] == 0) and np.all(got[:, 1] == 1) and np.all(got[:, 2] == 1)      # the scene's only light, pmf 1
    assert_rows_equal(got, mirror_rows(got, p, {0: light}), which)
    valid = got[:, 3] == 1
    counts = np.bincount(labels, minlength=8)
    if light.kind == M.LIGHT_PROJECTION:
        assert np.all(counts > 200), counts
        assert valid[labels == 0].sum() > 200 and not valid[(labels >= 1) & (labels <= 5)].any()
        assert 0 < valid[labels == 7].sum() < counts[7]      # at the screen edge: some in, some out
        if which != "slide 1x1":      # distinct texels: many different radiances per unit distance
            d2 = ((light.pos[None, :] - p) ** 2).sum(axis=1, dtype=f32)
            assert len(np.unique(np.round(got[valid, 7] * d2[valid], 3))) >= light.xres * light.yres - 2
    else:
        assert valid.all() and counts[0] > 200 and counts[6] > 200
    assert np.all(got[valid, 10] == 1) and np.all(got[valid, 14] == 1) and np.all(got[valid, 11:14] == light.pos)
    assert (got[valid, 3:][:, 12] == 0).all()
    dist = np.linalg.norm(p.astype(np.float64) - light.pos, axis=1)
    assert (dist < 2e-3).sum() > 200 and (dist > 500).sum() > 200
    assert (nn[valid] == 0).all(axis=1).sum() > 200 and (nn[valid] != 0).any(axis=1).sum() > 200      # medium and surface contexts


def test_goniometric_pole_is_clamped_not_wrapped(gpu_pkg):
    """Straight below a goniometric light without a CTM lies the map's southern pole, uv = (1, 1): the index leaves the image and the
    clamp shows the corner texel (3, 3) of a 4 x 4 map, where the octahedral wrap of the environment map would show (0, 1)."""
    P = gpu_pkg
    img = M.gonio_map(4, 7)
    light = M.goniometric_light((1, 1, 1), img)
    s = vacuum_scene(P)
    slot = P.add_goniometric_light(s, (1, 1, 1))
    r = P.Renderer(s, P.app_f_params(), W, H)
    r.set_light_image(slot, img)
    rr = np.array([0.25, 0.5, 1, 2, 4, 8], f32)
    p = np.stack([rr * f32(1e-6), -rr, rr * f32(1e-6)], axis=1).astype(f32)
    got = r.light_sample_batch(p, np.zeros_like(p), np.zeros_like(p))
    r.close()
    assert np.array_equal(got[:, 7], img[3, 3] / (rr * rr)) and np.all(got[:, 7] != img[1, 0] / (rr * rr))
    assert_rows_equal(got, mirror_rows(got, p, {0: light}), "pole")


# ---- 2. the three samplers over the five lights ------------------------------------------------------------------------------------
def scene_radius(corners):
    """Bounds3::BoundingSphere of the scene bounds, in float32 as the host computes it."""
    c = np.asarray(corners, f32)
    lo, hi = c.min(axis=0), c.max(axis=0)
    d = (lo + hi) / f32(2) - hi
    return np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])


# the first lies in the projector's beam, 1.2 units along its axis; the last above the projector, outside its bounding cone
def sampler_contexts():
    proj = M.projection_light(PROJ_I, np.ones((1, 1, 3), f32), PROJ_FOV, ctm_down())
    on_axis = (proj.pos.astype(np.float64) + 1.2 * proj.axis).astype(f32)
    return np.array([on_axis, [-1.2, 1.0, 0.7], [0.5, -1.0, 0.3], [0.4, 3.0, -0.3]], f32)


BRIGHT_SLIDE = (M.slide(8, 6, 1) * f32(16)).astype(f32)


def sampler_batches(P, sampler, steps):
    """Per step of `steps` (each a function of (renderer, slots, mirrors) run first): the batches of 2^14 stratified picks for each of
    four contexts (two as medium vertices, two with a normal), and the mirrors as they stand after the last step."""
    n = 1 << 14
    u = np.zeros((n, 3), f32)
    u[:, 0] = ((np.arange(n) + 0.5) / n).astype(f32)
    u[:, 1:] = np.random.default_rng(2).random((n, 2)).astype(f32)
    normals = np.array([[0, 0, 0], [0, 0, 0], [0, 1, 0], [0.6, -0.8, 0]], f32)
    s, slots, mirrors = five_light_scene(P)
    r = P.Renderer(s, sampler_params(P, sampler), W, H)
    out = []
    for step in steps:
        step(r, slots, mirrors)
        out.append([r.light_sample_batch(np.broadcast_to(c, (n, 3)), np.broadcast_to(nn, (n, 3)), u) for c, nn in zip(sampler_contexts(), normals)])
    r.close()
    return out, mirrors


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_sampler_consistency(gpu_pkg, sampler):
    P = gpu_pkg
    n = 1 << 14
    (first, live), mirrors = sampler_batches(P, sampler, [give_images, lambda r, slots, mirrors: r.set_light_image(slots[0], BRIGHT_SLIDE)])
    (fresh,), _ = sampler_batches(P, sampler, [lambda r, slots, mirrors: give_images(r, slots, mirrors, slide=BRIGHT_SLIDE)])
    proj, gonio = mirrors
    ctx = sampler_contexts()
    # the projector's bounding cone: context 3 sits above the light, further than theta_e from its axis; context 0 on the axis
    pos, axis, phi, cos_o, cos_e = proj.bounds()
    to_ctx = ctx[3].astype(np.float64) - pos
    assert cos_o == 1 and math.acos(float(to_ctx @ axis / np.linalg.norm(to_ctx))) > math.acos(float(cos_e)) + 0.2
    to_ctx = ctx[0].astype(np.float64) - pos
    assert math.acos(min(1.0, float(to_ctx @ axis / np.linalg.norm(to_ctx)))) < 0.01
    pmfs = []
    for k, got in enumerate(first):
        picked = got[:, 0] >= 0
        assert picked.all() or sampler == "bvh"
        g = got[picked]
        assert np.array_equal(u32(g[:, 1]), u32(g[:, 2])), (sampler, k, "Sample's pmf is not PMF(ctx, light)")
        idx = g[:, 0].astype(int)
        pmf = np.zeros(5)
        for li in range(5):
            vals = np.unique(g[idx == li, 1])
            assert len(vals) <= 1, (sampler, k, li, vals)      # one context, one light: one pmf
            pmf[li] = vals[0] if len(vals) else 0.0
        pmfs.append(pmf)
        count = np.bincount(idx, minlength=5)
        for li in range(5):      # picks reproduce the pmf: 4.5 binomial standard deviations (the stratified variates stay far inside)
            sd = math.sqrt(n * pmf[li] * (1 - pmf[li]))
            assert abs(count[li] - n * pmf[li]) <= 4.5 * sd + 1, (sampler, k, li, count[li], n * pmf[li])
        if sampler == "uniform":
            assert np.all(pmf == f32(1) / f32(5))
        if sampler == "bvh":
            # the one infinite light has pInfinite = 1 / 2; where every bounded light has a positive importance the pmfs sum to 1
            # (8 ulp: a product of at most three quotients per light, five terms)
            assert pmf[1] == f32(0.5)
            if picked.all() and np.all(pmf > 0):
                assert abs(pmf.sum() - 1) <= 8 * 2 * EPS, (k, pmf)
            if k == 3:
                assert count[3] == 0 and count[2] > 0 and count[4] > 0, count      # outside the projector's cone; the bulbs shine everywhere
            if k == 0:
                assert np.all(count > 0)
    if sampler == "power":
        r = scene_radius([(-6, -1.25, -6), (6, -1.25, 6), (-1.5, 2.0, 0.5), (-1.0, 2.0, 1.0)])
        point = PM.point_light(POINT_I, POINT_FROM)
        proj.set_image(SLIDE)
        phis = [PM.PI * f32(0.25) * np.array(QUAD_LE, f32), PM.PI * (r * r) * np.array(SUN_L, f32), point.phi(), proj.phi(), gonio.phi()]
        want = PM.power_pmf(phis)
        got_pmf = np.array([np.unique(np.concatenate([g[g[:, 0] == li, 1] for g in first])) for li in range(5)]).reshape(5)
        ulp = np.abs(u32(got_pmf).astype(np.int64) - u32(want).astype(np.int64))
        print("power pmf", got_pmf, "model", want, "ulp", ulp)
        assert np.all(ulp <= 2)
        proj.set_image(BRIGHT_SLIDE)
        phis[3] = proj.phi()
        want = PM.power_pmf(phis)
        got_pmf = np.array([np.unique(np.concatenate([g[g[:, 0] == li, 1] for g in live])) for li in range(5)]).reshape(5)
        assert np.all(np.abs(u32(got_pmf).astype(np.int64) - u32(want).astype(np.int64)) <= 2) and got_pmf[3] > first[0][first[0][:, 0] == 3, 1][0]
    # after set_light_image with the brighter slide: the rows of a renderer created and given that slide from the start, bit for bit
    for a, b in zip(live, fresh):
        assert np.array_equal(u32(a), u32(b))
    if sampler != "uniform":      # ... and the brighter slide is picked more often where it shines
        assert (live[0][:, 0] == 3).sum() > (first[0][:, 0] == 3).sum()


# ---- 3. a goniometric light with the 1 x 1 image is a point light ------------------------------------------------------------------
def family_scene(P, which, lights):
    """The media of tests/test_pointlight_gpu.py::family_scene; `lights(P, s)` adds the lights."""
    if which == "homogeneous":
        s = scenes.empty_scene(W, H, eye=(0, 0.3, -3), look=(0, 0, 0))
        m = s.medium
        m.type = P.MEDIUM_HOMOGENEOUS
        m.sigma_a[:] = (0.05, 0.05, 0.05)
        m.sigma_s[:] = (0.4, 0.4, 0.4)
        m.g = 0.3
        tp, tk = scenes.heightfield_triangles(4, x0=-4, x1=4, z0=-4, z1=4, y=-0.8)
        P.set_triangles(s, tp, tk)
    elif which == "grid":
        s = five_light_scene(P, "grid")[0]
        s.n_infinite_lights = 0
        s.n_point_lights = 0
        s.n_quads = 1      # the floor
    else:
        dens = np.array([0.2, 1, 0.7, 0.1, 0.9, 0.4, 1, 0.6], f32)
        s = scenes.cloud_scene(W, H, dens, 2, sigma_t=3.0, albedo=0.99, g=0.6, sphere=True, ground=True, sun=False, sky=False)
    return s, lights(P, s)


def render(P, scene, prm, kernel, waves=3, prepare=None):
    def go():
        r = P.Renderer(scene, prm, W, H)
        if prepare:
            prepare(r)
        name = r.kernel_name()
        for w in range(waves):
            r.render_wave(w, w + 1)
            r.post_process_wave()
        out = name, r.film(), r.counters()
        r.close()
        return out
    return with_kernel(kernel, go)


def counters_tuple(c):
    return tuple(sorted(c.items()))


@pytest.mark.parametrize("kernel", [None, "lane"])
@pytest.mark.parametrize("which", ["homogeneous", "grid", "grid_boundary"])
def test_goniometric_1x1_is_a_point_light(gpu_pkg, which, kernel):
    """Same I, same position (the swapped transform under a CTM that translates to the point light's `from`): batch rows, films and
    counters are the point light's bit for bit, on the default and the per-lane kernel."""
    P = gpu_pkg
    at = (0.2, 0.45, -0.1)
    ctm = PM.mat4_mul(PM.translate(at), PM.rotate(37.0, (1, 2, 3)))
    sg, _ = family_scene(P, which, lambda P, s: P.add_goniometric_light(s, POINT_I, scale=0.5, power=9.0, ctm=ctm))
    sp, _ = family_scene(P, which, lambda P, s: P.add_point_light(s, POINT_I, at, scale=0.5, power=9.0))
    assert np.array_equal(u32(np.array(sg.point_lights[0].I[:], f32)), u32(np.array(sp.point_lights[0].I[:], f32)))
    prm = sampler_params(P, "bvh")
    name_g, film_g, cnt_g = render(P, sg, prm, kernel)
    name_p, film_p, cnt_p = render(P, sp, prm, kernel)
    print(which, kernel, name_g)
    assert name_g == name_p and np.isfinite(film_g).all() and film_g[..., :3].max() > 0
    assert np.array_equal(u32(film_g), u32(film_p)) and counters_tuple(cnt_g) == counters_tuple(cnt_p)
    if kernel is None:
        light = M.goniometric_light(POINT_I, None, scale=0.5, power=9.0, ctm=ctm)
        p, nn, u, _ = M.contexts_around(light, 1024, 3)
        rows = []
        for s in (sg, sp):
            r = P.Renderer(s, prm, W, H)
            rows.append(r.light_sample_batch(p, nn, u))
            r.close()
        assert np.array_equal(u32(rows[0]), u32(rows[1])) and (rows[0][:, 3] == 1).sum() > 100


# ---- 4. kernel families ----------------------------------------------------------------------------------------------------------------
def both_lights(P, s):
    return add_image_lights(P, s, ctm_down((0.1, 1.2, -0.2)), PM.mat4_mul(PM.translate((-0.3, 0.4, 0.2)), PM.rotate(37.0, (1, 2, 3))))


@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("which", ["homogeneous", "grid", "grid_boundary"])
def test_kernel_families_agree(gpu_pkg, which, sampler):
    """A real slide and a real goniometric map: the default kernel's film equals the per-lane kernel's bit for bit."""
    P = gpu_pkg
    scene, (slots, mirrors) = family_scene(P, which, both_lights)
    prm = sampler_params(P, sampler)
    name_d, film_d, cnt_d = render(P, scene, prm, None, prepare=lambda r: give_images(r, slots, mirrors))
    name_l, film_l, cnt_l = render(P, scene, prm, "lane", prepare=lambda r: give_images(r, slots, mirrors))
    print(which, sampler, "default:", name_d, "| lane:", name_l)
    assert name_d != name_l and name_l.startswith("k_render_wave<")
    assert name_d.startswith("k_render_wave_wg2<HomogeneousMedium>" if which == "homogeneous" else "k_wf_")
    assert np.isfinite(film_d).all() and film_d[..., :3].max() > 0
    assert np.array_equal(u32(film_d), u32(film_l)) and counters_tuple(cnt_d) == counters_tuple(cnt_l)
    # ... and the images are in it: the same scene under the 1 x 1 images gives another film
    _, film_1, _ = render(P, scene, prm, None)
    assert not np.array_equal(u32(film_d), u32(film_1))


# ---- 5. a known answer, deterministic ---------------------------------------------------------------------------------------------------
KW, KH = 64, 48


def pixel_corner_dirs(scene, w, h):
    """Unit directions of the camera rays through the corners of every pixel: (h + 1, w + 1, 3), float64."""
    c = scene.camera
    x, y = np.meshgrid(np.arange(w + 1, dtype=np.float64), np.arange(h + 1, dtype=np.float64))
    v = np.stack([c.sx * x + c.ox, c.sy * y + c.oy, np.ones_like(x)], axis=-1)
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    return v[..., 0:1] * np.array(c.right[:]) + v[..., 1:2] * np.array(c.up[:]) + v[..., 2:3] * np.array(c.fwd[:])


@pytest.mark.parametrize("light", ["projection", "goniometric"])
def test_light_at_the_centre_of_a_diffuse_sphere(gpu_pkg, light):
    """A diffuse sphere of radius R around the camera and the light, a medium with zero coefficients, maxdepth 1: a pixel of one wave is
    direct light alone, Kd / pi * I * texel / R^2 * |cos| with cos = 1 (the light sits on every normal), weight 1 -- wherever the
    pixel's whole footprint falls inside one texel's solid angle, whichever point of the pixel the sample took.  The bound is
    tests/test_pointlight_gpu.py::test_light_at_the_centre_of_a_diffuse_sphere's 2 (2 sqrt(3) gamma(5) + 2 eps) + 16 eps with one more
    product, I * texel: + 1 eps.
    The projector (2 x 2 slide, fov 60, no CTM: it looks along +z like the camera, whose fov is 70) lights a square of 39.6 x 39.6 pixels
    in the middle of the 64 x 48 film, a quadrant per texel, the slide's top row upwards; a pixel wholly outside the frustum is an
    exact 0.  Pixels whose footprint touches a texel edge or the frustum's are set aside: computed here from the camera and the slide,
    at most 25 % of the lit pixels.  The goniometric light (2 x 2 map, no CTM) sees render (x, y, z) as the map's (x, z, y): the camera
    looks along the map's +y, so v = 0.5 (1 + sign(y) ...) > 0.5 in both hemispheres -- the map's bottom row -- and u = 0.5 (1 + sign(x)
    ...) puts the film's left half on texel (0, 1) and its right half on (1, 1); only the pixels of the middle column are set aside."""
    P = gpu_pkg
    R, Kd, I = 1.75, (0.5, 0.25, 0.75), (3.0, 2.0, 1.0)
    s = scenes.empty_scene(KW, KH, eye=(0, 0, 0), look=(0, 0, 1), fov=70.0)
    s.medium.type = P.MEDIUM_HOMOGENEOUS
    scenes.add_sphere(s, (0, 0, 0), R, kd=Kd)
    d = pixel_corner_dirs(s, KW, KH)
    corners = lambda a: np.stack([a[:-1, :-1], a[1:, :-1], a[:-1, 1:], a[1:, 1:]])
    margin = 1e-4
    if light == "projection":
        img = np.array([[[1, 0.5, 0.25], [0.25, 1, 0.5]], [[0.5, 0.25, 1], [1, 1, 0.125]]], f32)      # four distinct colours
        slot = P.add_projection_light(s, I, fov=60.0)
        t = 1.0 / math.tan(math.radians(30.0))
        sx, sy = corners(t * d[..., 0] / d[..., 2]), corners(-t * d[..., 1] / d[..., 2])      # screen coordinates: the flip turns +y up into v < 0.5
        out = (np.abs(sx) > 1 + margin) | (np.abs(sy) > 1 + margin)
        dark = ((sx > 1 + margin).all(axis=0) | (sx < -1 - margin).all(axis=0) | (sy > 1 + margin).all(axis=0) | (sy < -1 - margin).all(axis=0))
        inside = ((np.abs(sx) < 1 - margin) & (np.abs(sy) < 1 - margin)).all(axis=0)
        tx = np.where((sx > margin).all(axis=0), 1, np.where((sx < -margin).all(axis=0), 0, -1))
        ty = np.where((sy > margin).all(axis=0), 1, np.where((sy < -margin).all(axis=0), 0, -1))
        clean = inside & (tx >= 0) & (ty >= 0)
        lit = ~dark
        texel = img[np.clip(ty, 0, 1), np.clip(tx, 0, 1)]
    else:
        img = np.array([[0.5, 1.5], [2.5, 3.5]], f32)
        slot = P.add_goniometric_light(s, I)
        mx, my, mz = corners(d[..., 0]), corners(d[..., 2]), corners(d[..., 1])      # map space = (x, z, y) of render space
        assert (my > 0.3).all()      # the camera looks along map +y: every pixel has v > 0.5, the map's bottom row
        tx = np.where((mx > margin).all(axis=0), 1, np.where((mx < -margin).all(axis=0), 0, -1))
        clean = tx >= 0
        dark = np.zeros((KH, KW), bool)
        lit = np.ones((KH, KW), bool)
        texel = np.repeat(img[1, np.clip(tx, 0, 1)][..., None], 3, axis=-1)
    set_aside = lit & ~clean
    print(light, "lit", lit.sum(), "clean", clean.sum(), "set aside", set_aside.sum(), "dark", dark.sum())
    assert clean.sum() > 400 and set_aside.sum() <= 0.25 * lit.sum()
    if light == "projection":
        assert dark.sum() > 400 and all(((tx == a) & (ty == b) & clean).sum() > 100 for a in (0, 1) for b in (0, 1))
    prm = P.app_f_params()
    prm.maxdepth = 1
    gamma5 = 5 * EPS / (1 - 5 * EPS)
    bound = 2 * (2 * math.sqrt(3) * gamma5 + 2 * EPS) + 17 * EPS
    want = np.array(Kd) / math.pi * np.array(I) * texel.astype(np.float64) / (R * R)
    names = []
    for kernel in (None, "lane"):
        def go():
            r = P.Renderer(s, prm, KW, KH)
            r.set_light_image(slot, img)
            r.render_wave(0, 1)
            out = r.kernel_name(), r.film()
            r.close()
            return out
        name, film = with_kernel(kernel, go)
        names.append(name)
        assert np.all(film[..., 3] == 1)
        err = np.abs(film[..., :3][clean] / want[clean] - 1).max()
        print(light, name, "relative error %.3g (bound %.3g)" % (err, bound))
        assert err <= bound
        assert np.all(film[..., :3][dark] == 0)
    assert names[0] != names[1] and names[1].startswith("k_render_wave<")


# ---- 6. a known answer, statistical: the projector in fog ---------------------------------------------------------------------------
def fog_projector_scene(P, F):
    s = scenes.empty_scene(F.W, F.H, eye=F.eye, look=F.look, up=F.up, fov=F.fov)
    m = s.medium
    m.type = P.MEDIUM_HOMOGENEOUS
    m.sigma_a[:] = (F.sigma_a,) * 3
    m.sigma_s[:] = (F.sigma_s,) * 3
    m.g = F.g
    scenes.add_quad(s, (-6, -6, F.z_wall), (12, 0, 0), (0, 12, 0), kd=(0, 0, 0))      # the black backdrop every camera ray ends on
    slot = P.add_projection_light(s, F.I, fov=F.proj_fov, ctm=F.ctm())
    return s, slot


def test_projector_in_fog_agrees_with_the_quadrature(gpu_pkg):
    """Single scattering by NEE alone (maxdepth 1, nothing else emits, the backdrop is black), a 2 x 2 slide of four distinct colours: the
    means of the four film quadrants over 32 separately cleared waves against the float64 quadrature of
    tests/imagelight_model.py::FogProjector, |z| <= 4.5 each with the standard error taken from the spread over the waves -- the
    construction and the threshold of tests/test_pointlight_gpu.py::test_spot_in_fog_agrees_with_the_quadrature.
    tests/test_imagelight_model.py shows on the CPU that the quadrature's own error is below a tenth of that standard error, that the
    no-Y-flip and the m-for-mInv planted errors each move a quadrant by more than ten of them, and that the camera rays keep 0.5 units
    away from the light."""
    P = gpu_pkg
    F = M.FogProjector()
    prm = P.app_f_params()
    prm.maxdepth = 1
    s, slot = fog_projector_scene(P, F)
    r = P.Renderer(s, prm, F.W, F.H)
    r.set_light_image(slot, F.SLIDE)
    waves = []
    for w in range(F.WAVES):
        r.film_clear()
        r.render_wave(w, w + 1)
        f = r.film()
        assert np.all(f[..., 3] == 1)
        waves.append(F.quadrant_means(f))
    name = r.kernel_name()
    r.close()
    waves = np.array(waves)
    mean, se = waves.mean(axis=0), waves.std(axis=0, ddof=1) / math.sqrt(F.WAVES)
    want = F.quadrant_means(F.pixel_means(4, 256))
    z = (mean - want) / se
    print(name, "quadrant means", mean, "+-", se, "model", want, "z", z)
    assert np.all(se > 0) and np.all(np.abs(z) <= 4.5), z


# ---- 7. set_light_image on a live renderer -------------------------------------------------------------------------------------------
def test_set_light_image_on_a_live_renderer(gpu_pkg):
    """Two waves under the 1 x 1 images, then the images, then waves 2 and 3 into a cleared film: film and counters (their growth) equal
    those of a renderer given the images before its first wave, bit for bit.  The call itself leaves film and counters as they were.
    (No post_process_wave: the image-space VSP estimate it refreshes is state the first two waves would hand to the later ones.)"""
    P = gpu_pkg
    scene, (slots, mirrors) = family_scene(P, "homogeneous", both_lights)
    prm = sampler_params(P, "power")
    live = P.Renderer(scene, prm, W, H)
    for w in range(2):
        live.render_wave(w, w + 1)
    film_before, cnt_before = live.film(), counters_tuple(live.counters())
    give_images(live, slots, mirrors)
    assert np.array_equal(u32(live.film()), u32(film_before)) and counters_tuple(live.counters()) == cnt_before      # what the call keeps
    live.film_clear()
    for w in range(2, 4):
        live.render_wave(w, w + 1)
    film_live, cnt_live = live.film(), counters_tuple(live.counters())
    live.close()
    fresh = P.Renderer(scene, prm, W, H)
    give_images(fresh, slots, mirrors)
    for w in range(2, 4):
        fresh.render_wave(w, w + 1)
    film_fresh, cnt_fresh = fresh.film(), counters_tuple(fresh.counters())
    fresh.close()
    assert film_live[..., :3].max() > 0 and np.array_equal(u32(film_live), u32(film_fresh))
    growth = tuple((k, a - b) for (k, a), (_, b) in zip(cnt_live, cnt_before))
    assert growth == cnt_fresh and dict(cnt_fresh)["paths"] == 2 * W * H


def test_set_light_image_refusals_leave_the_renderer_unchanged(gpu_pkg):
    P = gpu_pkg
    lib = P.load()
    s, slots, mirrors = five_light_scene(P)      # point-light slots: 0 the point light, 1 the projector, 2 the goniometric light
    r = P.Renderer(s, sampler_params(P, "power"), W, H)
    give_images(r, slots, mirrors)
    p, nn, u, _ = M.contexts_around(mirrors[0], 1024, 4)
    before = r.light_sample_batch(p, nn, u)
    fp = C.POINTER(C.c_float)
    rgb, y = np.ones((4, 4, 3), f32), np.ones((4, 4), f32)
    nan_rgb, inf_y = rgb.copy(), y.copy()
    nan_rgb[2, 1, 0], inf_y[3, 3] = np.nan, np.inf

    def call(slot, img, xres, yres, channels, renderer=r.h):
        return lib.vspg_renderer_set_light_image(renderer, slot, None if img is None else img.ctypes.data_as(fp), xres, yres, channels, None)
    cases = [("null argument", call(slots[0], None, 4, 4, 3)), ("null argument", call(slots[0], rgb, 4, 4, 3, renderer=None)),
             ("no point-light slot", call(-1, rgb, 4, 4, 3)), ("no point-light slot", call(3, rgb, 4, 4, 3)),
             ("neither a projection nor a goniometric", call(0, rgb, 4, 4, 3)),
             ("3 channels", call(slots[0], y, 4, 4, 1)), ("1 channel", call(slots[1], rgb, 4, 4, 3)),
             ("resolution", call(slots[0], rgb, 0, 4, 3)), ("resolution", call(slots[0], rgb, 4, P.LIGHT_IMAGE_MAX_RES + 1, 3)),
             ("non-square", call(slots[1], y, 8, 2, 1)),
             ("not-a-number", call(slots[0], nan_rgb, 4, 4, 3)), ("infinite", call(slots[1], inf_y, 4, 4, 1))]
    # (each call's message is read right after it: evaluate them one by one)
    for needle, rc in cases:
        assert rc == P.VSPG_EINVAL, needle
    for needle, args in (("3 channels", (slots[0], y, 4, 4, 1)), ("non-square", (slots[1], y, 8, 2, 1)), ("not-a-number", (slots[0], nan_rgb, 4, 4, 3)),
                         ("neither a projection", (0, rgb, 4, 4, 3)), ("no point-light slot", (3, rgb, 4, 4, 3))):
        assert call(*args) == P.VSPG_EINVAL and needle in lib.vspg_last_error().decode(), lib.vspg_last_error()
    assert np.array_equal(u32(r.light_sample_batch(p, nn, u)), u32(before))
    with pytest.raises(ValueError):
        r.set_light_image(slots[0], rgb.astype(np.float64))
    r.set_light_image(slots[0], np.ascontiguousarray(rgb[:2]))      # a 4 x 2 slide is fine; the rows change
    assert not np.array_equal(u32(r.light_sample_batch(p, nn, u)), u32(before))
    r.close()


# ---- 8. guided ----------------------------------------------------------------------------------------------------------------------------
def test_guided_training_runs_and_kernels_agree(gpu_pkg):
    """Reference-default options on the grid behind its interface sphere with both lights: four training waves run, stay finite and
    leave a field with fitted regions; then, as tests/test_pointlight_gpu.py compares guided kernels, wave 4 with that field and that VSP
    buffer in place on the pipeline and on the per-lane kernel, bit for bit."""
    P = gpu_pkg
    scene, (slots, mirrors) = family_scene(P, "grid_boundary", both_lights)
    prm = P.default_params()
    prm.guide_num_training_waves = 4
    t = P.Renderer(scene, prm, W, H)
    give_images(t, slots, mirrors)
    assert "train" in t.kernel_name()
    for w in range(4):
        t.render_wave(w, w + 1)
        t.post_process_wave()
    assert np.isfinite(t.film()).all() and t.film()[..., :3].max() > 0
    st = t.training_stats()
    assert st["training"] == 0 and st["iteration"] == 4, st
    fields = []
    for vol in (0, 1):
        nodes, regs, nn, nr = t.get_guiding_field(vol)
        fields.append(P.Field(list(nodes)[:nn], list(regs)[:nr]))
    assert nr >= 1 and any(regs[i].n_lobes > 0 for i in range(nr)), "the volume field holds no fitted region"
    vsp, ready = t.vsp_buffer()
    t.close()
    films = {}
    for kernel in (None, "lane"):
        def wave4():
            r = P.Renderer(scene, prm, W, H)
            give_images(r, slots, mirrors)
            r.set_guiding_field(fields[0], fields[1])
            if ready:
                r.load_vsp_buffer(vsp)
            r.render_wave(4, 5)
            out = r.kernel_name(), r.film()
            r.close()
            return out
        name, film = with_kernel(kernel, wave4)
        films[name] = film
    print("guided kernels compared:", sorted(films))
    assert len(films) == 2 and any(n.startswith("k_render_wave<") for n in films) and any(n.startswith("k_wf_") for n in films)
    fa, fb = films.values()
    assert np.isfinite(fa).all() and fa[..., :3].max() > 0
    assert np.array_equal(u32(fa), u32(fb))


# ---- 9. the scene-file route ----------------------------------------------------------------------------------------------------------
def test_scene_file_image_lights(gpu_pkg, tmp_path):
    """tests/scenes/fog_box.pbrt with a LightSource "projection" and a LightSource "goniometric" under Translate / Rotate CTMs and
    generated PFM images, through vspg_pbrt, against the same scene built with the binding: the films are equal bit for bit."""
    import subprocess
    import exr_model as X
    from conftest import ROOT
    P = gpu_pkg
    host = os.path.join(ROOT, "vspg-pbrt-v4_amd", "host")
    exe = os.path.join(host, "vspg_pbrt")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", host])
    lines = open(os.path.join(ROOT, "tests", "scenes", "fog_box.pbrt")).read().splitlines()
    at = [i for i, l in enumerate(lines) if l.startswith("WorldBegin")][0]
    X.write_pfm(str(tmp_path / "slide.pfm"), SLIDE)
    X.write_pfm(str(tmp_path / "map.pfm"), MAP)
    lights = ['AttributeBegin', '  Translate 0.1 0.7 -0.6', '  Rotate 100 1 0 0',
              '  LightSource "projection" "float scale" 6 "float fov" 50 "string filename" "slide.pfm"', 'AttributeEnd',
              'AttributeBegin', '  Translate 0.3 -0.2 0.5', '  Rotate 37 1 2 3',
              '  LightSource "goniometric" "rgb I" [ 2 3 4 ] "float scale" 0.5 "float power" 10 "string filename" "map.pfm"', 'AttributeEnd']
    scene = tmp_path / "lights.pbrt"
    scene.write_text("\n".join(lines[:at + 1] + lights + lines[at + 1:]) + "\n")
    out = tmp_path / "lights.pfm"
    a = subprocess.run([exe, str(scene), "--outfile", str(out), "--spp", "3"], capture_output=True, text=True, timeout=120)
    assert a.returncode == 0, a.stdout + a.stderr
    got = X.read_pfm(str(out))
    s = P.fog_box_scene(64, 48)
    kp = P.add_projection_light(s, (6, 6, 6), fov=50, ctm=ctm_down((0.1, 0.7, -0.6)))
    kg = P.add_goniometric_light(s, (2, 3, 4), scale=0.5, power=10.0, ctm=ctm_oblique(), image=MAP)

    def film(images):
        r = P.Renderer(s, P.app_f_params(), 64, 48)
        if images:
            r.set_light_image(kp, SLIDE)
            r.set_light_image(kg, MAP)
        for w in range(3):
            r.render_wave(w, w + 1)
            r.post_process_wave()
        f = r.film()
        r.close()
        return f
    f = film(True)
    want = (f[..., :3] / f[..., 3:4]).astype(f32)
    assert want.max() > 0 and np.array_equal(u32(got), u32(want))
    assert not np.array_equal(u32(film(False)), u32(f))      # ... and the images are in it
