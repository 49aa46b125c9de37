"""The portal image infinite light on the device: vspg_portallight_batch and the table read-back against the float32 mirror of
tests/portallight_model.py bit for bit (trip counts of the hoisted bisection included), the light through whole paths (kernel families
against each other, a deterministic and a statistical known answer, NEE against escaping rays only, a hemisphere-wide portal against the
plain image light), and vspg_renderer_set_portal_environment_image on a live renderer.  Fixtures: portallight_model.CASES."""
import math
import os

import numpy as np
import pytest

import portallight_model as M
import scenes

pytestmark = pytest.mark.gpu

f32 = np.float32
SKY_L = M.L_RGB
# the room's ceiling opening (y = 1), vertices in the order that makes portalFrame's z point out of the room (+y)
ROOM_PORTAL = np.array([[-0.4, 1, -0.3], [0.4, 1, -0.3], [0.4, 1, 0.3], [-0.4, 1, 0.3]], f32)


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def with_kernel(kernel, fn):
    if kernel:
        os.environ["VSPG_KERNEL"] = kernel
    try:
        return fn()
    finally:
        os.environ.pop("VSPG_KERNEL", None)


def sky_only_scene(P, w=8, h=8, eye=(0, 0.2, -3), look=(0, 0, 0), fov=40.0):
    s = scenes.empty_scene(w, h, eye=eye, look=look, fov=fov)
    s.medium.type = P.MEDIUM_NONE
    s.camera_outside_medium = 1
    P.add_infinite_light(s, P.LIGHT_IMAGE_INFINITE, SKY_L)
    return s


@pytest.fixture(scope="module")
def batch_renderer(gpu_pkg):
    r = gpu_pkg.Renderer(sky_only_scene(gpu_pkg), gpu_pkg.app_f_params(), 8, 8)
    yield r
    r.close()


@pytest.fixture(scope="module")
def lights():
    return {c[0]: M.make_light(c) for c in M.CASES}


COLS = {"bounds": slice(0, 5), "Le inside": slice(5, 6), "Le uv": slice(6, 8), "Le": slice(8, 11), "PDF_Li": slice(11, 12), "sample valid": slice(12, 13),
        "sample uv": slice(13, 15), "mapPDF": slice(15, 16), "duv_dw": slice(16, 17), "wi": slice(17, 20), "pdf": slice(20, 21), "L": slice(21, 24),
        "trips": slice(24, 26), "why": slice(26, 27), "pLight": slice(27, 30), "unused": slice(30, 32)}


def assert_batch_equals_mirror(got, want, what):
    for name, c in COLS.items():
        bad = np.argwhere(u32(got[:, c]) != u32(want[:, c]))
        assert bad.size == 0, (what, name, len(bad), "first query", int(bad[0, 0]), got[bad[0, 0]], want[bad[0, 0]])


# 1. the device arithmetic and the tables, bit for bit
@pytest.mark.parametrize("case", M.CASES, ids=[c[0] for c in M.CASES])
def test_batch_and_tables_equal_the_mirror(gpu_pkg, batch_renderer, lights, case):
    light = lights[case[0]]
    r = batch_renderer
    r.set_portal_environment_image(0, light.src, light.portal, M.rotated() if case[4] else None)
    t = r.portallight_tables(0)
    rec = {"p0": light.p0, "p2": light.p2, "frame": np.stack([light.fx, light.fy, light.fz]), "area": light.area, "sum_phi": light.sum_phi,
           "image": light.image, "func": light.func, "table": light.table}
    assert t["res"] == light.res
    for k, want in rec.items():
        assert np.array_equal(u32(t[k]), u32(np.asarray(want, f32).reshape(np.shape(t[k])))), (case[0], k)
    p, d, u = M.make_queries(light, M.N_QUERIES, 100 + case[3])
    got = r.portallight_batch(0, p, d, u)
    light.scene_radius = f32(t["scene_radius"])     # pLight = ctx.p + 2 * sceneRadius * wi with the renderer's own radius
    want = light.batch(p, d, u)
    print(case[0], "samples %d of %d, max trips %d / %d, why %s" % ((want[:, 12] == 1).sum(), len(want), want[:, 24].max(), want[:, 25].max(),
                                                                  np.bincount(want[:, 26].astype(int), minlength=6)))
    assert_batch_equals_mirror(got, want, case[0])
    ok = got[:, 12] == 1
    assert np.all(got[~ok, 13:24] == 0) and np.all(got[~ok, 27:30] == 0)


def test_nan_inputs_read_inside_the_tables(gpu_pkg, batch_renderer, lights):
    """NaN context points, directions and variates: every index is clamped, nothing is sampled from a NaN bracket, nothing faults."""
    light = lights["16 peaked"]
    r = batch_renderer
    r.set_portal_environment_image(0, light.src, light.portal, None)
    p, d, u = M.make_queries(light, 96, 3)
    p[0::4, 1] = np.nan
    d[1::4, 0] = np.nan
    u[2::4, 0] = np.nan
    u[3::8, 1] = np.nan
    got = r.portallight_batch(0, p, d, u)
    assert np.all(got[0::4, 0] == 0) and np.all(got[0::4, 12] == 0) and np.all(got[0::4, 8:12] == 0)
    assert np.all(got[1::4, 5] == 0) and np.all(got[1::4, 8:11] == 0)
    nanu = np.isnan(u).any(axis=1) & (got[:, 0] == 1)
    assert nanu.any() and np.all(got[nanu, 12] == 0) and np.all(got[nanu, 26] == M.WHY_BAD_T)
    assert np.all(got[:, 24:26] < M.BISECT_CAP)


# 2. whole paths: the room with a rectangular opening in its ceiling
def room_scene(P, W, H, medium):
    """A box [-1, 1]^3 of diffuse walls whose ceiling has the opening ROOM_PORTAL, the camera inside, fog in the room."""
    s = scenes.empty_scene(W, H, eye=(0.0, -0.2, -0.95), look=(0, 0.1, 0.2), fov=70.0)
    q = scenes.add_quad
    q(s, (-1, -1, -1), (0, 0, 2), (2, 0, 0), kd=(0.6, 0.6, 0.6))      # floor
    q(s, (-1, -1, 1), (0, 2, 0), (2, 0, 0), kd=(0.7, 0.4, 0.4))       # far wall
    q(s, (-1, -1, -1), (0, 2, 0), (2, 0, 0), kd=(0.5, 0.5, 0.5))      # wall behind the camera
    q(s, (-1, -1, -1), (0, 2, 0), (0, 0, 2), kd=(0.4, 0.7, 0.4))      # left
    q(s, (1, -1, -1), (0, 2, 0), (0, 0, 2), kd=(0.4, 0.4, 0.7))       # right
    for p00, e1, e2 in (((-1, 1, -1), (0, 0, 0.7), (2, 0, 0)), ((-1, 1, 0.3), (0, 0, 0.7), (2, 0, 0)),
                        ((-1, 1, -0.3), (0, 0, 0.6), (0.6, 0, 0)), ((0.4, 1, -0.3), (0, 0, 0.6), (0.6, 0, 0))):
        q(s, p00, e1, e2, kd=(0.5, 0.5, 0.5))                         # the ceiling around the opening
    m = s.medium
    m.sigma_a[:] = (0.05, 0.05, 0.05)
    m.sigma_s[:] = (0.5, 0.5, 0.5)
    m.g = 0.3
    if medium == "homogeneous":
        m.type = P.MEDIUM_HOMOGENEOUS
    else:
        import ctypes as C
        dens = np.array([0.2, 1, 0.7, 0.1, 0.9, 0.4, 1, 0.6], f32)
        m.type = P.MEDIUM_GRID
        m.sigma_a[:] = (0.1,) * 3
        m.sigma_s[:] = (1.4,) * 3
        m.nx = m.ny = m.nz = 2
        m.bounds_min[:] = (-0.7, -0.9, -0.6)
        m.bounds_max[:] = (0.7, 0.8, 0.8)
        m.density = dens.ctypes.data_as(C.POINTER(C.c_float))
        s._density_keepalive = dens
        if medium == "grid_boundary":
            s.camera_outside_medium = 1
            scenes.interface_box(s, (-0.7, -0.9, -0.6), (0.7, 0.8, 0.8))
    if medium == "grid_boundary":
        # The second light is a point light INSIDE the medium's box.  With boundaries the pipeline walks a shadow ray's chain of
        # segments before any tracking and drops a ray that an opaque surface blocks anywhere along it (sample_Ld_begin,
        # vspg_wavefront.h: "0 either way"), where the per-lane kernel, in the reference's order, has already tracked the medium
        # segment in front of the blocker: equal films, but the per-lane kernel counts that segment's density queries.  A distant
        # light here would send rays out of the box and into the ceiling (measured under the PLAIN image light, "bvh", 16 x 16,
        # 3 waves: 235 shadow density queries on the pipeline against 1299 per lane, everything else equal).  No shadow ray of this
        # scene is blocked behind a medium segment -- the sky's samples leave through the opening, the point light's end in the
        # box --, so every counter must agree.
        P.add_point_light(s, (0.8, 0.7, 0.6), (0.1, 0.3, 0.2))
    else:
        P.add_infinite_light(s, P.LIGHT_DISTANT, (1.5, 1.2, 1.0), (0.1, 0.95, 0.2))
    P.add_infinite_light(s, P.LIGHT_IMAGE_INFINITE, SKY_L)
    return s


def sky_index(scene, P):
    return [k for k in range(scene.n_infinite_lights) if scene.infinite_lights[k].type == P.LIGHT_IMAGE_INFINITE][0]


def room_sky():
    img = M.make_image("peaked", 16, 11)
    img[:] += f32(0.5)
    return img


def render(P, scene, prm, kernel, W, H, waves=3, portal=ROOM_PORTAL, image=None, m=None, trace=None):
    def go():
        r = P.Renderer(scene, prm, W, H)
        k = sky_index(scene, P)
        before = r.kernel_name()
        if portal is not None:
            r.set_portal_environment_image(k, room_sky() if image is None else image, portal, m)
        elif image is not None:
            r.set_environment_image(k, image, m)
        name = r.kernel_name()
        assert name == before, "the call must not change the renderer's kernel"
        for w in range(waves):
            r.render_wave(w, w + 1)
            r.post_process_wave()
        out = (name, r.film(), r.counters(), r.trace_paths(trace, [0] * len(trace)) if trace is not None else None)
        r.close()
        return out
    return with_kernel(kernel, go)


SAMPLERS = {"uniform": "LIGHTSAMPLER_UNIFORM", "power": "LIGHTSAMPLER_POWER", "bvh": "LIGHTSAMPLER_BVH"}


@pytest.mark.parametrize("sampler", sorted(SAMPLERS))
@pytest.mark.parametrize("size", [(16, 16), (64, 48)], ids=["16x16", "64x48"])
@pytest.mark.parametrize("medium", ["homogeneous", "grid", "grid_boundary"])
def test_kernel_families_agree(gpu_pkg, medium, size, sampler):
    """The default kernel of the configuration (k_render_wave_wg2<HomogeneousMedium> / the wavefront pipeline without and with medium
    boundaries) against the per-lane kernel: films, counters and replayed paths bit for bit."""
    P = gpu_pkg
    W, H = size
    scene = room_scene(P, W, H, medium)
    prm = P.app_f_params()
    prm.lightsampler = getattr(P, SAMPLERS[sampler])
    pix = [(W // 2, H // 3), (3, 2), (W - 2, H - 3), (W // 3, H // 2)]
    name_d, film_d, cnt_d, tr_d = render(P, scene, prm, None, W, H, trace=pix)
    name_l, film_l, cnt_l, tr_l = render(P, scene, prm, "lane", W, H, trace=pix)
    print(medium, size, sampler, "default:", name_d, "| lane:", name_l, "| mean", film_d[..., :3].mean(), "shadow rays", cnt_d.get("shadow_rays"))
    assert name_l.startswith("k_render_wave<")
    want_default = {"homogeneous": "k_render_wave_wg2<HomogeneousMedium", "grid": "k_wf_dist_walk<GridMedium", "grid_boundary": "k_wf_walk<GridMedium"}[medium]
    assert name_d.startswith(want_default), (name_d, want_default)
    assert np.isfinite(film_d).all() and film_d[..., :3].max() > 0
    assert cnt_d["shadow_rays"] > 0 and (medium == "homogeneous" or cnt_d["shadow_density_queries"] > 0)
    assert np.array_equal(u32(film_d), u32(film_l))
    assert cnt_d == cnt_l
    assert np.array_equal(u32(tr_d[0]), u32(tr_l[0])) and np.array_equal(tr_d[1], tr_l[1])


def test_the_portal_changes_the_picture(gpu_pkg):
    """... and the films above are not the plain image light's: with the portal, the sky reaches the room through the opening only."""
    P = gpu_pkg
    scene = room_scene(P, 16, 16, "homogeneous")
    prm = P.app_f_params()
    _, with_portal, _, _ = render(P, scene, prm, None, 16, 16)
    _, plain, _, _ = render(P, scene, prm, None, 16, 16, portal=None, image=room_sky())
    assert not np.array_equal(u32(with_portal), u32(plain))


# 3. a deterministic known answer: the sky through the portal, seen by the camera
def camera_corner_directions(W, H, eye, look, up, fov):
    """Directions through the pixel corners of a perspective camera (fov across the shorter axis), [(H + 1), (W + 1), 3] float64."""
    eye, look, up = (np.array(v, np.float64) for v in (eye, look, up))
    d = look - eye
    d /= np.linalg.norm(d)
    right = np.cross(up / np.linalg.norm(up), d)
    right /= np.linalg.norm(right)
    nup = np.cross(d, right)
    aspect = W / H
    sx, sy = (aspect, 1.0) if aspect > 1 else (1.0, 1 / aspect)
    t = math.tan(math.radians(fov) / 2)
    xs = (2 * np.arange(W + 1) / W - 1) * sx * t
    ys = (1 - 2 * np.arange(H + 1) / H) * sy * t
    return d[None, None, :] + xs[None, :, None] * right[None, None, :] + ys[:, None, None] * nup[None, None, :]


def test_constant_sky_through_the_portal_is_exact(gpu_pkg):
    """A camera in an empty medium, a constant image c, depth 0: a pixel whose whole footprint lies inside the portal's projection
    holds c * L exactly, one wholly outside holds 0.  Pixels are classified with the mirror on the corners of the pixel and of its eight
    neighbours (so the camera's own roundings cannot move a footprint across the edge); only footprints near the edge are left out.
    "Exactly" holds where the rectified image holds c exactly: a 1 x 1 map under the identity (its one texel is resampled with the
    weights 1, 0, 0, 0).  Image::BilerpChannel's four float weights do not sum to 1 in general, so a larger map under a rotation
    holds c within an ulp or two per texel; there the pixel must lie between the mirror's smallest and largest rectified texel."""
    P = gpu_pkg
    W, H = 48, 32
    eye, look, fov = (0, 0.0, -3), (0, 0, 0), 40.0
    s = scenes.empty_scene(W, H, eye=eye, look=look, fov=fov)
    m = s.medium
    m.type = P.MEDIUM_HOMOGENEOUS
    m.sigma_a[:] = (0, 0, 0)
    m.sigma_s[:] = (0, 0, 0)
    P.add_infinite_light(s, P.LIGHT_IMAGE_INFINITE, SKY_L)
    portal = np.array([[-0.8, -0.5, 2], [-0.8, 0.5, 2], [0.8, 0.5, 2], [0.8, -0.5, 2]], f32)   # frame z = +z, away from the camera
    c = np.array([0.75, 0.5, 2.0], f32)
    light = M.PortalLight(np.broadcast_to(c, (4, 4, 3)).copy(), portal, SKY_L, M.rotated())
    lo, hi = light.image.reshape(-1, 3).min(axis=0) * f32(SKY_L), light.image.reshape(-1, 3).max(axis=0) * f32(SKY_L)
    assert np.all(np.abs(light.image - c) <= 4 * 2.0 ** -24 * c)
    assert np.array_equal(M.PortalLight(np.broadcast_to(c, (1, 1, 3)).copy(), portal, SKY_L).image.reshape(3), c)
    dirs = camera_corner_directions(W, H, eye, look, (0, 1, 0), fov)
    inside = light.Le(np.tile(f32(eye), ((H + 1) * (W + 1), 1)), dirs.reshape(-1, 3).astype(f32))[0].reshape(H + 1, W + 1)
    pad = np.pad(inside, 1, mode="edge")
    all_in, all_out = np.ones((H, W), bool), np.ones((H, W), bool)
    for dy in range(4):
        for dx in range(4):
            blk = pad[dy:dy + H, dx:dx + W]
            all_in &= blk
            all_out &= ~blk
    kept = all_in | all_out
    print("pixels inside %d, outside %d, left out %d of %d" % (all_in.sum(), all_out.sum(), (~kept).sum(), W * H))
    assert kept.mean() >= 0.75 and all_in.sum() > 20 and all_out.sum() > 20
    prm = P.app_f_params()
    prm.maxdepth = 0
    for kernel in (None, "lane"):
        for res, m in ((1, None), (4, M.rotated())):
            def go():
                r = P.Renderer(s, prm, W, H)
                r.set_portal_environment_image(0, np.broadcast_to(c, (res, res, 3)).copy(), portal, m)
                r.render_wave(0, 2)
                f = r.film()
                r.close()
                return f
            film = with_kernel(kernel, go)
            assert np.all(film[..., 3] == 2)
            rgb = film[..., :3] / film[..., 3:4]
            if res == 1:
                want = c * np.array(SKY_L, f32)
                assert np.array_equal(u32(rgb[all_in]), u32(np.broadcast_to(want, rgb[all_in].shape))), kernel
            else:
                assert np.all((rgb[all_in] >= lo) & (rgb[all_in] <= hi)), kernel
            assert np.all(rgb[all_out] == 0), (kernel, res)


# 4. statistical known answers on a diffuse floor
KD = 0.5
FLOOR_PORTAL = np.array([[-0.3, 1, -0.5], [0.9, 1, -0.5], [0.9, 1, 0.4], [-0.3, 1, 0.4]], f32)   # frame z = +y


def floor_scene(P, W=8, H=8):
    """A camera looking straight down at the floor point (0.2, 0, -0.1) through a very narrow lens; no medium; the sky alone."""
    s = scenes.empty_scene(W, H, eye=(0.2, 0.6, -0.1), look=(0.2, 0, -0.1), up=(0, 0, 1), fov=0.5)
    s.medium.type = P.MEDIUM_NONE
    s.camera_outside_medium = 1
    scenes.add_quad(s, (-6, 0, -6), (0, 0, 12), (12, 0, 0), kd=(KD, KD, KD))
    P.add_infinite_light(s, P.LIGHT_IMAGE_INFINITE, (1, 1, 1))
    return s


def wave_means(r, n, W=8, H=8):
    ms = []
    for w in range(n):
        r.film_clear()
        r.render_wave(w, w + 1)
        f = r.film()
        ms.append((f[..., :3] / f[..., 3:4]).astype(np.float64).mean(axis=(0, 1)))
    return np.array(ms)


def test_floor_point_under_a_constant_sky_sees_the_form_factor(gpu_pkg):
    """maxdepth 1: the pixel's mean is Kd * c * F with F the closed-form form factor of the portal's rectangle seen from the floor
    point (float64).  Judged by the sample's own standard error: |z| <= 4.5, the threshold of the Welch tests (false alarm ~7e-6).
    The footprint is 5 mm wide (fov 0.5 degrees from 0.6): F changes by < 1e-3 relative across it, far below the standard error."""
    P = gpu_pkg
    c = 1.5
    F = M.rect_form_factor_window(-0.3 - 0.2, 0.9 - 0.2, -0.5 + 0.1, 0.4 + 0.1, 1.0)
    prm = P.app_f_params()
    prm.maxdepth = 1
    r = P.Renderer(floor_scene(P), prm, 8, 8)
    r.set_portal_environment_image(0, np.full((8, 8, 3), c, f32), FLOOR_PORTAL, None)
    ms = wave_means(r, 48).mean(axis=1)
    r.close()
    se = ms.std(ddof=1) / math.sqrt(len(ms))
    z = (ms.mean() - KD * c * F) / se
    print("F = %.6f, expected %.6f, measured %.6f +- %.6f, z = %.2f" % (F, KD * c * F, ms.mean(), se, z))
    assert se < 0.05 * KD * c * F and abs(z) <= 4.5


def test_a_hemisphere_wide_portal_is_the_plain_image_light(gpu_pkg):
    """A portal that covers the floor point's hemisphere but for a 1e-6 sliver of form factor, against the plain image light."""
    P = gpu_pkg
    img = M.make_image("banded", 16, 4) + f32(0.2)
    big = np.array([[-1e3, 1, -1e3], [1e3, 1, -1e3], [1e3, 1, 1e3], [-1e3, 1, 1e3]], f32) + f32([0.2, 0, -0.1])
    prm = P.app_f_params()
    prm.maxdepth = 1
    means = []
    for portal in (big, None):
        r = P.Renderer(floor_scene(P), prm, 8, 8)
        if portal is None:
            r.set_environment_image(0, img, M.rotated())
        else:
            r.set_portal_environment_image(0, img, portal, M.rotated())
        means.append(wave_means(r, 32).mean(axis=1))
        r.close()
    a, b = means
    z = (a.mean() - b.mean()) / math.sqrt(a.var(ddof=1) / len(a) + b.var(ddof=1) / len(b))
    print("portal %.5f +- %.5f, plain %.5f +- %.5f, z = %.3f" % (a.mean(), a.std(ddof=1) / math.sqrt(32), b.mean(), b.std(ddof=1) / math.sqrt(32), z))
    assert a.mean() > 0 and abs(z) <= 4.5


def test_nee_agrees_with_escaped_rays_only(gpu_pkg):
    """Whole-film means of 32 separately cleared waves with NEE and 32 with usenee false, by Welch's statistic, in the fogged room lit
    by the sky through the opening alone."""
    P = gpu_pkg
    W, H = 48, 32
    scene = room_scene(P, W, H, "grid")
    scene.n_infinite_lights = 0
    P.add_infinite_light(scene, P.LIGHT_IMAGE_INFINITE, SKY_L)
    means = {}
    for nee in (1, 0):
        prm = P.app_f_params()
        prm.usenee = nee
        r = P.Renderer(scene, prm, W, H)
        r.set_portal_environment_image(0, room_sky(), ROOM_PORTAL, M.rotated())
        means[nee] = wave_means(r, 32, W, H).mean(axis=1)
        r.close()
    a, b = means[1], means[0]
    z = (a.mean() - b.mean()) / math.sqrt(a.var(ddof=1) / len(a) + b.var(ddof=1) / len(b))
    print("NEE %.5f +- %.5f, escaped only %.5f +- %.5f, z = %.3f" % (a.mean(), a.std(ddof=1) / math.sqrt(32), b.mean(), b.std(ddof=1) / math.sqrt(32), z))
    assert a.mean() > 0 and abs(z) <= 4.5, z


# 5. on a live renderer
def test_set_portal_on_a_live_renderer(gpu_pkg, lights):
    P = gpu_pkg
    W, H = 16, 16
    scene = room_scene(P, W, H, "grid")
    k = sky_index(scene, P)
    prm = P.app_f_params()
    prm.lightsampler = P.LIGHTSAMPLER_POWER
    prm.vspguiding = 0
    sky = room_sky()

    def fresh(portal):
        r = P.Renderer(scene, prm, W, H)
        if portal:
            r.set_portal_environment_image(k, sky, ROOM_PORTAL, M.rotated())
        else:
            r.set_environment_image(k, sky, M.rotated())
        return r

    def two_waves(r):
        r.film_clear()
        r.render_wave(0, 2)
        return r.film()
    r = fresh(False)
    name = r.kernel_name()
    r.render_wave(0, 1)
    r.post_process_wave()
    film1, cnt1, vsp1 = r.film(), r.counters(), r.vsp_buffer()
    r.set_portal_environment_image(k, sky, ROOM_PORTAL, M.rotated())       # mid-render: film weight, VSP buffer and counters stay
    assert np.array_equal(u32(r.film()), u32(film1)) and r.counters() == cnt1 and r.kernel_name() == name
    vsp2 = r.vsp_buffer()
    assert np.array_equal(u32(vsp1[0]), u32(vsp2[0])) and vsp1[1] == vsp2[1]
    twin_portal, twin_plain = fresh(True), fresh(False)
    film_portal, film_plain = two_waves(twin_portal), two_waves(twin_plain)
    assert not np.array_equal(u32(film_portal), u32(film_plain))
    assert np.array_equal(u32(two_waves(r)), u32(film_portal))              # plain -> portal == created with the portal
    with pytest.raises(P.VspgError):                                           # the plain probe does not serve a portal slot
        r.envlight_batch(k, np.zeros((1, 3), f32) + 1, np.zeros((1, 2), f32))
    # every refusal leaves a following wave bit-identical to the untouched twin
    fp = P.C.POINTER(P.C.c_float)
    ptr = lambda a: a.ctypes.data_as(fp) if a is not None else None
    raw = lambda idx, img, res, m, q: r.lib.vspg_renderer_set_portal_environment_image(r.h, idx, ptr(img), res, ptr(m), ptr(q), None)
    bad_img = sky.copy()
    bad_img[3, 4, 1] = np.nan
    sing = M.rotated().copy()
    sing[:, 1] = 0
    skew, para, deg, nanq = (ROOM_PORTAL.copy() for _ in range(4))
    skew[2] += f32([0.3, 0, 0])
    para[2:] += f32([0.3, 0, 0])
    deg[1] = deg[0]
    nanq[3, 2] = np.inf
    other = [i for i in range(scene.n_infinite_lights) if i != k][0]
    good = np.ascontiguousarray(ROOM_PORTAL)
    for args, words in (((other, sky, 16, None, good), b"not of type"), ((9, sky, 16, None, good), b"names no infinite light"),
                        ((k, sky, 0, None, good), b"resolution"), ((k, sky, 4097, None, good), b"resolution"), ((k, None, 16, None, good), b"null"),
                        ((k, bad_img, 16, None, good), b"not-a-number"), ((k, sky, 16, sing, good), b"singular"), ((k, sky, 16, None, None), b"null"),
                        ((k, sky, 16, None, nanq), b"not finite"), ((k, sky, 16, None, deg), b"degenerate"),
                        ((k, sky, 16, None, skew), b"planar quadrilateral"), ((k, sky, 16, None, para), b"perpendicular")):
        assert raw(*args) == P.VSPG_EINVAL and words in r.lib.vspg_last_error(), (words, r.lib.vspg_last_error())
    assert np.array_equal(u32(two_waves(r)), u32(film_portal))
    # portal -> plain image -> portal, and plain again == never-portal
    r.set_environment_image(k, sky, M.rotated())
    assert np.array_equal(u32(two_waves(r)), u32(film_plain))
    with pytest.raises(P.VspgError):
        r.portallight_batch(k, np.zeros((1, 3), f32), np.zeros((1, 3), f32), np.zeros((1, 2), f32))   # no portal light any more
    r.set_portal_environment_image(k, sky, ROOM_PORTAL, M.rotated())
    assert np.array_equal(u32(two_waves(r)), u32(film_portal))
    r.set_environment_image(k, sky, M.rotated())
    assert np.array_equal(u32(two_waves(r)), u32(film_plain))
    for x in (r, twin_portal, twin_plain):
        x.close()


def test_guided_rendering_with_training(gpu_pkg):
    """Reference-default parameters (guiding with in-loop training) for a few waves: finite films, the guiding fields survive the call,
    and the default kernel equals the per-lane kernel where the two differ."""
    P = gpu_pkg
    W, H = 16, 16
    scene = room_scene(P, W, H, "homogeneous")
    k = sky_index(scene, P)
    films, names = [], []
    for kernel in (None, "lane"):
        def go():
            r = P.Renderer(scene, P.default_params(), W, H)
            r.set_portal_environment_image(k, room_sky(), ROOM_PORTAL, None)
            for w in range(4):
                r.render_wave(w, w + 1)
                r.post_process_wave()
            st = r.training_stats()
            r.set_portal_environment_image(k, room_sky(), ROOM_PORTAL, M.rotated())
            assert r.training_stats() == st, "training state must survive the call"
            r.render_wave(4, 5)
            out = r.kernel_name(), r.film()
            r.close()
            return out
        n, f = with_kernel(kernel, go)
        names.append(n)
        films.append(f)
        assert np.isfinite(f).all() and f[..., :3].max() > 0
    print("guided:", names)
    assert names[1].startswith("k_render_wave<")
    # (a guided full scene with infinite lights is served by the per-lane kernel alone unless the choice record says otherwise:
    #  where the default is another kernel the two must agree, where it is the same one there is nothing to compare)
    assert names[0] == names[1] or names[0].startswith("k_render_wave_wg2<")
    if names[0] != names[1]:
        assert np.array_equal(u32(films[0]), u32(films[1]))
