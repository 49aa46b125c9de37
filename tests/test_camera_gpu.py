"""Thin-lens, orthographic and spherical cameras on the device: vspg_camera_ray_batch against the float32 mirror of
tests/camera_model.py bit for bit (given variates, and the renderer's own sampler against the oracle's), the pinhole identity, kernel
families against each other under every model, a deterministic known answer (a spherical camera photographs an environment map back),
a statistical known answer (depth of field across the edge of an emissive half-plane, tests/camera_dof.py), vspg_renderer_set_camera on a
live renderer with its refusals, pixel windows, in-loop training under a lens, and the scene-file route.  Films are 32 x 24 or smaller."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import camera_dof as D
import camera_model as M
import envlight_model as EM
import scenes
from conftest import ROOT

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 32, 24
BW, BH = 33, 17            # the batch's frame: no power of two, so that the uv division shows
EYE, LOOK, UP = (0.3, 0.2, -0.95), (0.0, 0.1, 0.0), (0.1, 1.0, 0.05)
HOST = os.path.join(ROOT, "vspg-pbrt-v4_amd", "host")
LENS = dict(model=M.PERSPECTIVE, lens_radius=0.05, focal_distance=1.95)      # the fog box's back wall in focus


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def with_env(env, fn):
    for k, v in env.items():
        os.environ[k] = v
    try:
        return fn()
    finally:
        for k in env:
            os.environ.pop(k, None)


def box_camera(P, model, w=W, h=H):
    """The fog box's own view (vspg_scene_fog_box) under camera model `model`; orthographic: the window [-0.8, 0.8] x [-0.6, 0.6]."""
    sw = (-0.8, 0.8, -0.6, 0.6) if model == M.ORTHOGRAPHIC else None
    return P.camera_look_at_window(model, (0, 0, -0.95), (0, 0, 0), (0, 1, 0), 60.0, w, h, screen_window=sw)


CAMERAS = {"lens": LENS, "ortho": dict(model=M.ORTHOGRAPHIC, lens_radius=0.0, focal_distance=1e6),
           "ortho_lens": dict(model=M.ORTHOGRAPHIC, lens_radius=0.08, focal_distance=1.5),
           "equalarea": dict(model=M.SPHERICAL_EQUALAREA), "equirect": dict(model=M.SPHERICAL_EQUIRECT)}


def set_cam(P, r, name, w=W, h=H):
    kw = CAMERAS[name]
    r.set_camera(box_camera(P, kw["model"], w, h), **kw)


def grid_medium(P, s, n=8, seed=2):
    dens = np.random.default_rng(seed).uniform(0.05, 1.0, n * n * n).astype(f32)
    m = s.medium
    m.type = P.MEDIUM_GRID
    m.sigma_a[:] = (0.05,) * 3
    m.sigma_s[:] = (0.9,) * 3
    m.g = 0.3
    m.nx = m.ny = m.nz = n
    m.bounds_min[:] = (-1, -1, -1)
    m.bounds_max[:] = (1, 1, 1)
    m.density = dens.ctypes.data_as(C.POINTER(C.c_float))
    s._density_keepalive = dens
    return s


def rgb_grid_medium(P, s, n=8, seed=4):
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.01, 0.2, (n, n, n, 3)).astype(f32)
    sc = rng.uniform(0.1, 1.0, (n, n, n, 3)).astype(f32)
    P.set_rgb_grid_medium(s, a, sc, None, p0=(-1, -1, -1), p1=(1, 1, 1), g=0.2)
    return s


def scene_of(P, kind, w=W, h=H):
    s = P.fog_box_scene(w, h)
    if kind == "grid":
        grid_medium(P, s)
    elif kind == "rgbgrid":
        rgb_grid_medium(P, s)
    elif kind == "boundary":     # the fog confined to a box of interface surfaces inside the room; the camera stands outside it
        s.camera_outside_medium = 1
        scenes.interface_box(s, (-0.5, -0.5, -0.4), (0.5, 0.5, 0.6))
    return s


def render(P, kind, camera, env=None, waves=4, nds=False, seed=0, trace=None, post=True):
    """-> (kernel name, film, counters, traced L or None) of `waves` one-sample waves under camera `camera` (a CAMERAS key, or None)."""
    def go():
        prm = P.app_f_params()
        if nds:
            prm.vspsamplingmethod = P.VSP_NDS
        r = P.Renderer(scene_of(P, kind), prm, W, H, seed=seed)
        if camera:
            set_cam(P, r, camera)
        name = r.kernel_name()
        for k in range(waves):
            r.render_wave(k, k + 1)
            if post:
                r.post_process_wave()
        out = (name, r.film(), r.counters(), r.trace_paths(*trace)[0] if trace else None)
        r.close()
        return out
    return with_env(env or {}, go)


# ---- 1. the batch against the mirror, bit for bit ---------------------------------------------------------------------------------------
def batch_inputs(n=1000):
    rng = np.random.default_rng(17)
    pix = np.stack([rng.integers(0, BW, n), rng.integers(0, BH, n)], axis=1).astype(np.int32)
    pix[:5] = [[0, 0], [BW - 1, 0], [0, BH - 1], [BW - 1, BH - 1], [BW // 2, BH // 2]]
    u = rng.random((n, 4)).astype(f32)
    below1 = np.nextafter(f32(1), f32(0))
    u[:12] = [[0, 0, 0, 0], [below1] * 4, [0, below1, below1, 0], [0.5, 0.5, 0.5, 0.5], [0.25, 0.75, 0.9, 0.6], [0.25, 0.75, 0.6, 0.9], [0.1, 0.2, 0.7, 0.7],
              [0.1, 0.2, 0.2, 0.2], [0.9, 0.9, 0.5, 0.1], [0.9, 0.9, 0.1, 0.5], [0.5, 0.5, 0.3, 0.7], [0.0, 0.0, 0.5, 0.5]]
    # (lens pairs: |x| > |y| and the other branch, x = y on both diagonals, a zero coordinate on each axis, the centre)
    return pix, u


BATCH_CAMERAS = [(M.PERSPECTIVE, 0.0, 1e6), (M.PERSPECTIVE, 0.05, 1.95), (M.PERSPECTIVE, 0.3, 0.7), (M.ORTHOGRAPHIC, 0.0, 1e6), (M.ORTHOGRAPHIC, 0.4, 0.6),
                 (M.SPHERICAL_EQUALAREA, 0.0, 1e6), (M.SPHERICAL_EQUIRECT, 0.0, 1e6)]


@pytest.fixture(scope="module")
def batch_renderer(gpu_pkg):
    r = gpu_pkg.Renderer(gpu_pkg.fog_box_scene(BW, BH), gpu_pkg.app_f_params(), BW, BH, seed=5)
    yield r
    r.close()


def batch_camera(P, model):
    sw = (-0.7, 0.9, -0.3, 0.5) if model == M.ORTHOGRAPHIC else None
    return P.camera_look_at_window(model, EYE, LOOK, UP, 50.0, BW, BH, screen_window=sw)


@pytest.mark.parametrize("model,R,F", BATCH_CAMERAS)
def test_ray_batch_equals_the_mirror(gpu_pkg, batch_renderer, model, R, F):
    """1000 elements (no multiple of 64) on given variates, all four models, with and without a lens: origin and direction equal the
    mirror's bits.  Then 500 (pixel, sample) pairs drawn by the renderer's own sampler against the mirror fed by the oracle's sampler:
    that pins the sampler dimensions."""
    import oracle_lib
    P, r = gpu_pkg, batch_renderer
    cam = batch_camera(P, model)
    r.set_camera(cam, model, R, F)
    mirror = M.Camera.from_c(cam, model, BW, BH, R, F)
    pix, u = batch_inputs()
    go, gd = r.camera_ray_batch(pix, np.zeros(len(pix), np.int32), u)
    wo, wd = M.rays_of_samples(mirror, pix, u)
    for name, got, want in (("origin", go, wo), ("direction", gd, wd)):
        bad = np.flatnonzero((u32(got) != u32(want)).any(axis=1))
        assert bad.size == 0, (name, len(bad), "first element", int(bad[0]), pix[bad[0]], u[bad[0]], got[bad[0]], want[bad[0]])
    assert np.unique(np.concatenate([u32(wo), u32(wd)], axis=1), axis=0).shape[0] > 900
    rng = np.random.default_rng(23)
    pix2 = np.stack([rng.integers(0, BW, 500), rng.integers(0, BH, 500)], axis=1).astype(np.int32)
    si = rng.integers(0, 4096, 500).astype(np.int32)
    go, gd = r.camera_ray_batch(pix2, si)
    us = M.sampler_variates(oracle_lib.load(), pix2, si, seed=5)
    wo, wd = M.rays_of_samples(mirror, pix2, us)
    assert np.array_equal(u32(go), u32(wo)) and np.array_equal(u32(gd), u32(wd))
    if mirror.has_lens:      # the lens variates matter: the wrong dimensions give other rays
        wrong = M.rays_of_samples(mirror, pix2, M.sampler_variates(oracle_lib.load(), pix2, si, seed=5, plant=("wrong_dims",)))[1]
        assert not np.array_equal(u32(gd), u32(wrong))


def test_ray_batch_refusals(gpu_pkg, batch_renderer):
    P, r = gpu_pkg, batch_renderer
    for pix, si in (([[BW, 0]], [0]), ([[0, -1]], [0]), ([[0, 0]], [-1])):
        with pytest.raises(P.VspgError) as e:
            r.camera_ray_batch(pix, si)
        assert e.value.code == P.VSPG_EINVAL


# ---- 2. the pinhole identity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fog", "grid"])
def test_pinhole_identity(gpu_pkg, kind):
    """set_camera(cam, NULL) and set_camera with perspective and lens_radius 0: the kernel name and the film of an untouched renderer."""
    P = gpu_pkg
    base = render(P, kind, None)
    assert base[0] == ("k_render_wave_wg3<HomogeneousMediumT<2,true>>" if kind == "fog" else "k_wf_dist_walk<GridMediumGrey>")
    for model_kw in (dict(model=None), dict(model=M.PERSPECTIVE, lens_radius=0.0, focal_distance=3.0)):
        def go():
            r = P.Renderer(scene_of(P, kind), P.app_f_params(), W, H)
            r.set_camera(box_camera(P, M.PERSPECTIVE), **model_kw)
            name = r.kernel_name()
            for k in range(4):
                r.render_wave(k, k + 1)
                r.post_process_wave()
            out = (name, r.film(), r.counters())
            r.close()
            return out
        name, film, cnt = go()
        assert name == base[0] and cnt == base[2]
        assert np.array_equal(u32(film), u32(base[1]))


# ---- 3. kernel families against each other ------------------------------------------------------------------------------------------------
TRACE = (np.array([(x, y) for y in range(2, H, 5) for x in range(1, W, 4)], np.int32)[:40],)


@pytest.mark.parametrize("kind,camera,nds", [("fog", "lens", False), ("fog", "ortho", False), ("fog", "ortho_lens", False), ("fog", "equalarea", False),
                                             ("fog", "equirect", False), ("grid", "lens", False), ("grid", "ortho", False), ("grid", "equalarea", False),
                                             ("grid", "equirect", False), ("rgbgrid", "lens", False), ("boundary", "lens", False), ("grid", "lens", True)])
def test_kernel_families_agree(gpu_pkg, kind, camera, nds):
    """Film and counters at 32 x 24, 4 spp: the default kernel of the configuration == the per-lane kernel, bit for bit, and differs
    from the pinhole's film."""
    P = gpu_pkg
    a = render(P, kind, camera, nds=nds)
    b = render(P, kind, camera, env={"VSPG_KERNEL": "lane"}, nds=nds)
    want = {"fog": "k_render_wave_wg2<HomogeneousMedium>", "boundary": "k_render_wave_wg2<HomogeneousMedium>",
            "grid": "k_wf_segment_vertex<GridMediumGrey>" if nds else "k_wf_dist_walk<GridMediumGrey>", "rgbgrid": "k_wf_dist_walk<RgbGridMedium>"}[kind]
    assert a[0] == want, a[0]
    assert b[0].startswith("k_render_wave<"), b[0]
    assert a[2] == b[2], (a[2], b[2])
    assert np.array_equal(u32(a[1]), u32(b[1]))
    assert np.isfinite(a[1]).all() and np.all(a[1][..., 3] == 4) and a[1][..., :3].max() > 0
    if not nds:
        assert not np.array_equal(u32(a[1]), u32(render(P, kind, None)[1]))


@pytest.mark.parametrize("kind,camera", [("fog", "lens"), ("grid", "equirect")])
def test_replayed_paths_sum_to_the_film(gpu_pkg, kind, camera):
    """vspg_trace_paths of 200 (pixel, sample) pairs -- 50 pixels, samples 0..3 -- sums to those pixels of a 4-sample film.  (No
    post-processing between the waves: the replay reads the VSP buffer as it stands.)"""
    P = gpu_pkg
    pix = np.array([(x, y) for y in range(1, H, 5) for x in range(0, W, 3)], np.int32)[:50]
    pairs = (np.repeat(pix, 4, axis=0), np.tile(np.arange(4, dtype=np.int32), 50))
    name, film, _, L = render(P, kind, camera, trace=pairs, post=False)
    got = film[pix[:, 1], pix[:, 0], :3]
    acc = np.zeros((50, 3), f32)
    for s in range(4):
        acc = (acc + L.reshape(50, 4, 3)[:, s]).astype(f32)
    assert np.array_equal(u32(got), u32(acc)), name


# ---- 4. a deterministic known answer: the panorama photographs the map back ---------------------------------------------------------------
@pytest.mark.parametrize("model", [M.SPHERICAL_EQUALAREA, M.SPHERICAL_EQUIRECT])
def test_spherical_camera_photographs_the_environment_map(gpu_pkg, model):
    """No medium, one image infinite light with an 8 x 8 image, a spherical camera at 16 x 16: for every (pixel, sample) pair the
    replayed path's L equals envlight_model's Le of the mirror's direction bit for bit."""
    import oracle_lib
    P = gpu_pkg
    w = h = 16
    s = scenes.empty_scene(w, h, eye=(0.1, 0.2, -0.3), look=(0.4, 0.1, 1.0))
    s.medium.type = P.MEDIUM_NONE
    s.camera_outside_medium = 1
    L = (1.5, 1.0, 0.5)
    P.add_infinite_light(s, P.LIGHT_IMAGE_INFINITE, L)
    img = np.ascontiguousarray(np.random.default_rng(8).uniform(0.1, 2.0, (8, 8, 3)).astype(f32))
    r = P.Renderer(s, P.app_f_params(), w, h, seed=2)
    r.set_environment_image(0, img, None)
    cam = P.camera_look_at_window(model, (0.1, 0.2, -0.3), (0.4, 0.1, 1.0), (0, 1, 0), 0.0, w, h)
    r.set_camera(cam, model)
    pix = np.array([(x, y) for y in range(h) for x in range(w)], np.int32)
    si = (np.arange(len(pix)) % 3).astype(np.int32)
    got, _ = r.trace_paths(pix, si)
    r.render_wave(0, 1)
    film = r.film()
    r.close()
    mirror = M.Camera.from_c(cam, model, w, h)
    light = EM.EnvLight(img, L=L)
    rd = M.rays_of_samples(mirror, pix, M.sampler_variates(oracle_lib.load(), pix, si, seed=2))[1]
    want = light.Le(rd)[0]
    assert np.array_equal(u32(got), u32(want))
    rd0 = M.rays_of_samples(mirror, pix, M.sampler_variates(oracle_lib.load(), pix, np.zeros(len(pix), np.int32), seed=2))[1]
    assert np.array_equal(u32(film[..., :3].reshape(-1, 3)), u32(light.Le(rd0)[0])) and np.all(film[..., 3] == 1)
    assert np.unique(u32(want), axis=0).shape[0] >= 48      # the panorama sees most of the map's 64 texels


# ---- 5. a statistical known answer: depth of field -------------------------------------------------------------------------------------------
def dof_film(P, g, spp):
    s = P.VspgScene()
    s.medium.type = P.MEDIUM_NONE
    P.add_quad(s, (0.0, -4.0, g.Z), (4.0, 0.0, 0.0), (0.0, 8.0, 0.0), kd=(0, 0, 0), le=(1, 1, 1), two_sided=1)
    cam = P.camera_look_at_window(g.model, (0, 0, 0), (0, 0, 1), (0, 1, 0), 90.0, D.XRES, D.YRES, screen_window=D.WINDOW)
    s.camera = cam
    r = P.Renderer(s, P.app_f_params(), D.XRES, D.YRES, seed=11)
    r.set_camera(cam, g.model, g.R, g.F)
    name = r.kernel_name()
    r.render_wave(0, spp)
    f = r.film()
    r.close()
    assert np.all(f[..., 3] == spp)
    return name, (f[D.ROW, :, :3].astype(np.float64) / spp)


@pytest.mark.parametrize("model", [M.PERSPECTIVE, M.ORTHOGRAPHIC])
def test_depth_of_field_across_an_edge(gpu_pkg, model):
    """Every sample is Le = 1 times a Bernoulli variable whose probability P per pixel is the area fraction of the lens disk on the
    bright side of the edge, averaged over the pixel (tests/camera_dof.py: the closed form, integrated in float64).  32 pixels of one
    row at n = 4096 spp: |film - P| <= 5 sqrt(P (1 - P) / n) per pixel and channel -- the binomial's standard deviation, not a measured
    tolerance; with a fixed seed the run is deterministic.  Focused on the plane (Z = F) the step is sharp: every pixel but the one
    the edge crosses is exactly 0 or 1."""
    P = gpu_pkg
    n = 4096
    g = D.geometry(model)
    prob = D.hit_probability(g)
    assert prob.min() >= 0.1 and prob.max() <= 0.9
    name, row = dof_film(P, g, n)
    assert name == "k_render_wave<HomogeneousMedium>", name
    sigma = np.sqrt(prob * (1 - prob) / n)
    z = np.abs(row - prob[:, None]) / sigma[:, None]
    print("model %d: max |film - P| / sigma = %.2f; P from %.3f to %.3f" % (model, z.max(), prob.min(), prob.max()))
    assert np.all(z <= 5), (z.max(), row[:, 0], prob)
    g = D.geometry(model, focused=True)
    _, row = dof_film(P, g, 256)
    edge = 16
    assert np.all(row[:edge] == 0) and np.all(row[edge + 1:] == 1) and 0 < row[edge, 0] < 1, row[:, 0]


# ---- 6. set_camera on a live renderer ----------------------------------------------------------------------------------------------------------
def test_set_camera_on_a_live_renderer(gpu_pkg):
    """A one-sample wave under the pinhole parks samples and suspends paths (k_render_wave_wg3); a lens camera is set; more waves
    follow.  Film and counters equal those of a renderer whose first wave was flushed and read back before the camera was set."""
    P = gpu_pkg

    def go(flush_first):
        r = P.Renderer(P.fog_box_scene(W, H), P.app_f_params(), W, H, seed=3)
        assert r.kernel_name() == "k_render_wave_wg3<HomogeneousMediumT<2,true>>"
        r.render_wave(0, 1)
        if flush_first:
            r.flush()
            r.film()
            r.counters()
        set_cam(P, r, "lens")
        assert r.kernel_name() == "k_render_wave_wg2<HomogeneousMedium>"
        r.render_wave(1, 2)
        r.render_wave(2, 3)
        set_cam(P, r, "equirect")
        r.render_wave(3, 4)
        r.set_camera(box_camera(P, M.PERSPECTIVE), None)
        assert r.kernel_name() == "k_render_wave_wg3<HomogeneousMediumT<2,true>>"
        r.render_wave(4, 5)
        out = (r.film(), r.counters())
        r.close()
        return out
    a, b = go(False), go(True)
    assert a[1] == b[1] and np.array_equal(u32(a[0]), u32(b[0]))
    assert np.all(a[0][..., 3] == 5)      # nothing was cleared, nothing lost


def test_set_camera_refusals_leave_the_renderer_alone(gpu_pkg):
    P = gpu_pkg
    lib = P.load()
    nan, inf = float("nan"), float("inf")

    def film_after(refusals):
        r = P.Renderer(P.fog_box_scene(W, H), P.app_f_params(), W, H, seed=4)
        set_cam(P, r, "lens")
        r.render_wave(0, 1)
        name = r.kernel_name()
        if refusals:
            good = box_camera(P, M.PERSPECTIVE)
            cases = [(good, P.VspgCameraModel(7, 0, 0)), (good, P.VspgCameraModel(-1, 0, 0)), (good, P.VspgCameraModel(0, -0.1, 1)), (good, P.VspgCameraModel(1, nan, 1)),
                     (good, P.VspgCameraModel(0, inf, 1)), (good, P.VspgCameraModel(0, 0.1, 0)), (good, P.VspgCameraModel(1, 0.1, -2)), (good, P.VspgCameraModel(0, 0.1, nan)),
                     (good, P.VspgCameraModel(1, 0.1, inf))]
            for field, k in (("origin", 1), ("right", 0), ("up", 2), ("fwd", 1)):
                for v in (nan, inf):
                    c = box_camera(P, M.ORTHOGRAPHIC)
                    getattr(c, field)[k] = v
                    cases.append((c, P.VspgCameraModel(1, 0, 0)))
            for field in ("sx", "ox", "sy", "oy"):
                c = box_camera(P, M.PERSPECTIVE)
                setattr(c, field, nan)
                cases.append((c, None))
            for c, m in cases:
                rc = lib.vspg_renderer_set_camera(r.h, C.byref(c), None if m is None else C.byref(m), None)
                assert rc == P.VSPG_EINVAL, (rc, lib.vspg_last_error())
            assert lib.vspg_renderer_set_camera(r.h, None, None, None) == P.VSPG_EINVAL
            assert lib.vspg_renderer_set_camera(None, C.byref(good), None, None) == P.VSPG_EINVAL
            assert r.kernel_name() == name
        r.render_wave(1, 2)
        out = (r.kernel_name(), r.film(), r.counters())
        r.close()
        return out
    a, b = film_after(False), film_after(True)
    assert a[0] == b[0] == "k_render_wave_wg2<HomogeneousMedium>" and a[2] == b[2] and np.array_equal(u32(a[1]), u32(b[1]))


# ---- 7. windows ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fog", "grid"])
def test_windows_tile_the_frame_under_a_lens(gpu_pkg, kind):
    P = gpu_pkg

    def go(windows):
        r = P.Renderer(scene_of(P, kind), P.app_f_params(), W, H, seed=6)
        set_cam(P, r, "lens")
        for k in range(2):
            for x0, y0, x1, y1 in windows:
                r.render_window(x0, y0, x1, y1, k, k + 1)
        f = r.film()
        r.close()
        return f
    full = go([(0, 0, W, H)])
    tiles = go([(0, 0, 13, 9), (13, 0, W, 9), (0, 9, 21, H), (21, 9, W, H)])
    assert np.array_equal(u32(full), u32(tiles)) and np.all(full[..., 3] == 2)


# ---- 8. guided: in-loop training under a lens ------------------------------------------------------------------------------------------------------
def test_training_under_a_lens(gpu_pkg):
    """Two updates of in-loop training on the fog box through a lens, then two guided waves.  The guided workgroup kernel is a
    rectangle-scene instantiation, so under a lens the per-lane kernel serves the default and VSPG_KERNEL=lane alike: no second kernel
    exists to compare with, and the names say so.  (Two training runs are not compared bit for bit: the update's sample order comes
    from atomics.)  The film is finite and complete, and both fields hold regions."""
    P = gpu_pkg

    def go():
        prm = P.default_params()
        prm.guide_num_training_waves = 2
        r = P.Renderer(P.fog_box_scene(W, H), prm, W, H, seed=9)
        set_cam(P, r, "lens")
        names = [r.kernel_name()]
        for k in range(4):
            r.render_wave(k, k + 1)
            r.post_process_wave()
            names.append(r.kernel_name())
        out = (names, r.film(), r.counters(), r.training_stats())
        r.close()
        return out
    a = go()
    b = with_env({"VSPG_KERNEL": "lane"}, go)
    assert a[0][0] == "k_render_wave<HomogeneousMedium,guided,train>" and a[0][-1] == "k_render_wave<HomogeneousMedium,guided>", a[0]
    assert a[0] == b[0]
    for names, film, cnt, st in (a, b):
        assert np.isfinite(film).all() and np.all(film[..., 3] == 4) and film[..., :3].max() > 0
        assert st["training"] == 0 and st["iteration"] == 2 and min(st["n_regions"]) >= 1 and cnt["segments"] > 4 * W * H


# ---- 9. the scene-file route ---------------------------------------------------------------------------------------------------------------------
def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = (int(v) for v in f.readline().split())
        assert float(f.readline()) < 0
        return np.frombuffer(f.read(), dtype="<f4").reshape(h, w, 3)[::-1]


@pytest.fixture(scope="module")
def vspg_pbrt():
    exe = os.path.join(HOST, "vspg_pbrt")
    assert os.path.exists(exe), "host adapter not built"
    return exe


def api_image(P, w, h, spp, cam, **model):
    r = P.Renderer(P.fog_box_scene(w, h), P.app_f_params(), w, h)
    r.set_camera(cam, **model)
    for k in range(spp):
        r.render_wave(k, k + 1)
        r.post_process_wave()
    f = r.film()
    r.close()
    return (f[..., :3] / f[..., 3:4]).astype(np.float32)


def test_scene_file_render_equals_the_api(gpu_pkg, vspg_pbrt, tmp_path):
    """`vspg_pbrt tests/scenes/fog_box_dof.pbrt` == the fog box through the C-ABI with the same lens, bit for bit; likewise one
    orthographic and one spherical scene text written here."""
    P = gpu_pkg
    src = open(os.path.join(ROOT, "tests", "scenes", "fog_box_dof.pbrt")).read()
    lens_line = 'Camera "perspective" "float fov" 60 "float lensradius" 0.05 "float focaldistance" 1.95'
    assert lens_line in src
    cases = [(None, dict(model=M.PERSPECTIVE, lens_radius=0.05, focal_distance=1.95), None),
             ('Camera "orthographic" "float screenwindow" [ -0.8 0.8 -0.6 0.6 ] "float lensradius" 0.08 "float focaldistance" 1.5',
              dict(model=M.ORTHOGRAPHIC, lens_radius=0.08, focal_distance=1.5), (-0.8, 0.8, -0.6, 0.6)),
             ('Camera "spherical" "string mapping" "equirectangular"', dict(model=M.SPHERICAL_EQUIRECT), None)]
    for k, (camera, model, sw) in enumerate(cases):
        path = os.path.join(ROOT, "tests", "scenes", "fog_box_dof.pbrt")
        if camera:
            path = str(tmp_path / ("scene%d.pbrt" % k))
            open(path, "w").write(src.replace(lens_line, camera))
        out = tmp_path / ("out%d.pfm" % k)
        a = subprocess.run([vspg_pbrt, path, "--outfile", str(out)], capture_output=True, text=True)
        assert a.returncode == 0, a.stdout + a.stderr
        img = read_pfm(str(out))
        cam = P.camera_look_at_window(model["model"], (0, 0, -0.95), (0, 0, 0), (0, 1, 0), 60.0, 64, 48, screen_window=sw)
        want = api_image(P, 64, 48, 4, cam, **model)
        assert np.isfinite(img).all() and img.max() > 0
        assert np.array_equal(u32(img), u32(want)), camera
