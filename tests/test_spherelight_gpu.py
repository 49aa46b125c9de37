"""Sphere area lights on the device: vspg_light_sample_batch and vspg_light_pdf_batch against the float32 mirror of
tests/spherelight_model.py bit for bit, the three light samplers over a scene with every light kind, and the lights through whole
paths -- kernel families against each other, a deterministic known answer, two statistical ones, NEE against emitter hits, the
samplers against each other, guided renders.  The acceptance rule of the statistical tests is the one of tests/test_envlight_gpu.py
and tests/test_pointlight_gpu.py: |z| <= 4.5 with the standard error taken from the spread over separately cleared waves."""
import math
import os

import numpy as np
import pytest

import scenes
import spherelight_model as M

pytestmark = pytest.mark.gpu

f32 = np.float32
EPS = 2.0 ** -24
W, H = 24, 16
SAMPLERS = ["uniform", "power", "bvh"]
Z_MAX = 4.5      # tests/test_envlight_gpu.py, tests/test_pointlight_gpu.py


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


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


def vacuum_scene(P, w=W, h=H, eye=(0, 0.2, -3), look=(0, 0, 0), fov=40.0):
    s = scenes.empty_scene(w, h, eye=eye, look=look, fov=fov)
    s.medium.type = P.MEDIUM_NONE
    s.camera_outside_medium = 1
    return s


def add_fixture_sphere(P, s, spec, kd=(0, 0, 0)):
    """A fixture sphere of tests/spherelight_model.py as an emissive sphere of the scene; returns its mirror, built from the
    matrices the scene record holds."""
    k = s.n_spheres
    sp = s.spheres[k]
    m, mi = M.fixture_transforms(spec)
    sp.render_from_object[:] = [float(v) for v in m.reshape(16)]
    sp.object_from_render[:] = [float(v) for v in mi.reshape(16)]
    sp.radius = spec["radius"]
    sp.Kd[:] = kd
    sp.reverse_orientation, sp.material, sp.medium_interface = int(spec["reverse"]), 0, 0
    s.n_spheres = k + 1
    P.add_sphere_light(s, k, spec["Le"], two_sided=spec["two_sided"])
    return M.SphereLight(np.array(sp.render_from_object[:], f32), np.array(sp.object_from_render[:], f32), sp.radius,
                         np.array(s.sphere_Le[k][:], f32), spec["two_sided"], spec["reverse"])


def two_sphere_scene(P):
    s = vacuum_scene(P)
    return s, [add_fixture_sphere(P, s, M.LAMP), add_fixture_sphere(P, s, M.SHELL)]


def assert_bits(got, want, what):
    bad = np.argwhere(u32(got) != u32(want))
    assert bad.size == 0, (what, len(bad), "first", bad[0].tolist(), got[bad[0, 0]], want[bad[0, 0]])


# ---- 1. the batches against the mirror, bit for bit ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_spheres(gpu_pkg):
    P = gpu_pkg
    s, lights = two_sphere_scene(P)
    r = P.Renderer(s, sampler_params(P, "uniform"), W, H)
    yield r, lights
    r.close()


def test_sample_batch_equals_the_mirror(gpu_pkg, two_spheres):
    """4099 contexts; the uniform pick takes the lamp for u < 1/2 and the shell otherwise, and each element's context lies around the
    light it picks, in every branch the CPU test counts."""
    r, lights = two_spheres
    fx = [M.fixture_contexts(l, seed=5 + k) for k, l in enumerate(lights)]
    u = fx[0][2]
    pick = (u[:, 0] >= 0.5).astype(int)
    p = np.where(pick[:, None] == 0, fx[0][0], fx[1][0])
    nn = np.where(pick[:, None] == 0, fx[0][1], fx[1][1])
    got = r.light_sample_batch(p, nn, u)
    assert np.array_equal(got[:, 0].astype(int), pick) and np.all(got[:, 1] == 0.5) and np.all(got[:, 2] == 0.5)
    want = got.copy()
    seen = {}
    for li, light in enumerate(lights):
        sel = pick == li
        s = light.sample_li(p[sel], nn[sel], u[sel, 1:])
        rows = np.zeros((sel.sum(), 13), f32)
        rows[:, 0], rows[:, 1:4], rows[:, 4:7], rows[:, 7], rows[:, 8:11] = s["ok"], s["wi"], s["L"], s["pdf"], s["p"]
        rows[~s["ok"]] = 0
        want[sel, 3:] = rows
        seen[li] = {k: int(s[k].sum()) for k in ("ok", "inside", "taylor", "dark")}
    print("branches reached:", seen)
    assert seen[0]["dark"] > 100 and seen[1]["inside"] > 100 and seen[0]["taylor"] > 100 and seen[1]["taylor"] > 100
    assert_bits(got, want, "light_sample_batch")


@pytest.mark.parametrize("with_perr", [False, True])
@pytest.mark.parametrize("which", [0, 1])
def test_pdf_batch_equals_the_mirror(gpu_pkg, two_spheres, which, with_perr):
    """PDF_Li, the hit, L at the hit and its distance for the sampled directions and for 4099 independent ones."""
    r, lights = two_spheres
    light = lights[which]
    p, nn, u, perr, kind = M.fixture_contexts(light, seed=5 + which)
    s = light.sample_li(p, nn, u[:, 1:])
    indep = M.fixture_directions()
    sampled = np.where(s["ok"][:, None], s["wi"], indep[::-1])
    e = perr if with_perr else None
    for what, wi in (("sampled", sampled), ("independent", indep)):
        got = r.light_pdf_batch(which, p, nn, wi, ctx_perr=e)
        pdf, hit, L, t = light.probe(p, nn, wi, e)
        want = np.zeros_like(got)
        want[:, 0], want[:, 1], want[:, 2], want[:, 3:6], want[:, 6] = pdf, 0.5, hit, L, t
        print(what, "perr" if with_perr else "exact", "light", which, "hits", int(hit.sum()), "pdf > 0", int((pdf > 0).sum()))
        assert hit.sum() > 500 and (~hit).sum() > (0 if what == "sampled" else 500)
        assert_bits(got, want, (what, which, with_perr))


def test_pdf_batch_on_a_rectangle_and_its_refusals(gpu_pkg):
    """The probe on a rectangle light against light_pdf_li's arithmetic restated here in float32 (vspg_path.h: the ray from
    OffsetRayOrigin against the plane, (1 / area) * d^2 / |n . wi| from the re-projected point), and VSPG_EINVAL for lights without
    a shape."""
    P = gpu_pkg
    s = vacuum_scene(P)
    scenes.add_quad(s, (-1.5, 2.0, 0.5), (0.5, 0, 0), (0, 0, 0.5), kd=(0, 0, 0), le=(4.0, 3.0, 2.0))      # n = -y, area 0.25
    P.add_infinite_light(s, P.LIGHT_DISTANT, (1, 1, 1), (0, 1, 0))
    P.add_point_light(s, (1, 1, 1), (0, 0.5, 0))
    add_fixture_sphere(P, s, M.LAMP)
    r = P.Renderer(s, sampler_params(P, "uniform"), W, H)
    rng = np.random.default_rng(9)
    n = M.N_FIXTURE
    p = rng.uniform(-2, 2, (n, 3)).astype(f32)
    p[:, 1] = rng.uniform(-1, 1.9, n).astype(f32)
    target = np.array([-1.5, 2.0, 0.5]) + rng.uniform(-0.2, 0.7, (n, 1)) * [0.5, 0, 0] + rng.uniform(-0.2, 0.7, (n, 1)) * [0, 0, 0.5]
    wi = target - p
    wi = (wi / np.linalg.norm(wi, axis=1, keepdims=True)).astype(f32)
    nn = np.zeros((n, 3), f32)
    got = r.light_pdf_batch(0, p, nn, wi)
    for bad in (1, 2, 4, -1):
        with pytest.raises(P.VspgError) as e:
            r.light_pdf_batch(bad, p[:4], nn[:4], wi[:4])
        assert e.value.code == P.VSPG_EINVAL
    assert r.light_pdf_batch(3, p[:4], nn[:4], wi[:4]).shape == (4, P.LIGHT_PDF_OUT)
    r.close()
    # quad_hit_uv / quad_point / light_pdf_li in float32; medium vertices: the ray starts at p
    qn, p00, e1, e2 = np.array([0, -1, 0], f32), np.array([-1.5, 2.0, 0.5], f32), np.array([0.5, 0, 0], f32), np.array([0, 0, 0.5], f32)
    corners = [p00, p00 + e1, p00 + e2, (p00 + e1) + e2]
    g6 = f32(6 * EPS) / (f32(1) - f32(6 * EPS))
    perr = ((np.abs(corners[0]) + np.abs(corners[2])) + (np.abs(corners[1]) + np.abs(corners[3]))) * g6
    o = (p + p) / f32(2)
    denom, num = M.dot(qn, wi), M.dot(qn, p00 - o)
    with np.errstate(all="ignore"):
        t = num / denom
        hit = (((num > 0) & (denom > 0)) | ((num < 0) & (denom < 0))) & (t > 0)
        rel = (o + wi * t[:, None]) - p00
        uu, vv = M.dot(rel, e1) * (f32(1) / M.len2(e1)), M.dot(rel, e2) * (f32(1) / M.len2(e2))
        hit &= ~((uu < 0) | (uu > 1) | (vv < 0) | (vv > 1))
        ph = p00 + (e1 * uu[:, None] + e2 * vv[:, None])
        ph = M.P3i.from_err(ph, np.broadcast_to(perr, ph.shape)).mid()
        pdf = (f32(1) / f32(0.25)) * (M.len2(o - ph) / np.abs(M.dot(qn, -wi)))
    pdf = np.where(hit & ~np.isinf(pdf), pdf, f32(0))
    want = np.zeros_like(got)
    want[:, 0], want[:, 1], want[:, 2], want[:, 6] = pdf, f32(1) / f32(4), hit, np.where(hit, t, 0)
    want[:, 3:6] = np.where((hit & (M.dot(qn, -wi) >= 0))[:, None], np.array([4.0, 3.0, 2.0], f32), 0)
    assert hit.sum() > 500 and (~hit).sum() > 500
    assert_bits(got, want, "rectangle")


# ---- 2. the three samplers over every light kind -------------------------------------------------------------------------------------
def mixed_scene(P, medium="none"):
    """Light list: 0 an emissive rectangle, 1 a distant light, 2 a point light, 3 the lamp, 4 the shell."""
    if medium == "grid":
        import ctypes as C
        s = scenes.empty_scene(W, H, eye=(0.0, 0.6, -4.2), look=(0, 0.15, 0), fov=38.0)
        dens = (np.random.default_rng(4).random(64) * 0.9 + 0.1).astype(f32)
        m = s.medium
        m.type = P.MEDIUM_GRID
        m.sigma_a[:] = (0.03,) * 3
        m.sigma_s[:] = (0.97,) * 3
        m.g = 0.6
        m.nx = m.ny = m.nz = 4
        m.bounds_min[:] = (-0.8, -0.5, -0.8)
        m.bounds_max[:] = (0.8, 0.9, 0.8)
        m.density = dens.ctypes.data_as(C.POINTER(C.c_float))
        s._density_keepalive = dens
    else:
        s = vacuum_scene(P)
    scenes.add_quad(s, (-6, -1.25, -6), (0, 0, 12), (12, 0, 0), kd=(0.4, 0.35, 0.3))                 # floor, n = +y
    scenes.add_quad(s, (-1.5, 2.0, 0.5), (0.5, 0, 0), (0, 0, 0.5), kd=(0, 0, 0), le=(4.0, 3.0, 2.0))  # emitter, n = -y
    P.add_infinite_light(s, P.LIGHT_DISTANT, (3.0, 2.5, 2.0), (0.4, 0.8, -0.3))
    P.add_point_light(s, (3.0, 2.0, 1.0), (0.2, 0.3, -0.1))
    return s, [add_fixture_sphere(P, s, M.LAMP, kd=(0.3, 0.3, 0.3)), add_fixture_sphere(P, s, M.SHELL)]


SAMPLER_CONTEXTS = np.array([[0.1, 0.3, -0.4], [-1.2, 1.0, 0.7], [0.5, -1.0, 0.3], [1.0, 3.0, -1.0]], f32)


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_sampler_consistency(gpu_pkg, sampler):
    """Per context 2^14 stratified picks: Sample's pmf is PMF(ctx, light); one pmf per (context, light); the pmfs over the list sum
    to 1 within the float32 summation bound the other light tests use (8 * 2 eps, where every light has a positive importance); the
    sphere lights are picked."""
    P = gpu_pkg
    n = 1 << 14
    u = np.zeros((n, 3), f32)
    u[:, 0] = ((np.arange(n) + 0.5) / n).astype(f32)
    u[:, 1:] = np.random.default_rng(2).random((n, 2)).astype(f32)
    normals = np.array([[0, 0, 0], [0, 0, 0], [0, 1, 0], [0.6, -0.8, 0]], f32)
    s, _ = mixed_scene(P)
    r = P.Renderer(s, sampler_params(P, sampler), W, H)
    for k, (c, nn) in enumerate(zip(SAMPLER_CONTEXTS, normals)):
        got = r.light_sample_batch(np.broadcast_to(c, (n, 3)), np.broadcast_to(nn, (n, 3)), u)
        g = got[got[:, 0] >= 0]
        assert len(g) == n or sampler == "bvh"
        assert np.array_equal(u32(g[:, 1]), u32(g[:, 2])), (sampler, k)
        idx = g[:, 0].astype(int)
        pmf = np.zeros(5)
        for li in range(5):
            vals = np.unique(g[idx == li, 1])
            assert len(vals) <= 1, (sampler, k, li, vals)
            pmf[li] = vals[0] if len(vals) else 0.0
        count = np.bincount(idx, minlength=5)
        print(sampler, "context", k, "pmf", pmf, "picks", count)
        for li in range(5):
            sd = math.sqrt(n * pmf[li] * (1 - pmf[li]))
            assert abs(count[li] - n * pmf[li]) <= Z_MAX * sd + 1, (sampler, k, li, count[li], n * pmf[li])
        if sampler == "uniform":
            assert np.all(pmf == f32(1) / f32(5))
        if sampler != "bvh" or (len(g) == n and np.all(pmf > 0)):
            assert abs(pmf.sum() - 1) <= 8 * 2 * EPS, (sampler, k, pmf)
        assert count[4] > 0 and (count[3] > 0 or sampler == "bvh")      # the shell (two-sided, all around) is always picked
        for li in (3, 4):      # the pick's PMF is also what the pdf probe reports for that light
            if count[li]:
                probe = r.light_pdf_batch(li, c[None], nn[None], np.array([[0, 0, 1]], f32))
                assert u32(probe[0, 1]) == u32(f32(pmf[li]))
    r.close()


# ---- 3. kernel families ----------------------------------------------------------------------------------------------------------------
def lamp_and_shell_scene(P, which, w=W, h=H):
    """One small lamp in front of the camera and one large reversed two-sided sphere enclosing the camera and everything else:
    contexts lie outside the one and inside the other."""
    s = scenes.empty_scene(w, h, eye=(0, 0.3, -3), look=(0, 0, 0))
    m = s.medium
    if which == "homogeneous":
        m.type = P.MEDIUM_HOMOGENEOUS
        m.sigma_a[:] = (0.05, 0.05, 0.05)
        m.sigma_s[:] = (0.4, 0.4, 0.4)
        m.g = 0.3
    else:
        import ctypes as C
        dens = (np.random.default_rng(4).random(64) * 0.9 + 0.1).astype(f32)
        m.type = P.MEDIUM_GRID
        m.sigma_a[:] = (0.03,) * 3
        m.sigma_s[:] = (0.97,) * 3
        m.g = 0.6
        m.nx = m.ny = m.nz = 4
        m.bounds_min[:] = (-1.5, -1.0, -1.5)
        m.bounds_max[:] = (1.5, 1.5, 1.5)
        m.density = dens.ctypes.data_as(C.POINTER(C.c_float))
        s._density_keepalive = dens
    scenes.add_quad(s, (-6, -1.25, -6), (0, 0, 12), (12, 0, 0), kd=(0.4, 0.35, 0.3))
    lamp = dict(M.LAMP)
    shell = dict(M.SHELL, center=(0.0, 0.5, 0.0), radius=6.5, Le=(0.05, 0.06, 0.08))
    return s, [add_fixture_sphere(P, s, lamp, kd=(0.2, 0.2, 0.2)), add_fixture_sphere(P, s, shell, kd=(0.5, 0.5, 0.5))]


def render(P, scene, prm, kernel, waves=4, w=W, h=H):
    def go():
        r = P.Renderer(scene, prm, w, h)
        name = r.kernel_name()
        for k in range(waves):
            r.render_wave(k, k + 1)
            r.post_process_wave()
        film = r.film()
        r.close()
        return name, film
    return with_kernel(kernel, go)


@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("which", ["homogeneous", "grid"])
def test_kernel_families_agree(gpu_pkg, which, sampler):
    P = gpu_pkg
    scene, _ = lamp_and_shell_scene(P, which)
    prm = sampler_params(P, sampler)
    name_d, film_d = render(P, scene, prm, None)
    name_l, film_l = render(P, scene, prm, "lane")
    print(which, sampler, "default:", name_d, "| lane:", name_l)
    assert name_d != name_l and name_l.startswith("k_render_wave<")
    assert name_d.startswith("k_render_wave_wg2<HomogeneousMedium>" if which == "homogeneous" else "k_wf_")
    assert np.isfinite(film_d).all() and film_d[..., :3].max() > 0
    assert np.array_equal(u32(film_d), u32(film_l))


# ---- 4. a known answer, deterministic ---------------------------------------------------------------------------------------------------
def test_camera_inside_a_black_emissive_sphere(gpu_pkg):
    """The camera inside a closed, reversed, emissive sphere with Kd = 0 and no medium: the camera ray hits the emitter at depth 0 (no
    MIS: L += beta * Le / r_u with beta = r_u = 1), the surface has no lobes and the path ends.  Every pixel of every wave is Le, bit
    for bit, on both kernel families."""
    P = gpu_pkg
    Le = np.array([1.75, 0.625, 3.0], f32)
    for kernel in (None, "lane"):
        s = vacuum_scene(P, eye=(0.1, -0.2, 0.3), look=(0.5, 0.1, 1.0))
        add_fixture_sphere(P, s, dict(center=(0, 0, 0), radius=2.0, Le=tuple(Le), two_sided=False, reverse=True))
        def go():
            r = P.Renderer(s, P.app_f_params(), W, H)
            films = []
            for w in range(3):
                r.film_clear()
                r.render_wave(w, w + 1)
                films.append(r.film())
            r.close()
            return films
        for f in with_kernel(kernel, go):
            assert np.all(f[..., 3] == 1) and np.array_equal(u32(f[..., :3]), u32(np.broadcast_to(Le, (H, W, 3))))


# ---- 5. known answers, statistical ----------------------------------------------------------------------------------------------------
def wave_means(r, waves, pick):
    out = []
    for w in range(waves):
        r.film_clear()
        r.render_wave(w, w + 1)
        f = r.film()
        out.append(pick(f[..., :3].astype(np.float64) / f[..., 3:4]))
    return np.array(out)


def test_plate_under_a_sphere_light(gpu_pkg):
    """Scene (a): a small diffuse plate (Kd) facing a sphere light (radius r, radiance L) whose centre lies at distance d on the
    plate's normal, in vacuum, maxdepth 1.  The reflected radiance at the plate's centre is
        Lo = (Kd / pi) * L * Integral_cone cos(theta) d omega = (Kd / pi) * L * 2 pi * Integral_0^thetamax cos sin d theta
           = Kd * L * sin^2(thetamax) = Kd * L * (r / d)^2
    (tests/test_spherelight_model.py reproduces it by quadrature).  The camera looks at the plate's centre from the side, through a
    1-degree field of view: across those pixels the plate point moves by +-0.01, which changes (r / d)^2 cos-weighted by less than
    1e-3 relative -- below the standard error; the comparison is |z| <= 4.5 over 32 waves.  The emitter hit at depth 1 is not seen
    (maxdepth 1 ends the path at the plate), so NEE alone carries the answer."""
    P = gpu_pkg
    r_, d_, Kd, L = 0.5, 2.0, 0.6, 3.0
    s = vacuum_scene(P, w=16, h=16, eye=(1.5, 1.0, 0.0), look=(0, 0, 0), fov=0.6)
    scenes.add_quad(s, (-0.05, 0, -0.05), (0, 0, 0.1), (0.1, 0, 0), kd=(Kd,) * 3)      # n = +y
    add_fixture_sphere(P, s, dict(center=(0, d_, 0), radius=r_, Le=(L,) * 3, two_sided=False, reverse=False))
    prm = P.app_f_params()
    prm.maxdepth = 1
    r = P.Renderer(s, prm, 16, 16)
    m = wave_means(r, 32, lambda img: img[6:10, 6:10].mean())
    name = r.kernel_name()
    r.close()
    want = Kd * L * (r_ / d_) ** 2
    se = m.std(ddof=1) / math.sqrt(len(m))
    print(name, "mean %.6f +- %.6f, closed form %.6f, z %.2f" % (m.mean(), se, want, (m.mean() - want) / se))
    assert se > 0 and abs(m.mean() - want) <= Z_MAX * se + 1e-3 * want


def test_furnace(gpu_pkg):
    """Scene (b): the camera inside the reversed emissive sphere with albedo rho, no medium.  Every ray sees the emitter, so the
    radiance along the camera ray is L * Sum_{k = 0..maxdepth} rho^k: Li adds emission at the camera hit (depth 0) and after each of
    the bounces it allows -- `if (depth++ >= maxDepth) return` (guidedvolpathvspgintegrator.cpp:~432) runs AFTER the emission of the
    hit was added, so hits at depth 0 .. maxdepth all contribute and the upper limit of the sum is maxdepth itself."""
    P = gpu_pkg
    L, rho, maxdepth = 0.5, 0.6, 3
    s = vacuum_scene(P, w=16, h=16, eye=(0.2, 0.1, -0.3), look=(0, 0, 1))
    add_fixture_sphere(P, s, dict(center=(0, 0, 0), radius=1.5, Le=(L,) * 3, two_sided=False, reverse=True), kd=(rho,) * 3)
    prm = P.app_f_params()
    prm.maxdepth = maxdepth
    r = P.Renderer(s, prm, 16, 16)
    m = wave_means(r, 32, lambda img: img.mean())
    r.close()
    want = M.furnace_series64(L, rho, maxdepth)
    se = m.std(ddof=1) / math.sqrt(len(m))
    print("furnace mean %.6f +- %.6f, series %.6f, z %.2f" % (m.mean(), se, want, (m.mean() - want) / se))
    assert se > 0 and abs(m.mean() - want) <= Z_MAX * se


def welch(a, b):
    return (a.mean() - b.mean()) / math.sqrt(a.var(ddof=1) / len(a) + b.var(ddof=1) / len(b))


def test_nee_and_emitter_hits_share_an_expectation(gpu_pkg):
    """The lamp-in-fog scene with usenee true and false (false: emitter hits alone carry the light): whole-film means of 32 + 32
    separately cleared waves, Welch's statistic.  Ties SampleLi, PDF_Li, L and the PMF together inside a medium: a wrong PDF_Li
    shifts the MIS weights of one estimator only."""
    P = gpu_pkg
    means = {}
    for nee in (1, 0):
        s, _ = lamp_and_shell_scene(P, "homogeneous")
        prm = P.app_f_params()
        prm.usenee = nee
        r = P.Renderer(s, prm, W, H)
        means[nee] = wave_means(r, 32, lambda img: img.mean())
        r.close()
    z = welch(means[1], means[0])
    print("usenee 1: %.5f, usenee 0: %.5f, z = %.2f" % (means[1].mean(), means[0].mean(), z))
    assert means[1].mean() > 0 and abs(z) <= Z_MAX


def test_uniform_and_bvh_share_an_expectation(gpu_pkg):
    P = gpu_pkg
    means = {}
    for sampler in ("uniform", "bvh"):
        s, _ = mixed_scene(P, "grid")
        r = P.Renderer(s, sampler_params(P, sampler), W, H)
        means[sampler] = wave_means(r, 32, lambda img: img.mean())
        r.close()
    z = welch(means["uniform"], means["bvh"])
    print("uniform %.5f, bvh %.5f, z = %.2f" % (means["uniform"].mean(), means["bvh"].mean(), z))
    assert means["uniform"].mean() > 0 and abs(z) <= Z_MAX


# ---- 6. guided ----------------------------------------------------------------------------------------------------------------------------
def test_guided_training_records_surface_emission_and_kernels_agree(gpu_pkg):
    """Reference-default options with in-loop training on the lamp-and-shell scene over the 4^3 grid (guided renders of a full scene
    over a homogeneous medium have one kernel, the per-lane one; over a grid the pipeline and the per-lane kernel both serve): the training statistics show surface-emission
    samples (paths that HIT the lamp or the shell hand their emission to the recorder, add_surface_emission: counted with NEE off), and with the trained
    field in place the workgroup and the per-lane kernel agree bit for bit (compared as tests/test_pointlight_gpu.py compares them)."""
    P = gpu_pkg
    scene, _ = lamp_and_shell_scene(P, "grid")
    prm = P.default_params()
    prm.guide_num_training_waves = 4
    t = P.Renderer(scene, prm, W, H)
    assert "train" in t.kernel_name()
    for w in range(4):
        t.render_wave(w, w + 1)
        t.post_process_wave()
    assert np.isfinite(t.film()).all() and t.film()[..., :3].max() > 0
    st = t.training_stats()
    print("training stats:", st)
    assert st["training"] == 0 and st["iteration"] == 4, st
    # surface emission reaches the recorder: with NEE off, emitter hits are the only radiance a path can carry, so every non-zero
    # radiance sample of a training wave exists because add_surface_emission ran on a sphere-light hit
    prm_hits = P.default_params()
    prm_hits.guide_num_training_waves = 4
    prm_hits.usenee = 0
    h = P.Renderer(scene, prm_hits, W, H)
    h.render_wave(0, 1)
    hs = h.training_stats()
    h.close()
    print("training stats with NEE off, before the first update:", hs)
    assert hs["n_samples"] > 128, hs
    fields = []
    for vol in (0, 1):
        nodes, regs, nn, nr = t.get_guiding_field(vol)
        fields.append(P.Field(list(nodes)[:nn], list(regs)[:nr]))
    vsp, ready = t.vsp_buffer()
    t.close()
    films = {}
    for kernel in (None, "lane"):
        def wave4():
            r = P.Renderer(scene, prm, W, H)
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
