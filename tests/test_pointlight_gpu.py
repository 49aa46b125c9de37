"""Point and spot lights on the device: vspg_light_sample_batch against the float32 mirror of tests/pointlight_model.py bit for bit,
the three light samplers over a scene with every light kind, and the lights through whole paths -- kernel families against each
other, a deterministic known answer, a statistical one (a spot in fog against a float64 quadrature), the samplers against each
other, guided renders, and the scene-file route.  Light list of the five-light scene: 0 the emissive rectangle, 1 the distant light,
2 the uniform sky, 3 the point light, 4 the spot."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import pointlight_model as M
import scenes
from conftest import ROOT

pytestmark = pytest.mark.gpu

f32 = np.float32
EPS = 2.0 ** -24
W, H = 32, 24
HOST = os.path.join(ROOT, "vspg-pbrt-v4_amd", "host")
COLS = {"index": 0, "pmf": 1, "PMF": 2, "valid": 3, "wi": slice(4, 7), "L": slice(7, 10), "pdf": 10, "pLight": slice(11, 14), "delta": 14, "zero": 15}
SAMPLERS = ["uniform", "power", "bvh"]

POINT_I, POINT_FROM = (3.0, 2.0, 1.0), (0.2, 0.3, -0.1)
SPOT_I, SPOT_FROM, SPOT_TO, SPOT_CONE = (6.0, 5.0, 4.0), (0.4, 1.5, -0.3), (-0.2, 0.1, 0.6), (30.0, 5.0)
QUAD_LE, SUN_L, SUN_W, SKY_L = (4.0, 3.0, 2.0), (3.0, 2.5, 2.0), (0.4, 0.8, -0.3), (0.25, 0.35, 0.5)


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ctm_oblique():
    return M.mat4_mul(M.translate((0.3, -0.2, 0.5)), M.rotate(37.0, (1, 2, 3)))


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


def add_lights(P, s, point=True, spot=True, ctm=None):
    """The two lights of this file, and their mirrors in light-list order."""
    mirrors = []
    if point:
        P.add_point_light(s, POINT_I, POINT_FROM)
        mirrors.append(M.point_light(POINT_I, POINT_FROM))
    if spot:
        P.add_spot_light(s, SPOT_I, SPOT_FROM, SPOT_TO, *SPOT_CONE, ctm=ctm)
        mirrors.append(M.spot_light(SPOT_I, SPOT_FROM, SPOT_TO, *SPOT_CONE, ctm=ctm))
    return mirrors


def vacuum_scene(P):
    s = scenes.empty_scene(W, H, eye=(0, 0.2, -3), look=(0, 0, 0))
    s.medium.type = P.MEDIUM_NONE
    s.camera_outside_medium = 1
    return s


def five_light_scene(P, medium="none"):
    """An emissive rectangle over a floor, a distant light, a uniform sky, the point light and the spot (under a CTM)."""
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
    P.add_infinite_light(s, P.LIGHT_UNIFORM_INFINITE, SKY_L)
    mirrors = add_lights(P, s, ctm=ctm_oblique())
    return s, mirrors


# ---- 1. the batch against the mirror, bit for bit ----------------------------------------------------------------------------------
def contexts_around(light, n, seed):
    """n contexts around a light: every regime of a spot's falloff (by the angle to its axis, in light space), points on the axis,
    points 1e-3 and 1e3 scene units away; the first half medium vertices (n = 0), the rest surface contexts."""
    rng = np.random.default_rng(seed)
    if light.kind == M.LIGHT_SPOT:
        end, start = math.acos(float(light.cos_end)), math.acos(float(light.cos_start))
        theta = np.concatenate([rng.uniform(0, start, n // 4), rng.uniform(start, end, n // 4), rng.uniform(end, math.pi, n // 4),
                                np.zeros(n // 16), rng.uniform(start - 1e-3, end + 1e-3, n - 3 * (n // 4) - n // 16)])
    else:
        theta = np.arccos(rng.uniform(-1, 1, n))
    phi = rng.uniform(0, 2 * math.pi, n)
    local = np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], axis=1)
    d = local @ light.m[:3, :3].astype(np.float64).T
    r = np.exp(rng.uniform(math.log(0.05), math.log(20.0), n))
    r[::7] = 1e-3
    r[3::7] = 1e3
    order = rng.permutation(n)
    p = (light.pos.astype(np.float64) + d * r[:, None]).astype(f32)[order]
    nn = rng.normal(size=(n, 3))
    nn = (nn / np.linalg.norm(nn, axis=1, keepdims=True)).astype(f32)
    nn[: n // 2] = 0
    return p, nn, rng.random((n, 3)).astype(f32)


def mirror_rows(got, p, lights_by_index, sun=None):
    """The mirror's rows [3:16] for the lights the device picked; rows of other lights (the rectangle: pinned by the oracle's tests) are
    copied from the device and not judged."""
    want = got.copy()
    idx = got[:, 0].astype(int)
    for li, light in lights_by_index.items():
        sel = idx == li
        valid, wi, L, pdf, pl, delta = light.sample_li(p[sel])
        rows = np.zeros((sel.sum(), 13), f32)
        rows[:, 0], rows[:, 1:4], rows[:, 4:7], rows[:, 7], rows[:, 8:11], rows[:, 11] = valid, wi, L, pdf, pl, delta
        rows[~valid] = 0
        want[sel, 3:] = rows
    if sun is not None:      # DistantLight::SampleLi: wi = w_light, L, pdf 1, a delta light (pLight depends on the scene radius: not judged)
        sel = idx == sun[0]
        want[sel, 3], want[sel, 4:7], want[sel, 7:10], want[sel, 10], want[sel, 14] = 1, sun[1], sun[2], 1, 1
    return want


def assert_rows_equal(got, want, what):
    for name, c in COLS.items():
        bad = np.argwhere(u32(got[:, c]) != u32(want[:, c]))
        assert bad.size == 0, (what, name, len(bad), "first query", int(bad[0, 0]), got[bad[0, 0]], want[bad[0, 0]])


def test_batch_equals_the_mirror(gpu_pkg):
    P = gpu_pkg
    total = 0
    # one point light; one spot light, oblique axis under a CTM
    for what, kw, n in (("point", dict(spot=False), 1024), ("spot", dict(point=False, ctm=ctm_oblique()), 1536)):
        s = vacuum_scene(P)
        (light,) = add_lights(P, s, **kw)
        r = P.Renderer(s, P.app_f_params(), W, H)
        p, nn, u = contexts_around(light, n, 11)
        got = r.light_sample_batch(p, nn, u)
        r.close()
        assert np.all(got[:, 0] == 0) and np.all(got[:, 1] == 1) and np.all(got[:, 2] == 1)      # the scene's only light, pmf 1
        want = mirror_rows(got, p, {0: light})
        assert_rows_equal(got, want, what)
        valid = got[:, 3] == 1
        if what == "spot":      # the regimes are there: no sample outside the cone, the full intensity, the falloff band, the axis
            full = valid & np.all(got[:, 7:10] == light.I[None, :] / ((light.pos[None, :] - p) ** 2).sum(axis=1, dtype=f32)[:, None], axis=1)
            assert (~valid).sum() > 300 and full.sum() > 300 and (valid & ~full).sum() > 300
        else:
            assert valid.all()
        assert np.all(got[valid, 10] == 1) and np.all(got[valid, 14] == 1) and np.all(got[valid, 11:14] == light.pos)
        dist = np.linalg.norm(p.astype(np.float64) - light.pos, axis=1)
        assert (dist < 2e-3).sum() > 100 and (dist > 500).sum() > 100
        total += n
    # both together, with a rectangle emitter, a distant light and a sky, under the uniform pick
    s, (point, spot) = five_light_scene(P)
    r = P.Renderer(s, sampler_params(P, "uniform"), W, H)
    n = 4096 - total
    p = np.concatenate([contexts_around(point, n // 2, 12)[0], contexts_around(spot, n - n // 2, 13)[0]])
    _, nn, u = contexts_around(spot, n, 14)
    got = r.light_sample_batch(p, nn, u)
    r.close()
    sun_w = np.array(SUN_W, np.float64)
    sun_w = (sun_w / np.linalg.norm(sun_w)).astype(f32)
    got_sun = got[got[:, 0] == 1]
    assert len(got_sun) > 100 and np.allclose(got_sun[:, 4:7], sun_w, atol=1e-6)      # (normalised by the binding: take the device's bits)
    want = mirror_rows(got, p, {3: point, 4: spot}, sun=(1, got_sun[0, 4:7], np.array(SUN_L, f32)))
    assert_rows_equal(got, want, "five lights")
    picked = np.bincount(got[:, 0].astype(int), minlength=5)
    assert np.all(picked > 200) and np.all(got[:, 1] == f32(1) / f32(5)) and np.all(got[got[:, 0] == 2, 3] == 0)      # the sky gives no sample


# ---- 2. the three samplers over the five lights ------------------------------------------------------------------------------------
def scene_radius(corners):
    """Bounds3::BoundingSphere of the scene bounds, in float32 as the host computes it."""
    c = np.asarray(corners, f32)
    lo, hi = c.min(axis=0), c.max(axis=0)
    d = (lo + hi) / f32(2) - hi
    return np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])


# the first lies on the spot's axis, 1.2 units in front of it (every light has a positive importance there); the last behind the spot
SAMPLER_CONTEXTS = np.array([[0.158, 0.245, 0.926], [-1.2, 1.0, 0.7], [0.5, -1.0, 0.3], [1.0, 3.0, -1.0]], f32)


@pytest.fixture(scope="module")
def sampler_runs(gpu_pkg):
    """Per sampler: 2^16 stratified picks for each of four contexts (two as medium vertices, two with a normal)."""
    P = gpu_pkg
    n = 1 << 16
    u = np.zeros((n, 3), f32)
    u[:, 0] = ((np.arange(n) + 0.5) / n).astype(f32)
    u[:, 1:] = np.random.default_rng(2).random((n, 2)).astype(f32)
    normals = np.array([[0, 0, 0], [0, 0, 0], [0, 1, 0], [0.6, -0.8, 0]], f32)
    runs = {}
    for sampler in SAMPLERS:
        s, mirrors = five_light_scene(P)
        r = P.Renderer(s, sampler_params(P, sampler), W, H)
        runs[sampler] = [r.light_sample_batch(np.broadcast_to(c, (n, 3)), np.broadcast_to(nn, (n, 3)), u) for c, nn in zip(SAMPLER_CONTEXTS, normals)]
        r.close()
    return runs, mirrors


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_sampler_consistency(gpu_pkg, sampler_runs, sampler):
    runs, (point, spot) = sampler_runs
    n = 1 << 16
    # the spot's bounding cone: context 3 sits behind the light, further than theta_o + theta_e from its axis
    pos, axis, phi, cos_o, cos_e = spot.bounds()
    to_ctx = SAMPLER_CONTEXTS[3].astype(np.float64) - pos
    assert math.acos(float(to_ctx @ axis / np.linalg.norm(to_ctx))) > math.acos(float(cos_o)) + math.acos(float(cos_e)) + 0.2
    to_ctx = SAMPLER_CONTEXTS[0].astype(np.float64) - pos
    assert math.acos(float(to_ctx @ axis / np.linalg.norm(to_ctx))) < 0.01 and abs(np.linalg.norm(to_ctx) - 1.2) < 0.01
    for k, got in enumerate(runs[sampler]):
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
        # picks reproduce the pmf: 4.5 binomial standard deviations (the stratified variates stay far inside)
        count = np.bincount(idx, minlength=5)
        for li in range(5):
            sd = math.sqrt(n * pmf[li] * (1 - pmf[li]))
            assert abs(count[li] - n * pmf[li]) <= 4.5 * sd + 1, (sampler, k, li, count[li], n * pmf[li])
        if sampler == "uniform":
            assert np.all(pmf == f32(1) / f32(5))
        if sampler == "bvh":
            # a light that is never picked has importance zero here; where every bounded light has a positive one the pmfs sum to 1:
            # the two infinite lights share pInfinite = 2 / 3 (8 ulp: a product of at most three quotients per light, five terms)
            assert pmf[1] == pmf[2] == f32(f32(2) / f32(3)) / f32(2)
            if picked.all() and np.all(pmf > 0):
                assert abs(pmf.sum() - 1) <= 8 * 2 * EPS, (k, pmf)
            if k == 3:
                assert count[4] == 0 and count[3] > 0, count      # outside the spot's bounding cone; the point light shines everywhere
            if k == 0:
                assert np.all(count > 0)
    if sampler == "power":
        r = scene_radius([(-6, -1.25, -6), (6, -1.25, 6), (-1.5, 2.0, 0.5), (-1.0, 2.0, 1.0)])
        phis = [M.PI * f32(0.25) * np.array(QUAD_LE, f32), M.PI * (r * r) * np.array(SUN_L, f32), f32(4) * M.PI * M.PI * (r * r) * np.array(SKY_L, f32),
                point.phi(), spot.phi()]
        want = M.power_pmf(phis)
        got_pmf = np.array([np.unique(np.concatenate([g[g[:, 0] == li, 1] for g in runs[sampler]])) for li in range(5)]).reshape(5)
        ulp = np.abs(u32(got_pmf).astype(np.int64) - u32(want).astype(np.int64))
        print("power pmf", got_pmf, "model", want, "ulp", ulp)
        assert np.all(ulp <= 2)


# ---- 3. kernel families ----------------------------------------------------------------------------------------------------------------
def family_scene(P, which):
    """A point light inside the medium and a spot aimed through it."""
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
    add_lights(P, s, ctm=None)
    return s


def render(P, scene, prm, kernel, waves=4):
    def go():
        r = P.Renderer(scene, prm, W, H)
        name = r.kernel_name()
        for w in range(waves):
            r.render_wave(w, w + 1)
            r.post_process_wave()
        film = r.film()
        r.close()
        return name, film
    return with_kernel(kernel, go)


@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("which", ["homogeneous", "grid", "grid_boundary"])
def test_kernel_families_agree(gpu_pkg, which, sampler):
    P = gpu_pkg
    scene = family_scene(P, which)
    prm = sampler_params(P, sampler)
    name_d, film_d = render(P, scene, prm, None)
    name_l, film_l = render(P, scene, prm, "lane")
    print(which, sampler, "default:", name_d, "| lane:", name_l)
    assert name_d != name_l and name_l.startswith("k_render_wave<")
    assert name_d.startswith("k_render_wave_wg2<HomogeneousMedium>" if which == "homogeneous" else "k_wf_")
    assert np.isfinite(film_d).all() and film_d[..., :3].max() > 0
    assert np.array_equal(u32(film_d), u32(film_l))


# ---- 4. a known answer, deterministic ---------------------------------------------------------------------------------------------------
def pixel_corner_dirs(scene):
    """Unit directions of the camera rays through the corners of every pixel: (H + 1, W + 1, 3), float64."""
    c = scene.camera
    x, y = np.meshgrid(np.arange(W + 1, dtype=np.float64), np.arange(H + 1, dtype=np.float64))
    v = np.stack([c.sx * x + c.ox, c.sy * y + c.oy, np.ones_like(x)], axis=-1)
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    return v[..., 0:1] * np.array(c.right[:]) + v[..., 1:2] * np.array(c.up[:]) + v[..., 2:3] * np.array(c.fwd[:])


@pytest.mark.parametrize("light", ["point", "spot"])
def test_light_at_the_centre_of_a_diffuse_sphere(gpu_pkg, light):
    """A diffuse sphere of radius R around the camera and the light, a medium with zero coefficients, maxdepth 1: every pixel of one
    wave is direct light alone, Kd / pi * I / R^2 * |cos| with cos = 1 (the light sits on every normal), weight 1.
    The bound, relative, with eps = 2^-24 and gamma(5) = 5 eps / (1 - 5 eps) (util/float.h:195):
      * the re-projected hit point lies within gamma(5) (|x| + |y| + |z|) <= sqrt(3) gamma(5) R of the sphere, and the shading
        context is that point pushed out of its error box along the normal (OffsetRayOrigin: the same length again, then one float up
        per component): the distance to the light is R (1 + e) with |e| <= 2 sqrt(3) gamma(5) + 2 eps; it enters squared: 2 |e|;
      * 1 / d^2 -- a difference, three squares, two sums, a division --                    6 eps
      * wi and the normal are both that point's direction to the rounding of two Normalize (5.5 eps each, perpendicular to first
        order: the cosine loses e^2), the dot product's five operations                      5 eps
      * f = Kd * (1 / pi) with the constant's own rounding, f * |cos|, * L, / the pmf's 1   5 eps
    2 (2 sqrt(3) gamma(5) + 2 eps) + 16 eps = 3.3e-6: near 1e-5, as expected.
    The spot (axis +x, 90 degrees with a falloff of 10) lights half the sphere: pixels whose four corners lie within 78 degrees of the
    axis hold the same value, pixels beyond 92 degrees an exact 0."""
    P = gpu_pkg
    R, Kd, I = 1.75, (0.5, 0.25, 0.75), (3.0, 2.0, 1.0)
    s = scenes.empty_scene(W, H, eye=(0, 0, 0), look=(0, 0, 1))
    s.medium.type = P.MEDIUM_HOMOGENEOUS
    scenes.add_sphere(s, (0, 0, 0), R, kd=Kd)
    if light == "point":
        P.add_point_light(s, I, (0, 0, 0))
    else:
        P.add_spot_light(s, I, (0, 0, 0), (1, 0, 0), coneangle=90, conedelta=10)
    prm = P.app_f_params()
    prm.maxdepth = 1
    gamma5 = 5 * EPS / (1 - 5 * EPS)
    bound = 2 * (2 * math.sqrt(3) * gamma5 + 2 * EPS) + 16 * EPS
    want = np.array(Kd) / math.pi * np.array(I) / (R * R)
    ang = np.degrees(np.arccos(np.clip(pixel_corner_dirs(s)[..., 0], -1, 1)))      # to the spot's axis +x
    corners = np.stack([ang[:-1, :-1], ang[1:, :-1], ang[:-1, 1:], ang[1:, 1:]])
    lit, dark = (corners.max(axis=0) < 78), (corners.min(axis=0) > 92)
    if light == "point":
        lit, dark = np.ones((H, W), bool), np.zeros((H, W), bool)
    else:
        assert lit.sum() > 100 and dark.sum() > 100
    names = []
    for kernel in (None, "lane"):
        def go():
            r = P.Renderer(s, prm, W, H)
            r.render_wave(0, 1)
            out = r.kernel_name(), r.film()
            r.close()
            return out
        name, film = with_kernel(kernel, go)
        names.append(name)
        assert np.all(film[..., 3] == 1)
        err = np.abs(film[..., :3][lit] / want - 1).max()
        print(light, name, "relative error %.3g (bound %.3g)" % (err, bound))
        assert err <= bound
        assert np.all(film[..., :3][dark] == 0)
    assert names[0] != names[1] and names[1].startswith("k_render_wave<")


# ---- 5. a known answer, statistical: a spot in fog ---------------------------------------------------------------------------------
def fog_spot_scene(P, F):
    s = scenes.empty_scene(F.W, F.H, eye=F.eye, look=F.look, up=F.up, fov=F.fov)
    m = s.medium
    m.type = P.MEDIUM_HOMOGENEOUS
    m.sigma_a[:] = (F.sigma_a,) * 3
    m.sigma_s[:] = (F.sigma_s,) * 3
    m.g = F.g
    scenes.add_quad(s, (-6, -6, F.z_wall), (12, 0, 0), (0, 12, 0), kd=(0, 0, 0))      # the black backdrop every camera ray ends on
    P.add_spot_light(s, F.I, F.light_from, F.light_to, coneangle=F.coneangle, conedelta=F.conedelta)
    return s


def test_spot_in_fog_agrees_with_the_quadrature(gpu_pkg):
    """Single scattering by NEE alone (maxdepth 1, nothing else emits, the backdrop is black; without it a ray of infinite extent is
    not medium-sampled): the means of the four film quadrants over 32 separately cleared waves against the float64 quadrature of
    tests/pointlight_model.py::FogSpot, |z| <= 4.5 each with the standard error taken from the spread over the waves -- a probability
    condition, not a measured tolerance.  tests/test_pointlight_model.py shows on the CPU that the quadrature's own error is below a
    tenth of that standard error, that each planted error of the model moves a quadrant by more than ten of them, and that the
    camera rays keep 0.5 units away from the light."""
    P = gpu_pkg
    F = M.FogSpot()
    prm = P.app_f_params()
    prm.maxdepth = 1
    r = P.Renderer(fog_spot_scene(P, F), prm, F.W, F.H)
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


# ---- 6. the samplers share an expectation ---------------------------------------------------------------------------------------
def test_uniform_and_bvh_share_an_expectation(gpu_pkg):
    """Whole-film means of 32 separately cleared waves of the five-light scene over the 2^3 grid under "uniform" and under "bvh", by
    Welch's statistic: |z| <= 4.5."""
    P = gpu_pkg
    means = {}
    for sampler in ("uniform", "bvh"):
        s, _ = five_light_scene(P, "grid")
        r = P.Renderer(s, sampler_params(P, sampler), W, H)
        ms = []
        for w in range(32):
            r.film_clear()
            r.render_wave(w, w + 1)
            ms.append(float((r.film()[..., :3].astype(np.float64).sum(axis=2) / 3).mean()))
        r.close()
        means[sampler] = np.array(ms)
    a, b = means["uniform"], means["bvh"]
    z = (a.mean() - b.mean()) / math.sqrt(a.var(ddof=1) / len(a) + b.var(ddof=1) / len(b))
    print("uniform %.5f +- %.5f, bvh %.5f +- %.5f, z = %.3f" % (a.mean(), a.std(ddof=1) / math.sqrt(32), b.mean(), b.std(ddof=1) / math.sqrt(32), z))
    assert a.mean() > 0 and abs(z) <= 4.5, z


# ---- 7. guided ----------------------------------------------------------------------------------------------------------------------------
def test_guided_training_runs_and_kernels_agree(gpu_pkg):
    """Reference-default options on the grid scene with the spot: four training waves run, stay finite and leave a field with fitted
    regions.  The kernels are then compared as tests/test_envlight_gpu.py compares guided kernels -- with that field and that VSP
    buffer in place, wave 4 on the pipeline and on the per-lane kernel, bit for bit (two in-loop TRAINING runs on different kernels
    hand their radiance samples to the update in different orders, include/vspg.h: their films differ in the last bits with any
    light)."""
    P = gpu_pkg
    # (the grid behind its interface sphere: with these two lights alone a wave of the scene the medium fills records a few dozen
    #  radiance samples at this film size -- no sky ends the escaping rays' segments -- and Field::Update wants more than 128)
    scene = family_scene(P, "grid_boundary")
    prm = P.default_params()
    prm.guide_num_training_waves = 4
    t = P.Renderer(scene, prm, W, H)
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


# ---- 8. the scene-file route ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(gpu_pkg):
    path = os.path.join(HOST, "vspg_pbrt")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", HOST])
    return path


def test_scene_file_point_light(gpu_pkg, exe, tmp_path):
    """tests/scenes/fog_box.pbrt with a LightSource "point" under a Translate / Rotate CTM, through vspg_pbrt, against the same scene
    built with add_point_light: the films are equal bit for bit."""
    import exr_model as X
    P = gpu_pkg
    lines = open(os.path.join(ROOT, "tests", "scenes", "fog_box.pbrt")).read().splitlines()
    at = [i for i, l in enumerate(lines) if l.startswith("WorldBegin")][0]
    light = ['AttributeBegin', '  Translate 0.3 -0.2 0.5', '  Rotate 37 1 2 3',
             '  LightSource "point" "rgb I" [ 2 4 8 ] "float scale" 0.5 "float power" 10 "point3 from" [ 0.1 0.2 -0.1 ]', 'AttributeEnd']
    scene = tmp_path / "point.pbrt"
    scene.write_text("\n".join(lines[:at + 1] + light + lines[at + 1:]) + "\n")
    out = tmp_path / "point.pfm"
    a = subprocess.run([exe, str(scene), "--outfile", str(out), "--spp", "3"], capture_output=True, text=True, timeout=120)
    assert a.returncode == 0, a.stdout + a.stderr
    got = X.read_pfm(str(out))
    s = P.fog_box_scene(64, 48)
    P.add_point_light(s, (2, 4, 8), (0.1, 0.2, -0.1), scale=0.5, power=10.0, ctm=ctm_oblique())
    pos = np.array(s.point_lights[0].render_from_light[:], f32).reshape(4, 4)[:3, 3]
    assert np.all(np.abs(pos) < 1)      # inside the box
    r = P.Renderer(s, P.app_f_params(), 64, 48)
    for w in range(3):
        r.render_wave(w, w + 1)
        r.post_process_wave()
    f = r.film()
    r.close()
    want = (f[..., :3] / f[..., 3:4]).astype(f32)
    assert want.max() > 0 and np.array_equal(u32(got), u32(want))
    plain = P.Renderer(P.fog_box_scene(64, 48), P.app_f_params(), 64, 48)      # ... and the light is in it
    for w in range(3):
        plain.render_wave(w, w + 1)
        plain.post_process_wave()
    assert not np.array_equal(u32(plain.film()), u32(f))
    plain.close()
