"""RGBGridMedium ("rgbgrid") on the device.

  1, 2  vspg_medium_point_batch and vspg_majorant_read against the float32 mirror of tests/rgbgrid_model.py, bit for bit;
  3     the equivalence to the oracle-pinned medium: an rgbgrid whose voxels are a d_i / s d_i in all channels, with a, s and the scale
        powers of two, IS the uniformgrid with those coefficients in every bit (tests/test_rgbgrid_model.py shows the precondition on the
        CPU) -- films, counters, free-flight batches and replayed paths of the two renderers agree bit for bit, on the pipeline and on
        the per-lane kernel, over every option set of OPTION_SETS;
  4     coloured grids: pipeline == per-lane kernel bit for bit over the same option sets; in-loop training;
  6     a statistical known answer against the chromatic uniformgrid (|z| <= 4.5, the project's Z_MAX);
  7     refusals on a live renderer, kernel names.
(5, the free flight of coloured grids against the float64 model of the mathematics, is tests/test_rgbgrid_free_flight.py; the scene-file
route of 7, `vspg_pbrt tests/scenes/rgb_smoke.pbrt` == the C-ABI scene, is tests/test_rgbgrid_host.py.)
Images are 24 x 16, a handful of waves."""
import ctypes as C
import os

import numpy as np
import pytest

import majorant_model
import oracle_lib
import rgbgrid_model as M
import scenes

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 24, 16
Z_MAX = 4.5   # tests/test_envlight_gpu.py, tests/test_pointlight_gpu.py, tests/test_spherelight_gpu.py
OPTION_SETS = ["resampling", "nds", "nds-emissive", "nds+", "guided", "boundary", "placed"]


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def with_kernel(kernel, fn):
    if kernel:
        os.environ["VSPG_KERNEL"] = kernel
    try:
        return fn()
    finally:
        os.environ.pop("VSPG_KERNEL", None)


def rgb_scene(P, med, base=None):
    """The fog box (or `base`) with `med` as its medium; the mirror gets the inverse matrix the scene record holds."""
    s = base if base is not None else oracle_lib.fog_box_scene(W, H)
    P.set_rgb_grid_medium(s, med.sigma_a, med.sigma_s, med.Le, p0=[float(v) for v in med.p0], p1=[float(v) for v in med.p1], g=med.g,
                          scale=float(med.scale), Lescale=float(med.Lescale))
    if med.m is not None:
        P.set_medium_transform(s, med.m)
        med.set_inverse(list(s.medium.medium_from_render))
    return s


FIXTURES = M.fixtures()


@pytest.fixture(scope="module")
def renderers(gpu_pkg):
    """One renderer per fixture, shared by the probes (read-only)."""
    P = gpu_pkg
    made = {}
    for name, med in FIXTURES.items():
        made[name] = P.Renderer(rgb_scene(P, med), P.app_f_params(), W, H)
    yield made
    for r in made.values():
        r.close()


# ---- 1, 2: the probes against the mirror ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_point_batch_equals_the_mirror(gpu_pkg, renderers, name):
    med = FIXTURES[name]
    p = M.probe_points(med)
    got = renderers[name].medium_point_batch(p)
    want = M.point_batch32(med, p)
    bad = np.argwhere(u32(got) != u32(want))
    print(name, len(p), "points,", int((want[:, 9] > 0).sum()), "inside the bounds,", int((want[:, :6] != 0).any(axis=1).sum()), "with a non-zero coefficient")
    assert bad.size == 0, (name, len(bad), "first", bad[0].tolist(), p[bad[0, 0]], got[bad[0, 0]], want[bad[0, 0]])


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_majorant_read_equals_the_mirror(gpu_pkg, renderers, name):
    got = renderers[name].majorant()
    want = M.majorant32(FIXTURES[name])
    assert got.shape == (16, 16, 16) and majorant_model.same_majorants(got, want)


# ---- 3, 4: whole paths ---------------------------------------------------------------------------------------------------------------
A, S, K = 0.25, 1.0, 2.0          # powers of two: the equivalence's precondition
LE, LESCALE = (2.0, 1.0, 0.5), 4.0
PLACE = [[1.0, 0.25, 0.0, 0.05], [0.0, 1.0, 0.0, -0.1], [0.0, -0.5, 1.0, 0.0], [0, 0, 0, 1]]   # a shear (volume-preserving), entries powers of two


def twin_density(n, seed=7):
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.2, 3.0, size=n[0] * n[1] * n[2]).astype(f32)
    d[rng.random(d.size) < 0.25] = 0
    return d


def option_setup(P, opt):
    """-> (n, build(kind) -> scene, params, field, tr): `kind` is "rgb-twin", "uniform" or "coloured"."""
    n = (9, 9, 9) if opt == "boundary" else (20, 18, 17)
    d = twin_density(n)
    emissive = opt == "nds-emissive"
    le_grid = twin_density(n, seed=8) if emissive else None
    if opt == "boundary":
        p0, p1 = (-0.8, -0.5, -0.8), (0.8, 0.9, 0.8)   # scenes.cloud_scene's bounds: inside its interface sphere
    else:
        p0, p1 = (-0.7, -0.8, -0.5), (0.8, 0.7, 0.9)

    def base():
        if opt == "boundary":
            return scenes.cloud_scene(W, H, d, n[0], sphere=True)
        return oracle_lib.fog_box_scene(W, H)

    def build(kind):
        s = base()
        if kind == "uniform":
            m = s.medium
            m.type = P.MEDIUM_GRID
            m.sigma_a[:] = (A * K,) * 3
            m.sigma_s[:] = (S * K,) * 3
            m.g = 0.5
            m.nx, m.ny, m.nz = n
            m.bounds_min[:] = p0
            m.bounds_max[:] = p1
            m.density = d.ctypes.data_as(C.POINTER(C.c_float))
            s._density_keepalive = d
            if emissive:
                m.Le[:] = LE
                m.le_scale = le_grid.ctypes.data_as(C.POINTER(C.c_float))
                m.le_nx, m.le_ny, m.le_nz = n
                s._le_keepalive = le_grid
        else:
            if kind == "rgb-twin":
                med = M.grey_twin(d, n, A, S, K, le=LE if emissive else None, le_scale=le_grid, Lescale=LESCALE, p0=p0, p1=p1, g=0.5)
            else:   # spatially varying albedo, different per channel
                med = M.RgbGrid(M.coloured(n, 51, hi=1.0), M.coloured(n, 52, hi=4.0), Le=M.coloured(n, 53, hi=0.5) if emissive else None,
                                p0=p0, p1=p1, g=0.5, scale=1.5, Lescale=2.0)
            s.medium.density = C.POINTER(C.c_float)()
            rgb_scene(P, med, base=s)
        if opt == "placed":
            P.set_medium_transform(s, PLACE)
        return s

    prm = P.default_params() if opt == "guided" else P.app_f_params()
    if opt in ("nds", "nds-emissive", "nds+"):
        prm.vspsamplingmethod = P.VSP_NDS
    tr = None
    if opt == "nds+":
        prm.collisionProbabilityBias = 1
        tr = np.random.default_rng(5).random((H, W, 3)).astype(f32) * 0.9 + 0.05
    field = scenes.light_field(P, n=4) if opt == "guided" else None
    return n, build, prm, field, tr


def tmaj_queries(P, n=257, seed=9):
    rng = np.random.default_rng(seed)
    q = []
    for i in range(n):
        o = rng.uniform(-0.95, 0.95, 3)
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        q.append(P.VspgTmajQuery(P.f3(*o), P.f3(*(d * rng.uniform(0.5, 2.0))), float(rng.uniform(0.3, 3.0)), float(rng.random()), float(rng.random()),
                                 float(rng.random()), float(rng.uniform(0.05, 0.95)) if i % 3 else -1.0, int(rng.integers(0, 3)), int(i % 5 == 0) * 2))
    return q


def run(P, scene, prm, field, tr, kernel, waves=3, seed=11):
    """film, counters, kernel name, the three free-flight batches and a replay of every pixel's sample 1."""
    def go():
        r = P.Renderer(scene, prm, W, H, seed=seed)
        if field is not None:
            r.set_guiding_field(field, field)
        if tr is not None:
            r.set_tr_buffer(tr)
        name = r.kernel_name()
        for w in range(waves):
            r.render_wave(w, w + 1)
            r.post_process_wave()
        out = dict(name=name, film=r.film(), counters=r.counters())
        q = tmaj_queries(P)
        out["tmaj"] = [b"".join(bytes(x) for x in r.sample_tmaj_batch(v, q)) for v in (P.TMAJ_PLAIN, P.TMAJ_OPTICAL_DEPTH, P.TMAJ_RESAMPLING)]
        xy = np.array([(x, y) for y in range(H) for x in range(W)], dtype=np.int32)
        out["trace"] = r.trace_paths(xy, np.ones(len(xy), dtype=np.int32))
        r.close()
        return out
    return with_kernel(kernel, go)


def assert_same_run(a, b, what):
    assert a["counters"] == b["counters"], (what, a["counters"], b["counters"])
    assert np.array_equal(u32(a["film"]), u32(b["film"])), (what, "film", int((u32(a["film"]) != u32(b["film"])).sum()))
    (La, sa), (Lb, sb) = a["trace"], b["trace"]
    assert np.array_equal(u32(La), u32(Lb)) and np.array_equal(sa, sb), (what, "trace_paths")
    if "tmaj" in a and "tmaj" in b:
        for v in range(3):
            assert a["tmaj"][v] == b["tmaj"][v], (what, "sample_tmaj_batch variant", v)


@pytest.mark.parametrize("opt", OPTION_SETS)
def test_grey_twin_equals_the_uniformgrid_bit_for_bit(gpu_pkg, opt):
    P = gpu_pkg
    n, build, prm, field, tr = option_setup(P, opt)
    rgb, uni = build("rgb-twin"), build("uniform")
    for kernel in (None, "lane"):
        a = run(P, rgb, prm, field, tr, kernel)
        b = run(P, uni, prm, field, tr, kernel)
        print(opt, kernel, a["name"], "==", b["name"], a["counters"])
        assert "RgbGridMedium" in a["name"] and "RgbGridMedium" not in b["name"]
        assert a["name"].startswith("k_render_wave<" if kernel else "k_wf_")
        assert a["film"][..., 3].min() == 3 and a["film"][..., :3].max() > 0 and a["counters"]["density_queries"] > 0
        assert_same_run(a, b, (opt, kernel))


@pytest.mark.parametrize("opt", OPTION_SETS)
def test_coloured_pipeline_equals_the_per_lane_kernel(gpu_pkg, opt):
    P = gpu_pkg
    n, build, prm, field, tr = option_setup(P, opt)
    s = build("coloured")
    a = run(P, s, prm, field, tr, None)
    b = run(P, s, prm, field, tr, "lane")
    print(opt, a["name"], "==", b["name"], a["counters"])
    assert a["name"].startswith("k_wf_") and b["name"].startswith("k_render_wave<RgbGridMedium")
    img = a["film"][..., :3] / a["film"][..., 3:4]
    assert np.isfinite(img).all() and img.max() > 0
    assert not np.array_equal(img[..., 0], img[..., 2]), "a coloured medium renders a coloured film"
    del a["tmaj"]   # (one renderer's medium either way: nothing to compare)
    assert_same_run(a, b, opt)


def test_in_loop_training_on_both_kernels(gpu_pkg):
    """Reference-default options, no field handed over: the renderer trains.  After the first wave both kernels have recorded the same
    radiance samples (compared sorted: their order is unspecified); the pipeline then trains on: finite film, one weight per wave."""
    P = gpu_pkg
    n, build, _, _, _ = option_setup(P, "resampling")
    s = build("coloured")
    prm = P.default_params()
    prm.guide_num_training_waves = 3
    stats, samples = {}, {}
    for kernel in (None, "lane"):
        def go():
            r = P.Renderer(s, prm, W, H, seed=3)
            assert "train" in r.kernel_name() and "RgbGridMedium" in r.kernel_name(), r.kernel_name()
            r.render_wave(0, 1)
            st = r.training_stats()
            sm = np.frombuffer(r.train_samples().tobytes(), dtype=np.uint32).reshape(-1, 10)
            film = None
            if kernel is None:
                r.post_process_wave()
                for w in range(1, 3):
                    r.render_wave(w, w + 1)
                    r.post_process_wave()
                film = r.film()
                assert r.training_stats()["iteration"] == 3
            r.close()
            return st, sm[np.lexsort(sm.T[::-1])], film
        stats[kernel], samples[kernel], film = with_kernel(kernel, go)
        if kernel is None:
            assert np.isfinite(film).all() and np.all(film[..., 3] == 3) and film[..., :3].max() > 0
    print("training stats after wave 0:", stats[None])
    assert stats[None] == stats["lane"] and stats[None]["n_samples"] > 100
    assert np.array_equal(samples[None], samples["lane"])


# ---- 6: a statistical known answer ---------------------------------------------------------------------------------------------------
def wave_means(r, n_waves, first=0):
    out = []
    for w in range(first, first + n_waves):
        r.film_clear()
        r.render_wave(w, w + 1)
        r.post_process_wave()
        f = r.film()
        out.append((f[..., :3] / f[..., 3:4]).reshape(-1, 3).mean(axis=0))
    return np.array(out, dtype=np.float64)


def welch(a, b):
    return (a.mean() - b.mean()) / np.sqrt(a.var(ddof=1) / len(a) + b.var(ddof=1) / len(b))


def test_proportional_channels_against_the_chromatic_uniformgrid(gpu_pkg):
    """sigma_a = (a_r, a_g, a_b) d, sigma_s likewise: the same medium as the chromatic uniformgrid with those spectra, under another
    majorant (a scalar sum of maxima against a per-channel product): the walks differ, the expectations do not.  Per-channel
    whole-film means of 32 + 32 separately cleared waves, Welch's statistic, |z| <= 4.5.  Condition: the red and the blue mean differ
    by many standard errors, so that a channel swap could not pass -- the coefficients are chosen for it on the CPU
    (tests/test_rgbgrid_model.py: albedos 0.57 against 0.98), but a standard error exists only once waves are rendered, so the
    condition itself is asserted here, on the means, before the comparison."""
    P = gpu_pkg
    n = (9, 9, 9)
    d = twin_density(n, seed=12).reshape(n[2], n[1], n[0])
    a_rgb, s_rgb = np.array(M.PROPORTIONAL_A, f32), np.array(M.PROPORTIONAL_S, f32)
    p0, p1 = (-0.7, -0.8, -0.5), (0.8, 0.7, 0.9)
    med = M.RgbGrid(d[..., None] * a_rgb, d[..., None] * s_rgb, p0=p0, p1=p1, g=0.3)
    rgb = rgb_scene(P, med)
    uni = scenes.grid_scene(np.ascontiguousarray(d.reshape(-1)), n, a_rgb, s_rgb, g=0.3, bmin=p0, bmax=p1, W=W, H=H)
    prm = P.app_f_params()
    means = {}
    for key, s in (("rgbgrid", rgb), ("uniformgrid", uni)):
        r = P.Renderer(s, prm, W, H, seed=21)
        means[key] = wave_means(r, 32, first=0 if key == "rgbgrid" else 100)
        r.close()
    zs = [welch(means["rgbgrid"][:, c], means["uniformgrid"][:, c]) for c in range(3)]
    z_rb = welch(means["rgbgrid"][:, 0], means["rgbgrid"][:, 2])
    print("means rgbgrid %s uniformgrid %s z %s; red against blue z = %.1f" % (means["rgbgrid"].mean(0), means["uniformgrid"].mean(0), np.round(zs, 2), z_rb))
    assert abs(z_rb) > 10, z_rb   # the condition
    assert all(abs(z) <= Z_MAX for z in zs), zs


# ---- 7: refusals and routes ----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_renderer_untouched(gpu_pkg):
    P = gpu_pkg
    med = FIXTURES["both-9x9x9"]
    r = P.Renderer(rgb_scene(P, med), P.app_f_params(), W, H, seed=2)
    r.render_wave(0, 1)
    film, counters = r.film(), r.counters()
    n = med.n[0] * med.n[1] * med.n[2]
    with pytest.raises(P.VspgError) as e:
        r.update_density(np.zeros(n, dtype=f32))
    assert e.value.code == P.VSPG_EINVAL
    for mode in (P.ARITH_FAST_WEIGHTS, P.ARITH_FAST):
        with pytest.raises(P.VspgError) as e:
            r.set_arithmetic(mode)
        assert e.value.code == P.VSPG_ESCOPE and "RgbGridMedium" in str(e.value)
    assert r.arithmetic() == P.ARITH_EXACT
    with pytest.raises(P.VspgError) as e:
        r.brick_info()
    assert e.value.code == P.VSPG_EINVAL
    assert r.lib.vspg_brick_read(r.h, None, None, None) == P.VSPG_EINVAL
    assert np.array_equal(u32(r.film()), u32(film)) and r.counters() == counters
    r.close()


def test_kernel_names(gpu_pkg):
    P = gpu_pkg
    med = FIXTURES["both-2x3x5"]
    s = rgb_scene(P, med)
    names = {}
    for label, prm_fn, env in [("default", P.app_f_params, None), ("wf", P.app_f_params, "wf"), ("lane", P.app_f_params, "lane"), ("wg", P.app_f_params, "wg"),
                               ("guided", P.default_params, None), ("guided-lane", P.default_params, "lane")]:
        def go():
            r = P.Renderer(s, prm_fn(), W, H)
            nm = r.kernel_name()
            r.close()
            return nm
        names[label] = with_kernel(env, go)
    prm = P.app_f_params()
    prm.vspsamplingmethod = P.VSP_NDS
    r = P.Renderer(s, prm, W, H)
    names["nds"] = r.kernel_name()
    r.close()
    print(names)
    assert names["default"] == names["wf"] == "k_wf_dist_walk<RgbGridMedium>"
    assert names["lane"] == names["wg"] == "k_render_wave<RgbGridMedium>"   # no workgroup kernel: VSPG_KERNEL=wg falls through to the per-lane kernel
    assert names["guided"] == "k_wf_walk<RgbGridMedium,guided,train>" and names["guided-lane"] == "k_render_wave<RgbGridMedium,guided,train>"
    assert names["nds"] == "k_wf_segment_vertex<RgbGridMedium>"
