"""vspg_renderer_update_rgb_grids on a live renderer.  Every comparison is between a renderer created with grids A and then updated to
B, and a renderer created fresh with B: create builds its storage on the host (build_rgb_octets, build_majorant_grid_rgb), the update
on the device (k_rgb_octet_build, k_majorant_build_rgb) -- so "updated == fresh" holds the kernels to an independent statement, and both
are held to the NumPy models (tests/rgbgrid_update_model.py octets32, tests/rgbgrid_model.py majorant32 / point_batch32).

Bit patterns throughout (uint32 views): the feature has no tolerance.  The one freedom is the majorant grid's, compared as
tests/test_medium_update_gpu.py compares it: equal under ==, equal in bits wherever the fresh value is not zero (max(-0, +0) depends
on the order).  Films are 32 x 24, two waves."""
import ctypes as C
import os

import numpy as np
import pytest

import majorant_model
import oracle_lib
import rgbgrid_model as M
import rgbgrid_update_model as U
import scenes

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 32, 24
P0, P1 = (-0.8, -0.7, -0.6), (0.8, 0.9, 0.7)


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def flat(a):
    return None if a is None else np.ascontiguousarray(a, dtype=f32).reshape(-1)


def rgb_scene(P, med, base=None, w=W, h=H):
    """The fog box (or `base`) with `med` as its medium (tests/test_rgbgrid_gpu.py)."""
    s = base if base is not None else oracle_lib.fog_box_scene(w, h)
    P.set_rgb_grid_medium(s, med.sigma_a, med.sigma_s, med.Le, p0=[float(v) for v in med.p0], p1=[float(v) for v in med.p1], g=med.g,
                          scale=float(med.scale), Lescale=float(med.Lescale))
    if med.m is not None:
        P.set_medium_transform(s, med.m)
        med.set_inverse(list(s.medium.medium_from_render))
    return s


def same_majorants_as_fresh(got, ref):
    return bool(np.all((got == ref) & ((u32(got) == u32(ref)) | (ref == 0))))


def medium(n, seed, which="both", le=False, **kw):
    """special_values grids: seed + 0 sigma_a, + 1 sigma_s, + 2 Le."""
    a = U.special_values(n, seed, hi=1.0) if which in ("both", "a") else None
    s = U.special_values(n, seed + 1, hi=4.0) if which in ("both", "s") else None
    Le = U.special_values(n, seed + 2, hi=0.5) if le else None
    kw.setdefault("p0", P0); kw.setdefault("p1", P1); kw.setdefault("g", 0.3); kw.setdefault("scale", 1.5); kw.setdefault("Lescale", 2.0)
    return M.RgbGrid(a, s, Le=Le, **kw)


def update_to(r, med, a=True, s=True, le=True, conv=flat):
    r.update_rgb(sigma_a=conv(med.sigma_a) if a else None, sigma_s=conv(med.sigma_s) if s else None, Le=conv(med.Le) if le else None)


def storage(r, med):
    return (r.majorant(), r.rgb_octets(0) if med.sigma_a is not None else None, r.rgb_octets(1) if med.sigma_s is not None else None)


def assert_storage(got, ref, med, what):
    """got: the updated renderer's (majorant, octets a, octets s); ref: the fresh renderer's; med: the model's medium."""
    want_maj = M.majorant32(med)
    assert majorant_model.same_majorants(ref[0], want_maj), (what, "create's builder differs from the model")
    bad = np.argwhere(~((got[0] == ref[0]) & ((u32(got[0]) == u32(ref[0])) | (ref[0] == 0))))
    assert bad.size == 0, (what, "majorant cells (z, y, x) that differ from the fresh renderer's:", bad[:8], len(bad))
    assert majorant_model.same_majorants(got[0], want_maj), what
    for k, grid in ((1, med.sigma_a), (2, med.sigma_s)):
        if grid is None:
            assert got[k] is None and ref[k] is None
            continue
        want = U.octets32(grid, med.n)
        assert got[k].shape == want.shape == ref[k].shape, (what, got[k].shape, want.shape)
        assert np.array_equal(u32(ref[k]), u32(want)), (what, "create's image differs from the model", k)
        diff = np.argwhere(u32(got[k]) != u32(want))
        assert diff.size == 0, (what, "grid", k, len(diff), "floats differ; first (bz by bx oz oy ox corner channel)", diff[:4].tolist())


# ---- octets and majorants: updated == fresh == model -----------------------------------------------------------------------------------------
SIZES = [(7, 7, 7), (8, 8, 8), (9, 9, 9), (16, 16, 16), (1, 5, 9), (17, 33, 40)]


@pytest.mark.parametrize("which", ["both", "a", "s"])
@pytest.mark.parametrize("n", SIZES, ids=lambda n: "%dx%dx%d" % n)
def test_octets_and_majorants_updated_equal_fresh_equal_model(gpu_pkg, n, which):
    P = gpu_pkg
    A, B = medium(n, 100, which), medium(n, 200, which)
    assert not majorant_model.same_majorants(M.majorant32(A), M.majorant32(B))
    for ga, gb in ((A.sigma_a, B.sigma_a), (A.sigma_s, B.sigma_s)):
        assert ga is None or not np.array_equal(U.octets32(ga, n), U.octets32(gb, n))
    upd, fresh = (P.Renderer(rgb_scene(P, m, w=8, h=8), P.app_f_params(), 8, 8) for m in (A, B))
    assert_storage(storage(upd, A), storage(upd, A), A, "created with A")
    update_to(upd, B, le=False)
    assert_storage(storage(upd, B), storage(fresh, B), B, (n, which))
    update_to(upd, A, le=False)   # back to A, from storage that held other values
    assert_storage(storage(upd, A), storage(upd, A), A, "back to A")
    upd.close(); fresh.close()


def test_majorants_of_boxes_larger_than_the_workgroup(gpu_pkg):
    """The smallest cubic grid whose largest majorant box holds more voxels than k_majorant_build_rgb's 256 lanes, sigma_a only: the
    strided loop and both reduction levels run.  (The box grows with n / 16: 6^3 = 216 up to n = 64, 7^3 = 343 from n = 65.)"""
    P = gpu_pkg

    def widest(k):
        lo, hi = M.axis_ranges((k, k, k))[0]
        return max(h - l + 1 for l, h in zip(lo, hi))

    n1 = next(k for k in range(16, 200) if widest(k) ** 3 > 256)
    assert n1 == 65 and widest(n1) ** 3 == 343 and widest(n1 - 1) ** 3 == 216
    n = (n1, n1, n1)
    A, B = medium(n, 300, "a"), medium(n, 400, "a")
    assert not majorant_model.same_majorants(M.majorant32(A), M.majorant32(B))
    upd, fresh = (P.Renderer(rgb_scene(P, m, w=8, h=8), P.app_f_params(), 8, 8) for m in (A, B))
    update_to(upd, B, le=False)
    got, ref, want = upd.majorant(), fresh.majorant(), M.majorant32(B)
    assert majorant_model.same_majorants(ref, want) and same_majorants_as_fresh(got, ref) and majorant_model.same_majorants(got, want)
    assert np.array_equal(u32(upd.rgb_octets(0)), u32(fresh.rgb_octets(0)))
    upd.close(); fresh.close()


# ---- partial updates: a kept grid's maxima come back from its own octets ---------------------------------------------------------------------
def test_partial_updates_equal_fresh_renderers(gpu_pkg):
    P = gpu_pkg
    n = (17, 9, 12)
    A, B = medium(n, 500, le=True), medium(n, 600, le=True)
    cur = {"a": A.sigma_a, "s": A.sigma_s, "le": A.Le}
    upd = P.Renderer(rgb_scene(P, A), P.app_f_params(), W, H)
    steps = [("s",), ("a",), ("le",), ("a", "s", "le"), ("a", "s", "le")]
    sources = [B, B, B, medium(n, 700, le=True), A]
    for step, (names, src) in enumerate(zip(steps, sources)):
        new = {"a": src.sigma_a, "s": src.sigma_s, "le": src.Le}
        for k in names:
            cur[k] = new[k]
        upd.update_rgb(sigma_a=flat(new["a"]) if "a" in names else None, sigma_s=flat(new["s"]) if "s" in names else None,
                       Le=flat(new["le"]) if "le" in names else None)
        med = M.RgbGrid(cur["a"], cur["s"], Le=cur["le"], p0=P0, p1=P1, g=0.3, scale=1.5, Lescale=2.0)
        fresh = P.Renderer(rgb_scene(P, med), P.app_f_params(), W, H)
        assert_storage(storage(upd, med), storage(fresh, med), med, ("step", step, names))
        p = M.probe_points(med, n_random=600)
        got, ref, want = upd.medium_point_batch(p), fresh.medium_point_batch(p), M.point_batch32(med, p)
        assert np.array_equal(u32(got), u32(ref)) and np.array_equal(u32(got), u32(want)), ("step", step, names)
        assert want[:, 6:9].max() > 0   # the Le grid is seen
        fresh.close()
    upd.close()


def test_point_batch_after_an_update_equals_the_mirror(gpu_pkg):
    """A placed medium (a sheared, scaled frame), all three grids replaced."""
    P = gpu_pkg
    n = (20, 18, 17)
    kw = dict(p0=(-0.6, -0.5, -0.7), p1=(0.7, 0.6, 0.5), scale=1.25, m=M.PLACEMENT)
    A, B = medium(n, 800, le=True, **kw), medium(n, 900, le=True, **kw)
    r = P.Renderer(rgb_scene(P, A), P.app_f_params(), W, H)
    rgb_scene(P, B)   # (fills B's inverse matrix from the scene record)
    p = M.probe_points(B)
    before = r.medium_point_batch(p)
    update_to(r, B)
    got, want = r.medium_point_batch(p), M.point_batch32(B, p)
    bad = np.argwhere(u32(got) != u32(want))
    assert bad.size == 0, (len(bad), "first", bad[0].tolist(), p[bad[0, 0]], got[bad[0, 0]], want[bad[0, 0]])
    assert not np.array_equal(u32(before), u32(got))
    r.close()


# ---- films, counters and replayed paths: updated == fresh -------------------------------------------------------------------------------------
FN = (9, 9, 9)
PLACE = [[1.0, 0.25, 0.0, 0.05], [0.0, 1.0, 0.0, -0.1], [0.0, -0.5, 1.0, 0.0], [0, 0, 0, 1]]
FILM_CASES = ["pipeline", "lane", "nds-le", "boundary", "placed", "guided"]


def film_setup(P, case):
    """-> (build(med) -> scene, params, field, kernel)."""
    boundary = case == "boundary"
    p0, p1 = ((-0.8, -0.5, -0.8), (0.8, 0.9, 0.8)) if boundary else ((-0.7, -0.8, -0.5), (0.8, 0.7, 0.9))   # the first: inside cloud_scene's interface sphere
    kw = dict(p0=p0, p1=p1, g=0.5, scale=1.5, Lescale=2.0)

    def build(med):
        base = None
        if boundary:
            base = scenes.cloud_scene(W, H, np.zeros(FN[0] ** 3, dtype=f32), FN[0], sphere=True)
            base.medium.density = C.POINTER(C.c_float)()
        s = rgb_scene(P, med, base=base)
        if case == "placed":
            P.set_medium_transform(s, PLACE)
        return s

    prm = P.default_params() if case == "guided" else P.app_f_params()
    if case == "nds-le":
        prm.vspsamplingmethod = P.VSP_NDS
    field = scenes.light_field(P, n=4) if case == "guided" else None
    return build, kw, prm, field, ("lane" if case == "lane" else None)


def render(P, r, field=None, waves=2):
    if field is not None:
        r.set_guiding_field(field, field)
    for w in range(waves):
        r.render_wave(w, w + 1)
        r.post_process_wave()
    xy = np.array([(x, y) for y in range(H) for x in range(W)], dtype=np.int32)
    return dict(film=r.film(), counters=r.counters(), trace=r.trace_paths(xy, np.ones(len(xy), dtype=np.int32)), name=r.kernel_name())


def assert_same_run(a, b, what):
    assert a["name"] == b["name"], (what, a["name"], b["name"])
    assert a["counters"] == b["counters"], (what, a["counters"], b["counters"])
    assert np.array_equal(u32(a["film"]), u32(b["film"])), (what, "film", int((u32(a["film"]) != u32(b["film"])).sum()))
    (La, sa), (Lb, sb) = a["trace"], b["trace"]
    assert np.array_equal(u32(La), u32(Lb)) and np.array_equal(sa, sb), (what, "trace_paths")


@pytest.mark.parametrize("case", FILM_CASES)
def test_film_counters_and_paths_updated_equal_fresh(gpu_pkg, case):
    P = gpu_pkg
    build, kw, prm, field, kernel = film_setup(P, case)
    le = case == "nds-le"
    A, B = medium(FN, 1000, le=le, **kw), medium(FN, 1100, le=le, **kw)
    with pytest.MonkeyPatch.context() as mp:     # the kernel is chosen per launch: the variable stays set while rendering
        if kernel:
            mp.setenv("VSPG_KERNEL", kernel)
        else:
            mp.delenv("VSPG_KERNEL", raising=False)
        upd, fresh, old = (P.Renderer(build(m), prm, W, H, seed=11) for m in (A, B, A))
        update_to(upd, B)
        a, b, c = render(P, upd, field), render(P, fresh, field), render(P, old, field)
        for r in (upd, fresh, old):
            r.close()
    print(case, a["name"], a["counters"])
    assert "RgbGridMedium" in a["name"] and a["name"].startswith("k_render_wave<" if kernel else "k_wf_")
    assert a["film"][..., 3].min() == 2 and a["film"][..., :3].max() > 0 and a["counters"]["density_queries"] > 0
    assert_same_run(a, b, case)
    assert not np.array_equal(u32(a["film"]), u32(c["film"])), "the update mattered: the film of A is another film"


@pytest.mark.parametrize("method", ["nds", "resampling"])
def test_an_le_only_update_changes_the_film_under_nds_only(gpu_pkg, method):
    """The Le grid is read by the delta-tracking callback ("nds"); "resampling" never looks at it."""
    P = gpu_pkg
    build, kw, prm, _, _ = film_setup(P, "nds-le" if method == "nds" else "pipeline")
    A, B = medium(FN, 1000, le=True, **kw), medium(FN, 1100, le=True, **kw)
    AB = M.RgbGrid(A.sigma_a, A.sigma_s, Le=B.Le, **kw)
    upd, fresh, old = (P.Renderer(build(m), prm, W, H, seed=11) for m in (A, AB, A))
    upd.update_rgb(Le=flat(B.Le))
    a, b, c = render(P, upd), render(P, fresh), render(P, old)
    for r in (upd, fresh, old):
        r.close()
    assert_same_run(a, b, method)
    assert a["film"][..., :3].max() > 0
    assert np.array_equal(u32(a["film"]), u32(c["film"])) == (method == "resampling")


# ---- the grey power-of-two twin: the new path against the oracle-pinned one ------------------------------------------------------------------
TA, TS, TK = 0.25, 1.0, 2.0


def twin_density(n, seed):
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.2, 3.0, size=n[0] * n[1] * n[2]).astype(f32)
    d[rng.random(d.size) < 0.25] = 0
    return d


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


def test_grey_twin_updated_equals_the_updated_uniformgrid(gpu_pkg):
    """An rgbgrid with voxels a d, s d in all channels (a, s and the scale powers of two) IS the uniformgrid with those coefficients in
    every bit (tests/test_rgbgrid_gpu.py).  Both renderers are created with d_A and updated to d_B -- the rgbgrid through the new
    call, the uniformgrid through update_density, which the oracle pins: films, counters, free-flight batches agree bit for bit."""
    P = gpu_pkg
    n = (20, 18, 17)
    p0, p1 = (-0.7, -0.8, -0.5), (0.8, 0.7, 0.9)
    dA, dB = twin_density(n, 7), twin_density(n, 17)
    tA = M.grey_twin(dA, n, TA, TS, TK, p0=p0, p1=p1, g=0.5)
    tB = M.grey_twin(dB, n, TA, TS, TK, p0=p0, p1=p1, g=0.5)
    uni = scenes.grid_scene(dA, n, (TA * TK,) * 3, (TS * TK,) * 3, g=0.5, bmin=p0, bmax=p1, W=W, H=H)
    prm = P.app_f_params()
    rgb, grid = P.Renderer(rgb_scene(P, tA), prm, W, H, seed=11), P.Renderer(uni, prm, W, H, seed=11)
    update_to(rgb, tB, le=False)
    grid.update_density(dB)
    a, b = render(P, rgb), render(P, grid)
    q = tmaj_queries(P)
    for v in (P.TMAJ_PLAIN, P.TMAJ_OPTICAL_DEPTH, P.TMAJ_RESAMPLING):
        ta, tb = (b"".join(bytes(x) for x in r.sample_tmaj_batch(v, q)) for r in (rgb, grid))
        assert ta == tb, ("sample_tmaj_batch variant", v)
    # the uniformgrid's cells hold the density maxima m; the rgbgrid's k (a m + s m) = fl((a k + s k) m) for powers of two
    assert np.array_equal(rgb.majorant(), f32(TA * TK + TS * TK) * grid.majorant())
    rgb.close(); grid.close()
    assert "RgbGridMedium" in a["name"] and "RgbGridMedium" not in b["name"]
    b["name"] = a["name"]
    assert_same_run(a, b, "grey twin")
    assert a["film"][..., :3].max() > 0 and a["counters"]["density_queries"] > 0


# ---- sources: device tensors give what host arrays give ----------------------------------------------------------------------------------------
def test_device_tensors_equal_host_arrays(gpu_pkg):
    """torch tensors on the renderer's device for one, two and three grids, whole and as a view at a non-zero offset of a larger
    allocation (its pointer is no allocation base and only 4-byte aligned); the sources are only read."""
    import torch
    P = gpu_pkg
    build, kw, prm, _, _ = film_setup(P, "nds-le")
    A, B = medium(FN, 1000, le=True, **kw), medium(FN, 1100, le=True, **kw)
    dev = torch.device("cuda", 0)
    host = {"sigma_a": flat(B.sigma_a), "sigma_s": flat(B.sigma_s), "Le": flat(B.Le)}
    whole = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
    big = {k: torch.zeros(v.size + 77, dtype=torch.float32, device=dev) for k, v in host.items()}
    view = {k: big[k][13:13 + v.size] for k, v in host.items()}
    for k in host:
        view[k].copy_(whole[k])            # (on the current stream, which the update then uses)
        assert view[k].data_ptr() == big[k].data_ptr() + 52 and view[k].is_contiguous()
    for names in (("sigma_s",), ("sigma_a", "Le"), ("sigma_a", "sigma_s", "Le")):
        results = []
        for src in (host, whole, view):
            r = P.Renderer(build(A), prm, W, H, seed=5)
            r.update_rgb(**{k: src[k] for k in names})
            out = render(P, r)
            results.append((r.majorant(), r.rgb_octets(0), r.rgb_octets(1), out))
            r.close()
        m0, a0, s0, o0 = results[0]
        assert o0["film"][..., :3].max() > 0
        for m, a, s, o in results[1:]:
            assert np.array_equal(u32(m), u32(m0)) and np.array_equal(u32(a), u32(a0)) and np.array_equal(u32(s), u32(s0)), names
            assert_same_run(o, o0, names)
    for k in host:
        assert torch.equal(whole[k].cpu(), torch.from_numpy(host[k])) and torch.equal(view[k].cpu(), torch.from_numpy(host[k]))
        assert float(big[k][:13].abs().sum()) == 0 and float(big[k][13 + host[k].size:].abs().sum()) == 0
    # what the wrapper refuses on a live renderer: mixed memory kinds, another dtype, size or layout, a tensor off the device -- the grids stay
    r = P.Renderer(build(A), prm, W, H, seed=5)
    before = (r.majorant(), r.rgb_octets(0), r.rgb_octets(1))
    wa = whole["sigma_a"]
    for bad in (dict(sigma_a=wa, sigma_s=host["sigma_s"]), dict(sigma_a=host["sigma_a"], Le=whole["Le"]), dict(sigma_a=wa.double()), dict(sigma_s=wa[:-1]),
                dict(Le=big["Le"][0:2 * wa.numel():2]), dict(sigma_a=wa.cpu()), dict()):
        with pytest.raises(ValueError):
            r.update_rgb(**bad)
    after = (r.majorant(), r.rgb_octets(0), r.rgb_octets(1))
    assert all(np.array_equal(u32(x), u32(y)) for x, y in zip(before, after))
    r.close()


# ---- what an update keeps ----------------------------------------------------------------------------------------------------------------------
def field_bytes(r):
    out = []
    for volume in (0, 1):
        nodes, regs, nn, nr = r.get_guiding_field(volume)
        out.append((nn, nr, bytes(nodes), bytes(regs)))
    return out


def test_update_keeps_film_counters_fields_vsp_buffer_reference_and_error_log(gpu_pkg):
    """A guided renderer that trains in-loop, a loaded VSP buffer, a reference image and one record in the error log: film, counters,
    both guiding fields, the training state and the VSP buffer read the same bytes before and after an update, the record enqueued
    before the update is still in the log, the reference image still serves the next record -- and the update is in force."""
    P = gpu_pkg
    build, kw, _, _, _ = film_setup(P, "pipeline")
    A, B = medium(FN, 1000, le=True, **kw), medium(FN, 1100, le=True, **kw)
    prm = P.default_params()
    prm.guide_num_training_waves = 3
    r = P.Renderer(build(A), prm, W, H, seed=3)
    vsp = np.random.default_rng(4).uniform(0.1, 0.9, (H, W)).astype(f32)
    r.load_vsp_buffer(vsp)
    ref = np.random.default_rng(5).uniform(0.0, 1.0, (H, W, 3)).astype(f32)
    r.set_reference_image(ref)
    for w in range(2):
        r.render_wave(w, w + 1)
        r.post_process_wave()

    def state():
        return r.film(), r.counters(), field_bytes(r), r.vsp_buffer(), r.training_stats()

    r.film_error_enqueue(tag=41)
    f0, c0, g0, (v0, ready0), t0 = state()
    assert f0[..., :3].max() > 0 and c0["paths"] > 0 and t0["iteration"] >= 1
    update_to(r, B)
    f1, c1, g1, (v1, ready1), t1 = state()
    assert np.array_equal(u32(f0), u32(f1)) and c0 == c1 and g0 == g1 and t0 == t1
    assert ready1 == ready0 and np.array_equal(u32(v0), u32(v1))
    r.film_error_enqueue(tag=42)   # the same film against the same reference image
    log = r.film_errors()
    assert [e.tag for e in log] == [41, 42]
    assert log[0].sum_se == log[1].sum_se and log[0].sum_rse == log[1].sum_rse and log[0].n_pixels == log[1].n_pixels == W * H
    assert min(log[0].sum_se) > 0
    fresh = P.Renderer(build(B), prm, W, H, seed=3)
    assert_storage(storage(r, B), storage(fresh, B), B, "after the update")
    p = M.probe_points(B, n_random=300)
    assert np.array_equal(u32(r.medium_point_batch(p)), u32(fresh.medium_point_batch(p)))
    r.close(); fresh.close()


@pytest.mark.parametrize("kernel", [None, "lane"])
def test_samples_parked_before_the_update_end_under_the_old_values(gpu_pkg, kernel):
    """A wave rendered and NOT read before the update: the film afterwards is the film of a twin that never updated."""
    P = gpu_pkg
    build, kw, prm, _, _ = film_setup(P, "pipeline")
    A, B = medium(FN, 1000, **kw), medium(FN, 1100, **kw)
    with pytest.MonkeyPatch.context() as mp:
        if kernel:
            mp.setenv("VSPG_KERNEL", kernel)
        else:
            mp.delenv("VSPG_KERNEL", raising=False)
        r, twin = (P.Renderer(build(A), prm, W, H, seed=3) for _ in range(2))
        for g in (r, twin):
            g.render_wave(0, 1)
        update_to(r, B, le=False)
        assert np.array_equal(u32(r.film()), u32(twin.film())) and r.counters() == twin.counters()
        assert twin.film()[..., :3].max() > 0
        r.close(); twin.close()


# ---- refusals leave the renderer as it was -------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(gpu_pkg):
    import torch
    P = gpu_pkg
    lib = P.load()
    build, kw, prm, _, _ = film_setup(P, "nds-le")      # "nds": the film sees the Le grid
    A, B = medium(FN, 1000, le=True, **kw), medium(FN, 1100, le=True, **kw)
    n3 = 3 * FN[0] * FN[1] * FN[2]
    r, twin = (P.Renderer(build(A), prm, W, H, seed=3) for _ in range(2))
    for g in (r, twin):
        g.render_wave(0, 1)               # (not read: whatever the launch parked stays parked through the refusals)
    before = storage(twin, A)
    a, s, le = (flat(g) for g in (B.sigma_a, B.sigma_s, B.Le))
    ap, sp_, lp = a.ctypes.data, s.ctypes.data, le.ctypes.data
    refused = [("null renderer", (None, ap, sp_, lp, n3, P.MEM_HOST, None)),
               ("nothing given", (r.h, None, None, None, n3, P.MEM_HOST, None)),
               ("nothing given", (r.h, None, None, None, n3, P.MEM_DEVICE, None)),
               ("n_floats", (r.h, ap, sp_, lp, n3 - 1, P.MEM_HOST, None)),
               ("n_floats", (r.h, ap, None, None, n3 + 1, P.MEM_HOST, None)),
               ("n_floats", (r.h, None, sp_, None, n3 // 3, P.MEM_HOST, None)),
               ("n_floats", (r.h, None, None, lp, 0, P.MEM_HOST, None)),
               ("memory", (r.h, ap, sp_, lp, n3, 2, None)),
               ("memory", (r.h, ap, None, None, n3, -1, None))]
    for what, args in refused:
        assert lib.vspg_renderer_update_rgb_grids(*args) == P.VSPG_EINVAL, what
        assert lib.vspg_last_error(), what
    # a value that is negative or not finite, in each grid, from host and from device memory; -0.0 is a legal value (checked below)
    dev = torch.device("cuda", 0)
    names = ("sigma_a", "sigma_s", "Le")
    for slot, good in enumerate((a, s, le)):
        for spoil, at in ((-1e-30, 0), (np.nan, good.size // 2 + 1), (np.inf, good.size - 1)):
            bad = good.copy()
            bad[at] = spoil
            for conv in (lambda v: v, lambda v: torch.from_numpy(v).to(dev)):
                args = [conv(a), conv(s), conv(le)]
                args[slot] = conv(bad)
                with pytest.raises(P.VspgError) as e:
                    r.update_rgb(*args)
                assert e.value.code == P.VSPG_EINVAL and '"%s"' % names[slot] in str(e.value) and "negative or not finite" in str(e.value)
                only = [None, None, None]
                only[slot] = conv(bad)
                with pytest.raises(P.VspgError) as e:
                    r.update_rgb(*only)
                assert e.value.code == P.VSPG_EINVAL and '"%s"' % names[slot] in str(e.value)
    # the read-back's own refusals
    out = np.empty(before[1].size + 1, dtype=f32)
    fp = out.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.vspg_rgb_octets_read(r.h, 2, fp, before[1].size, None) == P.VSPG_EINVAL
    assert lib.vspg_rgb_octets_read(r.h, -1, fp, before[1].size, None) == P.VSPG_EINVAL
    assert lib.vspg_rgb_octets_read(r.h, 0, fp, before[1].size + 1, None) == P.VSPG_EINVAL
    assert lib.vspg_rgb_octets_read(r.h, 0, None, before[1].size, None) == P.VSPG_EINVAL
    # the other update still refuses this medium
    with pytest.raises(P.VspgError) as e:
        r.update_density(np.zeros(n3 // 3, dtype=f32))
    assert e.value.code == P.VSPG_EINVAL
    # majorants, octets; Le, film and counters through the next render: the render without the refused calls
    after = storage(r, A)
    assert all(np.array_equal(u32(x), u32(y)) for x, y in zip(before, after))
    for g in (r, twin):
        g.post_process_wave()
        g.render_wave(1, 2)
    assert np.array_equal(u32(r.film()), u32(twin.film())) and r.counters() == twin.counters()
    assert twin.film()[..., :3].max() > 0
    # ... and the next valid update still works; -0.0 voxels are accepted, from both memory kinds
    z = a.copy()
    z[::7] = -0.0
    fresh = P.Renderer(build(B), prm, W, H, seed=3)
    r.update_rgb(z, s, le)
    r.update_rgb(torch.from_numpy(z).to(dev))
    update_to(r, B)
    assert_storage(storage(r, B), storage(fresh, B), B, "after the refusals")
    r.close(); twin.close(); fresh.close()


def test_a_grid_absent_at_create_is_refused(gpu_pkg):
    P = gpu_pkg
    lib = P.load()
    n = (9, 9, 9)
    n3 = 3 * 9 ** 3
    v = flat(U.special_values(n, 1))
    for which, absent in (("a", ("sigma_s", "Le")), ("s", ("sigma_a", "Le")), ("both", ("Le",))):
        med = medium(n, 100, which)
        r = P.Renderer(rgb_scene(P, med, w=8, h=8), P.app_f_params(), 8, 8)
        before = storage(r, med)
        for name in absent:
            with pytest.raises(P.VspgError) as e:
                r.update_rgb(**{name: v})
            assert e.value.code == P.VSPG_EINVAL and '"%s"' % name in str(e.value) and "created without" in str(e.value)
            given = {"sigma_a": v, "sigma_s": v, "Le": v}    # ... also next to grids the renderer has
            with pytest.raises(P.VspgError):
                r.update_rgb(**given)
        out = np.empty(512 * 32 * 8, dtype=f32)
        miss = 1 if which == "a" else 0
        if which != "both":
            assert lib.vspg_rgb_octets_read(r.h, miss, out.ctypes.data_as(C.POINTER(C.c_float)), out.size, None) == P.VSPG_EINVAL
        after = storage(r, med)
        assert all(x is None and y is None or np.array_equal(u32(x), u32(y)) for x, y in zip(before, after))
        r.close()


def test_other_media_refuse_both_calls(gpu_pkg):
    P = gpu_pkg
    lib = P.load()
    d = np.full(27, 0.5, dtype=f32)
    v = np.zeros(81, dtype=f32)
    out = np.zeros(512 * 32, dtype=f32)
    for scene in (P.fog_box_scene(16, 16), scenes.grid_scene(d, (3, 3, 3), 0.1, 1.0, W=16, H=16)):
        r = P.Renderer(scene, P.app_f_params(), 16, 16)
        for mem in (P.MEM_HOST, P.MEM_DEVICE):
            assert lib.vspg_renderer_update_rgb_grids(r.h, v.ctypes.data, None, None, v.size, mem, None) == P.VSPG_EINVAL
            assert b"RGB grid medium" in lib.vspg_last_error()
        assert lib.vspg_rgb_octets_read(r.h, 0, out.ctypes.data_as(C.POINTER(C.c_float)), out.size, None) == P.VSPG_EINVAL
        assert b"RGB grid medium" in lib.vspg_last_error()
        r.render_wave(0, 1)
        assert r.film()[..., :3].max() > 0
        r.close()
