"""Every kernel family that reads a guiding field, on the fields of tests/field_models.py, against the oracle or against each
other, bit for bit: trees past the 256 nodes the workgroup kernels stage in LDS (both node numberings), different surface and
volume fields, 0..8 lobes with NaN in the unset slots, the degenerate branches, a chain deeper than the descent, a field the
device trained itself, and uploads the library must refuse.  tests/test_guiding_fields.py asserts on the CPU that these inputs
reach the branches they are meant for."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import field_models as fm
import oracle_lib

pytestmark = pytest.mark.gpu

W, H = 64, 48
QUERY_KEYS = ("ok", "pdf", "incoming_pdf", "vsp", "pdf_s", "ws")


def _fog(P, w=W, h=H, g=0.4):
    scene = P.fog_box_scene(w, h)
    scene.medium.g = g
    return scene


def _cloud(w, h):
    import scenes
    return scenes.grid_scene(scenes.cloud_density(16), (16, 16, 16), (0.05, 0.08, 0.1), (3.0, 2.6, 2.2), g=0.5,
                             bmin=(-0.8, -0.8, -0.5), bmax=(0.8, 0.7, 0.9), W=w, H=h)


def _paths(w, h, n=30000, seed=23):
    rng = np.random.default_rng(seed)
    pix = np.stack([rng.integers(0, w, n), rng.integers(0, h, n)], axis=1).astype(np.int32)
    return pix, rng.integers(0, 4096, n).astype(np.int32)


def _assert_queries_equal(g, c, is_volume, gg, q):
    og = g.guiding_query_batch(is_volume, gg, *q)
    oc = c.guiding_query_batch(is_volume, gg, *q)
    for k in QUERY_KEYS:
        same = np.mean(og[k].view(np.uint32) == oc[k].view(np.uint32))
        print(k, "bit-identical fraction %.5f" % same)
        assert same == 1.0, k
    return oc


def _assert_paths_equal(g, c, w=W, h=H, n=30000):
    pix, si = _paths(w, h, n)
    Lg, sg = g.trace_paths(pix, si)
    Lc, sc = c.trace_paths(pix, si)
    print("paths: same segments %.5f bit-identical %.5f" % (np.mean(sg == sc), np.mean(np.all(Lg.view(np.uint32) == Lc.view(np.uint32), axis=1))))
    assert np.array_equal(sg, sc) and np.array_equal(Lg.view(np.uint32), Lc.view(np.uint32))
    return Lc, sc


def _film(P, scene, prm, w, h, seed, surface, volume, waves=3, kernel=None, nogrey="", count_paths=True):
    if kernel:
        os.environ["VSPG_KERNEL"] = kernel
    if nogrey:
        os.environ["VSPG_NO_GREY_GUIDED"] = nogrey
    try:
        r = P.Renderer(scene, prm, w, h, seed=seed)
        r.set_guiding_field(surface, volume)
        for k in range(waves):
            r.render_wave(k, k + 1); r.post_process_wave()
        name, film, cnt = r.kernel_name(), r.film(), r.counters()
        assert not count_paths or cnt["paths"] == waves * w * h
        r.close()
    finally:
        os.environ.pop("VSPG_KERNEL", None)
        os.environ.pop("VSPG_NO_GREY_GUIDED", None)
    return name, film


@pytest.fixture(scope="module")
def pair(gpu_pkg):
    """one device renderer and one oracle renderer over the fog box; the tests upload their own fields"""
    P = gpu_pkg
    prm = P.default_params()          # the reference's defaults: surface RIS, volume MIS, secondary VSP
    g = P.Renderer(_fog(P), prm, W, H, seed=2)
    c = oracle_lib.OracleRenderer(_fog(P), prm, W, H, seed=2)
    yield P, g, c
    g.close()
    c.close()


# ---- a. the query batch -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("is_volume,gg", fm.QUERY_CASES)
@pytest.mark.parametrize("name", fm.QUERY_FIELDS)
def test_query_batch_vs_oracle(pair, name, is_volume, gg):
    """k_guiding_query == the oracle in ok, pdf, incoming_pdf, vsp, pdf_s and ws, bit for bit, over 30 000 random queries plus
    the edge list (sampler values 0 and the largest float below 1, points on split planes, points 1e6 outside, the on-source
    point, the fallback / cancelling / untrained blocks)."""
    P, g, c = pair
    t0 = time.time()
    f = fm.field(P, name)
    g.set_guiding_field(f, f)
    c.set_guiding_field(f, f)
    q = fm.query_set(P, name, is_volume)
    assert not any(np.isnan(x).any() for x in q)
    oc = _assert_queries_equal(g, c, is_volume, gg, q)
    assert np.isfinite(oc["pdf"]).all() and 0 < oc["ok"].mean() < 1
    print("wall %.2f s" % (time.time() - t0))


# ---- b. different fields per vertex kind ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("surface,volume", [("kd199-creation", "kd8191-creation"), ("kd8191-creation", "kd255-creation"),
                                            (None, "kd8191-dfs")])
def test_paths_with_different_surface_and_volume_fields_vs_oracle(pair, surface, volume):
    """trace_paths with one field for surface vertices and another for volume vertices (or none for surfaces) == the oracle,
    radiance and segment counts bit for bit; with the two fields exchanged the paths differ, so the pairing is told apart."""
    P, g, c = pair
    t0 = time.time()
    fs = fm.field(P, surface) if surface else None
    fv = fm.field(P, volume)
    g.set_guiding_field(fs, fv)
    c.set_guiding_field(fs, fv)
    L, seg = _assert_paths_equal(g, c)
    assert np.isfinite(L).all()
    g.set_guiding_field(fv, fs)
    pix, si = _paths(W, H)
    L2, seg2 = g.trace_paths(pix, si)
    assert not np.array_equal(L2.view(np.uint32), L.view(np.uint32))
    print("wall %.2f s, paths changed by the exchange: %.3f" % (time.time() - t0, np.mean(np.any(L2 != L, axis=1))))


# ---- c. workgroup kernel against per-lane kernel ----------------------------------------------------------------------------------
@pytest.mark.parametrize("surface,volume", [("kd257-creation", "kd8191-creation"), ("kd8191-dfs", "kd257-dfs"),
                                            ("kd257-dfs", "kd8191-dfs"), ("kd8191-creation", "kd257-creation")])
def test_workgroup_kernel_equals_per_lane_kernel_past_the_lds_stage(gpu_pkg, surface, volume):
    """test_guided_workgroup_kernel_equals_per_lane_kernel with trees the LDS stage holds only the first 256 nodes of -- one node
    past it (257) and the trainer's cap (8191), in either slot, in both numberings: the four kernels' films bit for bit."""
    P = gpu_pkg
    t0 = time.time()
    w, h = 320, 200
    fs, fv = fm.field(P, surface), fm.field(P, volume)
    films = dict(_film(P, _fog(P, w, h), P.default_params(), w, h, 2, fs, fv, kernel=k, nogrey=n)
                 for k, n in ((None, ""), ("wg", "1"), ("lane", ""), ("lane", "1")))
    assert sorted(films) == ["k_render_wave<HomogeneousMedium,guided>", "k_render_wave<HomogeneousMediumT<2,true>,guided>",
                             "k_render_wave_wg2<HomogeneousMedium,guided>", "k_render_wave_wg2<HomogeneousMediumT<2,true>,guided>"], sorted(films)
    a = next(iter(films.values()))
    assert np.isfinite(a).all()
    for name, f in films.items():
        assert np.array_equal(a.view(np.uint32), f.view(np.uint32)), name
    print("wall %.2f s" % (time.time() - t0))


@pytest.mark.parametrize("stype,vtype", [(1, 0), (0, 1)])  # (ris, mis) = reference defaults; (mis, ris)
def test_workgroup_vertex_on_the_edge_field_equals_per_lane_kernel(gpu_pkg, stype, vtype):
    """The workgroup kernel's guided vertex (lobes in registers, the next lobe's loads in flight) against the per-lane kernel on
    lobe_edge_field: lobe counts 0..8 with NaN behind them, both kappa clamps, distances 0 / -1 / inf and the cancelling lobes;
    g = -0.6 so that volume vertices multiply with a backward lobe.  (The sum == 0 fallback needs |g| near 1:
    test_fallback_branch_in_path_kernels.)"""
    P = gpu_pkg
    t0 = time.time()
    w, h = 192, 128
    prm = P.default_params()
    prm.surfaceguidingtype, prm.volumeguidingtype = stype, vtype
    f = fm.field(P, "lobe_edge")
    films = []
    for kernel in ("wg", "lane"):
        name, film = _film(P, _fog(P, w, h, g=-0.6), prm, w, h, 11, f, f, kernel=kernel, nogrey="1")
        assert ("_wg" in name) == (kernel == "wg"), name
        films.append(film)
    assert np.isfinite(films[0]).all()
    assert np.array_equal(films[0].view(np.uint32), films[1].view(np.uint32))
    print("wall %.2f s" % (time.time() - t0))


@pytest.mark.parametrize("medium", fm.FALLBACK_MEDIA)
def test_fallback_branch_in_path_kernels(gpu_pkg, medium):
    """The sum == 0 fallback inside the path kernels -- the workgroup vertex's own copy of it (vspg_guided_wg.h), gdist_init's in
    the per-lane kernel and in the wavefront pipeline's k_wf_vertex: lobe_edge_field under a medium of g = -0.98
    (field_models.fallback_case).  Replayed paths equal the oracle's bit for bit, and the oracle's counter shows that the replay
    took the fallback (tests/test_guiding_fields.py asserts the same count without a device); the films of the default kernel
    (workgroup for the fog, wavefront pipeline for the grid) and of the per-lane kernel are equal bit for bit, in both vertex
    flavours."""
    P = gpu_pkg
    t0 = time.time()
    scene, prm, w, h, pix, si = fm.fallback_case(P, medium)
    f = fm.field(P, "lobe_edge")
    g = P.Renderer(scene, prm, w, h, seed=5)
    c = oracle_lib.OracleRenderer(scene, prm, w, h, seed=5)
    g.set_guiding_field(f, f)
    c.set_guiding_field(f, f)
    Lg, sg = g.trace_paths(pix, si)
    oracle_lib.guiding_branch_counts(reset=True)
    Lc, sc = c.trace_paths(pix, si)
    fallbacks, cancels = oracle_lib.guiding_branch_counts(reset=True)
    g.close(); c.close()
    print("fallbacks %d cancelling lobes %d over %d replayed paths" % (fallbacks, cancels, len(si)))
    assert fallbacks >= 100 and cancels >= 100
    assert np.isfinite(Lc).all()
    assert np.array_equal(sg, sc) and np.array_equal(Lg.view(np.uint32), Lc.view(np.uint32))
    for stype, vtype in ((1, 0), (0, 1)):
        prm2 = P.default_params()
        prm2.surfaceguidingtype, prm2.volumeguidingtype = stype, vtype
        films = dict(_film(P, scene, prm2, w, h, 11, f, f, kernel=k, nogrey="1", count_paths=medium == "fog") for k in (None, "lane"))
        assert len(films) == 2 and any(("_wg" in k) if medium == "fog" else k.startswith("k_wf_") for k in films), sorted(films)
        fa, fb = films.values()
        assert np.isfinite(fa).all() and np.array_equal(fa.view(np.uint32), fb.view(np.uint32)), (stype, vtype)
    print("wall %.2f s" % (time.time() - t0))


# ---- d. the wavefront pipeline ------------------------------------------------------------------------------------------------------
def test_wavefront_pipeline_past_the_lds_stage(gpu_pkg):
    """Guided k_wf_vertex / k_wf_walk over a 16^3 grid medium with a 257-node surface field and an 8191-node volume field: the
    film equals the per-lane kernel's bit for bit, and replayed paths are the oracle's."""
    P = gpu_pkg
    t0 = time.time()
    w, h = 96, 64
    prm = P.default_params()
    fs, fv = fm.field(P, "kd257-dfs"), fm.field(P, "kd8191-creation")
    films = dict(_film(P, _cloud(w, h), prm, w, h, 12, fs, fv, waves=4, kernel=k, count_paths=False) for k in (None, "lane"))
    print(sorted(films))
    assert len(films) == 2 and any(k.startswith("k_wf_") and "guided" in k for k in films) and any(k.startswith("k_render_wave<") for k in films)
    fa, fb = films.values()
    assert np.isfinite(fa).all() and np.array_equal(fa.view(np.uint32), fb.view(np.uint32))
    g = P.Renderer(_cloud(w, h), prm, w, h, seed=12)
    c = oracle_lib.OracleRenderer(_cloud(w, h), prm, w, h, seed=12)
    g.set_guiding_field(fs, fv)
    c.set_guiding_field(fs, fv)
    _assert_paths_equal(g, c, w, h, n=10000)
    g.close(); c.close()
    print("wall %.2f s" % (time.time() - t0))


# ---- e. a chain deeper than the descent ---------------------------------------------------------------------------------------------
def test_spine_field_render_and_paths(gpu_pkg):
    """spine_field: leaves at depths 1..70, the descent gives up after 64 steps, so within a wavefront Init fails for some
    lanes and not for others.  Workgroup film == per-lane film, replayed paths == the oracle's."""
    P = gpu_pkg
    t0 = time.time()
    w, h = 192, 128
    f = fm.field(P, "spine")
    prm = P.default_params()
    films = dict(_film(P, _fog(P, w, h), prm, w, h, 7, f, f, kernel=k) for k in (None, "lane"))
    assert len(films) == 2 and any("_wg" in k for k in films), sorted(films)
    fa, fb = films.values()
    assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32))
    g = P.Renderer(_fog(P), prm, W, H, seed=7)
    c = oracle_lib.OracleRenderer(_fog(P), prm, W, H, seed=7)
    g.set_guiding_field(f, f)
    c.set_guiding_field(f, f)
    _assert_paths_equal(g, c)
    g.close(); c.close()
    print("wall %.2f s" % (time.time() - t0))


# ---- f. a device-trained field, replayed ----------------------------------------------------------------------------------------------
def test_device_trained_field_replayed_vs_oracle(gpu_pkg):
    """Real trainer output as a parity input, without depending on trainer parity: train on the device (the configuration of
    test_training_in_loop_unbiased_and_useful: 96x72, 24 updates, seed 9), read both fields back, upload them to a fresh device
    renderer and to the oracle: query batch and replayed paths bit for bit."""
    P = gpu_pkg
    t0 = time.time()
    w, h = 96, 72
    prm = P.default_params()
    prm.guide_num_training_waves = 24
    t = P.Renderer(P.fog_box_scene(w, h), prm, w, h, seed=9)
    for k in range(24):
        t.render_wave(k, k + 1); t.post_process_wave()
    st = t.training_stats()
    assert st["training"] == 0 and st["iteration"] == 24
    fields = [fm.field_from_readback(P, *t.get_guiding_field(v)) for v in (0, 1)]
    t.close()
    print("trained trees: surface %d nodes / %d regions, volume %d nodes / %d regions, lobes per region %s" % (
        len(fields[0].np_nodes), len(fields[0].np_regions), len(fields[1].np_nodes), len(fields[1].np_regions),
        sorted(set(fields[0].np_regions["n_lobes"]) | set(fields[1].np_regions["n_lobes"]))))
    for f in fields:
        assert len(f.np_regions) > 1
    g = P.Renderer(_fog(P), P.default_params(), W, H, seed=3)
    c = oracle_lib.OracleRenderer(_fog(P), P.default_params(), W, H, seed=3)
    g.set_guiding_field(*fields)
    c.set_guiding_field(*fields)
    rng = np.random.default_rng(5)
    n = 30000
    unit = lambda v: (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    q = (rng.uniform(-1, 1, (n, 3)).astype(np.float32), unit(rng.normal(size=(n, 3))), unit(rng.normal(size=(n, 3))),
         rng.random((n, 2)).astype(np.float32))
    for is_volume, gg in ((0, 0.0), (1, 0.0), (1, 0.7), (1, -0.4)):
        assert _assert_queries_equal(g, c, is_volume, gg, q)["ok"].any()
    _assert_paths_equal(g, c)
    g.close(); c.close()
    print("wall %.2f s" % (time.time() - t0))


# ---- g. upload round trip -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("surface,volume", [("lobe_edge", "kd8191-dfs"), (None, "spine")])
def test_uploaded_field_reads_back_byte_for_byte(pair, surface, volume):
    P, g, c = pair
    fs = fm.field(P, surface) if surface else None
    fv = fm.field(P, volume)
    g.set_guiding_field(fs, fv)
    for vol, f in ((0, fs), (1, fv)):
        nodes, regs, nn, nr = g.get_guiding_field(vol)
        if f is None:
            assert (nn, nr) == (0, 0)
            continue
        assert (nn, nr) == (len(f.np_nodes), len(f.np_regions))
        assert bytes(nodes)[:nn * C.sizeof(P.VspgKdNode)] == f.np_nodes.tobytes()
        assert bytes(regs)[:nr * C.sizeof(P.VspgFieldRegion)] == f.np_regions.tobytes()     # NaN slots included


# ---- h. refused uploads ---------------------------------------------------------------------------------------------------------------
def test_refused_upload_leaves_the_renderer_as_it_was(gpu_pkg):
    """vspg_renderer_set_guiding_field validates BOTH fields before it frees, clears or switches anything.  Each malformed field
    (child index <= parent, child index + 1 >= n_nodes, leaf region >= n_regions, n_lobes 9 and -1, arrays missing) is refused
    with VSPG_EINVAL as surface and as volume field; the training flag keeps its value (1 on a renderer that trains, 0 on one
    with an uploaded pair); and the film rendered after the refusals equals the film rendered before them bit for bit -- on the
    same renderer after film_clear, and on a second renderer that saw the refusals first."""
    P = gpu_pkg
    t0 = time.time()
    lib = P.load()
    w, h = 96, 72
    prm = P.default_params()
    good_s, good_v = fm.field(P, "kd199-creation"), fm.field(P, "lobe_edge")
    bad = fm.malformed_fields(P)

    def refuse_all(r, training):
        for label, b in bad:
            for s, v in ((b, good_v), (good_s, b), (b, None), (None, b)):
                rc = lib.vspg_renderer_set_guiding_field(r.h, C.byref(s.pod) if s else None, C.byref(v.pod) if v else None, C.c_void_p(0))
                assert rc == P.VSPG_EINVAL, (label, rc)
                assert r.training_stats()["training"] == training, label

    a = P.Renderer(_fog(P, w, h), prm, w, h, seed=4)
    assert a.training_stats()["training"] == 1
    refuse_all(a, 1)                        # a renderer that trains goes on training
    a.set_guiding_field(good_s, good_v)
    assert a.training_stats()["training"] == 0
    a.render_wave(0, 3)
    film_a = a.film()
    refuse_all(a, 0)
    for vol, f in ((0, good_s), (1, good_v)):   # the fields are still the good pair
        nodes, regs, nn, nr = a.get_guiding_field(vol)
        assert bytes(nodes)[:nn * 8] == f.np_nodes.tobytes() and bytes(regs)[:nr * 240] == f.np_regions.tobytes()
    a.film_clear()
    a.render_wave(0, 3)
    film_b = a.film()
    a.close()
    assert np.isfinite(film_a).all() and film_a[..., 3].min() > 0
    assert np.array_equal(film_a.view(np.uint32), film_b.view(np.uint32))
    b = P.Renderer(_fog(P, w, h), prm, w, h, seed=4)
    b.set_guiding_field(good_s, good_v)
    refuse_all(b, 0)
    b.render_wave(0, 3)
    film_c = b.film()
    b.close()
    assert np.array_equal(film_a.view(np.uint32), film_c.view(np.uint32))
    print("wall %.2f s" % (time.time() - t0))
