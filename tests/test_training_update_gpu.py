"""Field::Update on the device, stage by stage, against tests/train_model.py.

The exchange hook (Renderer.set_exchange) is handed every intermediate sum of an update -- sample count, weight sum, the
accumulators after k_train_pos<true>, k_train_pos<false> and k_train_estep -- and may add to them, as another rank would.  So
    * what the counting sort, the lookup and RunAccumulator produce is compared with float64 sums over the samples the device
      itself recorded: counts exactly, float sums within the float32 summation bound m 2^-24 sum|x| (train_model.sum_bound),
      the only tolerance in this file;
    * everything the device computes FROM those sums -- decay, the split, the copied regions, pivots, the M-step -- must equal
      the NumPy mirror fed with the very buffers the hook handed back: nodes and regions byte for byte;
    * injected statistics steer the trees past the 512 nodes k_train_lookup stages in LDS and up to the caps.
No two independently evolved fields are ever compared.  tests/test_training_update.py validates the mirror on the CPU."""
import ctypes as C
import time

import numpy as np
import pytest

import field_models as fm
import oracle_lib
import train_model as tm

pytestmark = pytest.mark.gpu

F32 = np.float32
BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))      # the fog box


@pytest.fixture(scope="module")
def hip(gpu_pkg):
    """device <-> host copies through the HIP runtime the library itself is bound to"""
    lib = gpu_pkg.load()
    lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    lib.hipMemcpy.restype = C.c_int
    lib.hipDeviceSynchronize.restype = C.c_int
    return lib


def _fog(P, W, H):
    scene = P.fog_box_scene(W, H)
    scene.medium.g = 0.3
    return scene


def _field(P, r, vol):
    nodes, regs, nn, nr = r.get_guiding_field(vol)
    a = np.frombuffer(bytes(nodes)[:nn * C.sizeof(P.VspgKdNode)], dtype=fm.NODE_DTYPE)
    b = np.frombuffer(bytes(regs)[:nr * C.sizeof(P.VspgFieldRegion)], dtype=fm.REGION_DTYPE)
    return a, b


def leaf_injection(mirror, box=BOX, below=None):
    """Call-3 statistics that make leaves split through their cells' centres: per leaf n = 5000 samples of mean c (the centre of
    the leaf's cell, descending from `box`) and standard deviation a quarter of the cell's extent per axis.  `below`: only the
    leaves that own a region index under it."""
    add = np.zeros((tm.KEYS, tm.STAT_FLOATS), dtype=F32)
    for f, M in enumerate(mirror.f):
        for reg, lo, hi in M.leaf_cells(*box):
            if below is not None and reg >= below:
                continue
            c, sd = 0.5 * (lo + hi), 0.25 * (hi - lo)
            add[f * tm.CAP_REGIONS + reg, :7] = np.r_[5000.0, 5000.0 * c, 5000.0 * (c * c + sd * sd)]
    return lambda buf: buf + add.reshape(-1)


def _within(got, ref, m, abs_sum, what):
    err = np.abs(got.astype(np.float64) - ref)
    bound = tm.sum_bound(m, abs_sum)
    bad = ~(err <= bound)
    with np.errstate(all="ignore"):
        print("%s: largest error / bound %.4f" % (what, np.max(np.where(bound > 0, err / bound, 0.0), initial=0.0)))
    assert not bad.any(), (what, np.argwhere(bad)[:5], err[bad][:5], bound[bad][:5])


def run_update(P, lib, r, mirror, first, inject=None):
    """One post_process_wave of `r` with every stage checked against `mirror` (which is advanced by the update).  inject:
    {hook call number 1..5: f(float32 buffer) -> float32 buffer}.  Returns what the update did."""
    inject = inject or {}
    crit = int(r.params.vspcriterion)
    samples = r.train_samples()
    n = len(samples)
    st0 = r.training_stats()
    assert st0["n_samples"] == n and st0["n_dropped"] == 0
    for vol in (0, 1):
        a, b = _field(P, r, vol)
        if first:
            mirror.f[vol].set_tree(a, b)
        else:   # the state the mirror carried out of the last update
            assert a.tobytes() == mirror.f[vol].node_bytes() and b.tobytes() == mirror.f[vol].region_bytes()
    before = [(M.node_bytes(), M.region_bytes()) for M in mirror.f]
    raw, used = [], []

    def hook(ptr, nf, stream):
        assert lib.hipDeviceSynchronize() == 0
        a = np.empty(nf, dtype=F32)
        assert lib.hipMemcpy(a.ctypes.data, ptr, 4 * nf, 2) == 0
        raw.append(a)
        fn = inject.get(len(raw))
        if fn is not None:
            b = np.ascontiguousarray(fn(a.copy()), dtype=F32)
            assert b.shape == a.shape
            assert lib.hipMemcpy(ptr, b.ctypes.data, 4 * nf, 1) == 0
            a = b
        used.append(a)

    r.set_exchange(hook)
    try:
        r.post_process_wave()
    finally:
        r.set_exchange(None)
    st1 = r.training_stats()
    assert st1["n_samples"] == 0 and st1["n_zero"] == 0            # Clear()
    out = dict(n=n, samples=samples, calls=len(raw), raw=raw, used=used)

    # ---- call 1: the sample count, exactly ---------------------------------------------------------------------------------------
    assert len(raw) >= 1 and raw[0].shape == (1,) and raw[0][0] == F32(n)
    if not (float(used[0][0]) > tm.MIN_UPDATE_SAMPLES):
        assert len(raw) == 1 and st1["iteration"] == st0["iteration"]
        for vol in (0, 1):
            a, b = _field(P, r, vol)
            assert (a.tobytes(), b.tobytes()) == before[vol]
        out["updated"] = False
        return out
    assert len(raw) == 5 and st1["iteration"] == st0["iteration"] + 1
    assert raw[1].shape == (1,) and all(raw[k].shape == (tm.KEYS * tm.STAT_FLOATS,) for k in (2, 3, 4))
    # ---- call 2: the weight sum ------------------------------------------------------------------------------------------------------
    w = samples["weight"].astype(np.float64)
    _within(raw[1], np.array([w.sum()]), n, np.array([np.abs(w).sum()]), "weight sum")
    with np.errstate(all="ignore"):
        wmax = tm.WEIGHT_CLAMP * (F32(used[1][0]) / F32(used[0][0]))        # k_train_estep: 32 * (sumw[0] / sumw[1])
    out["wmax"] = wmax
    # ---- call 3: counting sort + lookup + k_train_pos<true> on the tree as it stood ------------------------------------------------
    keys3 = mirror.keys(samples)
    s, a, m = tm.bin_sums(keys3, tm.pos_terms(samples))
    acc = raw[2].reshape(tm.KEYS, tm.STAT_FLOATS)
    assert np.array_equal(acc[:, 0], m.astype(F32)) and int(m.sum()) == int((keys3 >= 0).sum())
    _within(acc[:, 1:7], s[:, 1:7], m[:, None], a[:, 1:7], "sum p, sum p^2")
    assert not acc[:, 7:].any()
    # ---- decay, +=, split: the mirror on the buffer as the hook handed it back ----------------------------------------------------
    bare = any(M.has_bare_region() for M in mirror.f)
    made = []
    for f, M in enumerate(mirror.f):
        M.decay()
        M.add_pos(tm.field_acc(used[2], f))
        made.append(M.split())
    out["made"] = made
    # ---- call 4: the second sort (only after a split) + k_train_pos<false> (only if a region lacks lobes) --------------------------
    keys4 = mirror.keys(samples) if sum(made) else keys3
    acc = raw[3].reshape(tm.KEYS, tm.STAT_FLOATS)
    if bare:
        s, a, m = tm.bin_sums(keys4, tm.pos_terms(samples)[:, :4])
        assert np.array_equal(acc[:, 0], m.astype(F32))
        _within(acc[:, 1:4], s[:, 1:4], m[:, None], a[:, 1:4], "sum p after the split")
        assert not acc[:, 4:].any()
    else:
        assert not acc.any()
    out["call4_zero"] = not raw[3].any()
    for f, M in enumerate(mirror.f):
        M.init_regions(tm.field_acc(used[3], f))
    # ---- call 5: the E-step on the regions as they stand now ---------------------------------------------------------------------------
    terms, valid = tm.estep_terms(mirror, samples, keys4, wmax)
    s, a, m = tm.bin_sums(keys4, terms)
    acc = raw[4].reshape(tm.KEYS, tm.STAT_FLOATS)
    assert not acc[:, :7].any()
    _within(acc[:, 7:], s, m[:, None], a, "E-step sums")
    lobeless = np.concatenate([np.r_[M.regions["n_lobes"] == 0] for M in mirror.f])
    assert not acc[lobeless].any()
    out.update(keys=keys4, valid=valid)
    # ---- M-step -------------------------------------------------------------------------------------------------------------------------
    for f, M in enumerate(mirror.f):
        M.mstep(tm.field_acc(used[4], f), crit)
    assert st1["n_nodes"] == [M.n_nodes for M in mirror.f] and st1["n_regions"] == [M.n_regions for M in mirror.f]
    for vol in (0, 1):
        a, b = _field(P, r, vol)
        M = mirror.f[vol]
        assert len(a) == M.n_nodes and len(b) == M.n_regions
        assert np.array_equal(a["packed"], M.nodes["packed"][:M.n_nodes]), vol
        assert a.tobytes() == M.node_bytes(), ("split planes", vol)
        if b.tobytes() != M.region_bytes():
            for name in fm.REGION_DTYPE.names:
                x, y = b[name], M.regions[name][:M.n_regions]
                same = x.view(np.uint32) == y.view(np.uint32) if x.dtype == F32 else x == y
                print("field %d %s: %d of %d differ" % (vol, name, np.count_nonzero(~same), same.size))
            raise AssertionError("field %d: regions differ from the mirror's M-step" % vol)
    out["updated"] = True
    return out


def _train(P, hip, scene, W, H, updates, crit=0, seed=1, inject_for=None, each=None):
    """`updates` waves of render + checked update; inject_for(u, mirror) -> inject dict of update u (1-based)"""
    prm = P.default_params()
    prm.vspcriterion = crit
    r = P.Renderer(scene, prm, W, H, seed=seed)
    mirror = tm.Mirror()
    outs = []
    for u in range(1, updates + 1):
        r.render_wave(u - 1, u)
        o = run_update(P, hip, r, mirror, u == 1, inject_for(u, mirror) if inject_for else None)
        assert o["updated"]
        if each:
            each(u, o, mirror)
        print("update %d: %d samples, splits %s -> regions %s" % (u, o["n"], o["made"], [M.n_regions for M in mirror.f]))
        o.pop("raw"), o.pop("used"), o.pop("samples")
        outs.append(o)
    return r, mirror, outs


# ---- 1. natural training ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("crit", [tm.VSP_CONTRIBUTION, tm.VSP_VARIANCE])
def test_natural_training_eight_updates(gpu_pkg, hip, crit):
    """Fog box g = 0.3 at 96 x 72 (about 11 500 samples a wave; on the CPU the fields split in updates 1-5 and rest from
    update 6 on): decay, halved statistics and copied regions in the later updates, both M-step criteria, and updates where no
    leaf splits -- the second sort skipped, call 4 all zero."""
    t0 = time.time()
    W, H = 96, 72
    r, mirror, outs = _train(gpu_pkg, hip, _fog(gpu_pkg, W, H), W, H, 8, crit=crit)
    assert sum(1 for o in outs if sum(o["made"]) > 0) >= 2
    quiet = [o for o in outs if sum(o["made"]) == 0]
    assert len(quiet) >= 1 and all(o["call4_zero"] for o in quiet)
    assert all(M.n_regions >= 4 for M in mirror.f)
    r.close()
    print("wall %.2f s" % (time.time() - t0))


# ---- 2. grid medium -------------------------------------------------------------------------------------------------------------------------
def test_grid_medium_three_updates(gpu_pkg, hip):
    """The 16^3 cloud of the sharded-training test at 48 x 40: samples recorded by the wavefront pipeline."""
    import scenes
    t0 = time.time()
    W, H = 48, 40
    scene = scenes.grid_scene(scenes.cloud_density(16), (16, 16, 16), (0.05, 0.08, 0.1), (3.0, 2.6, 2.2), g=0.5,
                              bmin=(-0.8, -0.8, -0.5), bmax=(0.8, 0.7, 0.9), W=W, H=H)
    r, mirror, outs = _train(gpu_pkg, hip, scene, W, H, 3, seed=3)
    assert all(o["valid"].sum() > 0.9 * o["n"] for o in outs)
    r.close()
    print("wall %.2f s" % (time.time() - t0))


# ---- 3. / 4. past the LDS stage, up to the caps -----------------------------------------------------------------------------------------------
def _spread(u, o, since):
    """from update `since` on: the real samples fall into at least 200 keys, and some 64 consecutive samples (a wavefront of
    k_train_lookup / k_train_scatter) hold more than the four keys lds_bin_add serves by ballot rounds"""
    if u < since:
        return
    keys = o["keys"]
    assert len(np.unique(keys[keys >= 0])) >= 200, u
    pad = np.concatenate([keys, np.full(-len(keys) % 64, -1)]).reshape(-1, 64)
    distinct = np.array([len(np.unique(row[row >= 0])) for row in pad])
    assert distinct.max() > 4, u
    print("update %d: %d keys in use, up to %d keys per 64 samples" % (u, len(np.unique(keys[keys >= 0])), distinct.max()))


def test_training_past_the_lds_stage_up_to_the_caps(gpu_pkg, hip):
    """Fog box at 64 x 48 (about 5 200 samples a wave), thirteen updates; at call 3 the hook adds 5 000 samples' worth of
    statistics to every leaf, so every leaf splits in every update: 1 024 regions / 2 047 nodes after update 10 (past the 512
    nodes k_train_lookup stages in LDS), 4 096 / 8 191 after update 12, and update 13 finds no room: sizes unchanged.  Then
    the device's own cap-size field, read back into the oracle, answers 20 000 queries as the device does, bit for bit."""
    P = gpu_pkg
    t0 = time.time()
    W, H = 64, 48
    sizes = {}

    def each(u, o, mirror):
        sizes[u] = [(M.n_regions, M.n_nodes) for M in mirror.f]
        _spread(u, o, 10)

    r, mirror, outs = _train(P, hip, _fog(P, W, H), W, H, 13, inject_for=lambda u, m: {3: leaf_injection(m)}, each=each)
    for u in range(1, 13):
        assert sizes[u] == [(2 ** u, 2 ** (u + 1) - 1)] * 2, (u, sizes[u])
    assert sizes[10] == [(1024, 2047)] * 2 and 2047 > tm.LDS_NODES
    assert sizes[12] == sizes[13] == [(4096, 8191)] * 2
    assert outs[12]["made"] == [0, 0] and outs[12]["call4_zero"]
    print("training wall %.2f s" % (time.time() - t0))
    # k_field_aux at cap size: the field the device fitted, queried on the device and -- read back -- by the oracle
    prm = P.default_params()
    c = oracle_lib.OracleRenderer(_fog(P, W, H), prm, W, H, seed=1)
    fields = [fm.field_from_readback(P, *r.get_guiding_field(vol)) for vol in (0, 1)]
    c.set_guiding_field(fields[0], fields[1])
    rng = np.random.default_rng(11)
    for is_volume in (0, 1):
        nq = 10000
        p = rng.uniform(-1, 1, (nq, 3)).astype(F32)
        a, wi = (rng.normal(size=(nq, 3)) for _ in range(2))
        a, wi = ((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F32) for x in (a, wi))
        u2 = rng.random((nq, 2)).astype(F32)
        og = r.guiding_query_batch(is_volume, 0.3, p, a, wi, u2)
        oc = c.guiding_query_batch(is_volume, 0.3, p, a, wi, u2)
        assert oc["ok"].mean() > 0.9
        for k in ("ok", "pdf", "incoming_pdf", "vsp", "pdf_s", "ws"):
            assert np.array_equal(og[k].view(np.uint32), oc[k].view(np.uint32)), (is_volume, k)
    r.close()
    c.close()
    print("wall %.2f s" % (time.time() - t0))


def test_partial_fit_at_the_node_cap(gpu_pkg, hip):
    """As above up to 2 048 regions (eleven updates); the twelfth injects only into the leaves that own regions below 952:
    3 000 regions, 5 999 nodes.  In the thirteenth every leaf wants to split and (8192 - 5999) / 2 = 1 096 fit: the first
    1 096 wanting leaves in node order (the mirror's sequential split), 4 096 regions and 8 191 nodes; the regions created are
    visible to the E-step, so the second sort ran."""
    P = gpu_pkg
    t0 = time.time()
    W, H = 64, 48
    sizes = {}

    def inject_for(u, m):
        return {3: leaf_injection(m, below=952 if u == 12 else None)}

    def each(u, o, mirror):
        sizes[u] = [(M.n_regions, M.n_nodes) for M in mirror.f]
        _spread(u, o, 10)

    r, mirror, outs = _train(P, hip, _fog(P, W, H), W, H, 13, inject_for=inject_for, each=each)
    assert sizes[11] == [(2048, 4095)] * 2
    assert outs[11]["made"] == [952, 952] and sizes[12] == [(3000, 5999)] * 2
    assert outs[12]["made"] == [1096, 1096] and sizes[13] == [(4096, 8191)] * 2
    keys = outs[12]["keys"]
    assert ((keys % tm.CAP_REGIONS)[keys >= 0] >= 3000).any()      # samples sorted into regions the last split created
    r.close()
    print("wall %.2f s" % (time.time() - t0))


# ---- 5. chunks of more than one iteration ------------------------------------------------------------------------------------------------
def test_sort_chunks_of_more_than_one_iteration(gpu_pkg, hip):
    """Fog box at 480 x 360: about 294 000 samples a wave, more than 256 workgroups x 1024 -- every workgroup of the counting
    sort walks its chunk in more than one iteration, the last chunk ragged."""
    t0 = time.time()
    W, H = 480, 360
    r, mirror, outs = _train(gpu_pkg, hip, _fog(gpu_pkg, W, H), W, H, 2)
    for o in outs:
        assert 256 * 1024 < o["n"] <= 300000 and o["n"] % 1024 != 0
    r.close()
    print("wall %.2f s" % (time.time() - t0))


# ---- 6. the weight clamp ---------------------------------------------------------------------------------------------------------------------
def test_estep_weight_clamp(gpu_pkg, hip):
    """Case 1's scene, one update; the hook adds 15 n to the sample count, which makes the E-step's clamp 32 * sum / (16 n):
    twice the mean weight."""
    P = gpu_pkg
    W, H = 96, 72
    r = P.Renderer(_fog(P, W, H), P.default_params(), W, H, seed=1)
    mirror = tm.Mirror()
    r.render_wave(0, 1)
    o = run_update(P, hip, r, mirror, True, {1: lambda buf: buf + F32(15) * buf})
    assert o["updated"]
    w = o["samples"]["weight"]
    assert o["used"][0][0] == F32(16 * o["n"])
    assert abs(float(o["wmax"]) / (2 * w.astype(np.float64).mean()) - 1) < 1e-3
    clamped = int((~(w < o["wmax"])).sum())
    print("%d of %d samples clamped at %.4g" % (clamped, o["n"], o["wmax"]))
    assert clamped >= 100
    r.close()


# ---- 7. few and no samples ---------------------------------------------------------------------------------------------------------------------
def test_too_few_samples_leave_the_field_alone(gpu_pkg, hip):
    """4 x 4 pixels: about 30 samples, not more than 128 -- the hook is asked once (the count), nothing is updated, the sample
    counters are cleared (all asserted in run_update)."""
    P = gpu_pkg
    W, H = 4, 4
    r = P.Renderer(_fog(P, W, H), P.default_params(), W, H, seed=1)
    mirror = tm.Mirror()
    r.render_wave(0, 1)
    o = run_update(P, hip, r, mirror, True)
    assert 0 < o["n"] <= tm.MIN_UPDATE_SAMPLES and o["calls"] == 1 and not o["updated"]
    assert r.training_stats()["iteration"] == 0
    r.close()


def test_rank_without_samples_takes_part_in_the_update(gpu_pkg, hip):
    """post_process_wave with no render before it: no samples of its own, but "the other ranks" (the hook) report 1 000 samples
    and position statistics -- the update runs on grids of one workgroup with n = 0; split, init and M-step are the mirror's,
    and no sum but the injected ones is nonzero."""
    P = gpu_pkg
    W, H = 64, 48
    r = P.Renderer(_fog(P, W, H), P.default_params(), W, H, seed=1)
    mirror = tm.Mirror()
    for u in (1, 2):
        o = run_update(P, hip, r, mirror, u == 1, {1: lambda buf: buf + F32(1000), 3: leaf_injection(mirror)})
        assert o["n"] == 0 and o["updated"] and o["calls"] == 5
        assert not any(x.any() for x in o["raw"])
        assert o["made"] == [u, u]            # every leaf: 1, then 2
    assert [M.n_regions for M in mirror.f] == [4, 4] and r.training_stats()["iteration"] == 2
    r.close()
