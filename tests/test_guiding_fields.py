"""The guiding-cache query on fields the rest of the suite never builds (tests/field_models.py): trees past the 256 nodes the
workgroup kernels stage in LDS, both node numberings, a chain deeper than the descent's 64 steps, 0..8 lobes per region with NaN
in every unset slot, kappas on both sides of both clamps, degenerate distances, and the fallback / cancelling-lobes branches.

CPU side: the oracle against an independent float64 model, and the conditions that keep the GPU file's cases from being
silently empty (which branch each query takes is counted here, on the query sets the GPU tests use)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import field_models as fm
import oracle_lib
from conftest import ROOT, load_package
from test_oracle_guiding import sphere_quadrature

MARGIN = 4.0


@pytest.fixture(scope="module")
def eps_fe():
    """FastExp's relative error against exp in float64 over the arguments of tests/golden/primitives.json (normal results)."""
    G = json.load(open(os.path.join(ROOT, "tests", "golden", "primitives.json")))
    x = np.array([float.fromhex(a) for a, _ in G["fast_exp"]])
    y = np.array([float.fromhex(b) for _, b in G["fast_exp"]])
    m = np.isfinite(y) & (y >= 2.0 ** -126)
    assert m.sum() > 100
    eps = float(np.max(np.abs(y[m] / np.exp(x[m]) - 1)))
    print("FastExp relative error on %d golden arguments: %.3e" % (m.sum(), eps))
    assert 1e-5 < eps < 1e-3
    return eps


@pytest.fixture(scope="module")
def orc():
    P = load_package()
    r = oracle_lib.OracleRenderer(oracle_lib.fog_box_scene(32, 32), oracle_lib.default_params(), 32, 32)
    yield P, r
    r.close()


@pytest.fixture(scope="module")
def answers(orc, eps_fe):
    """(field name, is_volume, g) -> (queries, the oracle's answer, the model's), computed once and left unchanged"""
    P, r = orc
    cache = {}

    def get(name, is_volume, g):
        key = (name, is_volume, g)
        if key not in cache:
            f = fm.field(P, name)
            r.set_guiding_field(f, f)
            q = fm.query_set(P, name, is_volume)
            cache[key] = (q, r.guiding_query_batch(is_volume, g, *q), fm.model_query(f, is_volume, g, *q[:3], eps_fe=eps_fe))
        return cache[key]
    return get


def test_generators_are_what_they_say(pkg):
    P = pkg
    for name, n_nodes in (("kd199-creation", 199), ("kd255-creation", 255), ("kd255-dfs", 255), ("kd257-creation", 257), ("kd257-dfs", 257),
                          ("kd8191-creation", 8191), ("kd8191-dfs", 8191), ("spine", 141), ("lobe_edge", 21)):
        f = fm.field(P, name)
        nodes, R = f.np_nodes, f.np_regions
        assert len(nodes) == n_nodes == 2 * len(R) - 1
        axis, idx = nodes["packed"] & 3, (nodes["packed"] >> 2).astype(np.int64)
        inner = axis != 3
        assert (idx[inner] > np.nonzero(inner)[0]).all() and (idx[inner] + 1 < n_nodes).all()   # what upload_field requires
        assert sorted(idx[~inner]) == list(range(len(R)))                                         # every region is some leaf's
        # every float of every unset lobe slot is NaN, every set one is not
        unset = np.arange(fm.GK)[None, :] >= R["n_lobes"][:, None]
        for key in fm.LOBE_FLOATS:
            assert np.array_equal(np.isnan(R[key]), unset), (name, key)
        assert np.array_equal(np.isnan(R["mu"]), np.repeat(unset[:, None, :], 3, axis=1))
        again = fm._BUILDERS[name](P)                                                             # deterministic
        assert again.np_nodes.tobytes() == nodes.tobytes() and again.np_regions.tobytes() == R.tobytes()
    # the two numberings hold the same tree; "dfs" keeps the left spine inside the LDS stage and leaves it at depth 1 on the right
    a, b = fm.field(P, "kd8191-creation"), fm.field(P, "kd8191-dfs")
    assert a.np_regions.tobytes() == b.np_regions.tobytes() and a.np_nodes.tobytes() != b.np_nodes.tobytes()
    assert (b.np_nodes["packed"][0] >> 2) == 1 and (b.np_nodes["packed"][1] >> 2) == 3
    right = b.np_nodes[2]
    assert (right["packed"] & 3) != 3 and (right["packed"] >> 2) > fm.KD_LDS_NODES
    assert set(fm.field(P, "lobe_edge").np_regions["n_lobes"]) == {0, 1, 2, 3, 4, 5, 7, 8}
    assert sorted(fm.field(P, "spine").leaf_depth.values()) == list(range(1, 71)) + [70]


@pytest.mark.parametrize("name", sorted(fm._BUILDERS))
def test_region_index_model_equals_oracle(answers, orc, eps_fe, pkg, name):
    """`ok` from the oracle == the model's "a region was found and it has lobes", on every generator: random points, points
    exactly on the split plane of the root and of a node numbered past the LDS stage (and one float to either side), points 1e6
    outside the bounds.  The pdfs of the next test depend on WHICH region was found; here the on-plane points also pin the
    side: `c < split` goes left, everything else right."""
    P = pkg
    f = fm.field(P, name)
    deep = fm.deep_split_node(f)
    assert (deep is not None) == (len(f.np_nodes) > fm.KD_LDS_NODES + 1)
    for is_volume in (0, 1):
        (p, a, wi, u), o, m = answers(name, is_volume, 0.0)
        assert np.abs(p).max() == 1e6
        assert np.array_equal(o["ok"], m["ok"])
        assert (o["vsp"][o["ok"] == 0] == -1).all() and (o["pdf"][o["ok"] == 0] == 0).all()
    for node in [0] + ([deep] if deep is not None else []):
        on, below, above = fm._plane_points(f, node)
        child = int(f.np_nodes["packed"][node] >> 2)
        for q, side in ((on, 1), (below, 0), (above, 1)):
            region, last = fm.model_lookup(f, q[None, :])
            if last[0] >= 0:   # (spine: the root's plane lies in the deepest cell, which the 64 steps do not reach)
                lo, hi = f.cells[child + side]   # the leaf the descent ended in lies under the expected child
                assert (f.cells[last[0], 0] >= lo).all() and (f.cells[last[0], 1] <= hi).all(), (name, node, side)
            else:
                assert name == "spine"
    # the oracle itself at the three points of each plane: its incident mixture and VSP are those of the region the model
    # found (c == split goes RIGHT), within the bound of test_pdfs_oracle_vs_float64_model; `told_apart` shows that the
    # values on the two sides of a plane differ by more than that bound, so a descent that went left would not pass
    P, r = orc
    r.set_guiding_field(f, f)
    told_apart = 0
    for node in [0] + ([deep] if deep is not None else []):
        pts = np.array(fm._plane_points(f, node))                  # on, one float below, one float above
        a = np.tile(np.float32((0.6, 0.0, 0.8)), (3, 1))
        wdir = np.tile(np.float32((0.0, 0.6, 0.8)), (3, 1))
        o = r.guiding_query_batch(1, 0.0, pts, a, wdir, np.full((3, 2), 0.5, dtype=np.float32))
        m = fm.model_query(f, 1, 0.0, pts, a, wdir, eps_fe=eps_fe)
        assert np.array_equal(o["ok"], m["ok"])
        tol = {}
        for key in ("incoming_pdf", "vsp"):
            tol[key] = MARGIN * (m["rtol_" + key] * np.abs(m[key]) + m["atol_" + key])
            assert (np.abs(o[key].astype(np.float64) - m[key]) <= tol[key]).all(), (name, node, key)
        assert m["region"][0] == m["region"][2] and (m["region"][0] != m["region"][1] or m["region"][0] < 0)
        told_apart += any(abs(m[key][0] - m[key][1]) > tol[key][0] + tol[key][1] for key in tol)
    assert told_apart >= 1, name   # a condition on the (deterministic) field, computed from the model alone


@pytest.mark.parametrize("is_volume,g", fm.QUERY_CASES)
@pytest.mark.parametrize("name", fm.QUERY_FIELDS)
def test_pdfs_oracle_vs_float64_model(answers, eps_fe, name, is_volume, g):
    """pdf, incoming_pdf and vsp of the oracle (float32, FastExp) against the model (float64, exp) within a bound computed
    per query from two sources, times a margin of 4:
      eps   FastExp's relative error against exp, measured in float64 on the arguments of tests/golden/primitives.json
            (1.15e-4), once per FastExp a value went through -- and amplified by E / (1 - E), E = e^{-2 kappa}, where the vMF
            normalisation subtracts it from one (50x at kappa = 0.01);
      u     the rounding of the exponent: FastExp(k x) with x known to `few` = 8 roundings of 2^-24 (a dot product of two unit
            vectors, the normalisation of the re-aimed direction, FastExp's own x * log2 e) costs k * few * 2^-24 relatively;
            re-aiming a lobe at a point near its source and a product whose two lobes nearly cancel amplify it, by factors
            the model computes from its own numbers (field_models.model_query states each term).
    A sum of positive terms has at most the largest relative error of its terms; a quotient adds numerator's and denominator's.
    Absolute part: FastExp returns 0 below 2^-126, where exp does not.
    The bound never comes from the oracle's output.  So that it cannot quietly grow until nothing is checked: on the random
    fields (kappa <= 500) at least 99 % of the queries are held to 5 % or better and half of them to 1.5 %; only lobe_edge,
    whose kappas of 1e4 put 1e4 * 8 * 2^-24 = 0.5 % per rounding source into every exponent, is held to a looser one."""
    q, o, m = answers(name, is_volume, g)
    ok = m["ok"] == 1
    assert np.array_equal(o["ok"], m["ok"]) and ok.sum() > 20000
    for key in ("pdf", "incoming_pdf", "vsp"):
        got, ref = o[key].astype(np.float64), m[key]
        assert np.isfinite(got).all(), key
        tol = MARGIN * (m["rtol_" + key] * np.abs(ref) + m["atol_" + key])
        err = np.abs(got - ref)
        worst = np.argmax(err - tol)
        rel = MARGIN * m["rtol_" + key][ok]
        print("%s %s: largest error / bound %.3f, bound median %.2e, 99 %% %.2e" % (name, key, np.max(err[ok] / tol[ok]), np.median(rel), np.quantile(rel, 0.99)))
        assert (err <= tol).all(), (key, worst, got[worst], ref[worst], tol[worst], fm.BRANCHES[m["branch"][worst]])
        if name != "lobe_edge":
            assert np.median(rel) <= 0.015 and np.quantile(rel, 0.99) <= 0.05, key
    # what the branches mean, on the oracle's own numbers
    fb = m["branch"] == fm.BRANCHES.index("fallback")
    assert np.array_equal(o["pdf"][fb].view(np.uint32), o["incoming_pdf"][fb].view(np.uint32))   # the incident mixture stands in
    un = np.isin(m["branch"], (fm.BRANCHES.index("untrained"), fm.BRANCHES.index("outside")))
    assert (o["ok"][un] == 0).all()
    if name == "lobe_edge" and not is_volume:
        cancel = m["branch"] == fm.BRANCHES.index("cancel")
        assert cancel.sum() >= 256
        # kappa_c = 0.01 and mu . w := 0: e^{-0.01} 0.01 / (2 pi (1 - e^{-0.02})) = 1.0000 / (4 pi); FastExp's error on e^{-0.02},
        # amplified by 1 / 0.02 = 50 (and once more, unamplified, on e^{-0.01}; float32 roundings are 1e-7), times the margin
        exact = 0.01 / np.sinh(0.01)     # = 2 k e^{-k} / (1 - e^{-2k}) at k = 0.01: 1 - 1.7e-5
        assert np.all(np.abs(o["pdf"][cancel].astype(np.float64) * 4 * np.pi - exact) <= MARGIN * 50 * eps_fe)


def test_conditions_of_the_gpu_query_set(answers, pkg):
    """No case of tests/test_guiding_fields_gpu.py is empty: over the query sets it runs (QUERY_FIELDS x QUERY_CASES), each of
    the five branches -- product, fallback, cancel, untrained, outside -- is taken by at least 100 queries, every lobe count
    0..8 is hit, at least 1000 descents end in a node numbered 256 or higher, and on the random fields at most 15 % of the
    queries fail Init (one region in ten has no lobes).  The branch is the model's; that it is also the oracle's shows in
    test_pdfs_oracle_vs_float64_model (ok, and pdf == incoming_pdf bit for bit in the fallback)."""
    P = pkg
    branch = np.zeros(len(fm.BRANCHES), dtype=np.int64)
    lobes = np.zeros(fm.GK + 1, dtype=np.int64)
    deep = 0
    for name in fm.QUERY_FIELDS:
        for is_volume, g in fm.QUERY_CASES:
            q, o, m = answers(name, is_volume, g)
            branch += np.bincount(m["branch"], minlength=len(fm.BRANCHES))
            found = m["region"] >= 0
            lobes += np.bincount(m["n_lobes"][found], minlength=fm.GK + 1)
            deep += int((m["node"] >= fm.KD_LDS_NODES).sum())
            if name in fm.RANDOM_FIELDS:
                share = float(np.mean(o["ok"] == 0))
                assert share <= 0.15, (name, share)
                if len(fm.field(P, name).np_nodes) > 1000:
                    assert (m["node"] >= fm.KD_LDS_NODES).sum() >= 1000
    print("branches", dict(zip(fm.BRANCHES, branch)), "lobe counts", lobes, "descents ending past the LDS stage", deep)
    for b in ("product", "fallback", "cancel", "untrained", "outside"):
        assert branch[fm.BRANCHES.index(b)] >= 100, b
    assert (lobes > 0).all()
    assert deep >= 1000
    # the fallback block of lobe_edge: wo = +z takes it at g = -0.98 and not at g = +0.98
    f = fm.field(P, "lobe_edge")
    lo, hi = f.slab["fallback"]
    for g, want in ((-0.98, "fallback"), (0.98, "product")):
        (p, a, wi, u), o, m = answers("lobe_edge", 1, g)
        block = (p[:, 0] >= lo[0]) & (p[:, 0] < hi[0]) & (np.abs(p).max(axis=1) <= 1) & (a[:, 2] == 1)
        assert block.sum() == 256 and (m["branch"][block] == fm.BRANCHES.index(want)).all(), g
    # the on-source point: re-aiming has no direction, the lobe keeps its own
    (p, a, wi, u), o, m = answers("lobe_edge", 0, 0.0)
    at = np.all(p == f.on_source, axis=1)
    assert at.sum() == 2 and (o["ok"][at] == 1).all() and np.isfinite(o["pdf"][at]).all() and np.isfinite(o["ws"][at]).all()


# kappas the 400 x 800 midpoint quadrature of test_oracle_guiding resolves: its cells are 0.005 wide in cos(theta); a lobe
# e^{k (cos - 1)} around a pole is integrated with relative error (k h)^2 / 24, and the product lobe of these cases reaches
# k + k2 <= 40 + 3.4: (43.4 * 0.005)^2 / 24 = 2e-3, inside the 5e-3 the checks allow.  Regions with a larger clamped kappa are left out.
QUADRATURE_KAPPA = 40.0


def _resolved_regions(P):
    f = fm.field(P, "lobe_edge")
    out = []
    for k, name in enumerate(fm.EDGE_REGIONS):
        R = f.np_regions[k]
        n = int(R["n_lobes"])
        if n > 0 and np.clip(R["kappa"][:n], 1e-2, 1e4).max() <= QUADRATURE_KAPPA:
            out.append(name)
    return f, out


@pytest.mark.parametrize("is_volume,g", [(0, 0.0), (1, 0.0), (1, 0.7), (1, -0.5)])
def test_edge_field_pdfs_are_normalised_and_vsp_in_range(orc, is_volume, g):
    """test_oracle_guiding's normalisation check on lobe_edge_field: the regions below the kappa clamp, with the on-source
    lobe and with the cancelling lobe (QUADRATURE_KAPPA states which and why)."""
    P, r = orc
    f, regions = _resolved_regions(P)
    assert {"n1", "source", "cancel"} <= set(regions)
    r.set_guiding_field(f, f)
    dirs, dw = sphere_quadrature()
    n = dirs.shape[0]
    for name in regions:
        lo, hi = f.slab[name]
        points = [(lo + hi) / 2 + np.float32(0.01), lo + (hi - lo) * np.float32(0.9)] + ([f.on_source] if name == "source" else [])
        for p in points:
            for a in ((0, 1, 0), (0.6, 0, 0.8)):
                out = r.guiding_query_batch(is_volume, g, np.tile(p, (n, 1)), np.tile(a, (n, 1)), dirs, np.zeros((n, 2)))
                assert out["ok"].all()
                assert abs(out["pdf"].astype(np.float64).sum() * dw - 1) < 5e-3, (name, p, a)
                assert abs(out["incoming_pdf"].astype(np.float64).sum() * dw - 1) < 5e-3, (name, p, a)
                assert (out["vsp"] >= 0).all() and (out["vsp"] <= 1).all() and (out["pdf"] >= 0).all()


@pytest.mark.parametrize("is_volume,g", [(0, 0.0), (1, 0.6)])
@pytest.mark.parametrize("region", ["n1", "source", "cancel"])
def test_edge_field_sample_pdf_draws_from_pdf(orc, region, is_volume, g):
    """test_oracle_guiding's sample-versus-pdf check on the same regions of lobe_edge_field."""
    P, r = orc
    f, regions = _resolved_regions(P)
    assert region in regions
    r.set_guiding_field(f, f)
    rng = np.random.default_rng(1)
    n = 200000
    lo, hi = f.slab[region]
    p = lo + (hi - lo) * np.float32(0.4)
    a = np.array((0.0, 1.0, 0.0) if not is_volume else (0.3, 0.2, 0.9))
    a = a / np.linalg.norm(a)
    u = rng.random((n, 2)).astype(np.float32)
    out = r.guiding_query_batch(is_volume, g, np.tile(p, (n, 1)), np.tile(a, (n, 1)), np.tile((0, 0, 1), (n, 1)), u)
    ws = out["ws"].astype(np.float64)
    assert np.allclose(np.linalg.norm(ws, axis=1), 1, atol=1e-4)
    nb_t, nb_p = 8, 12
    dirs, dw = sphere_quadrature(400, 600)
    m = dirs.shape[0]
    qd = r.guiding_query_batch(is_volume, g, np.tile(p, (m, 1)), np.tile(a, (m, 1)), dirs, np.zeros((m, 2)))["pdf"].astype(np.float64)

    def cell(w):
        it = np.clip(((w[:, 2] + 1) / 2 * nb_t).astype(int), 0, nb_t - 1)
        ip = np.clip(((np.arctan2(w[:, 1], w[:, 0]) % (2 * np.pi)) / (2 * np.pi) * nb_p).astype(int), 0, nb_p - 1)
        return it * nb_p + ip

    expected = np.bincount(cell(dirs.astype(np.float64)), weights=qd * dw, minlength=nb_t * nb_p)
    observed = np.bincount(cell(ws), minlength=nb_t * nb_p) / n
    assert abs(expected.sum() - 1) < 5e-3
    sigma = np.sqrt(np.maximum(expected, 1e-9) / n)
    assert np.all(np.abs(observed - expected) < 5 * sigma + 2e-3 * expected + 1e-4), np.max(np.abs(observed - expected) / sigma)
    out2 = r.guiding_query_batch(is_volume, g, np.tile(p, (n, 1)), np.tile(a, (n, 1)), out["ws"], u)
    assert np.array_equal(out2["pdf"], out["pdf_s"])


def test_oracle_refuses_malformed_fields_and_keeps_its_state(pkg):
    """oracle_renderer_set_guiding_field validates both fields (tree structure, 0..8 lobes, arrays present) before it touches
    anything: a refused call leaves fields and training state as they were, whichever of the two fields was the bad one."""
    P = pkg
    lib = oracle_lib.load()
    good_s, good_v = fm.field(P, "kd199-creation"), fm.field(P, "lobe_edge")
    q = fm.query_set(P, "lobe_edge", 1, n_random=2000)
    fresh = oracle_lib.OracleRenderer(oracle_lib.fog_box_scene(32, 32), oracle_lib.default_params(), 32, 32)
    r = oracle_lib.OracleRenderer(oracle_lib.fog_box_scene(32, 32), oracle_lib.default_params(), 32, 32)
    r.set_guiding_field(good_s, good_v)
    before = [r.guiding_query_batch(iv, 0.7, *q) for iv in (0, 1)]
    assert fresh.training_stats()["training"] == 1 and r.training_stats()["training"] == 0
    for label, bad in fm.malformed_fields(P):
        for s, v in ((bad, good_v), (good_s, bad), (bad, None), (None, bad)):
            for rr, training in ((r, 0), (fresh, 1)):
                rc = lib.oracle_renderer_set_guiding_field(rr.h, C.byref(s.pod) if s else None, C.byref(v.pod) if v else None)
                assert rc == P.VSPG_EINVAL, label
                assert rr.training_stats()["training"] == training, label
    after = [r.guiding_query_batch(iv, 0.7, *q) for iv in (0, 1)]
    for b, a in zip(before, after):
        for key in b:
            assert b[key].tobytes() == a[key].tobytes(), key
    assert fresh.training_stats()["n_regions"] == [1, 1]
    r.close(); fresh.close()


@pytest.mark.parametrize("medium", fm.FALLBACK_MEDIA)
def test_replayed_paths_reach_the_fallback_in_the_path_kernels(pkg, medium):
    """The GPU file's test_fallback_branch_in_path_kernels is not empty: over the paths it replays (lobe_edge_field, medium of
    g = -0.98) the oracle's Init takes the sum == 0 fallback, and meets a cancelling product lobe, at least 100 times each."""
    P = pkg
    scene, prm, w, h, pix, si = fm.fallback_case(P, medium)
    f = fm.field(P, "lobe_edge")
    c = oracle_lib.OracleRenderer(scene, prm, w, h, seed=5)
    c.set_guiding_field(f, f)
    oracle_lib.guiding_branch_counts(reset=True)
    L, seg = c.trace_paths(pix, si)
    fallbacks, cancels = oracle_lib.guiding_branch_counts(reset=True)
    c.close()
    print(medium, "fallbacks", fallbacks, "cancelling lobes", cancels)
    assert fallbacks >= 100 and cancels >= 100 and np.isfinite(L).all()
