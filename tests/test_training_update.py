"""The NumPy mirror of one guiding-field update (tests/train_model.py) validated without a device: against the oracle's
Field::Update bit for bit over six updates, on known answers of the split rule, and the float32 summation bound every
tolerance of tests/test_training_update_gpu.py is made of."""
import numpy as np
import pytest

import field_models as fm
import oracle_lib
import train_model as tm

F32 = np.float32


def oracle_field(c, vol):
    import ctypes as C
    nodes, regs, nn, nr = c.get_guiding_field(vol)
    a = np.frombuffer(bytes(nodes)[:nn * C.sizeof(c.P.VspgKdNode)], dtype=fm.NODE_DTYPE)
    b = np.frombuffer(bytes(regs)[:nr * C.sizeof(c.P.VspgFieldRegion)], dtype=fm.REGION_DTYPE)
    return a, b


def oracle_style_update(mirror, samples, vspcriterion):
    """one update of the mirror on sums taken as field_update_one takes them: sequential doubles in sample order, cast to float"""
    zeros = np.zeros(len(samples), dtype=np.int64)
    sw = np.bincount(zeros, weights=samples["weight"].astype(np.float64))[0]
    wmax = tm.WEIGHT_CLAMP * F32(sw / float(len(samples)))
    made = 0
    for M in mirror.f:
        M.decay()
    s3, _, _ = tm.bin_sums(mirror.keys(samples), tm.pos_terms(samples, squares=np.float64))
    for f, M in enumerate(mirror.f):
        acc3 = np.zeros((tm.CAP_REGIONS, tm.STAT_FLOATS), dtype=F32)
        acc3[:, :7] = s3[f * tm.CAP_REGIONS:(f + 1) * tm.CAP_REGIONS].astype(F32)
        M.add_pos(acc3)
        made += M.split()
    keys = mirror.keys(samples)
    s4, _, _ = tm.bin_sums(keys, tm.pos_terms(samples)[:, :4])
    for f, M in enumerate(mirror.f):
        M.init_regions(s4[f * tm.CAP_REGIONS:(f + 1) * tm.CAP_REGIONS])     # doubles: the oracle divides before it rounds
    terms, _ = tm.estep_terms(mirror, samples, keys, wmax)
    s5, _, _ = tm.bin_sums(keys, terms)
    for f, M in enumerate(mirror.f):
        acc5 = np.zeros((tm.CAP_REGIONS, tm.STAT_FLOATS), dtype=F32)
        acc5[:, 7:] = s5[f * tm.CAP_REGIONS:(f + 1) * tm.CAP_REGIONS].astype(F32)
        M.mstep(acc5, vspcriterion)
    return made


@pytest.mark.parametrize("vspcriterion", [tm.VSP_CONTRIBUTION, tm.VSP_VARIANCE])
def test_mirror_equals_oracle_bit_for_bit_over_six_updates(vspcriterion):
    """Fog box, g = 0.3, 128 x 96 (about 20 000 samples a wave): in six updates the surface field grows to 12 regions and the
    volume field to 14, three full split levels each.  After every update nodes and regions of both fields are the oracle's,
    byte for byte -- decay, halved statistics, copied regions, pivots, both M-step criteria."""
    W, H = 128, 96
    scene = oracle_lib.fog_box_scene(W, H)
    scene.medium.g = 0.3
    prm = oracle_lib.default_params()
    prm.vspcriterion = vspcriterion
    c = oracle_lib.OracleRenderer(scene, prm, W, H, seed=1)
    mirror = tm.Mirror()
    levels = [0, 0]
    for u in range(6):
        c.render_wave(u, u + 1)
        samples = c.train_samples()
        assert len(samples) > tm.MIN_UPDATE_SAMPLES
        for vol in (0, 1):     # the oracle allocates its one-node trees at the first sample
            a, b = oracle_field(c, vol)
            assert a.tobytes() == mirror.f[vol].node_bytes() and b.tobytes() == mirror.f[vol].region_bytes()
        before = [M.n_regions for M in mirror.f]
        oracle_style_update(mirror, samples, vspcriterion)
        c.post_process_wave()
        for vol in (0, 1):
            a, b = oracle_field(c, vol)
            assert len(a) == mirror.f[vol].n_nodes and len(b) == mirror.f[vol].n_regions, (u, vol)
            assert a.tobytes() == mirror.f[vol].node_bytes(), (u, vol)
            assert b.tobytes() == mirror.f[vol].region_bytes(), (u, vol)
            levels[vol] += mirror.f[vol].n_regions > before[vol]
    for vol in (0, 1):
        assert levels[vol] >= 3 and mirror.f[vol].n_regions >= 8, (levels, mirror.f[vol].n_regions)
        assert (mirror.f[vol].regions["n_lobes"][:mirror.f[vol].n_regions] == fm.GK).all()
    c.close()


# ---- split(): known answers -------------------------------------------------------------------------------------------------------------
def one_leaf(n, mean, var, depth=0):
    """a one-node field whose region holds n samples of the given mean and variance per axis"""
    M = tm.FieldMirror()
    mean, var = np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)
    M.stats[0, 0] = n
    M.stats[0, 1:4] = n * mean
    M.stats[0, 4:7] = n * (var + mean * mean)
    M.depth[0] = depth
    return M


@pytest.mark.parametrize("var,axis", [((1, 1, 1), 0), ((1, 2, 2), 1), ((2, 1, 2), 0), ((1, 1, 2), 2), ((1, 2, 1), 1), ((2, 2, 1), 0),
                                      ((0, 0, 1), 2), ((0, 1, 0), 1)])
def test_split_axis_tie_order(var, axis):
    """largest variance; among equals x before y before z (values exact in float32: mean 0)"""
    M = one_leaf(8192, (0, 0, 0), var)
    assert M.split() == 1
    assert (M.n_nodes, M.n_regions) == (3, 2)
    assert int(M.nodes["packed"][0]) == (1 << 2) | axis and M.nodes["split"][0] == 0
    assert [int(x) for x in M.nodes["packed"][1:3]] == [(0 << 2) | 3, (1 << 2) | 3]
    assert M.stats[0, 0] == M.stats[1, 0] == 4096 and M.depth[0] == M.depth[1] == 1


def test_split_plane_is_the_mean_and_children_inherit():
    M = one_leaf(5000, (0.5, -0.25, 0.125), (0.5, 1, 0.25))
    M.regions["n_lobes"][0] = 8
    M.regions["kappa"][0] = 7
    M.stats[0, 7:] = 3
    assert M.split() == 1
    assert int(M.nodes["packed"][0]) & 3 == 1 and M.nodes["split"][0] == F32(-0.25)
    assert M.regions[1].tobytes() == M.regions[0].tobytes()
    assert np.array_equal(M.stats[0], M.stats[1]) and (M.stats[0, 7:] == 1.5).all() and M.stats[0, 0] == 2500


@pytest.mark.parametrize("n,var,depth", [(4096, (1, 1, 1), 0),       # n == 4096: not MORE than the split count
                                         (8192, (0, 0, 0), 0),       # no extent
                                         (8192, (1, 1, 1), 24),      # at the depth limit
                                         (float("nan"), (1, 1, 1), 0)])
def test_split_refusals(n, var, depth):
    M = one_leaf(n, (0, 0, 0), var, depth)
    before = M.stats.copy()
    assert M.split() == 0 and (M.n_nodes, M.n_regions) == (1, 1)
    assert np.array_equal(M.stats, before, equal_nan=True)
    if depth == 24:
        M.depth[0] = 23
        assert M.split() == 1


def chain_field(n_regions):
    """a right-leaning chain: node 2i is internal with children 2i+1 (leaf -> region i) and 2i+2; every leaf wants to split"""
    M = tm.FieldMirror()
    n_nodes = 2 * n_regions - 1
    for i in range(n_regions - 1):
        M.nodes[2 * i] = (1.0 + i, ((2 * i + 1) << 2) | 0)
        M.nodes[2 * i + 1] = (0.0, (i << 2) | 3)
    M.nodes[n_nodes - 1] = (0.0, ((n_regions - 1) << 2) | 3)
    M.n_nodes, M.n_regions = n_nodes, n_regions
    M.stats[:n_regions, 0] = 8192
    M.stats[:n_regions, 4] = 8192          # variance 1 along x, mean 0
    return M


def test_split_partial_fit_is_cut_in_node_order():
    """3000 regions, 5999 nodes, every leaf wanting: (8192 - 5999) / 2 = 1096 splits fit (the region cap would allow 1097), and
    they are the FIRST 1096 wanting leaves in node order"""
    M = chain_field(3000)
    leaves = [nd for nd in range(M.n_nodes) if int(M.nodes["packed"][nd]) & 3 == 3]
    assert M.split() == 1096
    assert (M.n_nodes, M.n_regions) == (8191, 4096)
    for j, nd in enumerate(leaves):
        packed = int(M.nodes["packed"][nd])
        if j < 1096:
            assert packed == ((5999 + 2 * j) << 2) | 0, j            # internal now, children in creation order
            assert int(M.nodes["packed"][5999 + 2 * j + 1]) == ((3000 + j) << 2) | 3
        else:
            assert packed & 3 == 3 and M.stats[packed >> 2, 0] == 8192   # untouched
    # full tree: nothing fits any more, though every leaf still wants to
    M.stats[:M.n_regions, 0] = 8192
    M.stats[:M.n_regions, 4] = 8192
    before = M.node_bytes()
    assert M.split() == 0 and M.node_bytes() == before and (M.n_nodes, M.n_regions) == (8191, 4096)


def test_region_cap_binds_when_nodes_are_left():
    """4096 regions in a tree with room for nodes cannot occur by splitting (nodes = 2 regions - 1), but the rule is stated
    for both caps: 4097 regions stop the split"""
    M = chain_field(4)
    M.n_regions = tm.CAP_REGIONS
    assert M.split() == 0


# ---- the summation bound ----------------------------------------------------------------------------------------------------------------
def test_summation_bound_on_shuffled_float32_sums():
    """|float32 sum in any order - float64 sum| <= m 2^-24 sum |x_i|: checked on the E-step terms of recorded bins (one update
    of the fog box: a one-region bin of some 9 000 samples, both signs in the R columns) summed in float32 sequentially, in
    shuffled orders, pairwise and by wavefront-sized partial sums."""
    W, H = 96, 72
    scene = oracle_lib.fog_box_scene(W, H)
    scene.medium.g = 0.3
    c = oracle_lib.OracleRenderer(scene, oracle_lib.default_params(), W, H, seed=1)
    c.render_wave(0, 1)
    samples = c.train_samples()
    c.close()
    mirror = tm.Mirror()
    oracle_style_update(mirror, samples[:4000], tm.VSP_CONTRIBUTION)     # lobes to take responsibilities of
    keys = mirror.keys(samples)
    terms, valid = tm.estep_terms(mirror, samples, keys, F32(1e30))
    assert valid.sum() > 0.9 * len(samples)
    s, a, m = tm.bin_sums(keys, terms)
    rng = np.random.default_rng(5)
    worst = 0.0
    for key in np.nonzero(m)[0]:
        x = terms[keys == key]
        assert len(x) == m[key]
        bound = tm.sum_bound(m[key], a[key])
        orders = [np.arange(len(x)), np.arange(len(x))[::-1]] + [rng.permutation(len(x)) for _ in range(6)]
        for o in orders:
            y = x[o]
            seq = np.zeros(x.shape[1], dtype=F32)
            for row in y:
                seq = seq + row
            pad = np.concatenate([y, np.zeros((-len(y) % 64, x.shape[1]), dtype=F32)])
            waves = pad.reshape(-1, 64, x.shape[1]).sum(axis=1, dtype=F32)       # NumPy: pairwise within a group
            grouped = np.zeros(x.shape[1], dtype=F32)
            for row in waves:
                grouped = grouped + row
            for got in (seq, grouped):
                err = np.abs(got.astype(np.float64) - s[key])
                assert (err <= bound).all()
                worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
    print("largest error / bound: %.4f over %d bins" % (worst, np.count_nonzero(m)))
    assert 0 < worst <= 1
