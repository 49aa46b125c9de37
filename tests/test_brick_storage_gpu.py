"""The octet-brick storage of grid media on the device, both layouts: what the builder kernels wrote (read back through
vspg_brick_info / vspg_brick_read) against the NumPy model of tests/brick_model.py, and what every kernel family reads from it --
the indexed (sparse) layout, the dense layout and the oracle, which reads the raw density array and knows nothing of bricks.

Every comparison is of bit patterns: this feature has no tolerance.  Where a film is compared with the oracle's, one sample per
pixel is compared bit for bit (the oracle's film adds in double, the device's in float: one addition is the same number in both)
and several waves under the relMSE bound of test_gpu_parity.py::test_grid_paths_and_film_vs_oracle.

The layout is forced with VSPG_DENSE_BRICKS=0|1, which vspg_renderer_create reads; it is set around the constructor only."""
import ctypes as C
import os
import resource
import time

import numpy as np
import pytest

import brick_model as bm
import oracle_lib
import scenes

pytestmark = pytest.mark.gpu

N = (40, 33, 47)                                  # bricks 6 x 5 x 6
BMIN, BMAX = (-0.8, -0.8, -0.5), (0.8, 0.7, 0.9)  # non-cubic bounds
NVDB_IMIN = (-2, 1, 0)
LAYOUTS = ("indexed", "dense")


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def create(P, layout, scene, prm, W, H, seed=0):
    """P.Renderer under a forced layout ("indexed" / "dense") or the automatic choice (None)."""
    with pytest.MonkeyPatch.context() as mp:
        if layout is None:
            mp.delenv("VSPG_DENSE_BRICKS", raising=False)
        else:
            mp.setenv("VSPG_DENSE_BRICKS", "0" if layout == "indexed" else "1")
        r = P.Renderer(scene, prm, W, H, seed=seed)
    assert r.brick_info()["indexed"] == (layout == "indexed") or layout is None
    return r


# ---------------------------------------------------------------------------------------------
# the builder (k_brick_flags, the slot numbering, k_brick_fill) against the model, exhaustively
# ---------------------------------------------------------------------------------------------
def check_storage(P, dens, n, what=""):
    """Both layouts of `dens`: counts, the whole index and all 512 x 8 values of every stored brick equal the model's.
    Returns the number of bricks the indexed layout stores."""
    dens = np.ascontiguousarray(dens, dtype=np.float32).reshape(-1)
    scene = scenes.grid_scene(dens, n, 0.1, 1.0, W=8, H=8)
    keep = bm.flags(dens, n)
    bnx, bny, bnz = bm.brick_counts(n)
    nb = bnx * bny * bnz
    for layout in LAYOUTS:
        r = create(P, layout, scene, P.app_f_params(), 8, 8)
        info = r.brick_info()
        index, octs = r.brick_storage()
        r.close()
        want_index, want_octs = bm.storage(dens, n, layout == "indexed")
        n_stored = int(keep.sum()) if layout == "indexed" else nb
        assert (info["bnx"], info["bny"], info["bnz"]) == (bnx, bny, bnz), (what, layout, info)
        assert info["n_stored"] == n_stored == octs.shape[0], (what, layout, info)
        assert info["index_bytes"] == (4 * nb if layout == "indexed" else 0) and info["octet_bytes"] == max(n_stored, 1) * 512 * 32
        assert np.array_equal(index, want_index), (what, layout)
        if layout == "indexed":
            assert np.array_equal(index < 0, ~keep)
        else:
            assert np.array_equal(index.reshape(-1), np.arange(nb))
        bad = np.flatnonzero((u32(octs) != u32(want_octs)).reshape(n_stored, 8 * 8 * 8 * 8).any(axis=1))
        assert bad.size == 0, (what, layout, "stored bricks that differ from the model:", bad[:8])
        if layout == "dense":   # the bricks the model calls empty are stored as all-zero bits (a -0.0f there keeps its sign: raw copy)
            empty = octs[np.flatnonzero(~keep.reshape(-1))]
            assert not (u32(empty) & 0x7fffffff).any()
    return int(keep.sum())


@pytest.mark.parametrize("n", bm.SHAPES)
def test_builder_equals_model(gpu_pkg, n):
    """Blob-masked, all-non-zero and all-zero densities at every shape: brick counts, index and every stored value."""
    rng = np.random.default_rng(7 + sum(n))
    nvox = n[0] * n[1] * n[2]
    blob = bm.blob_density(n)
    if n in ((40, 33, 47), (64, 64, 64)):   # the sparse fixtures: asserted before the GPU is touched
        empty, seams = bm.sparse_enough(blob, n)
        assert 0.2 <= empty <= 0.9 and all(seams), (n, empty, seams)
    nb = int(np.prod(bm.brick_counts(n)))
    stored = check_storage(gpu_pkg, blob, n, "blob")
    if n in ((40, 33, 47), (64, 64, 64)):
        assert 0 < stored < nb
    assert check_storage(gpu_pkg, rng.uniform(0.05, 1.3, nvox).astype(np.float32), n, "full") == nb   # indexed: the identity
    assert check_storage(gpu_pkg, np.zeros(nvox, dtype=np.float32), n, "zero") == 0                 # no brick; the placeholder slot
    if n == (40, 33, 47):
        dens, voxels = bm.seam_fixture(n)
        check_storage(gpu_pkg, dens, n, "seam fixture")
        check_storage(gpu_pkg, bm.with_minus_zero(dens, n), n, "seam fixture with -0.0")


@pytest.mark.parametrize("n", [(40, 33, 47), (23, 15, 8)])
def test_isolated_voxels_switch_on_every_brick_that_reads_them(gpu_pkg, n):
    """One non-zero voxel in a zero grid.  Raw voxel v lies in brick v >> 3 and, when v = 7 (mod 8), in brick (v + 1) >> 3 as well
    (brick b reads raw 8b - 1 .. 8b + 7): 2 ^ (number of such axes) bricks keep it.  Coordinates 6, 7 and 0 (mod 8), 0 and n - 1,
    on each axis alone and on all three together."""
    mid = [min(3, k - 1) for k in n]
    cand = [sorted({c for c in (0, 6, 7, 8, 14, 15, 16, k - 1) if c < k}) for k in n]
    cases = []
    for a in range(3):
        for c in cand[a]:
            v = list(mid)
            v[a] = c
            cases.append(tuple(v))
    for c in (0, 6, 7, 8):
        if all(c < k for k in n):
            cases.append((c, c, c))
    cases += [(15, 7, 7), (7, 14, 7)] if n == (23, 15, 8) else [(39, 31, 7), (23, 15, 39)]
    cases.append(tuple(k - 1 for k in n))
    for x, y, z in cases:
        d = np.zeros((n[2], n[1], n[0]), dtype=np.float32)
        d[z, y, x] = 0.7
        want = 2 ** sum(1 for c in (x, y, z) if c % 8 == 7)
        assert check_storage(gpu_pkg, d, n, "voxel %r" % ((x, y, z),)) == want, (x, y, z)


def value_edge_density():
    """24^3 (4 x 4 x 4 bricks), one value each in a brick of its own: the smallest float32 subnormal, a negative value, -0.0f."""
    d = np.zeros((24, 24, 24), dtype=np.float32)
    d[3, 3, 3] = np.float32(1e-45)       # brick (0, 0, 0)
    d[3, 11, 19] = np.float32(-0.75)     # brick (2, 1, 0)
    d[19, 19, 11] = np.float32(-0.0)     # brick (1, 2, 2)
    return d


def test_value_edges_of_the_flag(gpu_pkg):
    """A subnormal and a negative value keep their bricks; -0.0f compares equal to zero: its brick is dropped and a lookup there
    answers +0.0f where the dense layout and the raw array hold -0.0f.  Whether that sign can reach any output is decided by
    test_minus_zero_voxels_change_no_output below: it cannot, so the flag stays a comparison with zero."""
    d = value_edge_density()
    assert u32(d)[19, 19, 11] == 0x80000000 and u32(d)[3, 3, 3] == 1
    keep = bm.flags(d.reshape(-1), (24, 24, 24))
    assert keep[0, 0, 0] and keep[0, 1, 2] and not keep[2, 2, 1] and keep.sum() == 2
    assert check_storage(gpu_pkg, d, (24, 24, 24), "value edges") == 2


def test_read_back_refuses_other_media(gpu_pkg):
    P = gpu_pkg
    r = P.Renderer(P.fog_box_scene(16, 16), P.app_f_params(), 16, 16)
    for call in (r.brick_info, r.brick_storage):
        with pytest.raises(P.VspgError) as e:
            call()
        assert e.value.code == P.VSPG_EINVAL and "grid medium" in str(e.value)
    r.close()
    assert r.lib.vspg_brick_info(None, None) == P.VSPG_EINVAL and r.lib.vspg_brick_read(None, None, None, None) == P.VSPG_EINVAL
    # either output may be left out
    dens = bm.blob_density((23, 15, 8))
    g = create(P, "indexed", scenes.grid_scene(dens, (23, 15, 8), 0.1, 1.0, W=8, H=8), P.app_f_params(), 8, 8)
    index, octs = g.brick_storage()
    assert g.brick_storage(octets=False)[1] is None and np.array_equal(g.brick_storage(octets=False)[0], index)
    assert g.brick_storage(index=False)[0] is None and np.array_equal(u32(g.brick_storage(index=False)[1]), u32(octs))
    g.close()


# ---------------------------------------------------------------------------------------------
# the read site (GridMediumT::octet) in every kernel family: indexed == dense == oracle
# ---------------------------------------------------------------------------------------------
def medium_scene(P, kind, dens, n, W, H):
    """The three shapes a grid reaches the kernels in.  "grid": GridMedium in the closed box, chromatic coefficients;
    "nvdb": NanoVDB semantics with a negative index_min component, a density offset and a majorant scale (CLOUD_SWEEP's);
    "cloud": the reference's cloud-scene shape -- camera in vacuum, interface sphere, grey coefficients."""
    if kind == "grid":
        return scenes.grid_scene(dens, n, (0.05, 0.08, 0.1), (3.0, 2.6, 2.2), g=0.5, bmin=BMIN, bmax=BMAX, W=W, H=H)
    if kind == "nvdb":
        vox = tuple(1.6 / n[k] for k in range(3))
        return scenes.nvdb_scene(dens, n, (0.05, 0.08, 0.1), (3.0, 2.6, 2.2), g=0.5, index_min=NVDB_IMIN, voxel=vox,
                                 origin=(-0.75 + 2 * vox[0], -0.8 - vox[1], -0.5), density_offset=0.01, majorant_scale=1.1, W=W, H=H)
    assert kind == "cloud"
    s = scenes.cloud_scene(W, H, dens, n[0])
    s.medium.nx, s.medium.ny, s.medium.nz = n
    return s


def to_world(scene, kind, c):
    """World position of the continuous raw-voxel coordinate c [m, 3] (voxel i's sample sits at c = i)."""
    m = scene.medium
    c = np.asarray(c, dtype=np.float64)
    n = np.array([m.nx, m.ny, m.nz], dtype=np.float64)
    if kind == "nvdb":
        return np.array(list(m.grid_origin)) + (c + np.array(list(m.index_min))) * np.array(list(m.voxel_size))
    lo, hi = np.array(list(m.bounds_min)), np.array(list(m.bounds_max))
    return lo + (c + 0.5) / n * (hi - lo)


def seam_sites(dens, n, voxels, per_axis=30):
    """(centre [3], axis): the lookups of a ray along `axis` change brick where the base voxel passes 8b - 1, i.e. at
    c[axis] = 8b - 1.  Sites: below the isolated voxels of the fixture (they sit at 8b; brick b - 1 is dropped), and on faces between
    a kept brick and a dropped neighbour along each axis, through the kept brick's non-zero voxel nearest the face (so that the
    voxel's majorant cell reaches across it) -- the nearest `per_axis` such faces per axis."""
    keep = bm.flags(dens, n)
    d = np.asarray(dens).reshape(n[2], n[1], n[0])
    sites = [(tuple(float(c) - (1.0 if k == a else 0.0) for k, c in enumerate((x, y, z))), a) for x, y, z, a in voxels]
    for a in range(3):
        found = []
        for bz, by, bx in np.argwhere(keep):
            b = (bx, by, bz)
            lo = [max(8 * b[k] - 1, 0) for k in range(3)]
            own = np.argwhere(d[lo[2]:8 * bz + 8, lo[1]:8 * by + 8, lo[0]:8 * bx + 8] != 0)[:, ::-1] + np.array(lo)   # (x, y, z)
            for step in (-1, 1):
                nb = list(b)
                nb[a] += step
                if not 0 <= nb[a] < keep.shape[2 - a] or keep[nb[2], nb[1], nb[0]] or len(own) == 0:
                    continue
                seam = 8.0 * max(b[a], nb[a]) - 1.0
                dist = np.abs(own[:, a] + (0.5 if step < 0 else -0.5) - seam)
                v = own[np.argmin(dist)]
                c = [float(v[k]) for k in range(3)]
                c[a] = seam
                found.append((float(dist.min()), tuple(c), a))
        found.sort()
        sites += [(c, ax) for _, c, ax in found[:per_axis]]
    return sites


def tmaj_queries(P, scene, kind, sites, n_random, seed):
    """n_random queries as test_grid_free_flight_vs_oracle draws them, then rays through the seams: along the axis across the seam
    (both ways, jittered sideways) and inside the planes c[axis] = 8b - 1 -+ eps along the other two axes."""
    rng = np.random.default_rng(seed)
    qs = []

    def add(o, d, tmax, i):
        qs.append(P.VspgTmajQuery(P.f3(*o), P.f3(*d), float(tmax), float(rng.random()), float(rng.random()), float(rng.random()),
                                  float(rng.random()) if i % 5 else -1.0, int(rng.integers(0, 3)), int(rng.integers(0, 4))))

    for i in range(n_random):
        d = rng.normal(size=3)
        d = d / np.linalg.norm(d) * rng.uniform(0.5, 2.0)
        add(rng.uniform(-1, 1, 3), d, rng.uniform(0.0, 3.0), i)
    i = 0
    for centre, a in sites:
        centre = np.array(centre)
        others = [k for k in range(3) if k != a]
        rays = []
        for sign in (1.0, -1.0):                           # across the seam
            for _ in range(12):
                c0 = centre + rng.uniform(-1.2, 1.2, 3)
                c0[a] = centre[a] - sign * rng.uniform(3.0, 5.0)
                rays.append((c0, a, sign, 9.0))
        for eps in (-1e-3, 1e-3):                          # inside the plane on either side of the seam
            for k in others:
                for sign in (1.0, -1.0):
                    for _ in range(3):
                        c0 = centre + rng.uniform(-1.0, 1.0, 3)
                        c0[a] = centre[a] + eps
                        c0[k] = centre[k] - sign * rng.uniform(3.0, 5.0)
                        rays.append((c0, k, sign, 9.0))
        for c0, k, sign, length in rays:
            c1 = c0.copy()
            c1[k] += sign * length
            o, e = to_world(scene, kind, c0[None])[0], to_world(scene, kind, c1[None])[0]
            s = rng.uniform(0.5, 2.0)                      # d need not be normalised: tMax is in units of d
            d = np.zeros(3)
            d[k] = sign * s
            add(o, d, abs(e[k] - o[k]) / s, i + 1)
            i += 1
    return qs


def result_bits(res):
    return np.frombuffer(b"".join(bytes(x) for x in res), dtype=np.uint32).reshape(len(res), -1)


@pytest.fixture(scope="module")
def fixture_density():
    dens, voxels = bm.seam_fixture(N)
    empty, seams = bm.sparse_enough(dens, N)
    assert 0.2 <= empty <= 0.9 and all(seams), (empty, seams)
    return dens, voxels


@pytest.fixture(scope="module", params=["grid", "nvdb", "cloud"])
def trio(request, gpu_pkg, fixture_density):
    """(kind, scene, indexed renderer, dense renderer, oracle) on the sparse fixture."""
    P = gpu_pkg
    kind = request.param
    dens, voxels = fixture_density
    W, H = 64, 48
    scene = medium_scene(P, kind, dens, N, W, H)
    prm = P.app_f_params()
    gi, gd = (create(P, layout, scene, prm, W, H, seed=3) for layout in LAYOUTS)
    ii, di = gi.brick_info(), gd.brick_info()
    assert ii["indexed"] == 1 and di["indexed"] == 0 and 0 < ii["n_stored"] < di["n_stored"] == 6 * 5 * 6
    c = oracle_lib.OracleRenderer(scene, prm, W, H, seed=3)
    yield kind, scene, gi, gd, c
    gi.close(); gd.close(); c.close()


# The shares below are about half of what the oracle gives for these seeds (printed by the test; random queries: 0.050 / 0.046 /
# 0.87 at least on "grid", 0.11 / 0 / 0.70 on "nvdb", 0.071 / 0.073 / 0.82 on "cloud"; seam queries: 0.13 / 0.12 at least):
# conditions on the test's own inputs that keep it from passing vacuously -- enough queries must meet density, enough must meet
# tentative collisions in empty space only (the lookups that land in dropped bricks or in the zero part of stored ones), enough
# must meet nothing.  (Under the density offset of "nvdb" every tentative collision sees a density: no second share there.)
MIN_SHARE = {"grid": (0.025, 0.02, 0.4), "nvdb": (0.05, 0.0, 0.3), "cloud": (0.035, 0.035, 0.4)}


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_free_flight_indexed_equals_dense_equals_oracle(gpu_pkg, trio, fixture_density, variant):
    """SampleT_maj / _OpticalDepthSpace / _Resampling with a recording callback: every field of every result."""
    kind, scene, gi, gd, c = trio
    dens, voxels = fixture_density
    P = gpu_pkg
    qs = tmaj_queries(P, scene, kind, seam_sites(dens, N, voxels), 20000, 40 + variant)
    oc = c.sample_tmaj_batch(variant, qs)
    co = result_bits(oc)
    ncb = np.array([x.n_callbacks for x in oc])
    ssum = np.array([x.sum_sigt_over_maj for x in oc])
    for lo, hi, what in ((0, 20000, "random"), (20000, len(qs), "seam")):
        dense_share = float(np.mean(ssum[lo:hi] > 0))
        empty_share = float(np.mean((ncb[lo:hi] > 0) & (ssum[lo:hi] == 0)))
        none_share = float(np.mean(ncb[lo:hi] == 0))
        print("%s variant %d %s queries: %d, saw density %.4f, collisions in empty space only %.4f, no collision %.4f"
              % (kind, variant, what, hi - lo, dense_share, empty_share, none_share))
        if what == "random":
            a, b, d = MIN_SHARE[kind]
            assert dense_share >= a and empty_share >= b and none_share >= d
        else:
            assert hi - lo >= 3000 and dense_share >= 0.06 and (empty_share >= 0.06 or kind == "nvdb")
    for g, layout in ((gi, "indexed"), (gd, "dense")):
        go = result_bits(g.sample_tmaj_batch(variant, qs))
        bad = np.flatnonzero((go != co).any(axis=1))
        assert bad.size == 0, (kind, variant, layout, "queries that differ from the oracle:", bad[:8], len(bad))


def test_replayed_paths_indexed_equals_dense_equals_oracle(trio):
    """The per-lane kernel (vspg_trace_paths): radiance bits and segment counts of 20 000 (pixel, sample) pairs."""
    kind, scene, gi, gd, c = trio
    rng = np.random.default_rng(9)
    n = 20000
    pix = np.stack([rng.integers(0, gi.xres, n), rng.integers(0, gi.yres, n)], axis=1).astype(np.int32)
    si = rng.integers(0, 4096, n).astype(np.int32)
    Lc, sc = c.trace_paths(pix, si)
    assert np.isfinite(Lc).all() and Lc.max() > 0 and sc.max() >= 3
    for g, layout in ((gi, "indexed"), (gd, "dense")):
        Lg, sg = g.trace_paths(pix, si)
        assert np.array_equal(sg, sc), (kind, layout, np.flatnonzero(sg != sc)[:8])
        bad = np.flatnonzero((u32(Lg) != u32(Lc)).any(axis=1))
        assert bad.size == 0, (kind, layout, bad[:8], len(bad))


def temperature_grid(scene, dens):
    rng = np.random.default_rng(9)
    temp = (150.0 + 2600.0 * np.clip(dens + 0.3 * rng.random(dens.size).astype(np.float32), 0, 1.4)).astype(np.float32)
    scene.medium.temperature = temp.ctypes.data_as(C.POINTER(C.c_float))
    scene.medium.temperature_offset, scene.medium.temperature_scale, scene.medium.nvdb_le_scale = 120.0, 1.3, 0.6
    scene._temp_keepalive = temp
    return scene


#             name                  scene    options     pipeline kernel                           per-lane kernel
WF_CASES = [("grid-app-f",         "grid",  "app-f",    "k_wf_dist_walk<GridMedium>",             "k_render_wave<GridMedium>"),
            ("grid-defaults",      "grid",  "defaults", "k_wf_walk<GridMedium,guided>",           "k_render_wave<GridMedium,guided>"),
            ("grid-nds",           "grid",  "nds",      "k_wf_segment_vertex<GridMedium>",        "k_render_wave<GridMedium>"),
            ("nvdb-app-f",         "nvdb",  "app-f",    "k_wf_dist_walk<NanoDenseMedium>",        "k_render_wave<NanoDenseMedium>"),
            ("nvdb-nds-blackbody", "nvdb",  "nds",      "k_wf_segment_vertex<NanoDenseMedium>",   "k_render_wave<NanoDenseMedium>"),
            ("cloud-app-f",        "cloud", "app-f",    "k_wf_walk<GridMediumGrey>",              "k_render_wave<GridMediumGrey>"),
            ("cloud-defaults",     "cloud", "defaults", "k_wf_walk<GridMedium,guided>",           "k_render_wave<GridMedium,guided>")]


def render_all_ways(P, scene, prm, field, W, H, seed, waves, expect_wf, expect_lane):
    """Films after wave 0 and after `waves` post-processed waves, and the counters, of {indexed, dense} x {pipeline, per-lane}."""
    out = {}
    for layout in LAYOUTS:
        for kernel, expect in ((None, expect_wf), ("lane", expect_lane)):
            with pytest.MonkeyPatch.context() as mp:     # the kernel is chosen per launch: the variable stays set while rendering
                if kernel:
                    mp.setenv("VSPG_KERNEL", kernel)
                else:
                    mp.delenv("VSPG_KERNEL", raising=False)
                g = create(P, layout, scene, prm, W, H, seed=seed)
                assert g.brick_info()["indexed"] == (layout == "indexed")
                if field is not None:
                    g.set_guiding_field(field, field)
                assert g.kernel_name() == expect, (layout, kernel, g.kernel_name())   # no case silently runs another family
                first = None
                for w in range(waves):
                    g.render_wave(w, w + 1)
                    g.post_process_wave()
                    if w == 0:
                        first = g.film()
                out[(layout, kernel or "wf")] = (first, g.film(), g.counters())
                g.close()
    return out


def check_all_ways(out, oracle_first, oracle_film):
    ref_first, ref_film, ref_counters = out[("dense", "wf")]
    for key, (first, film, counters) in out.items():
        assert np.array_equal(u32(first), u32(ref_first)) and np.array_equal(u32(film), u32(ref_film)), key
        assert counters == ref_counters, key
    assert np.array_equal(u32(ref_first), u32(oracle_first))     # one sample per pixel: the same number in float and double
    assert np.array_equal(ref_film[..., 3], oracle_film[..., 3])
    ig, ic = ref_film[..., :3] / ref_film[..., 3:4], oracle_film[..., :3] / oracle_film[..., 3:4]
    relmse = float(np.mean((ig - ic) ** 2 / (ic ** 2 + 1e-4)))
    assert relmse <= 1e-4, relmse
    assert ref_film[..., :3].max() > 0 and ref_counters["density_queries"] > 0
    return relmse


@pytest.mark.parametrize("case", [c[0] for c in WF_CASES])
def test_wavefront_pipeline_indexed_equals_dense_equals_lane_equals_oracle(gpu_pkg, fixture_density, case):
    """Three post-processed waves (the VSP buffer updates in between) on the wavefront pipeline -- k_wf_dist_walk + k_wf_shadow_walk,
    the merged k_wf_walk, the "nds" shape k_wf_segment_vertex + k_wf_shadow_walk -- and on the per-lane kernel, each on both
    layouts: the four films and counter sets are bit-identical, and the oracle's."""
    P = gpu_pkg
    _, kind, options, expect_wf, expect_lane = next(c for c in WF_CASES if c[0] == case)
    dens, voxels = fixture_density
    W, H = 64, 48
    scene = medium_scene(P, kind, dens, N, W, H)
    prm = P.default_params() if options == "defaults" else P.app_f_params()
    if options == "nds":
        prm.vspsamplingmethod = P.VSP_NDS
    if case == "nvdb-nds-blackbody":
        temperature_grid(scene, dens)
    field = None
    if options == "defaults":
        field = scenes.light_field(P, n=4) if kind != "cloud" else scenes.light_field(P, n=2, bmin=(-3, -3, -3), bmax=(3, 3, 3), light=(0.0, 2.9, 0.0))
    waves = 3
    out = render_all_ways(P, scene, prm, field, W, H, 14, waves, expect_wf, expect_lane)
    c = oracle_lib.OracleRenderer(scene, prm, W, H, seed=14)
    if field is not None:
        c.set_guiding_field(field, field)
    first = None
    for w in range(waves):
        c.render_wave(w, w + 1)
        c.post_process_wave()
        if w == 0:
            first = c.film()
    relmse = check_all_ways(out, first, c.film())
    assert out[("dense", "wf")][2] == c.counters()
    c.close()
    print(case, expect_wf, expect_lane, "relMSE vs oracle %.3e" % relmse)


def test_minus_zero_voxels_change_no_output(gpu_pkg, fixture_density):
    """-0.0f in every voxel the indexed layout drops: the dense layout and the oracle then interpolate -0.0f where the indexed
    one answers +0.0f.  Free flights, replayed paths and films of all three stay bit-identical -- the sign never reaches an
    output (a density of either zero gives sigma_t = +-0, which is added to positive sums or multiplies a probability of zero) --
    so k_brick_flags keeps comparing with 0.f."""
    P = gpu_pkg
    dens, voxels = fixture_density
    mz = bm.with_minus_zero(dens, N)
    W, H = 48, 32
    for kind in ("grid", "nvdb", "cloud"):
        scene = medium_scene(P, kind, mz, N, W, H)
        prm = P.app_f_params()
        gi, gd = (create(P, layout, scene, prm, W, H, seed=5) for layout in LAYOUTS)
        assert gi.brick_info()["n_stored"] == int(bm.flags(dens, N).sum())
        c = oracle_lib.OracleRenderer(scene, prm, W, H, seed=5)
        for variant in (0, 1, 2):
            qs = tmaj_queries(P, scene, kind, seam_sites(dens, N, voxels, per_axis=10), 6000, 90 + variant)
            co = result_bits(c.sample_tmaj_batch(variant, qs))
            for g in (gi, gd):
                assert np.array_equal(result_bits(g.sample_tmaj_batch(variant, qs)), co), (kind, variant)
        rng = np.random.default_rng(2)
        pix = np.stack([rng.integers(0, W, 8000), rng.integers(0, H, 8000)], axis=1).astype(np.int32)
        si = rng.integers(0, 1024, 8000).astype(np.int32)
        Lc, sc = c.trace_paths(pix, si)
        for g in (gi, gd):
            Lg, sg = g.trace_paths(pix, si)
            assert np.array_equal(sg, sc) and np.array_equal(u32(Lg), u32(Lc)), kind
        gi.close(); gd.close()
        wf = {"grid": "k_wf_dist_walk<GridMedium>", "nvdb": "k_wf_dist_walk<NanoDenseMedium>", "cloud": "k_wf_walk<GridMediumGrey>"}[kind]
        lane = {"grid": "k_render_wave<GridMedium>", "nvdb": "k_render_wave<NanoDenseMedium>", "cloud": "k_render_wave<GridMediumGrey>"}[kind]
        out = render_all_ways(P, scene, prm, None, W, H, 5, 2, wf, lane)
        first = None
        for w in range(2):
            c.render_wave(w, w + 1)
            c.post_process_wave()
            if w == 0:
                first = c.film()
        check_all_ways(out, first, c.film())
        c.close()


# ---------------------------------------------------------------------------------------------
# the automatic choice at production scale
# ---------------------------------------------------------------------------------------------
BIG = (1160, 520, 456)          # 146 x 66 x 58 = 558 888 bricks: above the dense budget of 524 288 (8 GiB of octets)
UNDER = (512, 512, 504)         # 65 x 65 x 64 = 270 400 bricks: below it


def test_automatic_layout_at_production_scale(gpu_pkg):
    """Without VSPG_DENSE_BRICKS a grid whose bricks exceed the dense budget takes the indexed layout by itself -- 2.75e8 voxels,
    three different brick counts per axis, n not a multiple of 8 on two axes, more than 2^16 stored bricks -- and computes what
    the oracle computes from the raw array; a grid just under the budget takes the dense layout.

    Measured on an MI355X: 2.7 s wall time for this test (0.8 s of it generating the density, 0.4 s creating the renderer:
    122 525 of 558 888 bricks stored, 2.0 GB of octets behind a 2.2 MB index), peak host RSS of the pytest process 3.5 GB (the
    density and the oracle's copy of it are 1.1 GB each).  An allocation that fails is a failure of the test."""
    P = gpu_pkg
    t0 = time.time()
    assert "VSPG_DENSE_BRICKS" not in os.environ and "VSPG_KERNEL" not in os.environ
    dens = bm.coarse_blob_density(BIG)
    keep = bm.flags_slabwise(dens, BIG)
    bnx, bny, bnz = bm.brick_counts(BIG)
    nb = bnx * bny * bnz
    assert (bnx, bny, bnz) == (146, 66, 58) and nb > (8 << 30) // (512 * 32) and len({bnx, bny, bnz}) == 3
    share = keep.mean()
    print("big grid: %d of %d bricks hold a value (%.3f), generated in %.1f s" % (keep.sum(), nb, share, time.time() - t0))
    assert 0.10 <= share <= 0.40
    W, H = 64, 48
    scene = scenes.grid_scene(dens, BIG, (0.05, 0.08, 0.1), (3.0, 2.6, 2.2), g=0.5, bmin=(-0.9, -0.8, -0.5), bmax=(0.9, 0.7, 0.9), W=W, H=H)
    prm = P.app_f_params()
    t1 = time.time()
    g = create(P, None, scene, prm, W, H, seed=3)
    print("big grid: renderer created in %.1f s" % (time.time() - t1))
    info = g.brick_info()
    assert info["indexed"] == 1 and (info["bnx"], info["bny"], info["bnz"]) == (bnx, bny, bnz)
    assert info["n_stored"] == int(keep.sum()) and info["octet_bytes"] == info["n_stored"] * 512 * 32 and info["index_bytes"] == 4 * nb
    index, _ = g.brick_storage(octets=False)
    assert np.array_equal(index, bm.slots(keep))        # the whole index against the slab-wise model
    del index
    # the model proper on a sub-box of bricks that holds kept and dropped ones: flags() of the voxels those bricks read
    edge = np.argwhere(keep[:, :, :-1] != keep[:, :, 1:])
    kz, ky, kx = edge[len(edge) // 2]
    b0 = [max(int(kx) - 3, 1), max(int(ky) - 3, 1), max(int(kz) - 3, 1)]
    d3 = dens.reshape(BIG[2], BIG[1], BIG[0])
    sub = np.ascontiguousarray(d3[8 * b0[2]:8 * b0[2] + 56, 8 * b0[1]:8 * b0[1] + 56, 8 * b0[0]:8 * b0[0] + 56])
    # sub voxel v = raw 8 b0 + v, 56 per axis: the sub-grid's bricks 1 .. 6 read voxels 7 .. 55 only, all inside it
    sub_keep = bm.flags(sub.reshape(-1), sub.shape[::-1])
    want = keep[b0[2] + 1:b0[2] + 7, b0[1] + 1:b0[1] + 7, b0[0] + 1:b0[0] + 7]
    assert np.array_equal(sub_keep[1:7, 1:7, 1:7], want) and want.any() and not want.all()
    c = oracle_lib.OracleRenderer(scene, prm, W, H, seed=3)
    rng = np.random.default_rng(17)
    n = 4000
    pix = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], axis=1).astype(np.int32)
    si = rng.integers(0, 4096, n).astype(np.int32)
    Lg, sg = g.trace_paths(pix, si)
    Lc, sc = c.trace_paths(pix, si)
    assert np.array_equal(sg, sc) and np.array_equal(u32(Lg), u32(Lc))
    assert np.isfinite(Lc).all() and Lc.max() > 0 and sc.max() >= 3
    for variant in (0, 1, 2):
        qs = tmaj_queries(P, scene, "grid", [], 3000, 60 + variant)
        oc = c.sample_tmaj_batch(variant, qs)
        assert np.mean([x.sum_sigt_over_maj > 0 for x in oc]) >= 0.06, variant   # (the oracle gives 0.12 .. 0.14 for these seeds)
        assert np.array_equal(result_bits(g.sample_tmaj_batch(variant, qs)), result_bits(oc)), variant
    c.close()
    assert g.kernel_name() == "k_wf_dist_walk<GridMedium>"
    g.render_wave(0, 1)
    film_wf = g.film()
    counters = g.counters()
    g.close()
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("VSPG_KERNEL", "lane")
        lane = create(P, None, scene, prm, W, H, seed=3)
        assert lane.brick_info()["indexed"] == 1 and lane.kernel_name() == "k_render_wave<GridMedium>"
        lane.render_wave(0, 1)
        assert np.array_equal(u32(lane.film()), u32(film_wf)) and lane.counters() == counters
        lane.close()
    assert film_wf[..., :3].max() > 0 and counters["density_queries"] > 0
    del dens, d3, scene
    # just under the budget: dense by itself (a mostly empty grid; no rendering)
    few = np.zeros(UNDER[0] * UNDER[1] * UNDER[2], dtype=np.float32)
    few.reshape(UNDER[2], UNDER[1], UNDER[0])[100:108, 200:216, 300:332] = 0.5
    under = create(P, None, scenes.grid_scene(few, UNDER, 0.1, 1.0, W=8, H=8), prm, 8, 8)
    ui = under.brick_info()
    under.close()
    assert ui["indexed"] == 0 and ui["n_stored"] == 65 * 65 * 64 == 270400 and ui["index_bytes"] == 0 and ui["octet_bytes"] == 270400 * 512 * 32
    print("big grid: wall time %.1f s, peak host RSS %.2f GB" % (time.time() - t0, resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20))
