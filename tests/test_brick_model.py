"""The NumPy model of the octet-brick layout (tests/brick_model.py) against something independent of it: the raw density
array read voxel by voxel.  This is where "dropping the empty bricks loses nothing" is checked without a GPU; the GPU tests
(test_brick_storage_gpu.py) then hold the builder kernels and the kernels' read site to the model."""
import numpy as np
import pytest

import brick_model as bm


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _densities(n):
    rng = np.random.default_rng(sum(n))
    full = rng.uniform(0.05, 1.3, n[0] * n[1] * n[2]).astype(np.float32)
    return {"blob": bm.blob_density(n), "full": full, "zero": np.zeros_like(full)}


def test_known_answers_of_the_model():
    n = (23, 15, 8)
    assert bm.brick_counts(n) == (3, 2, 2) and bm.brick_counts((40, 33, 47)) == (6, 5, 6)
    assert bm.brick_counts((7, 7, 7)) == (1, 1, 1) and bm.brick_counts((8, 8, 8)) == (2, 2, 2) and bm.brick_counts((1, 1, 1)) == (1, 1, 1)

    def kept(x, y, z, v=1.0):
        d = np.zeros((n[2], n[1], n[0]), dtype=np.float32)
        d[z, y, x] = v
        return {tuple(int(k) for k in b[::-1]) for b in np.argwhere(bm.flags(d.reshape(-1), n))}   # (bx, by, bz)

    assert kept(6, 3, 2) == {(0, 0, 0)}
    assert kept(7, 3, 2) == {(0, 0, 0), (1, 0, 0)}            # raw plane 7 belongs to bricks 0 and 1
    assert kept(8, 3, 2) == {(1, 0, 0)}
    assert kept(15, 7, 7) == {(bx, by, bz) for bx in (1, 2) for by in (0, 1) for bz in (0, 1)}
    assert kept(22, 14, 7) == {(2, 1, 0), (2, 1, 1)}
    assert kept(0, 0, 0) == {(0, 0, 0)}
    assert kept(3, 3, 3, np.float32(1e-45)) == {(0, 0, 0)} and kept(3, 3, 3, -2.0) == {(0, 0, 0)}
    assert kept(3, 3, 3, np.float32(-0.0)) == set()           # -0.0f == 0.f
    assert bm.slots(np.array([[[True, False, True], [False, False, True]]])).reshape(-1).tolist() == [0, -1, 1, -1, -1, 2]
    d = np.arange(1, 9, dtype=np.float32)                     # 2 x 2 x 2, x fastest
    assert bm.octet(d, (2, 2, 2), [0], [0], [0])[0].tolist() == [1, 2, 3, 4, 5, 6, 7, 8]
    assert bm.octet(d, (2, 2, 2), [-1], [-1], [-1])[0].tolist() == [0, 0, 0, 0, 0, 0, 0, 1]
    assert bm.octet(d, (2, 2, 2), [1], [0], [1])[0].tolist() == [6, 0, 8, 0, 0, 0, 0, 0]


def test_blob_fixture_is_sparse_with_seams():
    for n in ((40, 33, 47), (64, 64, 64)):
        empty, seams = bm.sparse_enough(bm.blob_density(n), n)
        print(n, "empty bricks %.3f" % empty, seams)
        assert 0.2 <= empty <= 0.9 and all(seams)


@pytest.mark.parametrize("n", bm.SHAPES)
@pytest.mark.parametrize("indexed", [True, False])
def test_stored_octets_equal_raw_reads(n, indexed):
    """Every octet a lookup can ask for (base voxels -2 .. n per axis, two past the valid range on either side), fetched from
    the model's storage, is the raw array's eight values bit for bit; so are both interpolations at random points."""
    ax = [np.arange(-2, k + 1) for k in n]
    iz, iy, ix = (v.reshape(-1) for v in np.meshgrid(ax[2], ax[1], ax[0], indexing="ij"))
    rng = np.random.default_rng(3)
    pts = rng.uniform(-0.1, 1.1, (4000, 3)).astype(np.float32)
    imin = (-2, 1, 0)
    xs = (rng.uniform(-1.5, 1.5 + np.array(n), (4000, 3)) + np.array(imin)).astype(np.float32)
    for name, dens in _densities(n).items():
        index, octs = bm.storage(dens, n, indexed)
        nb = int(np.prod(bm.brick_counts(n)))
        assert index.size == nb and octs.shape[0] == (int(bm.flags(dens, n).sum()) if indexed else nb)
        if name == "full" or not indexed:
            assert np.array_equal(index.reshape(-1), np.arange(nb))
        if name == "zero" and indexed:
            assert octs.shape[0] == 0 and np.all(index == -1)
        got, want = bm.fetch(index, octs, n, ix, iy, iz), bm.raw_octet(dens, n, ix, iy, iz)
        assert np.array_equal(_bits(got), _bits(want)), name
        inside = (ix >= -1) & (ix < n[0]) & (iy >= -1) & (iy < n[1]) & (iz >= -1) & (iz < n[2])
        assert np.array_equal(_bits(bm.octet(dens, n, ix[inside], iy[inside], iz[inside])), _bits(want[inside]))
        a = bm.lerp_grid(pts, n, lambda i, j, k: bm.fetch(index, octs, n, i, j, k))
        b = bm.lerp_grid(pts, n, lambda i, j, k: bm.raw_octet(dens, n, i, j, k))
        assert np.array_equal(_bits(a), _bits(b))
        a = bm.lerp_index(xs, imin, lambda i, j, k: bm.fetch(index, octs, n, i, j, k))
        b = bm.lerp_index(xs, imin, lambda i, j, k: bm.raw_octet(dens, n, i, j, k))
        assert np.array_equal(_bits(a), _bits(b))
        if name == "full":   # (the blob of a tiny grid may be empty)
            assert np.count_nonzero(a) > 0


def test_the_fixture_sees_a_swapped_stride():
    """A read site that numbered the bricks with bnx and bny exchanged, or the octets of a brick with x and y exchanged,
    disagrees with the raw array on the non-cubic sparse fixture: the shape can tell the strides apart."""
    n = (40, 33, 47)
    dens = bm.blob_density(n)
    index, octs = bm.storage(dens, n, True)
    ax = [np.arange(-1, k) for k in n]
    iz, iy, ix = (v.reshape(-1) for v in np.meshgrid(ax[2], ax[1], ax[0], indexing="ij"))
    want = bm.raw_octet(dens, n, ix, iy, iz)
    bnx, bny, bnz = bm.brick_counts(n)
    swapped = index.reshape(-1)[: bnz * bny * bnx].reshape(bnz, bnx, bny).transpose(0, 2, 1)   # cell = (bz * bnx + bx) * bny + by
    assert not np.array_equal(_bits(bm.fetch(np.ascontiguousarray(swapped), octs, n, ix, iy, iz)), _bits(want))
    assert not np.array_equal(_bits(bm.fetch(index, np.ascontiguousarray(octs.transpose(0, 1, 3, 2, 4)), n, ix, iy, iz)), _bits(want))
