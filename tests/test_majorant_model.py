"""Known answers of tests/majorant_model.py, the NumPy model the device-built majorant grids are compared with
(tests/test_medium_update_gpu.py).  The expected tables here are derived by hand (exact rational arithmetic on inputs every step of
which is exactly representable), not by the model's own code."""
from fractions import Fraction

import numpy as np

import majorant_model as mm


def brute_force(dens, n, ranges, res, start_at_lo):
    """Cell by cell over the cell's own box, as the builders' loops run (not separably, as the model does)."""
    d = np.asarray(dens, dtype=np.float32).reshape(n[2], n[1], n[0])
    out = np.zeros((res, res, res), dtype=np.float32)
    (xl, xh), (yl, yh), (zl, zh) = ranges
    for z in range(res):
        for y in range(res):
            rows = d[zl[z]:zh[z] + 1, yl[y]:yh[y] + 1]
            for x in range(res):
                box = rows[:, :, xl[x]:xh[x] + 1]
                mx = d[zl[z], yl[y], xl[x]] if start_at_lo else np.float32(0)
                out[z, y, x] = max(mx, box.max()) if box.size else mx
    return out


def test_grid_tables_by_hand():
    """n = 16: cell c reads samples c - 1 .. c + 1; n = 32: 2c - 1 .. 2c + 2; n = 8: floor(c / 2 - .5) .. floor((c + 1) / 2 - .5) + 1;
    all clipped to the grid."""
    (lo16, hi16), (lo32, hi32), (lo8, hi8) = mm.ranges_grid((16, 32, 8))
    c = np.arange(16)
    assert np.array_equal(lo16, np.maximum(c - 1, 0)) and np.array_equal(hi16, np.minimum(c + 1, 15))
    assert np.array_equal(lo32, np.maximum(2 * c - 1, 0)) and np.array_equal(hi32, np.minimum(2 * c + 2, 31))
    assert list(lo8) == [0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7]      # floor((c - 1) / 2), clipped below
    assert list(hi8) == [1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 7, 7]      # floor(c / 2) + 1, clipped above


def test_single_voxel_lights_exactly_the_cells_whose_tables_hold_it():
    n = (16, 32, 8)
    v = (5, 17, 7)
    d = np.zeros((n[2], n[1], n[0]), dtype=np.float32)
    d[v[2], v[1], v[0]] = 0.7
    maj = mm.majorant_grid(d, n)
    lit = np.argwhere(maj != 0)
    # by hand: x 5 in c - 1 .. c + 1 -> c = 4, 5, 6; y 17 in 2c - 1 .. 2c + 2 -> c = 8, 9; z 7 (the last sample) -> c = 12 .. 15
    want = [(z, y, x) for z in (12, 13, 14, 15) for y in (8, 9) for x in (4, 5, 6)]
    assert sorted(map(tuple, lit)) == sorted(want)
    assert (maj[maj != 0] == np.float32(0.7)).all()
    # and against the tables themselves, for a voxel on no special position
    r = mm.ranges_grid(n)
    sets = [np.flatnonzero((lo <= c) & (c <= hi)) for (lo, hi), c in zip(r, v)]
    assert len(lit) == len(sets[0]) * len(sets[1]) * len(sets[2])


def test_one_voxel_along_an_axis():
    """nx = 1: every cell's x range is the one sample; the majorants are constant along x."""
    n = (1, 5, 9)
    (xl, xh), (yl, yh), (zl, zh) = mm.ranges_grid(n)
    assert not xl.any() and not xh.any()
    assert yl[0] == 0 and yh[15] == 4 and zl[0] == 0 and zh[15] == 8 and (yh >= yl).all() and (zh >= zl).all()
    rng = np.random.default_rng(3)
    d = rng.uniform(0.1, 1.0, n[0] * n[1] * n[2]).astype(np.float32)
    maj = mm.majorant_grid(d, n)
    assert (maj == maj[:, :, :1]).all()
    assert np.array_equal(maj, brute_force(d, n, mm.ranges_grid(n), 16, True))


def test_grid_model_equals_the_loops_with_negative_values():
    """The start value is the sample at the low corner, not 0: a box of negative samples has a negative majorant."""
    n = (17, 33, 40)
    rng = np.random.default_rng(5)
    d = rng.uniform(0.05, 1.3, (n[2], n[1], n[0])).astype(np.float32)
    d[4:20, 3:18, 2:12] = -rng.uniform(0.1, 0.9, (16, 15, 10)).astype(np.float32)
    d[30:, :, :] = 0
    maj = mm.majorant_grid(d, n)
    assert (maj < 0).any() and (maj == 0).any() and (maj > 0).any()
    assert mm.same_majorants(maj, brute_force(d, n, mm.ranges_grid(n), 16, True))


NVDB = dict(index_min=(-8, 3, -20), voxel_size=(0.5, 0.25, 0.125), grid_origin=(0.0, 1.0, -2.0))


def nvdb_case(n):
    imin, vox, org = NVDB["index_min"], NVDB["voxel_size"], NVDB["grid_origin"]
    bmin = tuple(org[k] + imin[k] * vox[k] for k in range(3))
    bmax = tuple(org[k] + (imin[k] + n[k]) * vox[k] for k in range(3))
    return imin, bmin, bmax, org, vox


def test_nvdb_tables_by_hand():
    """Negative index_min, a non-cubic voxel, every quantity a small dyadic number: cell c of an axis with n samples spans the index
    interval imin + c n / 64 .. imin + (c + 1) n / 64 exactly; widened by one and TRUNCATED (towards zero: -18.5 -> -18), clipped to
    imin .. imin + n - 1."""
    n = (64, 16, 32)
    imin, bmin, bmax, org, vox = nvdb_case(n)
    got = mm.ranges_nvdb(n, imin, bmin, bmax, org, vox)
    for k in range(3):
        lo, hi = [], []
        for c in range(64):
            i0, i1 = imin[k] + Fraction(c * n[k], 64), imin[k] + Fraction((c + 1) * n[k], 64)
            trunc = lambda q: int(q) if q >= 0 else -int(-q)
            lo.append(max(trunc(i0 - 1), imin[k]) - imin[k])
            hi.append(min(trunc(i1 + 1), imin[k] + n[k] - 1) - imin[k])
        assert list(got[k][0]) == lo and list(got[k][1]) == hi, k
    # n = 64, imin = -8: index c - 8; lo = c - 9 (all integers), hi = c - 6  ->  array c - 1 .. c + 2
    c = np.arange(64)
    assert np.array_equal(got[0][0], np.maximum(c - 1, 0)) and np.array_equal(got[0][1], np.minimum(c + 2, 63))
    # n = 32, imin = -20: truncation towards zero shows on the negative half-integers: c = 5 -> -20 + 2.5 - 1 = -18.5 -> -18 -> array 2
    assert got[2][0][5] == 2 and got[2][0][4] == 1 and got[2][0][7] == 3


def test_nvdb_offset_scale_and_start_value():
    """(max + 0.25) * 1.5 in float; the start value is 0: a box of negative samples gives (0 + 0.25) * 1.5."""
    n = (64, 16, 32)
    imin, bmin, bmax, org, vox = nvdb_case(n)
    d = np.zeros((n[2], n[1], n[0]), dtype=np.float32)
    d[10, 5, 20] = 0.7
    d[20:, :, :] = -0.5
    maj = mm.majorant_nvdb(d, n, imin, bmin, bmax, org, vox, 0.25, 1.5)
    lit = np.argwhere(maj != np.float32(0.375))
    # x 20 in c - 1 .. c + 2 -> c = 18 .. 21; y (n = 16: index 3 + c / 4, -1 / +1, truncated) ; z likewise: from the tables
    r = mm.ranges_nvdb(n, imin, bmin, bmax, org, vox)
    sets = [np.flatnonzero((lo <= v) & (v <= hi)) for (lo, hi), v in zip(r, (20, 5, 10))]
    assert list(sets[0]) == [18, 19, 20, 21]
    assert sorted(map(tuple, lit)) == sorted((z, y, x) for z in sets[2] for y in sets[1] for x in sets[0])
    assert (maj[maj != np.float32(0.375)] == (np.float32(0.7) + np.float32(0.25)) * np.float32(1.5)).all()
    assert maj[63, 0, 0] == np.float32(0.375)     # all negative there


def test_nvdb_model_equals_the_loops_on_a_narrow_grid():
    """Fewer samples than cells on two axes, bounds that are no dyadic numbers."""
    n = (20, 7, 33)
    imin = (-7, 3, -20)
    vox = (0.05, 0.11, 0.03)
    org = (-0.3, -0.9, 0.2)
    bmin = tuple(np.float32(org[k] + imin[k] * vox[k]) for k in range(3))
    bmax = tuple(np.float32(org[k] + (imin[k] + n[k]) * vox[k]) for k in range(3))
    rng = np.random.default_rng(8)
    d = rng.uniform(0.05, 1.3, (n[2], n[1], n[0])).astype(np.float32)
    d[:10, :, :8] = -0.3
    d[25:, :, :] = 0
    r = mm.ranges_nvdb(n, imin, bmin, bmax, org, vox)
    for k, (lo, hi) in enumerate(r):
        assert lo.min() >= 0 and hi.max() <= n[k] - 1 and (np.diff(lo) >= 0).all() and (np.diff(hi) >= 0).all()
    maj = mm.majorant_nvdb(d, n, imin, bmin, bmax, org, vox, 0.25, 1.5)
    want = (brute_force(d, n, r, 64, False) + np.float32(0.25)) * np.float32(1.5)
    assert mm.same_majorants(maj, want.astype(np.float32))


def test_same_majorants_ignores_only_the_sign_of_zero():
    a = np.array([0.0, -0.0, 1.0, -1.0], dtype=np.float32)
    assert mm.same_majorants(a, np.array([-0.0, 0.0, 1.0, -1.0], dtype=np.float32))
    assert not mm.same_majorants(a, np.array([0.0, 0.0, np.nextafter(np.float32(1), np.float32(2)), -1.0], dtype=np.float32))
    assert not mm.same_majorants(a, np.array([0.0, 0.0, 1.0, 1.0], dtype=np.float32))
