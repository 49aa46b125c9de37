"""NumPy model of the majorant grids of grid media (inputs and expected values only; no device, no library).

GridMedium (media.cpp:262-269 with SampledGrid::MaxValue, containers.h:838-854): 16^3 cells; cell c of an axis with n samples covers
the samples floor(c / 16 * n - .5) .. floor((c + 1) / 16 * n - .5) + 1, clipped to 0 .. n - 1; the cell's majorant is the largest
sample of the box, the start value being the sample at the box's low corner.

NanoVDBMedium (media.cpp:600-671): 64^3 cells; the cell's world bounds (float Lerp over the medium bounds) go to index space (double:
(w - grid_origin) / voxel_size), are widened by one voxel, truncated to int and clipped to the index bounding box; the majorant is
(max(0, largest sample of the box) + density_offset) * majorant_scale in float.

A box separates per axis: ranges(...) gives the three tables of (lo, hi) in ARRAY coordinates (hi < lo: empty).  Every operation is
done in the precision the builders use (np.float32 scalars round after each operation, as the host code built without FMA contraction
does; the index-space division is float64)."""
import numpy as np

RES_GRID, RES_NVDB = 16, 64
f32 = np.float32


def ranges_grid(n):
    """[(lo, hi) int arrays of 16 cells] for the axes of a grid with n = (nx, ny, nz) samples."""
    out = []
    for nk in n:
        lo, hi = np.empty(RES_GRID, dtype=np.int64), np.empty(RES_GRID, dtype=np.int64)
        for c in range(RES_GRID):
            p0, p1 = f32(c) / f32(RES_GRID), f32(c + 1) / f32(RES_GRID)
            a = int(np.floor(p0 * f32(nk) - f32(0.5)))
            b = int(np.floor(p1 * f32(nk) - f32(0.5))) + 1
            lo[c], hi[c] = max(a, 0), min(b, nk - 1)
        out.append((lo, hi))
    return out


def lerp(t, a, b):
    return (f32(1) - t) * a + t * b


def ranges_nvdb(n, index_min, bounds_min, bounds_max, grid_origin, voxel_size):
    out = []
    for k, nk in enumerate(n):
        imin, imax = int(index_min[k]), int(index_min[k]) + nk - 1
        b0, b1 = f32(bounds_min[k]), f32(bounds_max[k])
        lo, hi = np.empty(RES_NVDB, dtype=np.int64), np.empty(RES_NVDB, dtype=np.int64)
        for c in range(RES_NVDB):
            w0 = lerp(f32(c) / f32(RES_NVDB), b0, b1)
            w1 = lerp(f32(c + 1) / f32(RES_NVDB), b0, b1)
            i0 = (np.float64(w0) - np.float64(f32(grid_origin[k]))) / np.float64(f32(voxel_size[k]))
            i1 = (np.float64(w1) - np.float64(f32(grid_origin[k]))) / np.float64(f32(voxel_size[k]))
            lo[c] = max(int(np.trunc(i0 - 1.0)), imin) - imin
            hi[c] = min(int(np.trunc(i1 + 1.0)), imax) - imin
        out.append((lo, hi))
    return out


def box_max(dens, n, ranges, empty):
    """[R, R, R] (z, y, x): the largest sample of every cell's box, `empty` where a box holds none.  Separable: x, then y, then z."""
    a = np.asarray(dens, dtype=np.float32).reshape(n[2], n[1], n[0])
    for axis, (lo, hi) in zip((2, 1, 0), ranges):
        parts = []
        for l, h in zip(lo, hi):
            sl = [slice(None)] * 3
            sl[axis] = slice(int(l), int(h) + 1)
            shape = list(a.shape)
            shape[axis] = 1
            parts.append(a[tuple(sl)].max(axis=axis, keepdims=True) if h >= l else np.full(shape, empty, dtype=np.float32))
        a = np.concatenate(parts, axis=axis)
    return a


def majorant_grid(dens, n):
    """GridMedium: [16, 16, 16] float32, z, y, x.  (A box is never empty: lo <= n - 1 and hi >= lo for every n >= 1.)"""
    r = ranges_grid(n)
    assert all((hi >= lo).all() for lo, hi in r)
    return box_max(dens, n, r, 0.0)


def majorant_nvdb(dens, n, index_min, bounds_min, bounds_max, grid_origin, voxel_size, density_offset, majorant_scale):
    """NanoVDBMedium: [64, 64, 64] float32, z, y, x."""
    r = ranges_nvdb(n, index_min, bounds_min, bounds_max, grid_origin, voxel_size)
    mx = np.maximum(box_max(dens, n, r, 0.0), f32(0))     # the start value 0: negative samples and empty boxes give 0
    return ((mx + f32(density_offset)) * f32(majorant_scale)).astype(np.float32)


def majorant_of_scene(scene, dens):
    """The model of the majorant grid a renderer of `scene` (a VspgScene with a GRID or NANOVDB medium) holds for samples `dens`."""
    m = scene.medium
    n = (int(m.nx), int(m.ny), int(m.nz))
    if int(m.type) == 3:   # MEDIUM_NANOVDB
        return majorant_nvdb(dens, n, list(m.index_min), list(m.bounds_min), list(m.bounds_max), list(m.grid_origin), list(m.voxel_size),
                             m.density_offset, m.majorant_scale)
    assert int(m.type) == 2
    return majorant_grid(dens, n)


def same_majorants(a, b):
    """The comparison of two majorant grids: equal under ==, and bit for bit wherever the value is not a zero (the maximum of zeros of
    both signs depends on the order they are met in: its sign is unspecified)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape or not np.array_equal(a, b):
        return False
    nz = a != 0
    return bool(np.array_equal(a.view(np.uint32)[nz], b.view(np.uint32)[nz]))
