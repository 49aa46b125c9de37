"""A plain NumPy statement of the device layout of a grid medium's density ("octet bricks"), written from the description
in csrc/vspg_capi.hip / csrc/vspg_probe_kernels.h / csrc/vspg_device.h / include/vspg.h and not from the builder kernels:

  * the octet of base voxel (ix, iy, iz), -1 <= i <= n - 1 per axis, is the eight raw values at (ix + dx, iy + dy, iz + dz),
    corner number dx + 2 dy + 4 dz, zero outside the grid: what one trilinear lookup reads;
  * the octets are grouped into bricks of 8 x 8 x 8: brick b holds base voxels 8b - 1 .. 8b + 6 per axis (raw voxels
    8b - 1 .. 8b + 7), so there are (n + 8) // 8 bricks per axis, numbered x fastest;
  * a brick is kept iff one of its raw voxels is non-zero; kept bricks take slots in increasing brick number.

`density` is the flat float32 array the scenes carry (x fastest), `n` = (nx, ny, nz).  Test inputs only."""
import numpy as np


def brick_counts(n):
    return tuple((k + 8) // 8 for k in n)   # (bnx, bny, bnz)


def padded(density, n):
    """[z][y][x] array over raw voxels -1 .. 8 bn - 1 per axis (index = voxel + 1), zero outside the grid."""
    nx, ny, nz = n
    bnx, bny, bnz = brick_counts(n)
    p = np.zeros((8 * bnz + 1, 8 * bny + 1, 8 * bnx + 1), dtype=np.float32)
    p[1:nz + 1, 1:ny + 1, 1:nx + 1] = np.asarray(density, dtype=np.float32).reshape(nz, ny, nx)
    return p


def flags(density, n):
    """bool [bnz][bny][bnx]: does the brick hold a non-zero raw voxel (IEEE comparison: -0.0 is zero, a subnormal is not)."""
    m = padded(density, n) != 0
    for axis in range(3):   # windows of 9 voxels, one every 8
        m = np.lib.stride_tricks.sliding_window_view(m, 9, axis=axis).any(axis=-1).take(np.arange(0, m.shape[axis] - 8, 8), axis=axis)
    assert m.shape == brick_counts(n)[::-1]
    return m


def slots(keep):
    """int32 [bnz][bny][bnx]: the kept bricks numbered in increasing brick number, -1 for the others."""
    k = keep.reshape(-1)
    return np.where(k, np.cumsum(k) - 1, -1).astype(np.int32).reshape(keep.shape)


def octet(density, n, ix, iy, iz, pad=None):
    """float32 [..., 8]: the octets of the base voxels (ix, iy, iz) (arrays, each -1 .. n - 1)."""
    p = padded(density, n) if pad is None else pad
    ix, iy, iz = (np.asarray(v, dtype=np.int64) for v in (ix, iy, iz))
    for v, k in zip((ix, iy, iz), n):
        assert v.min() >= -1 and v.max() <= k - 1
    return np.stack([p[iz + 1 + dz, iy + 1 + dy, ix + 1 + dx] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)], axis=-1)


def brick_octets(density, n, b, pad=None):
    """float32 [8][8][8][8] (z, y, x in the brick, corner): brick number b as it is stored.  Base voxels past n - 1 (the brick
    lattice overhangs the grid) read zeros only."""
    p = padded(density, n) if pad is None else pad
    bnx, bny, bnz = brick_counts(n)
    bx, by, bz = b % bnx, (b // bnx) % bny, b // (bnx * bny)
    out = np.empty((8, 8, 8, 8), dtype=np.float32)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                z0, y0, x0 = 8 * bz + dz, 8 * by + dy, 8 * bx + dx   # padded index of base voxel 8b - 1, plus the corner
                out[..., dx + 2 * dy + 4 * dz] = p[z0:z0 + 8, y0:y0 + 8, x0:x0 + 8]   # the padding reaches raw voxel 8 bn - 1
    return out


def storage(density, n, indexed):
    """(index int32 [bnz][bny][bnx], octets float32 [n_stored][8][8][8][8]) of either layout."""
    keep = flags(density, n)
    if not indexed:
        keep = np.ones_like(keep)
    index = slots(keep)
    pad = padded(density, n)
    stored = np.flatnonzero(keep.reshape(-1))
    octs = np.zeros((len(stored), 8, 8, 8, 8), dtype=np.float32)
    for s, b in enumerate(stored):
        octs[s] = brick_octets(density, n, int(b), pad)
    return index, octs


def fetch(index, octs, n, ix, iy, iz):
    """float32 [..., 8]: what a lookup of base voxel (ix, iy, iz) -- any integers -- reads from a stored layout: zeros outside
    -1 .. n - 1 and in a brick without a slot."""
    ix, iy, iz = (np.asarray(v, dtype=np.int64) for v in (ix, iy, iz))
    ox, oy, oz = ix + 1, iy + 1, iz + 1
    inside = (ox >= 0) & (ox <= n[0]) & (oy >= 0) & (oy <= n[1]) & (oz >= 0) & (oz <= n[2])
    cx, cy, cz = (np.where(inside, v, 0) for v in (ox, oy, oz))
    slot = np.where(inside, index[cz >> 3, cy >> 3, cx >> 3], -1)
    out = np.zeros(ix.shape + (8,), dtype=np.float32)
    have = slot >= 0
    out[have] = octs[slot[have], cz[have] & 7, cy[have] & 7, cx[have] & 7]
    return out


def raw_octet(density, n, ix, iy, iz):
    """float32 [..., 8]: the same eight values read from the raw array, voxels outside the grid as zero -- independent of
    everything above."""
    d = np.asarray(density, dtype=np.float32).reshape(n[2], n[1], n[0])
    ix, iy, iz = (np.asarray(v, dtype=np.int64) for v in (ix, iy, iz))
    out = []
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                x, y, z = ix + dx, iy + dy, iz + dz
                ok = (x >= 0) & (x < n[0]) & (y >= 0) & (y < n[1]) & (z >= 0) & (z < n[2])
                out.append(np.where(ok, d[np.where(ok, z, 0), np.where(ok, y, 0), np.where(ok, x, 0)], np.float32(0)))
    return np.stack(out, axis=-1).astype(np.float32)


def lerp_grid(p, n, read):
    """SampledGrid::Lookup(Point3f) in float32 (x, then y, then z; weights (1 - d) a + d b) at points p [m, 3] in [0, 1]^3
    coordinates; read(ix, iy, iz) -> [m, 8]."""
    f = np.float32
    p = np.asarray(p, dtype=f)
    s = [p[:, k] * f(n[k]) - f(0.5) for k in range(3)]
    i = [np.floor(v).astype(np.int64) for v in s]
    dx, dy, dz = (v - k.astype(f) for v, k in zip(s, i))
    o = read(i[0], i[1], i[2])
    one = f(1)
    d00 = (one - dx) * o[:, 0] + dx * o[:, 1]
    d10 = (one - dx) * o[:, 2] + dx * o[:, 3]
    d01 = (one - dx) * o[:, 4] + dx * o[:, 5]
    d11 = (one - dx) * o[:, 6] + dx * o[:, 7]
    a, b = (one - dy) * d00 + dy * d10, (one - dy) * d01 + dy * d11
    r = (one - dz) * a + dz * b
    assert r.dtype == f
    return r


def lerp_index(x, index_min, read):
    """The NanoVDB flavour in float32 at index-space points x [m, 3]: a + w (b - a) along z, then y, then x."""
    f = np.float32
    x = np.asarray(x, dtype=f)
    fl = np.floor(x)
    u, v, w = (x[:, k] - fl[:, k] for k in range(3))
    i = [fl[:, k].astype(np.int64) - index_min[k] for k in range(3)]
    o = read(i[0], i[1], i[2])
    v000, v100, v010, v110, v001, v101, v011, v111 = (o[:, k] for k in range(8))
    a00, a01 = v000 + w * (v001 - v000), v010 + w * (v011 - v010)
    a10, a11 = v100 + w * (v101 - v100), v110 + w * (v111 - v110)
    b0, b1 = a00 + v * (a01 - a00), a10 + v * (a11 - a10)
    r = b0 + u * (b1 - b0)
    assert r.dtype == f
    return r


# ---- test densities ---------------------------------------------------------------------------------------------------
SHAPES = [(40, 33, 47), (23, 15, 8), (8, 8, 8), (7, 7, 7), (1, 1, 1), (5, 9, 3), (64, 64, 64)]


def blob_density(n, seed=11, balls=6):
    """Random values in (0.05, 1.3] inside a few random balls (radius 0.10 .. 0.22 of the shortest side), exact zeros
    elsewhere; flat, x fastest."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = n
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    mask = np.zeros((nz, ny, nx), dtype=bool)
    side = min(n)
    for _ in range(balls):
        c = rng.uniform(0, 1, 3) * np.array([nx, ny, nz])
        r = rng.uniform(0.10, 0.22) * side
        mask |= (x + 0.5 - c[0]) ** 2 + (y + 0.5 - c[1]) ** 2 + (z + 0.5 - c[2]) ** 2 <= r * r
    v = rng.uniform(0.05, 1.3, (nz, ny, nx)).astype(np.float32)
    return np.ascontiguousarray(np.where(mask, v, np.float32(0)).reshape(-1))


def sparse_enough(density, n):
    """The condition a sparse fixture must meet (judged by the model): (share of empty bricks, does a kept brick have an
    empty neighbour along x / y / z)."""
    keep = flags(density, n)
    seam = []
    for axis in (2, 1, 0):
        a, b = np.moveaxis(keep, axis, 0)[:-1], np.moveaxis(keep, axis, 0)[1:]
        seam.append(bool(np.any(a != b)))
    return 1.0 - keep.mean(), tuple(seam)


def covered(keep, n):
    """bool [nz][ny][nx]: the raw voxel lies in at least one kept brick."""
    nx, ny, nz = n
    c = np.zeros((nz, ny, nx), dtype=bool)
    for bz, by, bx in np.argwhere(keep):
        c[max(8 * bz - 1, 0):8 * bz + 8, max(8 * by - 1, 0):8 * by + 8, max(8 * bx - 1, 0):8 * bx + 8] = True
    return c


def seam_fixture(n, seed=11):
    """The sparse fixture of the read-path tests: blob_density plus
      * a block of non-zero voxels filling raw 0 .. 6 per axis, so that slot 0 (brick 0) holds no zero octet a lookup could
        mistake for "empty" -- a read site that fetched slot 0 for a brick without a slot would see density;
      * one isolated voxel per axis at raw coordinate 8 b on that axis (3 mod 8 on the others) in a brick whose predecessor
        along the axis is empty and stays empty: a ray along the axis through the voxel crosses from a dropped brick into a
        stored one inside the voxel's own majorant cell.
    Returns (density, [(x, y, z, axis), ...])."""
    nx, ny, nz = n
    d = blob_density(n, seed).reshape(nz, ny, nx).copy()
    rng = np.random.default_rng(seed + 1)
    d[:min(7, nz), :min(7, ny), :min(7, nx)] = rng.uniform(0.3, 1.3, d[:7, :7, :7].shape).astype(np.float32)
    voxels = []
    for axis in range(3):
        keep = flags(d.reshape(-1), n)
        found = None
        for bz, by, bx in np.argwhere(~keep):
            b = [bx, by, bz]
            p = list(b)
            p[axis] -= 1
            v = [8 * b[k] + 3 for k in range(3)]
            v[axis] = 8 * b[axis]
            if p[axis] < 0 or keep[p[2], p[1], p[0]] or any(v[k] + 4 >= n[k] for k in range(3)):
                continue
            found = v
            break
        assert found is not None, "no room for an isolated voxel along axis %d" % axis
        d[found[2], found[1], found[0]] = np.float32(1.1)
        after = flags(d.reshape(-1), n)
        p = [found[k] >> 3 for k in range(3)]
        assert after[p[2], p[1], p[0]] and after.sum() == keep.sum() + 1   # the voxel switched on its own brick only
        voxels.append((found[0], found[1], found[2], axis))
    return np.ascontiguousarray(d.reshape(-1)), voxels


def with_minus_zero(density, n):
    """The same density with -0.0f in every voxel that lies in dropped bricks only: the kept set does not change (-0.0f == 0.f),
    the dense layout and the raw array now hold sign bits where the indexed layout answers +0.0f."""
    keep = flags(density, n)
    d = np.asarray(density, dtype=np.float32).reshape(n[2], n[1], n[0]).copy()
    hole = ~covered(keep, n)
    assert not d[hole].any()
    d[hole] = np.float32(-0.0)
    assert np.array_equal(flags(d.reshape(-1), n), keep) and hole.any()
    return np.ascontiguousarray(d.reshape(-1))


def flags_slabwise(density, n):
    """flags() for grids too large for a padded copy: one slab of bricks along z at a time, no full-size temporary."""
    nx, ny, nz = n
    bnx, bny, bnz = brick_counts(n)
    d = np.asarray(density).reshape(nz, ny, nx)
    keep = np.zeros((bnz, bny, bnx), dtype=bool)
    plane = np.zeros((8 * bny + 1, 8 * bnx + 1), dtype=bool)
    for bz in range(bnz):
        z0, z1 = max(8 * bz - 1, 0), min(8 * bz + 8, nz)
        plane[1:ny + 1, 1:nx + 1] = (d[z0:z1] != 0).any(axis=0)
        m = plane
        for axis in range(2):
            m = np.lib.stride_tricks.sliding_window_view(m, 9, axis=axis).any(axis=-1).take(np.arange(0, m.shape[axis] - 8, 8), axis=axis)
        keep[bz] = m
    return keep


def coarse_blob_density(n, seed=21, balls=32, shift=(3, 5, 2)):
    """A production-sized sparse density built slab by slab: a blob mask on the brick lattice, moved by `shift` voxels so that
    blob faces do not sit on brick planes, times a cheap integer-hash noise in [0.05, 1.25).  float32 throughout."""
    nx, ny, nz = n
    dims = np.array([(k + 8 + 7) // 8 for k in n])                    # coarse cells along x, y, z
    rng = np.random.default_rng(seed)
    cz, cy, cx = np.ogrid[:dims[2], :dims[1], :dims[0]]
    mask = np.zeros((dims[2], dims[1], dims[0]), dtype=bool)
    for _ in range(balls):
        c = rng.uniform(0.1, 0.9, 3) * dims
        r = rng.uniform(0.10, 0.24, 3) * dims.min()
        mask |= ((cx + 0.5 - c[0]) / r[0]) ** 2 + ((cy + 0.5 - c[1]) / r[1]) ** 2 + ((cz + 0.5 - c[2]) / r[2]) ** 2 <= 1.0
    xs, ys, zs = ((np.arange(k) + s) >> 3 for k, s in zip(n, shift))
    hx = (np.arange(nx, dtype=np.uint32) * np.uint32(73856093))[None, None, :]
    hy = (np.arange(ny, dtype=np.uint32) * np.uint32(19349663))[None, :, None]
    dens = np.empty(nx * ny * nz, dtype=np.float32)
    d = dens.reshape(nz, ny, nx)
    for z0 in range(0, nz, 8):
        z1 = min(z0 + 8, nz)
        hz = (np.arange(z0, z1, dtype=np.uint32) * np.uint32(83492791))[:, None, None]
        h = hx ^ hy ^ hz
        h ^= h >> np.uint32(13)
        h *= np.uint32(0x5bd1e995)
        v = ((h >> np.uint32(8)) & np.uint32(0xffff)).astype(np.float32)
        v *= np.float32(1.2 / 65536)
        v += np.float32(0.05)
        m = mask[zs[z0:z1]][:, ys][:, :, xs]
        v[~m] = 0
        d[z0:z1] = v
    return dens
