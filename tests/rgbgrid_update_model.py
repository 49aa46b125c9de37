"""NumPy model of the device image of one RGB grid ("RGB octets") -- inputs and expected values only, no device, no
library.  Written from the layout's description, not from the builders (csrc/vspg_scene_build.hip build_rgb_octets on the host,
csrc/vspg_rgb_update_kernels.h k_rgb_octet_build on the device), which are both held to it in every bit:

  * a grid of nx x ny x nz RGB voxels has an octet per base voxel (ix, iy, iz) in [-1, n - 1]^3: the eight voxels
    (ix + dx, iy + dy, iz + dz), corner number dx + 2 dy + 4 dz, each as R, G, B, 0; a voxel outside the grid is 0 0 0 0;
  * octet o = i + 1 in [0, n] lives in brick o >> 3 per axis at position o & 7; bn = (n + 8) / 8 bricks per axis, every brick stored,
    brick number (bz bny + by) bnx + bx, octets in a brick x fastest; the octets of a brick behind o = n are zero.

The majorant grid's model is tests/rgbgrid_model.py's (majorant32), re-exported: the update is held to the statement create is held to."""
import numpy as np

from rgbgrid_model import RgbGrid, axis_ranges, coloured, majorant32, point_batch32, probe_points  # noqa: F401  (re-exports)

f32 = np.float32


def brick_counts(n):
    return tuple((v + 8) // 8 for v in n)


def octets32(grid, n):
    """[bnz, bny, bnx, 8, 8, 8, 8, 4] float32 (brick z, y, x; octet z, y, x in the brick; corner; R G B 0) of grid [nz, ny, nx, 3]."""
    nx, ny, nz = n
    grid = np.asarray(grid, dtype=f32).reshape(nz, ny, nx, 3)
    bnx, bny, bnz = brick_counts(n)
    # the voxels -1 .. 8 bn - 1 per axis, zero outside the grid: index v + 1
    pad = np.zeros((8 * bnz + 1, 8 * bny + 1, 8 * bnx + 1, 4), dtype=f32)
    pad[1:nz + 1, 1:ny + 1, 1:nx + 1, :3] = grid
    img = np.zeros((8 * bnz, 8 * bny, 8 * bnx, 8, 4), dtype=f32)   # octet (oz, oy, ox), corner, channel
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
        # octet o has base voxel o - 1: corner voxel o - 1 + d, padded index o + d
        img[:, :, :, c, :] = pad[dz:dz + 8 * bnz, dy:dy + 8 * bny, dx:dx + 8 * bnx]
    img[nz + 1:] = 0   # octets behind o = n hold nothing
    img[:, ny + 1:] = 0
    img[:, :, nx + 1:] = 0
    img = img.reshape(bnz, 8, bny, 8, bnx, 8, 8, 4).transpose(0, 2, 4, 1, 3, 5, 6, 7)
    return np.ascontiguousarray(img)


def special_values(n, seed, hi=2.0):
    """coloured()-style random RGB [nz, ny, nx, 3] plus a zero slab (the last fifth in z), a zero block and one voxel far above the
    rest, whose majorant cells are decided by that single voxel."""
    nx, ny, nz = n
    rng = np.random.default_rng(1000 + seed)
    v = coloured(n, seed, hi=hi)
    v[nz - max(nz // 5, 1):] = 0
    z0, y0, x0 = (int(rng.integers(0, max(k // 2, 1))) for k in (nz, ny, nx))
    v[z0:z0 + max(nz // 3, 1), y0:y0 + max(ny // 3, 1), x0:x0 + max(nx // 3, 1)] = 0
    pz, py, px = (int(rng.integers(0, k)) for k in (max(nz - max(nz // 5, 1), 1), ny, nx))
    v[pz, py, px] = (f32(37.5), f32(0.25), f32(3.0)) if seed % 2 else (f32(0.5), f32(1.0), f32(41.25))
    return v
