"""NumPy model of RGBGridMedium ("rgbgrid", src/pbrt/media.h:391-467, media.cpp:369-484) in the RGB rendering build: inputs and
expected values only -- no device, no library.

Two statements of the same mathematics:
  *32  a float32 mirror with the reference's operations in the reference's order (np.float32 arrays round after every operation, as
       code built without FMA contraction does): SampledGrid::Lookup(p, convert) (util/containers.h:784-827), SamplePoint
       (media.h:417-441) and the constructor's majorant grid (media.cpp:395-408 with SampledGrid::MaxValue(bounds, convert),
       containers.h:837-854).  The device is held to it bit for bit.
  *64  the same in float64, from the same float32 inputs: what the mirror is held to, inside a bound derived from its operation count.
In the RGB build RGBUnboundedSpectrum / RGBIlluminantSpectrum::Sample(lambda) returns the RGB and MaxValue() its largest component.

`planted` switches one deliberate error on (PLANTED): the CPU tests show that the fixtures tell each of them from the truth."""
import numpy as np

f32 = np.float32
RES = 16
U = 2.0 ** -24   # unit roundoff of float32
PLANTED = ("max_of_sum", "absent_zero", "lerp_diff", "swap_channels", "short_box")


class RgbGrid:
    """sigma_a / sigma_s / Le: float32 [nz, ny, nx, 3] or None; p0, p1: the bounds; m: renderFromMedium (4x4 float32, affine) or None."""

    def __init__(self, sigma_a=None, sigma_s=None, Le=None, p0=(0, 0, 0), p1=(1, 1, 1), g=0.0, scale=1.0, Lescale=1.0, m=None):
        conv = lambda a: None if a is None else np.ascontiguousarray(a, dtype=f32)
        self.sigma_a, self.sigma_s, self.Le = conv(sigma_a), conv(sigma_s), conv(Le)
        first = next(a for a in (self.sigma_a, self.sigma_s, self.Le) if a is not None)
        self.n = (first.shape[2], first.shape[1], first.shape[0])   # nx, ny, nz
        self.p0, self.p1 = np.array(p0, dtype=f32), np.array(p1, dtype=f32)
        self.g, self.scale, self.Lescale = g, f32(scale), f32(Lescale)
        self.m = None if m is None else np.array(m, dtype=f32).reshape(4, 4)
        self.minv = None   # filled from the scene record (the library's vspg_transform_inverse) or by set_inverse

    def set_inverse(self, minv):
        self.minv = np.array(minv, dtype=f32).reshape(4, 4)
        return self


# ---- coordinates ---------------------------------------------------------------------------------------------------------------------
def to_medium32(med, p):
    """Transform::ApplyInverse(Point3f) with an affine matrix: (m0 x + m1 y) + (m2 z + m3) per row, in float32."""
    p = np.asarray(p, dtype=f32).reshape(-1, 3)
    if med.minv is None:
        return p
    a = med.minv
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([(a[r, 0] * x + a[r, 1] * y) + (a[r, 2] * z + a[r, 3]) for r in range(3)], axis=-1).astype(f32)


def offset32(med, pm):
    """Bounds3::Offset (vecmath.h:1323-1332): (p - pMin) / (pMax - pMin) per axis (the bounds have positive extent)."""
    return ((pm - med.p0[None, :]) / (med.p1 - med.p0)[None, :]).astype(f32)


def offset64(med, pm):
    return (pm.astype(np.float64) - med.p0.astype(np.float64)) / (med.p1.astype(np.float64) - med.p0.astype(np.float64))


# ---- Lookup(p, convert) --------------------------------------------------------------------------------------------------------------
def _corners(grid, n, ix, iy, iz, dtype):
    """[m, 8, 3]: the RGB of the eight voxels around base voxel (ix, iy, iz), zero outside the grid, x fastest then y then z."""
    out = []
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                x, y, z = ix + dx, iy + dy, iz + dz
                ok = (x >= 0) & (x < n[0]) & (y >= 0) & (y < n[1]) & (z >= 0) & (z < n[2])
                v = grid[np.where(ok, z, 0), np.where(ok, y, 0), np.where(ok, x, 0)].astype(dtype)
                out.append(np.where(ok[:, None], v, dtype(0)))
    return np.stack(out, axis=1)


def lookup32(grid, n, o, planted=()):
    """SampledGrid::Lookup(Point3f p, convert) at offset-space points o [m, 3], float32, per channel: [m, 3]."""
    o = np.asarray(o, dtype=f32)
    s = [o[:, k] * f32(n[k]) - f32(0.5) for k in range(3)]
    i = [np.floor(v).astype(np.int64) for v in s]
    d = [(v - k.astype(f32))[:, None] for v, k in zip(s, i)]
    c = _corners(grid, n, i[0], i[1], i[2], f32)
    if "swap_channels" in planted:
        c = c[..., ::-1]
    one = f32(1)
    if "lerp_diff" in planted:
        lerp = lambda t, a, b: a + t * (b - a)
    else:
        lerp = lambda t, a, b: (one - t) * a + t * b   # pbrt::Lerp (util/math.h)
    d00, d10 = lerp(d[0], c[:, 0], c[:, 1]), lerp(d[0], c[:, 2], c[:, 3])
    d01, d11 = lerp(d[0], c[:, 4], c[:, 5]), lerp(d[0], c[:, 6], c[:, 7])
    r = lerp(d[2], lerp(d[1], d00, d10), lerp(d[1], d01, d11))
    assert r.dtype == f32
    return r


def lookup64(grid, n, o):
    o = np.asarray(o, dtype=np.float64)
    s = [o[:, k] * n[k] - 0.5 for k in range(3)]
    i = [np.floor(v).astype(np.int64) for v in s]
    d = [(v - k)[:, None] for v, k in zip(s, i)]
    c = _corners(grid, n, i[0], i[1], i[2], np.float64)
    lerp = lambda t, a, b: (1 - t) * a + t * b
    d00, d10 = lerp(d[0], c[:, 0], c[:, 1]), lerp(d[0], c[:, 2], c[:, 3])
    d01, d11 = lerp(d[0], c[:, 4], c[:, 5]), lerp(d[0], c[:, 6], c[:, 7])
    return lerp(d[2], lerp(d[1], d00, d10), lerp(d[1], d01, d11))


# ---- SamplePoint ---------------------------------------------------------------------------------------------------------------------
def sample_point32(med, p, planted=()):
    """(sigma_a, sigma_s, Le), each [m, 3] float32, at render-space points p."""
    o = offset32(med, to_medium32(med, p))
    absent = f32(0) if "absent_zero" in planted else f32(1)
    ones = np.full((len(o), 3), absent, dtype=f32)
    sa = med.scale * (lookup32(med.sigma_a, med.n, o, planted) if med.sigma_a is not None else ones)
    ss = med.scale * (lookup32(med.sigma_s, med.n, o, planted) if med.sigma_s is not None else ones)
    le = np.zeros((len(o), 3), dtype=f32)
    if med.Le is not None and med.Lescale > 0:
        le = med.Lescale * lookup32(med.Le, med.n, o, planted)
    return sa.astype(f32), ss.astype(f32), le.astype(f32)


def sample_point64(med, pm):
    """The same from MEDIUM-space points pm (float32 values, float64 arithmetic)."""
    o = offset64(med, np.asarray(pm, dtype=f32))
    ones = np.ones((len(o), 3))
    sc, ls = float(med.scale), float(med.Lescale)
    sa = sc * (lookup64(med.sigma_a, med.n, o) if med.sigma_a is not None else ones)
    ss = sc * (lookup64(med.sigma_s, med.n, o) if med.sigma_s is not None else ones)
    le = ls * lookup64(med.Le, med.n, o) if med.Le is not None and ls > 0 else np.zeros((len(o), 3))
    return sa, ss, le


def lookup_bound(med, grid):
    """|mirror - statement| of scale * Lookup, per point and channel, for offset coordinates in [-1, 2]: with M the grid's largest value,
      coordinates  o = fl(fl(p - p0) / fl(p1 - p0)): 3 roundings, s = fl(fl(o n) - .5): 2 more, each relative to a magnitude <= 2 n + 1;
                   d = s - floor(s): exact, or one rounding of a value <= 1 below voxel 0   -> |delta d| <= (5 (2 n + 1) + 1) U per axis;
                   the interpolant is continuous across voxel planes and changes by at most M per unit of d along an axis
                                                                                            -> 3 (5 (2 n + 1) + 1) U M;
      arithmetic   three levels of Lerp = fl(fl(fl(1 - t) a) + fl(t b)) on values in [0, M]: 4 roundings a level, and the scale's:
                                                                                            -> 13 U M (first order),
    times the scale, with a factor 1.01 for the second-order terms."""
    M = float(grid.max())
    nmax = max(med.n)
    return 1.01 * abs(float(med.scale)) * M * U * (3 * (5 * (2 * nmax + 1) + 1) + 13)


# ---- the majorant grid ---------------------------------------------------------------------------------------------------------------
def axis_ranges(n, planted=()):
    """Per axis the (lo, hi) sample range of each of the 16 cells: SampledGrid::MaxValue's pi[0], pi[1] (containers.h:839-845) for the
    cell's bounds [c / 16, (c + 1) / 16] (MajorantGrid::VoxelBounds)."""
    out = []
    for nk in n:
        lo, hi = [], []
        for c in range(RES):
            p0, p1 = f32(c) / f32(RES), f32(c + 1) / f32(RES)
            a = int(np.floor(p0 * f32(nk) - f32(0.5)))
            b = int(np.floor(p1 * f32(nk) - f32(0.5))) + (0 if "short_box" in planted else 1)
            lo.append(max(a, 0))
            hi.append(max(min(b, nk - 1), lo[-1]))   # (never below lo in the truth; the planted short box keeps its start voxel)
        out.append((lo, hi))
    return out


def _box_values(v, rx, ry, rz, x, y, z):
    return v[rz[0][z]:rz[1][z] + 1, ry[0][y]:ry[1][y] + 1, rx[0][x]:rx[1][x] + 1]


def majorant32(med, planted=()):
    """[16, 16, 16] float32 (z, y, x): sigmaScale * (MaxValue(sigma_a box) + MaxValue(sigma_s box)), an absent grid counting as 1."""
    rx, ry, rz = axis_ranges(med.n, planted)
    absent = f32(0) if "absent_zero" in planted else f32(1)
    mx = lambda g: None if g is None else g.max(axis=-1)   # convert = RGBUnboundedSpectrum::MaxValue
    a, s = mx(med.sigma_a), mx(med.sigma_s)
    out = np.empty((RES, RES, RES), dtype=f32)
    for z in range(RES):
        for y in range(RES):
            for x in range(RES):
                if "max_of_sum" in planted and a is not None and s is not None:
                    tot = _box_values(med.sigma_a + med.sigma_s, rx, ry, rz, x, y, z).max()
                else:
                    ma = absent if a is None else _box_values(a, rx, ry, rz, x, y, z).max()
                    ms = absent if s is None else _box_values(s, rx, ry, rz, x, y, z).max()
                    tot = f32(ma) + f32(ms)
                out[z, y, x] = med.scale * f32(tot)
    return out


def majorant64(med):
    rx, ry, rz = axis_ranges(med.n)
    mx = lambda g: None if g is None else g.max(axis=-1).astype(np.float64)
    a, s = mx(med.sigma_a), mx(med.sigma_s)
    out = np.empty((RES, RES, RES))
    for z in range(RES):
        for y in range(RES):
            for x in range(RES):
                ma = 1.0 if a is None else _box_values(a, rx, ry, rz, x, y, z).max()
                ms = 1.0 if s is None else _box_values(s, rx, ry, rz, x, y, z).max()
                out[z, y, x] = float(med.scale) * (ma + ms)
    return out


def majorant_cell32(med, maj, p):
    """The value of the cell that holds each render-space point (0 outside the bounds): the cell the DDA starts in,
    clamp(int(Offset(p) * 16), 0, 15) per axis."""
    o = offset32(med, to_medium32(med, p))
    inside = np.all((o >= 0) & (o <= 1), axis=1)
    c = np.clip((np.where(inside[:, None], o, 0) * f32(RES)).astype(np.int64), 0, RES - 1)
    return np.where(inside, maj[c[:, 2], c[:, 1], c[:, 0]], f32(0)).astype(f32)


def point_batch32(med, p, maj=None):
    """What vspg_medium_point_batch returns: [m, 10]."""
    maj = majorant32(med) if maj is None else maj
    sa, ss, le = sample_point32(med, p)
    return np.concatenate([sa, ss, le, majorant_cell32(med, maj, p)[:, None]], axis=1).astype(f32)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (2, 3, 5), (9, 9, 9), (20, 18, 17)]   # nx, ny, nz: a tent; tiny; across the 8-wide brick edge; more than 16 cells
PLACEMENT = np.array([[0.0, -1.2, 0.0, 0.1], [0.9, 0.0, 0.5, -0.2], [-0.4, 0.0, 1.1, 0.05], [0, 0, 0, 1]], dtype=f32)   # a sheared, scaled frame


def coloured(n, seed, lo=0.0, hi=2.0):
    """[nz, ny, nx, 3] float32: independent channels, a fifth of the voxels empty."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(lo, hi, size=(n[2], n[1], n[0], 3)).astype(f32)
    v[rng.random((n[2], n[1], n[0])) < 0.2] = 0
    return v


def fixtures():
    """name -> RgbGrid.  Every shape with both sigma grids (and an Le grid on two of them); one with only sigma_a, one with only
    sigma_s, one whose sigma_a grid is all zero, one placed by a non-identity affine transform."""
    fx = {}
    for k, n in enumerate(SHAPES):
        name = "both-%dx%dx%d" % n
        fx[name] = RgbGrid(coloured(n, 10 + k), coloured(n, 20 + k, hi=3.0), Le=coloured(n, 30 + k, hi=0.5) if k % 2 else None,
                           p0=(-0.8, -0.7, -0.6), p1=(0.8, 0.9, 0.7), g=0.3, scale=1.5, Lescale=2.0)
    n = (9, 9, 9)
    fx["only-a"] = RgbGrid(sigma_a=coloured(n, 41), p0=(-0.5, -0.5, -0.5), p1=(0.5, 0.5, 0.5), scale=0.75)
    fx["only-s"] = RgbGrid(sigma_s=coloured(n, 42), p0=(-0.5, -0.5, -0.5), p1=(0.5, 0.5, 0.5), scale=2.0)
    fx["zero-a"] = RgbGrid(np.zeros((5, 3, 2, 3), f32), coloured((2, 3, 5), 43), p0=(-0.5, -0.5, -0.5), p1=(0.5, 0.5, 0.5))
    fx["placed"] = RgbGrid(coloured((20, 18, 17), 44), coloured((20, 18, 17), 45), Le=coloured((20, 18, 17), 46, hi=0.5),
                           p0=(-0.6, -0.5, -0.7), p1=(0.7, 0.6, 0.5), scale=1.25, m=PLACEMENT)
    fx["placed"].set_inverse(np.linalg.inv(PLACEMENT.astype(np.float64)))
    return fx


def probe_points(med, n_random=1500, seed=3):
    """Render-space points [m, 3] (m no multiple of 64): random ones inside and around the bounds, points on voxel planes (offset
    coordinate (k + .5) / n), on the bounds' faces and corners, in the half-voxel rim, and outside."""
    rng = np.random.default_rng(seed)
    n = np.array(med.n, dtype=np.float64)
    o = [rng.uniform(-0.3, 1.3, size=(n_random, 3))]
    k = rng.integers(-1, n + 1, size=(400, 3))
    planes = rng.uniform(0, 1, size=(400, 3))
    on = rng.random((400, 3)) < 0.6
    o.append(np.where(on, (k + 0.5) / n, planes))                                            # voxel planes, several axes at once
    faces = rng.uniform(0, 1, size=(300, 3))
    pick = rng.random((300, 3)) < 0.5
    o.append(np.where(pick, rng.integers(0, 2, size=(300, 3)).astype(np.float64), faces))   # faces, edges and corners of the bounds
    rim = rng.uniform(0, 1, size=(300, 3))
    ax = rng.integers(0, 3, size=300)
    side = rng.integers(0, 2, size=300)
    rim[np.arange(300), ax] = np.where(side == 1, 1 - rng.uniform(0, 0.5, 300) / n[ax], rng.uniform(0, 0.5, 300) / n[ax])
    o.append(rim)                                                                            # the half-voxel rim inside the bounds
    o.append(rng.uniform(-3, 4, size=(203, 3)))                                              # well outside
    o.append(np.array([[0.5, 0.5, 0.5], [0, 0, 0], [1, 1, 1]]))
    o = np.concatenate(o)
    pm = med.p0.astype(np.float64) + o * (med.p1.astype(np.float64) - med.p0.astype(np.float64))
    if med.m is not None:
        pm = pm @ med.m[:3, :3].astype(np.float64).T + med.m[:3, 3].astype(np.float64)
    p = pm.astype(f32)
    assert len(p) % 64 != 0
    return p


# ---- the statistical known answer's medium (tests/test_rgbgrid_gpu.py): channels proportional to one density -----------------------------
PROPORTIONAL_A = (0.6, 0.2, 0.05)   # sigma_a = PROPORTIONAL_A d: red absorbs twelve times as much as blue ...
PROPORTIONAL_S = (0.8, 1.6, 3.2)    # ... and scatters a quarter as much: albedo 0.57 / 0.89 / 0.98


# ---- the grey twin: the uniformgrid the oracle pins ----------------------------------------------------------------------------------
def grey_twin(density, n, a, s, k, le=None, le_scale=None, Lescale=1.0, **kw):
    """The rgbgrid with voxels a d_i and s d_i in all three channels and scale k: for a, s, k powers of two it equals the uniformgrid
    with grey sigma_a = a, sigma_s = s, "scale" k and density d in every bit (tests/test_rgbgrid_model.py shows it).
    le, le_scale, Lescale: the emissive pair -- uniformgrid Le = le (RGB, each a power of two) with the LeScale grid le_scale_i
    (density-sized) against rgb Le voxels (le * le_scale_i) / Lescale and "Lescale" Lescale (a power of two)."""
    d = np.asarray(density, dtype=f32).reshape(n[2], n[1], n[0])
    rep = lambda v: np.repeat(v[..., None], 3, axis=-1).astype(f32)
    Le = None
    if le is not None:
        Le = ((np.asarray(le, dtype=f32)[None, None, None, :] * np.asarray(le_scale, dtype=f32).reshape(d.shape)[..., None]) / f32(Lescale)).astype(f32)
    return RgbGrid(rep(f32(a) * d), rep(f32(s) * d), Le=Le, scale=k, Lescale=Lescale, **kw)
