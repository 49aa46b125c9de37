"""A model of the image infinite light, written from the reference's text (not a port of the device code):

  * a FLOAT32 MIRROR of what the device evaluates -- EqualAreaSquareToSphere / EqualAreaSphereToSquare (util/math.cpp:292-361), the
    octahedral remap (util/image.h:100-125), Image::GetSamplingDistribution (:450-469), the compensated function
    (lights.cpp:1104-1110), PiecewiseConstant1D / 2D with their sequential float sums (util/sampling.h:625-779), ImageInfiniteLight's
    Le / SampleLi / PDF_Li (lights.h:643-687, lights.cpp:1113-1123) and the rotation.  Every operation is one IEEE float32 operation in
    the reference's order; fmaf, sinf and cosf are the C library's, through ctypes (tests/test_libm_model.py holds the device's sinf /
    cosf to them).  tests/test_envlight_gpu.py compares the device with this mirror bit for bit.
  * a FLOAT64 STATEMENT of the mathematics: the exact equal-area map with atan, the exact integrals of the step function.

The planted errors of tests/test_envlight_model.py are switches of the mirror (`plant`)."""
import ctypes
import ctypes.util
import math

import numpy as np

f32 = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n, _k in (("fmaf", 3), ("sinf", 1), ("cosf", 1)):
    getattr(_libm, _n).restype = ctypes.c_float
    getattr(_libm, _n).argtypes = [ctypes.c_float] * _k


def _map(fn, *arrs):
    arrs = [np.asarray(a, dtype=f32).reshape(-1) for a in arrs]
    return np.array([fn(*[float(a[i]) for a in arrs]) for i in range(arrs[0].shape[0])], dtype=f32)


def fmaf(a, b, c):
    a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
    return _map(_libm.fmaf, a, b, c)


def sinf(x):
    return _map(_libm.sinf, x)


def cosf(x):
    return _map(_libm.cosf, x)


PI = f32(3.14159265358979323846)
T_COEF = [f32(x) for x in (0.406758566246788489601959989e-5, 0.636226545274016134946890922156, 0.61572017898280213493197203466e-2,
                           -0.247333733281268944196501420480, 0.881770664775316294736387951347e-1,
                           0.419038818029165735901852432784e-1, -0.251390972343483509333252996350e-1)]


def _safe_sqrt(x):
    return np.sqrt(np.maximum(f32(0), x), dtype=f32)


# ---------------------------------------------------------------------------------------------------------------------------
# float32 mirror: the two mappings
def sphere_to_square(d):
    """EqualAreaSphereToSquare (util/math.cpp:317-361) on an [n, 3] float32 array -> (u, v)."""
    d = np.asarray(d, f32).reshape(-1, 3)
    x, y, z = np.abs(d[:, 0]), np.abs(d[:, 1]), np.abs(d[:, 2])
    r = _safe_sqrt(f32(1) - z)
    a, b = np.maximum(x, y), np.minimum(x, y)
    with np.errstate(divide="ignore", invalid="ignore"):
        b = np.where(a == 0, f32(0), b / np.where(a == 0, f32(1), a)).astype(f32)
    phi = fmaf(b, T_COEF[6], T_COEF[5])
    for c in T_COEF[4::-1]:
        phi = fmaf(b, phi, c)
    phi = np.where(x < y, f32(1) - phi, phi).astype(f32)
    v = phi * r
    u = r - v
    south = d[:, 2] < 0
    u, v = np.where(south, f32(1) - v, u).astype(f32), np.where(south, f32(1) - u, v).astype(f32)
    u = np.copysign(u, d[:, 0])
    v = np.copysign(v, d[:, 1])
    return (f32(0.5) * (u + f32(1))).astype(f32), (f32(0.5) * (v + f32(1))).astype(f32)


def square_to_sphere(px, py):
    """EqualAreaSquareToSphere (util/math.cpp:292-314) -> [n, 3]."""
    px, py = np.asarray(px, f32).reshape(-1), np.asarray(py, f32).reshape(-1)
    u, v = f32(2) * px - f32(1), f32(2) * py - f32(1)
    up, vp = np.abs(u), np.abs(v)
    sd = f32(1) - (up + vp)
    dd = np.abs(sd)
    r = f32(1) - dd
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(r == 0, f32(1), (vp - up) / np.where(r == 0, f32(1), r) + f32(1)).astype(f32)
    phi = q * PI / f32(4)
    z = np.copysign(f32(1) - r * r, sd)
    c = np.copysign(cosf(phi), u)
    s = np.copysign(sinf(phi), v)
    k = _safe_sqrt(f32(2) - r * r)
    return np.stack([c * r * k, s * r * k, z], axis=1).astype(f32)


def remap(px, py, res, plant=()):
    """RemapPixelCoords under WrapMode::OctahedralSphere (util/image.h:100-125) on integer arrays."""
    px, py = px.astype(np.int64).copy(), py.astype(np.int64).copy()
    flip = () if "no_v_flip" in plant else (1,)
    lo, hi = px < 0, px >= res
    py = np.where((lo | hi) & bool(flip), res - 1 - py, py)
    px = np.where(lo, -px, np.where(hi, 2 * res - 1 - px, px))
    lo, hi = py < 0, py >= res
    px = np.where(lo | hi, res - 1 - px, px)
    py = np.where(lo, -py, np.where(hi, 2 * res - 1 - py, py))
    if res == 1:
        px[:] = 0
        py[:] = 0
    return px, py


# ---------------------------------------------------------------------------------------------------------------------------
# float32 mirror: the distribution
def build_1d(func):
    """PiecewiseConstant1D over [0, 1] (util/sampling.h:625-649): (|func|, cdf[n + 1], funcInt), sequential float sums."""
    func = np.abs(np.asarray(func, f32))
    n = func.shape[0]
    cdf = np.zeros(n + 1, f32)
    step = (func * (f32(1) - f32(0)) / f32(n)).astype(f32)
    for i in range(1, n + 1):
        cdf[i] = cdf[i - 1] + step[i - 1]
    func_int = cdf[n]
    if func_int == 0:
        for i in range(1, n + 1):
            cdf[i] = f32(i) / f32(n)
    else:
        cdf[1:] = cdf[1:] / func_int
    return func, cdf, f32(func_int)


def sampling_function(image, compensated=True):
    """Image::GetSamplingDistribution with dxdA = 1 (util/image.h:205-210, 450-469), then lights.cpp:1104-1110."""
    img = np.asarray(image, f32)
    s = (f32(0) + img[..., 0]).astype(f32)
    s = (s + img[..., 1]).astype(f32)
    s = (s + img[..., 2]).astype(f32)
    d = (s / f32(3)).astype(f32)
    if not compensated:
        return d
    acc = 0.0
    for v in d.reshape(-1):      # std::accumulate(d.begin(), d.end(), 0.)
        acc += float(v)
    average = f32(acc / d.size)        # `Float average`: the double quotient rounded to float once
    d = np.maximum((d - average).astype(f32), f32(0))      # `v - average`: a float subtraction
    if np.all(d == 0):
        d = np.ones_like(d)
    return d


def find_interval(cdf, u):
    """FindInterval(size, cdf[i] <= u) (util/math.h:508-519) for one u."""
    sz = cdf.shape[0]
    size, first = sz - 2, 1
    while size > 0:
        half = size >> 1
        middle = first + half
        if cdf[middle] <= u:
            first, size = middle + 1, size - (half + 1)
        else:
            size = half
    return min(max(first - 1, 0), sz - 2)


def sample_1d(func, cdf, func_int, u):
    """PiecewiseConstant1D::Sample (util/sampling.h:657-675) for one u -> (x, pdf, offset)."""
    u = f32(u)
    n = func.shape[0]
    o = find_interval(cdf, u)
    du = f32(u - cdf[o])
    w = f32(cdf[o + 1] - cdf[o])
    if w > 0:
        du = f32(du / w)
    pdf = f32(func[o] / func_int) if func_int > 0 else f32(0)
    x = f32(f32(f32(o) + du) / f32(n))
    return f32(f32(f32(1) - x) * f32(0) + x * f32(1)), pdf, o      # Lerp(x, min, max)


def mat3_and_inverse(m34):
    """Linear part of a 3 x 4 render_from_light and its inverse as include/vspg.h states it: cofactors over the determinant in
    double, each entry rounded to float once.  None -> identity.  Raises ValueError for a singular / non-finite matrix."""
    s = np.eye(3, 4, dtype=f32) if m34 is None else np.asarray(m34, f32).reshape(3, 4)
    m = s[:, :3].copy()
    if not np.all(np.isfinite(m)):
        raise ValueError("not finite")
    a, b, c, d, e, f, g, h, i = [float(x) for x in m.reshape(-1)]
    c00, c01, c02 = e * i - f * h, f * g - d * i, d * h - e * g
    det = (a * c00 + b * c01) + c * c02
    if det == 0 or not math.isfinite(det):
        raise ValueError("singular")
    adj = [c00, c * h - b * i, b * f - c * e, c01, a * i - c * g, c * d - a * f, c02, b * g - a * h, a * e - b * d]
    mi = np.array([x / det for x in adj], dtype=np.float64).astype(f32).reshape(3, 3)
    if not np.all(np.isfinite(mi)):
        raise ValueError("singular")
    return m, mi


def xform(m, v):
    v = np.asarray(v, f32).reshape(-1, 3)
    return np.stack([((m[r, 0] * v[:, 0]).astype(f32) + m[r, 1] * v[:, 1]).astype(f32) + m[r, 2] * v[:, 2] for r in range(3)],
                    axis=1).astype(f32)


def normalize(v):
    l = np.sqrt(((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]).astype(f32) + v[:, 2] * v[:, 2]).astype(f32), dtype=f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (v / l[:, None]).astype(f32)


class EnvLight:
    """ImageInfiniteLight of the RGB build, allowIncompletePDF = true.  image: [res, res, 3] float32, top row first; L: the RGB
    multiplier; m34: render_from_light (3 x 4) or None.  plant: a set of planted errors --
    'no_4pi', 'uncompensated', 'swap_variates', 'no_v_flip', 'normalize_in_pdf'."""

    def __init__(self, image, L=(1, 1, 1), m34=None, scene_radius=0.0, plant=()):
        self.plant = frozenset(plant)
        self.image = np.ascontiguousarray(image, f32)
        assert self.image.ndim == 3 and self.image.shape[0] == self.image.shape[1] and self.image.shape[2] == 3
        self.res = self.image.shape[0]
        self.L = np.asarray(L, f32)
        self.m, self.mi = mat3_and_inverse(m34)
        self.scene_radius = f32(scene_radius)
        d = sampling_function(self.image, compensated="uncompensated" not in self.plant)
        self.func = np.zeros((self.res, self.res), f32)
        self.cdf = np.zeros((self.res, self.res + 1), f32)
        row_int = np.zeros(self.res, f32)
        for v in range(self.res):
            self.func[v], self.cdf[v], row_int[v] = build_1d(d[v])
        self.mfunc, self.mcdf, self.integral = build_1d(row_int)
        self.four_pi = f32(1) if "no_4pi" in self.plant else f32(f32(4) * PI)

    def image_le(self, u, v):
        res = self.res
        px = np.trunc(np.asarray(u, f32) * f32(res)).astype(np.int64)
        py = np.trunc(np.asarray(v, f32) * f32(res)).astype(np.int64)
        px, py = remap(px, py, res, self.plant)
        rgb = np.maximum(f32(0), self.image[py, px])
        return (rgb * self.L[None, :]).astype(f32)

    def Le(self, dirs):
        w = normalize(xform(self.mi, dirs))
        u, v = sphere_to_square(w)
        return self.image_le(u, v), np.stack([u, v], axis=1)

    def pdf_uv(self, u, v):
        res = self.res
        iu = np.clip(np.trunc(np.asarray(u, f32) * f32(res)).astype(np.int64), 0, res - 1)
        iv = np.clip(np.trunc(np.asarray(v, f32) * f32(res)).astype(np.int64), 0, res - 1)
        return (self.func[iv, iu] / self.integral).astype(f32)

    def pdf_li(self, dirs):
        w = xform(self.mi, dirs)
        if "normalize_in_pdf" in self.plant:
            w = normalize(w)
        u, v = sphere_to_square(w)
        return (self.pdf_uv(u, v) / self.four_pi).astype(f32)

    def sample_uv(self, u):
        """PiecewiseConstant2D::Sample (util/sampling.h:760-770) -> (uv [n, 2], mapPDF [n], offsets [n, 2])."""
        u = np.asarray(u, f32).reshape(-1, 2)
        if "swap_variates" in self.plant:
            u = u[:, ::-1]
        n = u.shape[0]
        uv, pdf, off = np.zeros((n, 2), f32), np.zeros(n, f32), np.zeros((n, 2), np.int64)
        for i in range(n):
            d1, p1, o1 = sample_1d(self.mfunc, self.mcdf, self.integral, u[i, 1])
            d0, p0, o0 = sample_1d(self.func[o1], self.cdf[o1], self.mfunc[o1], u[i, 0])
            uv[i], pdf[i], off[i] = (d0, d1), f32(p0 * p1), (o0, o1)
        return uv, pdf, off

    def sample_li(self, u, ctxp=(0, 0, 0)):
        """-> valid [n] bool, uv [n, 2], wi [n, 3], pdf [n], L [n, 3], pLight [n, 3]; rows without a sample are zero."""
        uv, map_pdf, _ = self.sample_uv(u)
        valid = map_pdf != 0
        w = square_to_sphere(uv[:, 0], uv[:, 1])
        wi = xform(self.m, w)
        pdf = (map_pdf / self.four_pi).astype(f32)
        L = self.image_le(uv[:, 0], uv[:, 1])
        p = (np.asarray(ctxp, f32)[None, :] + wi * f32(f32(2) * self.scene_radius)).astype(f32)
        z = ~valid
        for a in (uv, wi, L, p):
            a[z] = 0
        pdf[z] = 0
        return valid, uv, wi, pdf, L, p

    def batch(self, dirs, u):
        """What Renderer.envlight_batch returns: [n, 16]."""
        le, uv = self.Le(dirs)
        valid, suv, wi, pdf, L, _ = self.sample_li(u)
        return np.concatenate([le, uv, self.pdf_li(dirs)[:, None], valid.astype(f32)[:, None], suv, wi, pdf[:, None], L], axis=1).astype(f32)

    def phi(self, scene_radius):
        """ImageInfiniteLight::Phi per channel in the reference's order (lights.cpp:1127-1141): the clamped texels summed in float in
        image order, then 4 * Pi * Pi * Sqr(sceneRadius) * scale * sumL / (width * height)."""
        s = np.zeros(3, f32)
        for t in np.maximum(f32(0), self.image.reshape(-1, 3)):
            s = (s + t).astype(f32)
        r = f32(scene_radius)
        k = f32(f32(f32(4) * PI) * PI) * f32(r * r)
        return ((k * self.L).astype(f32) * s).astype(f32) / f32(self.res * self.res)


# ---------------------------------------------------------------------------------------------------------------------------
# float64 statement of the mathematics
def sphere_to_square_exact(d):
    """The equal-area octahedral map (Clarberg 2008) with atan, in float64: [n, 3] unit vectors -> [n, 2] in [0, 1]^2."""
    d = np.asarray(d, np.float64).reshape(-1, 3)
    x, y, z = np.abs(d[:, 0]), np.abs(d[:, 1]), np.abs(d[:, 2])
    r = np.sqrt(np.maximum(0.0, 1.0 - z))
    phi = np.arctan2(y, x) * (2.0 / np.pi)      # in [0, 1]; atan2(0, 0) = 0
    v = phi * r
    u = r - v
    south = d[:, 2] < 0
    u, v = np.where(south, 1.0 - v, u), np.where(south, 1.0 - u, v)
    u = np.copysign(u, d[:, 0])
    v = np.copysign(v, d[:, 1])
    return np.stack([0.5 * (u + 1.0), 0.5 * (v + 1.0)], axis=1)


def square_to_sphere_exact(uv):
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    u, v = 2.0 * uv[:, 0] - 1.0, 2.0 * uv[:, 1] - 1.0
    up, vp = np.abs(u), np.abs(v)
    sd = 1.0 - (up + vp)
    r = 1.0 - np.abs(sd)
    phi = np.where(r == 0, 1.0, (vp - up) / np.where(r == 0, 1.0, r) + 1.0) * (np.pi / 4.0)
    z = np.copysign(1.0 - r * r, sd)
    k = r * np.sqrt(np.maximum(0.0, 2.0 - r * r))
    return np.stack([np.copysign(np.cos(phi), u) * k, np.copysign(np.sin(phi), v) * k, z], axis=1)


def pdf_exact(func):
    """The normalised step function over the unit square in float64: func / (its exact integral)."""
    f = np.abs(np.asarray(func, np.float64))
    return f / (f.sum() / f.size)


def expected_radiance_exact(image, L):
    """The mean of Le over the sphere in float64 (an equal-area map: the plain mean of the clamped texels) times L."""
    return np.maximum(0.0, np.asarray(image, np.float64)).reshape(-1, 3).mean(axis=0) * np.asarray(L, np.float64)


# ---------------------------------------------------------------------------------------------------------------------------
# fixtures shared by the CPU and the GPU tests
def make_image(kind, res, seed, peak=1e3):
    """'peaked': a seeded positive image with one texel `peak` (1e3) times the rest; 'banded': the same with every other row zero (res >= 2)
    -- the funcInt == 0 rows --; 'equal': all texels equal -- the fill-with-ones branch."""
    rng = np.random.default_rng(seed)
    if kind == "equal":
        return np.full((res, res, 3), f32(0.75), f32)
    img = rng.uniform(0.2, 1.0, (res, res, 3)).astype(f32)
    if kind == "banded" and res >= 2:
        img[1::2] = 0
    py, px = (int(rng.integers(0, res)), int(rng.integers(0, res)))
    if kind == "banded":
        py -= py % 2
    img[py, px] = img[py, px] * f32(peak)
    return img


def rounded_average_image():
    """A 2 x 2 grey image whose mean is not a float: d = [[1, 1], [1 + 2^-22, 1 + 2^-21]] (each the exact float average of its three equal
    channels), sum 4 + 3 * 2^-22, mean 1 + 3 * 2^-24 -- halfway between the floats 1 + 2^-23 and 1 + 2^-22.  `Float average`
    (lights.cpp:1105) rounds it to the even one, 1 + 2^-22, and `v - average` is a float subtraction: the compensated function is
    [[0, 0], [0, 2^-22]].  Keeping the average in double instead gives [[0, 0], [2^-24, 5 * 2^-24]]: another texel becomes samplable."""
    e = f32(2.0 ** -22)
    d = np.array([[1, 1], [f32(1) + e, f32(1) + f32(2) * e]], f32)
    return np.repeat(d[..., None], 3, axis=2).copy()


UNBIASED_PEAK = 30      # the sky of the GPU unbiasedness test: chosen by tests/test_envlight_model.py::test_planted_errors_shift_...


def unbiased_sky():
    return make_image("peaked", 16, 11, peak=UNBIASED_PEAK)


def make_queries(light, n, seed):
    """n (direction, variate) queries for `light`: seeded unit directions in all octants and seeded variates, with the exact cases in
    front -- the six axis directions (the poles: r == 0, a == 0), x == y, and the directions that give u or v of EXACTLY 0 or 1 and the
    wrap that follows.  Those are not +-x and +-y with z = 0: the polynomial's value at b = 0 is t1 = 4.07e-6, not 0, so +x maps to
    u = 1 - 4.07e-6 / 2.  They are the south pole (u = v = 1; with a negative zero in x or y, 0) and the directions next to it along
    an axis, where 1 - phi * r rounds to 1: (+-1e-3, 0, -0.9999995) gives u == 1 / u == 0 with v = 0.99965, the same in y gives v.
    And variates exactly on CDF entries (0, entries of the marginal and of the first sampled rows, 1 - ulp, 1)."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    u = rng.random((n, 2)).astype(f32)
    exact = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0, 0, 0.5), (0.6, 0.6, 0.52915026), (0.6, 0.8, 0.0),
             (-0.8, 0.6, -0.0), (1, 0, -0.0), (0, 1, -0.0), (-0.0, 0, -1), (0, -0.0, -1), (-0.0, -0.0, -1),
             (1e-3, 0, -0.9999995), (-1e-3, 0, -0.9999995), (0, 1e-3, -0.9999995), (0, -1e-3, -0.9999995)]
    d[:len(exact)] = np.asarray(exact, f32)
    k = 0
    edges = [f32(0), f32(np.nextafter(f32(1), f32(0)))] + [c for c in light.mcdf[1:-1][:8]]
    rows = [v for v in range(light.res) if light.mfunc[v] > 0][:2]
    for e in edges:                      # marginal variate on an entry, conditional variate free
        u[k, 1] = e
        k += 1
    for v in rows:                       # conditional variate on an entry of row v; the marginal variate picks row v
        lo, hi = light.mcdf[v], light.mcdf[v + 1]
        for c in [f32(0)] + [c for c in light.cdf[v][1:-1][:6]]:
            u[k] = (c, f32(lo + (hi - lo) * f32(0.5)))
            k += 1
    # a variate of exactly 1 (outside [0, 1), but the guard `cdf[o + 1] - cdf[o] > 0` exists for it): behind trailing zero entries the
    # last interval has no width
    u[k] = (f32(0.3), f32(1))
    u[k + 1] = (f32(1), u[k + 1, 1])
    return d, u
