"""Point and spot lights restated from the reference's text (src/pbrt/lights.h:203-263, 811-873; lights.cpp:196-248, 1425-1555;
util/math.h:268-274 SmoothStep; util/vecmath.h:1007-1013 CoordinateSystem, :1867-1871 Frame::FromZ; util/transform.h:310-319, 401-406).

Two statements of the same mathematics:
  * a float32 NumPy MIRROR -- one rounding per operation, in the reference's order of operations; what the device computes bit for bit
    (tests/test_pointlight_gpu.py) and what vspg_spot_light_look_at / vspg_point_light_at compute on the host;
  * a float64 STATEMENT (suffix 64) of what those operations mean, against which the mirror's rounding error is bounded.
libm results that must equal the host's bit for bit (cosf, acosf, atanhf, coshf) come from the running libm itself, through ctypes.

`planted` names a deliberate error, for the tests that show each of them is caught:
  swap_cos   cosFalloffStart and cosFalloffEnd swapped        plus_wi   wi instead of -wi into ApplyInverse
  use_m      m instead of mInv                                linear    linear instead of smooth falloff
  no_d2      the division by the squared distance is missing
"""
import ctypes as C
import ctypes.util
import math
from fractions import Fraction

import numpy as np

f32 = np.float32
PI = f32(3.14159265358979323846)
LIGHT_POINT, LIGHT_SPOT = 3, 4
PLANTED = ("swap_cos", "plus_wi", "use_m", "linear", "no_d2")

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("cosf", "acosf", "atanhf", "coshf"):
    getattr(_libm, _n).restype = C.c_float
    getattr(_libm, _n).argtypes = [C.c_float]


def cosf(x):
    return f32(_libm.cosf(float(f32(x))))


def acosf(x):
    return f32(_libm.acosf(float(f32(x))))


# ---- exact float32 fused multiply-add (SquareMatrix's products accumulate by FMA) ------------------------------------------------
def _round_f32(q):
    """The float32 nearest the rational q, ties to even."""
    if q == 0:
        return f32(0)
    c = f32(float(q))  # double rounding may be off by one float32 ulp: look at the neighbours
    best = None
    for cand in (np.nextafter(c, f32(-np.inf)), c, np.nextafter(c, f32(np.inf))):
        err = abs(Fraction(float(cand)) - q)
        even = (int(np.array(cand, f32).view(np.uint32)) & 1) == 0
        key = (err, 0 if even else 1)
        if best is None or key < best[0]:
            best = (key, cand)
    return f32(best[1])


def fma32(a, b, c):
    a, b, c = float(f32(a)), float(f32(b)), float(f32(c))
    q = Fraction(a) * Fraction(b) + Fraction(c)
    if q == 0:  # the sign of an exact zero sum: +0 unless both addends are -0
        prod_neg = math.copysign(1.0, a) * math.copysign(1.0, b) < 0
        return f32(-0.0) if (prod_neg and math.copysign(1.0, c) < 0) else f32(0.0)
    return _round_f32(q)


def mat4_mul(a, b):
    a, b = np.asarray(a, f32).reshape(4, 4), np.asarray(b, f32).reshape(4, 4)
    r = np.zeros((4, 4), f32)
    for i in range(4):
        for j in range(4):
            s = f32(0)
            for k in range(4):
                s = fma32(a[i, k], b[k, j], s)
            r[i, j] = s
    return r


def translate(v):
    m = np.eye(4, dtype=f32)
    m[:3, 3] = np.asarray(v, f32)
    return m


def transform_inverse(m):
    """vspg_transform_inverse: the affine inverse by cofactors in double, rounded once."""
    m = np.asarray(m, f32).reshape(4, 4).astype(np.float64)
    a, b, c, d, e, f, g, h, i = m[0, 0], m[0, 1], m[0, 2], m[1, 0], m[1, 1], m[1, 2], m[2, 0], m[2, 1], m[2, 2]
    A, B, Cc = e * i - f * h, -(d * i - f * g), d * h - e * g
    det = a * A + b * B + c * Cc
    r = np.array([[A / det, -(b * i - c * h) / det, (b * f - c * e) / det], [B / det, (a * i - c * g) / det, -(a * f - c * d) / det],
                  [Cc / det, -(a * h - b * g) / det, (a * e - b * d) / det]])
    t = m[:3, 3]
    inv = np.zeros((4, 4), f32)
    inv[:3, :3] = r.astype(f32)
    for row in range(3):
        inv[row, 3] = f32(-(r[row, 0] * t[0] + r[row, 1] * t[1] + r[row, 2] * t[2]))
    inv[3, 3] = 1
    return inv


def normalize32(v):
    v = np.asarray(v, f32)
    l = np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])
    return v / l[..., None]


def frame_from_z(z):
    """Frame::FromZ: CoordinateSystem (vecmath.h:1007-1013), rows x, y, z of Transform(Frame)."""
    z = np.asarray(z, f32)
    sign = f32(math.copysign(1.0, float(z[2])))
    a = f32(-1) / (sign + z[2])
    b = z[0] * z[1] * a
    x = np.array([f32(1) + sign * (z[0] * z[0]) * a, sign * b, -sign * z[0]], f32)
    y = np.array([b, sign + (z[1] * z[1]) * a, -z[1]], f32)
    return x, y


def compose(ctm, t, t_inv):
    if ctm is None:
        return t, t_inv
    ctm = np.asarray(ctm, f32).reshape(4, 4)
    return mat4_mul(ctm, t), mat4_mul(t_inv, transform_inverse(ctm))


def point_transform(from_, ctm=None):
    """PointLight::Create (lights.cpp:240-242): ctm * Translate(from), and the inverse."""
    fr = np.asarray(from_, f32)
    return compose(ctm, translate(fr), translate(-fr))


def spot_transform(from_, to, ctm=None):
    """SpotLight::Create (lights.cpp:1531-1536): ctm * Translate(from) * Inverse(Frame::FromZ(Normalize(to - from)))."""
    fr, to = np.asarray(from_, f32), np.asarray(to, f32)
    z = normalize32(to - fr)
    x, y = frame_from_z(z)
    f = np.eye(4, dtype=f32)
    f[0, :3], f[1, :3], f[2, :3] = x, y, z
    fi = transform_inverse(f)
    return compose(ctm, mat4_mul(translate(fr), fi), mat4_mul(f, translate(-fr)))


def rotate(theta_deg, axis):
    """Rotate(theta, axis) (transform.h:220-247) in float32, for CTMs."""
    a = normalize32(np.asarray(axis, f32))
    rad = (PI / f32(180)) * f32(theta_deg)
    s, c = f32(math.sin(float(rad))), f32(math.cos(float(rad)))
    x, y, z = a
    m = np.eye(4, dtype=f32)
    m[0, :3] = [x * x + (1 - x * x) * c, x * y * (1 - c) - z * s, x * z * (1 - c) + y * s]
    m[1, :3] = [x * y * (1 - c) + z * s, y * y + (1 - y * y) * c, y * z * (1 - c) - x * s]
    m[2, :3] = [x * z * (1 - c) - y * s, y * z * (1 - c) + x * s, z * z + (1 - z * z) * c]
    return m


def smooth_step(x, a, b, linear=False):
    """SmoothStep (util/math.h:268-274), float32."""
    x = np.asarray(x, f32)
    if a == b:
        return np.where(x < a, f32(0), f32(1)).astype(f32)
    t = np.clip((x - f32(a)) / (f32(b) - f32(a)), f32(0), f32(1)).astype(f32)
    if linear:
        return t
    return (t * t) * (f32(3) - f32(2) * t)


class Light:
    """A point or spot light as the library holds it: I = scale * I multiplied out, both matrices, the constructor's cosines."""

    def __init__(self, kind, I, m, mi, cone_angle=30.0, cone_delta=5.0):
        self.kind = kind
        self.I = np.asarray(I, f32)
        self.m, self.mi = np.asarray(m, f32).reshape(4, 4), np.asarray(mi, f32).reshape(4, 4)
        m_ = self.m
        # renderFromLight(Point3f(0, 0, 0)) (transform.h:310-319): the sums as written, then the `wp == 1` test
        q = [((m_[k, 0] * f32(0) + m_[k, 1] * f32(0)) + m_[k, 2] * f32(0)) + m_[k, 3] for k in range(4)]
        self.pos = np.array([q[k] if q[3] == 1 else q[k] / q[3] for k in range(3)], f32)
        self.cos_end = self.cos_start = f32(0)
        self.axis = np.array([0, 0, 1], f32)
        if kind == LIGHT_SPOT:
            rad = PI / f32(180)
            self.cos_end = cosf(rad * f32(cone_angle))                              # lights.cpp:1438
            self.cos_start = cosf(rad * (f32(cone_angle) - f32(cone_delta)))        # :1439, falloffStart = coneangle - conedelta
            w = np.array([(m_[k, 0] * f32(0) + m_[k, 1] * f32(0)) + m_[k, 2] * f32(1) for k in range(3)], f32)
            self.axis = normalize32(w)

    # ---- SampleLi ----
    def sample_li(self, ctx_p, planted=None):
        """(valid, wi, L, pdf, pLight, delta) for contexts ctx_p (n, 3), float32, the reference's order of operations."""
        p = np.asarray(ctx_p, f32).reshape(-1, 3)
        d = self.pos[None, :] - p
        l2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]      # DistanceSquared = LengthSquared(p - ctx.p)
        wi = d / np.sqrt(l2)[:, None]                                       # Normalize: one division per component
        I = np.broadcast_to(self.I, p.shape).astype(f32)
        if self.kind == LIGHT_SPOT:
            w = wi if planted == "plus_wi" else -wi
            M = self.m if planted == "use_m" else self.mi
            v = np.stack([(M[k, 0] * w[:, 0] + M[k, 1] * w[:, 1]) + M[k, 2] * w[:, 2] for k in range(3)], axis=1).astype(f32)
            wl = normalize32(v)
            a, b = (self.cos_start, self.cos_end) if planted == "swap_cos" else (self.cos_end, self.cos_start)
            s = smooth_step(wl[:, 2], a, b, linear=planted == "linear")   # (swapped arguments: the formula as it stands, a reversed ramp)
            I = I * s[:, None]
        L = I if planted == "no_d2" else I / l2[:, None]
        valid = np.ones(len(p), bool) if self.kind == LIGHT_POINT else np.any(L != 0, axis=1)     # `if (!Li) return {}`
        return valid, wi.astype(f32), L.astype(f32), np.ones(len(p), f32), np.broadcast_to(self.pos, p.shape).astype(f32), np.ones(len(p), f32)

    def sample_li64(self, ctx_p, planted=None):
        """The float64 statement: L = I(w) / |pos - p|^2, wi = (pos - p) / |pos - p|, falloff by the angle to the axis."""
        p = np.asarray(ctx_p, np.float64).reshape(-1, 3)
        pos = self.m[:3, 3].astype(np.float64)
        d = pos[None, :] - p
        l2 = (d * d).sum(axis=1)
        wi = d / np.sqrt(l2)[:, None]
        I = np.broadcast_to(self.I.astype(np.float64), p.shape)
        if self.kind == LIGHT_SPOT:
            M = (self.m if planted == "use_m" else self.mi)[:3, :3].astype(np.float64)
            w = wi if planted == "plus_wi" else -wi
            v = w @ M.T
            cos_t = v[:, 2] / np.sqrt((v * v).sum(axis=1))
            ce, cs = float(self.cos_end), float(self.cos_start)
            if planted == "swap_cos":
                ce, cs = cs, ce
            if ce == cs:
                s = np.where(cos_t < ce, 0.0, 1.0)
            else:
                t = np.clip((cos_t - ce) / (cs - ce), 0.0, 1.0)
                s = t if planted == "linear" else t * t * (3 - 2 * t)
            I = I * s[:, None]
        L = I if planted == "no_d2" else I / l2[:, None]
        return wi, L

    def intensity64(self, w_light):
        """I(w) / I for unit directions in LIGHT space (z = the axis), float64: the smoothstep of cos(theta)."""
        if self.kind == LIGHT_POINT:
            return np.ones(len(w_light))
        ce, cs = float(self.cos_end), float(self.cos_start)
        if ce == cs:
            return np.where(w_light[:, 2] < ce, 0.0, 1.0)
        t = np.clip((w_light[:, 2] - ce) / (cs - ce), 0.0, 1.0)
        return t * t * (3 - 2 * t)

    # ---- Phi / Bounds ----
    def phi(self):
        """PointLight::Phi = 4 Pi scale I (lights.cpp:196-198); SpotLight::Phi (:1452-1455), RGB, float32."""
        if self.kind == LIGHT_POINT:
            return (f32(4) * PI) * self.I
        cone = (f32(1) - self.cos_start) + (self.cos_start - self.cos_end) / f32(2)
        return self.I * f32(2) * PI * cone

    def bounds(self):
        """LightBounds of PointLight::Bounds (lights.cpp:200-205) / SpotLight::Bounds (:1457-1467):
        (p, w, phi, cosTheta_o, cosTheta_e)."""
        mx = f32(max(self.I))
        if self.kind == LIGHT_POINT:
            return self.pos, np.array([0, 0, 1], f32), (f32(4) * PI) * mx, cosf(PI), cosf(PI / f32(2))
        ce = cosf(acosf(self.cos_end) - acosf(self.cos_start))
        if ce == 1 and self.cos_end != self.cos_start:
            ce = f32(0.999)
        return self.pos, self.axis, mx * f32(4) * PI, self.cos_start, ce


def point_light(I, from_, scale=1.0, power=None, ctm=None):
    sc = f32(scale)
    if power is not None and power > 0:
        sc = sc * (f32(power) / (f32(4) * PI))       # lights.cpp:234-238
    m, mi = point_transform(from_, ctm)
    return Light(LIGHT_POINT, np.asarray(I, f32) * sc, m, mi)


def spot_light(I, from_, to, coneangle=30.0, conedelta=5.0, scale=1.0, ctm=None):
    m, mi = spot_transform(from_, to, ctm)
    return Light(LIGHT_SPOT, np.asarray(I, f32) * f32(scale), m, mi, coneangle, conedelta)


# ---- PowerLightSampler (lightsamplers.cpp:76-99): phi = SafeDiv(Phi(lambda), lambda.PDF()).Average() at SampleVisible(0.5) ------------
def wavelength_pdfs():
    out = []
    for i in range(3):
        up = f32(0.5) + f32(i) / f32(3)
        if up > 1:
            up = up - f32(1)
        lam = f32(538) - f32(138.888889) * f32(_libm.atanhf(float(f32(0.85691062) - f32(1.82750197) * up)))
        ch = f32(_libm.coshf(float(f32(0.0072) * (lam - f32(538)))))
        out.append(f32(0) if (lam < 360 or lam > 830) else f32(0.0039398042) / (ch * ch))
    return out


def power_pmf(phis):
    """phis: per light the RGB Phi (float32).  The sampler's pmf: power_i / float(sum in double)."""
    pdf = wavelength_pdfs()
    power = []
    for phi in phis:
        s = f32(0)
        for c in range(3):
            s = s + (f32(phi[c]) / pdf[c] if pdf[c] != 0 else f32(0))
        power.append(s / f32(3))
    total = f32(sum(float(x) for x in power))
    return np.array([x / total for x in power], f32)


# ---- a spot in fog: single scattering by next-event estimation, float64 (tests/test_pointlight_gpu.py, the statistical known answer) ----
class FogSpot:
    """Homogeneous grey medium, one spot light, a pinhole camera, a black backdrop in the plane z = z_wall, maxdepth = 1: a pixel sample is
        int_0^t_wall sigma_s exp(-sigma_t t) p_HG(dot(-d, wi)) I(w) / dist^2 exp(-sigma_t dist) dt
    along its camera ray (o, d), averaged over the pixel's area (box filter).  The scene's numbers live here so that the GPU test and
    the CPU conditions on it read the same ones."""
    sigma_a, sigma_s, g = 0.05, 0.4, 0.3
    I = (3.0, 2.0, 1.0)
    light_from, light_to = (0.0, 1.5, 0.0), (0.0, 0.0, 0.0)
    coneangle, conedelta = 25.0, 8.0
    # The view is what was adjusted on the CPU (tests/test_pointlight_model.py holds the conditions): a narrow look at the EDGE of the
    # cone well below the light, the falloff band crossing the film from left to right.  A view of the whole shaft does not tell a
    # linear falloff from the smooth one -- both integrate to (cosStart - cosEnd) / 2 across the band, the quadrant means moved by 0.04
    # standard errors -- while the right-hand quadrants here see the band's outer half alone, where the two differ by a factor.
    eye, look, up = (0.0, 0.0, -3.0), (1.3, -1.5, 0.0), (0.0, 1.0, 0.0)
    fov = 6.0
    z_wall = 2.0
    W, H, WAVES = 32, 24, 32

    def __init__(self):
        self.light = spot_light(self.I, self.light_from, self.light_to, self.coneangle, self.conedelta)
        self.sigma_t = self.sigma_a + self.sigma_s
        # vspg_camera_look_at: pbrt's LookAt + "perspective", fov across the shorter image axis, raster y down
        e, f, u = (np.array(v, np.float64) for v in (self.eye, np.subtract(self.look, self.eye), self.up))
        f /= np.linalg.norm(f)
        u /= np.linalg.norm(u)
        r = np.cross(u, f)
        r /= np.linalg.norm(r)
        nu = np.cross(f, r)
        aspect = self.W / self.H
        wx, wy = (aspect, 1.0) if aspect > 1 else (1.0, 1.0 / aspect)
        th = math.tan(self.fov * math.pi / 360.0)
        self.cam = (e, r, nu, f, 2 * wx * th / self.W, -wx * th, -2 * wy * th / self.H, wy * th)

    def rays(self, px, py):
        """Unit directions of the camera rays through raster points (px, py)."""
        e, r, nu, f, sx, ox, sy, oy = self.cam
        c = np.stack([sx * px + ox, sy * py + oy, np.ones_like(px)], axis=-1)
        c /= np.linalg.norm(c, axis=-1, keepdims=True)
        return c[..., 0:1] * r + c[..., 1:2] * nu + c[..., 2:3] * f

    def integrand(self, d, t, planted=None):
        """The integrand at distance t (.., n) along directions d (.., 3): RGB (.., n, 3)."""
        p = self.cam[0] + d[..., None, :] * t[..., None]
        wi, L = self.light.sample_li64(p.reshape(-1, 3), planted)
        wi, L = wi.reshape(p.shape), L.reshape(p.shape)
        dist = np.linalg.norm(np.asarray(self.light.m[:3, 3], np.float64) - p, axis=-1)
        cos_t = np.einsum("...k,...nk->...n", -d, wi)
        g = self.g
        hg = (1 - g * g) / (4 * math.pi * (1 + g * g + 2 * g * cos_t) ** 1.5)      # HenyeyGreenstein (util/scattering.h)
        return (self.sigma_s * np.exp(-self.sigma_t * (t + dist)) * hg)[..., None] * L

    def t_wall(self, d):
        return (self.z_wall - self.cam[0][2]) / d[..., 2]

    def pixel_means(self, nsub=4, nt=256, planted=None):
        """(H, W, 3): midpoint rule over nsub x nsub raster points per pixel and nt steps along each ray."""
        sub = (np.arange(nsub) + 0.5) / nsub
        px = (np.arange(self.W)[None, :, None, None] + sub[None, None, None, :]) + np.zeros((self.H, 1, nsub, 1))
        py = (np.arange(self.H)[:, None, None, None] + sub[None, None, :, None]) + np.zeros((1, self.W, 1, nsub))
        d = self.rays(px, py)
        tw = self.t_wall(d)
        t = (np.arange(nt) + 0.5) / nt * tw[..., None]
        v = self.integrand(d, t, planted).sum(axis=-2) * (tw / nt)[..., None]
        return v.mean(axis=(2, 3))

    def quadrant_means(self, img):
        """Means of the (R + G + B) / 3 image over the four film quadrants: top-left, top-right, bottom-left, bottom-right."""
        y = np.asarray(img, np.float64)[..., :3].sum(axis=-1) / 3
        h, w = self.H // 2, self.W // 2
        return np.array([y[:h, :w].mean(), y[:h, w:].mean(), y[h:, :w].mean(), y[h:, w:].mean()])

    def monte_carlo_waves(self, n_waves, seed=1, planted=None):
        """The same estimator by NumPy Monte Carlo, one sample per pixel and wave: a uniform point in the pixel, a free-flight distance
        t ~ sigma_t exp(-sigma_t t); beyond the wall the sample is 0, else sigma_s / sigma_t times the rest of the integrand.  Returns the
        quadrant means per wave (n_waves, 4): their spread sizes the standard error the GPU test will see."""
        rng = np.random.default_rng(seed)
        out = []
        for _ in range(n_waves):
            px = np.arange(self.W)[None, :] + rng.random((self.H, self.W))
            py = np.arange(self.H)[:, None] + rng.random((self.H, self.W))
            d = self.rays(px, py)
            t = -np.log1p(-rng.random((self.H, self.W))) / self.sigma_t
            v = self.integrand(d, t[..., None], planted)[..., 0, :] / (self.sigma_t * np.exp(-self.sigma_t * t))[..., None]
            v = np.where((t < self.t_wall(d))[..., None], v, 0.0)
            out.append(self.quadrant_means(v))
        return np.array(out)

    def min_distance_to_light(self):
        """The smallest distance between the light and any camera ray through the film (its corners and edges bound it)."""
        k = np.linspace(0.0, 1.0, 65)
        px, py = np.meshgrid(k * self.W, k * self.H)
        d = self.rays(px, py)
        v = np.asarray(self.light.m[:3, 3], np.float64) - self.cam[0]
        along = np.clip((d * v).sum(axis=-1), 0.0, self.t_wall(d))
        return float(np.linalg.norm(v - d * along[..., None], axis=-1).min())
