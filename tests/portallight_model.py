"""A model of the portal image infinite light, written from the reference's text (not a port of the device code):

  * a FLOAT32 MIRROR of what the host builder and the device evaluate -- PortalImageInfiniteLight (src/pbrt/lights.h:699-808,
    lights.cpp:1181-1345) over SummedAreaTable / WindowedPiecewiseConstant2D (util/sampling.h:829-983), Image::BilerpChannel and
    GetSamplingDistribution (util/image.h:279-292, 450-469).  Every operation is one IEEE float32 operation in the reference's order;
    Integral's subtraction and quotient are double; fmaf, sinf and cosf are the C library's through tests/envlight_model.py (the
    device's sinf / cosf are held to them by tests/test_libm_model.py).  tan and atan2 are the project's own two functions
    (csrc/vspg_trig.h), restated here operation for operation.  Every Lookup is evaluated in full, the straightforward way: the
    device hoists the loop-invariant half of each bisection step, and the comparison of trip counts and results bit for bit is what
    shows that the hoisting changed nothing.  The bisection carries the device's iteration cap (BISECT_CAP).
  * a FLOAT64 STATEMENT of the mathematics: the exact gnomonic-angle map and its Jacobian, the windowed density as the function over
    its window integral.

The planted errors of tests/test_portallight_model.py are switches of the mirror (`plant`)."""
import math

import numpy as np

from envlight_model import cosf, fmaf, mat3_and_inverse, normalize, remap, sinf, sphere_to_square, xform

f32 = np.float32
PI = f32(3.14159265358979323846)
PI_OVER_2 = f32(1.57079632679489661923)
PI_OVER_4 = f32(0.78539816339744830961)
BISECT_CAP = 40  # kPortalBisectCap (csrc/vspg_portalmap.h)
OUT = 32
WHY_OK, WHY_NO_BOUNDS, WHY_ZERO_WINDOW, WHY_ZERO_COLUMN, WHY_BAD_T, WHY_ZERO_JACOBIAN = range(6)
FLT_MAX = f32(3.402823466e+38)
_ERR = dict(divide="ignore", invalid="ignore", over="ignore")


# ---------------------------------------------------------------------------------------------------------------------------
# float32 mirror: the project's tan and atan2 (csrc/vspg_trig.h)
def tanf(a):
    a = np.asarray(a, f32).reshape(-1)
    with np.errstate(**_ERR):
        return (sinf(a) / cosf(a)).astype(f32)


def atanf(t):
    t = np.asarray(t, f32).reshape(-1)
    a = np.abs(t)
    big = a > f32(2.414213562373095)
    mid = ~big & (a > f32(0.4142135623730950))
    with np.errstate(**_ERR):
        z = np.where(big, f32(-1) / a, np.where(mid, (a - f32(1)) / (a + f32(1)), a)).astype(f32)
    y0 = np.where(big, PI_OVER_2, np.where(mid, PI_OVER_4, f32(0))).astype(f32)
    w = (z * z).astype(f32)
    p = fmaf(w, f32(8.05374449538e-2), f32(-1.38776856032e-1))
    p = fmaf(w, p, f32(1.99777106478e-1))
    p = fmaf(w, p, f32(-3.33329491539e-1))
    r = (y0 + fmaf((p * w).astype(f32), z, z)).astype(f32)
    return np.copysign(r, t).astype(f32)


def atan2f(y, x):
    with np.errstate(**_ERR):
        return atanf((np.asarray(y, f32) / np.asarray(x, f32)).astype(f32))


def _dot(a, b):
    return ((a[:, 0] * b[0]).astype(f32) + a[:, 1] * b[1]).astype(f32) + a[:, 2] * b[2]


def _dop(a, b, c, d):  # DifferenceOfProducts (util/math.h:569-574)
    cd = f32(c * d)
    return f32(fmaf(a, b, -cd)[0] + fmaf(-c, d, cd)[0])


def _cross(v, w):
    return np.array([_dop(v[1], w[2], v[2], w[1]), _dop(v[2], w[0], v[0], w[2]), _dop(v[0], w[1], v[1], w[0])], f32)


def _clamp01(x):
    return np.where(x < f32(0), f32(0), np.where(x > f32(1), f32(1), x)).astype(f32)


def _idx(x, n):
    """portal_idx: the float -> int of a table coordinate; NaN and negatives give 0, n and beyond give n."""
    x = np.asarray(x, f32)
    with np.errstate(invalid="ignore"):
        ok = x >= 0
        inside = ok & (x < f32(n))
        return np.where(inside, np.trunc(np.where(inside, x, 0)).astype(np.int64), np.where(ok, n, 0))


def portal_checks(portal):
    """The constructor's two tests (lights.cpp:1218-1228) plus finite vertices and non-degenerate edges: None, or the reason."""
    q = np.asarray(portal, f32).reshape(4, 3)
    if not np.all(np.isfinite(q)):
        return "not finite"
    e = [q[1] - q[0], q[2] - q[1], q[2] - q[3], q[3] - q[0]]
    if any(not (np.dot(x.astype(np.float64), x.astype(np.float64)) > 0) for x in e):
        return "degenerate"
    p01, p12, p32, p03 = [normalize(x.reshape(1, 3))[0] for x in e]
    d = lambda a, b: float(_dot(a.reshape(1, 3), b)[0])
    if abs(float(f32(d(p01, p32)) - f32(1))) > .001 or abs(float(f32(d(p12, p03)) - f32(1))) > .001:
        return "not parallel"
    if abs(d(p01, p12)) > .001 or abs(d(p12, p32)) > .001 or abs(d(p32, p03)) > .001 or abs(d(p03, p01)) > .001:
        return "not perpendicular"
    return None


class PortalLight:
    """PortalImageInfiniteLight of the RGB build.  image: [res, res, 3] float32 equal-area map, top row first; portal: [4, 3] render
    space; L: the RGB multiplier (scale); m34: render_from_light or None.  plant: a set of planted errors --
    'float_table', 'exclusive_top', 'no_jacobian_in_d', 'portal1', 'multiply_jacobian'."""

    def __init__(self, image, portal, L=(1, 1, 1), m34=None, scene_radius=0.0, plant=()):
        self.plant = frozenset(plant)
        self.src = np.ascontiguousarray(image, f32)
        self.res = res = self.src.shape[0]
        self.L = np.asarray(L, f32)
        self.m, self.mi = mat3_and_inverse(m34)
        self.scene_radius = f32(scene_radius)
        self.portal = q = np.asarray(portal, f32).reshape(4, 3)
        self.fx = normalize((q[3] - q[0]).reshape(1, 3))[0]
        self.fy = normalize((q[1] - q[0]).reshape(1, 3))[0]
        self.fz = _cross(self.fx, self.fy)
        self.p0, self.p2 = q[0], (q[1] if "portal1" in self.plant else q[2])
        ln = lambda v: np.sqrt(f32(f32(f32(v[0] * v[0]) + f32(v[1] * v[1])) + f32(v[2] * v[2])), dtype=f32)
        self.area = f32(ln(q[1] - q[0]) * ln(q[3] - q[0]))
        # the rectified image, d and Phi's sums
        xs = ((np.arange(res, dtype=f32) + f32(0.5)) / f32(res)).astype(f32)
        u, v = np.tile(xs, res), np.repeat(xs, res)
        w, jac = self.render_from_image(u, v)
        self.centre_jac = jac.reshape(res, res)
        ue, ve = sphere_to_square(normalize(xform(self.mi, w)))
        fxp, fyp = (ue * f32(res) - f32(0.5)).astype(f32), (ve * f32(res) - f32(0.5)).astype(f32)
        xi, yi = np.floor(fxp).astype(np.int64), np.floor(fyp).astype(np.int64)
        dx, dy = (fxp - xi.astype(f32)).astype(f32), (fyp - yi.astype(f32)).astype(f32)
        t = []
        for j in range(4):
            px, py = remap(xi + (j & 1), yi + (j >> 1), res)
            t.append(self.src[np.clip(py, 0, res - 1), np.clip(px, 0, res - 1)])
        omx, omy = (f32(1) - dx).astype(f32), (f32(1) - dy).astype(f32)
        k = [(omx * omy).astype(f32), (dx * omy).astype(f32), (omx * dy).astype(f32), (dx * dy).astype(f32)]
        img = (((k[0][:, None] * t[0]).astype(f32) + k[1][:, None] * t[1]).astype(f32) + k[2][:, None] * t[2]).astype(f32) + k[3][:, None] * t[3]
        self.image = img.astype(f32).reshape(res, res, 3)
        avg = ((((f32(0) + img[:, 0]).astype(f32) + img[:, 1]).astype(f32) + img[:, 2]).astype(f32) / f32(3)).astype(f32)
        d = avg if "no_jacobian_in_d" in self.plant else (avg * jac).astype(f32)
        self.func = d.reshape(res, res)
        with np.errstate(**_ERR):
            terms = (np.maximum(f32(0), img) / jac[:, None]).astype(f32)
        s = np.zeros(3, f32)
        for i in range(terms.shape[0]):
            s = (s + terms[i]).astype(f32)
        self.sum_phi = s
        self.table = self._summed_area(self.func)

    def _summed_area(self, func):
        """SummedAreaTable's constructor (util/sampling.h:834-848): double sums in its order, each rounded to float once."""
        res = self.res
        T = np.float32 if "float_table" in self.plant else np.float64
        f = func.astype(T)
        s = np.zeros((res, res), T)
        s[0, 0] = f[0, 0]
        for x in range(1, res):
            s[0, x] = f[0, x] + s[0, x - 1]
        for y in range(1, res):
            s[y, 0] = f[y, 0] + s[y - 1, 0]
        for y in range(1, res):
            for x in range(1, res):
                s[y, x] = T(T(T(f[y, x] + s[y, x - 1]) + s[y - 1, x]) - s[y - 1, x - 1])
        return s.astype(f32)

    def phi(self):
        """Phi (lights.cpp:1284): scale * Area() * sumL / (width * height), per channel."""
        return ((self.L * self.area).astype(f32) * self.sum_phi / f32(self.res * self.res)).astype(f32)

    # ---- the map ----
    def jacobian(self, w):
        with np.errstate(**_ERR):
            a = (f32(PI * PI) * (f32(1) - (w[:, 0] * w[:, 0]).astype(f32))).astype(f32)
            return ((a * (f32(1) - (w[:, 1] * w[:, 1]).astype(f32))).astype(f32) / w[:, 2]).astype(f32)

    def render_from_image(self, u, v):
        u, v = np.asarray(u, f32).reshape(-1), np.asarray(v, f32).reshape(-1)
        alpha, beta = (-PI_OVER_2 + (u * PI).astype(f32)).astype(f32), (-PI_OVER_2 + (v * PI).astype(f32)).astype(f32)
        w = normalize(np.stack([tanf(alpha), tanf(beta), np.ones_like(u)], axis=1).astype(f32))
        out = ((w[:, 0:1] * self.fx[None, :]).astype(f32) + w[:, 1:2] * self.fy[None, :]).astype(f32) + w[:, 2:3] * self.fz[None, :]
        return out.astype(f32), self.jacobian(w)

    def image_from_render(self, wr):
        """(valid, u, v, duv_dw); u, v are 0 where not valid."""
        wr = np.asarray(wr, f32).reshape(-1, 3)
        w = np.stack([_dot(wr, self.fx), _dot(wr, self.fy), _dot(wr, self.fz)], axis=1).astype(f32)
        with np.errstate(invalid="ignore"):
            valid = w[:, 2] > 0
        with np.errstate(**_ERR):
            u = _clamp01(((atan2f(w[:, 0], w[:, 2]) + PI_OVER_2).astype(f32) / PI).astype(f32))
            v = _clamp01(((atan2f(w[:, 1], w[:, 2]) + PI_OVER_2).astype(f32) / PI).astype(f32))
        return valid, np.where(valid, u, f32(0)).astype(f32), np.where(valid, v, f32(0)).astype(f32), self.jacobian(w)

    def image_bounds(self, p):
        """(valid, b[n, 4] = pMin.x, pMin.y, pMax.x, pMax.y)."""
        p = np.asarray(p, f32).reshape(-1, 3)
        ok0, u0, v0, _ = self.image_from_render(normalize((self.p0[None, :] - p).astype(f32)))
        ok1, u1, v1, _ = self.image_from_render(normalize((self.p2[None, :] - p).astype(f32)))
        b = np.stack([np.minimum(u0, u1), np.minimum(v0, v1), np.maximum(u0, u1), np.maximum(v0, v1)], axis=1).astype(f32)
        valid = ok0 & ok1
        return valid, np.where(valid[:, None], b, f32(0)).astype(f32)

    # ---- the summed-area table ----
    def lookup(self, x, y):
        """SummedAreaTable::Lookup (util/sampling.h:864-876), every term, with the defined float -> int."""
        res = self.res
        x, y = (np.asarray(x, f32) * f32(res)).astype(f32), (np.asarray(y, f32) * f32(res)).astype(f32)
        x0, y0 = _idx(x, res), _idx(y, res)

        def li(ix, iy):
            zero = (ix == 0) | (iy == 0)
            return np.where(zero, f32(0), self.table[np.clip(np.minimum(iy - 1, res - 1), 0, None), np.clip(np.minimum(ix - 1, res - 1), 0, None)]).astype(f32)
        v00, v10, v01, v11 = li(x0, y0), li(x0 + 1, y0), li(x0, y0 + 1), li(x0 + 1, y0 + 1)
        dx, dy = (x - x0.astype(f32)).astype(f32), (y - y0.astype(f32)).astype(f32)
        ox, oy = (f32(1) - dx).astype(f32), (f32(1) - dy).astype(f32)
        with np.errstate(**_ERR):
            r = ((ox * oy).astype(f32) * v00).astype(f32) + ((ox * dy).astype(f32) * v01).astype(f32)
            r = r.astype(f32) + ((dx * oy).astype(f32) * v10).astype(f32)
            return (r.astype(f32) + ((dx * dy).astype(f32) * v11).astype(f32)).astype(f32)

    def integral(self, b):
        """SummedAreaTable::Integral (util/sampling.h:851-857) of windows b[n, 4]."""
        b = np.asarray(b, f32).reshape(-1, 4)
        l = lambda x, y: self.lookup(x, y).astype(np.float64)
        with np.errstate(**_ERR):
            s = (l(b[:, 2], b[:, 3]) - l(b[:, 0], b[:, 3])) + (l(b[:, 0], b[:, 1]) - l(b[:, 2], b[:, 1]))
            q = (s / np.float64(self.res * self.res)).astype(f32)
            return np.where(q < 0, f32(0), q).astype(f32)

    def eval(self, u, v):
        res = self.res
        iu = np.minimum(_idx((np.asarray(u, f32) * f32(res)).astype(f32), res), res - 1)
        iv = np.minimum(_idx((np.asarray(v, f32) * f32(res)).astype(f32), res), res - 1)
        return self.func[iv, iu]

    def image_lookup(self, u, v):
        res = self.res
        iu = np.minimum(_idx((np.asarray(u, f32) * f32(res)).astype(f32), res), res - 1)
        iv = np.minimum(_idx((np.asarray(v, f32) * f32(res)).astype(f32), res), res - 1)
        return (np.maximum(f32(0), self.image[iv, iu]) * self.L[None, :]).astype(f32)

    def _bisect(self, along_x, win, norm, u, lo, hi):
        """SampleBisection (util/sampling.h:955-971) with the cap.  win: the window whose moving pMax coordinate P(c) replaces."""
        n = f32(self.res)
        lo, hi = lo.copy(), hi.copy()
        col = 2 if along_x else 3

        def cdf(c):
            w = win.copy()
            w[:, col] = c
            with np.errstate(**_ERR):
                return (self.integral(w) / norm).astype(f32)
        trips = np.zeros(lo.shape[0], np.int64)
        for _ in range(BISECT_CAP):
            with np.errstate(invalid="ignore"):
                go = (np.ceil((n * hi).astype(f32)) - np.floor((n * lo).astype(f32))) > 1
            if not go.any():
                break
            mid = ((lo + hi).astype(f32) / f32(2)).astype(f32)
            with np.errstate(invalid="ignore"):
                gt = cdf(mid) > u
            hi = np.where(go & gt, mid, hi).astype(f32)
            lo = np.where(go & ~gt, mid, lo).astype(f32)
            trips += go
        plo, phi = cdf(lo), cdf(hi)
        with np.errstate(**_ERR):
            t = ((u - plo).astype(f32) / (phi - plo).astype(f32)).astype(f32)
            bad = ~(np.abs(t) <= FLT_MAX)
            x = (((f32(1) - t).astype(f32) * lo).astype(f32) + (t * hi).astype(f32)).astype(f32)
            x = np.where(x < lo, lo, np.where(x > hi, hi, x)).astype(f32)
        return x, trips, bad

    def sample_uv(self, b, u):
        """WindowedPiecewiseConstant2D::Sample (util/sampling.h:903-942): dict of why, u, v, mapPDF, trips_x, trips_y."""
        b, u = np.asarray(b, f32).reshape(-1, 4), np.asarray(u, f32).reshape(-1, 2)
        n = b.shape[0]
        why = np.zeros(n, np.int64)
        bint = self.integral(b)
        why[bint == 0] = WHY_ZERO_WINDOW
        px, tx, bad_x = self._bisect(True, b, bint, u[:, 0], b[:, 0], b[:, 2])
        why[(why == 0) & bad_x] = WHY_BAD_T
        nx = f32(self.res)
        cond = b.copy()
        with np.errstate(**_ERR):
            cond[:, 0] = np.floor((px * nx).astype(f32)) / nx
            c1 = (np.ceil((px * nx).astype(f32)) / nx).astype(f32)
        cond[:, 2] = np.where(cond[:, 0] == c1, (c1 + f32(1) / nx).astype(f32), c1)
        cint = self.integral(cond)
        why[(why == 0) & (cint == 0)] = WHY_ZERO_COLUMN
        py, ty, bad = self._bisect(False, cond, cint, u[:, 1], b[:, 1], b[:, 3])
        why[(why == 0) & bad] = WHY_BAD_T
        with np.errstate(**_ERR):
            pdf = (self.eval(px, py) / bint).astype(f32)
        # the trip counts as the device reports them: a bisection that was not reached counts 0
        x_ran = bint != 0
        y_ran = x_ran & ~bad_x & (cint != 0)
        return dict(why=why, u=px, v=py, mapPDF=pdf, trips_x=np.where(x_ran, tx, 0), trips_y=np.where(y_ran, ty, 0), cond=cond, bint=bint,
                    cint=cint)

    # ---- the light ----
    def Le(self, ro, rd):
        """(inside, uv [n, 2] -- 0 where the direction has no image point --, Le [n, 3])."""
        ok, u, v, _ = self.image_from_render(normalize(np.asarray(rd, f32).reshape(-1, 3)))
        bok, b = self.image_bounds(ro)
        top = (u < b[:, 2]) & (v < b[:, 3]) if "exclusive_top" in self.plant else (u <= b[:, 2]) & (v <= b[:, 3])
        inside = ok & bok & (u >= b[:, 0]) & (v >= b[:, 1]) & top
        return inside, np.stack([u, v], axis=1), np.where(inside[:, None], self.image_lookup(u, v), f32(0)).astype(f32)

    def pdf_li(self, ctxp, w):
        ok, u, v, jac = self.image_from_render(np.asarray(w, f32).reshape(-1, 3))
        bok, b = self.image_bounds(ctxp)
        fint = self.integral(b)
        with np.errstate(**_ERR):
            pdf = np.where(fint == 0, f32(0), (self.eval(u, v) / fint).astype(f32)).astype(f32)
            out = (pdf * jac).astype(f32) if "multiply_jacobian" in self.plant else (pdf / jac).astype(f32)
        return np.where(ok & (jac != 0) & bok, out, f32(0)).astype(f32)

    def batch(self, ctxp, dirs, u):
        """The [n, 32] array vspg_portallight_batch returns."""
        ctxp, dirs, u = np.asarray(ctxp, f32).reshape(-1, 3), np.asarray(dirs, f32).reshape(-1, 3), np.asarray(u, f32).reshape(-1, 2)
        n = ctxp.shape[0]
        o = np.zeros((n, OUT), f32)
        bok, b = self.image_bounds(ctxp)
        o[:, 0], o[:, 1:5] = bok, b
        inside, uv, le = self.Le(ctxp, dirs)
        o[:, 5], o[:, 6:8], o[:, 8:11] = inside, uv, le
        o[:, 11] = self.pdf_li(ctxp, dirs)
        s = self.sample_uv(b, u)
        why = np.where(bok, s["why"], WHY_NO_BOUNDS)
        wi, jac = self.render_from_image(s["u"], s["v"])
        why = np.where((why == 0) & (jac == 0), WHY_ZERO_JACOBIAN, why)
        ok = why == 0
        with np.errstate(**_ERR):
            pdf = (s["mapPDF"] * jac).astype(f32) if "multiply_jacobian" in self.plant else (s["mapPDF"] / jac).astype(f32)
        pl = (ctxp + (wi * f32(f32(2) * self.scene_radius)).astype(f32)).astype(f32)
        vals = np.concatenate([s["u"][:, None], s["v"][:, None], s["mapPDF"][:, None], jac[:, None], wi, pdf[:, None],
                               self.image_lookup(s["u"], s["v"])], axis=1)
        o[:, 12] = ok
        o[:, 13:24] = np.where(ok[:, None], vals, f32(0))
        o[:, 27:30] = np.where(ok[:, None], pl, f32(0))
        o[:, 24] = np.where(bok, s["trips_x"], 0)
        o[:, 25] = np.where(bok, s["trips_y"], 0)
        o[:, 26] = why
        return o


# ---------------------------------------------------------------------------------------------------------------------------
# float64 statement of the mathematics
def image_from_local_exact(w):
    """The gnomonic-angle map: (u, v) = ((atan2(x, z) + pi/2) / pi, (atan2(y, z) + pi/2) / pi) for z > 0, and d(u, v)/d(omega) =
    pi^2 (1 - x^2)(1 - y^2) / z of the unit vector w."""
    w = np.asarray(w, np.float64).reshape(-1, 3)
    w = w / np.linalg.norm(w, axis=1, keepdims=True)
    u = (np.arctan2(w[:, 0], w[:, 2]) + math.pi / 2) / math.pi
    v = (np.arctan2(w[:, 1], w[:, 2]) + math.pi / 2) / math.pi
    return u, v, math.pi ** 2 * (1 - w[:, 0] ** 2) * (1 - w[:, 1] ** 2) / w[:, 2]


def local_from_image_exact(u, v):
    x, y = np.tan(-math.pi / 2 + np.asarray(u, np.float64) * math.pi), np.tan(-math.pi / 2 + np.asarray(v, np.float64) * math.pi)
    w = np.stack([x, y, np.ones_like(x)], axis=1)
    return w / np.linalg.norm(w, axis=1, keepdims=True)


def window_integral_exact(func, b):
    """The exact integral of the step function `func` ([res, res], unit square) over the window b = (x0, y0, x1, y1), float64."""
    func = np.asarray(func, np.float64)
    res = func.shape[0]
    edges = np.arange(res + 1, dtype=np.float64) / res
    ox = np.clip(np.minimum(edges[1:], b[2]) - np.maximum(edges[:-1], b[0]), 0, None)
    oy = np.clip(np.minimum(edges[1:], b[3]) - np.maximum(edges[:-1], b[1]), 0, None)
    return float(oy @ func @ ox)


def window_pdf_exact(func, b, u, v):
    """The windowed density at (u, v): func / its integral over the window."""
    res = func.shape[0]
    iu, iv = min(int(u * res), res - 1), min(int(v * res), res - 1)
    return float(func[iv, iu]) / window_integral_exact(func, b)


def window_cdf_x_exact(func, b, x):
    """The marginal CDF in x of the windowed density at x."""
    return window_integral_exact(func, (b[0], b[1], x, b[3])) / window_integral_exact(func, b)


def rect_form_factor(a, b, h):
    """Form factor from a differential element to a parallel a x b rectangle at distance h, one of whose corners lies on the
    element's normal (the classic closed form); rectangles anywhere follow by signed sums of four such corners."""
    if a == 0 or b == 0:
        return 0.0
    sa, sb = math.copysign(1, a), math.copysign(1, b)
    a, b = abs(a) / h, abs(b) / h
    f = (a / math.sqrt(1 + a * a) * math.atan(b / math.sqrt(1 + a * a)) + b / math.sqrt(1 + b * b) * math.atan(a / math.sqrt(1 + b * b))) / (2 * math.pi)
    return sa * sb * f


def rect_form_factor_window(x0, x1, y0, y1, h):
    return rect_form_factor(x1, y1, h) - rect_form_factor(x0, y1, h) - rect_form_factor(x1, y0, h) + rect_form_factor(x0, y0, h)


# ---------------------------------------------------------------------------------------------------------------------------
# fixtures
def make_image(kind, res, seed=0):
    """Equal-area test maps: 'peaked', 'banded', 'constant', 'half_zero' (v < 0.5 all zero), 'random'."""
    rng = np.random.default_rng(seed)
    img = np.zeros((res, res, 3), f32)
    if kind == "constant":
        img[:] = f32(0.75)
    elif kind == "banded":
        img[:] = (f32(0.05) + (np.arange(res) % 3 == 0).astype(f32))[None, :, None] * np.array([1.0, 0.5, 0.25], f32)
    elif kind == "peaked":
        img[:] = f32(0.01)
        img[res // 3, (2 * res) // 3] = (500, 300, 100)
    elif kind == "half_zero":
        img[:] = rng.uniform(0.1, 1.0, (res, res, 3)).astype(f32)
        img[: res // 2] = 0
    else:
        img[:] = rng.uniform(0.0, 2.0, (res, res, 3)).astype(f32)
    return img


AXIS_PORTAL = np.array([[-1, -1, 2], [1, -1, 2], [1, 1, 2], [-1, 1, 2]], f32)  # in z = 2, frame x = +y, y = +x, z = -z (towards -z) ...


def oblique_portal():
    """A 2 x 1.2 rectangle in a tilted plane (exact right angles in float64, rounded once)."""
    ex = np.array([1.0, 0.5, 0.25])
    ex /= np.linalg.norm(ex)
    ey = np.cross(np.array([0.3, -0.2, 1.0]), ex)
    ey /= np.linalg.norm(ey)
    c = np.array([0.4, -0.3, 1.5])
    return np.array([c - ex - 0.6 * ey, c + ex - 0.6 * ey, c + ex + 0.6 * ey, c - ex + 0.6 * ey]).astype(f32)


def make_queries(light, n, seed):
    """Context points in front of the portal (away from its vertices) with a few behind its plane, directions through and beside the
    opening, variates in [0, 1)."""
    rng = np.random.default_rng(seed)
    q = light.portal.astype(np.float64)
    c = q.mean(axis=0)
    ex, ey = q[1] - q[0], q[3] - q[0]
    nz = light.fz.astype(np.float64)
    a, b, h = rng.uniform(-0.9, 0.9, n), rng.uniform(-0.9, 0.9, n), rng.uniform(0.3, 3.0, n)
    h[::11] *= -1  # behind the portal plane: no bounds
    p = c[None, :] + a[:, None] * ex[None, :] + b[:, None] * ey[None, :] - h[:, None] * nz[None, :]
    t = q[0][None, :] + rng.uniform(-0.3, 1.3, n)[:, None] * ex[None, :] + rng.uniform(-0.3, 1.3, n)[:, None] * ey[None, :]
    d = t - p
    d *= rng.uniform(0.5, 2.0, n)[:, None] / np.linalg.norm(d, axis=1, keepdims=True)
    return p.astype(f32), d.astype(f32), rng.uniform(0, 1, (n, 2)).astype(f32)


# the fixtures tests/test_portallight_model.py and tests/test_portallight_gpu.py share
def rotated():
    a, b = 0.7, -0.4
    rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    m = np.zeros((3, 4), f32)
    m[:, :3] = (rz @ rx).astype(f32)
    return m


# (name, image kind, res, seed, rotated?, oblique portal?)
CASES = [("1 constant", "constant", 1, 0, False, False), ("2 random", "random", 2, 1, False, True), ("3 random rot", "random", 3, 2, True, False),
         ("16 peaked", "peaked", 16, 3, False, False), ("16 banded rot oblique", "banded", 16, 4, True, True),
         ("16 half zero", "half_zero", 16, 5, False, False), ("64 random oblique", "random", 64, 6, False, True),
         ("64 constant rot", "constant", 64, 7, True, False), ("3 half zero", "half_zero", 3, 8, False, True)]
L_RGB = (0.5, 2.0, 1.0)
RADIUS = 7.5
N_QUERIES = 203  # no multiple of 64


def make_light(case, plant=()):
    name, kind, res, seed, rot, obl = case
    return PortalLight(make_image(kind, res, seed), oblique_portal() if obl else AXIS_PORTAL, L=L_RGB, m34=rotated() if rot else None,
                         scene_radius=RADIUS, plant=plant)
