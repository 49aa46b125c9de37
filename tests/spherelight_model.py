"""DiffuseAreaLight on a full Shape "sphere", restated from the reference's text (src/pbrt/shapes.h:293-393 Sphere::Sample(ctx, u) and
PDF(ctx, wi); shapes.cpp:33-58 Bounds and Sample(u); shapes.h:147-284 BasicIntersect / InteractionFromIntersection; lights.cpp:796-864
SampleLi, PDF_Li, Phi, Bounds; lights.h:492-511 L; util/sampling.h:391-396; util/vecmath.h:1007-1013, 1666-1672, 1867-1871, 1915;
util/transform.h:133-175, 310-334; shapes.h:63-90 ShapeSampleContext).

Three statements of the same mathematics:
  * a float32 NumPy MIRROR (class SphereLight) -- one rounding per operation in the reference's order of operations, fused operations
    only where the reference's FMA / DifferenceOfProducts / SumOfProducts stand (Dot(Normal3f, Vector3f)); what the device computes
    bit for bit (tests/test_spherelight_gpu.py).  sinf / cosf are the running host libm's, which vspg_libm.h equals;
  * a float64 STATEMENT (suffix 64): the uniform cone and the uniform area, against which the mirror's rounding is bounded;
  * a float64 direct-lighting QUADRATURE / Monte Carlo for the known answers of the GPU tests.
The (u, v) of a sample is not computed (nothing reads it without textures).

`planted` names a deliberate error, for the tests that show each of them is caught:
  no_taylor     the small-angle Taylor branch dropped           dist_pdf     Distance for DistanceSquared in PDF's inside branch
  no_reverse    the normal not flipped under reverseOrientation  one_sided_L  two_sided ignored in L
  inside_on_p   the inside test on ctx.p instead of the offset origin
"""
import ctypes as C
import ctypes.util
import math

import numpy as np

from pointlight_model import fma32 as _fma32_scalar

f32 = np.float32
PI = f32(3.14159265358979323846)
EPS = 2.0 ** -24
PLANTED = ("no_taylor", "dist_pdf", "no_reverse", "one_sided_L", "inside_on_p")
INF = f32(np.inf)


def gamma(n):
    return f32(f32(n) * f32(EPS)) / (f32(1) - f32(n) * f32(EPS))


G3, G5 = gamma(3), gamma(5)

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("cosf", "sinf", "acosf"):
    getattr(_libm, _n).restype = C.c_float
    getattr(_libm, _n).argtypes = [C.c_float]
sinf = np.vectorize(lambda x: f32(_libm.sinf(float(x))), otypes=[f32])
cosf = np.vectorize(lambda x: f32(_libm.cosf(float(x))), otypes=[f32])

def _fma32_any(a, b, c):  # the exact fused multiply-add of tests/pointlight_model.py; NaN / infinite operands give what IEEE gives
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return f32(np.float64(a) * np.float64(b) + np.float64(c))
    return _fma32_scalar(a, b, c)


fma32 = np.vectorize(_fma32_any, otypes=[f32])


def A(x):
    return np.asarray(x, f32)


def up(v):      # NextFloatUp (util/float.h:164-178)
    return np.nextafter(A(v), INF)


def down(v):    # NextFloatDown
    return np.nextafter(A(v), -INF)


def sqr(x):
    return x * x


def fmax0(x):   # std::max(0.f, x): `0 < x ? x : 0` -- a NaN gives 0 (np.maximum would hand it on)
    x = A(x)
    return np.where(f32(0) < x, x, f32(0))


def safe_sqrt(x):
    return np.sqrt(fmax0(x))


def len2(v):
    return sqr(v[..., 0]) + sqr(v[..., 1]) + sqr(v[..., 2])


def length(v):
    return np.sqrt(len2(v))


def normalize(v):
    return v / length(v)[..., None]


def dot(a, b):  # Dot(Vector3f, Vector3f) (vecmath.h:964-967)
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def dot_n(n, v):
    """Dot(Normal3f, Vector3f) (vecmath.h:1057-1061): FMA(n.x, v.x, SumOfProducts(n.y, v.y, n.z, v.z)) (math.h:577-583)."""
    n, v = np.broadcast_arrays(A(n), A(v))
    cd = n[..., 2] * v[..., 2]
    sop = fma32(n[..., 1], v[..., 1], cd)
    err = fma32(n[..., 2], v[..., 2], -cd)
    return fma32(n[..., 0], v[..., 0], sop + err)


def dop(a, b, c, d):
    """DifferenceOfProducts (math.h:569-574): a * b - c * d with the product's rounding error added back."""
    cd = c * d
    return fma32(a, b, -cd) + fma32(-c, d, cd)


def cross(v, w):  # Cross (vecmath.h:999-1004)
    return np.stack([dop(v[..., 1], w[..., 2], v[..., 2], w[..., 1]), dop(v[..., 2], w[..., 0], v[..., 0], w[..., 2]),
                     dop(v[..., 0], w[..., 1], v[..., 1], w[..., 0])], -1)


# ---- Interval (util/math.h:815-1000) and Point3fi -------------------------------------------------------------------------------------
class Ivl:
    def __init__(self, lo, hi):
        lo, hi = np.broadcast_arrays(A(lo), A(hi))
        self.lo, self.hi = np.minimum(lo, hi), np.maximum(lo, hi)

    @staticmethod
    def from_err(v, e):
        v, e = np.broadcast_arrays(A(v), A(e))
        return Ivl(np.where(e == 0, v, down(v - e)), np.where(e == 0, v, up(v + e)))

    def mid(self):
        return (self.lo + self.hi) / f32(2)

    def err(self):
        return (self.hi - self.lo) / f32(2)

    def has(self, v):
        return (v >= self.lo) & (v <= self.hi)

    def __add__(self, o):
        return Ivl(down(self.lo + o.lo), up(self.hi + o.hi))

    def __sub__(self, o):
        return Ivl(down(self.lo + -o.hi), up(self.hi + -o.lo))

    def __mul__(self, o):
        p = [self.lo * o.lo, self.hi * o.lo, self.lo * o.hi, self.hi * o.hi]
        return Ivl(np.minimum.reduce([down(q) for q in p]), np.maximum.reduce([up(q) for q in p]))

    def __truediv__(self, o):
        zero = o.has(f32(0))
        q = [self.lo / o.lo, self.hi / o.lo, self.lo / o.hi, self.hi / o.hi]
        lo, hi = np.minimum.reduce([down(v) for v in q]), np.maximum.reduce([up(v) for v in q])
        return Ivl(np.where(zero, -INF, lo), np.where(zero, INF, hi))

    def sqr(self):
        alow, ahigh = np.abs(self.lo), np.abs(self.hi)
        alow, ahigh = np.minimum(alow, ahigh), np.maximum(alow, ahigh)
        return Ivl(np.where(self.has(f32(0)), f32(0), down(alow * alow)), up(ahigh * ahigh))

    def fmul(self, f):  # operator*(Float, Interval)
        f = f32(f)
        if f > 0:
            return Ivl(down(f * self.lo), up(f * self.hi))
        return Ivl(down(f * self.hi), up(f * self.lo))

    def sqrt(self):
        return Ivl(fmax0(down(np.sqrt(self.lo))), up(np.sqrt(self.hi)))

    def pick(self, cond, other):
        return Ivl.raw(np.where(cond, self.lo, other.lo), np.where(cond, self.hi, other.hi))

    @staticmethod
    def raw(lo, hi):
        r = Ivl.__new__(Ivl)
        r.lo, r.hi = A(lo), A(hi)
        return r


class P3i:
    """Point3fi as three intervals; .mid() = Point3f(pi), .err() = pi.Error()."""

    def __init__(self, lo, hi):
        self.lo, self.hi = A(lo), A(hi)

    @staticmethod
    def exact(p):
        return P3i(A(p), A(p))

    @staticmethod
    def from_err(p, e):
        p, e = np.broadcast_arrays(A(p), A(e))
        i = Ivl.from_err(p, e)
        return P3i(i.lo, i.hi)

    def mid(self):
        return (self.lo + self.hi) / f32(2)

    def err(self):
        return (self.hi - self.lo) / f32(2)


def offset_ray_origin(pi, n, w):
    """ShapeSampleContext::OffsetRayOrigin(Vector3f w) (shapes.h:63-80) as the library's offset_ray_origin evaluates it for every
    context (vspg_device.h): d = Dot(Abs(n), pi.Error()), offset = d * n flipped where Dot(w, n) < 0, po = p + offset, each component
    rounded away from p."""
    n, w = A(n), A(w)
    d = dot(np.abs(n), pi.err())
    offset = n * d[..., None]
    offset = np.where((dot(w, n) < 0)[..., None], -offset, offset)
    po = pi.mid() + offset
    return np.where(offset > 0, up(po), np.where(offset < 0, down(po), po))


def coordinate_system(v):
    sign = np.copysign(f32(1), v[..., 2])
    a = f32(-1) / (sign + v[..., 2])
    b = v[..., 0] * v[..., 1] * a
    x = np.stack([f32(1) + sign * sqr(v[..., 0]) * a, sign * b, -sign * v[..., 0]], -1)
    y = np.stack([b, sign + sqr(v[..., 1]) * a, -v[..., 1]], -1)
    return x, y


class SphereLight:
    """The float32 mirror.  m / mi: renderFromObject and its inverse (4 x 4, affine); the records the library derives on the host
    (centre, 1 / Area, phiMax, thetaZMin / thetaZMax) are formed here by the same operations."""

    def __init__(self, m, mi, radius, Le, two_sided=False, reverse=False, planted=None):
        self.m, self.mi = A(m).reshape(4, 4), A(mi).reshape(4, 4)
        self.radius, self.Le = f32(radius), A(Le)
        self.two_sided, self.reverse, self.planted = bool(two_sided), bool(reverse), planted
        r = self.radius
        self.phi_max = (PI / f32(180)) * f32(360)                         # Radians(360)
        self.theta_zmin = f32(_libm.acosf(float(min(max(-r / r, -1), 1))))
        self.theta_zmax = f32(_libm.acosf(float(min(max(r / r, -1), 1))))
        self.area = (self.phi_max * r) * (r - (-r))                        # phiMax * radius * (zMax - zMin)
        self.inv_area = f32(1) / self.area
        q = [((self.m[k, 0] * f32(0) + self.m[k, 1] * f32(0)) + self.m[k, 2] * f32(0)) + self.m[k, 3] for k in range(4)]
        self.center = A([q[k] if q[3] == 1 else q[k] / q[3] for k in range(3)])
        # Transform::SwapsHandedness: the hit normal flips by reverseOrientation ^ that
        self.flip = self.reverse ^ bool(np.linalg.det(self.m[:3, :3].astype(np.float64)) < 0)

    # -- transforms ----------------------------------------------------------------------------------------------------------------------
    def point_to_render(self, pObj):
        """(*renderFromObject)(Point3fi(pObj, gamma(5) * Abs(pObj))) (transform.h:133-175)."""
        i = Ivl.from_err(pObj, G5 * np.abs(pObj))
        c, e = i.mid(), i.err()
        exact = np.all((i.hi - i.lo) == 0, axis=-1)
        x, y, z = c[..., 0], c[..., 1], c[..., 2]
        pv, pe = [], []
        for k in range(3):
            row = self.m[k]
            pv.append((row[0] * x + row[1] * y) + (row[2] * z + row[3]))
            ea = G3 * (np.abs(row[0] * x) + np.abs(row[1] * y) + np.abs(row[2] * z) + np.abs(row[3]))
            pe.append(np.where(exact, ea, (G3 + f32(1)) * (np.abs(row[0]) * e[..., 0] + np.abs(row[1]) * e[..., 1] + np.abs(row[2]) * e[..., 2]) + ea))
        return P3i.from_err(np.stack(pv, -1), np.stack(pe, -1))

    def normal_to_render(self, no):
        mi = self.mi
        x, y, z = no[..., 0], no[..., 1], no[..., 2]
        return normalize(np.stack([mi[0, k] * x + mi[1, k] * y + mi[2, k] * z for k in range(3)], -1))

    # -- L ---------------------------------------------------------------------------------------------------------------------------------
    def L(self, n, w):
        """DiffuseAreaLight::L (lights.h:492-511): zero for !twoSided && Dot(n, w) < 0.  Returns (N, 3)."""
        two = self.two_sided and self.planted != "one_sided_L"
        dark = np.zeros(np.broadcast(n[..., 0], w[..., 0]).shape, bool) if two else dot_n(n, w) < 0
        return np.where(dark[..., None], f32(0), self.Le)

    # -- the inside / outside decision -------------------------------------------------------------------------------------------------
    def inside(self, pi, n):
        p = pi.mid()
        if self.planted == "inside_on_p":
            pOrigin = p
        else:
            pOrigin = offset_ray_origin(pi, n, self.center - p)
        return len2(pOrigin - self.center) <= sqr(self.radius)

    # -- Sphere::Sample(ctx, u) + DiffuseAreaLight::SampleLi ---------------------------------------------------------------------------
    def sample_li(self, ctx_p, ctx_n, u, ctx_perr=None):
        """Returns a dict of arrays: ok, wi, L, pdf, p (the sampled point, Point3f(pi)), n, inside, taylor, perr (pi.Error())."""
        with np.errstate(all="ignore"):
            ctx_p, ctx_n, u = A(ctx_p).reshape(-1, 3), A(ctx_n).reshape(-1, 3), A(u).reshape(-1, 2)
            pi_ctx = P3i.exact(ctx_p) if ctx_perr is None else P3i.from_err(ctx_p, A(ctx_perr).reshape(-1, 3))
            ctxp = pi_ctx.mid()
            u0, u1 = u[:, 0], u[:, 1]
            r = self.radius
            inside = self.inside(pi_ctx, ctx_n)
            flip = self.reverse and self.planted != "no_reverse"
            # inside: Sphere::Sample(u) (shapes.cpp:38-58)
            z = f32(1) - f32(2) * u0
            rr = safe_sqrt(f32(1) - sqr(z))
            phi = (f32(2) * PI) * u1
            pObj = np.stack([f32(0) + r * (rr * cosf(phi)), f32(0) + r * (rr * sinf(phi)), f32(0) + r * z], -1)
            pObj = pObj * (r / length(pObj))[..., None]
            n_in = self.normal_to_render(pObj)
            if flip:
                n_in = -n_in
            pi_in = self.point_to_render(pObj)
            wi_in = pi_in.mid() - ctxp
            zero_in = len2(wi_in) == 0
            wi_in = normalize(wi_in)
            pdf_in = self.inv_area / (np.abs(dot_n(n_in, -wi_in)) / len2(ctxp - pi_in.mid()))
            ok_in = ~zero_in & ~np.isinf(pdf_in)
            # outside: the cone (shapes.h:316-360)
            sinThetaMax = r / length(ctxp - self.center)
            sin2ThetaMax = sqr(sinThetaMax)
            cosThetaMax = safe_sqrt(f32(1) - sin2ThetaMax)
            oneMinus = f32(1) - cosThetaMax
            cosTheta = (cosThetaMax - f32(1)) * u0 + f32(1)
            sin2Theta = f32(1) - sqr(cosTheta)
            taylor = sin2ThetaMax < f32(0.00068523)
            if self.planted == "no_taylor":
                taylor = np.zeros_like(taylor)
            t_s2 = sin2ThetaMax * u0
            sin2Theta = np.where(taylor, t_s2, sin2Theta)
            cosTheta = np.where(taylor, np.sqrt(f32(1) - t_s2), cosTheta)
            oneMinus = np.where(taylor, sin2ThetaMax / f32(2), oneMinus)
            cosAlpha = sin2Theta / sinThetaMax + cosTheta * safe_sqrt(f32(1) - sin2Theta / sqr(sinThetaMax))
            sinAlpha = safe_sqrt(f32(1) - sqr(cosAlpha))
            phi2 = u1 * f32(2) * PI
            sA, cA = np.clip(sinAlpha, f32(-1), f32(1)), np.clip(cosAlpha, f32(-1), f32(1))
            w = np.stack([sA * cosf(phi2), sA * sinf(phi2), cA], -1)
            fz = normalize(self.center - ctxp)
            fx, fy = coordinate_system(fz)
            mw = -w
            n_out = mw[:, 0:1] * fx + mw[:, 1:2] * fy + mw[:, 2:3] * fz
            p_out = self.center + r * n_out
            if flip:
                n_out = -n_out
            pi_out = P3i.from_err(p_out, G5 * np.abs(p_out))
            pdf_out = f32(1) / ((f32(2) * PI) * oneMinus)
            # merge, then DiffuseAreaLight::SampleLi (lights.cpp:803-819)
            sel = inside[:, None]
            p = np.where(sel, pi_in.mid(), pi_out.mid())
            perr = np.where(sel, pi_in.err(), pi_out.err())
            n = np.where(sel, n_in, n_out)
            pdf = np.where(inside, pdf_in, pdf_out)
            ok = np.where(inside, ok_in, True)
            d = p - ctxp
            ok = ok & ~(pdf == 0) & ~(len2(d) == 0)
            wi = normalize(d)
            Le = self.L(n, -wi)
            dark = ~np.any(Le != 0, axis=-1)
            res = dict(ok=ok & ~dark, wi=wi, L=Le, pdf=pdf, p=p, n=n, inside=inside, taylor=taylor & ~inside, perr=perr, dark=ok & dark,
                       inf_rejected=inside & ~zero_in & np.isinf(pdf_in))
            return res

    # -- Sphere::BasicIntersect (shapes.h:147-229) for the full sphere, tMax = Infinity; InteractionFromIntersection's n and pi -----------
    def intersect(self, ro, rd, tMax=INF):
        """Returns (hit, tHit, pObj)."""
        with np.errstate(all="ignore"):
            ro, rd = A(ro).reshape(-1, 3), A(rd).reshape(-1, 3)
            r = self.radius
            oi, di = [], []
            for k in range(3):
                row = self.mi[k]
                v = (row[0] * ro[:, 0] + row[1] * ro[:, 1]) + (row[2] * ro[:, 2] + row[3])
                e = G3 * (np.abs(row[0] * ro[:, 0]) + np.abs(row[1] * ro[:, 1]) + np.abs(row[2] * ro[:, 2]) + np.abs(row[3]))
                oi.append(Ivl.from_err(v, e))
                ev = G3 * (np.abs(row[0] * rd[:, 0]) + np.abs(row[1] * rd[:, 1]) + np.abs(row[2] * rd[:, 2]))
                vv = row[0] * rd[:, 0] + row[1] * rd[:, 1] + row[2] * rd[:, 2]
                di.append(Ivl.from_err(vv, ev))
            rI = Ivl.raw(np.full(ro.shape[0], r, f32), np.full(ro.shape[0], r, f32))
            a = di[0].sqr() + di[1].sqr() + di[2].sqr()
            b = (di[0] * oi[0] + di[1] * oi[1] + di[2] * oi[2]).fmul(2)
            c = (oi[0].sqr() + oi[1].sqr() + oi[2].sqr()) - rI.sqr()
            f = b / a.fmul(2)
            v = [oi[k] - f * di[k] for k in range(3)]
            ln = (v[0].sqr() + v[1].sqr() + v[2].sqr()).sqrt()
            discrim = a.fmul(4) * (rI + ln) * (rI - ln)
            hit = ~(discrim.lo < 0)
            root = discrim.sqrt()
            neg = b.mid() < 0
            q = (b - root).fmul(-.5).pick(neg, (b + root).fmul(-.5))
            t0, t1 = q / a, c / q
            swap = t0.lo > t1.lo
            t0, t1 = t1.pick(swap, t0), t0.pick(swap, t1)
            hit &= ~((t0.hi > tMax) | (t1.lo <= 0))
            use1 = t0.lo <= 0
            hit &= ~(use1 & (t1.hi > tMax))
            ts = t1.pick(use1, t0).mid()
            pHit = np.stack([oi[k].mid() + ts * di[k].mid() for k in range(3)], -1)
            pHit = pHit * (r / length(pHit))[..., None]
            fix = (pHit[:, 0] == 0) & (pHit[:, 1] == 0)
            pHit[:, 0] = np.where(fix, f32(1e-5) * r, pHit[:, 0])
            return hit, ts, pHit

    def hit_normal(self, pHit):
        """InteractionFromIntersection's geometric normal (shapes.h:237-284) carried to render space and normalised."""
        with np.errstate(all="ignore"):
            r = self.radius
            cosTheta = pHit[:, 2] / r
            zRadius = np.sqrt(sqr(pHit[:, 0]) + sqr(pHit[:, 1]))
            cosPhi, sinPhi = pHit[:, 0] / zRadius, pHit[:, 1] / zRadius
            dpdu = np.stack([-self.phi_max * pHit[:, 1], self.phi_max * pHit[:, 0], np.zeros_like(cosPhi)], -1)
            sinTheta = safe_sqrt(f32(1) - sqr(cosTheta))
            dth = self.theta_zmax - self.theta_zmin
            dpdv = np.stack([dth * (pHit[:, 2] * cosPhi), dth * (pHit[:, 2] * sinPhi), dth * (-r * sinTheta)], -1)
            no = normalize(cross(dpdu, dpdv))
            if self.flip:
                no = -no
            return self.normal_to_render(no)

    # -- Sphere::PDF(ctx, wi) ----------------------------------------------------------------------------------------------------------
    def pdf_li(self, ctx_p, ctx_n, wi, ctx_perr=None):
        with np.errstate(all="ignore"):
            ctx_p, ctx_n, wi = A(ctx_p).reshape(-1, 3), A(ctx_n).reshape(-1, 3), A(wi).reshape(-1, 3)
            pi_ctx = P3i.exact(ctx_p) if ctx_perr is None else P3i.from_err(ctx_p, A(ctx_perr).reshape(-1, 3))
            ctxp = pi_ctx.mid()
            inside = self.inside(pi_ctx, ctx_n)
            hit, t, pObj = self.intersect(offset_ray_origin(pi_ctx, ctx_n, wi), wi)
            n = self.hit_normal(pObj)
            ph = self.point_to_render(pObj).mid()
            d2 = len2(ctxp - ph)
            if self.planted == "dist_pdf":
                d2 = np.sqrt(d2)
            pdf_in = self.inv_area / (np.abs(dot_n(n, -wi)) / d2)
            pdf_in = np.where(np.isinf(pdf_in), f32(0), pdf_in)
            pdf_in = np.where(hit, pdf_in, f32(0))
            sin2ThetaMax = self.radius * self.radius / len2(ctxp - self.center)
            cosThetaMax = safe_sqrt(f32(1) - sin2ThetaMax)
            oneMinus = f32(1) - cosThetaMax
            taylor = sin2ThetaMax < f32(0.00068523)
            if self.planted == "no_taylor":
                taylor = np.zeros_like(taylor)
            oneMinus = np.where(taylor, sin2ThetaMax / f32(2), oneMinus)
            pdf_out = f32(1) / ((f32(2) * PI) * oneMinus)
            return np.where(inside, pdf_in, pdf_out)

    def probe(self, ctx_p, ctx_n, wi, ctx_perr=None):
        """What vspg_light_pdf_batch returns besides the PMF: PDF_Li, hit, L at the hit towards -wi, tHit."""
        ctx_p, ctx_n, wi = A(ctx_p).reshape(-1, 3), A(ctx_n).reshape(-1, 3), A(wi).reshape(-1, 3)
        pi_ctx = P3i.exact(ctx_p) if ctx_perr is None else P3i.from_err(ctx_p, A(ctx_perr).reshape(-1, 3))
        hit, t, pObj = self.intersect(offset_ray_origin(pi_ctx, ctx_n, wi), wi)
        L = np.where(hit[:, None], self.L(self.hit_normal(pObj), -wi), f32(0))
        return self.pdf_li(ctx_p, ctx_n, wi, ctx_perr), hit, L, np.where(hit, t, f32(0))

    # -- Phi, Bounds -------------------------------------------------------------------------------------------------------------------
    def phi(self):
        """DiffuseAreaLight::Phi (lights.cpp:826-843): Pi * (twoSided ? 2 : 1) * area * L."""
        return PI * f32(2 if self.two_sided else 1) * self.area * self.Le

    def bounds(self):
        """Sphere::Bounds (shapes.cpp:33-36): the object box's eight corners through Transform::operator()(Point3f) (transform.h:310-319)."""
        r = self.radius
        lo, hi = np.full(3, np.inf, f32), np.full(3, -np.inf, f32)
        for c in range(8):
            x, y, z = (r if c & 1 else -r), (r if c & 2 else -r), (r if c & 4 else -r)
            p = A([((self.m[k, 0] * x + self.m[k, 1] * y) + self.m[k, 2] * z) + self.m[k, 3] for k in range(3)])
            lo, hi = np.minimum(lo, p), np.maximum(hi, p)
        return lo, hi

    def light_bounds(self):
        """DiffuseAreaLight::Bounds (lights.cpp:845-864): (bmin, bmax, w, phi, cosTheta_o, cosTheta_e, twoSided)."""
        lo, hi = self.bounds()
        phi = f32(max(self.Le)) * (f32(1) * self.area * PI)
        return lo, hi, A([0, 0, 1]), phi, f32(-1), f32(_libm.cosf(float(PI / f32(2)))), self.two_sided


# ---- the float64 statement ---------------------------------------------------------------------------------------------------------------
def cone_pdf64(radius, dist):
    """Uniform over the cone a sphere of `radius` subtends from `dist` > radius: 1 / (2 pi (1 - cos theta_max))."""
    s2 = (radius / dist) ** 2
    return 1.0 / (2 * math.pi * (1 - math.sqrt(max(0.0, 1 - s2))))


def area_pdf64(radius, ctx_p, p, n):
    """Uniform over the area, in solid angle from ctx_p: (1 / (4 pi r^2)) * d^2 / |n . w|."""
    d = np.asarray(p, np.float64) - np.asarray(ctx_p, np.float64)
    d2 = np.sum(d * d, -1)
    w = d / np.sqrt(d2)[..., None]
    return d2 / (4 * math.pi * radius * radius * np.abs(np.sum(np.asarray(n, np.float64) * w, -1)))


def cone_hit64(center, radius, ctx_p, wi):
    """Does the ray ctx_p + t wi (t > 0) meet the sphere?"""
    oc = np.asarray(ctx_p, np.float64) - np.asarray(center, np.float64)
    wi = np.asarray(wi, np.float64)
    b = np.sum(oc * wi, -1)
    c = np.sum(oc * oc, -1) - radius * radius
    disc = b * b - np.sum(wi * wi, -1) * c
    return (disc >= 0) & ((-b + np.sqrt(np.maximum(disc, 0))) > 0)


# ---- float64 direct lighting for the known answers of the GPU tests ----------------------------------------------------------------------
def lambert_plate_quadrature64(r, d, Kd, L, n_theta=4096):
    """Scene (a): a diffuse plate (reflectance Kd, normal +z at the origin) under a sphere light of radius r whose centre sits at distance
    d on the normal.  Reflected radiance = (Kd / pi) * L * Integral over the cone of cos(theta) d omega, by the midpoint rule in theta
    (the integrand does not depend on phi).  Closed form: Kd * L * (r / d)^2."""
    tmax = math.asin(r / d)
    th = (np.arange(n_theta) + 0.5) * (tmax / n_theta)
    integral = 2 * math.pi * np.sum(np.cos(th) * np.sin(th)) * (tmax / n_theta)
    return Kd / math.pi * L * integral


def furnace_series64(L, rho, maxdepth):
    """Scene (b): inside a closed emissive sphere of albedo rho every ray sees L + rho * (the same); the path integrator adds emission at
    the camera hit (depth 0) and at every bounce up to depth == maxdepth: L * Sum_{k=0..maxdepth} rho^k."""
    return L * sum(rho ** k for k in range(maxdepth + 1))


def furnace_monte_carlo64(L, rho, maxdepth, n, seed=1):
    """The same by simulation of the estimator without NEE: cosine-weighted bounces inside the unit sphere (every bounce hits the
    sphere again, throughput rho per bounce, emission L at each hit while depth <= maxdepth).  Deterministic given geometry, so the
    Monte Carlo only checks the depth counting: the value is exact."""
    rng = np.random.default_rng(seed)
    total = np.zeros(n)
    beta = np.ones(n)
    for depth in range(maxdepth + 1):
        total += beta * L
        beta = beta * rho * np.ones_like(rng.random(n))
    return total.mean()


# ---- the fixtures the CPU and the GPU tests share -----------------------------------------------------------------------------------------
N_FIXTURE = 4099      # no multiple of 64
LAMP = dict(center=(0.3, -0.2, 0.5), radius=0.4, Le=(5.0, 4.0, 3.0), two_sided=False, reverse=False)
SHELL = dict(center=(-1.0, 0.8, 1.5), radius=1.25, Le=(2.0, 3.0, 4.0), two_sided=True, reverse=True, rotate=(37.0, (1, 2, 3)))
# minimum number of the N_FIXTURE contexts that land in each branch (tests/test_spherelight_model.py checks the mirror alone reaches them)
MIN_COUNT = dict(inside=500, surface=200, outside=1000, taylor=500)


def fixture_transforms(spec):
    """(m, mInv) of a fixture sphere: Translate(center) [* Rotate(angle, axis)], the inverse as vspg_transform_inverse forms it."""
    import pointlight_model as PM
    m = PM.translate(spec["center"])
    if "rotate" in spec:
        m = PM.mat4_mul(m, PM.rotate(*spec["rotate"]))
    return m, PM.transform_inverse(m)


def fixture_light(spec, planted=None):
    m, mi = fixture_transforms(spec)
    return SphereLight(m, mi, spec["radius"], spec["Le"], spec["two_sided"], spec["reverse"], planted=planted)


def fixture_contexts(light, n=N_FIXTURE, seed=5):
    """n contexts around `light`, in a fixed shuffled order: inside the sphere; ON it (the centre plus radius times a unit vector, in
    float32: the offset origin's squared distance lands on either side of Sqr(radius) and on it); outside at 1.02 to 25 radii; and
    beyond radius / sqrt(0.00068523) = 38.2 radii, where the Taylor branch takes over.  The first half are medium vertices (n = 0), the
    rest carry a unit normal.  Returns (p, normals, u (n x 3: pick, u0, u1), perr, kind) with kind 0 inside, 1 surface, 2 outside,
    3 far; perr is a Point3fi error of a few gamma(7) |p|, as a triangle hit carries."""
    rng = np.random.default_rng(seed)
    kind = np.concatenate([np.zeros(n // 4, int), np.ones(n // 8, int), np.full(n - n // 4 - n // 8 - n // 4, 2), np.full(n // 4, 3)])
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = float(light.radius)
    rho = np.where(kind == 0, r * rng.uniform(0.0, 0.98, n) ** (1 / 3), np.where(kind == 1, r, np.where(
        kind == 2, r * np.exp(rng.uniform(math.log(1.02), math.log(25.0), n)), r * np.exp(rng.uniform(math.log(40.0), math.log(4000.0), n)))))
    p = (light.center.astype(np.float64) + d * rho[:, None]).astype(f32)
    nn = rng.normal(size=(n, 3))
    nn = (nn / np.linalg.norm(nn, axis=1, keepdims=True)).astype(f32)
    u = rng.random((n, 3)).astype(f32)
    perr = (np.abs(p) * f32(7 * EPS) * rng.uniform(1, 4, (n, 3))).astype(f32)
    order = rng.permutation(n)
    p, nn, u, perr, kind = p[order], nn[order], u[order], perr[order], kind[order]
    nn[: n // 2] = 0
    return p, nn, u, perr, kind


def fixture_directions(n=N_FIXTURE, seed=6):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
