"""Projection and goniometric lights restated from the reference's text (src/pbrt/lights.h:342-455; lights.cpp:319-441, 490-624, 652-734;
util/transform.cpp:35-45 Scale, :119-131 Perspective; util/transform.h:310-319, 401-406; util/math.h:1571-1624 Inverse;
util/vecmath.h:1228-1240 Lerp / Offset, :1454-1456 Inside; util/image.h:352-356 LookupNearestChannel, :136-138 the clamp wrap).

Two statements of the same mathematics, as in tests/pointlight_model.py (whose exact-FMA matrix product and transform helpers serve here):
  * a float32 NumPy MIRROR -- one rounding per operation, in the reference's order of operations; what the device computes bit for bit
    (tests/test_imagelight_gpu.py) and what the host's table builder and transform helpers compute;
  * a float64 STATEMENT (suffix 64) of what those operations mean.
tanf and cosf come from the running libm, through ctypes; the equal-area mapping is tests/envlight_model.py's.

`planted` names a deliberate error, for the tests that show each of them is caught:
  no_flip   the projection's Scale(1, -1, 1) is missing        use_m     m instead of mInv
  round     the texel index rounded instead of truncated       octa      the octahedral wrap instead of the clamp (goniometric)
  no_hither no `w.z < hither` test (projection)
"""
import ctypes as C
import math

import numpy as np

import envlight_model as E
import pointlight_model as PM

f32 = np.float32
PI = PM.PI
LIGHT_PROJECTION, LIGHT_GONIOMETRIC = 5, 6
PLANTED = ("no_flip", "use_m", "round", "octa", "no_hither")
HITHER = f32(1e-3)

PM._libm.tanf.restype = C.c_float
PM._libm.tanf.argtypes = [C.c_float]


def tanf(x):
    return f32(PM._libm.tanf(float(f32(x))))


FLIP_Y = np.diag([1, -1, 1, 1]).astype(f32)                                                  # Scale(1, -1, 1): its own inverse
SWAP_YZ = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], f32)            # lights.cpp:724: its own inverse


def projection_transform(ctm=None):
    """ProjectionLight::Create (lights.cpp:555-556): ctm * Scale(1, -1, 1), and the inverse."""
    return PM.compose(ctm, FLIP_Y.copy(), FLIP_Y.copy())


def goniometric_transform(ctm=None):
    """GoniometricLight::Create (lights.cpp:724-726): ctm * swapYZ, and the inverse."""
    return PM.compose(ctm, SWAP_YZ.copy(), SWAP_YZ.copy())


def _apply_inverse(M, w):
    """ApplyInverse(Vector3f) (transform.h:401-406): the linear part, the sums as written."""
    return np.stack([(M[k, 0] * w[:, 0] + M[k, 1] * w[:, 1]) + M[k, 2] * w[:, 2] for k in range(3)], axis=1).astype(f32)


class Perspective:
    """Perspective(fov, 1e-3, 1e30) (transform.cpp:119-131) and its inverse, float32.  Next to exact zeros and ones every entry of the
    FMA products is one factor as it stands; of Inverse(persp)'s 2 x 2 sub-determinants only s0 = 1 and c5 = -b are not zero."""

    def __init__(self, fov):
        n, f = HITHER, f32(1e30)
        self.a, self.b = f / (f - n), -f * n / (f - n)
        self.half = ((PI / f32(180)) * f32(fov)) / f32(2)
        self.inv_tan = f32(1) / tanf(self.half)
        self.m = np.zeros((4, 4), f32)                       # screenFromLight
        self.m[0, 0] = self.m[1, 1] = self.inv_tan
        self.m[2, 2], self.m[2, 3], self.m[3, 2] = self.a, self.b, f32(1)
        det = -self.b
        s = f32(1) / det
        one = s * -self.b
        self.mi = np.zeros((4, 4), f32)                      # lightFromScreen
        self.mi[0, 0] = self.mi[1, 1] = one * (f32(1) / self.inv_tan)
        self.mi[2, 3], self.mi[3, 2], self.mi[3, 3] = one, -s, s * self.a

    def screen_dir(self, x, y):
        """Normalize(Vector3f(lightFromScreen(Point3f(x, y, 0)))): [n, 3] float32."""
        x, y = np.asarray(x, f32).reshape(-1), np.asarray(y, f32).reshape(-1)
        L = self.mi
        z0 = f32(0)
        xp = ((L[0, 0] * x + L[0, 1] * y) + L[0, 2] * z0) + L[0, 3]
        yp = ((L[1, 0] * x + L[1, 1] * y) + L[1, 2] * z0) + L[1, 3]
        zp = ((L[2, 0] * x + L[2, 1] * y) + L[2, 2] * z0) + L[2, 3]
        wp = ((L[3, 0] * x + L[3, 1] * y) + L[3, 2] * z0) + L[3, 3]
        v = np.stack([xp, yp, zp], axis=1).astype(f32)
        v = np.where((wp == 1)[:, None], v, v / wp[:, None]).astype(f32)
        return PM.normalize32(v)


def sphere_to_square64(d):
    """EqualAreaSphereToSquare (util/math.cpp:317-361) as it is written -- the degree-6 polynomial for atan included, which is off from
    atan by up to 4e-6: the statement says what the reference's formula means, not what another formula would -- in float64."""
    d = np.asarray(d, np.float64).reshape(-1, 3)
    x, y, z = np.abs(d[:, 0]), np.abs(d[:, 1]), np.abs(d[:, 2])
    r = np.sqrt(np.maximum(0.0, 1.0 - z))
    a, b = np.maximum(x, y), np.minimum(x, y)
    b = np.where(a == 0, 0.0, b / np.where(a == 0, 1.0, a))
    phi = np.zeros_like(b)
    for c in E.T_COEF[::-1]:
        phi = phi * b + float(c)
    phi = np.where(x < y, 1 - phi, phi)
    v = phi * r
    u = r - v
    south = d[:, 2] < 0
    u, v = np.where(south, 1 - v, u), np.where(south, 1 - u, v)
    return np.stack([0.5 * (np.copysign(u, d[:, 0]) + 1), 0.5 * (np.copysign(v, d[:, 1]) + 1)], axis=1)


def octa_remap(px, py, res):
    return E.remap(px, py, res)


class ImageLight:
    """A projection or goniometric light as the library holds it: I multiplied out, both matrices, the image."""

    def __init__(self, kind, I, m, mi, image, fov=90.0):
        self.kind = kind
        self.I = np.asarray(I, f32)
        self.m, self.mi = np.asarray(m, f32).reshape(4, 4), np.asarray(mi, f32).reshape(4, 4)
        m_ = self.m
        q = [((m_[k, 0] * f32(0) + m_[k, 1] * f32(0)) + m_[k, 2] * f32(0)) + m_[k, 3] for k in range(4)]
        self.pos = np.array([q[k] if q[3] == 1 else q[k] / q[3] for k in range(3)], f32)
        self.axis = PM.normalize32(np.array([(m_[k, 0] * f32(0) + m_[k, 1] * f32(0)) + m_[k, 2] * f32(1) for k in range(3)], f32))
        self.set_image(image, fov)

    def set_image(self, image, fov=None):
        img = np.asarray(image, f32)
        if self.kind == LIGHT_PROJECTION:
            assert img.ndim == 3 and img.shape[2] == 3
            self.fov = self.fov if fov is None else fov
            self.raw = img
            self.texels = np.where(f32(0) < img, img, f32(0)).astype(f32)          # ClampZero: std::max<Float>(0, v)
            self.yres, self.xres = img.shape[:2]
            aspect = f32(self.xres) / f32(self.yres)
            self.aspect = aspect
            if aspect > 1:
                self.sb = np.array([-aspect, -1, aspect, 1], f32)
            else:
                self.sb = np.array([-1, f32(-1) / aspect, 1, f32(1) / aspect], f32)
            self.persp = Perspective(self.fov)
            opposite = tanf(self.persp.half)
            self.A = f32(4) * (opposite * opposite) * (aspect if aspect > 1 else f32(1) / aspect)
        else:
            img = img.reshape(img.shape[0], img.shape[1])
            assert img.shape[0] == img.shape[1]
            self.raw = self.texels = img
            self.yres, self.xres = img.shape

    def device_image(self):
        """The bytes the host uploads: a float4 per texel with a zero pad (projection), the texels as given (goniometric)."""
        if self.kind == LIGHT_GONIOMETRIC:
            return np.ascontiguousarray(self.texels, f32)
        out = np.zeros((self.yres, self.xres, 4), f32)
        out[..., :3] = self.texels
        return out

    # ---- SampleLi ----
    def texel_index(self, ctx_p, planted=None):
        """(inside, ix, iy, wl) per context: the texel the light shows towards ctx_p (inside = it shows one)."""
        p = np.asarray(ctx_p, f32).reshape(-1, 3)
        d = self.pos[None, :] - p
        l2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        wi = d / np.sqrt(l2)[:, None]
        M = self.m if planted == "use_m" else self.mi
        if planted == "no_flip" and self.kind == LIGHT_PROJECTION:
            M = PM.mat4_mul(FLIP_Y, M)      # undo the flip in front of mInv = flip * ctm^-1
        wl = _apply_inverse(M, -wi)

        def index(uv, res):
            t = uv * f32(res)
            i = np.floor(t + f32(0.5)) if planted == "round" else np.trunc(t)
            return i.astype(np.int64)
        with np.errstate(all="ignore"):
            if self.kind == LIGHT_GONIOMETRIC:
                u, v = E.sphere_to_square(wl)
                ix, iy = index(u, self.xres), index(v, self.yres)
                if planted == "octa":
                    ix, iy = octa_remap(ix, iy, self.xres)
                inside = np.ones(len(p), bool)
            else:
                S = self.persp.m
                xp = ((S[0, 0] * wl[:, 0] + S[0, 1] * wl[:, 1]) + S[0, 2] * wl[:, 2]) + S[0, 3]
                yp = ((S[1, 0] * wl[:, 0] + S[1, 1] * wl[:, 1]) + S[1, 2] * wl[:, 2]) + S[1, 3]
                wp = ((S[3, 0] * wl[:, 0] + S[3, 1] * wl[:, 1]) + S[3, 2] * wl[:, 2]) + S[3, 3]
                xp = np.where(wp == 1, xp, xp / wp).astype(f32)
                yp = np.where(wp == 1, yp, yp / wp).astype(f32)
                sb = self.sb
                inside = (xp >= sb[0]) & (xp <= sb[2]) & (yp >= sb[1]) & (yp <= sb[3])
                if planted != "no_hither":
                    inside &= ~(wl[:, 2] < HITHER)
                ox = (xp - sb[0]) / (sb[2] - sb[0])
                oy = (yp - sb[1]) / (sb[3] - sb[1])
                ox, oy = np.where(inside, ox, f32(0)).astype(f32), np.where(inside, oy, f32(0)).astype(f32)
                ix, iy = index(ox, self.xres), index(oy, self.yres)
        ix, iy = np.clip(ix, 0, self.xres - 1), np.clip(iy, 0, self.yres - 1)
        return inside, ix, iy, wl, wi.astype(f32), l2

    def sample_li(self, ctx_p, planted=None):
        """(valid, wi, L, pdf, pLight, delta) for contexts ctx_p (n, 3), float32, the reference's order of operations."""
        p = np.asarray(ctx_p, f32).reshape(-1, 3)
        inside, ix, iy, wl, wi, l2 = self.texel_index(p, planted)
        if self.kind == LIGHT_GONIOMETRIC:
            t = self.texels[iy, ix]
            L = (self.I[None, :] * t[:, None]) / l2[:, None]
            valid = np.ones(len(p), bool)                                              # a sample is always returned
        else:
            rgb = np.where(inside[:, None], self.texels[iy, ix], f32(0)).astype(f32)
            L = (self.I[None, :] * rgb) / l2[:, None]
            valid = np.any(L != 0, axis=1)                                             # `if (!Li) return {}`
        return valid, wi, L.astype(f32), np.ones(len(p), f32), np.broadcast_to(self.pos, p.shape).astype(f32), np.ones(len(p), f32)

    def texel_index64(self, ctx_p, planted=None):
        """The float64 statement of which texel: (inside, ix, iy)."""
        p = np.asarray(ctx_p, np.float64).reshape(-1, 3)
        pos = self.m[:3, 3].astype(np.float64)
        d = pos[None, :] - p
        wi = d / np.linalg.norm(d, axis=1, keepdims=True)
        Mx = (self.m if planted == "use_m" else self.mi)[:3, :3].astype(np.float64)
        if planted == "no_flip" and self.kind == LIGHT_PROJECTION:
            Mx = FLIP_Y[:3, :3].astype(np.float64) @ Mx
        wl = -wi @ Mx.T
        if self.kind == LIGHT_GONIOMETRIC:
            uv = sphere_to_square64(wl / np.linalg.norm(wl, axis=1, keepdims=True))
            ix, iy = np.trunc(uv[:, 0] * self.xres), np.trunc(uv[:, 1] * self.yres)
            inside = np.ones(len(p), bool)
        else:
            t = 1.0 / math.tan(math.radians(self.fov) / 2)
            with np.errstate(all="ignore"):
                x, y = t * wl[:, 0] / wl[:, 2], t * wl[:, 1] / wl[:, 2]
            sb = self.sb.astype(np.float64)
            inside = (wl[:, 2] >= float(HITHER)) & (x >= sb[0]) & (x <= sb[2]) & (y >= sb[1]) & (y <= sb[3])
            with np.errstate(all="ignore"):
                ix = np.trunc(np.where(inside, (x - sb[0]) / (sb[2] - sb[0]), 0) * self.xres)
                iy = np.trunc(np.where(inside, (y - sb[1]) / (sb[3] - sb[1]), 0) * self.yres)
        return inside, np.clip(ix, 0, self.xres - 1).astype(np.int64), np.clip(iy, 0, self.yres - 1).astype(np.int64)

    def sample_li64(self, ctx_p, planted=None):
        """The float64 statement: wi = (pos - p) / |pos - p|, L = I * texel(direction) / |pos - p|^2."""
        p = np.asarray(ctx_p, np.float64).reshape(-1, 3)
        pos = self.m[:3, 3].astype(np.float64)
        d = pos[None, :] - p
        l2 = (d * d).sum(axis=1)
        inside, ix, iy = self.texel_index64(ctx_p, planted)
        t = self.texels.astype(np.float64)[iy, ix]
        if self.kind == LIGHT_GONIOMETRIC:
            t = t[:, None]
        else:
            t = np.where(inside[:, None], t, 0.0)
        return d / np.sqrt(l2)[:, None], self.I.astype(np.float64)[None, :] * t / l2[:, None]

    # ---- Phi / Bounds ----
    def _sums(self):
        """Projection: (per channel sum of ClampZero(texel) * dwdA, sum of max(R, G, B) of the raw texels), sequential in image order."""
        ys, xs = np.mgrid[0:self.yres, 0:self.xres]
        tx = ((xs.astype(f32) + f32(0.5)) / f32(self.xres)).astype(f32).reshape(-1)
        ty = ((ys.astype(f32) + f32(0.5)) / f32(self.yres)).astype(f32).reshape(-1)
        sb = self.sb
        px = (f32(1) - tx) * sb[0] + tx * sb[2]
        py = (f32(1) - ty) * sb[1] + ty * sb[3]
        c = self.persp.screen_dir(px, py)[:, 2]
        dwdA = (c * c) * c
        tex = self.texels.reshape(-1, 3)
        s = np.zeros(3, f32)
        for i in range(len(dwdA)):
            s = (s + tex[i] * dwdA[i]).astype(f32)
        mx = f32(0)
        for v in self.raw.reshape(-1, 3).max(axis=1):
            mx = mx + v
        return s, mx

    def _sum_y(self):
        s = f32(0)
        for v in self.raw.reshape(-1):
            s = s + v
        return s

    def phi(self):
        """ProjectionLight::Phi (lights.cpp:404-424) per channel of I; GoniometricLight::Phi (:603-610).  RGB, float32."""
        n = f32(self.xres * self.yres)
        if self.kind == LIGHT_GONIOMETRIC:
            return self.I * f32(4) * PI * self._sum_y() / n
        s, _ = self._sums()
        return self.I * self.A * s / n

    def cos_total_width(self):
        return self.persp.screen_dir([self.sb[2]], [self.sb[3]])[0, 2]

    def bounds(self):
        """(p, w, phi, cosTheta_o, cosTheta_e) of ProjectionLight::Bounds (lights.cpp:426-441) / GoniometricLight::Bounds (:612-624)."""
        mx, n = f32(max(self.I)), f32(self.xres * self.yres)
        if self.kind == LIGHT_GONIOMETRIC:
            return self.pos, np.array([0, 0, 1], f32), mx * f32(4) * PI * self._sum_y() / n, PM.cosf(PI), PM.cosf(PI / f32(2))
        _, smax = self._sums()
        return self.pos, self.axis, mx * smax / n, PM.cosf(f32(0)), self.cos_total_width()


def projection_light(I, image, fov=90.0, ctm=None):
    m, mi = projection_transform(ctm)
    return ImageLight(LIGHT_PROJECTION, np.asarray(I, f32), m, mi, image, fov)


def goniometric_light(I, image=None, scale=1.0, power=None, ctm=None):
    img = np.ones((1, 1), f32) if image is None else np.asarray(image, f32)
    sc = f32(scale)
    if power is not None and power > 0:          # lights.cpp:714-722
        s = f32(0)
        for v in img.reshape(-1):
            s = s + v
        sc = sc * (f32(power) / (f32(4) * PI * s / f32(img.size)))
    m, mi = goniometric_transform(ctm)
    return ImageLight(LIGHT_GONIOMETRIC, np.asarray(I, f32) * sc, m, mi, img)


# ---- images and contexts for the tests ------------------------------------------------------------------------------------------------
def slide(xres, yres, seed=0):
    """A slide with distinct texels, a few of them negative (ClampZero) and zero."""
    rng = np.random.default_rng(seed)
    img = rng.uniform(0.25, 4.0, (yres, xres, 3)).astype(f32)
    if xres * yres >= 4:
        img[0, 0, 1] = -0.5
        img[-1, -1] = (0.0, -1.0, 0.0)
    return img


def gonio_map(res, seed=0):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.1, 3.0, (res, res)).astype(f32)


def contexts_around(light, n, seed):
    """n contexts around a light, regime by regime (returned as labels): for a projection light inside the frustum, outside it on each
    of the four sides, behind the light, within 1e-6 (relative) of a texel edge and of the screen edge; for a goniometric light
    uniform directions and directions within 1e-6 of a texel edge.  Distances from 0.05 to 20, every seventh 1e-3 and every (7k + 3)rd
    1e3 units.  The first half are medium vertices (normal 0), the rest surface contexts."""
    rng = np.random.default_rng(seed)
    labels = np.zeros(n, np.int64)
    if light.kind == LIGHT_PROJECTION:
        sb = light.sb.astype(np.float64)
        t = 1.0 / math.tan(math.radians(light.fov) / 2)
        k, ke = n // 8, max(1, n * 7 // 128)                                                       # (224 of 4096 per edge regime: the cap on flipped texels)
        x, y = rng.uniform(sb[0], sb[2], n), rng.uniform(sb[1], sb[3], n)                       # 0: inside
        wx, wy = sb[2] - sb[0], sb[3] - sb[1]
        x[k:2 * k] = sb[0] - rng.uniform(1e-3, 2, k) * wx; labels[k:2 * k] = 1                   # 1..4: outside, one side each
        x[2 * k:3 * k] = sb[2] + rng.uniform(1e-3, 2, k) * wx; labels[2 * k:3 * k] = 2
        y[3 * k:4 * k] = sb[1] - rng.uniform(1e-3, 2, k) * wy; labels[3 * k:4 * k] = 3
        y[4 * k:5 * k] = sb[3] + rng.uniform(1e-3, 2, k) * wy; labels[4 * k:5 * k] = 4
        e = slice(6 * k, 6 * k + ke)                                                             # 6: at a texel edge
        ex = sb[0] + wx * rng.integers(1, max(2, light.xres), ke) / light.xres
        on_x = rng.random(ke) < 0.5
        x[e] = np.where(on_x, ex * (1 + rng.uniform(-1e-6, 1e-6, ke)), x[e])
        ey = sb[1] + wy * rng.integers(1, max(2, light.yres), ke) / light.yres
        y[e] = np.where(on_x, y[e], ey * (1 + rng.uniform(-1e-6, 1e-6, ke)))
        labels[e] = 6
        s = slice(6 * k + ke, 6 * k + 2 * ke)                                                    # 7: at the screen edge
        side = rng.integers(0, 4, ke)
        jit = 1 + rng.uniform(-1e-6, 1e-6, ke)
        x[s] = np.where(side == 0, sb[0] * jit, np.where(side == 1, sb[2] * jit, x[s]))
        y[s] = np.where(side == 2, sb[1] * jit, np.where(side == 3, sb[3] * jit, y[s]))
        labels[s] = 7
        local = np.stack([x / t, y / t, np.ones(n)], axis=1)
        local[5 * k:6 * k, 2] = -rng.uniform(0.0, 2.0, k)                                        # 5: behind the light
        local[5 * k:5 * k + k // 4, 2] = rng.uniform(-2e-3, 2e-3, k // 4) * np.linalg.norm(local[5 * k:5 * k + k // 4, :2], axis=1)      # ... around hither
        labels[5 * k:6 * k] = 5
        local /= np.linalg.norm(local, axis=1, keepdims=True)
    else:
        local = rng.normal(size=(n, 3))
        local /= np.linalg.norm(local, axis=1, keepdims=True)
        k = max(1, n * 7 // 128)
        uv = rng.random((k, 2))
        edge = rng.integers(1, max(2, light.xres), k) / light.xres * (1 + rng.uniform(-1e-6, 1e-6, k))
        which = rng.random(k) < 0.5
        uv[:, 0] = np.where(which, edge, uv[:, 0])
        uv[:, 1] = np.where(which, uv[:, 1], edge)
        local[:k] = E.square_to_sphere_exact(np.clip(uv, 0, 1))
        labels[:k] = 6
    d = local @ light.m[:3, :3].astype(np.float64).T
    r = np.exp(rng.uniform(math.log(0.05), math.log(20.0), n))
    r[::7] = 1e-3
    r[3::7] = 1e3
    order = rng.permutation(n)
    p = (light.pos.astype(np.float64) + d * r[:, None]).astype(f32)[order]
    nn = rng.normal(size=(n, 3))
    nn = (nn / np.linalg.norm(nn, axis=1, keepdims=True)).astype(f32)
    nn[: n // 2] = 0
    return p, nn, rng.random((n, 3)).astype(f32), labels[order]


# ---- a projector in fog: single scattering by next-event estimation, float64 (tests/test_imagelight_gpu.py, the statistical known answer) --
class FogProjector(PM.FogSpot):
    """tests/pointlight_model.py::FogSpot with the spot replaced by a projector: the same homogeneous grey medium, pinhole camera, black
    backdrop and maxdepth 1, the same integrand with I(w) = I * texel(w).  The projector hangs 0.8 above the camera, tilted 12 degrees down
    so that its beam crosses the camera's view, and ROLLED by 45 degrees about its axis -- under a roll m and mInv turn the slide in
    opposite senses, which the flip alone (its own inverse) would not show.  The camera looks along the beam: the film's quadrants see
    different mixtures of the 2 x 2 slide's four colours."""
    I = (1.0, 1.0, 1.0)
    SLIDE = np.array([[[3, 1, 0.5], [1, 6, 2]], [[0.5, 1, 12], [8, 8, 8]]], f32)
    proj_fov = 40.0
    eye, look, up = (0.0, 0.0, -3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)
    fov = 14.0
    z_wall = 2.0

    @staticmethod
    def ctm():
        return PM.mat4_mul(PM.mat4_mul(PM.translate((0.0, 0.8, -3.0)), PM.rotate(12.0, (1, 0, 0))), PM.rotate(45.0, (0, 0, 1)))

    def __init__(self):
        PM.FogSpot.__init__(self)
        self.light = projection_light(self.I, self.SLIDE, self.proj_fov, self.ctm())
