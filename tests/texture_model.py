"""Image textures on diffuse reflectance (csrc/vspg_texture.h): a float32 NumPy mirror of the device's seven steps and of both uv
functions, operation by operation, and beside it a float64 statement of the mathematics -- the exact bilinear interpolant of the
wrapped texel lattice (the nearest texel for "point").  `planted` names one of five errors the tests must be able to see."""
import numpy as np

f32, f64 = np.float32, np.float64
EPS = 2.0 ** -24
REPEAT, CLAMP, BLACK = 0, 1, 2
POINT, BILINEAR = 0, 1
PLANTED = ("no_flip", "no_half", "trunc", "c_mod", "scale_after_invert")
DEFAULT_TRI_UV = np.array([0, 0, 1, 0, 1, 1], f32)


class Texture:
    """image: [yres, xres] / [yres, xres, 1] (grey, broadcast) or [yres, xres, 3] float32, top row first."""

    def __init__(self, image, filter=BILINEAR, wrap=REPEAT, scale=1.0, invert=False, su=1.0, sv=1.0, du=0.0, dv=0.0):
        img = np.asarray(image, f32)
        if img.ndim == 2:
            img = img[..., None]
        self.image = np.ascontiguousarray(np.broadcast_to(img, img.shape[:2] + (3,)), f32)
        self.yres, self.xres = self.image.shape[:2]
        self.filter, self.wrap, self.invert = filter, wrap, bool(invert)
        self.scale, self.su, self.sv, self.du, self.dv = (f32(x) for x in (scale, su, sv, du, dv))

    def device_image(self):
        """What the host builds: one float4 {R, G, B, 0} per texel."""
        out = np.zeros((self.yres, self.xres, 4), f32)
        out[..., :3] = self.image
        return out


# ---- the (u, v) of a hit ---------------------------------------------------------------------------------------------------------
def uv_quad(p00, e1, e2, p):
    """u = (d.x e1.x + d.y e1.y + d.z e1.z) * inv_l1, d = p - p00, inv_l1 = 1 / (e1.x^2 + e1.y^2 + e1.z^2); likewise v with e2."""
    p00, e1, e2 = (np.asarray(a, f32) for a in (p00, e1, e2))
    d = np.asarray(p, f32).reshape(-1, 3) - p00

    def one(e):
        inv = f32(1) / ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        return ((d[:, 0] * e[0] + d[:, 1] * e[1]) + d[:, 2] * e[2]) * inv
    return one(e1), one(e2)


def uv_tri(uv6, b):
    """uv = b0 uv0 + b1 uv1 + b2 uv2 per component, summed left to right."""
    uv6 = np.asarray(uv6, f32).reshape(6)
    b = np.asarray(b, f32).reshape(-1, 3)
    return ((b[:, 0] * uv6[0] + b[:, 1] * uv6[2]) + b[:, 2] * uv6[4]), ((b[:, 0] * uv6[1] + b[:, 1] * uv6[3]) + b[:, 2] * uv6[5])


# ---- the wrap ----------------------------------------------------------------------------------------------------------------------
def pbrt_mod(a, b):
    r = np.fmod(a, b)  # C's %: the sign of a
    return np.where(r < 0, r + b, r)


def wrap_coord(p, res, wrap, planted=None):
    """RemapPixelCoords on one coordinate: (index inside the image, whether the texel counts)."""
    inside = (p >= 0) & (p < res)
    if wrap == REPEAT:
        if planted == "c_mod":
            r = np.fmod(p, res)
            return np.where(r < 0, 0, r), r >= 0  # (C would read in front of the row: the model counts such a texel as 0)
        return pbrt_mod(p, res), np.ones(p.shape, bool)
    return np.clip(p, 0, res - 1), inside | (wrap == CLAMP)


def round_half_away(x):
    x = x.astype(f64)
    return np.trunc(x + np.copysign(0.5, x)).astype(np.int64)  # exact: x + 0.5 of a float is a double


def tex_coord(x):
    """A texel coordinate held to [-1e9, 1e9] (NaN: 0) before it becomes an integer, as the device holds it."""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), f32(0), np.clip(x, f32(-1e9), f32(1e9))).astype(f32)


# ---- the float32 mirror --------------------------------------------------------------------------------------------------------------
def lookup(tex, u, v, planted=None):
    """Steps 1-7 in float32.  Returns (s, t, R [n, 3], has_lobes)."""
    u, v = np.asarray(u, f32).reshape(-1), np.asarray(v, f32).reshape(-1)
    s = tex.su * u + tex.du
    t = tex.sv * v + tex.dv
    if planted != "no_flip":
        t = f32(1) - t
    half = f32(0.0 if planted == "no_half" else 0.5)
    x, y = tex_coord(s * f32(tex.xres) - half), tex_coord(t * f32(tex.yres) - half)
    img = tex.image
    if tex.filter == POINT:
        xi, cx = wrap_coord(round_half_away(x), tex.xres, tex.wrap, planted)
        yi, cy = wrap_coord(round_half_away(y), tex.yres, tex.wrap, planted)
        f = np.where((cx & cy)[:, None], img[yi, xi], f32(0))
    else:
        fl = np.trunc if planted == "trunc" else np.floor
        xi, yi = fl(x).astype(np.int64), fl(y).astype(np.int64)
        dx, dy = x - xi.astype(f32), y - yi.astype(f32)
        x0, cx0 = wrap_coord(xi, tex.xres, tex.wrap, planted)
        x1, cx1 = wrap_coord(xi + 1, tex.xres, tex.wrap, planted)
        y0, cy0 = wrap_coord(yi, tex.yres, tex.wrap, planted)
        y1, cy1 = wrap_coord(yi + 1, tex.yres, tex.wrap, planted)
        one = f32(1)
        w = [(one - dx) * (one - dy), dx * (one - dy), (one - dx) * dy, dx * dy]
        vals = [np.where((c)[:, None], img[yy, xx], f32(0)) for yy, xx, c in ((y0, x0, cx0 & cy0), (y0, x1, cx1 & cy0), (y1, x0, cx0 & cy1), (y1, x1, cx1 & cy1))]
        f = ((w[0][:, None] * vals[0] + w[1][:, None] * vals[1]) + w[2][:, None] * vals[2]) + w[3][:, None] * vals[3]
    f = f.astype(f32)
    if planted == "scale_after_invert":
        rgb = tex.scale * (f32(1) - f if tex.invert else f)
    else:
        rgb = tex.scale * f
        if tex.invert:
            rgb = f32(1) - rgb
    rgb = np.where(f32(0) < rgb, rgb, f32(0))                            # ClampZero: std::max(0, x)
    R = np.where(rgb < 0, f32(0), np.where(rgb > 1, f32(1), rgb)).astype(f32)  # Clamp(x, 0, 1)
    return s.astype(f32), t.astype(f32), R, np.any(R != 0, axis=1)


# ---- the float64 statement -----------------------------------------------------------------------------------------------------------
def statement(tex, u, v):
    """The mathematics in double: st from the float inputs, the bilinear interpolant of the wrapped lattice (texel centres at
    (i + 0.5) / res) or the nearest texel, scale, invert, both clamps.  Returns (R [n, 3], distance of (x, y) from the nearest point at
    which the point filter's choice changes -- texel edges -- in texels)."""
    u, v = np.asarray(u, f32).astype(f64).reshape(-1), np.asarray(v, f32).astype(f64).reshape(-1)
    s = f64(tex.su) * u + f64(tex.du)
    t = 1.0 - (f64(tex.sv) * v + f64(tex.dv))
    x, y = s * tex.xres - 0.5, t * tex.yres - 0.5
    img = tex.image.astype(f64)

    def texel(xi, yi):
        xx, cx = wrap_coord(xi, tex.xres, tex.wrap)
        yy, cy = wrap_coord(yi, tex.yres, tex.wrap)
        return np.where((cx & cy)[:, None], img[yy, xx], 0.0)
    edge = np.minimum(np.abs(x - np.floor(x) - 0.5), np.abs(y - np.floor(y) - 0.5))
    if tex.filter == POINT:
        f = texel(round_half_away(x), round_half_away(y))
    else:
        xi, yi = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
        dx, dy = (x - xi)[:, None], (y - yi)[:, None]
        f = (1 - dx) * (1 - dy) * texel(xi, yi) + dx * (1 - dy) * texel(xi + 1, yi) + (1 - dx) * dy * texel(xi, yi + 1) + dx * dy * texel(xi + 1, yi + 1)
    rgb = f64(tex.scale) * f
    if tex.invert:
        rgb = 1.0 - rgb
    return np.clip(np.maximum(rgb, 0.0), 0.0, 1.0), edge


def error_bound(tex, u, v):
    """How far the mirror may lie from the statement, from the operation count (EPS = 2^-24, one rounding = a relative EPS):
      s, t    a product and a sum (and the flip): |err| <= 3 EPS M with M = |su u| + |du| + 1 (likewise v)
      x       st * res - 0.5: |err_x| <= res * err_s + 2 EPS (|x| + 0.5); xi is exact, dx = x - xi adds one rounding of a value below 1
      f       the interpolant moves by at most D = (the largest difference of two texels next to each other, zeros outside under black
              included) per texel of x and of y: D (err_x + err_y + 2 EPS); its own arithmetic is four weights of two roundings, four
              products and three sums on values of at most V = max |texel|: 12 EPS V
      R       scale and invert are two more roundings of values of at most |scale| V + 1; the clamps move nothing apart
    The bound is per element and generous by small factors only; it holds for both filters away from the point filter's jumps."""
    u, v = np.abs(np.asarray(u, f64)).reshape(-1), np.abs(np.asarray(v, f64)).reshape(-1)
    V = float(np.abs(tex.image).max())
    D = 2 * V if tex.wrap != CLAMP else float(max(np.abs(np.diff(tex.image, axis=0)).max(initial=0), np.abs(np.diff(tex.image, axis=1)).max(initial=0), V))
    D = max(D, V)
    Ms, Mt = abs(float(tex.su)) * u + abs(float(tex.du)) + 1, abs(float(tex.sv)) * v + abs(float(tex.dv)) + 1
    ex = tex.xres * 3 * EPS * Ms + 2 * EPS * (tex.xres * Ms + 1)
    ey = tex.yres * 3 * EPS * Mt + 2 * EPS * (tex.yres * Mt + 1)
    sc = abs(float(tex.scale))
    return sc * (D * (ex + ey + 2 * EPS) + 12 * EPS * V) + 2 * EPS * (sc * V + 1)
