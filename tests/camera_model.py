"""A model of the camera rays, written from the reference's text (src/pbrt/cameras.cpp: PerspectiveCamera::GenerateRay :410-433,
OrthographicCamera::GenerateRay :290-312, SphericalCamera::GenerateRay :616-636; SampleUniformDiskConcentric util/sampling.h:325-341;
SphericalDirection util/vecmath.h:1666-1672; WrapEqualAreaSquare util/math.cpp:363-379), not a port of the device code:

  * a FLOAT32 MIRROR (generate_ray): every operation is one IEEE float32 operation in the reference's order.  No operation is
    fused -- the reference calls no FMA in these functions and is built without contraction -- so every product-sum below is a rounded
    product followed by a rounded sum, left to right.  sinf and cosf are the C library's (envlight_model's ctypes calls;
    tests/test_libm_model.py holds the device's pair to them through tests/libm_model_shim.cpp); the equal-area map is envlight_model's.
    tests/test_camera_gpu.py compares the device with this mirror bit for bit.
  * a FLOAT64 STATEMENT of the same mathematics (generate_ray64): exact sin / cos, the thin lens as geometry.
  * the camera sample's variates from the oracle's bit-pinned IndependentSampler: wavelength, filter 2, time, lens 2.

The project's camera record (VspgCamera) stands for cameraFromRaster and renderFromCamera: raster (x, y) -> (sx x + ox, sy y + oy) and
the frame (right, up, fwd) at `origin`.  Render space: ro = origin + ((o.x right + o.y up) + o.z fwd) -- `origin` itself where o is the
camera-space origin --, rd = (d.x right + d.y up) + d.z fwd.

The planted errors of tests/test_camera_model.py are switches of the mirror (`plant`):
  'lens_plus_pcamera'  the lens origin added to pCamera instead of replacing it
  'ft_no_divide'       ft = focalDistance without the division by d.z
  'no_yz_swap'         the spherical direction without swap(dir.y, dir.z)
  'uv_reciprocal'      uv = pFilm * (1 / resolution) instead of the division
  'wrong_dims'         the lens variates taken from sampler dimensions 3 and 4 (time and lens x) instead of 4 and 5"""
import ctypes as C

import numpy as np

import envlight_model as EM

f32 = np.float32
PI = EM.PI
PI_OVER_2 = f32(1.57079632679489661923)
PI_OVER_4 = f32(0.78539816339744830961)
PERSPECTIVE, ORTHOGRAPHIC, SPHERICAL_EQUALAREA, SPHERICAL_EQUIRECT = 0, 1, 2, 3
MODELS = (PERSPECTIVE, ORTHOGRAPHIC, SPHERICAL_EQUALAREA, SPHERICAL_EQUIRECT)


class Camera:
    """The camera record: origin, right, up, fwd (float32 [3]), the raster map, the model and its lens, the full resolution."""

    def __init__(self, origin, right, up, fwd, sx, ox, sy, oy, model, xres, yres, lens_radius=0.0, focal_distance=1e6):
        self.origin, self.right, self.up, self.fwd = (np.asarray(v, f32).reshape(3) for v in (origin, right, up, fwd))
        self.sx, self.ox, self.sy, self.oy = f32(sx), f32(ox), f32(sy), f32(oy)
        self.model, self.xres, self.yres = int(model), int(xres), int(yres)
        self.lens_radius, self.focal_distance = f32(lens_radius), f32(focal_distance)

    @classmethod
    def from_c(cls, cam, model, xres, yres, lens_radius=0.0, focal_distance=1e6):
        """From a VspgCamera (ctypes)."""
        return cls(list(cam.origin), list(cam.right), list(cam.up), list(cam.fwd), cam.sx, cam.ox, cam.sy, cam.oy, model, xres, yres,
                   lens_radius, focal_distance)

    @property
    def has_lens(self):
        return self.model in (PERSPECTIVE, ORTHOGRAPHIC) and self.lens_radius > 0


# ---------------------------------------------------------------------------------------------------------------------------
# the camera sample
def raster_point(px, py, f0, f1):
    """GetCameraSample (samplers.h:796-815) under BoxFilter radius .5 (filters.h:67-69): pFilm = pPixel + Lerp(u, -r, r) + 0.5."""
    px, py = np.asarray(px, np.int64).reshape(-1), np.asarray(py, np.int64).reshape(-1)
    f0, f1 = np.asarray(f0, f32).reshape(-1), np.asarray(f1, f32).reshape(-1)
    fx = ((f32(1) - f0) * f32(-0.5)).astype(f32) + (f0 * f32(0.5)).astype(f32)
    fy = ((f32(1) - f1) * f32(-0.5)).astype(f32) + (f1 * f32(0.5)).astype(f32)
    return ((px.astype(f32) + fx).astype(f32) + f32(0.5)).astype(f32), ((py.astype(f32) + fy).astype(f32) + f32(0.5)).astype(f32)


def sampler_variates(oracle, pixel_xy, sample_index, seed=0, plant=()):
    """[n, 4] float32 (filter u0 u1, lens u0 u1) of IndependentSampler's dimensions 1, 2 and 4, 5 (0 = wavelength, 3 = time)."""
    pix = np.asarray(pixel_xy, np.int32).reshape(-1, 2)
    si = np.asarray(sample_index, np.int32).reshape(-1)
    out = np.zeros((len(si), 4), f32)
    buf = (C.c_float * 6)()
    lens = (3, 4) if "wrong_dims" in plant else (4, 5)
    for i in range(len(si)):
        oracle.oracle_independent_sampler(int(pix[i, 0]), int(pix[i, 1]), int(seed), int(si[i]), 6, buf)
        out[i] = (buf[1], buf[2], buf[lens[0]], buf[lens[1]])
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# float32 mirror
def _normalize(x, y, z):
    l = np.sqrt(((x * x + y * y).astype(f32) + z * z).astype(f32), dtype=f32)   # Length = sqrt(Sqr(x) + Sqr(y) + Sqr(z))
    with np.errstate(divide="ignore", invalid="ignore"):
        return (x / l).astype(f32), (y / l).astype(f32), (z / l).astype(f32)     # v / Length(v): one division per component


def disk_concentric(u0, u1):
    """SampleUniformDiskConcentric (util/sampling.h:325-341) -> (x, y)."""
    u0, u1 = np.asarray(u0, f32).reshape(-1), np.asarray(u1, f32).reshape(-1)
    ox, oy = (f32(2) * u0 - f32(1)).astype(f32), (f32(2) * u1 - f32(1)).astype(f32)
    zero = (ox == 0) & (oy == 0)
    xmajor = np.abs(ox) > np.abs(oy)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(xmajor, oy / np.where(zero, f32(1), ox), ox / np.where(zero | (oy == 0), f32(1), oy)).astype(f32)
    t = (PI_OVER_4 * q).astype(f32)
    theta = np.where(xmajor, t, (PI_OVER_2 - t).astype(f32)).astype(f32)
    r = np.where(xmajor, ox, oy).astype(f32)
    x, y = (r * EM.cosf(theta)).astype(f32), (r * EM.sinf(theta)).astype(f32)
    return np.where(zero, f32(0), x).astype(f32), np.where(zero, f32(0), y).astype(f32)


def wrap_equal_area_square(u, v):
    """WrapEqualAreaSquare (util/math.cpp:363-379)."""
    u, v = np.asarray(u, f32).copy(), np.asarray(v, f32).copy()
    lo, hi = u < 0, u > 1
    v = np.where(lo | hi, f32(1) - v, v).astype(f32)
    u = np.where(lo, -u, np.where(hi, f32(2) - u, u)).astype(f32)
    lo, hi = v < 0, v > 1
    u = np.where(lo | hi, f32(1) - u, u).astype(f32)
    v = np.where(lo, -v, np.where(hi, f32(2) - v, v)).astype(f32)
    return u, v


def _from_local(cam, x, y, z):
    """Frame::FromLocal (vecmath.h:1914): x right + y up + z fwd per component, summed left to right."""
    return np.stack([((x * cam.right[k]).astype(f32) + (y * cam.up[k]).astype(f32)).astype(f32) + (z * cam.fwd[k]).astype(f32) for k in range(3)],
                    axis=1).astype(f32)


def camera_space_ray(cam, pfx, pfy, ulx, uly, plant=()):
    """(o [n, 3], d [n, 3], at_origin) in camera space."""
    pfx, pfy = np.asarray(pfx, f32).reshape(-1), np.asarray(pfy, f32).reshape(-1)
    n = pfx.shape[0]
    zeros, ones = np.zeros(n, f32), np.ones(n, f32)
    if cam.model in (SPHERICAL_EQUALAREA, SPHERICAL_EQUIRECT):
        if "uv_reciprocal" in plant:
            u, v = (pfx * (f32(1) / f32(cam.xres))).astype(f32), (pfy * (f32(1) / f32(cam.yres))).astype(f32)
        else:
            u, v = (pfx / f32(cam.xres)).astype(f32), (pfy / f32(cam.yres)).astype(f32)
        if cam.model == SPHERICAL_EQUIRECT:
            theta, phi = (PI * v).astype(f32), (f32(f32(2) * PI) * u).astype(f32)
            st, ct = np.clip(EM.sinf(theta), f32(-1), f32(1)), np.clip(EM.cosf(theta), f32(-1), f32(1))
            d = np.stack([(st * EM.cosf(phi)).astype(f32), (st * EM.sinf(phi)).astype(f32), ct], axis=1).astype(f32)
        else:
            u, v = wrap_equal_area_square(u, v)
            d = EM.square_to_sphere(u, v)
        if "no_yz_swap" not in plant:
            d = d[:, [0, 2, 1]]
        return np.zeros((n, 3), f32), np.ascontiguousarray(d, f32), True
    cx = ((cam.sx * pfx).astype(f32) + cam.ox).astype(f32)
    cy = ((cam.sy * pfy).astype(f32) + cam.oy).astype(f32)
    if cam.model == ORTHOGRAPHIC:
        o, d, at_origin = (cx, cy, zeros), (zeros, zeros, ones), False
    else:
        o, d, at_origin = (zeros, zeros, zeros), _normalize(cx, cy, ones), True
    if cam.has_lens:
        dx, dy = disk_concentric(ulx, uly)
        lx, ly = (cam.lens_radius * dx).astype(f32), (cam.lens_radius * dy).astype(f32)
        with np.errstate(divide="ignore", invalid="ignore"):
            ft = np.full(n, cam.focal_distance, f32) if "ft_no_divide" in plant else (cam.focal_distance / d[2]).astype(f32)
        focus = [(o[k] + (d[k] * ft).astype(f32)).astype(f32) for k in range(3)]     # ray(ft) = o + d * t
        if "lens_plus_pcamera" in plant:
            o = ((o[0] + lx).astype(f32), (o[1] + ly).astype(f32), o[2])
        else:
            o = (lx, ly, zeros)
        d = _normalize(*[(focus[k] - o[k]).astype(f32) for k in range(3)])
        at_origin = False
    return np.stack(o, axis=1).astype(f32), np.stack(d, axis=1).astype(f32), at_origin


def generate_ray(cam, pfx, pfy, ulx, uly, plant=()):
    """The render-space ray (ro [n, 3], rd [n, 3]) in float32."""
    o, d, at_origin = camera_space_ray(cam, pfx, pfy, ulx, uly, plant)
    rd = _from_local(cam, d[:, 0], d[:, 1], d[:, 2])
    if at_origin:
        ro = np.tile(cam.origin, (o.shape[0], 1)).astype(f32)
    else:
        ro = (cam.origin[None, :] + _from_local(cam, o[:, 0], o[:, 1], o[:, 2])).astype(f32)
    return ro, rd


def rays_of_samples(cam, pixel_xy, u, plant=()):
    """generate_ray for pixels [n, 2] and variates [n, 4] (filter u0 u1, lens u0 u1)."""
    pix = np.asarray(pixel_xy, np.int64).reshape(-1, 2)
    u = np.asarray(u, f32).reshape(-1, 4)
    pfx, pfy = raster_point(pix[:, 0], pix[:, 1], u[:, 0], u[:, 1])
    return generate_ray(cam, pfx, pfy, u[:, 2], u[:, 3], plant)


# ---------------------------------------------------------------------------------------------------------------------------
# float64 statement
def disk_concentric64(u0, u1):
    ox, oy = 2.0 * np.asarray(u0, np.float64) - 1.0, 2.0 * np.asarray(u1, np.float64) - 1.0
    zero = (ox == 0) & (oy == 0)
    xmajor = np.abs(ox) > np.abs(oy)
    with np.errstate(divide="ignore", invalid="ignore"):
        theta = np.where(xmajor, (np.pi / 4) * (oy / np.where(zero, 1.0, ox)), np.pi / 2 - (np.pi / 4) * (ox / np.where(zero | (oy == 0), 1.0, oy)))
    r = np.where(xmajor, ox, oy)
    return np.where(zero, 0.0, r * np.cos(theta)), np.where(zero, 0.0, r * np.sin(theta))


def camera_space_ray64(cam, pfx, pfy, ulx, uly):
    """(o, d) in camera space in float64 from the float32 record and inputs."""
    pfx, pfy = np.asarray(pfx, np.float64).reshape(-1), np.asarray(pfy, np.float64).reshape(-1)
    n = pfx.shape[0]
    if cam.model in (SPHERICAL_EQUALAREA, SPHERICAL_EQUIRECT):
        u, v = pfx / cam.xres, pfy / cam.yres
        if cam.model == SPHERICAL_EQUIRECT:
            theta, phi = np.pi * v, 2 * np.pi * u
            d = np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], axis=1)
        else:
            d = EM.square_to_sphere_exact(np.stack([np.clip(u, 0, 1), np.clip(v, 0, 1)], axis=1))   # (pFilm lies inside the frame: no wrap)
        return np.zeros((n, 3)), d[:, [0, 2, 1]]
    cx, cy = float(cam.sx) * pfx + float(cam.ox), float(cam.sy) * pfy + float(cam.oy)
    if cam.model == ORTHOGRAPHIC:
        o, d = np.stack([cx, cy, np.zeros(n)], axis=1), np.tile([0.0, 0.0, 1.0], (n, 1))
    else:
        d = np.stack([cx, cy, np.ones(n)], axis=1)
        o, d = np.zeros((n, 3)), d / np.linalg.norm(d, axis=1)[:, None]
    if cam.has_lens:
        dx, dy = disk_concentric64(ulx, uly)
        R, F = float(cam.lens_radius), float(cam.focal_distance)
        focus = o + d * (F / d[:, 2])[:, None]
        o = np.stack([R * dx, R * dy, np.zeros(n)], axis=1)
        d = focus - o
        d = d / np.linalg.norm(d, axis=1)[:, None]
    return o, d


def generate_ray64(cam, pfx, pfy, ulx, uly):
    o, d = camera_space_ray64(cam, pfx, pfy, ulx, uly)
    M = np.stack([cam.right, cam.up, cam.fwd], axis=0).astype(np.float64)       # rows: the frame's axes
    return cam.origin.astype(np.float64)[None, :] + o @ M, d @ M
