"""The geometry of the depth-of-field known answer (tests/test_camera_gpu.py; its conditions are checked on the CPU by
tests/test_camera_model.py): a camera at the origin looking along +z photographs the edge x = 0 of an emissive half-plane (Le = 1,
Kd = 0, no medium) at camera depth Z through a lens of radius R focused at depth F.  Every sample is Le times a Bernoulli variable.

A pixel sample with screen coordinate X (perspective: the pinhole ray's x at depth 1 times F, i.e. its x on the plane of focus;
orthographic: pCamera.x) and lens point l = R t, t the x-coordinate of a uniform point of the unit disk, meets depth Z at
    x(Z) = X Z / F + l (1 - Z / F) = a + c R t,      a = X Z / F,  c = 1 - Z / F
-- for both cameras, because the reference's orthographic lens ray starts at the lens point itself.  It is bright when x(Z) > 0:
t > s (c > 0) or t < s (c < 0) with s = -a / (c R), and the fraction of the unit disk with t > s is
    A(s) = (acos(s) - s sqrt(1 - s^2)) / Pi   for |s| <= 1,   1 for s < -1,   0 for s > 1.
P of a pixel is A averaged over the pixel's footprint (the box filter: pFilm.x uniform over the pixel), integrated here in float64 by
the midpoint rule.  With Z = F, c = 0: x(Z) = a, the step is sharp."""
import numpy as np

import camera_model as M

XRES, YRES, ROW = 32, 8, 4
WINDOW = (-0.165, 0.155, -0.04, 0.04)      # the edge falls inside pixel 16; every other pixel is at least half a pixel away from it


class Geometry:
    def __init__(self, model, R, F, Z):
        self.model, self.R, self.F, self.Z = model, R, F, Z
        self.pixels = np.array([(x, ROW) for x in range(XRES)], np.int32)
        x0, x1, y0, y1 = WINDOW
        # vspg_camera_look_at_window at fov 90 (perspective: tan(45 degrees) rounds to 1 in float32) with this window
        self.cam = M.Camera((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (x1 - x0) / XRES, x0, -(y1 - y0) / YRES, y1, model, XRES, YRES, R, F)


def geometry(model, focused=False):
    """Z = 1, F = 2 (c = 1/2).  Perspective: a = cx Z and R = 0.5, so s = -4 cx; orthographic: a = X / 2 and R = 0.25, so s = -4 X: both
    span +-0.66 over the row, where A(s) stays inside [0.1, 0.9].  focused: Z = F = 1."""
    return Geometry(model, 0.5 if model == M.PERSPECTIVE else 0.25, 1.0 if focused else 2.0, 1.0)


def disk_fraction(s):
    s = np.clip(np.asarray(s, np.float64), -1.0, 1.0)
    return (np.arccos(s) - s * np.sqrt(1.0 - s * s)) / np.pi


def edge_offset(g, pfx):
    """(a, c): the pinhole position at depth Z and the lens coefficient, from the raster x."""
    cx = float(g.cam.sx) * np.asarray(pfx, np.float64) + float(g.cam.ox)
    X = cx * g.F if g.model == M.PERSPECTIVE else cx
    return X * g.Z / g.F, 1.0 - g.Z / g.F


def hit_probability(g, nodes=4000):
    t = (np.arange(nodes) + 0.5) / nodes
    P = np.zeros(len(g.pixels))
    for i, (px, _) in enumerate(g.pixels):
        a, c = edge_offset(g, px + t)
        if c == 0:
            P[i] = np.mean(a > 0)
        else:
            f = disk_fraction(-a / (c * g.R))
            P[i] = np.mean(f if c > 0 else 1.0 - f)
    return P


def hit_probability_by_statement(g, n, seed):
    """The same probability counted with the float64 statement of the camera: n samples per pixel."""
    rng = np.random.default_rng(seed)
    P = np.zeros(len(g.pixels))
    for i, (px, py) in enumerate(g.pixels):
        u = rng.random((n, 4))
        ro, rd = M.generate_ray64(g.cam, px + u[:, 0], py + u[:, 1], u[:, 2], u[:, 3])
        x = ro[:, 0] + rd[:, 0] * ((g.Z - ro[:, 2]) / rd[:, 2])
        P[i] = np.mean(x > 0)
    return P
