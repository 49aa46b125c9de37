"""Scenes and images shared by the texture tests (inputs only)."""
import ctypes as C

import numpy as np

import oracle_lib
import scenes
import texture_model as M
from conftest import load_package

f32 = np.float32
WRAPS = {"repeat": M.REPEAT, "clamp": M.CLAMP, "black": M.BLACK}
FILTERS = {"point": M.POINT, "bilinear": M.BILINEAR}


def coloured_image(xres, yres, seed=0, channels=3):
    """Seeded texels in [0.05, 0.95]; no two neighbours alike."""
    rng = np.random.default_rng(100 + seed)
    return np.ascontiguousarray(rng.uniform(0.05, 0.95, (yres, xres, channels)).astype(f32))


def constant_image(xres, yres, colour):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(colour, f32), (yres, xres, 3)))


def write_pfm(path, image):
    """image [yres, xres, 3] float32, top row first; a PFM holds the bottom row first."""
    img = np.asarray(image, f32)
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n-1.0\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img[::-1]).astype("<f4").tobytes())


FLOOR, BACK = 0, 2   # rectangles of the App.-F fog box (vspg_scene_fog_box): the floor y = -1, the back wall z = +1 the camera looks at
CORNER_TRIANGLE = np.array([[[0.9, -0.99, 0.9], [0.9, -0.99, 0.99], [0.99, -0.99, 0.9]]], f32)   # faces +y, just above the floor


def fog_box(W, H, triangle=True):
    """The App.-F fog box; `triangle` adds one small diffuse triangle in a corner so that the scene is not `simple`: a constant-Kd
    twin of a textured scene must run the full-scene kernels too."""
    P = load_package()
    s = oracle_lib.fog_box_scene(W, H)
    if triangle:
        P.set_triangles(s, CORNER_TRIANGLE.copy(), np.full((1, 3), 0.5, f32))
    return s


def small_grid_medium(P, s):
    """A 2^3 grid medium over the box in place of the fog (the pipeline's kernels)."""
    dens = np.array([0.2, 1, 0.7, 0.1, 0.9, 0.4, 1, 0.6], f32)
    m = s.medium
    m.type = P.MEDIUM_GRID
    m.sigma_a[:] = (0.05,) * 3
    m.sigma_s[:] = (0.9,) * 3
    m.g = 0.3
    m.nx = m.ny = m.nz = 2
    m.bounds_min[:] = (-1, -1, -1)
    m.bounds_max[:] = (1, 1, 1)
    m.density = dens.ctypes.data_as(C.POINTER(C.c_float))
    s._density_keepalive = dens
    return s
