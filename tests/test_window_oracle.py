"""The contract the device tests of vspg_render_window lean on, pinned on the oracle: pixel samples are independent
(Hash(pPixel, seed)), so oracle_render_window gives the full render's bits inside the window and nothing outside it, and disjoint
windows that tile the frame give the full render's film, statistics and counters."""
import numpy as np
import pytest

import oracle_lib
import scenes

W, H = 100, 76


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _setup(kind, w=W, h=H):
    if kind == "fog":
        scene = oracle_lib.fog_box_scene(w, h)
    else:
        scene = scenes.grid_scene(scenes.cloud_density(12), (12, 12, 12), (0.05, 0.08, 0.1), (3.0, 2.6, 2.2), g=0.5,
                                  bmin=(-0.8, -0.8, -0.5), bmax=(0.8, 0.7, 0.9), W=w, H=h)
    prm = oracle_lib.default_params()
    prm.surfaceguiding = prm.volumeguiding = 0          # the two directional guiding switches off: no field needed
    return scene, prm


@pytest.mark.parametrize("kind,w,h", [("fog", W, H), ("grid", 50, 38)])
def test_window_is_the_crop_of_the_full_render(kind, w, h):
    scene, prm = _setup(kind, w, h)
    win = (13, 5, 77, 50) if w == W else (7, 3, 39, 25)
    full = oracle_lib.OracleRenderer(scene, prm, w, h, seed=3)
    part = oracle_lib.OracleRenderer(scene, prm, w, h, seed=3)
    full.render_wave(0, 3)
    part.render_window(*win, 0, 3)
    x0, y0, x1, y1 = win
    inside = np.zeros((h, w), dtype=bool)
    inside[y0:y1, x0:x1] = True
    for a, b in ((part.film_f64(), full.film_f64()), (part.isg_stats(), full.isg_stats())):
        assert np.array_equal(_u32(a)[inside], _u32(b)[inside])
        assert not _u32(a)[~inside].any()
    assert part.counters()["paths"] == 3 * (x1 - x0) * (y1 - y0)
    full.close(); part.close()


@pytest.mark.parametrize("kind,w,h", [("fog", W, H), ("grid", 50, 38)])
def test_windows_that_tile_the_frame_equal_the_full_render(kind, w, h):
    scene, prm = _setup(kind, w, h)
    cx, cy = (45, 29) if w == W else (21, 17)
    quads = [(0, 0, cx, cy), (cx, 0, w, cy), (0, cy, cx, h), (cx, cy, w, h)]
    full = oracle_lib.OracleRenderer(scene, prm, w, h, seed=3)
    full.render_wave(0, 3)
    for order in (quads, quads[::-1]):
        r = oracle_lib.OracleRenderer(scene, prm, w, h, seed=3)
        for win in order:
            r.render_window(*win, 0, 3)
        assert np.array_equal(_u32(r.film_f64()), _u32(full.film_f64()))
        assert np.array_equal(_u32(r.isg_stats()), _u32(full.isg_stats()))
        assert r.counters() == full.counters()
        r.close()
    full.close()
