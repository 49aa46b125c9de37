"""The kernel-choice table (tests/test_kernel_choice.py) on the device: the C ABI reports the name the table gives, and every
kernel family still launches -- at 24 x 16, three by two 8 x 8 tiles: few enough for the tile count to clamp every workgroup
grid.  The families of a configuration are bit-identical by design, so their films and
counters are compared as bit patterns: there is no tolerance here.  The environment is read at every call: it stays set while a
renderer renders."""
import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

W, H = 24, 16
ENV = ("VSPG_KERNEL", "VSPG_WG_SCHED", "VSPG_NO_GREY_GUIDED", "VSPG_WF_MERGED")


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def render(P, scene, prm, field, env, name):
    """The film's bits and the counters after waves 0-1, 1-2 and 2-4, each followed by post_process_wave, under `env`."""
    with pytest.MonkeyPatch.context() as mp:
        for k in ENV:
            mp.delenv(k, raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        r = P.Renderer(scene, prm, W, H, seed=11)
        if field is not None:
            r.set_guiding_field(field, field)
        assert r.kernel_name() == name, (env, r.kernel_name())
        for a, b in ((0, 1), (1, 2), (2, 4)):   # (no film read in between: one-sample launches park samples and carry paths over)
            r.render_wave(a, b)
            r.post_process_wave()
        film, counters = u32(r.film()), r.counters()
        r.close()
    return film, counters


def check_rows(P, scene, prm, field, rows):
    ref_film, ref_counters = None, None
    for env, name in rows:
        film, counters = render(P, scene, prm, field, env, name)
        assert film.any() and counters["paths"] == 4 * W * H, (env, counters)
        if ref_film is None:
            ref_film, ref_counters = film, counters
        assert np.array_equal(film, ref_film), (env, "film words that differ:", int((film != ref_film).sum()))
        assert counters == ref_counters, (env, counters, ref_counters)


def test_unguided_fog_families(gpu_pkg):
    P = gpu_pkg
    check_rows(P, P.fog_box_scene(W, H), P.app_f_params(), None,
               [({}, "k_render_wave_wg3<HomogeneousMediumT<2,true>>"),
                ({"VSPG_WG_SCHED": "2"}, "k_render_wave_wg2<HomogeneousMediumT<2,true>>"),
                ({"VSPG_WG_SCHED": "1"}, "k_render_wave_wg<HomogeneousMediumT<2,true>>"),
                ({"VSPG_KERNEL": "lane"}, "k_render_wave<HomogeneousMedium>")])


def test_guided_fog_families(gpu_pkg):
    P = gpu_pkg
    check_rows(P, P.fog_box_scene(W, H), P.default_params(), scenes.light_field(P, n=4),
               [({}, "k_render_wave_wg2<HomogeneousMediumT<2,true>,guided>"),
                ({"VSPG_KERNEL": "lane"}, "k_render_wave<HomogeneousMediumT<2,true>,guided>")])


def test_grid_families(gpu_pkg):
    P = gpu_pkg
    scene = scenes.grid_scene(scenes.cloud_density(24), (24, 24, 24), (0.05, 0.08, 0.1), (3.0, 2.6, 2.2), g=0.5, bmin=(-0.8, -0.8, -0.5),
                              bmax=(0.8, 0.7, 0.9), W=W, H=H)
    check_rows(P, scene, P.app_f_params(), None,
               [({}, "k_wf_dist_walk<GridMedium>"),
                ({"VSPG_KERNEL": "wg"}, "k_render_wave_wg<GridMedium>"),
                ({"VSPG_KERNEL": "lane"}, "k_render_wave<GridMedium>")])
