"""vspg_render_window on the device: a launch over a pixel window [x0, x1) x [y0, y1) (the film's pixelBounds, film.cpp:97-172;
the render loop covers nothing else, integrators.cpp:183) computes exactly what the full-frame launch computes for those pixels
and touches nothing outside them.  Every comparison is of bit patterns (array_equal on uint32 views): there is no tolerance in
this feature.

Comparisons against the oracle use ONE sample index per pixel between film reads: the oracle's film accumulates in double and
the device's in float (RGBFilm's float pixels), so only a single addition per pixel is the same number in both; several samples
per pixel are compared against the same renderer configuration's full-frame launch instead, which adds in the same order."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib
from conftest import ROOT

pytestmark = pytest.mark.gpu

W, H = 100, 76                           # not a multiple of 8 either way
INTERIOR = (13, 5, 77, 50)               # unaligned interior window
SHAPES = [INTERIOR,
          (37, 41, 38, 42),              # one pixel
          (16, 24, 24, 32),              # exactly one tile
          (61, 30, 100, 76),             # touches the right and bottom edges (ragged tiles)
          (3, 33, 97, 34),               # one row
          (0, 0, W, H)]                  # the full frame


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def crop_equal(film_win, film_full, win):
    """film_win == film_full inside the window and is untouched (all zero bits) outside it"""
    x0, y0, x1, y1 = win
    inside = np.zeros(film_full.shape[:2], dtype=bool)
    inside[y0:y1, x0:x1] = True
    a, b = u32(film_win), u32(film_full)
    return np.array_equal(a[inside], b[inside]) and not a[~inside].any()


def dev_stats(r):
    import torch
    ptr, n = r.isg_stats_ptr()

    class Dev:
        __cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (ptr, False), "version": 2}
    r.flush()
    torch.cuda.synchronize()
    return torch.as_tensor(Dev(), device="cuda:0").cpu().numpy().copy()


# ---- the kernel families, selected the way tests/test_gpu_parity.py selects them: scene + options (+ VSPG_KERNEL / VSPG_WG_SCHED) ----
def _open_fog_scene(P, w, h):
    """fog + a ground rectangle + triangles + a sphere + infinite lights: the workgroup kernel's full-scene instantiation"""
    import scenes
    scene = P.fog_box_scene(w, h)
    for k in range(3):
        scene.medium.sigma_a[k] = 0.02
        scene.medium.sigma_s[k] = 0.25
    floor = type(scene.quads[0]).from_buffer_copy(scene.quads[0])
    for i in range(P.VSPG_MAX_QUADS):
        scene.quads[i] = type(floor)()
    scene.quads[0] = floor
    scene.n_quads = 1
    tris, kd = scenes.heightfield_triangles(40, y=-0.75, amp=0.2)
    P.set_triangles(scene, tris, kd)
    scenes.add_sphere(scene, (0.2, -0.2, 0.1), 0.3)
    P.add_infinite_light(scene, P.LIGHT_UNIFORM_INFINITE, (0.35, 0.5, 0.9))
    P.add_infinite_light(scene, P.LIGHT_DISTANT, (9.0, 8.0, 6.5), (0.3, 1.0, -0.4))
    return scene


def _temperature_grid(scene):
    m = scene.medium
    nvox = m.nx * m.ny * m.nz
    rng = np.random.default_rng(9)
    temp = (150.0 + 2600.0 * np.clip(rng.random(nvox).astype(np.float32) * 1.3, 0, 1.4)).astype(np.float32)
    m.temperature = temp.ctypes.data_as(C.POINTER(C.c_float))
    m.temperature_offset, m.temperature_scale, m.nvdb_le_scale = 120.0, 1.3, 0.6
    scene._temp_keepalive = temp
    return scene


def _case(P, name, w=W, h=H):
    """-> scene, params, guiding field or None, environment, expected kernel-name prefix"""
    import scenes
    dens = scenes.cloud_density(24)
    grid = lambda: scenes.grid_scene(dens, (24, 24, 24), (0.05, 0.08, 0.1), (3.0, 2.6, 2.2), g=0.5, bmin=(-0.8, -0.8, -0.5), bmax=(0.8, 0.7, 0.9), W=w, H=h)
    nvdb = lambda: scenes.nvdb_scene(dens, (24, 24, 24), (0.25, 0.3, 0.35), (3.0, 2.6, 2.2), g=0.5, index_min=(-3, 2, 0), voxel=(0.066, 0.0625, 0.058),
                                     origin=(-0.6, -0.93, -0.5), density_offset=0.02, majorant_scale=1.25, W=w, H=h)
    nds = P.app_f_params()
    nds.vspsamplingmethod = P.VSP_NDS
    if name == "fog-wg3":
        return P.fog_box_scene(w, h), P.app_f_params(), None, {}, "k_render_wave_wg3<"
    if name == "fog-wg":
        return P.fog_box_scene(w, h), P.app_f_params(), None, {"VSPG_WG_SCHED": "1"}, "k_render_wave_wg<"
    if name == "fog-lane":
        return P.fog_box_scene(w, h), P.app_f_params(), None, {"VSPG_KERNEL": "lane"}, "k_render_wave<"
    if name == "fog-guided-wg2":
        return P.fog_box_scene(w, h), P.default_params(), scenes.light_field(P, n=4), {}, "k_render_wave_wg2<HomogeneousMediumT<2,true>,guided"
    if name == "fog-guided-lane":
        return P.fog_box_scene(w, h), P.default_params(), scenes.light_field(P, n=4), {"VSPG_KERNEL": "lane"}, "k_render_wave<HomogeneousMediumT<2,true>,guided"
    if name == "fog-full-wg2":
        return _open_fog_scene(P, w, h), P.app_f_params(), None, {}, "k_render_wave_wg2<HomogeneousMedium>"
    if name == "cloud-grid":
        return grid(), P.app_f_params(), None, {}, "k_wf_dist_walk<GridMedium"
    if name == "cloud-grid-lane":
        return grid(), P.app_f_params(), None, {"VSPG_KERNEL": "lane"}, "k_render_wave<GridMedium"
    if name == "cloud-nvdb":
        return nvdb(), P.app_f_params(), None, {}, "k_wf_dist_walk<NanoDenseMedium"
    if name == "cloud-scene":
        return scenes.cloud_scene(w, h, dens, 24), P.app_f_params(), None, {}, "k_wf_walk<GridMedium"
    if name == "nds-temperature":
        return _temperature_grid(nvdb()), nds, None, {}, "k_wf_segment_vertex<NanoDenseMedium"
    raise KeyError(name)


CASES = ["fog-wg3", "fog-wg", "fog-lane", "fog-guided-wg2", "fog-guided-lane", "fog-full-wg2", "cloud-grid", "cloud-grid-lane", "cloud-nvdb",
         "cloud-scene", "nds-temperature"]


class _Env:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k in self.env:
            os.environ.pop(k, None)


def _gpu(P, case, seed=3, w=W, h=H, **kw):
    scene, prm, field, env, prefix = case
    for k, v in kw.items():
        setattr(prm, k, v)
    r = P.Renderer(scene, prm, w, h, seed=seed)
    if field is not None:
        r.set_guiding_field(field, field)
    assert r.kernel_name().startswith(prefix), (r.kernel_name(), prefix)   # no case silently runs another kernel
    return r


def _cpu(case, seed=3, w=W, h=H):
    scene, prm, field, env, prefix = case
    c = oracle_lib.OracleRenderer(scene, prm, w, h, seed=seed)
    if field is not None:
        c.set_guiding_field(field, field)
    return c


@pytest.mark.parametrize("name", CASES)
def test_window_equals_crop_of_full_frame_and_oracle_window(gpu_pkg, name):
    """Every kernel family, every window shape: three sample indices in one launch == the full-frame launch inside the window,
    nothing outside; the full-frame window == render_wave.  One sample index of the unaligned interior window: film, image-space
    statistics and counters == oracle_render_window's."""
    P = gpu_pkg
    case = _case(P, name)
    with _Env(case[3]):
        full = _gpu(P, case)
        full.render_wave(0, 3)
        film_full, cnt_full = full.film(), full.counters()
        full.close()
        for win in SHAPES:
            r = _gpu(P, case)
            r.render_window(*win, 0, 3)
            film = r.film()
            assert crop_equal(film, film_full, win), (name, win)
            assert r.counters()["paths"] == 3 * (win[2] - win[0]) * (win[3] - win[1]), (name, win)
            if win == (0, 0, W, H):
                assert r.counters() == cnt_full
            r.close()
        g, c = _gpu(P, case), _cpu(case)
        g.render_window(*INTERIOR, 0, 1)
        c.render_window(*INTERIOR, 0, 1)
        fg, fc = g.film(), c.film()
        sg, sc = dev_stats(g), c.isg_stats().reshape(-1)
        cg, cc = g.counters(), c.counters()
        print(name, "film bits differ in", int((u32(fg) != u32(fc)).sum()), "stats bits differ in", int((u32(sg) != u32(sc)).sum()), cg, cc)
        assert np.array_equal(u32(fg), u32(fc))
        assert np.array_equal(u32(sg), u32(sc))
        assert cg == cc
        g.close(); c.close()


@pytest.mark.parametrize("name", ["fog-wg3", "fog-guided-wg2", "cloud-grid", "cloud-scene"])
def test_windows_that_tile_the_frame_equal_one_full_frame_render(gpu_pkg, name):
    """Four disjoint windows (cut off the tile grid) in either launch order == one full-frame launch: film, statistics, counters."""
    P = gpu_pkg
    case = _case(P, name)
    quads = [(0, 0, 45, 29), (45, 0, W, 29), (0, 29, 45, H), (45, 29, W, H)]
    with _Env(case[3]):
        full = _gpu(P, case)
        full.render_wave(0, 2)
        ref = (full.film(), dev_stats(full), full.counters())
        full.close()
        for order in (quads, quads[::-1]):
            r = _gpu(P, case)
            for win in order:
                r.render_window(*win, 0, 2)
            assert np.array_equal(u32(r.film()), u32(ref[0])), name
            assert np.array_equal(u32(dev_stats(r)), u32(ref[1])), name
            assert r.counters() == ref[2]
            r.close()


@pytest.mark.parametrize("name", ["fog-wg3", "fog-guided-wg2"])
def test_one_sample_launches_alternating_between_two_windows(gpu_pkg, name):
    """The parked-sample path: a one-sample launch parks its samples and the next launch is a DIFFERENT window (they overlap); film
    reads in between.  Each read == the oracle doing the same, and the end == the same sequence with every launch resolving its
    own samples at once (VSPG_WG2_DEFER=0)."""
    P = gpu_pkg
    case = _case(P, name)
    a, b = INTERIOR, (40, 20, 100, 76)
    seq = [(a, 0), (b, 0), (a, 1), (a, 2), (b, 1), (a, 3)]
    ends = []
    for defer in ("1", "0"):
        with _Env(dict(case[3], VSPG_WG2_DEFER=defer)):
            g, c = _gpu(P, case), _cpu(case)
            for k, (win, w) in enumerate(seq):
                g.render_window(*win, w, w + 1)
                c.render_window(*win, w, w + 1)
                if k in (1, 3):                      # a read between the launches
                    fg, fc = g.film(), c.film()
                    assert np.array_equal(fg[..., 3], fc[..., 3])       # the weight sums: who got which sample
                    once = fc[..., 3] == 1
                    assert np.array_equal(u32(fg)[once], u32(fc)[once])  # (one addition per pixel: the same float in both)
            assert np.array_equal(u32(dev_stats(g)), u32(c.isg_stats().reshape(-1)))
            assert g.counters() == c.counters()
            ends.append(g.film())
            g.close(); c.close()
    assert np.array_equal(u32(ends[0]), u32(ends[1]))


@pytest.mark.parametrize("name", ["fog-wg3", "cloud-grid"])
def test_window_post_process_then_another_window_vsp_buffer_equals_oracle(gpu_pkg, name):
    P = gpu_pkg
    case = _case(P, name)
    with _Env(case[3]):
        g, c = _gpu(P, case), _cpu(case)
        for r in (g, c):
            r.render_window(*INTERIOR, 0, 1)
            r.post_process_wave()                      # wave counter 1: the buffer updates, from the window's statistics alone
            r.render_window(40, 20, 100, 76, 1, 2)     # (its pixels inside the first window read the updated buffer)
            r.post_process_wave()
        vg, rg = g.vsp_buffer()
        vc, rc = c.vsp_buffer()
        assert rg and rc
        assert np.array_equal(u32(vg), u32(vc))
        fg, fc = g.film(), c.film()
        once = fc[..., 3] == 1
        assert np.array_equal(fg[..., 3], fc[..., 3]) and np.array_equal(u32(fg)[once], u32(fc)[once])
        g.close(); c.close()


def _sorted_samples(a):
    v = np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1)
    return a[np.lexsort(v.T[::-1])]


@pytest.mark.parametrize("name", ["fog-guided-wg2", "fog-guided-lane", "cloud-grid"])
def test_training_and_tr_buffer_on_a_window(gpu_pkg, name):
    """In-loop training on a window: the multiset of training records == the oracle's; storeTrBuffer on a window of a grid medium:
    the TrBuffer == the oracle's, untouched outside the window."""
    P = gpu_pkg
    scene, prm, field, env, prefix = _case(P, name)
    with _Env(env):
        if name.startswith("fog-guided"):
            g = P.Renderer(scene, prm, W, H, seed=3)          # no field uploaded: the renderer trains its own
            c = oracle_lib.OracleRenderer(scene, prm, W, H, seed=3)
            assert g.kernel_name().startswith(prefix) and g.kernel_name().endswith("train>")
            for r in (g, c):
                r.render_window(*INTERIOR, 0, 2)
            sg, sc = g.training_stats(), c.training_stats()
            assert sg["n_samples"] == sc["n_samples"] > 200 and sg["n_zero"] == sc["n_zero"]
            assert _sorted_samples(g.train_samples()).tobytes() == _sorted_samples(c.train_samples()).tobytes()
        else:
            prm.storeTrBuffer = 1
            g = P.Renderer(scene, prm, W, H, seed=3)
            c = oracle_lib.OracleRenderer(scene, prm, W, H, seed=3)
            assert g.kernel_name().startswith(prefix)
            for r in (g, c):
                r.render_window(*INTERIOR, 0, 3)
            tg, spp = g.tr_buffer()
            tc = c.tr_buffer()
            x0, y0, x1, y1 = INTERIOR
            inside = np.zeros((H, W), dtype=bool)
            inside[y0:y1, x0:x1] = True
            assert np.all(spp[inside] == 3) and not spp[~inside].any()
            assert np.array_equal(u32(tg), u32(tc))
        g.close(); c.close()


def test_fast_arithmetic_modes_render_a_window(gpu_pkg):
    """The tolerance modes of vspg_renderer_set_arithmetic: a window == the crop of the same mode's full frame."""
    P = gpu_pkg
    case = _case(P, "fog-wg3")
    for mode in (P.ARITH_FAST_WEIGHTS, P.ARITH_FAST):
        films = []
        for win in ((0, 0, W, H), INTERIOR):
            r = _gpu(P, case)
            r.set_arithmetic(mode)
            r.render_window(*win, 0, 2)
            films.append(r.film())
            r.close()
        assert crop_equal(films[1], films[0], INTERIOR)


def test_strict_window_arguments(gpu_pkg):
    P = gpu_pkg
    r = _gpu(P, _case(P, "fog-wg3"))
    for bad in [(5, 5, 5, 9), (5, 5, 9, 5), (9, 5, 5, 9), (-1, 0, 8, 8), (0, -1, 8, 8), (0, 0, W + 1, 8), (0, 0, 8, H + 1)]:
        with pytest.raises(P.VspgError) as e:
            r.render_window(*bad, 0, 1)
        assert e.value.code == P.VSPG_EINVAL and "window" in str(e.value)
    with pytest.raises(P.VspgError) as e:                 # the wave range rules are render_wave's
        r.render_window(0, 0, W, H, 2, 1)
    assert e.value.code == P.VSPG_EINVAL
    r.render_window(0, 0, W, H, 1, 1)                     # an empty range is no work
    assert r.counters()["paths"] == 0 and not r.film().any()
    r.close()


@pytest.mark.parametrize("win", [(717, 403, 781, 467), (1003, 610, 1027, 626)])   # 64 x 64 and 24 x 16, unaligned, interior
def test_small_windows_of_a_large_frame_repeat(gpu_pkg, win):
    """Small windows of a 1920 x 1080 fog frame, 64 sample indices in one call: k_render_wave_wg3's eight tile cursors run dry at
    once, the case in which a wavefront used to read its claimed free-ring entries only after going round the cursors.  Five fresh
    renderers: every film equal to the first and to the crop of a full-frame render, the counters equal to the oracle's.  (A
    repeatability check of a correct result; what closes the ordering is the early read in vspg_wg3.h.)"""
    P = gpu_pkg
    w, h, n = 1920, 1080, 64
    case = _case(P, "fog-wg3", w, h)
    x0, y0, x1, y1 = win
    full = _gpu(P, case, w=w, h=h)
    full.render_wave(0, n)
    film_full = full.film()
    full.close()
    c = _cpu(case, w=w, h=h)
    c.render_window(*win, 0, n)
    cc = c.counters()
    c.close()
    first = None
    for k in range(5):
        r = _gpu(P, case, w=w, h=h)
        r.render_window(*win, 0, n)
        film = r.film()
        if first is None:
            first = film
            assert crop_equal(film, film_full, win)
        assert np.array_equal(u32(film), u32(first)), k
        assert r.counters() == cc, k
        r.close()


def _read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = map(int, f.readline().split())
        scale = float(f.readline())
        a = np.frombuffer(f.read(), dtype="<f4" if scale < 0 else ">f4").reshape(h, w, 3)
    return a[::-1]        # PFM rows go bottom-up


def _interior_equal(part, whole, x0, y0, x1, y1, reach):
    """part == whole[y0:y1, x0:x1] on the pixels at least `reach` away from every edge of the window that is not the frame's"""
    hh, ww = whole.shape[:2]
    l, r = (reach if x0 > 0 else 0), (reach if x1 < ww else 0)
    t, b = (reach if y0 > 0 else 0), (reach if y1 < hh else 0)
    crop = whole[y0:y1, x0:x1]
    return np.array_equal(u32(part[t:part.shape[0] - b, l:part.shape[1] - r]), u32(crop[t:crop.shape[0] - b, l:crop.shape[1] - r]))


def test_host_adapter_writes_the_window(gpu_pkg, tmp_path):
    """vspg_pbrt --pixelbounds / a "cropwindow" in the file: a PFM of the window's size that holds the window's pixels
    (RGBFilm::WriteImage over pixelBounds, film.cpp:541-557).

    At one sample per pixel the image == the crop of the uncropped run's, every pixel.  From the second wave on a pixel's path
    depends on the image-space VSP buffer, which PostProcessWave filters from the statistics of the 5 x 5 pixels around it
    (kIsgRadius = 2): a cropped run has no statistics outside its window -- in the reference too, whose buffer covers the crop
    only -- so pixels near a cut edge legitimately differ from the uncropped run.  The buffer updates after waves 0 and 1 feed
    the scene's 4 waves (the one after wave 3 feeds nothing), each reaching 2 pixels further: pixels 4 or more away from every
    cut edge == the uncropped run's, which the fog box's 4-sample runs check.  tests/scenes/cloud_boundary.pbrt runs the reference's
    default options: the guiding field trains in the loop from the records of every rendered pixel, so from the second wave on a
    cropped run guides with another field than the uncropped one, everywhere; its comparison is the one-sample run's, and a copy
    of the scene with the directional guiding switches off (nothing trains) takes the 4-sample interior check on the boundary
    pipeline."""
    import re
    exe = os.path.join(ROOT, "vspg-pbrt-v4_amd", "host", "vspg_pbrt")

    def run(scene, out, *extra):
        subprocess.run([exe, scene, "--outfile", str(out)] + list(extra), check=True, timeout=300)
        return _read_pfm(out)
    fog = os.path.join(ROOT, "tests", "scenes", "fog_box.pbrt")
    x0, x1, y0, y1 = 13, 60, 5, 40
    for spp, reach in ((1, 0), (4, 4)):
        whole = run(fog, tmp_path / "fog.pfm", "--spp", str(spp))
        assert whole.shape == (48, 64, 3)
        part = run(fog, tmp_path / "fog_win.pfm", "--spp", str(spp), "--pixelbounds", "%d,%d,%d,%d" % (x0, x1, y0, y1))
        assert part.shape == (y1 - y0, x1 - x0, 3)
        assert _interior_equal(part, whole, x0, y0, x1, y1, reach), spp
    src_path = os.path.join(ROOT, "tests", "scenes", "cloud_boundary.pbrt")
    src = open(src_path).read()
    text, n = re.subn(r'(Film\s+"rgb")', r'\1 "float cropwindow" [0.25 0.8 0.1 0.6]', src, count=1)
    assert n == 1
    cropped = tmp_path / "cloud_boundary_crop.pbrt"
    cropped.write_text(text)
    for dep in os.listdir(os.path.dirname(src_path)):      # (files the scene names by relative path)
        if not dep.endswith(".pbrt"):
            os.symlink(os.path.join(os.path.dirname(src_path), dep), tmp_path / dep)
    f32 = np.float32
    # ... and the same scene with the directional guiding switches off (no field, nothing trains): the boundary pipeline through
    # the adapter from the second wave on, where only the image-space filter reaches across the cut
    unguided = 'Integrator "guidedvolpathvspg" "bool surfaceguiding" false "bool volumeguiding" false "bool vspsecondaryguiding" false'
    assert src.count('Integrator "guidedvolpathvspg"\n') == 1
    plain, plain_crop = tmp_path / "cb_plain.pbrt", tmp_path / "cb_plain_crop.pbrt"
    plain.write_text(src.replace('Integrator "guidedvolpathvspg"\n', unguided + "\n"))
    plain_crop.write_text(text.replace('Integrator "guidedvolpathvspg"\n', unguided + "\n"))
    for full_scene, crop_scene, spp, reach in ((src_path, str(cropped), 1, 0), (str(plain), str(plain_crop), 1, 0), (str(plain), str(plain_crop), 4, 4)):
        whole = run(full_scene, tmp_path / "cb.pfm", "--spp", str(spp))
        hh, ww = whole.shape[:2]
        bx0, bx1 = int(np.ceil(f32(ww) * f32(0.25))), int(np.ceil(f32(ww) * f32(0.8)))
        by0, by1 = int(np.ceil(f32(hh) * f32(0.1))), int(np.ceil(f32(hh) * f32(0.6)))
        part = run(crop_scene, tmp_path / "cb_win.pfm", "--spp", str(spp))
        assert part.shape == (by1 - by0, bx1 - bx0, 3)
        assert _interior_equal(part, whole, bx0, by0, bx1, by1, reach), (crop_scene, spp)


def test_two_rank_band_sharding_on_one_card_equals_one_renderer(gpu_pkg, tmp_path):
    """Band mode on the HIP renderer, two ranks rehearsed on ONE card over gloo (tests/band_rehearse_worker.py; no multi-GPU node has
    been available to this project, so what runs here is the plumbing, as in tests/test_bench_rehearsal.py): the all-reduced film
    and the VSP buffer == a single renderer's, bit for bit."""
    import socket
    import sys
    P = gpu_pkg
    w, h, steps = 96, 76, 5
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "band.npz")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "tests", "band_rehearse_worker.py"), str(w), str(h), str(steps), out]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    got = np.load(out)
    one = P.Renderer(P.fog_box_scene(w, h), P.app_f_params(), w, h, seed=3)
    for step in range(steps):
        one.render_wave(step, step + 1)
        one.post_process_wave()
    assert int(got["paths"][0]) == w * h * steps
    assert np.array_equal(u32(got["film"]), u32(one.film()))
    assert np.array_equal(u32(got["vsp"]), u32(one.vsp_buffer()[0]))
    one.close()
