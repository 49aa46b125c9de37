"""k_render_wave_wg3's scheduler (csrc/vspg_wg3.h: the two-read decision, w3_policy, ring_push_all with the chunk's tail behind its
commits) computes what the other schedulers compute.

Every case is a function that drives a renderer and records film, VSP buffer and counters; it runs under the default (k_render_wave_wg3
with carried launches), VSPG_WG3_CARRY=0 (the same kernel, every launch self-contained) and VSPG_WG_SCHED=2 (k_render_wave_wg2, lock
step, no queues), and the three records are compared on bit patterns.  A launch that left through the idle valve would have lost paths:
the counters say so.  The shapes are the smallest at which each branch of the scheduler runs; the single tile is also held to the
oracle's paths, the way tests/test_rect_frame_gpu.py holds the 64 x 64 film."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib

pytestmark = pytest.mark.gpu

SETTINGS = (("wg3 carried", {}, "k_render_wave_wg3"), ("wg3 self-contained", {"VSPG_WG3_CARRY": "0"}, "k_render_wave_wg3"),
            ("wg2", {"VSPG_WG_SCHED": "2"}, "k_render_wave_wg2"))


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def resumes(r):
    f = r.lib.vspg_debug_carry_resumes
    f.restype = C.c_longlong
    f.argtypes = [C.c_void_p]
    return int(f(r.h))


class _Env:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def snapshot(r, obs, tag):
    obs.append((tag + ":film", u32(r.film())))
    obs.append((tag + ":counters", np.array(list(r.counters().values()), dtype=np.uint64)))
    obs.append((tag + ":vsp", u32(r.vsp_buffer()[0])))


def under_every_scheduler(case, P):
    """-> the default setting's observations and its count of resumed launches; asserts the three settings' observations equal"""
    runs = []
    for label, env, prefix in SETTINGS:
        with _Env(env):
            obs = []
            name, k = case(P, obs)
            assert name.startswith(prefix), (label, name)   # no setting silently runs another kernel
            runs.append((label, obs, k))
    first = runs[0][1]
    assert len(first) > 0
    for label, obs, _ in runs[1:]:
        assert len(obs) == len(first)
        for (ta, xa), (tb, xb) in zip(first, obs):
            diff = int((xa != xb).sum()) if ta == tb and xa.shape == xb.shape else -1
            print("%-20s %-16s %8d words, %d differ" % (label, ta, xa.size, diff))
            assert diff == 0, (label, ta)
    assert runs[1][2] == 0 and runs[2][2] == 0, "a reference setting resumed launches"
    return first, runs[0][2]


def test_single_tile_and_the_oracles_paths(gpu_pkg):
    """8 x 8: one tile, fewer tiles than cursors; every workgroup but one leaves at once.  Four waves without post-processing: the
    film is the oracle's paths added in wave order (RGBFilm::AddSample), every pixel."""
    P = gpu_pkg
    W = H = 8
    scene, prm = P.fog_box_scene(W, H), P.app_f_params()

    def case(P, obs):
        r = P.Renderer(scene, prm, W, H, seed=4)
        name = r.kernel_name()
        for w in range(4):
            r.render_wave(w, w + 1)
        snapshot(r, obs, "end")
        k = resumes(r)
        r.close()
        return name, k
    first, _ = under_every_scheduler(case, P)
    film = first[0][1].view(np.float32).reshape(H, W, 4)
    assert np.array_equal(film[..., 3], np.full((H, W), 4.0, dtype=np.float32))
    assert int(first[1][1][0]) == W * H * 4                                    # paths
    ys, xs = np.mgrid[0:H, 0:W]
    pix = np.repeat(np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.int32), 4, axis=0)
    si = np.tile(np.arange(4, dtype=np.int32), W * H)
    c = oracle_lib.OracleRenderer(scene, prm, W, H, seed=4)
    L, _ = c.trace_paths(pix, si)
    c.close()
    L = L.astype(np.float32).reshape(W * H, 4, 3)
    want = ((L[:, 0] + L[:, 1]) + L[:, 2]) + L[:, 3]
    got = film[pix[::4, 1], pix[::4, 0], :3]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "film != oracle paths"


def test_six_post_processed_waves(gpu_pkg):
    """72 x 40 at 1 spp for 6 waves with post_process_wave after each: carried launches, predicted and unpredicted updates of the VSP
    buffer (waves 1, 2, 4), the drain, the frame-end flush."""
    P = gpu_pkg
    W, H, n = 72, 40, 6

    def case(P, obs):
        r = P.Renderer(P.fog_box_scene(W, H), P.app_f_params(), W, H, spp=n, seed=5)
        name = r.kernel_name()
        for w in range(n):
            r.render_wave(w, w + 1)
            r.post_process_wave()
            if w == 2:
                snapshot(r, obs, "mid")
        snapshot(r, obs, "end")
        k = resumes(r)
        r.close()
        return name, k
    first, k = under_every_scheduler(case, P)
    assert k > 0, "no launch resumed paths: the carried side was not exercised"
    assert int(first[-2][1][0]) == W * H * n


def test_three_sample_launch(gpu_pkg):
    """200 x 120, samples 0..2 in one launch: the restart bit (a slot goes back to Q_A for its pixel's next sample), atomics to the
    film, nothing parked; then a second such launch."""
    P = gpu_pkg
    W, H = 200, 120

    def case(P, obs):
        r = P.Renderer(P.fog_box_scene(W, H), P.app_f_params(), W, H, spp=6, seed=6)
        name = r.kernel_name()
        r.render_wave(0, 3)
        snapshot(r, obs, "first")
        r.render_wave(3, 6)
        snapshot(r, obs, "end")
        k = resumes(r)
        r.close()
        return name, k
    first, k = under_every_scheduler(case, P)
    assert k == 0                                                              # (multi-sample launches carry nothing)
    film = first[-3][1].view(np.float32).reshape(H, W, 4)
    assert np.array_equal(film[..., 3], np.full((H, W), 6.0, dtype=np.float32))
    assert int(first[-2][1][0]) == W * H * 6


def test_window_with_padding_lanes_and_dry_cursors(gpu_pkg):
    """A 50 x 30 window at (13, 7) of a 128 x 64 film, four one-sample launches: 8 x 5 tiles, every border tile with padding lanes (their
    slots freed inside a fresh chunk); fewer tiles than workgroups, so fresh claims meet dry cursors and hand their 64 slots back."""
    P = gpu_pkg
    W, H = 128, 64
    win = (13, 7, 63, 37)

    def case(P, obs):
        r = P.Renderer(P.fog_box_scene(W, H), P.app_f_params(), W, H, spp=4, seed=7)
        name = r.kernel_name()
        for s in range(4):
            r.render_window(*win, s, s + 1)
        snapshot(r, obs, "end")
        k = resumes(r)
        r.close()
        return name, k
    first, k = under_every_scheduler(case, P)
    assert k > 0
    film = first[0][1].view(np.float32).reshape(H, W, 4)
    inside = np.zeros((H, W), dtype=bool)
    inside[win[1]:win[3], win[0]:win[2]] = True
    assert np.array_equal(film[..., 3], np.where(inside, np.float32(4.0), np.float32(0.0)))
    assert int(first[1][1][0]) == 50 * 30 * 4


def test_maxdepth_one_keeps_the_segment_queue_partial(gpu_pkg):
    """The fog box with maxdepth 1: a path is a camera segment, one vertex and at most one more segment, so Q_A rarely fills and its
    chunks are the partial ones taken while no vertex chunk is in flight (`busyV == 0`)."""
    P = gpu_pkg
    W, H, n = 96, 56, 4
    prm = P.app_f_params()
    prm.maxdepth = 1

    def case(P, obs):
        r = P.Renderer(P.fog_box_scene(W, H), prm, W, H, spp=n, seed=8)
        name = r.kernel_name()
        for w in range(n):
            r.render_wave(w, w + 1)
            r.post_process_wave()
        snapshot(r, obs, "end")
        k = resumes(r)
        r.close()
        return name, k
    first, _ = under_every_scheduler(case, P)
    assert int(first[1][1][0]) == W * H * n
