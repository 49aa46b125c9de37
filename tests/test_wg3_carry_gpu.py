"""k_render_wave_wg3_carry: one-sample launches that hand their in-flight paths to the next launch (csrc/vspg_wg3.h, CARRY) compute
exactly what self-contained launches compute.

Reference side: the same library with VSPG_WG3_CARRY=0 -- today's k_render_wave_wg3, itself pinned to the oracle by the rest of the
suite.  Every scenario is a function that drives renderers and records observations (film, VSP buffer, image-space statistics,
counters); it runs once per setting and the two lists are compared on bit patterns.  Each scenario also reports how many launches
resumed paths (vspg_debug_carry_resumes): with carrying on that must be what the scenario expects, with it off zero -- a test that
passes because the feature silently stayed off shows nothing."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dev_stats(r):
    import torch
    ptr, n = r.isg_stats_ptr()

    class Dev:
        __cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (ptr, False), "version": 2}
    r.flush()
    torch.cuda.synchronize()
    return torch.as_tensor(Dev(), device="cuda:0").cpu().numpy().copy()


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
    """everything the issue compares, at this point of the sequence (each read drains, on both sides alike)"""
    obs.append((tag + ":film", u32(r.film())))
    obs.append((tag + ":counters", np.array(list(r.counters().values()), dtype=np.uint64)))
    obs.append((tag + ":vsp", u32(r.vsp_buffer()[0])))
    obs.append((tag + ":stats", u32(dev_stats(r))))


def both(scenario, P, env=None):
    """-> resumed launches with carrying on; asserts the observations equal those with carrying off, where nothing resumes"""
    out = []
    for carry in ("1", "0"):
        with _Env(dict(env or {}, VSPG_WG3_CARRY=carry)):
            obs = []
            n = scenario(P, obs)
            out.append((obs, n))
    (a, na), (b, nb) = out
    assert nb == 0, "VSPG_WG3_CARRY=0 still resumed %d launches" % nb
    assert len(a) == len(b) and len(a) > 0
    for (ta, xa), (tb, xb) in zip(a, b):
        assert ta == tb
        diff = int((xa != xb).sum()) if xa.shape == xb.shape else -1
        print("%-28s %9d words, %d differ" % (ta, xa.size, diff))
        assert diff == 0, ta
    return na


def fog(P, w, h, chromatic=False):
    scene = P.fog_box_scene(w, h)
    if chromatic:   # sigma_s no longer grey: the HomogeneousMediumSimple instantiation
        scene.medium.sigma_s[0] *= 1.25
        scene.medium.sigma_s[2] *= 0.8
    return scene


def waves(r, w0, w1, stream=None):
    for w in range(w0, w1):
        r.render_wave(w, w + 1, stream)
        r.post_process_wave(stream)


@pytest.mark.parametrize("inst", ["grey-nullzero", "grey", "chromatic"])
def test_full_frame_sequence_is_bit_identical(gpu_pkg, inst):
    """1920x1080 fog box, 24 one-sample waves with post_process_wave after each (updates at waves 1, 2, 4, 8, 16 inside)."""
    P = gpu_pkg
    n = 24

    def scenario(P, obs):
        r = P.Renderer(fog(P, 1920, 1080, chromatic=inst == "chromatic"), P.app_f_params(), 1920, 1080, spp=n, seed=3)
        expect = {"grey-nullzero": "HomogeneousMediumT<2,true>", "grey": "HomogeneousMediumT<2,false>", "chromatic": "HomogeneousMediumT<0"}[inst]
        assert r.kernel_name().startswith("k_render_wave_wg3<") and expect in r.kernel_name().replace(" ", ""), r.kernel_name()
        waves(r, 0, n)
        snapshot(r, obs, "end")
        k = resumes(r)
        r.close()
        return k
    k = both(scenario, P, {"VSPG_NO_NULLZERO": "1"} if inst == "grey" else {})
    # a launch resumes unless the wave before it ended in a buffer update (1, 2, 4, 8, 16) or is the first: 24 - 1 - 5
    assert k == n - 6, k


@pytest.mark.parametrize("wh", [(8, 8), (64, 64), (100, 60), (160, 96)])
def test_small_frames_drain_old_paths_before_suspending(gpu_pkg, wh):
    """The cursors are dry at once (8x8: one tile; 100x60: tile padding; 160x96: 240 tiles, fewer than workgroups): a workgroup
    finishes the paths it resumed before it suspends the new ones."""
    P = gpu_pkg
    w, h = wh

    def scenario(P, obs):
        r = P.Renderer(fog(P, w, h), P.app_f_params(), w, h, spp=21, seed=5)
        waves(r, 0, 11)
        snapshot(r, obs, "mid")
        waves(r, 11, 21)
        snapshot(r, obs, "end")
        k = resumes(r)
        r.close()
        return k
    assert both(scenario, P) > 0


def test_windows_multi_sample_calls_and_reads_in_the_middle(gpu_pkg):
    P = gpu_pkg
    w, h = 200, 120
    a, b = (13, 5, 177, 90), (40, 20, 200, 120)

    def scenario(P, obs):
        r = P.Renderer(fog(P, w, h), P.app_f_params(), w, h, spp=40, seed=7)
        for s in range(0, 4):                      # a window kept over several waves ...
            r.render_window(*a, s, s + 1)
        k_kept = resumes(r)
        for s in range(4, 7):                      # ... then changed
            r.render_window(*b, s, s + 1)
        snapshot(r, obs, "windows")
        waves(r, 7, 10)
        r.render_wave(10, 13)                      # a multi-sample call in the middle
        waves(r, 13, 16)
        obs.append(("film-mid", u32(r.film())))
        waves(r, 16, 18)
        obs.append(("counters-mid", np.array(list(r.counters().values()), dtype=np.uint64)))
        waves(r, 18, 20)
        r.reset_counters()
        waves(r, 20, 22)
        obs.append(("counters-after-reset", np.array(list(r.counters().values()), dtype=np.uint64)))
        waves(r, 22, 24)
        r.film_clear()
        waves(r, 24, 27)
        snapshot(r, obs, "end")
        k = resumes(r)
        r.close()
        return k if k_kept == 3 or k == 0 else -1   # (the kept window: launches 1..3 resume)
    assert both(scenario, P) > 3


def test_arithmetic_switch_two_renderers_two_streams(gpu_pkg):
    import torch
    P = gpu_pkg
    w, h = 160, 120

    def scenario(P, obs):
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        r = P.Renderer(fog(P, w, h), P.app_f_params(), w, h, spp=40, seed=9)
        q = P.Renderer(fog(P, w, h, chromatic=True), P.app_f_params(), w, h, spp=40, seed=11)
        for s in range(0, 6):                      # two renderers interleaved on one stream
            r.render_wave(s, s + 1, s1.cuda_stream)
            q.render_wave(s, s + 1, s1.cuda_stream)
        r.set_arithmetic(P.ARITH_FAST)             # switched mid-sequence: paths in flight end in the mode they started in
        for s in range(6, 9):
            r.render_wave(s, s + 1, s1.cuda_stream)
        r.set_arithmetic(P.ARITH_EXACT)
        for s in range(9, 15):                     # consecutive waves on two different streams
            r.render_wave(s, s + 1, (s1 if s & 1 else s2).cuda_stream)
            q.render_wave(s, s + 1, (s2 if s & 1 else s1).cuda_stream)
        torch.cuda.synchronize()
        snapshot(r, obs, "r")
        snapshot(q, obs, "q")
        k = resumes(r) + resumes(q)
        r.close(); q.close()
        return k
    assert both(scenario, P) > 10


def test_close_with_paths_pending_leaks_nothing(gpu_pkg):
    P = gpu_pkg
    w, h = 320, 200

    def scenario(P, obs):
        r = P.Renderer(fog(P, w, h), P.app_f_params(), w, h, spp=8, seed=13)
        for s in range(4):
            r.render_wave(s, s + 1)
        k = resumes(r)
        r.close()                                   # paths pending: freed, not run
        n = P.Renderer(fog(P, w, h), P.app_f_params(), w, h, spp=8, seed=13)
        waves(n, 0, 3)
        snapshot(n, obs, "new")
        k += resumes(n)
        n.close()
        return k
    assert both(scenario, P) >= 3


def test_sharded_sequence(gpu_pkg):
    """shard_count 2, both indices, each carrying over its own sample indices: every shard == itself without carrying.  The two
    films summed: the weight plane == one renderer's exactly; the radiance sums the same float samples in another order (even
    indices, odd indices, then the two halves -- not one after the other), so it agrees to the rounding of a 12-term float sum,
    not bit for bit: |a - b| <= 12 * 2^-24 * sum|samples| <= 1e-6 * (1 + |b|) * 12 per channel."""
    P = gpu_pkg
    w, h, steps = 200, 120, 6

    def scenario(P, obs):
        k = 0
        for idx in (0, 1):
            r = P.Renderer(fog(P, w, h), P.app_f_params(), w, h, spp=2 * steps, seed=3, shard_index=idx, shard_count=2)
            for i in range(steps):
                r.render_wave(2 * i, 2 * i + 2)
            obs.append(("shard%d:film" % idx, u32(r.film())))
            obs.append(("shard%d:counters" % idx, np.array(list(r.counters().values()), dtype=np.uint64)))
            k += resumes(r)
            r.close()
        return k
    with _Env({"VSPG_WG3_CARRY": "1"}):
        obs = []
        scenario(P, obs)
        one = P.Renderer(fog(P, w, h), P.app_f_params(), w, h, spp=2 * steps, seed=3)
        for s in range(2 * steps):
            r = one.render_wave(s, s + 1)
        f1 = one.film()
        one.close()
    total = obs[0][1].view(np.float32).reshape(h, w, 4) + obs[2][1].view(np.float32).reshape(h, w, 4)
    assert np.array_equal(total[..., 3], f1[..., 3])
    assert np.all(np.abs(total[..., :3] - f1[..., :3]) <= 12e-6 * (1 + np.abs(f1[..., :3])))
    assert int(obs[1][1][0]) + int(obs[3][1][0]) == w * h * 2 * steps
    assert both(scenario, P) == 2 * (steps - 1)
