"""The boundary of a carried one-sample launch of k_render_wave_wg3 (csrc/vspg_wg3.h): the fresh chunk's loads issued together, the
workgroup image copied in 16-byte pieces, and the launch that suspends nothing because an update of the VSP buffer is due behind it
(csrc/vspg_capi.hip) -- all three compute what self-contained launches compute.

Reference side: the same library with VSPG_WG3_CARRY=0 (every launch drains its own paths) and with VSPG_WG2_DEFER=0 (nothing is
parked, so nothing is resolved at a pixel's start either); both are pinned to the oracle by the rest of the suite.  Film, VSP buffer,
image-space statistics and counters are compared on bit patterns after 9 one-sample waves (updates fall at wave counts 1, 2, 4, 8).

Frames are the smallest at which the hoisted loads or the image copy can go wrong: 5x3 (less than a tile: 49 padding lanes whose
pixel index lies outside the buffers), 8x8 (one tile), 203x117 (padding on both edges, several workgroups), 136x72 (153 tiles: fewer
than workgroups x 8 wavefronts, so most images are empty) and a window with odd bounds inside 203x117.

Call sequences:
  every   post_process_wave after every wave: the prediction is right (launches 1, 3, 7 suspend nothing; launch 0 has no history)
  stops   post_process_wave after waves 0..2, then never: launch 3 is predicted not to suspend and no update follows it
  step2   post_process_step(n_waves=2) after every one-sample wave: updates fall where none was predicted (launches 1, 3, 7)
  read    `every` with a film() read after wave 4
The prediction is made only for a caller that post-processed its previous step (vspg_debug_carry_kept counts the launches that took
it), so a caller that never post-processes keeps carrying: that is the sequence of the oracle comparison below, where no update may
change the VSP buffer between the samples the oracle traces."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib

pytestmark = pytest.mark.gpu

N = 9
SETTINGS = ({}, {"VSPG_WG3_CARRY": "0"}, {"VSPG_WG2_DEFER": "0"})
KEPT = {"every": 3, "stops": 2, "step2": 0, "read": 3}
GENERIC = {"VSPG_NO_GREY": "1", "VSPG_NO_GREY_KD": "1", "VSPG_NO_NULLZERO": "1"}


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


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


def dev_stats(r):
    import torch
    ptr, n = r.isg_stats_ptr()

    class Dev:
        __cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (ptr, False), "version": 2}
    r.flush()
    torch.cuda.synchronize()
    return torch.as_tensor(Dev(), device="cuda:0").cpu().numpy().copy()


def debug_count(r, name):
    f = getattr(r.lib, name)
    f.restype = C.c_longlong
    f.argtypes = [C.c_void_p]
    return int(f(r.h))


def run(P, scene, w, h, seq, env, window=None, arith=None, seed=6):
    """-> observations [(tag, words)], launches that resumed, launches that suspended nothing on a predicted update"""
    with _Env(env):
        r = P.Renderer(scene, P.app_f_params(), w, h, spp=N, seed=seed)
        if arith is not None:
            r.set_arithmetic(arith)
        obs = []
        for s in range(N):
            if window is None:
                r.render_wave(s, s + 1)
            else:
                r.render_window(*window, s, s + 1)
            if seq in ("every", "read") or (seq == "stops" and s < 3):
                r.post_process_wave()
            elif seq == "step2":
                r.post_process_step(2)
            if seq == "read" and s == 4:
                obs.append(("mid:film", u32(r.film())))
        obs.append(("end:film", u32(r.film())))
        obs.append(("end:counters", np.array(list(r.counters().values()), dtype=np.uint64)))
        obs.append(("end:vsp", u32(r.vsp_buffer()[0])))
        obs.append(("end:stats", u32(dev_stats(r))))
        out = (obs, debug_count(r, "vspg_debug_carry_resumes"), debug_count(r, "vspg_debug_carry_kept"), r.kernel_name())
        r.close()
    return out


def same(a, b, what):
    assert len(a) == len(b) and len(a) > 0
    for (ta, xa), (tb, xb) in zip(a, b):
        assert ta == tb and xa.shape == xb.shape, (what, ta, tb)
        diff = int((xa != xb).sum())
        print("%-34s %-14s %9d words, %d differ" % (what, ta, xa.size, diff))
        assert diff == 0, (what, ta)


@pytest.mark.parametrize("frame", ["5x3", "8x8", "203x117", "136x72", "window"])
def test_sequences_against_carry_off_and_defer_off(gpu_pkg, frame):
    P = gpu_pkg
    w, h = (203, 117) if frame == "window" else tuple(int(v) for v in frame.split("x"))
    window = (13, 5, 178, 91) if frame == "window" else None
    scene = P.fog_box_scene(w, h)
    for seq in ("every", "stops", "step2", "read"):
        runs = [run(P, scene, w, h, seq, env, window) for env in SETTINGS]
        obs, resumed, kept, name = runs[0]
        assert name.startswith("k_render_wave_wg3<") and "HomogeneousMediumT<2,true>" in name.replace(" ", ""), name   # the headline instantiation
        print("%s %s: %d launches resumed, %d suspended nothing" % (frame, seq, resumed, kept))
        assert kept == KEPT[seq], (seq, kept)
        assert resumed > 0, seq
        weight = obs[-4][1].view(np.float32).reshape(h, w, 4)[..., 3]
        inside = np.zeros((h, w), dtype=bool)
        x0, y0, x1, y1 = window or (0, 0, w, h)
        inside[y0:y1, x0:x1] = True
        assert np.array_equal(weight, np.where(inside, np.float32(N), np.float32(0)))   # every sample entered the film once
        for other, env in zip(runs[1:], SETTINGS[1:]):
            assert other[1] == 0 and other[2] == 0, (env, other[1], other[2])
            same(obs, other[0], "%s %s vs %s" % (frame, seq, env))


@pytest.mark.parametrize("inst", ["no-grey", "no-grey-kd", "no-nullzero", "generic", "fast"])
def test_other_instantiations_against_carry_off(gpu_pkg, inst):
    """The generic instantiations (another pool layout and size: another image) and one tolerance mode against itself."""
    P = gpu_pkg
    w, h = 203, 117
    scene = P.fog_box_scene(w, h)
    env = {"no-grey": {"VSPG_NO_GREY": "1"}, "no-grey-kd": {"VSPG_NO_GREY_KD": "1"}, "no-nullzero": {"VSPG_NO_NULLZERO": "1"}, "generic": GENERIC, "fast": {}}[inst]
    arith = P.ARITH_FAST if inst == "fast" else None
    on = run(P, scene, w, h, "every", env, arith=arith)
    off = run(P, scene, w, h, "every", dict(env, VSPG_WG3_CARRY="0"), arith=arith)
    print("%s: %s, %d resumed, %d suspended nothing" % (inst, on[3], on[1], on[2]))
    assert "k_render_wave_wg3<" in on[3], on[3]
    if inst != "fast":
        assert "HomogeneousMediumT<2,true>" not in on[3].replace(" ", ""), on[3]
    assert on[1] > 0 and on[2] == KEPT["every"] and off[1] == 0 and off[2] == 0
    same(on[0], off[0], inst)


def emitter_box(P, w, h):
    """the fog box with a two-sided light over the whole ceiling (tests/test_needless_work_gpu.py)"""
    s = P.fog_box_scene(w, h)
    q = s.quads[6]
    assert any(v != 0 for v in q.Le)
    q.p00[:] = (-1.0, 0.999, -1.0)
    q.e1[:] = (2.0, 0.0, 0.0)
    q.e2[:] = (0.0, 0.0, 2.0)
    q.Le[:] = (1.7, 1.2, 0.4)
    q.two_sided = 1
    return s


@pytest.mark.parametrize("box", ["fog", "emitter-ceiling"])
def test_film_after_carried_waves_is_the_oracles_paths(gpu_pkg, box):
    """203x117, 9 carried one-sample waves and no update (the VSP buffer stays out of the paths, so the oracle's paths of the 9
    sample indices, summed in sample order as RGBFilm::AddSample does, are the film): 400 random pixels, bit for bit."""
    P = gpu_pkg
    w, h = 203, 117
    scene = emitter_box(P, w, h) if box == "emitter-ceiling" else P.fog_box_scene(w, h)
    rng = np.random.default_rng(17)
    pix = np.stack([rng.integers(0, w, 400), rng.integers(0, h, 400)], axis=1).astype(np.int32)
    c = oracle_lib.OracleRenderer(scene, P.app_f_params(), w, h, seed=6)
    L, _ = c.trace_paths(np.repeat(pix, N, axis=0), np.tile(np.arange(N, dtype=np.int32), len(pix)))
    c.close()
    Ls = L.astype(np.float32).reshape(len(pix), N, 3)
    sums = Ls[:, 0]
    for k in range(1, N):
        sums = sums + Ls[:, k]
    assert np.count_nonzero(sums) > sums.size // 2
    obs, resumed, kept, name = run(P, scene, w, h, "never", {})
    assert name.startswith("k_render_wave_wg3<"), name
    assert resumed == N - 1 and kept == 0, (resumed, kept)
    film = obs[0][1].view(np.float32).reshape(h, w, 4)
    bad = (u32(film[pix[:, 1], pix[:, 0], :3]) != u32(sums)).any(axis=1)
    assert not bad.any(), "film != oracle paths in %d of %d pixels" % (int(bad.sum()), len(pix))
