"""The path kernels without the work their results never needed (csrc/vspg_path.h: light_pdf_li_hit at an emitter hit, the
medium vertex's shadow-ray origin without an offset; csrc/vspg_device.h: medium_ray_origin) compute what they computed: every
comparison here is on bit patterns.

  - fog box, 64 x 48, four one-sample waves: trace_paths of 2000 (pixel, sample) pairs equals the oracle's, and the film is the
    oracle's paths summed in sample order;
  - the same scene at 64 x 48 and at 16 x 16 (the pools drain through chunks that mix volume and surface vertices, so both sides of
    the shadow-ray origin's branch run in one wavefront): film, VSP buffer and counters after four waves with their post-processing
    are the same under VSPG_WG_SCHED=1, 2, the default kernel, and the default kernel with VSPG_WG3_CARRY=0;
  - a box whose light covers the whole ceiling, two-sided, and one whose light is tilted (a generic record): paths that hit the
    emitter after a bounce are in every chunk.  The film equals the oracle's replayed paths on the rectangles-only kernel, on
    k_render_wave_wg2 with guiding off (VSPG_WG_SCHED=2) and on the per-lane kernel (VSPG_KERNEL=lane);
  - the generic instantiation (VSPG_NO_GREY=1 VSPG_NO_GREY_KD=1 VSPG_NO_NULLZERO=1) at 64 x 48 gives the default kernel's film."""
import os

import numpy as np
import pytest

import oracle_lib

pytestmark = pytest.mark.gpu

N_WAVES = 4


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


def render(P, scene, prm, W, H, env, post, seed=4):
    """-> kernel name, film, VSP buffer, counters after N_WAVES one-sample waves"""
    with _Env(env):
        r = P.Renderer(scene, prm, W, H, seed=seed)
        name = r.kernel_name()
        for w in range(N_WAVES):
            r.render_wave(w, w + 1)
            if post:
                r.post_process_wave()
        out = (name, r.film(), r.vsp_buffer()[0], r.counters())
        r.close()
    return out


_ORACLE = {}


def oracle_sums(key, scene, prm, W, H, pix, seed=4):
    """The oracle's paths of N_WAVES samples per pixel of `pix`, summed in sample order as RGBFilm::AddSample does: computed once
    per scene and shared."""
    if key not in _ORACLE:
        c = oracle_lib.OracleRenderer(scene, prm, W, H, seed=seed)
        L, seg = c.trace_paths(np.repeat(pix, N_WAVES, axis=0), np.tile(np.arange(N_WAVES, dtype=np.int32), len(pix)))
        c.close()
        Ls = L.astype(np.float32).reshape(len(pix), N_WAVES, 3)
        s = Ls[:, 0]
        for k in range(1, N_WAVES):
            s = s + Ls[:, k]
        _ORACLE[key] = (L, seg, s)
    return _ORACLE[key]


def test_fog_box_paths_are_the_oracles(gpu_pkg):
    P = gpu_pkg
    W, H = 64, 48
    scene, prm = P.fog_box_scene(W, H), P.app_f_params()
    rng = np.random.default_rng(11)
    pix = np.stack([rng.integers(0, W, 500), rng.integers(0, H, 500)], axis=1).astype(np.int32)
    L, seg, sums = oracle_sums("fog", scene, prm, W, H, pix)
    g = P.Renderer(scene, prm, W, H, seed=4)
    Lg, segg = g.trace_paths(np.repeat(pix, N_WAVES, axis=0), np.tile(np.arange(N_WAVES, dtype=np.int32), len(pix)))
    g.close()
    assert len(Lg) == 2000
    assert np.array_equal(segg, seg)
    assert np.array_equal(u32(Lg), u32(L)), "trace_paths != oracle for %d pairs" % int((u32(Lg) != u32(L)).any(axis=1).sum())
    name, film, _, _ = render(P, scene, prm, W, H, {}, post=False)
    assert name.startswith("k_render_wave_wg3"), name
    assert np.array_equal(u32(film[pix[:, 1], pix[:, 0], :3]), u32(sums)), "film != oracle paths"


@pytest.mark.parametrize("wh", [(64, 48), (16, 16)])
def test_schedulers_and_carry_agree_on_film_vsp_buffer_and_counters(gpu_pkg, wh):
    P = gpu_pkg
    W, H = wh
    scene, prm = P.fog_box_scene(W, H), P.app_f_params()
    runs = [render(P, scene, prm, W, H, env, post=True) for env in ({}, {"VSPG_WG3_CARRY": "0"}, {"VSPG_WG_SCHED": "1"}, {"VSPG_WG_SCHED": "2"})]
    names = [r[0] for r in runs]
    assert names[0].startswith("k_render_wave_wg3") and len(set(names[1:])) == 3, names
    ref = runs[0]
    assert np.array_equal(ref[1][..., 3], np.full((H, W), float(N_WAVES), dtype=np.float32))
    assert ref[3]["paths"] == W * H * N_WAVES and ref[3]["volume_scatters"] > 0 and ref[3]["surface_hits"] > 0
    for name, film, vsp, cnt in runs[1:]:
        assert np.array_equal(u32(film), u32(ref[1])), name
        assert np.array_equal(u32(vsp), u32(ref[2])), name
        assert cnt == ref[3], (name, cnt, ref[3])


def emitter_box(P, W, H, tilted):
    """The fog box with a light over the whole ceiling, two-sided; `tilted`: no longer axis-aligned (a generic record)."""
    s = P.fog_box_scene(W, H)
    q = s.quads[6]
    assert any(v != 0 for v in q.Le)
    if tilted:
        q.p00[:] = (-1.0, 0.9, -1.0)
        q.e1[:] = (2.0, 0.05, 0.0)
        q.e2[:] = (0.0, 0.03, 2.0)
    else:
        q.p00[:] = (-1.0, 0.999, -1.0)
        q.e1[:] = (2.0, 0.0, 0.0)
        q.e2[:] = (0.0, 0.0, 2.0)
    q.Le[:] = (1.7, 1.2, 0.4)
    q.two_sided = 1
    return s


@pytest.mark.parametrize("light", ["ceiling", "tilted"])
def test_emitter_hits_in_every_chunk_are_the_oracles_paths(gpu_pkg, light):
    P = gpu_pkg
    W, H = 32, 24
    scene, prm = emitter_box(P, W, H, light == "tilted"), P.app_f_params()
    pix = np.stack(np.meshgrid(np.arange(W), np.arange(H)), axis=-1).reshape(-1, 2).astype(np.int32)
    _, _, sums = oracle_sums(light, scene, prm, W, H, pix)
    assert np.count_nonzero(sums) > sums.size // 2
    seen = []
    for env, prefix in (({}, "k_render_wave_wg3"), ({"VSPG_WG_SCHED": "2"}, "k_render_wave_wg2"), ({"VSPG_KERNEL": "lane"}, "k_render_wave<")):
        name, film, _, cnt = render(P, scene, prm, W, H, env, post=False)
        assert name.startswith(prefix), name
        seen.append(name)
        assert cnt["surface_hits"] > 0 and cnt["volume_scatters"] > 0
        got = film[pix[:, 1], pix[:, 0], :3]
        bad = (u32(got) != u32(sums)).any(axis=1)
        assert not bad.any(), "%s: film != oracle paths in %d of %d pixels" % (name, int(bad.sum()), len(pix))
    assert len(set(seen)) == 3


def test_generic_instantiation_gives_the_default_film(gpu_pkg):
    P = gpu_pkg
    W, H = 64, 48
    scene, prm = P.fog_box_scene(W, H), P.app_f_params()
    a = render(P, scene, prm, W, H, {}, post=True)
    b = render(P, scene, prm, W, H, {"VSPG_NO_GREY": "1", "VSPG_NO_GREY_KD": "1", "VSPG_NO_NULLZERO": "1"}, post=True)
    assert a[0] != b[0], (a[0], b[0])
    assert np.array_equal(u32(a[1]), u32(b[1]))
    assert np.array_equal(u32(a[2]), u32(b[2])) and a[3] == b[3]
