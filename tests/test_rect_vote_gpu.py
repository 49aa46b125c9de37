"""The rectangle walks with one wave vote per record (csrc/vspg_device.h: rect_hit_uv, rects_closest, rects_any) on the device: a lane's
result must not depend on what the other 63 lanes of its wavefront do at the vote, so the inputs here are arranged BY WAVEFRONT.

ray_batch (closest hit, then hit2 / any2 on the spawned ray; every field against the oracle, bit for bit) on the fog box, on the 16
rectangles of tests/test_rect_frame_gpu.py (generic and axis-aligned records mixed) and on that file's tie rays.  A batch of 4096 is
64 wavefronts of four kinds in turn:
  - every ray inside the scene with its direction (and its spawned direction) in ONE octant: for the walls behind them no lane is a
    candidate, the wavefront skips those records whole;
  - every ray outside the scene, pointing away: no record has a candidate, in either loop;
  - one of those two with ONE lane turned round: records with exactly one candidate lane, 63 lanes run a body whose result they drop;
  - random rays.
Batches of 1, 63, 64 and 65 rays are cut from it where the kinds differ (one lane; a ragged wavefront; one whole; one and a lane).

Films (four samples per pixel, bit patterns): 8 x 8, 9 x 7 and 64 x 48 frames at one and at three samples per launch, and a pixel
window of the 64 x 48 frame, equal the oracle's replayed paths summed in sample order -- 2000 (pixel, sample) pairs at 64 x 48, every
pixel of the small frames -- and are the same bytes under the default kernel, VSPG_WG3_CARRY=0, VSPG_WG_SCHED=1 and 2, the generic
instantiation (VSPG_NO_GREY, VSPG_NO_GREY_KD, VSPG_NO_NULLZERO) and the per-lane kernel.  The guided fog box (k_render_wave_wg2,
guided) and a fog box with one triangle in it (the full-scene instantiation, the same loops through scene_intersect<true>) equal
the oracle's film."""
import os

import numpy as np
import pytest

import oracle_lib
from test_rect_frame_gpu import _check_ties, _random_queries, _same_bits, edge_and_corner_queries, sixteen_rectangles   # that file's scenes and rays, by its own builders

pytestmark = pytest.mark.gpu

N_SAMPLES = 4
ENVS = [("default", {}, "k_render_wave_wg3"),
        ("carry off", {"VSPG_WG3_CARRY": "0"}, "k_render_wave_wg3"),
        ("sched 1", {"VSPG_WG_SCHED": "1"}, "k_render_wave_wg<"),
        ("sched 2", {"VSPG_WG_SCHED": "2"}, "k_render_wave_wg2"),
        ("generic", {"VSPG_NO_GREY": "1", "VSPG_NO_GREY_KD": "1", "VSPG_NO_NULLZERO": "1"}, "k_render_wave_wg3"),
        ("per lane", {"VSPG_KERNEL": "lane"}, "k_render_wave<")]


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


# ---- ray batches, arranged by wavefront ---------------------------------------------------------------------------------------
def wavefront_queries(P, span, seed):
    """4096 rays = 64 wavefronts; wavefront w is of kind w % 4 (see the module text).  `span`: the scene lies within [-span, span]^3."""
    rng = np.random.default_rng(seed)
    q = _random_queries(P, 4096, seed, span)
    kinds = np.arange(64) % 4
    for w in range(64):
        s = slice(64 * w, 64 * w + 64)
        if kinds[w] == 3:
            continue
        octant = np.array([1.0 if (w >> (2 + k)) & 1 else -1.0 for k in range(3)], dtype=np.float32)
        away = kinds[w] == 1 or (kinds[w] == 2 and (w >> 5) & 1)
        d = np.abs(q["d"][s]) + np.float32(1e-3)
        q["d"][s] = d * octant
        q["mode"][s] = 1                                         # the spawned ray: a direction, in the same octant
        q["w"][s] = (np.abs(q["w"][s]) + np.float32(1e-3)) * octant
        if away:
            q["o"][s] = (span * rng.uniform(1.05, 1.5, (64, 3))).astype(np.float32) * octant
        if kinds[w] == 2:
            lane = 64 * w + (w * 7) % 64
            q["d"][lane] = -q["d"][lane]
            q["w"][lane] = -q["w"][lane]
    return q, kinds


def _batch_cases(P, which):
    if which == "fog box":
        scene = P.fog_box_scene(8, 8)
        q, kinds = wavefront_queries(P, 0.98, 21)
    elif which == "sixteen rectangles":
        scene = sixteen_rectangles(P)
        q, kinds = wavefront_queries(P, 1.6, 22)
    else:
        scene = P.fog_box_scene(8, 8)
        e = edge_and_corner_queries(P)
        q, kinds = np.resize(e, 4096), None
    return scene, q, kinds


@pytest.mark.parametrize("which", ["fog box", "sixteen rectangles", "edges and corners"])
def test_ray_batches_by_wavefront_equal_the_oracle(gpu_pkg, which):
    P = gpu_pkg
    scene, q, kinds = _batch_cases(P, which)
    prm = P.app_f_params()
    g = P.Renderer(scene, prm, 8, 8)
    o = oracle_lib.OracleRenderer(scene, prm, 8, 8)
    want = o.ray_batch(q)
    o.close()
    # 1, 63, 64, 65 rays from where the wavefront kinds differ (waves 0..3 are kinds 0..3; wave 2 holds the one turned lane), then all
    cuts = [(0, 4096)] + [(64 * w + a, n) for n in (1, 63, 64, 65) for w, a in ((0, 0), (1, 0), (2, 0), (2, (2 * 7) % 64), (3, 5))]
    for start, n in cuts:
        got = g.ray_batch(q[start:start + n])
        assert len(got) == n
        _same_bits(want[start:start + n], got, "%s, rays [%d, %d)" % (which, start, start + n))
    g.close()
    hit = want["hit"].reshape(64, 64) != 0
    if kinds is None:
        _check_ties(P, q[:len(edge_and_corner_queries(P))], want[:len(edge_and_corner_queries(P))])
        return
    print("%s: hits per wavefront kind %s, spawned hits %d, occluded %d" % (
        which, [int(hit[kinds == k].sum()) for k in range(4)], int(want["hit2"].sum()), int(want["any2"].sum())))
    # the arrangement reaches what it is meant for
    assert not hit[kinds == 1].any() and not (want["hit2"].reshape(64, 64)[kinds == 1] != 0).any()      # pointing away: nothing, for a whole wavefront
    away_turned = [w for w in range(64) if kinds[w] == 2 and (w >> 5) & 1]
    for w in away_turned:                                                                              # ... and with one lane turned: at most that lane
        assert not np.delete(hit[w], (w * 7) % 64).any()
    assert hit[kinds == 0].any() and hit[kinds == 3].any() and 0 < want["any2"].sum() and 0 < want["hit2"].sum()
    if which == "fog box":
        # a closed box: the turned lanes look at it from outside, the octant wavefronts hit a wall in front unless tMax ends them first
        assert sum(int(hit[w, (w * 7) % 64]) for w in away_turned) > 0
        assert hit[kinds == 0].mean() > 0.8


# ---- films ----------------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle_sums(W, H, seed=4):
    """-> pixels, and the oracle's N_SAMPLES paths per pixel summed in sample order (RGBFilm::AddSample); once per frame size"""
    if (W, H) not in _ORACLE:
        P = oracle_lib
        if W * H * N_SAMPLES <= 2000:
            pix = np.stack(np.meshgrid(np.arange(W), np.arange(H)), axis=-1).reshape(-1, 2).astype(np.int32)
        else:
            rng = np.random.default_rng(5)
            pix = np.stack([rng.integers(0, W, 2000 // N_SAMPLES), rng.integers(0, H, 2000 // N_SAMPLES)], axis=1).astype(np.int32)
        c = P.OracleRenderer(P.fog_box_scene(W, H), P.app_f_params(), W, H, seed=seed)
        L, _ = c.trace_paths(np.repeat(pix, N_SAMPLES, axis=0), np.tile(np.arange(N_SAMPLES, dtype=np.int32), len(pix)))
        c.close()
        Ls = L.astype(np.float32).reshape(len(pix), N_SAMPLES, 3)
        s = Ls[:, 0]
        for k in range(1, N_SAMPLES):
            s = s + Ls[:, k]
        _ORACLE[(W, H)] = (pix, s)
    return _ORACLE[(W, H)]


def _render(P, W, H, env, per_launch, window=None, seed=4):
    with _Env(env):
        r = P.Renderer(P.fog_box_scene(W, H), P.app_f_params(), W, H, seed=seed)
        name = r.kernel_name()
        s = 0
        while s < N_SAMPLES:
            e = min(s + per_launch, N_SAMPLES)
            if window is None:
                r.render_wave(s, e)
            else:
                r.render_window(*window, s, e)
            s = e
        out = (name, r.film(), r.counters())
        r.close()
    return out


@pytest.mark.parametrize("per_launch", [1, 3])
@pytest.mark.parametrize("wh", [(8, 8), (9, 7), (64, 48)])
def test_films_are_the_oracles_paths_on_every_kernel(gpu_pkg, wh, per_launch):
    P = gpu_pkg
    W, H = wh
    pix, sums = _oracle_sums(W, H)
    assert len(pix) * N_SAMPLES == (2000 if wh == (64, 48) else W * H * N_SAMPLES)
    ref = None
    names = set()
    for label, env, prefix in ENVS:
        name, film, cnt = _render(P, W, H, env, per_launch)
        assert name.startswith(prefix), (label, name)
        names.add(name)
        if ref is None:
            ref = (film, cnt)
            assert np.array_equal(film[..., 3], np.full((H, W), float(N_SAMPLES), dtype=np.float32))
            bad = (u32(film[pix[:, 1], pix[:, 0], :3]) != u32(sums)).any(axis=1)
            assert not bad.any(), "%s: film != oracle paths in %d of %d pixels" % (name, int(bad.sum()), len(pix))
            assert cnt["paths"] == W * H * N_SAMPLES and cnt["surface_hits"] > 0 and cnt["shadow_rays"] > 0
        else:
            assert np.array_equal(u32(film), u32(ref[0])), (label, name)
            assert cnt == ref[1], (label, cnt, ref[1])
    assert len(names) >= 5, sorted(names)   # (carry on / off may share a name; every other row is a kernel of its own)


@pytest.mark.parametrize("per_launch", [1, 3])
def test_pixel_window_films_are_the_oracles_paths(gpu_pkg, per_launch):
    P = gpu_pkg
    W, H = 64, 48
    win = (5, 3, 42, 31)   # unaligned on every side: ragged tiles, wavefronts with lanes outside the window
    pix, sums = _oracle_sums(W, H)
    inside = (pix[:, 0] >= win[0]) & (pix[:, 0] < win[2]) & (pix[:, 1] >= win[1]) & (pix[:, 1] < win[3])
    assert 100 < inside.sum() < len(pix)
    mask = np.zeros((H, W), dtype=bool)
    mask[win[1]:win[3], win[0]:win[2]] = True
    ref = None
    for label, env, prefix in ENVS:
        name, film, cnt = _render(P, W, H, env, per_launch, window=win)
        assert name.startswith(prefix), (label, name)
        if ref is None:
            ref = film
            assert not u32(film)[~mask].any()
            assert np.array_equal(film[mask][:, 3], np.full(int(mask.sum()), float(N_SAMPLES), dtype=np.float32))
            got = film[pix[inside, 1], pix[inside, 0], :3]
            assert np.array_equal(u32(got), u32(sums[inside])), "%s: window film != oracle paths" % name
            assert cnt["paths"] == int(mask.sum()) * N_SAMPLES
        else:
            assert np.array_equal(u32(film), u32(ref)), (label, name)


def _one_triangle_box(P, W, H):
    s = P.fog_box_scene(W, H)
    tri = np.array([[[-0.6, -0.4, 0.3], [0.5, -0.5, 0.1], [0.0, 0.45, 0.4]]], dtype=np.float32)
    P.set_triangles(s, tri, np.array([[0.6, 0.45, 0.3]], dtype=np.float32))
    return s


@pytest.mark.parametrize("which", ["guided", "one triangle"])
def test_guided_and_full_scene_kernels_equal_the_oracles_film(gpu_pkg, which):
    P = gpu_pkg
    import scenes
    W, H = 24, 16
    if which == "guided":
        scene, prm, field, prefix = P.fog_box_scene(W, H), P.default_params(), scenes.light_field(P, n=4), "k_render_wave_wg2<HomogeneousMediumT<2,true>,guided"
    else:
        scene, prm, field, prefix = _one_triangle_box(P, W, H), P.app_f_params(), None, "k_render_wave_wg2<HomogeneousMedium"
    g = P.Renderer(scene, prm, W, H, seed=4)
    c = oracle_lib.OracleRenderer(scene, prm, W, H, seed=4)
    if field is not None:
        g.set_guiding_field(field, field)
        c.set_guiding_field(field, field)
    assert g.kernel_name().startswith(prefix), g.kernel_name()
    for w in range(2):
        g.render_wave(w, w + 1)
        c.render_wave(w, w + 1)
    fg, fc, cg, cc = g.film(), c.film(), g.counters(), c.counters()
    g.close()
    c.close()
    assert cg["surface_hits"] > 0 and cg["shadow_rays"] > 0
    assert np.array_equal(u32(fg), u32(fc)), "%s: film bits differ in %d values" % (which, int((u32(fg) != u32(fc)).sum()))
    assert cg == cc, (cg, cc)
