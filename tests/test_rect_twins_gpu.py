"""The closest-hit walk that tests the two walls of a twin pair in one pass (csrc/vspg_device.h: rect_twins_mark, rects_closest_twins)
on the device: what a lane reports must not depend on which way its wavefront goes at the pair's two votes -- merged body, fallback
to the plain iterations, or on to the record after the pair -- so the rays here are arranged BY WAVEFRONT.

ray_batch (closest hit, then hit2 / any2 on the spawned ray; every field against the oracle, bit for bit) on the fog box, on the
same box seen from outside and on 16 records with seven twin pairs (every transition between two frames, both (u, v) orders, a
generic record between pairs).  4096 rays are 64 wavefronts of four kinds in turn:
  0 every lane inside every slab: no lane is a candidate of both walls of any pair, every pair runs merged (outside view: every lane
    outside, aimed at the box: whole wavefronts fall back);
  1 the same with ONE lane moved outside the first pair's slab and aimed at it: exactly one both-candidate lane, the wavefront falls
    back for that pair (outside view: one lane moved inside);
  2 mixed: origins inside and outside, a tenth with a finite tMax;
  3 every lane outside, pointing away: no candidate of anything.
The arrangement is checked here with the pre-test's sign rule at tMax = inf, which is exact for the first pair of a list.

Films of a 128 x 64 fog box at four samples equal the oracle's replayed paths on k_render_wave_wg3 through both entry points, its
generic instantiation, k_render_wave_wg, _wg2 and the per-lane kernel, and are the same bytes on all of them; film, VSP buffer and
counters are the same bytes under the three schedulers.  The guided _wg2 equals the oracle's film (two films of two samples), and the wavefront pipeline over a
small grid medium in the same room equals the oracle's paths and the per-lane kernel."""
import numpy as np
import pytest

import oracle_lib
import scenes
from test_rect_any_table_gpu import grid_box
from test_rect_frame_gpu import _random_queries, _same_bits
from test_rect_vote_gpu import ENVS, N_SAMPLES, _Env, u32

pytestmark = pytest.mark.gpu

W, H = 128, 64
PAIR_AXES = (0, -1, 1, 2, 0, -1, 2, 1, 0)   # the 16 records' entries: a twin pair on that axis, or (-1) one generic record


def sixteen_twins(P):
    """pairs x G y z x G z y x: nested slabs (half width 0.45 + 0.11 k), every other pair with one wall's e1 / e2 traded"""
    s = oracle_lib.fog_box_scene(8, 8)
    s.n_quads = 0
    s.medium.type = P.MEDIUM_NONE
    rng = np.random.default_rng(61)
    pair = 0
    for a in PAIR_AXES:
        if a < 0:
            first = s.n_quads < 4
            e1 = np.array([1.5, 0.2, 0.6 if first else -0.5])
            e2 = np.array([-0.1, 1.7, 0.3])
            e2 = e2 - e1 * (e1 @ e2) / (e1 @ e1)
            P.add_quad(s, (-0.8, -0.9, -0.3 if first else 0.4), tuple(float(np.float32(v)) for v in e1), tuple(float(np.float32(v)) for v in e2),
                       reverse=not first)
            continue
        a1, a2 = (a + 1) % 3, (a + 2) % 3
        half = 0.45 + 0.11 * pair
        c1, c2 = rng.uniform(-1.4, -0.9, 2)
        l1, l2 = rng.uniform(1.9, 2.6, 2)
        for w in range(2):
            p00, e1, e2 = [0.0] * 3, [0.0] * 3, [0.0] * 3
            p00[a], p00[a1], p00[a2] = (half if w else -half - 0.02 * pair), c1, c2
            if (pair + w) & 1 and (pair % 3 != 0 or w == 1):
                e1[a2], e2[a1] = l2, l1
            else:
                e1[a1], e2[a2] = l1, l2
            P.add_quad(s, p00, e1, e2, le=(3, 3, 3) if s.n_quads == 0 else (0, 0, 0), reverse=((pair >> 1) & 1) != w)
        pair += 1
    assert s.n_quads == 16 and pair == 7
    return s


# (the first pair's axis, its two planes, the half width within which an origin is inside EVERY slab, the scene's span)
VIEWS = {"fog box": (1, (-1.0, 1.0), 0.98, 1.0), "outside view": (1, (-1.0, 1.0), 0.98, 1.0), "sixteen twins": (0, (-0.45, 0.45), 0.44, 1.3)}


def twin_wavefronts(P, view, seed):
    axis, planes, inner, span = VIEWS[view]
    rng = np.random.default_rng(seed)
    q = _random_queries(P, 4096, seed, 3.0 * span)                 # kind 2 as it stands, but for half of its origins (below)
    kinds = np.arange(64) % 4
    for w in range(64):
        s = slice(64 * w, 64 * w + 64)
        inside = rng.uniform(-inner, inner, (64, 3)).astype(np.float32)
        if kinds[w] == 2:
            q["o"][s][::2] = inside[::2]
            continue
        octant = np.array([1.0 if (w >> (2 + k)) & 1 else -1.0 for k in range(3)], dtype=np.float32)
        outside = (span * rng.uniform(1.05, 2.5, (64, 3))).astype(np.float32) * octant
        q["tMax"][s] = np.inf
        q["mode"][s] = 1
        if kinds[w] == 3:                                            # outside, pointing away, the spawned ray too
            q["o"][s] = outside
            q["d"][s] = (np.abs(q["d"][s]) + np.float32(1e-3)) * octant
            q["w"][s] = (np.abs(q["w"][s]) + np.float32(1e-3)) * octant
            continue
        aimed = (rng.uniform(-0.4, 0.4, (64, 3)) * span).astype(np.float32) - outside   # from outside towards the middle of the scene
        lane = 64 * w + (w * 7) % 64
        if view == "outside view":
            q["o"][s] = outside
            q["d"][s] = aimed
            if kinds[w] == 1:
                q["o"][lane] = inside[0]
        else:
            q["o"][s] = inside
            q["d"][s] = np.where(np.abs(q["d"][s]) < 1e-3, np.float32(0.5), q["d"][s])
            if kinds[w] == 1:
                q["o"][lane] = outside[0]
                q["d"][lane] = aimed[0]
    return q, kinds


def _both_candidates(q, axis, planes):
    """lanes that pass the sign pre-test of BOTH planes of the first pair (tMax = inf: nothing is beyond)"""
    d = q["d"][:, axis]
    both = np.ones(len(q), dtype=bool)
    for c in planes:
        num = np.float32(c) - q["o"][:, axis]
        both &= (u32(num) ^ u32(d)) >> 31 == 0
    return both.reshape(64, 64)


@pytest.mark.parametrize("view", sorted(VIEWS))
def test_ray_batches_by_wavefront_equal_the_oracle(gpu_pkg, view):
    P = gpu_pkg
    scene = sixteen_twins(P) if view == "sixteen twins" else P.fog_box_scene(8, 8)
    q, kinds = twin_wavefronts(P, view, 71 + len(view))
    axis, planes, _, _ = VIEWS[view]
    both = _both_candidates(q, axis, planes)
    per_wave = both.sum(axis=1)
    print("%s: both-candidate lanes per wavefront kind %s" % (view, [per_wave[kinds == k].tolist() for k in range(4)]))
    # the arrangement reaches what it is meant for
    if view == "outside view":
        assert (per_wave[kinds == 0] == 64).all() and (per_wave[kinds == 1] == 63).all()
    else:
        assert (per_wave[kinds == 0] == 0).all() and (per_wave[kinds == 1] == 1).all()
    assert ((per_wave[kinds == 2] > 0) & (per_wave[kinds == 2] < 64)).all() and (per_wave[kinds == 3] == 0).all()
    prm = P.app_f_params()
    o = oracle_lib.OracleRenderer(scene, prm, 8, 8)
    want = o.ray_batch(q)
    o.close()
    g = P.Renderer(scene, prm, 8, 8)
    # all of it, then one wavefront of each kind on its own, a ragged one, one lane, one and a lane
    for start, n in [(0, 4096), (0, 64), (64, 64), (128, 64), (192, 64), (64, 63), (64 + 7, 1), (256, 65)]:
        got = g.ray_batch(q[start:start + n])
        assert len(got) == n
        _same_bits(want[start:start + n], got, "%s, rays [%d, %d)" % (view, start, start + n))
    g.close()
    hit = want["hit"].reshape(64, 64) != 0
    print("%s: hits per wavefront kind %s, spawned hits %d, occluded %d" % (
        view, [int(hit[kinds == k].sum()) for k in range(4)], int(want["hit2"].sum()), int(want["any2"].sum())))
    assert not hit[kinds == 3].any()
    assert hit[kinds == 0].mean() > 0.5 and hit[kinds == 1].any() and hit[kinds == 2].any() and want["hit2"].sum() > 0
    if view != "outside view":
        assert len(np.unique(want["prim"][(want["hit"] != 0)])) == scene.n_quads   # every record wins some ray, second walls too


_PATHS = {}


def _paths(P, which):
    """-> pixels, and the oracle's N_SAMPLES replayed paths per pixel summed in sample order (RGBFilm::AddSample); once per scene"""
    if which not in _PATHS:
        rng = np.random.default_rng(5)
        pix = np.stack([rng.integers(0, W, 2000 // N_SAMPLES), rng.integers(0, H, 2000 // N_SAMPLES)], axis=1).astype(np.int32)
        scene = P.fog_box_scene(W, H) if which == "fog" else grid_box(P, W, H, False)
        c = oracle_lib.OracleRenderer(scene, P.app_f_params(), W, H, seed=4)
        L, _ = c.trace_paths(np.repeat(pix, N_SAMPLES, axis=0), np.tile(np.arange(N_SAMPLES, dtype=np.int32), len(pix)))
        c.close()
        Ls = L.astype(np.float32).reshape(len(pix), N_SAMPLES, 3)
        s = Ls[:, 0]
        for k in range(1, N_SAMPLES):
            s = s + Ls[:, k]
        _PATHS[which] = (pix, s)
    return _PATHS[which]


def _render(P, scene, env):
    with _Env(env):
        r = P.Renderer(scene, P.app_f_params(), W, H, seed=4)
        name = r.kernel_name()
        for w in range(N_SAMPLES):
            r.render_wave(w, w + 1)
        vsp, ready = r.vsp_buffer()
        out = (name, r.film(), r.counters(), (vsp, ready))
        r.close()
    return out


def test_fog_box_films_are_the_oracles_paths_on_every_kernel(gpu_pkg):
    P = gpu_pkg
    pix, sums = _paths(P, "fog")
    ref = None
    names = set()
    for label, env, prefix in ENVS:
        name, film, cnt, vsp = _render(P, P.fog_box_scene(W, H), env)
        assert name.startswith(prefix), (label, name)
        names.add(name)
        if ref is None:
            ref = (film, cnt, vsp)
            assert np.array_equal(film[..., 3], np.full((H, W), float(N_SAMPLES), dtype=np.float32))
            bad = (u32(film[pix[:, 1], pix[:, 0], :3]) != u32(sums)).any(axis=1)
            assert not bad.any(), "%s: film != oracle paths in %d of %d pixels" % (name, int(bad.sum()), len(pix))
            assert cnt["paths"] == W * H * N_SAMPLES and cnt["surface_hits"] > 0 and cnt["shadow_rays"] > 0
        else:
            assert np.array_equal(u32(film), u32(ref[0])), (label, name)
            assert cnt == ref[1], (label, cnt, ref[1])
            if label in ("sched 1", "sched 2"):   # the three schedulers: film, VSP buffer and counters, every byte
                assert vsp[1] == ref[2][1] and vsp[0].tobytes() == ref[2][0].tobytes(), (label, name)
    assert len(names) >= 5, sorted(names)   # (carry on / off may share a name; every other row is a kernel of its own)


def test_wavefront_pipeline_film_is_the_oracles_paths(gpu_pkg):
    P = gpu_pkg
    pix, sums = _paths(P, "grid")
    name, film, cnt, _ = _render(P, grid_box(P, W, H, False), {})
    lane_name, lane_film, _, _ = _render(P, grid_box(P, W, H, False), {"VSPG_KERNEL": "lane"})
    print("%s: %s" % (name, cnt))
    assert name.startswith("k_wf_"), name
    assert lane_name.startswith("k_render_wave<"), lane_name
    assert cnt["shadow_rays"] > 0 and cnt["surface_hits"] > 0
    bad = (u32(film[pix[:, 1], pix[:, 0], :3]) != u32(sums)).any(axis=1)
    assert not bad.any(), "%s: film != oracle paths in %d of %d pixels" % (name, int(bad.sum()), len(pix))
    assert np.array_equal(u32(film), u32(lane_film)), name


def test_guided_workgroup_kernel_equals_the_oracles_film(gpu_pkg):
    """The oracle's film accumulates in double and the device's in float: the sum of TWO samples rounds once either way, a third
    would not.  So the four samples go into two films of two samples each (0, 1 and 2, 3), each equal to the oracle's, every bit."""
    P = gpu_pkg
    scene, prm, field = P.fog_box_scene(W, H), P.default_params(), scenes.light_field(P, n=4)
    for first in range(0, N_SAMPLES, 2):
        g = P.Renderer(scene, prm, W, H, seed=4)
        c = oracle_lib.OracleRenderer(scene, prm, W, H, seed=4)
        g.set_guiding_field(field, field)
        c.set_guiding_field(field, field)
        name = g.kernel_name()
        assert name.startswith("k_render_wave_wg2<") and "guided" in name, name
        for w in range(first, first + 2):
            g.render_wave(w, w + 1)
            c.render_wave(w, w + 1)
        fg, fc, cg, cc = g.film(), c.film(), g.counters(), c.counters()
        g.close()
        c.close()
        assert cg["surface_hits"] > 0 and cg["shadow_rays"] > 0
        assert np.array_equal(u32(fg), u32(fc)), "%s, samples %d and %d: film bits differ in %d values" % (name, first, first + 1, int((u32(fg) != u32(fc)).sum()))
        assert cg == cc, (cg, cc)
