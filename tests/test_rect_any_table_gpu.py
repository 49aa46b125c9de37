"""The any-hit walk in two stages (csrc/vspg_device.h: RectPlanes, rects_any_planes) on the device: the pre-pass votes per plane over
the wavefront, so the inputs here are arranged BY WAVEFRONT, and every answer is the oracle's.

ray_batch (every field against the oracle, bit for bit; any2 is the any-hit query of the spawned ray) on the fog box, the 16
rectangles of tests/test_rect_frame_gpu.py (five planes on x and on z: the fifth is walked without a pre-test; two tilted records),
one axis-aligned rectangle, and two tilted rectangles with no axis-aligned one.  On the fog box 256 rays = four wavefronts, every
first ray hitting a wall near its middle, the spawned ray going towards a point (mode 2):
  0  tMax2 = 1e-4 and targets inside the room: no lane is a candidate of any plane -- the pre-pass ends the walk;
  1  the same with ONE lane at tMax2 = infinity: planes with exactly one candidate lane;
  2  random targets inside and outside the room, random tMax2: mixed;
  3  lane l aims through wall l % 6 at a target outside the room, tMax2 = 2: the lanes are candidates of different records.
What each wavefront is meant to be is checked from the spawned rays the oracle reports, with the pre-test's own float32 operations.
The other scenes take the wavefront arrangement of tests/test_rect_vote_gpu.py.

Films: 64 x 48, four waves, the fog box and the fog box with three more rectangles in the room -- two across it on y, which makes
five planes on y, and a tilted one; shadow rays there are candidates of something all the time.  Over the homogeneous fog on the
kernels of tests/test_rect_vote_gpu.py's list -- k_render_wave_wg3 through both entry points, k_render_wave_wg, k_render_wave_wg2,
the generic k_render_wave_wg3 instantiation, the per-lane kernel --: 2000 (pixel, sample) pairs equal the oracle's replayed paths
summed in sample order, and the films and counters of all of them are the same bytes.  Over a 16^3 grid medium in the same two
rooms on the wavefront pipeline (k_wf_*, whose shadow set-up asks scene_intersect_any from regrouped jobs under divergent control
flow): the same 2000 pairs against the oracle, and the film against the per-lane kernel's, byte for byte.  With a guiding field in
the same two rooms on the guided k_render_wave_wg2 instantiation: film and counters equal the oracle's."""
import numpy as np
import pytest

import oracle_lib
import scenes
from test_rect_frame_gpu import _queries, _same_bits, sixteen_rectangles
from test_rect_vote_gpu import ENVS, N_SAMPLES, _Env, u32, wavefront_queries

pytestmark = pytest.mark.gpu

WALLS = [(1, -1.0), (1, 1.0), (2, 1.0), (2, -1.0), (0, -1.0), (0, 1.0), (1, 0.999)]   # (axis, plane) of the fog box's records, in index order


def _empty_scene(P):
    s = oracle_lib.fog_box_scene(8, 8)
    s.n_quads = 0
    s.medium.type = P.MEDIUM_NONE
    return s


def one_rectangle(P):
    s = _empty_scene(P)
    P.add_quad(s, (-1.0, 0.25, -1.0), (2.0, 0, 0), (0, 0, 2.0), le=(3, 3, 3))
    return s


def tilted_rectangles(P):
    s = _empty_scene(P)
    for i in range(2):
        e1 = np.array([1.5, 0.2, -0.5 if i else 0.6])
        e2 = np.array([-0.1, 1.7, 0.3])
        e2 = e2 - e1 * (e1 @ e2) / (e1 @ e1)
        P.add_quad(s, (-0.8, -0.9, 0.4 if i else -0.3), tuple(float(np.float32(v)) for v in e1), tuple(float(np.float32(v)) for v in e2),
                   le=(3, 3, 3) if i == 0 else (0, 0, 0), reverse=i)
    return s


def add_occluders(P, s):
    P.add_quad(s, (-0.6, 0.2, -0.1), (0.7, 0, 0), (0, 0, 0.8))            # two shelves across the room: planes four and five on y
    P.add_quad(s, (0.1, -0.35, -0.5), (0, 0, 0.9), (0.6, 0, 0))
    e1 = np.array([0.9, 0.1, 0.3])
    e2 = np.array([-0.1, 0.8, 0.05])
    e2 = e2 - e1 * (e1 @ e2) / (e1 @ e1)
    P.add_quad(s, (-0.5, -0.9, 0.2), tuple(float(np.float32(v)) for v in e1), tuple(float(np.float32(v)) for v in e2))   # tilted
    return s


def occluder_box(P, W, H):
    return add_occluders(P, P.fog_box_scene(W, H))


def grid_box(P, W, H, occluders):
    """the fog box's geometry around a 16^3 grid medium: the wavefront pipeline's scene"""
    s = scenes.grid_scene(scenes.cloud_density(16), (16, 16, 16), (0.05, 0.08, 0.1), (3.0, 2.6, 2.2), g=0.5,
                          bmin=(-0.8, -0.8, -0.5), bmax=(0.8, 0.7, 0.9), W=W, H=H)
    return add_occluders(P, s) if occluders else s


def fog_box_wavefronts(P):
    rng = np.random.default_rng(31)
    q = _queries(P, 256)
    lane = np.arange(256) % 64
    wave = np.arange(256) // 64
    wall = rng.integers(0, 6, 256)
    wall[192:] = (lane[192:] % 6 + rng.integers(1, 6, 64)) % 6   # wavefront 3 aims at another wall than the one it starts from
    q["o"] = rng.uniform(-0.3, 0.3, (256, 3)).astype(np.float32)
    tgt = rng.uniform(-0.4, 0.4, (256, 3))
    for i in range(256):
        a, c = WALLS[wall[i]]
        tgt[i, a] = c
    q["d"] = (tgt - q["o"]).astype(np.float32) * np.float32(1.5)           # reaches the wall at t = 2 / 3
    q["mode"] = 2
    q["w"] = rng.uniform(-0.6, 0.6, (256, 3)).astype(np.float32)
    q["tMax2"] = np.float32(1e-4)   # (the light hangs 1e-3 below the ceiling: out of reach from there too)
    q["tMax2"][64 + 37] = np.inf
    mixed = wave == 2
    q["w"][mixed] = rng.uniform(-1.6, 1.6, (64, 3)).astype(np.float32)
    q["tMax2"][mixed] = np.where(rng.random(64) < 0.5, rng.uniform(0.05, 1.5, 64), np.inf).astype(np.float32)
    for i in np.nonzero(wave == 3)[0]:
        a, c = WALLS[lane[i] % 6]
        w = rng.uniform(-0.8, 0.8, 3)
        w[a] = 1.3 * c
        q["w"][i] = w
        q["tMax2"][i] = 2.0
    return q


def _candidates(res, tmax2, planes):
    """[ray, plane]: the pre-test of rect_hit_uv / plane_vote on the spawned rays, in float32"""
    out = np.zeros((len(res), len(planes)), dtype=bool)
    one = np.float32(1.000001)
    for j, (a, c) in enumerate(planes):
        num = np.float32(c) - res["o2"][:, a]
        den = res["d2"][:, a]
        with np.errstate(all="ignore"):
            thr = (tmax2 * np.abs(den)).astype(np.float32) * one
            out[:, j] = ((u32(num) ^ u32(den)) >> 31 == 0) & ~(np.abs(num) > thr)
    return out & (res["hit"] != 0)[:, None]


def test_fog_box_wavefronts_by_candidates_equal_the_oracle(gpu_pkg):
    P = gpu_pkg
    scene, prm = P.fog_box_scene(8, 8), P.app_f_params()
    q = fog_box_wavefronts(P)
    o = oracle_lib.OracleRenderer(scene, prm, 8, 8)
    want = o.ray_batch(q)
    o.close()
    g = P.Renderer(scene, prm, 8, 8)
    got = g.ray_batch(q)
    _same_bits(want, got, "fog box, 256 rays")
    for w in range(4):   # each wavefront on its own: nothing of a neighbouring wavefront reaches it
        _same_bits(want[64 * w:64 * w + 64], g.ray_batch(q[64 * w:64 * w + 64]), "fog box, wavefront %d" % w)
    g.close()
    assert (want["hit"] != 0).all()
    cand = _candidates(want, q["tMax2"], WALLS).reshape(4, 64, len(WALLS))
    print("candidate (lane, plane) pairs per wavefront %s, occluded %s" % (cand.sum(axis=(1, 2)).tolist(), want["any2"].reshape(4, 64).sum(axis=1).tolist()))
    assert not cand[0].any() and not want["any2"][:64].any()
    assert cand[1].any(axis=1).sum() == 1 and cand[1][37].any() and want["any2"][64 + 37] == 1
    assert 0 < cand[2].any(axis=1).sum() < 64 and 0 < want["any2"][128:192].sum() < 64
    assert cand[3].any(axis=1).all() and len({tuple(r) for r in cand[3]}) >= 6 and want["any2"][192:].all()


@pytest.mark.parametrize("which", ["sixteen rectangles", "one rectangle", "no axis-aligned rectangle"])
def test_ray_batches_by_wavefront_equal_the_oracle(gpu_pkg, which):
    P = gpu_pkg
    scene = {"sixteen rectangles": sixteen_rectangles, "one rectangle": one_rectangle, "no axis-aligned rectangle": tilted_rectangles}[which](P)
    q, kinds = wavefront_queries(P, 1.6, 41)
    prm = P.app_f_params()
    o = oracle_lib.OracleRenderer(scene, prm, 8, 8)
    want = o.ray_batch(q)
    o.close()
    g = P.Renderer(scene, prm, 8, 8)
    for start, n in [(0, 4096), (0, 64), (64, 64), (128, 65), (135, 1), (192, 63)]:
        _same_bits(want[start:start + n], g.ray_batch(q[start:start + n]), "%s, rays [%d, %d)" % (which, start, start + n))
    g.close()
    print("%s: hits %d, spawned hits %d, occluded %d" % (which, int(want["hit"].sum()), int(want["hit2"].sum()), int(want["any2"].sum())))
    assert want["hit"].sum() > 100
    if which != "one rectangle":   # (nothing can lie between one rectangle and a ray that leaves it)
        assert 0 < want["any2"].sum() < want["hit"].sum()


def _paths(P, scene_of, W, H):
    """-> pixels, and the oracle's N_SAMPLES replayed paths per pixel summed in sample order (RGBFilm::AddSample)"""
    rng = np.random.default_rng(5)
    pix = np.stack([rng.integers(0, W, 2000 // N_SAMPLES), rng.integers(0, H, 2000 // N_SAMPLES)], axis=1).astype(np.int32)
    c = oracle_lib.OracleRenderer(scene_of(P, W, H), P.app_f_params(), W, H, seed=4)
    L, _ = c.trace_paths(np.repeat(pix, N_SAMPLES, axis=0), np.tile(np.arange(N_SAMPLES, dtype=np.int32), len(pix)))
    c.close()
    Ls = L.astype(np.float32).reshape(len(pix), N_SAMPLES, 3)
    s = Ls[:, 0]
    for k in range(1, N_SAMPLES):
        s = s + Ls[:, k]
    return pix, s


@pytest.mark.parametrize("which", ["fog box", "occluders"])
def test_films_are_the_oracles_paths_on_every_kernel(gpu_pkg, which):
    P = gpu_pkg
    W, H = 64, 48
    scene_of = (lambda M, w, h: M.fog_box_scene(w, h)) if which == "fog box" else occluder_box
    pix, sums = _paths(P, scene_of, W, H)
    ref = None
    names = set()
    for label, env, prefix in ENVS:
        with _Env(env):
            r = P.Renderer(scene_of(P, W, H), P.app_f_params(), W, H, seed=4)
            name = r.kernel_name()
            for w in range(N_SAMPLES):
                r.render_wave(w, w + 1)
            film, cnt = r.film(), r.counters()
            r.close()
        assert name.startswith(prefix), (label, name)
        names.add(name)
        if ref is None:
            ref = (film, cnt)
            bad = (u32(film[pix[:, 1], pix[:, 0], :3]) != u32(sums)).any(axis=1)
            assert not bad.any(), "%s, %s: film != oracle paths in %d of %d pixels" % (which, name, int(bad.sum()), len(pix))
            assert cnt["paths"] == W * H * N_SAMPLES and cnt["surface_hits"] > 0 and cnt["shadow_rays"] > 0
        else:
            assert np.array_equal(u32(film), u32(ref[0])), (which, label, name)
            assert cnt == ref[1], (which, label, cnt, ref[1])
    assert len(names) >= 5, sorted(names)


@pytest.mark.parametrize("which", ["fog box", "occluders"])
def test_wavefront_pipeline_films_are_the_oracles_paths(gpu_pkg, which):
    P = gpu_pkg
    W, H = 64, 48
    scene_of = lambda M, w, h: grid_box(M, w, h, which == "occluders")   # noqa: E731
    pix, sums = _paths(P, scene_of, W, H)
    films = {}
    for label, env in (("default", {}), ("per lane", {"VSPG_KERNEL": "lane"})):
        with _Env(env):
            r = P.Renderer(scene_of(P, W, H), P.app_f_params(), W, H, seed=4)
            name = r.kernel_name()
            for w in range(N_SAMPLES):
                r.render_wave(w, w + 1)
            films[label] = (name, r.film(), r.counters())
            r.close()
    name, film, cnt = films["default"]
    print("%s: %s, %s" % (which, name, cnt))
    assert name.startswith("k_wf_"), name
    assert films["per lane"][0].startswith("k_render_wave<"), films["per lane"][0]
    assert cnt["shadow_rays"] > 0 and cnt["surface_hits"] > 0
    bad = (u32(film[pix[:, 1], pix[:, 0], :3]) != u32(sums)).any(axis=1)
    assert not bad.any(), "%s, %s: film != oracle paths in %d of %d pixels" % (which, name, int(bad.sum()), len(pix))
    assert np.array_equal(u32(film), u32(films["per lane"][1])), (which, name)


@pytest.mark.parametrize("which", ["fog box", "occluders"])
def test_guided_workgroup_kernel_equals_the_oracles_film(gpu_pkg, which):
    P = gpu_pkg
    W, H = 24, 16
    scene = occluder_box(P, W, H) if which == "occluders" else P.fog_box_scene(W, H)
    prm, field = P.default_params(), scenes.light_field(P, n=4)
    g = P.Renderer(scene, prm, W, H, seed=4)
    c = oracle_lib.OracleRenderer(scene, prm, W, H, seed=4)
    g.set_guiding_field(field, field)
    c.set_guiding_field(field, field)
    name = g.kernel_name()
    assert name.startswith("k_render_wave_wg2<") and "guided" in name, name
    for w in range(2):
        g.render_wave(w, w + 1)
        c.render_wave(w, w + 1)
    fg, fc, cg, cc = g.film(), c.film(), g.counters(), c.counters()
    g.close()
    c.close()
    assert cg["surface_hits"] > 0 and cg["shadow_rays"] > 0
    assert np.array_equal(u32(fg), u32(fc)), "%s, %s: film bits differ in %d values" % (which, name, int((u32(fg) != u32(fc)).sum()))
    assert cg == cc, (cg, cc)
