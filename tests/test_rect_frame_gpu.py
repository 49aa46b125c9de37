"""The rectangle loops walk the ray through the records' axis frames (csrc/vspg_device.h: rect_frame, rect_hit_uv, rects_closest,
rects_any); every decision and every bit they report stays the oracle's.

Renderer.ray_batch against OracleRenderer.ray_batch, all fields bit for bit (hit / prim / t / p / n: the closest-hit loop and the
(u, v) it hands to the hit point; hit2 / t2 / any2: both loops again on the spawned ray), on three inputs:
  - the fog box, 10^5 random rays;
  - 16 rectangles -- every axis x e1 / e2 order x reverse_orientation, two more with negative extents, two tilted ones in the
    middle -- in an order that holds every transition between axis frames, 10^5 random rays;
  - rays from inside the fog box aimed exactly at its edges and corners: their distances to two or three walls are bit-equal (checked
    on the CPU, wall by wall, without a GPU), and the reported rectangle must be the lowest index among them.
Then a 64 x 64 fog-box film of four one-sample waves under VSPG_WG_SCHED=1, 2 and the default kernel: the three films are the same
bits, and 2000 (pixel, sample) pairs of them are the oracle's paths, summed in sample order."""
import os

import numpy as np
import pytest

import oracle_lib
from conftest import load_package

N_RANDOM = 100000


def _queries(P, n):
    q = np.zeros(n, dtype=P.RAY_QUERY_DTYPE)
    q["tMax"] = np.inf
    q["tMax2"] = np.inf
    return q


def _random_queries(P, n, seed, span):
    """Origins in [-span, span]^3, directions of every sign and length, a tenth with a finite tMax; the spawned ray goes along a
    random direction (mode 1) or towards a random point (mode 2), a third of them with a tMax2 inside the scene."""
    rng = np.random.default_rng(seed)
    q = _queries(P, n)
    q["o"] = rng.uniform(-span, span, (n, 3)).astype(np.float32)
    q["d"] = (rng.normal(size=(n, 3)) * rng.uniform(0.3, 2.0, (n, 1))).astype(np.float32)
    q["tMax"] = np.where(rng.random(n) < 0.1, rng.uniform(0.1, 3.0, n), np.inf).astype(np.float32)
    q["mode"] = rng.integers(1, 3, n)
    q["w"] = np.where((q["mode"] == 1)[:, None], rng.normal(size=(n, 3)), rng.uniform(-span, span, (n, 3))).astype(np.float32)
    q["tMax2"] = np.where(rng.random(n) < 0.33, rng.uniform(0.05, 1.5, n), np.inf).astype(np.float32)
    return q


def _same_bits(a, b, what):
    for name in a.dtype.names:
        x, y = a[name].view(np.uint32), b[name].view(np.uint32)
        bad = np.nonzero((x != y).reshape(len(a), -1).any(axis=1))[0]
        assert bad.size == 0, "%s: device != oracle in %s for %d rays, first %s" % (what, name, bad.size, bad[:4])


# ---- the 16-rectangle scene ---------------------------------------------------------------------------------------------------
AXES = (0, 0, 1, 1, 2, 2, 0, 2, -1, -1, 1, 0, 2, 1, 2, 0)   # -1: tilted.  Transitions x-x x-y y-y y-z z-z z-x x-z z-(x) (x)-y y-x x-z z-y y-z z-x


def sixteen_rectangles(P, W=8, H=8):
    s = oracle_lib.fog_box_scene(W, H)
    s.n_quads = 0
    s.medium.type = P.MEDIUM_NONE
    rng = np.random.default_rng(16)
    seen = [0, 0, 0]
    combos = set()
    for i, a in enumerate(AXES):
        if a < 0:
            e1 = np.array([1.5, 0.2, 0.6 if i == 8 else -0.5])
            e2 = np.array([-0.1, 1.7, 0.3])
            e2 = e2 - e1 * (e1 @ e2) / (e1 @ e1)
            p00 = (-0.8, -0.9, -0.3 if i == 8 else 0.4)
            P.add_quad(s, p00, tuple(float(np.float32(v)) for v in e1), tuple(float(np.float32(v)) for v in e2), reverse=i & 1)
            continue
        k = seen[a]
        seen[a] += 1
        order, reverse, negative = k & 1, (k >> 1) & 1, k >= 4
        combos.add((a, order, reverse))
        a1, a2 = ((a + 2) % 3, (a + 1) % 3) if order else ((a + 1) % 3, (a + 2) % 3)
        p00, e1, e2 = [0.0] * 3, [0.0] * 3, [0.0] * 3
        p00[a] = -0.9 + 0.12 * i
        p00[a1], p00[a2] = rng.uniform(-1.2, -0.4, 2)
        e1[a1], e2[a2] = rng.uniform(1.0, 2.0, 2)
        if negative:
            p00[a1] += e1[a1]
            e1[a1] = -e1[a1]
        P.add_quad(s, p00, e1, e2, le=(3, 3, 3) if i == 0 else (0, 0, 0), reverse=reverse)
    assert s.n_quads == 16 and len(combos) == 12
    return s


# ---- rays at the fog box's edges and corners ----------------------------------------------------------------------------------
def edge_and_corner_queries(P):
    """d = target - o with dyadic coordinates: exact, so the quotient (wall - o) / d is exactly 1 for every wall through the target."""
    targets = [(x, y, z) for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)]                              # corners
    for c in (-0.5, 0.0, 0.625):
        targets += [(x, y, c) for x in (-1, 1) for y in (-1, 1)] + [(x, c, z) for x in (-1, 1) for z in (-1, 1)] + \
                   [(c, y, z) for y in (-1, 1) for z in (-1, 1)]                                        # points on the twelve edges
    origins = [(0, 0, 0), (0.25, -0.5, 0.125), (-0.375, 0.5, -0.75), (0.5, 0.5, 0.5)]
    rays = [(o, tuple(np.subtract(t, o)), s) for o in origins for t in targets for s in (1.0, 0.5, 4.0)]
    rays += [((0, 0, 0), d, 1.0) for d in ((1, 1, 0), (1, 1, 1), (-1, 1, 0), (0, -1, 1), (-1, -1, -1))]   # the issue's own examples
    q = _queries(P, len(rays))
    for i, (o, d, s) in enumerate(rays):
        q["o"][i] = o
        q["d"][i] = np.float32(s) * np.array(d, dtype=np.float32)   # a power of two: still exact
    q["mode"] = 1
    q["w"] = -q["d"]                                                  # the spawned ray goes back the way it came
    return q


def _wall_hits(P, q):
    """hit, t of every ray against every rectangle of the fog box ALONE (the oracle, one single-rectangle scene each)"""
    full = oracle_lib.fog_box_scene(8, 8)
    hit, t = [], []
    for k in range(full.n_quads):
        one = oracle_lib.fog_box_scene(8, 8)
        one.quads[0] = full.quads[k]
        one.n_quads = 1
        o = oracle_lib.OracleRenderer(one, oracle_lib.app_f_params(), 8, 8)
        r = o.ray_batch(q)
        o.close()
        hit.append(r["hit"] != 0)
        t.append(np.where(r["hit"] != 0, r["t"], np.inf).astype(np.float32))
    return np.array(hit), np.array(t)


def _check_ties(P, q, res):
    hit, t = _wall_hits(P, q)
    tmin = t.min(axis=0)
    tied = hit & (t.view(np.uint32) == tmin.view(np.uint32)[None, :])
    n_tied = tied.sum(axis=0)
    assert np.all(n_tied >= 2), "rays that do not tie: %s" % np.nonzero(n_tied < 2)[0][:8]
    assert np.any(n_tied >= 3)                                          # the corners
    lowest = tied.argmax(axis=0)                                        # the first rectangle in index order among the tied ones
    assert np.all(res["hit"] == 1)
    assert np.array_equal(res["t"].view(np.uint32), tmin.view(np.uint32))
    assert np.array_equal(res["prim"], lowest), np.nonzero(res["prim"] != lowest)[0][:8]
    return n_tied


def test_edge_and_corner_rays_tie_on_the_oracle():
    """No GPU: the engineered rays really meet two or three walls at bit-equal distances, and the oracle names the lowest index."""
    P = load_package()
    q = edge_and_corner_queries(P)
    o = oracle_lib.OracleRenderer(oracle_lib.fog_box_scene(8, 8), oracle_lib.app_f_params(), 8, 8)
    res = o.ray_batch(q)
    o.close()
    n_tied = _check_ties(P, q, res)
    print("%d engineered rays, %d of them meet three walls at one distance" % (len(q), int((n_tied >= 3).sum())))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["fog box", "sixteen rectangles", "edges and corners"])
def test_ray_batch_equals_the_oracle_bit_for_bit(gpu_pkg, which):
    P = gpu_pkg
    if which == "sixteen rectangles":
        scene, q = sixteen_rectangles(P), _random_queries(P, N_RANDOM, 2, 1.6)
    elif which == "fog box":
        scene, q = P.fog_box_scene(8, 8), _random_queries(P, N_RANDOM, 1, 0.98)
    else:
        scene, q = P.fog_box_scene(8, 8), edge_and_corner_queries(P)
    prm = P.app_f_params()
    g = P.Renderer(scene, prm, 8, 8)
    o = oracle_lib.OracleRenderer(scene, prm, 8, 8)
    a, b = o.ray_batch(q), g.ray_batch(q)
    g.close()
    o.close()
    print("%s: %d rays, %d hit, %d spawned rays hit, %d occluded; rectangles that win: %s" % (
        which, len(q), int(a["hit"].sum()), int(a["hit2"].sum()), int(a["any2"].sum()), sorted(set(a["prim"][a["hit"] != 0].tolist()))))
    _same_bits(a, b, which)
    if which == "edges and corners":
        _check_ties(P, q, b)
    else:   # the inputs reach what they are meant for: every rectangle wins some ray, both loops see hits and misses on the spawned ray
        assert set(a["prim"][a["hit"] != 0].tolist()) == set(range(scene.n_quads))
        assert 0 < a["any2"].sum() < a["hit"].sum() and 0 < a["hit2"].sum()


@pytest.mark.gpu
def test_fog_box_film_is_the_oracles_paths_under_every_scheduler(gpu_pkg):
    P = gpu_pkg
    W = H = 64
    scene, prm = P.fog_box_scene(W, H), P.app_f_params()
    films = {}
    for sched in ("1", "2", None):
        if sched:
            os.environ["VSPG_WG_SCHED"] = sched
        try:
            r = P.Renderer(scene, prm, W, H, seed=4)
            name = r.kernel_name()
            for w in range(4):   # no post_process_wave in between: the image-space buffer keeps its initial state, as in trace_paths
                r.render_wave(w, w + 1)
            films[name] = r.film()
            r.close()
        finally:
            os.environ.pop("VSPG_WG_SCHED", None)
    assert len(films) == 3 and any(n.startswith("k_render_wave_wg3") for n in films), sorted(films)
    first = next(iter(films.values()))
    assert np.array_equal(first[..., 3], np.full((H, W), 4.0, dtype=np.float32))
    for name, f in films.items():
        assert np.array_equal(first.view(np.uint32), f.view(np.uint32)), name
    rng = np.random.default_rng(8)
    pix = np.repeat(np.stack([rng.integers(0, W, 500), rng.integers(0, H, 500)], axis=1).astype(np.int32), 4, axis=0)
    si = np.tile(np.arange(4, dtype=np.int32), 500)
    c = oracle_lib.OracleRenderer(scene, prm, W, H, seed=4)
    L, _ = c.trace_paths(pix, si)
    c.close()
    L = L.astype(np.float32).reshape(500, 4, 3)
    want = ((L[:, 0] + L[:, 1]) + L[:, 2]) + L[:, 3]                    # RGBFilm::AddSample, one sample per wave, in wave order
    got = first[pix[::4, 1], pix[::4, 0], :3]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "film != oracle paths"
