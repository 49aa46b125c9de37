"""The triangle traversal on the device (csrc/vspg_device.h: bvh_closest, bvh_any through scene_intersect / scene_intersect_any in
k_ray_batch) against the oracle's brute-force walk, on the rays that touch the traversal's edge cases: every field of VspgRayResult
bit for bit, as tests/test_reference_scenarios.py compares its ray batches.

The families are those of tests/test_bvh_traverse_bits.py (which runs the same text on the CPU, where the counts of what went wrong
before are): flat grids in a plane of each axis with perpendicular rays through every vertex, edge midpoint and cell centre and
+0 / -0 in all sign combinations, tMax at the hit distance and one float above, rays in the plane; tilted triangles; two layers; nine
and fourteen coincident copies with shuffled ids and two triangulations of one plane; soups of 1, 2, 3, 7, 8, 9, 1000 triangles in one
box, stacked sheets, the cascade at x = 2^-k; a random soup of 2000 with zeros and denormals in d.  No NaN or infinite ray component.

A third of each batch has mode 1 (SpawnRay(w)) and a third mode 2 (SpawnRayTo(w)), with w such that the spawned ray is axis-parallel
again -- on along the first ray, back along it, or along the surface -- from an origin that OffsetRayOrigin moved along the normal
only: a vertex or an edge midpoint again.  hit2 / t2 / any2 are the second closest hit and bvh_any's answer from there.  The device
gets every batch in pieces whose sizes are no multiple of 64 (a last wavefront with idle lanes, a wavefront of one lane).

Beside equality: no perpendicular ray through a flat grid escapes it, and on the coincident copies prim is the smallest id of the
copies.  The oracle side is brute force: at most about 4 * 10^7 triangle tests per scene."""
import itertools

import numpy as np
import pytest

import oracle_lib
from conftest import load_package
from test_reference_scenarios import empty_scene, queries, renderers

f32 = np.float32
ZERO = (f32(0.0), f32(-0.0))
PLANE_OF = (0.5, -0.25, 0.0)   # the flat grids: x = 0.5, y = -0.25, z = 0
SIZES = (1, 63, 65, 130, 997, 4001)   # the pieces the device gets: none a multiple of 64


def in_plane(axis, u, v, c):
    """(u, v) in a plane, c along `axis`: each axis takes the flat role."""
    u, v, c = np.broadcast_arrays(np.asarray(u, f32), np.asarray(v, f32), np.asarray(c, f32))
    return np.stack({2: (u, v, c), 0: (c, u, v), 1: (v, c, u)}[axis], axis=-1).astype(f32)


def grid(axis, n, c, other=False, height=None):
    """n x n cells over [0, 1]^2 of the plane `axis` = c, two triangles per cell (`other`: the other diagonal)."""
    def vtx(i, j):
        return in_plane(axis, f32(i) / f32(n), f32(j) / f32(n), f32(c) + (f32(height(i, j)) if height else f32(0)))
    tris = []
    for j in range(n):
        for i in range(n):
            if not other:
                tris += [[vtx(i, j), vtx(i + 1, j), vtx(i + 1, j + 1)], [vtx(i, j), vtx(i + 1, j + 1), vtx(i, j + 1)]]
            else:
                tris += [[vtx(i, j), vtx(i + 1, j), vtx(i, j + 1)], [vtx(i + 1, j), vtx(i + 1, j + 1), vtx(i, j + 1)]]
    return np.array(tris, dtype=f32).reshape(-1, 9)


def perpendicular(P, axis, n, c, dist, signs=(0, 1, 2, 3), tMax=np.inf):
    """Rays along `axis` through the (2n + 1)^2 vertices, edge midpoints and cell centres, from c + dist down and from c - dist up;
    the zero components of d take the signs of `signs` (bit 0, bit 1: negative).  Every third ray spawns on along d (mode 1), every
    third to the point one unit further along its own line (mode 2)."""
    k = np.arange(2 * n + 1, dtype=f32) / f32(2 * n)
    u, v = [a.ravel() for a in np.meshgrid(k, k)]
    parts = []
    for s in signs:
        for side in (0, 1):
            q = queries(P, len(u))
            q["o"] = in_plane(axis, u, v, f32(c) - f32(dist) if side else f32(c) + f32(dist))
            q["d"] = in_plane(axis, ZERO[s & 1], ZERO[s >> 1], f32(1) if side else f32(-1))
            q["tMax"] = tMax
            m = np.arange(len(u)) % 3
            q["mode"] = m
            q["w"][m == 1] = q["d"][m == 1]
            q["w"][m == 2] = in_plane(axis, u, v, f32(c) + f32(2) if side else f32(c) - f32(2))[m == 2]
            parts.append(q)
    return np.concatenate(parts)


def random_rays(P, rng, n, extent, tris=None):
    """Random rays; with tris, every other one aimed at a random point of a random triangle.  Modes 0, 1, 2 in turn with random w."""
    q = queries(P, n)
    q["o"] = rng.uniform(-extent, extent, (n, 3)).astype(f32)
    q["d"] = rng.uniform(-1, 1, (n, 3)).astype(f32)
    if tris is not None:
        t = tris[rng.integers(0, len(tris), n)].reshape(n, 3, 3)
        b = rng.uniform(0, 1, (n, 2))
        flip = b.sum(axis=1) > 1
        b[flip] = 1 - b[flip]
        p = (b[:, :1] * t[:, 0] + b[:, 1:] * t[:, 1] + (1 - b.sum(axis=1, keepdims=True)) * t[:, 2]).astype(f32)
        aimed = np.arange(n) % 2 == 1
        q["d"][aimed] = (p - q["o"])[aimed]
    q["tMax"][::7] = rng.uniform(0, 2 * extent, len(q["tMax"][::7])).astype(f32)
    q["mode"] = np.arange(n) % 3
    q["w"] = rng.uniform(-1, 1, (n, 3)).astype(f32)
    q["tMax2"][::5] = 1.0
    return q


def at_the_hit_distance(q, res):
    """The rays that hit, with tMax exactly the hit distance (a miss: t < tMax is strict) and with the next float above (a hit)."""
    hit = res["hit"] != 0
    a, b = q[hit].copy(), q[hit].copy()
    a["tMax"] = res["t"][hit]
    b["tMax"] = np.nextafter(res["t"][hit], f32(np.inf))
    return a, b


class Scene:
    """One soup: the oracle's answers computed once per batch, the device's compared with them in pieces."""

    def __init__(self, P, tris, gpu):
        self.P, self.tris = P, np.ascontiguousarray(tris, dtype=f32).reshape(-1, 9)
        self.scene = empty_scene(P)
        P.set_triangles(self.scene, self.tris)
        self.o, self.g = renderers(P, self.scene, gpu)
        self.tests = 0

    def batch(self, q, what):
        want = self.o.ray_batch(q)
        self.tests += len(self.tris) * (len(q) + 2 * int((q["mode"] != 0).sum()))
        if self.g is not None:
            start = 0
            for size in itertools.cycle(SIZES):
                if start >= len(q):
                    break
                n = min(size, len(q) - start)
                if n % 64 == 0:
                    n -= 1
                got = self.g.ray_batch(q[start:start + n])
                for name in want.dtype.names:
                    same = (want[name][start:start + n].view(np.uint32) == got[name].view(np.uint32)).reshape(n, -1).all(axis=1)
                    assert same.all(), "%s: device != oracle in %s for %d of the rays [%d, %d), first %s" % (
                        what, name, int((~same).sum()), start, start + n, q[start + int(np.argmin(same))])
                start += n
        return want

    def close(self):
        assert self.tests <= 5e7, self.tests   # the oracle's side stays cheap
        self.o.close()
        if self.g is not None:
            self.g.close()


# ---- the families -----------------------------------------------------------------------------------------------------------------
def flat_grid(P, gpu, axis):
    c = PLANE_OF[axis]
    S = Scene(P, grid(axis, 8, c), gpu)
    q = np.concatenate([perpendicular(P, axis, 8, c, 1.0), perpendicular(P, axis, 8, c, 0.7)])
    res = S.batch(q, "flat grid %d, perpendicular" % axis)
    assert len(q) == 2 * 2312 and res["hit"].all(), "%d perpendicular rays escaped the grid" % int((res["hit"] == 0).sum())
    assert (res["prim"] >= 1000000).all() and (res["prim"] < 1000128).all()
    assert not res["hit2"].any() and not res["any2"].any()   # on along the ray or to a point behind the grid: nothing else is there
    miss, hit = at_the_hit_distance(q, res)
    assert not S.batch(miss, "flat grid %d, tMax at the hit distance" % axis)["hit"].any()
    assert S.batch(hit, "flat grid %d, tMax one float above the hit distance" % axis)["hit"].all()
    # back along the ray and along the surface (w an in-plane axis, of both signs): the spawned ray runs beside the plane
    along = perpendicular(P, axis, 8, c, 1.0, signs=(0, 3))
    m = np.arange(len(along)) % 4
    along["mode"] = 1
    surface = np.array([[0, 0, 0], [1, 0, 0.0], [0, -1, -0.0], [-1, 1, -0.0]], dtype=f32)[m]   # (u, v, c): c = +-0 leaves d2 in the plane
    along["w"] = np.where((m == 0)[:, None], -along["d"], in_plane(axis, surface[:, 0], surface[:, 1], surface[:, 2]))
    res = S.batch(along, "flat grid %d, spawned back and along the surface" % axis)
    assert res["hit"].all() and not res["hit2"].any() and not res["any2"].any()
    # rays in the grid's plane: NaN on both faces of every flat box, and brute force says miss
    dirs = np.array([[1, 0], [-1, 0], [0, 1], [0, -1], [1, 1], [-1, 1], [0.25, -1], [-1, -0.375]], dtype=f32)
    k = np.arange(-1, 18, dtype=f32) / f32(16)
    u, v = [a.ravel() for a in np.meshgrid(k[::3], k)]
    parts = []
    for d in dirs:
        for z in ZERO:
            p = queries(P, len(u))
            p["o"] = in_plane(axis, u, v, c)
            p["d"] = in_plane(axis, d[0], d[1], z)
            parts.append(p)
    assert not S.batch(np.concatenate(parts), "flat grid %d, rays in its plane" % axis)["hit"].any()
    S.close()


def tilted(P, gpu):
    S = Scene(P, grid(2, 8, 0.0, height=lambda i, j: ((3 * i + 5 * j) % 4) / 8.0), gpu)   # steps of 1/8: a box face holds a vertex or an edge only
    parts = [perpendicular(P, 2, 8, 0.0, 1.0)]
    k, h = np.arange(17, dtype=f32) / f32(16), np.arange(-1, 9, dtype=f32) / f32(16)
    u, z = [a.ravel() for a in np.meshgrid(k, h)]
    for axis in (0, 1):   # along x and along y through the lattice of sixteenths, heights included: along the faces of the boxes
        for s in range(4):
            for side in (0, 1):
                q = queries(P, len(u))
                far = np.full(len(u), -1.0 if side else 2.0, dtype=f32)
                along = np.full(len(u), 1.0 if side else -1.0, dtype=f32)
                zero0, zero1 = np.full(len(u), ZERO[s & 1]), np.full(len(u), ZERO[s >> 1])
                q["o"] = np.stack([far, u, z] if axis == 0 else [u, far, z], axis=-1)
                q["d"] = np.stack([along, zero0, zero1] if axis == 0 else [zero0, along, zero1], axis=-1)
                m = np.arange(len(u)) % 3
                q["mode"] = m
                q["w"][m == 1] = q["d"][m == 1]                      # on along the ray: through the next step of the heightfield
                q["w"][m == 2] = (q["o"] + f32(4) * q["d"])[m == 2]    # to the point behind the heightfield on the ray's own line
                parts.append(q)
    q = np.concatenate(parts)
    res = S.batch(q, "tilted triangles")
    assert res["hit"][:2312].all() and res["hit"].mean() > 0.5 and res["hit2"].any() and res["any2"].any()
    miss, hit = at_the_hit_distance(q, res)
    assert not S.batch(miss, "tilted triangles, tMax at the hit distance")["hit"].any()
    assert S.batch(hit, "tilted triangles, tMax one float above the hit distance")["hit"].all()
    S.close()


def two_layers(P, gpu):
    S = Scene(P, np.concatenate([grid(2, 8, 0.0), grid(2, 8, -0.5)]), gpu)
    rng = np.random.default_rng(20)
    q = np.concatenate([perpendicular(P, 2, 8, 0.0, 1.0), perpendicular(P, 2, 8, -0.25, 0.125, signs=(0, 3)),
                        perpendicular(P, 2, 8, 0.0, 1.0, signs=(0, 3), tMax=1.25)])
    ob = queries(P, 3001)   # oblique rays through both layers
    ob["o"] = np.stack([rng.uniform(-0.5, 1.5, 3001), rng.uniform(-0.5, 1.5, 3001), np.where(np.arange(3001) % 2, 1.0, -1.5)], axis=-1).astype(f32)
    ob["d"] = (np.stack([rng.uniform(0, 1, 3001), rng.uniform(0, 1, 3001), np.full(3001, -0.25)], axis=-1).astype(f32) - ob["o"]).astype(f32)
    ob["mode"] = np.arange(3001) % 3
    ob["w"] = ob["d"]
    ob["w"][ob["mode"] == 2] = (ob["o"] + f32(2) * ob["d"])[ob["mode"] == 2]
    q = np.concatenate([q, ob])
    res = S.batch(q, "two layers")
    first = res[:2312]   # from c + 1 and c - 1 through both layers
    assert first["hit"].all() and (first["hit2"] == (q["mode"][:2312] != 0)).all() and (first["any2"] == first["hit2"]).all()
    miss, hit = at_the_hit_distance(q, res)
    assert not S.batch(miss, "two layers, tMax at the hit distance")["hit"].any()
    assert S.batch(hit, "two layers, tMax one float above the hit distance")["hit"].all()
    S.close()


def ties(P, gpu):
    rng = np.random.default_rng(9)
    for copies in (9, 14):   # identical centroids force the median split: leaves of 4 and 5, two full leaves of 7
        base = grid(2, 2, 0.0)
        slot = rng.permutation(np.arange(8 * copies) % 8)   # which of the 8 triangles the soup's triangle i is a copy of
        tris = base[slot]
        smallest = np.array([int(np.argmax(slot == k)) for k in range(8)])
        S = Scene(P, tris, gpu)
        q = np.concatenate([perpendicular(P, 2, 2, 0.0, 1.0), perpendicular(P, 2, 4, 0.0, 0.7, signs=(0, 3)), random_rays(P, rng, 3001, 2.0, tris)])
        res = S.batch(q, "ties, %d coincident copies" % copies)
        hit = res["hit"] != 0
        assert hit[:200 + 324].all() and hit.mean() > 0.5
        prim = res["prim"][hit] - 1000000
        assert (prim == smallest[slot[prim]]).all(), "%d winners are not the smallest id of their copies" % int((prim != smallest[slot[prim]]).sum())
        S.close()
    tris = np.concatenate([grid(2, 8, 0.0), grid(2, 8, 0.0, other=True), grid(2, 5, 0.0)])
    S = Scene(P, tris, gpu)
    q = np.concatenate([perpendicular(P, 2, 8, 0.0, 1.0), perpendicular(P, 2, 5, 0.0, 0.7, signs=(0, 3)), random_rays(P, rng, 3001, 2.0, tris)])
    res = S.batch(q, "ties, two triangulations of one plane")
    assert res["hit"][:2312 + 484].all()
    S.close()


def tree_shapes(P, gpu):
    rng = np.random.default_rng(48)
    for n in (1, 2, 3, 7, 8, 9):   # a root with one child, absent children, full leaves
        c = rng.uniform(-0.5, 0.5, (n, 1, 3))
        tris = (c + rng.uniform(-0.5, 0.5, (n, 3, 3))).astype(f32).reshape(n, 9)
        S = Scene(P, tris, gpu)
        res = S.batch(random_rays(P, rng, 3001, 1.5, tris), "soup of %d" % n)
        assert 0.2 < res["hit"].mean() < 1
        S.close()
    # per coordinate one vertex at 0, one at 1 and one between: every triangle's box is [0, 1]^3
    v = rng.uniform(0, 1, (1000, 3, 3))
    lo = rng.integers(0, 3, (1000, 3))
    hi = (lo + 1 + rng.integers(0, 2, (1000, 3))) % 3
    for k in range(3):
        v[:, k, :] = np.where(lo == k, 0.0, np.where(hi == k, 1.0, v[:, k, :]))
    tris = v.astype(f32).reshape(1000, 9)
    S = Scene(P, tris, gpu)
    q = random_rays(P, rng, 4001, 1.5, tris)
    face = queries(P, 601)   # along the box's faces and through its corners, with zeros of both signs
    face["o"] = (rng.integers(0, 3, (601, 3)) * 0.5).astype(f32)
    face["d"] = np.where(rng.integers(0, 2, (601, 3)) == 1, ZERO[1], ZERO[0])
    a = np.arange(601) % 3
    face["o"][np.arange(601), a] = np.where(np.arange(601) % 2, 2.0, -1.0)
    face["d"][np.arange(601), a] = np.where(np.arange(601) % 2, -1.0, 1.0)
    face["mode"] = 1
    face["w"] = face["d"]
    res = S.batch(np.concatenate([q, face]), "1000 triangles in one box")
    assert res["hit"].mean() > 0.25 and res["hit2"].any()
    S.close()
    for n in (7, 8, 60, 2000):
        z = (np.arange(n, dtype=f32) / f32(64))[:, None]
        tris = np.concatenate([np.zeros((n, 2)), z, np.ones((n, 1)), np.zeros((n, 1)), z, np.zeros((n, 1)), np.ones((n, 1)), z], axis=1).astype(f32)
        S = Scene(P, tris, gpu)
        q = random_rays(P, rng, 2001, 1.5, tris)
        q["o"][::2, 2] = rng.uniform(0, n / 64.0, len(q["o"][::2])).astype(f32)   # from between the sheets
        res = S.batch(np.concatenate([perpendicular(P, 2, 2, 0.0, 40.0), q]), "%d stacked sheets" % n)
        assert res["hit"].mean() > 0.25 and res["hit2"].any() == (n > 1)
        S.close()
    for n in (48, 126):   # the unit triangle in the plane z = 0 with its corner at x = 2^-t: one plane, ever smaller steps
        x = np.ldexp(f32(1), -np.arange(1, n + 1)).astype(f32)[:, None]
        zero, one = np.zeros((n, 1), dtype=f32), np.ones((n, 1), dtype=f32)
        tris = np.concatenate([x, zero, zero, x + one, zero, zero, x, one, zero], axis=1).astype(f32)
        S = Scene(P, tris, gpu)
        xs = np.concatenate([[f32(0)], np.ldexp(f32(1), -np.arange(1, n + 2)).astype(f32)])
        u, v = [a.ravel() for a in np.meshgrid(xs, np.arange(5, dtype=f32) / f32(4))]
        parts = []
        for s in range(4):
            for side in (0, 1):
                q = queries(P, len(u))
                q["o"] = np.stack([u, v, np.full(len(u), -1.0 if side else 1.0, dtype=f32)], axis=-1)
                q["d"] = np.stack([np.full(len(u), ZERO[s & 1]), np.full(len(u), ZERO[s >> 1]), np.full(len(u), 1.0 if side else -1.0, dtype=f32)], axis=-1)
                parts.append(q)
        res = S.batch(np.concatenate(parts + [random_rays(P, rng, 3001, 2.0, tris)]), "cascade of %d" % n)
        assert res["hit"].mean() > 0.25
        S.close()


def random_soup(P, gpu):
    rng = np.random.default_rng(2000)
    c = rng.uniform(-1, 1, (2000, 1, 3))
    tris = (c + rng.uniform(-0.08, 0.08, (2000, 3, 3))).astype(f32).reshape(2000, 9)
    S = Scene(P, tris, gpu)
    q = random_rays(P, rng, 4001, 1.5, tris)
    inside = random_rays(P, rng, 1001, 1.0)
    inside["o"] = tris[rng.integers(0, 2000, 1001), :3]   # origins inside boxes: on a triangle's vertex
    odd = random_rays(P, rng, 3001, 1.2, tris)
    specials = np.array([0.0, -0.0, 1e-45, -1e-45, 5.877472e-39, -1.1754942e-38], dtype=f32)   # zeros and denormals
    k = rng.integers(0, 3, 3001)
    odd["d"][np.arange(3001), k] = specials[rng.integers(0, 6, 3001)]
    two = np.arange(3001) % 2 == 0
    odd["d"][np.arange(3001)[two], (k[two] + 1) % 3] = specials[rng.integers(0, 6, int(two.sum()))]
    on_face = np.arange(3001) % 4 == 0   # the origin on a triangle's box face: a vertex's coordinate
    odd["o"][np.arange(3001)[on_face], k[on_face]] = tris[rng.integers(0, 2000, int(on_face.sum())), k[on_face]]
    res = S.batch(np.concatenate([q, inside, odd]), "random soup")
    assert 0.1 < res["hit"].mean() < 1 and res["hit2"].any() and res["any2"].any()
    S.close()


FAMILIES = {"flat grid x": lambda P, gpu: flat_grid(P, gpu, 0), "flat grid y": lambda P, gpu: flat_grid(P, gpu, 1),
            "flat grid z": lambda P, gpu: flat_grid(P, gpu, 2), "tilted triangles": tilted, "two layers": two_layers, "ties": ties,
            "tree shapes": tree_shapes, "random soup": random_soup}


@pytest.mark.gpu
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_ray_batches_equal_the_oracle_bit_for_bit(gpu_pkg, family):
    FAMILIES[family](gpu_pkg, True)


def test_oracle_alone_holds_the_independent_assertions():
    """The same batches without a device (no ray escapes a flat grid, the smallest id wins a tie, tMax at the hit distance misses)."""
    P = load_package()
    flat_grid(P, False, 1)
    two_layers(P, False)
    ties(P, False)
