"""Hand-built guiding fields at the sizes and shapes a trainer could produce, the query sets the CPU and GPU tests share, and
an independent float64 model of the guiding-cache query (csrc/vspg_guiding.h's header comment).

Generators: deterministic from their seed, return `P.Field` with two extra attributes: `np_nodes` / `np_regions` (structured
NumPy copies of what was uploaded) and `cells` (per node: lower and upper corner of its cell).  EVERY float of a lobe slot
k >= n_lobes is NaN, so a read of an unset slot cannot go unnoticed.

Model: the kd descent with float32 comparisons (exact), everything else in float64 with `exp` in place of FastExp -- except
FastExp's flush (a result below 2^-126 is 0), which decides two branches.  Next to each value the model returns the error a
float32 / FastExp evaluation of the same formulas may have (see `model_query`)."""
import numpy as np

GK = 8
NODE_DTYPE = np.dtype([("split", "<f4"), ("packed", "<u4")])
REGION_DTYPE = np.dtype([("pivot", "<f4", 3), ("n_lobes", "<i4"), ("weight", "<f4", GK), ("kappa", "<f4", GK),
                         ("mu", "<f4", (3, GK)), ("distance", "<f4", GK), ("vsp", "<f4", GK)])
assert NODE_DTYPE.itemsize == 8 and REGION_DTYPE.itemsize == 240
LOBE_FLOATS = ("weight", "kappa", "distance", "vsp")
KD_LDS_NODES = 256     # nodes per field the workgroup kernels stage in LDS (kKdLdsNodes)
MAX_DESCENT = 64       # steps of field_lookup
COSINE_KAPPA = np.float32(2.18853)
BRANCHES = ("product", "fallback", "cancel", "untrained", "outside", "plain")   # "plain": isotropic phase function, no product lobe


def make_field(P, nodes, regions, cells=None):
    """P.Field over copies of two structured arrays (P.Field's own constructor wants one ctypes object per record)."""
    import ctypes as C
    nodes = np.ascontiguousarray(nodes, dtype=NODE_DTYPE)
    regions = np.ascontiguousarray(regions, dtype=REGION_DTYPE)
    assert C.sizeof(P.VspgKdNode) == NODE_DTYPE.itemsize and C.sizeof(P.VspgFieldRegion) == REGION_DTYPE.itemsize
    f = P.Field.__new__(P.Field)
    f.nodes = (P.VspgKdNode * len(nodes)).from_buffer_copy(nodes.tobytes())
    f.regions = (P.VspgFieldRegion * len(regions)).from_buffer_copy(regions.tobytes())
    f.pod = P.VspgField(len(nodes), len(regions), f.nodes, f.regions)
    f.np_nodes, f.np_regions, f.cells = nodes, regions, cells
    return f


def field_from_readback(P, nodes, regs, n_nodes, n_regions):
    """What get_guiding_field returned, as an uploadable field."""
    import ctypes as C
    a = np.frombuffer(bytes(nodes)[:n_nodes * C.sizeof(P.VspgKdNode)], dtype=NODE_DTYPE)
    b = np.frombuffer(bytes(regs)[:n_regions * C.sizeof(P.VspgFieldRegion)], dtype=REGION_DTYPE)
    return make_field(P, a, b)


def empty_regions(n):
    """n regions without lobes: every lobe float NaN."""
    R = np.zeros(n, dtype=REGION_DTYPE)
    for name in LOBE_FLOATS + ("mu",):
        R[name] = np.nan
    return R


def set_lobes(R, i, lobes):
    """lobes: (weight, kappa, mu, distance, vsp) each; the slots after them stay NaN."""
    R["n_lobes"][i] = len(lobes)
    for k, (w, kap, mu, d, vsp) in enumerate(lobes):
        R["weight"][i, k], R["kappa"][i, k], R["distance"][i, k], R["vsp"][i, k] = w, kap, d, vsp
        R["mu"][i, :, k] = mu


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def random_lobes(rng, n):
    """n lobes a trainer could have fitted: weights summing to one, kappa log-uniform in [0.05, 500], half of the distances
    infinite, the others in [0.2, 3]."""
    w = rng.random(n) + 0.05
    w = w / w.sum()
    out = []
    for k in range(n):
        d = np.inf if rng.random() < 0.5 else rng.uniform(0.2, 3.0)
        out.append((w[k], float(np.exp(rng.uniform(np.log(0.05), np.log(500.0)))), _unit(rng.normal(size=3)), d, rng.random()))
    return out


class _Tree:
    """Binary tree under construction: per node its cell and, once split, (axis, split, left, right)."""

    def __init__(self, bounds):
        self.lo = [np.array(bounds[0], dtype=np.float32)]
        self.hi = [np.array(bounds[1], dtype=np.float32)]
        self.kids = [None]

    def split(self, i, axis, split):
        split = np.float32(split)
        assert self.kids[i] is None and self.lo[i][axis] < split < self.hi[i][axis]
        l, r = len(self.kids), len(self.kids) + 1
        for side in (0, 1):
            lo, hi = self.lo[i].copy(), self.hi[i].copy()
            (hi if side == 0 else lo)[axis] = split
            self.lo.append(lo); self.hi.append(hi); self.kids.append(None)
        self.kids[i] = (axis, split, l, r)
        return l, r

    def number(self, numbering):
        """node numbers: children adjacent and after their parent.  "creation": the order of the splits (the trainer's: upper
        levels first).  "dfs": a pair of slots per split, then the whole left subtree, then the right one (light_field's)."""
        n = len(self.kids)
        if numbering == "creation":
            return np.arange(n)
        assert numbering == "dfs"
        new = np.full(n, -1)
        new[0] = 0
        count = 1
        stack = [0]
        while stack:
            i = stack.pop()
            if self.kids[i] is None:
                continue
            _, _, l, r = self.kids[i]
            new[l], new[r] = count, count + 1
            count += 2
            stack.append(r)   # popped after the whole left subtree
            stack.append(l)
        return new

    def arrays(self, numbering, region_of_leaf):
        new = self.number(numbering)
        n = len(self.kids)
        nodes = np.zeros(n, dtype=NODE_DTYPE)
        cells = np.zeros((n, 2, 3), dtype=np.float32)
        for i in range(n):
            j = new[i]
            cells[j, 0], cells[j, 1] = self.lo[i], self.hi[i]
            if self.kids[i] is None:
                nodes[j] = (0.0, 3 | (region_of_leaf[i] << 2))
            else:
                axis, split, l, r = self.kids[i]
                assert new[r] == new[l] + 1 and new[l] > j
                nodes[j] = (split, axis | (int(new[l]) << 2))
        return nodes, cells


def random_kd_field(P, n_regions, seed, numbering="creation", bounds=((-1, -1, -1), (1, 1, 1)), lobes=None):
    """Unbalanced tree of 2 n_regions - 1 nodes: random leaves split on a random axis at 20-80 % of their cell.  `lobes(rng, i)`
    gives region i's lobe list; the default leaves one region in ten without lobes and gives the others 1..8."""
    rng = np.random.default_rng(seed)
    t = _Tree(bounds)
    leaves = [0]
    while len(leaves) < n_regions:
        i = leaves.pop(int(rng.integers(len(leaves))))
        axis = int(rng.integers(3))
        lo, hi = float(t.lo[i][axis]), float(t.hi[i][axis])
        l, r = t.split(i, axis, lo + (hi - lo) * rng.uniform(0.2, 0.8))
        leaves += [l, r]
    region_of_leaf = {int(i): int(k) for i, k in zip(leaves, rng.permutation(n_regions))}   # region numbers unrelated to node numbers
    nodes, cells = t.arrays(numbering, region_of_leaf)
    R = empty_regions(n_regions)
    for i, k in sorted(region_of_leaf.items(), key=lambda e: e[1]):
        R["pivot"][k] = (t.lo[i] + t.hi[i]) / 2
        if lobes is not None:
            set_lobes(R, k, lobes(rng, k))
        else:
            set_lobes(R, k, random_lobes(rng, 0 if rng.random() < 0.1 else int(rng.integers(1, GK + 1))))
    return make_field(P, nodes, R, cells)


def spine_field(P, depth=70, bounds=((-1, -1, -1), (1, 1, 1))):
    """A chain along x: leaves at depths 1 .. depth (and the last cell at depth `depth` too), of equal width, cut off the low
    and the high end in turn.  field_lookup stops after 64 steps on both sides: leaves at depth <= 63 answer, deeper ones do not."""
    rng = np.random.default_rng(70)
    t = _Tree(bounds)
    width = (bounds[1][0] - bounds[0][0]) / (depth + 1)
    cur, region_of_leaf, leaf_depth = 0, {}, {}
    for level in range(depth):
        lo, hi = float(t.lo[cur][0]), float(t.hi[cur][0])
        low_end = level % 2 == 0
        l, r = t.split(cur, 0, lo + width if low_end else hi - width)
        leaf, cur = (l, r) if low_end else (r, l)
        region_of_leaf[leaf] = len(region_of_leaf)
        leaf_depth[region_of_leaf[leaf]] = level + 1
    region_of_leaf[cur] = len(region_of_leaf)
    leaf_depth[region_of_leaf[cur]] = depth
    nodes, cells = t.arrays("creation", region_of_leaf)
    R = empty_regions(len(region_of_leaf))
    for i, k in region_of_leaf.items():
        R["pivot"][k] = (t.lo[i] + t.hi[i]) / 2
        set_lobes(R, k, random_lobes(rng, 3))
    f = make_field(P, nodes, R, cells)
    f.leaf_depth = leaf_depth
    return f


# lobe_edge_field's regions, as slabs along x in this order
EDGE_REGIONS = ("n0", "n1", "n2", "n3", "n4", "n5", "n7", "n8", "source", "fallback", "cancel")


def lobe_edge_field(P, bounds=((-1, -1, -1), (1, 1, 1))):
    """Eleven slabs along x (balanced tree, 21 nodes).  n_lobes 0, 1, 2, 3, 4, 5, 7, 8; kappas on both sides of both clamps
    (1e-3, 1e-2, 1e4, 3e4); distances +inf, 0, -1, 1e-3 and finite ones; and three regions made for one branch each:
      "source"    lobe 0's source pivot + mu d is a point of the region (`f.on_source`): re-aiming has no direction there;
      "fallback"  8 lobes mu = (0,0,1), kappa 1e4, distance +inf: a volume vertex with wo = (0,0,1) and g = -0.98 multiplies them
                  with a lobe around -z, every product mass is below FastExp's flush, sum == 0;
      "cancel"    one lobe mu = (0,-1,0), kappa 2.18853: against the cosine lobe of the normal (0,1,0) the two cancel exactly.
    `f.slab[name]` = (lower, upper corner) of the region's cell."""
    rng = np.random.default_rng(11)
    n = len(EDGE_REGIONS)
    (x0, y0, z0), (x1, y1, z1) = bounds
    edges = np.linspace(x0, x1, n + 1).astype(np.float32)
    t = _Tree(bounds)
    region_of_leaf = {}

    def build(node, a, b):   # slabs a .. b-1 under `node`
        if b - a == 1:
            region_of_leaf[node] = a
            return
        m = (a + b) // 2
        l, r = t.split(node, 0, edges[m])
        build(l, a, m)
        build(r, m, b)

    build(0, 0, n)
    nodes, cells = t.arrays("creation", region_of_leaf)
    R = empty_regions(n)
    leaf_of = {k: i for i, k in region_of_leaf.items()}
    slab = {}
    for k, name in enumerate(EDGE_REGIONS):
        i = leaf_of[k]
        R["pivot"][k] = (t.lo[i] + t.hi[i]) / 2
        slab[name] = (t.lo[i].copy(), t.hi[i].copy())
    up, px = (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)
    rl = lambda m: random_lobes(rng, m)
    ix = EDGE_REGIONS.index
    set_lobes(R, ix("n1"), [(1.0, 1e-3, _unit((1, 2, -1)), np.inf, 0.3)])
    set_lobes(R, ix("n2"), [(0.6, 1e-2, up, 0.0, 0.2), (0.4, 3e4, _unit((0.2, 1, 0.1)), -1.0, 0.9)])
    set_lobes(R, ix("n3"), [(0.5, 1e4, _unit((0, 1, 0.05)), 1e-3, 0.1), (0.3, 5.0, up, 0.7, 0.5), (0.2, 0.5, px, np.inf, 0.8)])
    set_lobes(R, ix("n4"), [(0.25, 3e4, up, np.inf, 0.0), (0.25, 1e-3, px, 0.0, 1.0)] + rl(2))
    set_lobes(R, ix("n5"), rl(4) + [(0.1, 1e4, _unit((1, 1, 1)), 1e-3, 0.6)])
    set_lobes(R, ix("n7"), rl(6) + [(0.1, 1e-2, _unit((-1, 0, 1)), -1.0, 0.4)])
    set_lobes(R, ix("n8"), rl(7) + [(0.1, 3e4, _unit((0, -1, 0)), 2.0, 0.7)])
    # pivot + mu d with mu = (0,1,0), d = 0.5: exact in float32, and (pivot - p) + mu d == 0 exactly at that point
    k = ix("source")
    R["pivot"][k, 1] = 0.0
    set_lobes(R, k, [(0.7, 40.0, up, 0.5, 0.3), (0.3, 2.0, px, np.inf, 0.6)])
    on_source = R["pivot"][k] + np.array([0, 0.5, 0], dtype=np.float32)
    assert slab["source"][0][1] < on_source[1] < slab["source"][1][1]
    set_lobes(R, ix("fallback"), [(0.125, 1e4, (0.0, 0.0, 1.0), np.inf, 0.1 * j) for j in range(8)])
    set_lobes(R, ix("cancel"), [(1.0, float(COSINE_KAPPA), (0.0, -1.0, 0.0), np.inf, 0.5)])
    for k in range(n):   # incident-radiance mixtures: the weights of a region sum to one
        m = R["n_lobes"][k]
        if m > 0:
            R["weight"][k, :m] /= R["weight"][k, :m].sum(dtype=np.float64)
    f = make_field(P, nodes, R, cells)
    f.slab, f.on_source = slab, on_source
    return f


# ---------------------------------------------------------------------------------------------
# the fields the tests use, built once per process and never modified
# ---------------------------------------------------------------------------------------------
_BUILDERS = {
    "kd199-creation": lambda P: random_kd_field(P, 100, 100, "creation"),
    "kd255-creation": lambda P: random_kd_field(P, 128, 128, "creation"),
    "kd255-dfs": lambda P: random_kd_field(P, 128, 128, "dfs"),
    "kd257-creation": lambda P: random_kd_field(P, 129, 129, "creation"),
    "kd257-dfs": lambda P: random_kd_field(P, 129, 129, "dfs"),
    "kd8191-creation": lambda P: random_kd_field(P, 4096, 4096, "creation"),
    "kd8191-dfs": lambda P: random_kd_field(P, 4096, 4096, "dfs"),
    "spine": spine_field,
    "lobe_edge": lobe_edge_field,
}
RANDOM_FIELDS = tuple(k for k in _BUILDERS if k.startswith("kd"))
QUERY_FIELDS = ("kd255-creation", "kd257-dfs", "kd8191-creation", "kd8191-dfs", "spine", "lobe_edge")   # the GPU query test's
QUERY_CASES = ((0, 0.0), (1, 0.0), (1, 0.7), (1, -0.4), (1, 0.98), (1, -0.98))                          # (is_volume, g)
_cache = {}


def field(P, name):
    if name not in _cache:
        _cache[name] = _BUILDERS[name](P)
    return _cache[name]


def _plane_points(f, node):
    """points of `node`'s cell exactly on its split plane, and the two floats next to the plane"""
    nd = f.np_nodes[node]
    axis = int(nd["packed"] & 3)
    c = ((f.cells[node, 0].astype(np.float64) + f.cells[node, 1]) / 2).astype(np.float32)
    out = []
    for v in (nd["split"], np.nextafter(nd["split"], np.float32(-np.inf)), np.nextafter(nd["split"], np.float32(np.inf))):
        q = c.copy()
        q[axis] = v
        out.append(q)
    return out


def deep_split_node(f):
    """an interior node numbered past the LDS stage (the highest-numbered one), or None"""
    interior = np.nonzero((f.np_nodes["packed"] & 3) != 3)[0]
    return int(interior[-1]) if len(interior) and interior[-1] > KD_LDS_NODES else None


def query_set(P, name, is_volume, n_random=30000):
    """(p, n_or_wo, wi, u) float32: n_random random queries in the box, then the deterministic edge list: sampler values 0 and the
    largest float below 1; points exactly on the split plane of the root and of a node past the LDS stage (and one float to either
    side); points far outside the bounds; for lobe_edge the on-source point and the blocks that take the fallback, the
    cancelling-lobes and the untrained branch.  No NaN anywhere.  Deterministic per (name, is_volume)."""
    f = field(P, name)
    rng = np.random.default_rng([sum(map(ord, name)), int(is_volume)])
    p = rng.uniform(-1, 1, (n_random, 3)).astype(np.float32)
    a = _unit(rng.normal(size=(n_random, 3)))
    wi = _unit(rng.normal(size=(n_random, 3)))
    u = rng.random((n_random, 2)).astype(np.float32)
    below1 = np.nextafter(np.float32(1), np.float32(0))
    ep, ea, ew, eu = [], [], [], []

    def add(pt, aa=None, ww=None, uu=(0.5, 0.5)):
        ep.append(np.asarray(pt, dtype=np.float32))
        ea.append(_unit(rng.normal(size=3)) if aa is None else np.asarray(aa, dtype=np.float32))
        ew.append(_unit(rng.normal(size=3)) if ww is None else np.asarray(ww, dtype=np.float32))
        eu.append(np.asarray(uu, dtype=np.float32))

    for j in range(16):
        for uu in ((0, 0), (0, below1), (below1, 0), (below1, below1)):
            add(p[j], a[j], wi[j], uu)
    planes = _plane_points(f, 0)
    deep = deep_split_node(f)
    if deep is not None:
        planes += _plane_points(f, deep)
    for q in planes:
        add(q)
    for s in (-1e6, 1e6):
        for axis in range(3):
            q = np.zeros(3)
            q[axis] = s
            add(q)
        add((s, s, s))
        add((s, -s, 0.25))
    if name == "lobe_edge":
        def inside(region, m):
            lo, hi = f.slab[region]
            return (lo + (hi - lo) * rng.uniform(0.05, 0.95, (m, 3))).astype(np.float32)
        add(f.on_source)
        add(f.on_source, (0, 1, 0), (0, 1, 0), (0.1, 0.9))
        z = (0.0, 0.0, 1.0)
        for j, q in enumerate(inside("fallback", 256)):    # wo = +z: fallback at g = -0.98, a plain product at g = +0.98
            add(q, z, _unit((0.01 * rng.normal(), 0.01 * rng.normal(), 1.0)) if j % 2 else None)
        for q in inside("cancel", 256):                    # the surface normal the lobe was made to cancel
            add(q, (0.0, 1.0, 0.0))
        for q in inside("n0", 128):
            add(q)
    return (np.concatenate([p, np.array(ep)]), np.concatenate([a, np.array(ea)]), np.concatenate([wi, np.array(ew)]),
            np.concatenate([u, np.array(eu)]))


# ---------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------
def model_lookup(f, p):
    """field_lookup: (region or -1, the node the descent ended in or -1, steps taken).  float32 comparisons, as on the device."""
    nodes, n_nodes, n_regions = f.np_nodes, len(f.np_nodes), len(f.np_regions)
    p = np.ascontiguousarray(p, dtype=np.float32)
    N = len(p)
    node = np.zeros(N, dtype=np.int64)
    region = np.full(N, -1, dtype=np.int64)
    last = np.full(N, -1, dtype=np.int64)
    active = np.ones(N, dtype=bool)
    rows = np.arange(N)
    for _ in range(MAX_DESCENT):
        if not active.any():
            break
        nd = nodes[node]
        axis = (nd["packed"] & 3).astype(np.int64)
        idx = (nd["packed"] >> 2).astype(np.int64)
        leaf = active & (axis == 3)
        region[leaf] = np.where(idx[leaf] < n_regions, idx[leaf], -1)
        last[leaf] = node[leaf]
        active &= ~leaf
        c = p[rows, np.minimum(axis, 2)]
        nxt = idx + np.where(c < nd["split"], 0, 1)
        gone = active & (nxt >= n_nodes)
        active &= ~gone
        node = np.where(active, nxt, node)
    return region, last


def _flush_exp(x):
    """exp, zero where FastExp returns zero: FastExp(x) = 2^floor(x') * poly(x' - floor(x')), x' = x * log2(e) in float32, poly in
    [1, 2), and a result with exponent below -126 is returned as 0 -- i.e. exactly where x' < -126."""
    xp = (np.asarray(x, dtype=np.float64)).astype(np.float32) * np.float32(1.442695041)
    with np.errstate(under="ignore", over="ignore"):
        return np.where(xp < -126, 0.0, np.exp(np.minimum(x, 700.0)))


def _clamp(k):
    return np.clip(k, np.float32(1e-2).astype(np.float64), 1e4)


def _norm(k):
    """vMF normalisation kappa / (2 pi (1 - e^{-2 kappa}))"""
    return k / (2 * np.pi * (1 - _flush_exp(-2 * k)))


def model_query(f, is_volume, g, p, n_or_wo, wi, eps_fe=0.0, few=8.0):
    """DESIGN 10 in float64.  f may be None (no field of that kind uploaded).  Returns per query: region, node, ok, branch (index
    into BRANCHES), pdf, incoming_pdf, vsp, and for each of the three a relative and an absolute error bound (rtol_*, atol_*) for
    an evaluation in float32 with FastExp, BEFORE any safety margin:

      u = 2^-24.  A value built from positive terms has the largest relative error of its terms.  Per lobe:
        direction   raw . w carries  few u (1 + A),  A = (|pivot - p| + d) / |pivot - p + mu d|  (the cancellation in re-aiming),
        norm(k)     (eps + 4 u k) E / (1 - E) + 4 u,  E = e^{-2k}: FastExp's relative error eps on E and the rounding of its
                    argument, amplified by the subtraction 1 - E (about 1 / (2k) for small k),
        exponent    FastExp(k x), x = c . w - 1: the rounding of x (direction error, one more u for FastExp's own x log2 e) times k,
        product     kp = |raw kr + m2 k2| carries dkp = 2 few u (kr + k2)(1 + A) absolutely; it enters the weight's exponent
                    (kp - kr) - k2 as is, the mass through kc = clamp(kp) relatively, and the evaluation's exponent through
                    c1 = kr / kp, c2 = k2 / kp:  (kc / kp)(kr + k2)(direction + 2 dkp / kp + 4 u) + 2 dkp.
      pdf = (sum of terms) / (sum of masses): the two bounds add.  vsp = num / den: twice the incident term's bound.
      Absolute: FastExp flushes results below 2^-126 and float32 products lose bits below it: (sum of weights) 2^-125 + 8 * 2^-149,
      scaled like the value."""
    p = np.ascontiguousarray(p, dtype=np.float32)
    N = len(p)
    u_ = 2.0 ** -24
    out = dict(region=np.full(N, -1, dtype=np.int64), node=np.full(N, -1, dtype=np.int64), ok=np.zeros(N, dtype=np.int32),
               branch=np.full(N, BRANCHES.index("outside")), n_lobes=np.zeros(N, dtype=np.int64))
    for k in ("pdf", "incoming_pdf", "rtol_pdf", "rtol_incoming_pdf", "rtol_vsp", "atol_pdf", "atol_incoming_pdf", "atol_vsp"):
        out[k] = np.zeros(N)
    out["vsp"] = np.full(N, -1.0)
    if f is None:
        return out
    region, node = model_lookup(f, p)
    out["region"], out["node"] = region, node
    R = f.np_regions[np.maximum(region, 0)]
    n = np.where(region >= 0, np.minimum(R["n_lobes"], GK), 0)
    out["n_lobes"] = n
    out["ok"] = ((region >= 0) & (n > 0)).astype(np.int32)
    out["branch"][(region >= 0) & (n <= 0)] = BRANCHES.index("untrained")
    ok = out["ok"] == 1
    live = np.arange(GK)[None, :] < n[:, None]                      # [N, GK]
    with np.errstate(all="ignore"):
        P64 = p.astype(np.float64)
        w = np.asarray(wi, dtype=np.float32).astype(np.float64)
        a_in = np.asarray(n_or_wo, dtype=np.float32).astype(np.float64)
        # ---- the lobes re-aimed at the query point
        mu = np.transpose(R["mu"].astype(np.float64), (0, 2, 1))    # [N, GK, 3]
        d = R["distance"].astype(np.float64)
        pp = (R["pivot"].astype(np.float32) - p).astype(np.float64)  # the one float32 subtraction the position enters through
        t = pp[:, None, :] + mu * d[..., None]
        tl = np.linalg.norm(t, axis=-1)
        aim = live & (d > 0) & np.isfinite(d) & (tl > 0)
        raw = np.where(aim[..., None], t / np.where(tl > 0, tl, 1)[..., None], mu)
        A = np.where(aim, (np.linalg.norm(pp, axis=-1)[:, None] + np.abs(d)) / np.where(tl > 0, tl, 1), 0.0)
        dirr = few * u_ * (1 + A)
        kr = _clamp(R["kappa"].astype(np.float64))
        wt = R["weight"].astype(np.float64)

        def rnorm(k):
            E = np.exp(-2 * k)
            return (eps_fe + 4 * u_ * k) * E / (1 - E) + 4 * u_

        def mx(x):
            return np.max(np.where(live, x, 0.0), axis=1)

        def sm(x):
            return np.sum(np.where(live, x, 0.0), axis=1)

        b = wt * _norm(kr)
        x1 = np.einsum("nkc,nc->nk", raw, w)
        e = b * _flush_exp(kr * (x1 - 1))
        r_inc = rnorm(kr) + eps_fe + kr * (dirr + 4 * u_) + 4 * u_
        inc = sm(e)
        out["incoming_pdf"] = np.where(ok, inc, 0.0)
        out["rtol_incoming_pdf"] = mx(r_inc) + 8 * u_
        floor_ = sm(b) * 2.0 ** -125 + 8 * 2.0 ** -149
        out["atol_incoming_pdf"] = floor_
        vsp = sm(e * R["vsp"].astype(np.float64)) / inc
        out["vsp"] = np.where(ok & (inc > 0), vsp, -1.0)
        out["rtol_vsp"] = 2 * mx(r_inc) + 16 * u_
        out["atol_vsp"] = np.where(inc > 0, floor_ / inc, 0.0)
        # ---- the product lobe
        if is_volume:
            ag = abs(float(np.float32(g)))
            have = ag >= 1e-3
            ag = min(ag, float(np.float32(0.99)))
            k2 = ag * (3 - ag * ag) / (1 - ag * ag) if have else 0.0
            axis = a_in if g > 0 else -a_in
            m2 = axis / np.linalg.norm(axis, axis=1, keepdims=True)
        else:
            have, k2, m2 = True, float(COSINE_KAPPA), a_in
        if not have:
            pdf = inc / sm(wt)
            out["pdf"] = np.where(ok, pdf, 0.0)
            out["rtol_pdf"] = out["rtol_incoming_pdf"] + 16 * u_
            out["atol_pdf"] = floor_ / sm(wt)
            out["branch"][ok] = BRANCHES.index("plain")
            return out
        s = raw * kr[..., None] + m2[:, None, :] * k2
        kp = np.linalg.norm(s, axis=-1)
        # the cancel decision as the device takes it: in float32
        s32 = raw.astype(np.float32) * kr.astype(np.float32)[..., None] + (m2.astype(np.float32) * np.float32(k2))[:, None, :]
        kp32 = np.sqrt(np.sum(s32 * s32, axis=-1, dtype=np.float32))
        cancel = live & ~(kp32 > np.float32(1e-6))
        kc = _clamp(kp)
        a = b * _norm(k2) * _flush_exp((kp - kr) - k2)
        mass = a * (2 * np.pi * (1 - _flush_exp(-2 * kc))) / kc
        total = sm(mass)
        fallback = ok & ~((total > 0) & np.isfinite(total))
        x2 = np.einsum("nkc,nc->nk", s, w) / np.where(kp > 0, kp, 1)     # (product's mean direction) . w
        x2 = np.where(cancel, 0.0, x2)
        term = a * _flush_exp(kc * (x2 - 1))
        pdf = sm(term) / total
        dkp = 2 * few * u_ * (kr + k2) * (1 + A)
        rel_kp = dkp / np.maximum(kp, 1e-300)
        free = (kp > 1e-2) & (kp < 1e4)                                # kc follows kp
        r_a = rnorm(kr) + rnorm(k2) + eps_fe + dkp + 4 * u_ * (kp + kr + k2)
        r_mass = r_a + rnorm(kc) + np.where(free, rel_kp, 0.0) + 4 * u_
        r_term = r_a + eps_fe + np.where(cancel, 0.0, (kc / np.maximum(kp, 1e-300)) * (kr + k2) * (dirr + 2 * rel_kp + 4 * u_)) \
            + 2 * np.where(free, dkp, 0.0) + 4 * kc * u_
        out["pdf"] = np.where(ok, np.where(fallback, inc, pdf), 0.0)
        out["rtol_pdf"] = np.where(fallback, out["rtol_incoming_pdf"], mx(r_term) + mx(r_mass) + 16 * u_)
        out["atol_pdf"] = np.where(fallback, floor_, (sm(b * _norm(k2)) * 2.0 ** -125 + 8 * 2.0 ** -149) / np.where(total > 0, total, 1))
        out["branch"][ok] = BRANCHES.index("product")
        out["branch"][ok & np.any(cancel, axis=1)] = BRANCHES.index("cancel")
        out["branch"][fallback] = BRANCHES.index("fallback")
    return out


# ---------------------------------------------------------------------------------------------
# fields upload must refuse
# ---------------------------------------------------------------------------------------------
class _Raw:
    """something with a .pod, like P.Field, around arrays that may be absent"""

    def __init__(self, P, n_nodes, n_regions, nodes, regions):
        self.nodes, self.regions = nodes, regions
        self.pod = P.VspgField(n_nodes, n_regions, nodes, regions)


def malformed_fields(P):
    """(label, field) pairs: lobe_edge_field with one thing wrong each"""
    good = field(P, "lobe_edge")
    n_nodes, n_regions = len(good.np_nodes), len(good.np_regions)
    leaf = int(np.nonzero((good.np_nodes["packed"] & 3) == 3)[0][0])
    out = []

    def variant(label, node=None, region=None):
        nodes, regions = good.np_nodes.copy(), good.np_regions.copy()
        if node is not None:
            nodes["packed"][node[0]] = node[1]
        if region is not None:
            regions["n_lobes"][region[0]] = region[1]
        out.append((label, make_field(P, nodes, regions)))

    variant("child index == parent", node=(0, 0 | (0 << 2)))
    variant("child index < parent", node=(2, 1 | (1 << 2)))
    variant("child index + 1 == n_nodes", node=(0, 0 | ((n_nodes - 1) << 2)))
    variant("child index past the array", node=(0, 2 | ((n_nodes + 5) << 2)))
    variant("leaf region == n_regions", node=(leaf, 3 | (n_regions << 2)))
    variant("n_lobes 9", region=(3, 9))
    variant("n_lobes -1", region=(3, -1))
    out.append(("no node array", _Raw(P, n_nodes, n_regions, None, good.regions)))
    out.append(("no region array", _Raw(P, n_nodes, n_regions, good.nodes, None)))
    return out


# ---------------------------------------------------------------------------------------------
# the sum == 0 fallback inside the path kernels
# ---------------------------------------------------------------------------------------------
FALLBACK_G = -0.98
FALLBACK_MEDIA = ("fog", "grid")


def fallback_case(P, medium, n=30000):
    """(scene, params, W, H, pixel_xy, sample_index): lobe_edge_field under a medium of g = -0.98.  A volume vertex in the
    "fallback" slab whose ray runs along +z multiplies eight kappa = 1e4 lobes around +z with an HG lobe of kappa 50 around
    -z: every product mass is below FastExp's flush, sum == 0, and the vertex works with the incident-radiance mixture."""
    import scenes
    W, H = 64, 48
    if medium == "fog":
        scene = P.fog_box_scene(W, H)
        scene.medium.g = FALLBACK_G
    else:
        scene = scenes.grid_scene(scenes.cloud_density(16), (16, 16, 16), (0.05, 0.08, 0.1), (3.0, 2.6, 2.2), g=FALLBACK_G,
                                  bmin=(-0.8, -0.8, -0.5), bmax=(0.8, 0.7, 0.9), W=W, H=H)
    rng = np.random.default_rng(98)
    pix = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], axis=1).astype(np.int32)
    return scene, P.default_params(), W, H, pix, rng.integers(0, 4096, n).astype(np.int32)
