"""A NumPy mirror of ONE guiding-field update (Field::Update: csrc/vspg_train_kernels.h k_train_*, oracle/vspg_oracle.c field_update_one).

The update consists of sums over the samples (position statistics, E-step statistics) and of plain float32 arithmetic on
those sums (decay, +=, the split decision, the halving, the pivot division, the M-step).  The mirror does the second kind --
bit for bit, in float32, in the code's order -- on sums it is HANDED: the device's own (as the exchange hook shows them) or the
oracle's (sequential doubles cast to float).  For the first kind it offers float64 reference sums and the one tolerance the
tests use, the float32 summation bound.  No device and no oracle renderer in here; the per-sample E-step terms come from
oracle_lib.train_estep_terms.

Buffers: an accumulator `acc` is float32 [KEYS, STAT_FLOATS] (key = field * CAP_REGIONS + region; columns in the order of
RegionStats: n, sum_p[3], sum_p2[3], then S, R0, R1, R2, D, V, Qv, Qs per lobe), `acc[f]`-style views per field are
`field_acc(acc, f)`."""
import numpy as np

import field_models as fm

GK = fm.GK
F32 = np.float32
CAP_NODES, CAP_REGIONS = 8192, 4097          # kTrainCapNodes, kTrainCapRegions
KEYS = 2 * CAP_REGIONS                        # kTrainKeys
STAT_FLOATS = 7 + 8 * GK                      # kStatFloats
SPLIT_COUNT, DECAY, MAX_DEPTH = F32(4096.0), F32(0.75), 24
WEIGHT_CLAMP, KAPPA_INIT = F32(32.0), F32(2.0)
MIN_UPDATE_SAMPLES = 128
LDS_NODES = 512                               # kTrainLdsNodes: nodes per field k_train_lookup stages in LDS
SAMPLE_VOLUME, SAMPLE_NEXT_VOLUME = 1, 2
VSP_CONTRIBUTION, VSP_VARIANCE = 0, 1
EPS = 2.0 ** -24                              # unit roundoff of float32


def field_acc(acc, f):
    return np.asarray(acc).reshape(KEYS, STAT_FLOATS)[f * CAP_REGIONS:(f + 1) * CAP_REGIONS]


def kappa_clamp(k):
    k = np.asarray(k, dtype=F32)
    return np.where(k < F32(1e-2), F32(1e-2), np.where(k > F32(1e4), F32(1e4), k)).astype(F32)


class _Tree:
    """what field_models.model_lookup reads"""

    def __init__(self, nodes, regions):
        self.np_nodes, self.np_regions = nodes, regions


class FieldMirror:
    """One field: nodes, regions, RegionStats (float part + depth)."""

    def __init__(self):
        self.nodes = np.zeros(CAP_NODES, dtype=fm.NODE_DTYPE)
        self.regions = np.zeros(CAP_REGIONS, dtype=fm.REGION_DTYPE)
        self.stats = np.zeros((CAP_REGIONS, STAT_FLOATS), dtype=F32)
        self.depth = np.zeros(CAP_REGIONS, dtype=np.int32)
        self.n_nodes = self.n_regions = 1
        self.nodes["packed"][0] = 3           # one leaf -> region 0, untrained

    def set_tree(self, nodes, regions):
        """adopt a field as read back (the statistics stay as they are)"""
        self.n_nodes, self.n_regions = len(nodes), len(regions)
        self.nodes[:] = 0
        self.regions[:] = 0
        self.nodes[:self.n_nodes] = nodes
        self.regions[:self.n_regions] = regions

    def node_bytes(self):
        return self.nodes[:self.n_nodes].tobytes()

    def region_bytes(self):
        return self.regions[:self.n_regions].tobytes()

    # ---- field_lookup ------------------------------------------------------------------------------------------------------------
    def lookup(self, points):
        """region per point (-1: outside the tree); float32 compares"""
        region, _ = fm.model_lookup(_Tree(self.nodes[:self.n_nodes], self.regions[:self.n_regions]), np.asarray(points, dtype=F32).reshape(-1, 3))
        return region

    def leaf_cells(self, bmin, bmax):
        """(region, lower corner, upper corner) of every leaf, descending from the box [bmin, bmax]"""
        out = []
        stack = [(0, np.array(bmin, dtype=np.float64), np.array(bmax, dtype=np.float64))]
        while stack:
            nd, lo, hi = stack.pop()
            packed, split = int(self.nodes["packed"][nd]), float(self.nodes["split"][nd])
            axis, idx = packed & 3, packed >> 2
            if axis == 3:
                out.append((idx, lo, hi))
                continue
            l_hi, r_lo = hi.copy(), lo.copy()
            l_hi[axis] = r_lo[axis] = split
            stack.append((idx, lo, l_hi))
            stack.append((idx + 1, r_lo, hi))
        return out

    # ---- k_train_decay -------------------------------------------------------------------------------------------------------------
    def decay(self):
        self.stats[:self.n_regions] *= DECAY

    # ---- k_train_split, first half: the batch's position statistics ----------------------------------------------------------------
    def add_pos(self, acc3):
        a = np.asarray(acc3).reshape(CAP_REGIONS, STAT_FLOATS)[:self.n_regions, :7].astype(F32)
        self.stats[:self.n_regions, :7] += a

    # ---- k_train_split, second half -------------------------------------------------------------------------------------------------
    def split(self):
        """One split level, sequential over the nodes as they stood (field_update_one step 3): a leaf splits if its region has
        n > 4096 and depth < 24, two node slots and one region slot are left, and the variance of its largest-variance axis
        (ties: x before y before z ... `>=`) is > 0.  Returns the number of splits."""
        st, nodes, regs = self.stats, self.nodes, self.regions
        n_nodes0, made = self.n_nodes, 0
        with np.errstate(all="ignore"):
            for nd in range(n_nodes0):
                packed = int(nodes["packed"][nd])
                if (packed & 3) != 3:
                    continue
                reg = packed >> 2
                s0 = st[reg]
                if not (s0[0] > SPLIT_COUNT) or self.depth[reg] >= MAX_DEPTH:
                    continue
                if self.n_nodes + 2 > CAP_NODES or self.n_regions + 1 > CAP_REGIONS:
                    continue
                mean = s0[1:4] / s0[0]                       # float32 throughout
                var = s0[4:7] / s0[0] - mean * mean
                axis = (0 if var[0] >= var[2] else 2) if var[0] >= var[1] else (1 if var[1] >= var[2] else 2)
                if not (var[axis] > 0):
                    continue
                left, newreg = self.n_nodes, self.n_regions
                self.n_nodes += 2
                self.n_regions += 1
                s0 *= F32(0.5)
                self.depth[reg] += 1
                st[newreg] = s0
                self.depth[newreg] = self.depth[reg]
                regs[newreg] = regs[reg]
                nodes[left] = (0.0, (reg << 2) | 3)
                nodes[left + 1] = (0.0, (newreg << 2) | 3)
                nodes[nd] = (mean[axis], (left << 2) | axis)
                made += 1
        return made

    def has_bare_region(self):
        return bool((self.regions["n_lobes"][:self.n_regions] == 0).any())

    # ---- k_train_init_regions ----------------------------------------------------------------------------------------------------------
    def init_regions(self, acc4):
        """pivot = sum_p / n and the eight diagonal lobes for every region without lobes that saw a sample.  The division is done
        in acc4's precision and the quotient stored as float32: float32 sums as the device has them, doubles as in the oracle."""
        a = np.asarray(acc4).reshape(CAP_REGIONS, -1)[:self.n_regions]
        R = self.regions
        c = F32(0.57735026918962576451)
        k = np.arange(GK)
        with np.errstate(all="ignore"):
            for i in np.nonzero((R["n_lobes"][:self.n_regions] == 0) & (a[:, 0] > 0))[0]:
                R["pivot"][i] = (a[i, 1:4] / a[i, 0]).astype(F32)
                R["n_lobes"][i] = GK
                R["weight"][i] = F32(1.0) / F32(GK)
                R["kappa"][i] = KAPPA_INIT
                R["mu"][i, 0] = np.where(k & 1, -c, c)
                R["mu"][i, 1] = np.where(k & 2, -c, c)
                R["mu"][i, 2] = np.where(k & 4, -c, c)
                R["distance"][i] = np.inf
                R["vsp"][i] = F32(0.5)

    # ---- k_train_mstep ----------------------------------------------------------------------------------------------------------------
    def mstep(self, acc5, vspcriterion):
        """statistics += the E-step sums (lobes k < n_lobes only), then weights, mean directions, concentrations, distances and
        vsp, float32 in the code's order"""
        n = self.n_regions
        a = np.asarray(acc5).reshape(CAP_REGIONS, STAT_FLOATS)[:n, 7:].astype(F32).reshape(n, 8, GK)
        R = self.regions[:n]
        nl = np.minimum(R["n_lobes"], GK)
        lobe = np.arange(GK)[None, :] < nl[:, None]                    # [n, GK]: k < n_lobes (no row at all where n_lobes <= 0)
        st = self.stats[:n, 7:].reshape(n, 8, GK)                      # view: S, R0, R1, R2, D, V, Qv, Qs
        with np.errstate(all="ignore"):
            st += np.where(lobe[:, None, :], a, F32(0))
            S, R0, R1, R2, D, V, Qv, Qs = (st[:, j, :] for j in range(8))
            Stot = np.zeros(n, dtype=F32)
            for k in range(GK):
                Stot = np.where(lobe[:, k], Stot + S[:, k], Stot).astype(F32)
            go = Stot > 0                                              # regions the M-step rewrites (n_lobes > 0 is implied)
            go &= nl > 0
            floorw = F32(1e-3) / F32(GK)
            weight = R["weight"].copy()
            wsum = np.zeros(n, dtype=F32)
            for k in range(GK):
                wk = S[:, k] / Stot
                wk = np.where(wk < floorw, floorw, wk).astype(F32)
                on = go & lobe[:, k]
                weight[:, k] = np.where(on, wk, weight[:, k])
                wsum = np.where(on, wsum + wk, wsum).astype(F32)
            rl = np.sqrt(((R0 * R0 + R1 * R1).astype(F32) + R2 * R2).astype(F32)).astype(F32)
            fit = go[:, None] & lobe & (S > 0) & (rl > 0)
            rbar = rl / S
            rbar = np.where(rbar > F32(0.9999), F32(0.9999), rbar).astype(F32)
            r2 = (rbar * rbar).astype(F32)
            kappa = kappa_clamp((rbar * (F32(3) - r2)).astype(F32) / (F32(1) - r2))
            dist = np.where(D > 0, S / D, F32(np.inf)).astype(F32)
            if vspcriterion == VSP_VARIANCE:
                qv, qs = np.sqrt(Qv).astype(F32), np.sqrt(Qs).astype(F32)
                vsp = np.where(qv + qs > 0, qv / (qv + qs), F32(0.5)).astype(F32)
            else:
                vsp = (V / S).astype(F32)
            for a_, Ra in enumerate((R0, R1, R2)):
                R["mu"][:, a_, :] = np.where(fit, Ra / rl, R["mu"][:, a_, :])
            R["kappa"] = np.where(fit, kappa, R["kappa"])
            R["distance"] = np.where(fit, dist, R["distance"])
            R["vsp"] = np.where(fit, vsp, R["vsp"])
            R["weight"] = np.where(go[:, None] & lobe, weight / wsum[:, None], R["weight"])
        self.stats[:n, 7:] = st.reshape(n, 8 * GK)


class Mirror:
    """both fields of a renderer: 0 surface, 1 volume"""

    def __init__(self):
        self.f = [FieldMirror(), FieldMirror()]

    def keys(self, samples):
        """sort key of every sample as k_train_lookup computes it: field * CAP_REGIONS + region, -1 outside the tree"""
        vol = (samples["flags"] & SAMPLE_VOLUME) != 0
        key = np.full(len(samples), -1, dtype=np.int64)
        for f in (0, 1):
            m = vol == bool(f)
            if m.any():
                reg = self.f[f].lookup(samples["p"][m])
                key[m] = np.where(reg >= 0, f * CAP_REGIONS + reg, -1)
        return key


# ---- reference sums ---------------------------------------------------------------------------------------------------------------------
def bin_sums(keys, terms):
    """Per key and column: (the sum of `terms` as sequential doubles in sample order, the sum of |terms|, the number of
    samples of the key).  terms: [n, C]; samples with key < 0 are left out."""
    keys = np.asarray(keys)
    ok = keys >= 0
    k = keys[ok]
    t = np.asarray(terms)[ok]
    C = t.shape[1]
    s, a = np.zeros((KEYS, C)), np.zeros((KEYS, C))
    for j in range(C):
        col = t[:, j].astype(np.float64)
        s[:, j] = np.bincount(k, weights=col, minlength=KEYS)
        a[:, j] = np.bincount(k, weights=np.abs(col), minlength=KEYS)
    return s, a, np.bincount(k, minlength=KEYS)


def pos_terms(samples, squares=F32):
    """[n, 7]: 1, p, p^2 -- the squares as float32 products (k_train_pos) or as double products (field_update_one)"""
    p = samples["p"].astype(F32)
    p2 = (p * p).astype(F32).astype(np.float64) if squares == F32 else p.astype(np.float64) ** 2
    return np.concatenate([np.ones((len(p), 1)), p.astype(np.float64), p2], axis=1)


def estep_terms(mirror, samples, keys, wmax):
    """[n, 8 * GK] float32 per-sample E-step terms on the mirror's regions as they stand (zero for a sample outside the tree),
    and the valid flags: oracle_train_estep_terms, region by region"""
    import oracle_lib
    keys = np.asarray(keys)
    terms = np.zeros((len(samples), 8 * GK), dtype=F32)
    valid = np.zeros(len(samples), dtype=np.int32)
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    first = np.nonzero(np.r_[True, sk[1:] != sk[:-1]])[0] if len(sk) else np.zeros(0, dtype=np.int64)
    ends = np.r_[first[1:], len(sk)]
    for b, e in zip(first, ends):
        key = int(sk[b])
        if key < 0:
            continue
        f, reg = divmod(key, CAP_REGIONS)
        idx = order[b:e]
        t, v = oracle_lib.train_estep_terms(mirror.f[f].regions[reg], samples[idx], wmax)
        terms[idx], valid[idx] = t, v
    return terms, valid


def sum_bound(m, abs_sum):
    """|float32 sum in any order - exact sum| <= m * 2^-24 * sum |x_i| for m terms: every one of the m - 1 additions rounds
    once (relative error 2^-24 of a partial sum that never exceeds sum |x_i|); m in place of m - 1 covers the reference's
    final rounding to float32 where one is compared."""
    return np.asarray(m, dtype=np.float64) * EPS * np.asarray(abs_sum, dtype=np.float64)
