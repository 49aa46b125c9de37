"""Free flight through a COLOURED RGB grid medium against the mathematics: VSPG_TMAJ_PLAIN of vspg_sample_tmaj_batch -- T_maj, the
callback count, the last collision, and sigma_t / sigma_maj of the hero channel at every callback -- against the float64 walk of
tests/free_flight_model.py, which is imported, not edited, and given the new medium:

  * the majorant lattice is rgbgrid_model.majorant32's 16^3 grid with sigma_t = (1, 1, 1): one scalar step function for all channels;
  * the density function is per channel: scale * (Lookup(sigma_a) + Lookup(sigma_s))[channel], the trilinear interpolant of the model.

Comparison rules of this file (the forms of free_flight_model.compare, for the quantities compared here):
  count     exact on rays without a tie;
  T_maj     relative error <= pieces * FastExp's error + d V + 1e-5                     (d, V: free_flight_model.pieces);
  position  of the LAST collision (and of every stepped one): <= d + (k + 4) 2^-24 (|o| + t + 1) + 1e-4 cell extents;
  ratio     |sigma_t[ch] / sigma_maj - model| <= 2^-24 sum + (density_rounding(sigma_a) + density_rounding(sigma_s)) / M
            + 5 2^-24 ratio + 1e-6: two interpolations, the two scalings, the sum and the quotient;
  misses    exact.
Tie rules: free_flight_model's (a draw within TIE_MARGIN of its piece's end or within the float32 uncertainty of that end takes the
ray out from there on; grazing rays are out).  Its cap -- at most 1 % of a fixture's rays tied -- is a CONDITION of the fixtures,
shown on the CPU with the model alone (test_model_alone_stays_under_the_tie_cap) before the GPU test relies on it."""
import functools

import numpy as np
import pytest

import free_flight_model as ff
import oracle_lib
import rgbgrid_model as M
from conftest import load_package

f32 = np.float32
EPS = 2.0 ** -24
RECORD = 48          # collisions of a walk kept one by one: the last collision is compared where the walk has at most this many
FLIGHT_FIXTURES = ("coloured-20x18x17", "coloured-placed-9x9x9")
BOUNDS = {"tail": 1e-5, "position": 1e-4, "ratio": 1e-6}


def fixture_medium(name):
    n = (20, 18, 17) if name == "coloured-20x18x17" else (9, 9, 9)
    seed = 60 if name == "coloured-20x18x17" else 70
    # spatially varying, different per channel, a fifth of the voxels empty; majorants up to 0.75 (1 + 2): tau_maj stays below ~6
    med = M.RgbGrid(M.coloured(n, seed, hi=1.0), M.coloured(n, seed + 1, hi=2.0), p0=ff.BMIN, p1=ff.BMAX, g=0.2, scale=0.75)
    if "placed" in name:
        med.m = ff.placement()
    return med


class FlightMedium(ff.Medium):
    """free_flight_model.Medium for an RGB grid: the lattice and its majorants; `dens` is one channel's density field."""

    def __init__(self, scene, med, dens):
        m = scene.medium
        f = lambda a: np.array([np.float32(x) for x in a], dtype=np.float64)
        self.nvdb = False
        self.n = med.n
        self.bmin, self.bmax = f(m.bounds_min), f(m.bounds_max)
        self.sigma_t = np.ones(3)                      # SampleRay: DDAMajorantIterator with sigma_t = 1 (media.h:453-454)
        self.dens = np.asarray(dens, dtype=np.float64)
        self.M = M.majorant32(med).astype(np.float64)
        self.MR = 16
        self.index_min, self.voxel, self.origin, self.offset = np.zeros(3), np.ones(3), np.zeros(3), 0.0
        self.xform = f(m.medium_from_render).reshape(4, 4) if int(m.has_transform) else None


class FlightCase:
    def __init__(self, name):
        P = load_package()
        self.name, self.med = name, fixture_medium(name)
        med = self.med
        s = oracle_lib.fog_box_scene(16, 16)
        P.set_rgb_grid_medium(s, med.sigma_a, med.sigma_s, None, p0=[float(v) for v in med.p0], p1=[float(v) for v in med.p1], g=med.g, scale=float(med.scale))
        if med.m is not None:
            P.set_medium_transform(s, med.m)
            med.set_inverse(np.array(s.medium.medium_from_render[:], f32))   # the mirror reads the matrix the record holds
        self.scene = s
        k = np.float64(med.scale)
        a, sg = med.sigma_a.astype(np.float64) * k, med.sigma_s.astype(np.float64) * k
        self.sigma_t = [FlightMedium(s, med, a[..., c] + sg[..., c]) for c in range(3)]     # the new density function, per channel
        self.parts = [(FlightMedium(s, med, a[..., c]), FlightMedium(s, med, sg[..., c])) for c in range(3)]   # for its float32 rounding term
        self.q = ff.make_queries(self.sigma_t[0], 900 + FLIGHT_FIXTURES.index(name), zero_group=med.m is None)
        self.w = ff.walk(self.sigma_t[0], self.q, ff.PLAIN, record=RECORD)          # (the walk itself reads the lattice only)

    def out_all(self):
        return np.abs(self.w["pc"]["slack"]) < ff.GRAZE

    def tie_share(self):
        return float(np.mean(self.out_all() | self.w["tied"]))

    def ratio(self, p_render, ch):
        """(sigma_t[ch] / 1 at the points, its derived float32 rounding term): per point its own channel."""
        val, err = np.zeros(len(p_render)), np.zeros(len(p_render))
        for c in range(3):
            sel = ch == c
            if sel.any():
                val[sel] = ff.density(self.sigma_t[c], p_render[sel])
                err[sel] = ff.density_rounding(self.parts[c][0], p_render[sel]) + ff.density_rounding(self.parts[c][1], p_render[sel])
        return val, err


@functools.lru_cache(maxsize=None)
def flight_case(name):
    return FlightCase(name)


@pytest.mark.parametrize("name", FLIGHT_FIXTURES)
def test_model_alone_stays_under_the_tie_cap(name):
    """The condition of the GPU comparison, on the CPU: the fixture's batch, walked by the model alone, has at most 1 % of its rays
    tied or grazing; it also has what the comparison needs -- hits, misses, collisions, channels that differ."""
    cs = flight_case(name)
    w = cs.w
    print("%s: %d rays, %d hit, ties %.4f, callbacks per ray up to %d, tau_maj up to %.2f" % (name, len(cs.q), int(w["hit"].sum()), cs.tie_share(), int(w["K"].max()),
                                                                                                   float(w["tau"].max())))
    assert cs.tie_share() <= ff.TIE_CAP
    assert w["hit"].sum() > 1000 and (~w["hit"]).sum() > 100 and (w["K"] > 0).sum() > 1000 and w["K"].max() <= RECORD and w["tau"].max() < 8
    p = np.random.default_rng(1).uniform(cs.sigma_t[0].bmin, cs.sigma_t[0].bmax, size=(500, 3))
    if cs.med.m is not None:
        p = p @ cs.med.m[:3, :3].astype(np.float64).T + cs.med.m[:3, 3].astype(np.float64)
    v = [ff.density(cs.sigma_t[c], p) for c in range(3)]
    assert np.abs(v[0] - v[1]).mean() > 0.1 and np.abs(v[1] - v[2]).mean() > 0.1, "the channels of a coloured fixture differ"
    # the model's density function is the mirror's SamplePoint (float32) to rounding
    sa, ss, _ = M.sample_point32(cs.med, p.astype(f32))
    for c in range(3):
        assert np.abs((sa[:, c].astype(np.float64) + ss[:, c]) - ff.density(cs.sigma_t[c], p.astype(f32))).max() <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("name", FLIGHT_FIXTURES)
def test_plain_free_flight_equals_the_model(gpu_pkg, name):
    P = gpu_pkg
    cs = flight_case(name)
    w, q, N = cs.w, cs.q, len(cs.q)
    pc = w["pc"]
    r = P.Renderer(cs.scene, P.app_f_params(), 16, 16)
    res0 = ff.run_batch(r, ff.PLAIN, q)
    ray, k, qs = ff.step_queries(q, res0["n_callbacks"])
    resk = ff.run_batch(r, ff.PLAIN, qs)
    r.close()
    out_all = cs.out_all()
    untied = ~out_all & ~w["tied"]
    ties = cs.tie_share()
    worst = lambda err, derived, unit: float(np.max((err - derived) / unit)) if len(err) else -np.inf
    # ---- counts and misses: exact
    count_mismatches = int(np.sum(untied & (res0["n_callbacks"] != w["K"])))
    To = res0["T_maj"].astype(np.float64)
    miss = ~w["hit"] & ~out_all
    miss_violations = int(np.sum(miss & ((res0["n_callbacks"] != 0) | (To != 1).any(axis=1) | (res0["last_t"] != -1))))
    # ---- T_maj: what lies behind the last collision, the same scalar in the three channels
    sel = untied & w["hit"]
    dV = pc["delta"] * pc["variation"]
    terr = np.abs(To / w["tail"] - 1).max(axis=1)
    tail = worst(terr[sel], (ff.fast_exp_error() * np.maximum(w["tail_pieces"], 1) + dV)[sel], np.ones(int(sel.sum())))
    # ---- the last collision of the whole walk
    last = sel & (w["K"] >= 1) & (w["K"] <= RECORD)
    rows, kl = np.flatnonzero(last), w["K"][last] - 1
    perr = np.maximum(np.linalg.norm(res0["last_p"][rows].astype(np.float64) - w["p"][rows, kl], axis=1), np.abs(res0["last_t"][rows].astype(np.float64) - w["t"][rows, kl]))
    mag = np.abs(pc["o"][rows]).max(axis=1) + np.abs(w["t"][rows, kl]) + 1
    position_last = worst(perr, pc["delta"][rows] + (kl + 4) * EPS * mag, w["ext"][rows, kl])
    # ---- every stepped callback: position, and sigma_t / sigma_maj of the ray's hero channel
    ok = ~out_all[ray] & (k <= w["valid_k"][ray]) & (k <= np.minimum(w["K"][ray], ff.MAX_STEPS))
    r_, k_ = ray[ok], k[ok] - 1
    lp, lt = resk["last_p"][ok].astype(np.float64), resk["last_t"][ok].astype(np.float64)
    perr = np.maximum(np.linalg.norm(lp - w["p"][r_, k_], axis=1), np.abs(lt - w["t"][r_, k_]))
    mag = np.abs(pc["o"][r_]).max(axis=1) + np.abs(w["t"][r_, k_]) + 1
    position = worst(perr, pc["delta"][r_] + (k_ + 4) * EPS * mag, w["ext"][r_, k_])
    sums = resk["sum"].astype(np.float64)
    prev = np.where(k > 1, np.concatenate([[0.0], sums[:-1]]), 0.0)
    Mk = w["Mk"][r_, k_]
    val, rnd = cs.ratio(lp, q["channel"][r_].astype(np.int64))
    rho = val / Mk
    ratio = worst(np.abs((sums - prev)[ok] - rho), EPS * sums[ok] + rnd / Mk + 5 * EPS * rho, np.ones(len(rho)))
    stop_violations = int(np.sum(resk["n_callbacks"] != k))
    print("%s: ties %.4f of %d rays; %d whole walks and %d callbacks compared; excess over the derived terms: tail %.2g, last collision %.2g, position %.2g, ratio %.2g; "
          "count mismatches %d, miss violations %d, stop violations %d" % (name, ties, N, int(sel.sum()), int(ok.sum()), tail, position_last, position, ratio, count_mismatches,
                                                                           miss_violations, stop_violations))
    assert ties <= ff.TIE_CAP and sel.sum() > 1000 and ok.sum() > 1000 and last.sum() > 500
    assert count_mismatches == 0 and miss_violations == 0 and stop_violations == 0
    assert tail <= BOUNDS["tail"] and position_last <= BOUNDS["position"] and position <= BOUNDS["position"] and ratio <= BOUNDS["ratio"]
