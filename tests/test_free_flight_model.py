"""The oracle's free flight through grid media (DDA over the majorant grid, SampledGrid::Lookup and NanoVDB-semantics density,
SampleT_maj, SampleT_maj_Resampling) held to tests/free_flight_model.py, a float64 model written from the mathematics: the first
check of this layer that does not pass through the oracle's restatement of the reference's code.

Per fixture (free_flight_model.CASES) and variant, the batch driver's recording callback gives, deterministically, the majorant
optical depth of the ray (through majorant_scale and vrc), the k-th tentative collision's point and parameter, the density over
majorant there, the number of collisions and the tail transmittance; the model predicts each.  Every check reads
error <= derived float32 term + C * unit (free_flight_model.compare lists the terms).

Measured here, oracle against model, over all 12 fixtures and both variants (2160 rays each, 79 771 callbacks compared):
  * the error alone, in the check's unit: position 8.5e-3 of the cell's extent (the 64^3 lattice of NanoVDB semantics: cells a
    quarter the size, and the float32 crossing parameters, up to ~3e-6 off, are where the collisions of a piece start from), ratio
    4.3e-6 (the float32 array coordinate, up to 52, times the interpolant's slope), tau 5.8e-4 and scale 6.8e-3 relative (rays that
    clip a corner of the box or run through empty cells: tau itself is 1e-3 and less), vrc 7.8e-4, tail 7.6e-3 relative, on_ray
    1.71 units of 2^-24 (|o| + t + 1);
  * against the derived float32 terms the error stays inside them for every kind: largest share used position 0.94, vrc 0.98,
    tail 0.85, ratio 0.62, tau 0.32, scale 0.20 (on_ray has none).
  Eight times a measured excess of 0 is 0, so the constants C are floors (free_flight_model.BOUNDS): position 1e-4 of the cell's
  extent (the condition is <= 1e-3), ratio 1e-6 (<= 1e-5), tau and scale 1e-6 relative, vrc and tail 1e-5 relative; on_ray 14
  (8 x 1.71).  The kernels give the oracle's bits (tests/test_free_flight_gpu.py asserts it), hence the same figures.
  * ties: at most 0.0037 of a fixture's rays (cap 0.01), 62 rays of 51 840 in all.

One departure of the reference from the mathematics was found; it is excluded by rule.  Its float32 DDA
places a crossing up to ~3e-6 off in t (the lattice coordinate of the entry point, rounded, divided by the direction's slowest
component; then one rounding per step).  That is more than 1e-4 of a short piece -- a 64^3 lattice has pieces of 1e-3 and less --
so the rule "a draw within 1e-4 of its piece's length from the piece's end is a tie" does not cover it.  A draw closer to its
piece's end than that uncertainty (pieces()["delta"], derived from the DDA's operations, 2e-6 .. 1e-5 here) is a tie as well;
both kinds count under the cap.  Without the second rule one ray of the 51 840 has another count than the model's
(nvdb-40x33x47, resampling: a draw 2.5e-6 before the end of a piece 0.015 long).

The planted errors are wrong MODELS (flags of the model's functions): with each of them the same assertions fail on every fixture
with more than one majorant cell."""
import numpy as np
import pytest

import brick_model
import free_flight_model as ff
import oracle_lib
from conftest import load_package

fh = float.fromhex
_runs = {}


def runs(name, variant):
    """The oracle's two batches of a case, run once."""
    if (name, variant) not in _runs:
        cs = ff.case(name)
        r = oracle_lib.OracleRenderer(cs.scene, oracle_lib.app_f_params(), 16, 16)
        _runs[name, variant] = ff.run_case(r, cs, variant)
        r.close()
    return _runs[name, variant]


@pytest.mark.parametrize("name", sorted(ff.CASES))
def test_fixture_is_what_the_walk_needs(name):
    cs = ff.case(name)
    med, q = cs.med, cs.q
    w = cs.walk(ff.RESAMPLING)
    pc = w["pc"]
    N = len(q)
    assert N == ff.N_GENERIC + ff.N_ZERO
    # directions: every octant, no ill-conditioned component, |d| in [0.5, 2]
    dm = med.to_medium(pc["dhat"], vector=True)
    dm /= np.linalg.norm(dm, axis=1)[:, None]
    nz = dm != 0
    assert np.abs(dm[nz]).min() >= ff.MIN_COMPONENT
    gen = np.all(nz, axis=1)
    octant = ((dm[gen] > 0) * np.array([1, 2, 4])).sum(axis=1)
    assert np.bincount(octant, minlength=8).min() >= 200
    dl = np.linalg.norm(q["d"].astype(np.float64), axis=1)
    assert dl.min() >= 0.5 - 1e-6 and dl.max() <= 2 + 1e-6 and dl.std() > 0.3
    # exact zeros of both signs, the origin strictly inside a cell on those axes
    if cs.spec["kind"] != "placed":
        zero = ~gen
        assert zero.sum() == ff.N_ZERO
        comp = q["d"][zero]
        is0 = comp == 0
        assert set(is0.sum(axis=1)) == {1, 2}
        assert (np.signbit(comp) & is0).any() and (~np.signbit(comp) & is0).any()
        frac = pc["go"][zero] % 1.0
        assert frac[is0].min() >= 0.2 and frac[is0].max() <= 0.8
        assert w["hit"][zero].mean() > 0.3
    # origins inside and outside, misses, rays that end inside the box
    go = pc["go"]
    inside = np.all((go > 0) & (go < med.MR), axis=1)
    assert 0.25 < inside.mean() < 0.75
    assert (~w["hit"]).sum() >= 100 and (w["hit"] & ~inside).sum() >= 400
    dlen = np.linalg.norm(q["d"].astype(np.float64), axis=1)
    ends_inside = w["hit"] & (np.abs(pc["t1"] - q["tMax"] * dlen) < 1e-5)
    assert ends_inside.sum() >= 300
    # vsp groups, channels
    top = q["vsp"] == np.float32(0.999)
    mid = (q["vsp"] > 0) & ~top
    assert (q["vsp"] < 0).sum() == top.sum() == mid.sum() == N // 3
    assert q["vsp"][mid].min() >= 0.05 and q["vsp"][mid].max() <= 0.6
    assert w["tau"][top].max() < 6 < -np.log1p(-np.float64(np.float32(0.999)))
    live = mid & (w["tau"] > 0)
    assert (w["scale"][live] > 1).sum() >= 50 and (w["scale"][live] == 1).sum() >= 50      # both sides of the branch
    for g in (q["vsp"] < 0, top, mid):
        assert np.bincount(q["channel"][g], minlength=3).min() >= N // 12
    assert len(set(med.sigma_t)) == 3
    # the lattice: contrast between neighbouring cells, empty cells where promised
    # (A majorant is a maximum over a box wider than its cell, so neighbouring cells mostly share it and a step between them
    # sits only where a block of the density ends: what counts is that the rays cross such steps.)
    M = med.M
    if np.ptp(M) > 0:
        near = np.zeros(M.shape, dtype=bool)
        for axis in range(3):
            a, h = np.moveaxis(M, axis, 0), np.moveaxis(near, axis, 0)
            c = (a[:-1] != a[1:]) & (np.maximum(a[:-1], a[1:]) >= 2 * np.minimum(a[:-1], a[1:]))
            h[:-1] |= c
            h[1:] |= c
        a, b = pc["M"][:, :-1], pc["M"][:, 1:]
        step = (np.arange(1, pc["M"].shape[1])[None, :] < w["nseg"][:, None]) & (a != b) & (np.maximum(a, b) >= 2 * np.minimum(a, b))
        several = w["nseg"] >= 4
        share = step.any(axis=1)[several].mean()
        print("%s: %.2f of the majorant cells have a neighbour 2x off; %.2f of the rays with 4 pieces or more cross such a step" % (name, near.mean(), share))
        assert share >= (0.3 if max(med.n) >= 7 else 0.1)
    if cs.spec["holes"]:
        # whole majorant cells without density: majorant 0 (the branch that draws no u) -- under NanoVDB semantics the
        # density_offset alone, which keeps that branch to the GridMedium fixture
        floor = np.float32(ff.NVDB_OFFSET) * np.float32(ff.NVDB_SCALE) if med.nvdb else 0.0
        empty = (pc["M"] == floor) & (np.arange(pc["M"].shape[1])[None, :] < w["nseg"][:, None])
        assert (M == floor).mean() > 0.05 and (empty.any(axis=1) & (w["tau"] > 0)).sum() >= 200
    # bounds: not a cube, not centred
    ext = med.bmax - med.bmin
    assert len(set(np.round(ext, 3))) == 3 and np.abs(med.bmax + med.bmin).min() > 0.04
    if med.nvdb:
        assert np.all(med.index_min != 0) and len(set(np.round(med.voxel, 5))) == 3 and med.offset != 0
        assert cs.scene.medium.majorant_scale != 1


@pytest.mark.parametrize("variant", [ff.PLAIN, ff.RESAMPLING])
@pytest.mark.parametrize("name", sorted(ff.CASES))
def test_oracle_free_flight_vs_model(name, variant):
    cs = ff.case(name)
    res0, steps = runs(name, variant)
    dev = ff.compare(cs, variant, res0, steps)
    what = "oracle, %s, variant %d" % (name, variant)
    ff.report(dev, what)
    ff.assert_within(dev, what)
    assert res0["n_callbacks"].sum() > 500


def _applies(error, cs):
    kind = cs.spec["kind"]
    if error in ("roll_majorants", "flip_step"):
        return np.ptp(cs.med.M) > 0                      # more than one majorant cell
    if error == "no_half":
        return kind in ("grid", "placed")
    if error == "no_index_min":
        return kind == "nvdb"
    if error == "no_point_transform":
        return kind == "placed"
    return True


@pytest.mark.parametrize("error", ff.PLANTED)
def test_planted_error_fails_the_comparison(error):
    """The same assertions against a deliberately wrong model: they fail on every fixture the error can show on."""
    seen = 0
    for name in sorted(ff.CASES):
        cs = ff.case(name)
        if not _applies(error, cs):
            continue
        res0, steps = runs(name, ff.RESAMPLING)
        dev = ff.compare(cs, ff.RESAMPLING, res0, steps, planted=(error,))
        with pytest.raises(AssertionError, match="departs from the model"):
            ff.assert_within(dev, name)
        seen += 1
    assert seen >= (1 if error == "no_point_transform" else 5)


@pytest.mark.parametrize("name", ["grid-23x15x8", "grid-40x33x47", "nvdb-23x15x8", "nvdb-40x33x47", "grid-1x1x1", "nvdb-2x3x5"])
def test_model_density_vs_float32_lookups(name):
    """The model's densities, written from the definitions, against tests/brick_model.py's float32 lerp_grid / lerp_index (the
    arithmetic of the device's fetches) at random points in and around the box: equal to float32 rounding (density_rounding)."""
    cs = ff.case(name)
    med = cs.med
    rng = np.random.default_rng(3)
    ext = med.bmax - med.bmin
    p = rng.uniform(med.bmin - 0.1 * ext, med.bmax + 0.1 * ext, (4000, 3)).astype(np.float32)
    read = lambda ix, iy, iz: brick_model.raw_octet(cs.dens, med.n, ix, iy, iz)
    if med.nvdb:
        f = np.float32
        inv = [f(1) / f(v) for v in med.voxel]
        x = np.stack([(p[:, k] - f(med.origin[k])) * inv[k] for k in range(3)], axis=1)
        got = brick_model.lerp_index(x, [int(v) for v in med.index_min], read) + f(med.offset)
    else:
        f = np.float32
        po = np.stack([(p[:, k] - f(med.bmin[k])) / (f(med.bmax[k]) - f(med.bmin[k])) for k in range(3)], axis=1)
        got = brick_model.lerp_grid(po, med.n, read)
    want = ff.density(med, p)
    assert (want > 0).mean() > 0.5
    assert np.all(np.abs(got - want) <= ff.density_rounding(med, p) + 2 * ff.EPS * np.abs(want))


def test_model_reproduces_the_references_recorded_outputs():
    """SURVEY.md App. D.3 (the reference's own outputs on the 8^3 grid of RNG(7)), from the model, within the bounds above."""
    from scenes import d3_density, grid_scene
    dens = d3_density()
    scene = grid_scene(dens, (8, 8, 8), 0.5, 4.5)
    med = ff.Medium(scene, dens)
    q = np.zeros(1, dtype=ff.QUERY_DTYPE)
    q["o"], q["d"], q["tMax"], q["u"], q["rng_a"], q["rng_b"], q["vsp"], q["channel"] = (0.1, 0.2, -0.5), (0.3, 0.2, 1.0), 2.0, 0.37, 0.25, 0.75, 0.6, 1
    w = ff.walk(med, q, ff.RESAMPLING)
    assert w["K"][0] == 8 and not w["tied"][0] and w["scale"][0] == 1.0
    rho = w["rho"][0, :8]
    rounding = (ff.density_rounding(med, w["p"][0, :8]) / w["Mk"][0, :8]).sum() + w["pc"]["delta"][0] * 8 * 8    # slope <= n = 8 per unit box
    assert abs(rho.sum() - fh("0x1.dd496p+1")) <= 8 * ff.EPS * rho.sum() + rounding + 8 * ff.BOUNDS["ratio"]
    tail_tol = ff.fast_exp_error() * w["tail_pieces"][0] + 5.0 * w["pc"]["delta"][0] * w["pc"]["variation"][0] + ff.BOUNDS["tail"]
    assert abs(fh("0x1.8f239ep-2") / w["tail"][0, 1] - 1) <= tail_tol
    T = w["tau"][0]
    amp = np.exp(-T) / -np.expm1(-T)
    assert abs(fh("0x1.356952p-1") / w["vrc"][0] - 1) <= amp * (ff.fast_exp_error() + (w["nseg"][0] + 3) * ff.EPS * T + 5.0 * w["pc"]["delta"][0] * w["pc"]["variation"][0]) + ff.BOUNDS["vrc"]
    q["vsp"] = -1.0
    w = ff.walk(med, q, ff.PLAIN)
    assert w["K"][0] >= 3 and w["valid_k"][0] >= 3
    assert abs(w["p"][0, 2, 2] - fh("0x1.717118p-2")) <= w["pc"]["delta"][0] + 7 * ff.EPS * 3 + ff.BOUNDS["position"] * w["ext"][0, 2]


def test_model_constant_density_closed_form():
    """A constant density c: tau_maj = sigma_t * c * (t1 - t0) and the tail of a walk without a collision exp(-scale * tau) per
    channel, the chord worked out by hand -- along an axis the box's width, and from one corner to the opposite one its diagonal."""
    from scenes import grid_scene
    c = 0.625
    n = (5, 4, 6)
    dens = np.full(5 * 4 * 6, c, dtype=np.float32)
    scene = grid_scene(dens, n, (0.25, 0.5, 0.75), (1.0, 1.0, 1.0), bmin=(-0.5, -0.25, 0.0), bmax=(1.0, 0.5, 2.0))
    med = ff.Medium(scene, dens)
    q = np.zeros(3, dtype=ff.QUERY_DTYPE)
    q["o"] = [(-2.0, 0.1, 0.7), (0.3, 0.2, 0.5), (-0.5, -0.25, 0.0)]
    q["d"] = [(2.0, 0.0, 0.0), (0.0, -0.0, -0.5), (1.5, 0.75, 2.0)]
    q["tMax"], q["u"], q["rng_a"], q["rng_b"], q["vsp"] = 100.0, 0.5, 0.1, 0.2, 0.5
    q["channel"] = (0, 1, 2)
    chord = np.array([1.5, 0.5, np.sqrt(1.5 ** 2 + 0.75 ** 2 + 2.0 ** 2)])
    for variant in (ff.PLAIN, ff.RESAMPLING):
        w = ff.walk(med, q, variant)
        assert np.allclose(w["tau"], med.sigma_t * c * chord, rtol=1e-12)
        behind = chord - (np.where(w["K"] > 0, w["t"][np.arange(3), np.minimum(w["K"], ff.MAX_STEPS) - 1], w["pc"]["t0"]) - w["pc"]["t0"])
        assert w["K"].max() <= ff.MAX_STEPS
        assert np.allclose(w["tail"], np.exp(-np.outer(c * behind * w["scale"], med.sigma_t)), rtol=1e-12)
