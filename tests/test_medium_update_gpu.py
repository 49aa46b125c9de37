"""vspg_renderer_update_grid on a live renderer: every comparison is between a renderer created with values A and then updated to
B, and a renderer created fresh with B -- majorants (vspg_majorant_read; also against tests/majorant_model.py, which pins create's
host builder and the device builder k_majorant_build to the same numbers), bricks (against tests/brick_model.py, both layouts),
films, counters and replayed paths (also against the oracle created with B).  Bit patterns throughout: the feature has no tolerance.
The one freedom is the sign of a majorant that is a zero (majorant_model.same_majorants).

Films are compared with the oracle's after two waves: the oracle's film adds in double, the device's in float, and the float sum of
two floats is the correctly rounded double sum of them.

The brick layout is forced with VSPG_DENSE_BRICKS around the constructor only, as tests/test_brick_storage_gpu.py does."""
import ctypes as C

import numpy as np
import pytest

import brick_model as bm
import majorant_model as mm
import oracle_lib
import scenes

pytestmark = pytest.mark.gpu

W, H = 32, 24
NVDB_IMIN = (-7, 3, -20)
LAYOUTS = ("indexed", "dense")


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def create(P, layout, scene, prm, w, h, seed=0):
    """P.Renderer under a forced brick layout ("indexed" / "dense")."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("VSPG_DENSE_BRICKS", "0" if layout == "indexed" else "1")
        r = P.Renderer(scene, prm, w, h, seed=seed)
    assert r.brick_info()["indexed"] == (layout == "indexed")
    return r


def values(n, seed):
    """Random positives, a block of negatives, zero slabs; [nz, ny, nx] float32."""
    nx, ny, nz = n
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.05, 1.3, (nz, ny, nx)).astype(np.float32)
    z0, y0, x0 = rng.integers(0, max(nz // 2, 1)), ny // 4 + rng.integers(0, max(ny // 4, 1)), rng.integers(0, max(nx // 2, 1))
    blk = d[z0:z0 + max(nz // 3, 1), y0:y0 + max(ny // 3, 1), x0:x0 + max(nx // 3, 1)]
    blk[...] = -rng.uniform(0.1, 0.9, blk.shape).astype(np.float32)
    d[nz - max(nz // 5, 1):, :, :] = 0
    if ny > 4:
        d[:, :ny // 4, :] = 0
    return d


def nvdb_scene_of(dens, n, w=8, h=8, sa=0.1, ss=1.0, g=0.0):
    """NanoVDB semantics: a negative index_min, a non-cubic voxel, density offset 0.25, majorant scale 1.5."""
    vox = (1.5 / n[0], 1.7 / n[1], 1.3 / n[2])
    org = tuple(-0.75 - NVDB_IMIN[k] * vox[k] + (0.01, -0.1, 0.1)[k] for k in range(3))
    return scenes.nvdb_scene(dens, n, sa, ss, g=g, index_min=NVDB_IMIN, voxel=vox, origin=org, density_offset=0.25, majorant_scale=1.5, W=w, H=h)


def flat(d):
    return np.ascontiguousarray(d, dtype=np.float32).reshape(-1)


# ---------------------------------------------------------------------------------------------
# majorants: updated == fresh == model
# ---------------------------------------------------------------------------------------------
GRID_SIZES = [(1, 5, 9), (15, 15, 15), (16, 16, 16), (17, 33, 40), (112, 112, 112)]
NVDB_SIZES = [(20, 7, 33), (150, 70, 33)]


@pytest.mark.parametrize("kind,n", [("grid", n) for n in GRID_SIZES] + [("nvdb", n) for n in NVDB_SIZES])
def test_majorants_updated_equal_fresh_equal_model(gpu_pkg, kind, n):
    """k_majorant_build against create's host builder and the NumPy model.  112^3: a cell's box is 9^3 = 729 voxels, more than the
    workgroup's 256 lanes -- the strided loop and both reduction levels run; 1 x 5 x 9 and 20 x 7 x 33: boxes of fewer voxels than a
    wavefront, cells that share their box."""
    P = gpu_pkg
    a, b = flat(values(n, 1)), flat(values(n, 2))
    assert (b < 0).any() and (b == 0).any() and (b > 0).any()
    make = (lambda d: scenes.grid_scene(d, n, 0.1, 1.0, W=8, H=8)) if kind == "grid" else (lambda d: nvdb_scene_of(d, n))
    sa, sb = make(a), make(b)
    if kind == "grid" and n == (112, 112, 112):
        r = mm.ranges_grid(n)
        assert max(int((hi - lo + 1).max()) for lo, hi in r) == 9
    want_a, want_b = mm.majorant_of_scene(sa, a), mm.majorant_of_scene(sb, b)
    assert not mm.same_majorants(want_a, want_b)
    upd, fresh = P.Renderer(sa, P.app_f_params(), 8, 8), P.Renderer(sb, P.app_f_params(), 8, 8)
    res = 16 if kind == "grid" else 64
    assert upd.majorant().shape == (res, res, res)
    assert mm.same_majorants(upd.majorant(), want_a), "create's builder differs from the model"
    upd.update_density(b)
    got, ref = upd.majorant(), fresh.majorant()
    assert mm.same_majorants(ref, want_b), "create's builder differs from the model"
    bad = np.argwhere(~((got == ref) & ((u32(got) == u32(ref)) | (ref == 0))))
    assert bad.size == 0, (kind, n, "cells (z, y, x) that differ from the fresh renderer's:", bad[:8], len(bad))
    assert mm.same_majorants(got, want_b)
    if kind == "nvdb":     # negative boxes start from 0: (0 + 0.25) * 1.5 appears, and nothing lies below it
        assert got.min() == np.float32(0.375)
    elif min(n) >= 15:   # a box of negative samples has a negative majorant (the start value is a sample, not 0)
        assert (got < 0).any()
    # a third update, back to A, from a box that held other values
    upd.update_density(a)
    assert mm.same_majorants(upd.majorant(), want_a)
    upd.close(); fresh.close()


# ---------------------------------------------------------------------------------------------
# bricks: updated == fresh == model, both layouts; the indexed layout follows the new values
# ---------------------------------------------------------------------------------------------
BN = (40, 33, 47)


def assert_storage(r, dens, n, indexed, what):
    info = r.brick_info()
    index, octs = r.brick_storage()
    want_index, want_octs = bm.storage(dens, n, indexed)
    keep = bm.flags(dens, n)
    nb = int(np.prod(bm.brick_counts(n)))
    n_stored = int(keep.sum()) if indexed else nb
    assert info["indexed"] == int(indexed) and info["n_stored"] == n_stored == octs.shape[0], (what, info)
    assert info["index_bytes"] == (4 * nb if indexed else 0) and info["octet_bytes"] == max(n_stored, 1) * 512 * 32, (what, info)
    assert np.array_equal(index, want_index), what
    assert np.array_equal(u32(octs), u32(want_octs)), what
    return info, index, octs


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", ["grid", "nvdb"])
def test_bricks_updated_equal_fresh_equal_model(gpu_pkg, layout, kind):
    P = gpu_pkg
    a, b = bm.blob_density(BN, seed=11), bm.blob_density(BN, seed=12)
    b = b.copy()
    b.reshape(BN[2], BN[1], BN[0])[20:30, 10:20, 5:15] *= -1     # negative values keep their bricks
    make = (lambda d: scenes.grid_scene(d, BN, 0.1, 1.0, W=8, H=8)) if kind == "grid" else (lambda d: nvdb_scene_of(d, BN))
    upd, fresh = create(P, layout, make(a), P.app_f_params(), 8, 8), create(P, layout, make(b), P.app_f_params(), 8, 8)
    ia, _, _ = assert_storage(upd, a, BN, layout == "indexed", "created with A")
    with pytest.MonkeyPatch.context() as mp:       # the layout is the one create chose: the variable is not read again
        mp.setenv("VSPG_DENSE_BRICKS", "1" if layout == "indexed" else "0")
        upd.update_density(b)
    iu, xu, ou = assert_storage(upd, b, BN, layout == "indexed", "updated to B")
    i_f, xf, of = assert_storage(fresh, b, BN, layout == "indexed", "created with B")
    assert iu == i_f and np.array_equal(xu, xf) and np.array_equal(u32(ou), u32(of))
    if layout == "indexed":
        assert ia["n_stored"] != iu["n_stored"] and 0 < iu["n_stored"] < int(np.prod(bm.brick_counts(BN)))
    upd.close(); fresh.close()


def test_indexed_bricks_follow_the_values_through_a_sequence(gpu_pkg):
    """A -> B (bricks switch on and off) -> all zero (only the placeholder brick is left) -> B (regrows) -> the same B again
    (the count does not change: the octet buffer is kept)."""
    P = gpu_pkg
    a, b = bm.blob_density(BN, seed=11), bm.blob_density(BN, seed=12)
    ka, kb = bm.flags(a, BN), bm.flags(b, BN)
    assert (ka & ~kb).any() and (kb & ~ka).any() and ka.sum() != kb.sum()
    r = create(P, "indexed", scenes.grid_scene(a, BN, 0.1, 1.0, W=8, H=8), P.app_f_params(), 8, 8)
    zero = np.zeros_like(a)
    for dens, what, count in ((a, "A", int(ka.sum())), (b, "A -> B", int(kb.sum())), (zero, "-> zero", 0), (b, "-> B", int(kb.sum())),
                              (b, "-> B again", int(kb.sum())), (a, "-> A", int(ka.sum()))):
        if what != "A":
            r.update_density(dens)
        info, index, octs = assert_storage(r, dens, BN, True, what)
        assert info["n_stored"] == count, (what, info)
        if count == 0:
            assert info["octet_bytes"] == 512 * 32 and (index == -1).all() and octs.shape[0] == 0
        assert mm.same_majorants(r.majorant(), mm.majorant_grid(dens, BN)), what
    r.close()


# ---------------------------------------------------------------------------------------------
# films and replayed paths: updated == fresh == oracle, on every kernel family
# ---------------------------------------------------------------------------------------------
RN = (23, 15, 18)


def render_values(seed):
    """What a render can use: values in (0.05, 1.3] inside a few balls (radius 0.25 .. 0.4 of the shortest side), exact zeros
    elsewhere -- empty bricks, seams between stored and dropped ones; flat, x fastest."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = RN
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    mask = np.zeros((nz, ny, nx), dtype=bool)
    for _ in range(3):
        c = rng.uniform(0.1, 0.9, 3) * np.array([nx, ny, nz])
        r = rng.uniform(0.25, 0.4) * min(RN)
        mask |= (x + 0.5 - c[0]) ** 2 + (y + 0.5 - c[1]) ** 2 + (z + 0.5 - c[2]) ** 2 <= r * r
    v = rng.uniform(0.05, 1.3, (nz, ny, nx)).astype(np.float32)
    return np.ascontiguousarray(np.where(mask, v, np.float32(0)).reshape(-1))


def temperature_values(dens, seed):
    rng = np.random.default_rng(seed)
    return (150.0 + 2600.0 * np.clip(dens + 0.3 * rng.random(dens.size).astype(np.float32), 0, 1.4)).astype(np.float32)


def with_temperature(scene, temp):
    scene.medium.temperature = temp.ctypes.data_as(C.POINTER(C.c_float))
    scene.medium.temperature_offset, scene.medium.temperature_scale, scene.medium.nvdb_le_scale = 120.0, 1.3, 0.6
    scene._temp_keepalive = temp
    return scene


def film_scene(P, shape, dens, temp=None):
    if shape == "grid":
        return scenes.grid_scene(dens, RN, (0.05, 0.08, 0.1), (3.0, 2.6, 2.2), g=0.5, bmin=(-0.8, -0.8, -0.5), bmax=(0.8, 0.7, 0.9), W=W, H=H)
    if shape == "nvdb":
        s = nvdb_scene_of(dens, RN, W, H, sa=(0.05, 0.08, 0.1), ss=(3.0, 2.6, 2.2), g=0.5)
        return with_temperature(s, temp) if temp is not None else s
    assert shape == "cloud"
    s = scenes.cloud_scene(W, H, dens, RN[0])
    s.medium.nx, s.medium.ny, s.medium.nz = RN
    return s


#        name           scene    options   VSPG_KERNEL  kernel expected
FILM_CASES = [("default",     "grid",  "app-f",  None,   "k_wf_dist_walk<GridMedium>"),
              ("nds",         "grid",  "nds",    None,   "k_wf_segment_vertex<GridMedium>"),
              ("lane",        "grid",  "app-f",  "lane", "k_render_wave<GridMedium>"),
              ("wg",          "grid",  "app-f",  "wg",   "k_render_wave_wg<GridMedium>"),
              ("boundary",    "cloud", "app-f",  None,   "k_wf_walk<GridMediumGrey>"),
              ("nvdb",        "nvdb",  "app-f",  None,   "k_wf_dist_walk<NanoDenseMedium>"),
              ("temperature", "nvdb",  "nds",    None,   "k_wf_segment_vertex<NanoDenseMedium>")]


@pytest.mark.parametrize("case", [c[0] for c in FILM_CASES])
def test_film_and_paths_updated_equal_fresh_equal_oracle(gpu_pkg, case):
    P = gpu_pkg
    _, shape, options, kernel, expect = next(c for c in FILM_CASES if c[0] == case)
    a, b = render_values(31), render_values(32)
    ta = tb = None
    if case == "temperature":
        ta, tb = temperature_values(a, 1), temperature_values(b, 2)
    prm = P.app_f_params()
    if options == "nds":
        prm.vspsamplingmethod = P.VSP_NDS
    sa, sb = film_scene(P, shape, a, ta), film_scene(P, shape, b, tb)
    rng = np.random.default_rng(9)
    pix = np.stack([rng.integers(0, W, 200), rng.integers(0, H, 200)], axis=1).astype(np.int32)
    si = rng.integers(0, 4096, 200).astype(np.int32)
    with pytest.MonkeyPatch.context() as mp:     # the kernel is chosen per launch: the variable stays set while rendering
        if kernel:
            mp.setenv("VSPG_KERNEL", kernel)
        else:
            mp.delenv("VSPG_KERNEL", raising=False)
        upd, fresh = P.Renderer(sa, prm, W, H, seed=14), P.Renderer(sb, prm, W, H, seed=14)
        name = upd.kernel_name()
        assert name == expect == fresh.kernel_name()
        upd.update_density(b)
        if tb is not None:
            upd.update_temperature(tb)
        assert upd.kernel_name() == name
        out = []
        for g in (upd, fresh):
            for w in range(2):
                g.render_wave(w, w + 1)
                g.post_process_wave()
            out.append((g.film(), g.counters(), g.trace_paths(pix, si), g.vsp_buffer()))
        assert upd.kernel_name() == name
        upd.close(); fresh.close()
    c = oracle_lib.OracleRenderer(sb, prm, W, H, seed=14)
    for w in range(2):
        c.render_wave(w, w + 1)
        c.post_process_wave()
    ref = (c.film(), c.counters(), c.trace_paths(pix, si))
    (fu, cu, (lu, su), vu), (ff, cf, (lf, sf), vf) = out
    assert np.array_equal(u32(fu), u32(ff)), (case, "film: updated vs fresh", int((u32(fu) != u32(ff)).any(axis=-1).sum()))
    assert cu == cf and np.array_equal(su, sf) and np.array_equal(u32(lu), u32(lf))
    assert np.array_equal(u32(vu[0]), u32(vf[0])) and vu[1] == vf[1]
    assert np.array_equal(u32(fu), u32(ref[0])), (case, "film: updated vs oracle", int((u32(fu) != u32(ref[0])).any(axis=-1).sum()))
    assert cu == ref[1]
    assert np.array_equal(su, ref[2][1]) and np.array_equal(u32(lu), u32(ref[2][0]))
    assert fu[..., :3].max() > 0 and cu["density_queries"] > 0 and su.max() >= 3
    # the update mattered: the film of A is another film
    c.close()
    ca = oracle_lib.OracleRenderer(sa, prm, W, H, seed=14)
    ca.render_wave(0, 1)
    cb = oracle_lib.OracleRenderer(sb, prm, W, H, seed=14)
    cb.render_wave(0, 1)
    assert not np.array_equal(u32(ca.film()), u32(cb.film()))
    ca.close(); cb.close()


# ---------------------------------------------------------------------------------------------
# sources: a device tensor gives what the host array gives
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["grid", "nvdb"])
def test_device_tensor_equals_host_array(gpu_pkg, kind):
    """A torch tensor on the renderer's device, whole and as a view into a larger allocation (its pointer is no allocation base and
    only 4-byte aligned): bricks, majorants and film of the NumPy path.  A tensor written on torch's current stream just before the
    call is read behind that write."""
    import torch
    P = gpu_pkg
    a, b = render_values(31), render_values(32)
    tb = temperature_values(b, 2) if kind == "nvdb" else None
    ta = temperature_values(a, 1) if kind == "nvdb" else None
    prm = P.app_f_params()
    if kind == "nvdb":
        prm.vspsamplingmethod = P.VSP_NDS
    shape = "grid" if kind == "grid" else "nvdb"
    dev = torch.device("cuda", 0)
    whole = torch.from_numpy(b).to(dev)
    big = torch.zeros(b.size + 77, dtype=torch.float32, device=dev)
    view = big[13:13 + b.size]
    view.copy_(whole)                     # (on the current stream, which the update then uses)
    assert view.data_ptr() == big.data_ptr() + 52 and view.is_contiguous()
    results = []
    for src in (b, whole, view):
        r = create(P, "indexed", film_scene(P, shape, a, ta), prm, W, H, seed=5)
        r.update_density(src)
        if tb is not None:
            r.update_temperature(tb if isinstance(src, np.ndarray) else torch.from_numpy(tb).to(dev))
        info, (index, octs), maj = r.brick_info(), r.brick_storage(), r.majorant()
        for w in range(2):
            r.render_wave(w, w + 1)
            r.post_process_wave()
        results.append((info, index, octs, maj, r.film(), r.counters()))
        r.close()
    assert torch.equal(whole.cpu(), torch.from_numpy(b)) and torch.equal(view.cpu(), torch.from_numpy(b))   # the source is only read
    i0, x0, o0, m0, f0, c0 = results[0]
    assert mm.same_majorants(m0, mm.majorant_of_scene(film_scene(P, shape, b, tb), b)) and f0[..., :3].max() > 0
    for info, index, octs, maj, film, counters in results[1:]:
        assert info == i0 and np.array_equal(index, x0) and np.array_equal(u32(octs), u32(o0))
        assert np.array_equal(u32(maj), u32(m0))
        assert np.array_equal(u32(film), u32(f0)) and counters == c0
    # what the wrapper refuses on a live renderer: a tensor of another dtype, size or layout -- the grid stays
    r = create(P, "indexed", film_scene(P, shape, a, ta), prm, W, H, seed=5)
    before = r.majorant()
    for bad in (whole.double(), whole[:-1], big[0:2 * b.size:2], whole.cpu()):
        with pytest.raises(ValueError):
            r.update_density(bad)
    assert np.array_equal(u32(r.majorant()), u32(before))
    r.close()


# ---------------------------------------------------------------------------------------------
# what persists
# ---------------------------------------------------------------------------------------------
def field_bytes(r):
    out = []
    for volume in (0, 1):
        nodes, regs, nn, nr = r.get_guiding_field(volume)
        out.append((nn, nr, bytes(nodes), bytes(regs)))
    return out


def test_update_keeps_film_counters_fields_and_vsp_buffer(gpu_pkg):
    """A guided renderer with an uploaded field and a loaded VSP buffer, one wave rendered: film, counters, both guiding fields, the
    training state and the VSP buffer read the same bytes before and after an update -- and the update is in force afterwards."""
    P = gpu_pkg
    a, b = render_values(31), render_values(32)
    prm = P.default_params()
    r = P.Renderer(film_scene(P, "grid", a), prm, W, H, seed=3)
    field = scenes.light_field(P, n=4)
    r.set_guiding_field(field, field)
    vsp = np.random.default_rng(4).uniform(0.1, 0.9, (H, W)).astype(np.float32)
    r.load_vsp_buffer(vsp)
    r.render_wave(0, 1)

    def state():
        return r.film(), r.counters(), field_bytes(r), r.vsp_buffer(), r.training_stats()

    f0, c0, g0, (v0, ready0), t0 = state()
    assert f0[..., :3].max() > 0 and c0["paths"] > 0 and g0[0][0] > 1 and ready0 and np.array_equal(v0, vsp)
    r.update_density(b)
    f1, c1, g1, (v1, ready1), t1 = state()
    assert np.array_equal(u32(f0), u32(f1)) and c0 == c1 and g0 == g1 and t0 == t1
    assert ready1 == ready0 and np.array_equal(u32(v0), u32(v1))
    assert mm.same_majorants(r.majorant(), mm.majorant_grid(b, RN))
    assert_storage(r, b, RN, bool(r.brick_info()["indexed"]), "after the update")
    r.close()


@pytest.mark.parametrize("kernel", [None, "wg"])
def test_samples_in_flight_end_under_the_old_values(gpu_pkg, kernel):
    """A wave rendered and NOT read before the update (samples a launch parked, paths it suspended: the update finishes them first):
    the film afterwards is the film of a twin that never updated."""
    P = gpu_pkg
    a, b = render_values(31), render_values(32)
    prm = P.app_f_params()
    with pytest.MonkeyPatch.context() as mp:
        if kernel:
            mp.setenv("VSPG_KERNEL", kernel)
        else:
            mp.delenv("VSPG_KERNEL", raising=False)
        r, twin = (P.Renderer(film_scene(P, "grid", a), prm, W, H, seed=3) for _ in range(2))
        for g in (r, twin):
            g.render_wave(0, 1)
        r.update_density(b)
        assert np.array_equal(u32(r.film()), u32(twin.film())) and r.counters() == twin.counters()
        r.close(); twin.close()


# ---------------------------------------------------------------------------------------------
# refusals leave the renderer as it was
# ---------------------------------------------------------------------------------------------
def test_refusals_change_nothing(gpu_pkg):
    P = gpu_pkg
    lib = P.load()
    a, b = render_values(31), render_values(32)
    prm = P.app_f_params()
    n = a.size
    r, twin = (create(P, "indexed", film_scene(P, "grid", a), prm, W, H, seed=3) for _ in range(2))
    for g in (r, twin):
        g.render_wave(0, 1)               # (not read: whatever the launch parked stays parked through the refusals)
    maj0, info0, (index0, octs0) = twin.majorant(), twin.brick_info(), twin.brick_storage()
    bp = b.ctypes.data
    refused = [("null renderer", (None, P.GRID_DENSITY, bp, n, P.MEM_HOST, None)),
               ("null values", (r.h, P.GRID_DENSITY, None, n, P.MEM_HOST, None)),
               ("which", (r.h, 2, bp, n, P.MEM_HOST, None)),
               ("which", (r.h, -1, bp, n, P.MEM_HOST, None)),
               ("memory", (r.h, P.GRID_DENSITY, bp, n, 2, None)),
               ("memory", (r.h, P.GRID_DENSITY, bp, n, -1, None)),
               ("n_floats", (r.h, P.GRID_DENSITY, bp, n - 1, P.MEM_HOST, None)),
               ("n_floats", (r.h, P.GRID_DENSITY, bp, n + 1, P.MEM_HOST, None)),
               ("n_floats", (r.h, P.GRID_DENSITY, bp, 0, P.MEM_HOST, None)),
               ("no temperature grid", (r.h, P.GRID_TEMPERATURE, bp, n, P.MEM_HOST, None)),
               ("no temperature grid", (r.h, P.GRID_TEMPERATURE, bp, n, P.MEM_DEVICE, None))]
    for what, args in refused:
        assert lib.vspg_renderer_update_grid(*args) == P.VSPG_EINVAL, what
        assert lib.vspg_last_error(), what
    with pytest.raises(P.VspgError) as e:
        r.update_temperature(b)
    assert e.value.code == P.VSPG_EINVAL and "temperature" in str(e.value)
    out = np.empty(16 ** 3 + 1, dtype=np.float32)
    res = C.c_int32(0)
    fp = out.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.vspg_majorant_read(r.h, fp, 16 ** 3 + 1, C.byref(res), None) == P.VSPG_EINVAL and res.value == 16
    assert lib.vspg_majorant_read(r.h, fp, 64 ** 3, None, None) == P.VSPG_EINVAL
    assert lib.vspg_majorant_read(r.h, None, 16 ** 3, None, None) == P.VSPG_EINVAL
    # majorants, bricks, film; and the next render is the render without the refused calls
    assert np.array_equal(u32(r.majorant()), u32(maj0)) and r.brick_info() == info0
    index, octs = r.brick_storage()
    assert np.array_equal(index, index0) and np.array_equal(u32(octs), u32(octs0))
    for g in (r, twin):
        g.post_process_wave()
        g.render_wave(1, 2)
    assert np.array_equal(u32(r.film()), u32(twin.film())) and r.counters() == twin.counters()
    assert twin.film()[..., :3].max() > 0
    r.close(); twin.close()


def test_other_media_refuse_both_calls(gpu_pkg):
    P = gpu_pkg
    lib = P.load()
    r = P.Renderer(P.fog_box_scene(16, 16), P.app_f_params(), 16, 16)
    v = np.zeros(8, dtype=np.float32)
    for which in (P.GRID_DENSITY, P.GRID_TEMPERATURE):
        for n in (8, 0):
            assert lib.vspg_renderer_update_grid(r.h, which, v.ctypes.data, n, P.MEM_HOST, None) == P.VSPG_EINVAL
            assert b"grid medium" in lib.vspg_last_error()
    with pytest.raises(P.VspgError) as e:
        r.majorant()
    assert e.value.code == P.VSPG_EINVAL and "grid medium" in str(e.value)
    r.render_wave(0, 1)
    assert r.film()[..., :3].max() > 0
    r.close()
