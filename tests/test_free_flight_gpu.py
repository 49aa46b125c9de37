"""The kernels' free flight through grid media (vspg_sample_tmaj_batch: DDA over the majorant grid, both density fetches,
SampleT_maj and SampleT_maj_Resampling) held to tests/free_flight_model.py, the float64 model of the mathematics, with the
assertions, fixtures and bounds of tests/test_free_flight_model.py -- and, on the same batches, to the oracle bit for bit, which
places a deviation from the model on one side.  One renderer and two batches per variant and test."""
import numpy as np
import pytest

import free_flight_model as ff
import oracle_lib

pytestmark = pytest.mark.gpu


def held_to_model_and_oracle(P, g, cs, what):
    c = oracle_lib.OracleRenderer(cs.scene, P.app_f_params(), 16, 16)
    try:
        for variant in (ff.PLAIN, ff.RESAMPLING):
            res0, steps = ff.run_case(g, cs, variant)
            ref0, ref_steps = ff.run_case(c, cs, variant)
            assert ff.same_results(res0, ref0) and ff.same_results(steps[2], ref_steps[2]), "%s, variant %d: device != oracle" % (what, variant)
            dev = ff.compare(cs, variant, res0, steps)
            ff.report(dev, "%s, variant %d" % (what, variant))
            ff.assert_within(dev, "%s, variant %d" % (what, variant))
            assert res0["n_callbacks"].sum() > 500
    finally:
        c.close()


def renderer(P, cs, indexed=None):
    with pytest.MonkeyPatch.context() as mp:
        if indexed is not None:
            mp.setenv("VSPG_DENSE_BRICKS", "0" if indexed else "1")
        g = P.Renderer(cs.scene, P.app_f_params(), 16, 16)
    if indexed is not None:
        assert g.brick_info()["indexed"] == int(indexed)
    return g


@pytest.mark.parametrize("layout", ["dense", "indexed"])
@pytest.mark.parametrize("name", ["grid-holes-40x33x47", "nvdb-40x33x47", "grid-23x15x8", "nvdb-23x15x8"])
def test_free_flight_vs_model(gpu_pkg, name, layout):
    """GridMedium and NanoVDB semantics in both brick layouts (the 40x33x47 densities have empty bricks to leave out)."""
    cs = ff.case(name)
    g = renderer(gpu_pkg, cs, indexed=layout == "indexed")
    try:
        bi = g.brick_info()
        if layout == "indexed" and cs.spec["holes"]:
            assert bi["n_stored"] < bi["bnx"] * bi["bny"] * bi["bnz"]
        held_to_model_and_oracle(gpu_pkg, g, cs, "%s (%s)" % (name, layout))
    finally:
        g.close()


def test_placed_medium_free_flight_vs_model(gpu_pkg):
    """The GridMedium under a rotation and a non-uniform scale: ray and sample point both go through medium_from_render."""
    cs = ff.case("placed-grid-23x15x8")
    g = renderer(gpu_pkg, cs)
    try:
        held_to_model_and_oracle(gpu_pkg, g, cs, cs.name)
    finally:
        g.close()


@pytest.mark.parametrize("name", ff.SMALLEST)
def test_smallest_grids_free_flight_vs_model(gpu_pkg, name):
    cs = ff.case(name)
    g = renderer(gpu_pkg, cs)
    try:
        held_to_model_and_oracle(gpu_pkg, g, cs, name)
    finally:
        g.close()


@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("name", ["grid-40x33x47", "nvdb-40x33x47"])
def test_updated_density_free_flight_vs_model(gpu_pkg, name, source):
    """A renderer created over density A and moved to B by update_density (vspg_renderer_update_grid), from a host array and from
    a device tensor: the walk is the model's walk through B."""
    a = ff.case(name)
    b = a.with_density(ff.contrast_density(a.spec["n"], 977, holes=not a.spec["holes"]))
    assert not np.array_equal(a.dens, b.dens) and not np.array_equal(a.med.M, b.med.M)
    g = renderer(gpu_pkg, a)
    try:
        if source == "device":
            import torch
            g.update_density(torch.from_numpy(b.dens).to(torch.device("cuda", 0)))
        else:
            g.update_density(b.dens)
        held_to_model_and_oracle(gpu_pkg, g, b, "%s updated from %s memory" % (name, source))
    finally:
        g.close()
