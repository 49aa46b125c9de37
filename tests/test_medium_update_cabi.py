"""vspg_renderer_update_grid / vspg_majorant_read in the C-ABI: declared in the header with what the update keeps, listed in the
package's SYMBOLS, exported, purely additive (the ABI version stays 7); and the Python wrappers refuse a wrong dtype, size or layout
with ValueError before the library is called.  Without a device no renderer can be created (there is no CPU fallback): the
wrappers are exercised on a Renderer object whose library handle raises if it is ever used; the checks on a live renderer are
tests/test_medium_update_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def header():
    return open(os.path.join(ROOT, "include", "vspg.h")).read()


def params_of(name):
    m = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, header())
    assert m, name
    return [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")]


def test_header_declares_both_functions():
    h = header()
    assert params_of("vspg_renderer_update_grid") == ["r", "which", "values", "n_floats", "memory", "stream"]
    assert params_of("vspg_majorant_read") == ["r", "host_out", "n_floats", "res", "stream"]
    for define in ("VSPG_GRID_DENSITY     0", "VSPG_GRID_TEMPERATURE 1", "VSPG_MEM_HOST   0", "VSPG_MEM_DEVICE 1"):
        assert "#define " + define in h
    assert "#define VSPG_ABI_VERSION 7" in h
    # the contract the header has to spell out: the synchronisation, what stays, the NaN clause
    doc = h[h.index("In-place update of a grid"):h.index("int vspg_renderer_update_grid")]
    for words in ("finishes parked samples and suspended paths", "synchronises `stream` before it returns", "the film", "image-space statistics",
                  "VSP buffer and its", "ready flag", "TrBuffer", "guiding fields and the training state", "counters", "reference image",
                  "error log", "vspg_film_clear", "NaN voxels are the caller's contract to avoid", "VSPG_DENSE_BRICKS is not read again"):
        assert words in " ".join(doc.replace(" * ", " ").split()), words


def test_symbols_list_them_and_the_library_exports_them(pkg):
    by_name = {name: (res, args) for name, res, args in pkg.SYMBOLS}
    res, args = by_name["vspg_renderer_update_grid"]
    assert res is C.c_int and len(args) == 6 and args[3] is C.c_size_t
    res, args = by_name["vspg_majorant_read"]
    assert res is C.c_int and len(args) == 5 and args[2] is C.c_size_t
    lib = pkg.load()
    assert hasattr(lib, "vspg_renderer_update_grid") and hasattr(lib, "vspg_majorant_read")
    assert lib.vspg_abi_version() == 7
    assert (pkg.GRID_DENSITY, pkg.GRID_TEMPERATURE, pkg.MEM_HOST, pkg.MEM_DEVICE) == (0, 1, 0, 1)
    for method in ("update_density", "update_temperature", "majorant"):
        assert hasattr(pkg.Renderer, method)


def test_null_arguments_are_refused(pkg):
    lib = pkg.load()
    v = np.zeros(8, dtype=np.float32)
    assert lib.vspg_renderer_update_grid(None, 0, v.ctypes.data, 8, 0, None) == pkg.VSPG_EINVAL
    assert b"null argument" in lib.vspg_last_error()
    assert lib.vspg_majorant_read(None, None, 0, None, None) == pkg.VSPG_EINVAL
    assert b"null argument" in lib.vspg_last_error()


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s): the wrapper must refuse first" % name)


def renderer_without_device(pkg, n=(4, 3, 2)):
    """A Renderer as __init__ leaves it, minus the device: scene, cfg, a handle nothing may be called with."""
    r = pkg.Renderer.__new__(pkg.Renderer)
    scene = pkg.VspgScene()
    scene.medium.type = pkg.MEDIUM_GRID
    scene.medium.nx, scene.medium.ny, scene.medium.nz = n
    r.scene, r.cfg, r.lib, r.h = scene, pkg.VspgRenderConfig(8, 8, 1, 0, 0, 1, 0), NoLibrary(), None
    return r


@pytest.mark.parametrize("method", ["update_density", "update_temperature"])
def test_wrappers_refuse_bad_numpy_input_before_the_library(pkg, method):
    r = renderer_without_device(pkg)
    call = getattr(r, method)
    good = np.zeros((2, 3, 4), dtype=np.float32)
    for bad, what in ((good.astype(np.float64), "float32"), (good.astype(np.int32), "float32"), (np.zeros(23, dtype=np.float32), "elements"),
                      (np.zeros(25, dtype=np.float32), "elements"), (np.zeros((2, 3, 8), dtype=np.float32)[:, :, ::2], "contiguous"),
                      (np.zeros((4, 3, 2), dtype=np.float32).transpose(2, 1, 0), "contiguous"), ([0.0] * 24, "NumPy array or a torch tensor")):
        with pytest.raises(ValueError) as e:
            call(bad)
        assert what in str(e.value), (what, str(e.value))
    with pytest.raises(AssertionError):     # a good array does reach the library
        call(good)


def test_wrappers_refuse_bad_torch_input_before_the_library(pkg):
    """dtype, size, layout and device of a tensor: a CPU tensor is not on the renderer's device (no device is needed to say so)."""
    import torch
    r = renderer_without_device(pkg)
    for bad, what in ((torch.zeros(24, dtype=torch.float64), "float32"), (torch.zeros(23, dtype=torch.float32), "elements"),
                      (torch.zeros(24, dtype=torch.float32), "device"), (torch.zeros(48, dtype=torch.float32)[::2], "device")):
        with pytest.raises(ValueError) as e:
            r.update_density(bad)
        assert what in str(e.value), (what, str(e.value))
