"""vspg_render_window in the C-ABI: exported, declared in the package's SYMBOLS, purely additive (the ABI version stays 7), and
strict about its arguments.  Without a device no renderer can be created (there is no CPU fallback), so only the null-renderer
case is reachable here; the window checks on a real renderer are tests/test_window_gpu.py::test_strict_window_arguments."""
import ctypes as C
import os
import re

from conftest import ROOT


def test_render_window_is_exported_and_declared(pkg):
    lib = pkg.load()
    assert hasattr(lib, "vspg_render_window")
    by_name = {name: (res, args) for name, res, args in pkg.SYMBOLS}
    res, args = by_name["vspg_render_window"]
    assert res is C.c_int and len(args) == 8
    header = open(os.path.join(ROOT, "include", "vspg.h")).read()
    m = re.search(r"int\s+vspg_render_window\s*\(([^)]*)\)", header)
    assert m and [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")] == ["r", "x0", "y0", "x1", "y1", "wave_start", "wave_end", "stream"]
    assert "film.cpp:97-172" in header and "integrators.cpp:111,183" in header
    assert lib.vspg_abi_version() == 7 and "#define VSPG_ABI_VERSION 7" in header
    assert hasattr(pkg.Renderer, "render_window")


def test_render_window_refuses_a_null_renderer(pkg):
    """(the window checks proper need a renderer, hence a device: tests/test_window_gpu.py::test_strict_window_arguments)"""
    lib = pkg.load()
    assert lib.vspg_render_window(None, 0, 0, 8, 8, 0, 1, None) == pkg.VSPG_EINVAL
    assert b"null renderer" in lib.vspg_last_error()
