"""The RGB grid update (vspg_renderer_update_rgb_grids) without a device: the NumPy model of the octet image
(tests/rgbgrid_update_model.py) against create's host builder build_rgb_octets, run as a stand-alone program under sanitizers together
with the value check factored out of validate_rgb_grid; the C-ABI additions (exported, declared, refusing a null renderer, the header
still C, the records' sizes unchanged); the wrapper's refusals."""
import ctypes as C
import os
import shlex
import subprocess

import numpy as np
import pytest

import rgbgrid_update_model as U

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vspg-pbrt-v4_amd", "csrc")
# nx, ny, nz: exactly one brick; two bricks per axis, the second holding one layer; 9; a third brick of one layer; degenerate; unequal counts
SIZES = [(7, 7, 7), (8, 8, 8), (9, 9, 9), (16, 16, 16), (1, 5, 9), (17, 33, 40)]


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the model itself: hand-derived answers ----------------------------------------------------------------------------------------------
def test_octet_model_known_answers():
    """The 2 x 1 x 1 grid of tests/rgbgrid_build_check.cpp: one brick; base voxel (ix, iy, iz) at octet (ix + 1, iy + 1, iz + 1)."""
    a = np.array([[[[1, 5, 2], [3, 0, 4]]]], f32)
    img = U.octets32(a, (2, 1, 1))
    assert img.shape == (1, 1, 1, 8, 8, 8, 8, 4)
    o = img[0, 0, 0]
    assert o[1, 1, 1, 0].tolist() == [1, 5, 2, 0] and o[1, 1, 1, 1].tolist() == [3, 0, 4, 0] and not o[1, 1, 1, 2:].any()
    assert o[0, 0, 0, 7].tolist() == [1, 5, 2, 0] and not o[0, 0, 0, :7].any()          # base voxel (-1, -1, -1): only corner 7
    assert o[0, 1, 2, 4].tolist() == [3, 0, 4, 0] and not o[0, 1, 2, 5].any()           # base voxel (1, 0, -1): only corner 4 = voxel (1, 0, 0)
    assert not o[2:].any() and not o[:, 2:].any() and not o[:, :, 3:].any()             # octets behind o = n
    assert img.sum() == 8 * (1 + 5 + 2 + 3 + 0 + 4) and not img[..., 3].any()           # every voxel in exactly eight octets; .w = 0
    assert U.brick_counts((7, 7, 7)) == (1, 1, 1) and U.brick_counts((8, 8, 8)) == (2, 2, 2) and U.brick_counts((17, 33, 40)) == (3, 5, 6)


def test_special_values_have_what_the_gpu_tests_need():
    for n in SIZES:
        a, b = U.special_values(n, 1), U.special_values(n, 2)
        assert a.shape == (n[2], n[1], n[0], 3) and a.dtype == f32 and (a >= 0).all() and np.isfinite(a).all()
        assert a.max() == f32(37.5) and b.max() == f32(41.25) and (a == 0).any()
        assert not np.array_equal(U.octets32(a, n), U.octets32(b, n))


# ---- the host builder and the value check under sanitizers: a stand-alone program ---------------------------------------------------------
def test_host_builder_equals_the_model_and_value_check_under_sanitizers(tmp_path):
    """tests/rgbgrid_update_check.cpp with the two host-only units, compiled with the library's flags plus AddressSanitizer and
    UndefinedBehaviorSanitizer on the host side, linked without the HIP runtime and run directly (as tests/test_rgbgrid_model.py does)."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    hipcc, clangxx = os.path.join(rocm, "bin", "hipcc"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")
    for tool in (hipcc, clangxx):
        if not os.path.exists(tool):
            pytest.fail("%s not found (ROCm)" % tool)
    flags = shlex.split(subprocess.check_output(["make", "-s", "--no-print-directory", "-C", CSRC, "print-HIPFLAGS"], text=True))
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    host = [a for s in sanitize for a in ("-Xarch_host", s)]
    jobs = [(os.path.join(CSRC, u + ".hip"), []) for u in ("vspg_scene_build", "vspg_scene_api")] + \
           [(os.path.join(ROOT, "tests", "rgbgrid_update_check.cpp"), ["-x", "hip", "-I", CSRC])]
    procs, objs = [], []
    for src, extra in jobs:
        obj = str(tmp_path / (os.path.splitext(os.path.basename(src))[0] + ".o"))
        objs.append(obj)
        cmd = [hipcc] + flags + host + ["-g"] + extra + ["-c", "-o", obj, src]
        procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for cmd, p in procs:
        out = p.communicate()[0]
        assert p.returncode == 0, "%s\n%s" % (" ".join(cmd), out)
    exe = str(tmp_path / "rgbgrid_update_check")
    subprocess.check_call([clangxx] + sanitize + ["-o", exe] + objs)
    grids = {}
    for k, n in enumerate(SIZES):
        grids[n] = U.special_values(n, 60 + k)
        grids[n].tofile(str(tmp_path / ("in_%dx%dx%d.bin" % n)))
    p = subprocess.run([exe, str(tmp_path)] + [str(v) for n in SIZES for v in n], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, "exit status %d\n%s\n%s" % (p.returncode, p.stdout, p.stderr)
    assert "all checks passed" in p.stdout
    for n in SIZES:
        got = np.fromfile(str(tmp_path / ("out_%dx%dx%d.bin" % n)), dtype=f32)
        want = U.octets32(grids[n], n)
        assert got.size == want.size, n
        assert np.array_equal(u32(got), u32(want).reshape(-1)), (n, int((u32(got) != u32(want).reshape(-1)).sum()))


# ---- the C-ABI additions -----------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("vspg_renderer_update_rgb_grids", "vspg_rgb_octets_read")


def test_new_symbols_are_declared_and_exported(pkg):
    names = [s[0] for s in pkg.SYMBOLS]
    for name in NEW_SYMBOLS:
        assert names.count(name) == 1
    lib = pkg.load()   # raises if a declared symbol is not exported
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None


def test_argument_checks_that_need_no_device(pkg):
    lib = pkg.load()
    v = np.zeros(24, dtype=f32)
    out = np.zeros(512 * 32, dtype=f32)
    for mem in (pkg.MEM_HOST, pkg.MEM_DEVICE, 7):
        assert lib.vspg_renderer_update_rgb_grids(None, v.ctypes.data, None, None, v.size, mem, None) == pkg.VSPG_EINVAL
        assert b"null renderer" in lib.vspg_last_error()
    assert lib.vspg_renderer_update_rgb_grids(None, None, None, None, 0, pkg.MEM_HOST, None) == pkg.VSPG_EINVAL
    assert lib.vspg_rgb_octets_read(None, 0, out.ctypes.data_as(C.POINTER(C.c_float)), out.size, None) == pkg.VSPG_EINVAL
    assert lib.vspg_last_error()


ABI_PROGRAM = r"""
#include <stdio.h>
#include <stddef.h>
#include "vspg.h"
#ifdef TAKE_THE_DECLARATIONS
int (*update)(VspgRenderer *, const float *, const float *, const float *, size_t, int, void *) = vspg_renderer_update_rgb_grids;
int (*read_octets)(VspgRenderer *, int, float *, size_t, void *) = vspg_rgb_octets_read;
#endif
int main(void) {
    printf("%zu %zu %d %d %d\n", sizeof(VspgMedium), sizeof(VspgScene), VSPG_ABI_VERSION, VSPG_MEM_HOST, VSPG_MEM_DEVICE);
    return 0;
}
"""


def test_header_still_compiles_as_c_and_the_records_keep_their_size(pkg, tmp_path):
    """C99: the two declarations taken by their exact types (a mismatch is an error under -Werror; compiled only -- the library is not
    linked), then the sizes from a program that runs: sizeof(VspgMedium) / sizeof(VspgScene) are the parent's
    (tests/test_rgbgrid_model.py), VSPG_ABI_VERSION stays 7."""
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text(ABI_PROGRAM)
    cc = ["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include")]
    subprocess.check_call(cc + ["-DTAKE_THE_DECLARATIONS", "-c", "-o", str(tmp_path / "abi.o"), str(src)])
    subprocess.check_call(cc + ["-o", str(exe), str(src)])
    v = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert v == [312, 4392, 7, 0, 1]
    assert C.sizeof(pkg.VspgMedium) == 312 and C.sizeof(pkg.VspgScene) == 4392


# ---- the wrapper's refusals ----------------------------------------------------------------------------------------------------------------
def test_wrapper_refusals_need_no_device(pkg):
    n = 2 * 3 * 5
    good = np.zeros((5, 3, 2, 3), dtype=f32)
    ptrs, memory, stream = pkg.rgb_update_sources(n, good, None, good, 0)
    assert ptrs == [good.ctypes.data, None, good.ctypes.data] and memory == pkg.MEM_HOST and stream is None
    with pytest.raises(ValueError, match="at least one"):
        pkg.rgb_update_sources(n, None, None, None, 0)
    bad = [good.astype(np.float64),                      # dtype
           np.zeros(3 * n - 1, dtype=f32),               # size
           np.zeros(n, dtype=f32),                       # size: a scalar grid's
           np.zeros((5, 3, 2, 6), dtype=f32)[..., ::2],  # layout
           [0.0] * (3 * n)]                              # no array
    for b in bad:
        for slot in range(3):
            args = [good, good, good]
            args[slot] = b
            with pytest.raises(ValueError):
                pkg.rgb_update_sources(n, *args, 0)
            only = [None, None, None]
            only[slot] = b
            with pytest.raises(ValueError):
                pkg.rgb_update_sources(n, *only, 0)
    # the method refuses before the library is called: no handle is needed to get the ValueError
    r = pkg.Renderer.__new__(pkg.Renderer)
    r.lib, r.h = None, None
    r.scene = pkg.fog_box_scene(8, 8)
    r.scene.medium.nx, r.scene.medium.ny, r.scene.medium.nz = 2, 3, 5
    r.cfg = pkg.VspgRenderConfig(8, 8, 1, 0, 0, 1, 0)
    with pytest.raises(ValueError):
        r.update_rgb()
    with pytest.raises(ValueError):
        r.update_rgb(sigma_s=good.astype(np.float64))


def test_wrapper_refuses_tensors_off_the_device(pkg):
    """(NumPy arrays mixed with tensors ON the device: tests/test_rgbgrid_update_gpu.py.)"""
    import torch
    n = 4
    host = np.zeros(3 * n, dtype=f32)
    cpu_tensor = torch.zeros(3 * n, dtype=torch.float32)
    with pytest.raises(ValueError):      # a torch tensor that is not on the renderer's device
        pkg.rgb_update_sources(n, cpu_tensor, None, None, 0)
    with pytest.raises(ValueError):
        pkg.rgb_update_sources(n, host, cpu_tensor, None, 0)
