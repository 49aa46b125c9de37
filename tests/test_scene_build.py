"""The host-side scene preprocessing on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer (no GPU needed).

csrc/vspg_scene_build.hip (validation, the device scene record, light samplers, the triangle BVH, majorant grids, environment tables)
and csrc/vspg_scene_api.hip (the entry points that need no renderer) hold no kernel and call no HIP function, so they link without
the HIP runtime.  This test compiles both with the library's own flags (csrc/Makefile: HIPFLAGS -- -ffp-contract=off -fno-fast-math
are part of what the code computes) plus the sanitizers on the host side, links them with tests/scene_build_check.cpp by plain
clang++ and runs the program, which builds small scenes and checks structural facts of the results (see its cases).  It is the part
of the library that indexes fixed-size arrays from scene input.  Nothing is loaded into Python."""
import os
import shlex
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vspg-pbrt-v4_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
UNITS = ("vspg_scene_build", "vspg_scene_api")


def _run(cmd, **kw):
    p = subprocess.run(cmd, capture_output=True, text=True, **kw)
    assert p.returncode == 0, "%s\n%s\n%s" % (" ".join(cmd), p.stdout, p.stderr)
    return p


def test_scene_preprocessing_under_sanitizers(tmp_path):
    hipcc = os.path.join(ROCM, "bin", "hipcc")
    clangxx = os.path.join(ROCM, "lib", "llvm", "bin", "clang++")
    for tool in (hipcc, clangxx):
        if not os.path.exists(tool):
            pytest.fail("%s not found (ROCm)" % tool)
    flags = shlex.split(_run(["make", "-s", "--no-print-directory", "-C", CSRC, "print-HIPFLAGS"]).stdout)
    assert "-ffp-contract=off" in flags and "-fno-fast-math" in flags, flags
    host = [a for s in SANITIZE for a in ("-Xarch_host", s)]
    objs = []
    jobs = [(os.path.join(CSRC, u + ".hip"), []) for u in UNITS] + [(os.path.join(ROOT, "tests", "scene_build_check.cpp"), ["-x", "hip", "-I", CSRC])]
    procs = []
    for src, extra in jobs:
        obj = str(tmp_path / (os.path.splitext(os.path.basename(src))[0] + ".o"))
        objs.append(obj)
        cmd = [hipcc] + flags + host + ["-g"] + extra + ["-c", "-o", obj, src]
        procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for cmd, p in procs:
        out = p.communicate()[0]
        assert p.returncode == 0, "%s\n%s" % (" ".join(cmd), out)
    for obj in objs:  # host code only: a unit with device code would need the HIP runtime to link
        assert b"__CLANG_OFFLOAD_BUNDLE__" not in open(obj, "rb").read(), obj
    exe = str(tmp_path / "scene_build_check")
    _run([clangxx] + SANITIZE + ["-o", exe] + objs)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, "exit status %d\n%s\n%s" % (p.returncode, p.stdout, p.stderr)
    assert p.stderr.strip() == "", p.stderr
