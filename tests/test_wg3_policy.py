"""k_render_wave_wg3's chunk policy (csrc/vspg_wg3.h: w3_policy) as host code: tests/wg3_policy_check.cpp includes the kernel's
header, calls the function the kernel calls and compares it, over every combination of the values listed there, with a transcription
of the `if` chain the kernel's loop held before (no GPU needed).  Compiled for the host only with the library's flags, linked and run
directly."""
import os
import shlex
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vspg-pbrt-v4_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "wg3_policy_check.cpp")


def test_policy_equals_the_former_chain_exhaustively(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    hipcc, clangxx = os.path.join(rocm, "bin", "hipcc"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")
    for tool in (hipcc, clangxx):
        if not os.path.exists(tool):
            pytest.fail("%s not found (ROCm)" % tool)
    flags = shlex.split(subprocess.check_output(["make", "-s", "--no-print-directory", "-C", CSRC, "print-HIPFLAGS"], text=True))
    obj, exe = str(tmp_path / "wg3_policy_check.o"), str(tmp_path / "wg3_policy_check")
    cmd = [hipcc] + flags + ["--cuda-host-only", "-x", "hip", "-I", CSRC, "-c", "-o", obj, DRIVER]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, "%s\n%s\n%s" % (" ".join(cmd), p.stdout, p.stderr)
    subprocess.check_call([clangxx, "-o", exe, obj])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, "exit status %d\n%s\n%s" % (p.returncode, p.stdout, p.stderr)
    # 6^4 avail x 2 x 2 x 2 x 2 x 3 shared words, CARRY and not
    assert p.stdout.startswith("%d cases" % (6 ** 4 * 48 * 2)) and p.stdout.rstrip().endswith(", 0 differ"), p.stdout
