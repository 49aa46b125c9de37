"""Static instruction census of the benchmark's kernel, read from the built library's code object (no GPU needed).

The headline instantiation of k_render_wave_wg3 is vector-issue bound, and about half of its vector instructions are not arithmetic
(moves, selects, compares, bit ops).  Its ray spawning used to form both float neighbours of each origin component and pick one with
two selects (offset_axis, csrc/vspg_device.h), and the atomic optimizer wrapped every lane-0 scheduler atomic in a wave reduction
(csrc/vspg_wg3_exact.hip): vector instructions 5944 -> 5726, v_cndmask_b32 472 -> 397, v_cmp_* 695 -> 608.  v_mov_b32 barely moved
(896 -> 888), so selects and compares are what is pinned.  These ceilings keep that from growing back unnoticed;
they sit a little above the current counts so that unrelated scheduling changes do not trip them."""
import os
import re
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("VSPG_LIB") or os.path.join(ROOT, "vspg-pbrt-v4_amd", "csrc", "libvspg_hip.so")
HEADLINE = "_ZN4vspg17k_render_wave_wg3INS_18HomogeneousMediumTILi2ELb1ELb1EEELb0ELi704ELi512ELi4ELb0E"
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
MAX_VALU = 5760        # ceilings to lower, never to raise
MAX_SELECT_COMPARE = 1010  # v_cndmask_b32 + v_cmp_*


def _objdump():
    for cand in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-objdump"),
                 shutil.which("llvm-objdump")):
        if cand and os.path.exists(cand):
            return cand
    pytest.fail("llvm-objdump not found (ROCm's LLVM)")


def _code_objects(data):
    """The gfx950 code objects of every offload bundle embedded in the library (uncompressed clang offload bundles)."""
    out = []
    pos = data.find(BUNDLE_MAGIC)
    while pos >= 0:
        (n,) = struct.unpack_from("<Q", data, pos + 24)
        p = pos + 32
        for _ in range(n):
            off, size, idlen = struct.unpack_from("<QQQ", data, p)
            ident = data[p + 24:p + 24 + idlen].decode()
            p += 24 + idlen
            if "gfx950" in ident:
                out.append(data[pos + off:pos + off + size])
        pos = data.find(BUNDLE_MAGIC, pos + 1)
    return out


@pytest.fixture(scope="module")
def headline_ops(tmp_path_factory):
    if not os.path.exists(LIB):
        pytest.fail("%s not built (run __graft_entry__.build())" % LIB)
    objdump = _objdump()
    tmp = tmp_path_factory.mktemp("census")
    found = []
    for k, co in enumerate(_code_objects(open(LIB, "rb").read())):
        path = tmp / ("co%d.o" % k)
        path.write_bytes(co)
        text = subprocess.run([objdump, "-d", str(path)], check=True, capture_output=True, text=True).stdout
        ops, cur = None, None
        for line in text.split("\n"):
            m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
            if m:
                cur = m.group(1)
                if cur.startswith(HEADLINE):
                    ops = []
                    found.append((cur, ops))
                continue
            m = re.match(r"^\s+([a-z_0-9]+)", line)
            if m and cur is not None and cur.startswith(HEADLINE):
                ops.append(m.group(1))
    assert len(found) == 1, [n for n, _ in found]
    return found[0][1]


def test_headline_kernel_vector_instructions_stay_down(headline_ops):
    assert sum(op.startswith("v_") for op in headline_ops) <= MAX_VALU


def test_headline_kernel_selects_and_compares_stay_down(headline_ops):
    n = sum(op.startswith(("v_cndmask_b32", "v_cmp_")) for op in headline_ops)
    assert n <= MAX_SELECT_COMPARE
