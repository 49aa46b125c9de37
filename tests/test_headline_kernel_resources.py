"""Register budget of the benchmark's kernel, read from the built library's code-object metadata (no GPU needed).

The headline workload (bench.py, the 1080p fog box) runs almost entirely in one instantiation of k_render_wave_wg3: the grey
homogeneous medium over grey surfaces with a null-collision coefficient of exactly 0.  Its launch bound asks for four waves per
SIMD, so it has at most 128 VGPRs, and it used to run out of SGPRs: 50 of them were spilled into lanes of a VGPR and read back
with v_readlane at every use.  Scene fields inside the record's first 4 KB and the per-use forms of the launch flags and the
lane compares (csrc/vspg_wg3.h) brought that down to the three pointers and the PCG jump of the launch, held over the whole loop:
8 SGPRs.  These checks keep the count from growing back unnoticed.  (The tolerance-mode objects of csrc/Makefile hold their own
copies in other namespaces; the benchmark's figure is the exact one checked here.)
"""
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
MAX_SGPR_SPILLS = 8  # a ceiling to lower, never to raise


def _readelf():
    for cand in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-readelf"),
                 shutil.which("llvm-readelf")):
        if cand and os.path.exists(cand):
            return cand
    pytest.fail("llvm-readelf not found (ROCm's LLVM)")


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


def _kernels(readelf, code_object, tmp_path, k):
    path = tmp_path / ("co%d.o" % k)
    path.write_bytes(code_object)
    notes = subprocess.run([readelf, "--notes", str(path)], check=True, capture_output=True, text=True).stdout
    # the AMDGPU metadata note lists one block per kernel, each starting with '- .agpr_count:' (fields in alphabetical order)
    blocks = re.split(r"\n\s+- \.agpr_count:", notes)[1:]
    kernels = {}
    for b in blocks:
        name = re.search(r"\n\s+\.name:\s+(\S+)", b)
        if name:
            kernels[name.group(1)] = b
    return kernels


def _field(block, key):
    m = re.search(r"\n\s+\.%s:\s+(\d+)" % re.escape(key), block)
    assert m, "metadata field .%s missing" % key
    return int(m.group(1))


@pytest.fixture(scope="module")
def headline_blocks(tmp_path_factory):
    if not os.path.exists(LIB):
        pytest.fail("%s not built (run __graft_entry__.build())" % LIB)
    readelf = _readelf()
    data = open(LIB, "rb").read()
    cos = _code_objects(data)
    assert cos, "no gfx950 code object in %s" % LIB
    tmp = tmp_path_factory.mktemp("co")
    found = []
    for k, co in enumerate(cos):
        for name, block in _kernels(readelf, co, tmp, k).items():
            if name.startswith(HEADLINE):
                found.append((name, block))
    assert len(found) == 1, [n for n, _ in found]
    return found


def test_headline_kernel_sgpr_spills_stay_down(headline_blocks):
    for name, b in headline_blocks:
        assert _field(b, "sgpr_spill_count") <= MAX_SGPR_SPILLS, name


def test_headline_kernel_spills_no_vgprs(headline_blocks):
    for name, b in headline_blocks:
        assert _field(b, "vgpr_spill_count") == 0, name


def test_headline_kernel_uses_no_scratch(headline_blocks):
    for name, b in headline_blocks:
        assert _field(b, "private_segment_fixed_size") == 0, name


def test_headline_kernel_keeps_four_waves_per_simd(headline_blocks):
    for name, b in headline_blocks:
        assert _field(b, "vgpr_count") <= 128, name
