"""Static checks of k_render_wave_wg3_carry's headline instantiation, read from the built library's code object (no GPU needed), next
to the pinned k_render_wave_wg3 instantiation OF THE SAME LIBRARY (tests/test_headline_kernel_census.py, _resources.py).

The carry entry point shares the kernel's body (csrc/vspg_wg3.h, CARRY): what it adds is a prologue that copies the workgroup's image
back into LDS, an epilogue that writes it out and marks the suspended pixels, and a few instructions per chunk that tell resumed
paths apart.  It runs the benchmark's steps, so it has to keep the pinned kernel's budget: four waves per SIMD (<= 128 VGPRs), no
scratch, no more SGPR spills than the pinned kernel, LDS within VSPG_WG3_LDS_BUDGET, and a vector-instruction count of at most the
pinned kernel's plus the size of prologue + epilogue.

First clean build: pinned kernel 5728 vector instructions, carry kernel 6077: 349 more -- the prologue's unrolled copy loops, the
epilogue, resolve_sample inlined where a resumed path ends (once per chunk kind) and the per-chunk tests that tell such a path --
to which 8 are added for scheduling noise."""
import os
import re
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("VSPG_LIB") or os.path.join(ROOT, "vspg-pbrt-v4_amd", "csrc", "libvspg_hip.so")
HEADER = os.path.join(ROOT, "vspg-pbrt-v4_amd", "csrc", "vspg_wg3.h")
PINNED = "_ZN4vspg17k_render_wave_wg3INS_18HomogeneousMediumTILi2ELb1ELb1EEELb0ELi704ELi512ELi4ELb0E"
CARRY = "_ZN4vspg23k_render_wave_wg3_carryINS_18HomogeneousMediumTILi2ELb1ELb1EEELb0ELi704ELi512ELi4ELb0E"   # (the full-frame one)
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
CARRY_EXTRA = 349   # vector instructions of prologue + epilogue + per-chunk tests, measured on the first clean build
MARGIN = 8


def _tool(name):
    for cand in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", name), shutil.which(name)):
        if cand and os.path.exists(cand):
            return cand
    pytest.fail("%s not found (ROCm's LLVM)" % name)


def _code_objects(data):
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
def kernels(tmp_path_factory):
    """{PINNED: (metadata block, opcodes), CARRY: (...)}: exactly one symbol each"""
    if not os.path.exists(LIB):
        pytest.fail("%s not built (run __graft_entry__.build())" % LIB)
    readelf, objdump = _tool("llvm-readelf"), _tool("llvm-objdump")
    tmp = tmp_path_factory.mktemp("carry")
    meta, ops = {PINNED: [], CARRY: []}, {PINNED: [], CARRY: []}
    for k, co in enumerate(_code_objects(open(LIB, "rb").read())):
        path = tmp / ("co%d.o" % k)
        path.write_bytes(co)
        notes = subprocess.run([readelf, "--notes", str(path)], check=True, capture_output=True, text=True).stdout
        for b in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
            name = re.search(r"\n\s+\.name:\s+(\S+)", b)
            for key in meta:
                if name and name.group(1).startswith(key):
                    meta[key].append(b)
        if not any(key.encode() in co for key in ops):
            continue
        text = subprocess.run([objdump, "-d", str(path)], check=True, capture_output=True, text=True).stdout
        cur = None
        for line in text.split("\n"):
            m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
            if m:
                cur = next((key for key in ops if m.group(1).startswith(key)), None)
                if cur:
                    ops[cur].append([])
                continue
            m = re.match(r"^\s+([a-z_0-9]+)", line)
            if m and cur:
                ops[cur][-1].append(m.group(1))
    for key in meta:
        assert len(meta[key]) == 1 and len(ops[key]) == 1, (key, len(meta[key]), len(ops[key]))
    return {key: (meta[key][0], ops[key][0]) for key in meta}


def _field(block, key):
    m = re.search(r"\n\s+\.%s:\s+(\d+)" % re.escape(key), block)
    assert m, "metadata field .%s missing" % key
    return int(m.group(1))


def test_carry_kernel_keeps_the_register_budget(kernels):
    b, pinned = kernels[CARRY][0], kernels[PINNED][0]
    print("carry: vgpr %d, sgpr spills %d (pinned %d), scratch %d, lds %d" % (_field(b, "vgpr_count"), _field(b, "sgpr_spill_count"),
          _field(pinned, "sgpr_spill_count"), _field(b, "private_segment_fixed_size"), _field(b, "group_segment_fixed_size")))
    assert _field(b, "vgpr_count") <= 128
    assert _field(b, "vgpr_spill_count") == 0
    assert _field(b, "private_segment_fixed_size") == 0
    assert _field(b, "sgpr_spill_count") <= _field(pinned, "sgpr_spill_count")


def test_carry_kernel_lds_within_budget(kernels):
    m = re.search(r"#define VSPG_WG3_LDS_BUDGET (\d+)", open(HEADER).read())
    assert m
    assert _field(kernels[CARRY][0], "group_segment_fixed_size") <= int(m.group(1))
    assert _field(kernels[CARRY][0], "group_segment_fixed_size") == _field(kernels[PINNED][0], "group_segment_fixed_size")   # same pool, same rings


def test_carry_kernel_path_code_is_the_pinned_kernels_size(kernels):
    valu = {key: sum(op.startswith("v_") for op in kernels[key][1]) for key in kernels}
    print("vector instructions: pinned %d, carry %d (+%d)" % (valu[PINNED], valu[CARRY], valu[CARRY] - valu[PINNED]))
    assert valu[CARRY] <= valu[PINNED] + CARRY_EXTRA + MARGIN
