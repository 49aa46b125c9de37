"""Static checks of how k_render_wave_wg3_carry's headline instantiation moves its workgroup image, read from the built library's code
object next to the pinned k_render_wave_wg3 of the same library, the way tests/test_wg3_carry_kernel.py reads them (no GPU needed).

The image -- pool, rings, queue words: 76 160 bytes for the headline pool -- lies in global memory as it lies in LDS and is copied in
16-byte pieces: ten 128-bit loads per lane (4752 pieces over 512 lanes), every one in flight before the first LDS write, and ten
128-bit stores in the epilogue.  The dword copy it replaced took 35 loads per lane in five load-then-write batches and repacked the
rings; with it gone the carry entry point's surplus of vector instructions over the pinned kernel fell from 355 to CARRY_EXTRA
(the pinned kernel itself lost 35 in the same change, with the fresh chunk's grouped loads)."""
import os
import re
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("VSPG_LIB") or os.path.join(ROOT, "vspg-pbrt-v4_amd", "csrc", "libvspg_hip.so")
PINNED = "_ZN4vspg17k_render_wave_wg3INS_18HomogeneousMediumTILi2ELb1ELb1EEELb0ELi704ELi512ELi4ELb0E"
CARRY = "_ZN4vspg23k_render_wave_wg3_carryINS_18HomogeneousMediumTILi2ELb1ELb1EEELb0ELi704ELi512ELi4ELb0E"   # (the full-frame one)
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
CARRY_EXTRA = 306   # vector instructions of prologue + epilogue + per-chunk tests, measured on the first clean build with the 16-byte copy
MARGIN = 8
IMAGE_PIECES = (25 * 704 + 4 * 704 // 2) // 4   # 16-byte pieces of pool + rings, headline layout (25 dwords per path, 704 paths)
ROUNDS = -(-IMAGE_PIECES // 512)


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
    """{PINNED: opcodes, CARRY: opcodes}: exactly one symbol each"""
    if not os.path.exists(LIB):
        pytest.fail("%s not built (run __graft_entry__.build())" % LIB)
    objdump = _tool("llvm-objdump")
    tmp = tmp_path_factory.mktemp("boundary")
    ops = {PINNED: [], CARRY: []}
    for k, co in enumerate(_code_objects(open(LIB, "rb").read())):
        if not any(key.encode() in co for key in ops):
            continue
        path = tmp / ("co%d.o" % k)
        path.write_bytes(co)
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
    for key in ops:
        assert len(ops[key]) == 1, (key, len(ops[key]))
    return {key: ops[key][0] for key in ops}


def test_carry_surplus_of_vector_instructions(kernels):
    valu = {key: sum(op.startswith("v_") for op in kernels[key]) for key in kernels}
    print("vector instructions: pinned %d, carry %d (+%d)" % (valu[PINNED], valu[CARRY], valu[CARRY] - valu[PINNED]))
    assert valu[CARRY] - valu[PINNED] <= CARRY_EXTRA + MARGIN


def test_prologue_loads_the_image_in_16_byte_pieces_before_the_first_lds_write(kernels):
    ops = kernels[CARRY]
    first = ops.index("global_load_dwordx4")                      # the prologue's copy: from its first piece to the barrier behind it
    prologue = ops[first:first + ops[first:].index("s_barrier")]
    wide = [i for i, op in enumerate(prologue) if op == "global_load_dwordx4"]
    narrow = [op for op in prologue if op.startswith("global_load") and op != "global_load_dwordx4"]
    writes = [i for i, op in enumerate(prologue) if op == "ds_write_b128"]
    print("prologue: %d instructions, %d 128-bit loads, narrower loads %s, %d 128-bit LDS writes" % (len(prologue), len(wide), narrow, len(writes)))
    assert len(wide) == ROUNDS and len(writes) == ROUNDS
    assert narrow in ([], ["global_load_dword"])                  # (the queue words: one dword in 20 lanes)
    assert wide[-1] < writes[0], "a piece is loaded behind the first LDS write: a second round trip"
    assert not any(op.startswith("global_load") for op in prologue[writes[0]:])


def test_epilogue_stores_the_image_in_16_byte_pieces(kernels):
    n = {key: sum(op == "global_store_dwordx4" for op in kernels[key]) for key in kernels}
    reads = sum(op == "ds_read_b128" for op in kernels[CARRY]) - sum(op == "ds_read_b128" for op in kernels[PINNED])
    print("128-bit global stores: pinned %d, carry %d; 128-bit LDS reads: carry has %d more" % (n[PINNED], n[CARRY], reads))
    assert n[CARRY] - n[PINNED] >= ROUNDS and reads >= ROUNDS
