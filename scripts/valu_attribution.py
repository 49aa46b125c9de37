"""Per-source-line attribution of a kernel's non-arithmetic vector instructions (moves, selects, compares, bit and lane ops) and of
its exec-mask bookkeeping, from a line-table assembly listing.

    hipcc <the Makefile's HIPFLAGS> -gline-tables-only --cuda-device-only -S -o k.s <unit that instantiates the kernel>
    python scripts/valu_attribution.py k.s [kernel symbol prefix] [--top N]

Every instruction is charged to the `.loc` in force where it stands (the innermost inlined source line; the compiler's own
materialisations at a block's start carry the line of the block).  Classes are scripts/static_instmix.py's; "non-arithmetic" is its
`mov_sel` + `cmp` classes plus the bitwise integer ops (and / or / xor / not / bfi / bfe / perm / alignbit).  `v_mov_b32` is split by
its source operand: an inline constant, a 32-bit literal, a VGPR copy, an SGPR copy.  Static counts: what the compiler emitted, not
what runs."""
import collections
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from static_instmix import classify  # noqa: E402

HEADLINE = "_ZN4vspg17k_render_wave_wg3INS_18HomogeneousMediumTILi2ELb1ELb1EEELb0ELi704ELi512ELi4ELb0E"
BITOP = re.compile(r"^v_(and|or|xor|not|xnor|or3|and_or|xor3|bfi|bfe|perm|alignbit)_")
SALU_EXEC = ("s_and_saveexec_b64", "s_or_b64", "s_xor_b64", "s_andn2_b64", "s_or_saveexec_b64", "s_andn2_saveexec_b64", "s_cbranch_execz",
             "s_cbranch_execnz")


def mov_kind(args):
    src = args.split(",")[-1].strip().split()[0] if "," in args else ""
    if re.match(r"^v\d+$", src):
        return "mov_vgpr"
    if re.match(r"^s\d+$", src) or src in ("vcc_lo", "vcc_hi", "exec_lo", "exec_hi"):
        return "mov_sgpr"
    if src.startswith("0x") or (re.match(r"^-?\d+$", src) and not -16 <= int(src) <= 64):
        return "mov_literal"
    return "mov_inline"


def kernel_lines(path, prefix):
    files, out, inside = {}, [], False
    loc = ("?", 0)
    for line in open(path):
        m = re.match(r'^\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', line)
        if m:
            files[m.group(1)] = os.path.basename(m.group(3) or m.group(2))
            continue
        if not inside:
            if line.startswith(prefix) and line.split(":")[0].startswith(prefix) and not line.startswith((" ", "\t")):
                inside = True
            continue
        if line.startswith(".Lfunc_end"):
            break
        m = re.match(r"^\s*\.loc\s+(\d+)\s+(\d+)", line)
        if m:
            loc = (files.get(m.group(1), m.group(1)), int(m.group(2)))
            continue
        m = re.match(r"^\s+([a-z_0-9]+)\s*(.*)", line)
        if m and not m.group(1).startswith("."):
            out.append((loc, m.group(1), m.group(2)))
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    top = 40
    if "--top" in sys.argv:
        top = int(sys.argv[sys.argv.index("--top") + 1])
        args.remove(str(top))
    path = args[0]
    prefix = args[1] if len(args) > 1 else HEADLINE
    insts = kernel_lines(path, prefix)
    tot, per = collections.Counter(), collections.defaultdict(collections.Counter)
    for loc, op, a in insts:
        c = per[loc]
        if op.startswith("v_"):
            cls = classify(op)
            keys = ["valu"]
            if cls in ("mov_sel", "cmp") or BITOP.match(op):
                keys.append("nonarith")
                if op.startswith("v_mov_b32"):
                    keys += ["v_mov", mov_kind(a)]
                elif op.startswith("v_cndmask"):
                    keys.append("v_cndmask")
                elif cls == "cmp":
                    keys.append("v_cmp")
                else:
                    keys.append("bit_lane")
            for k in keys:
                c[k] += 1
                tot[k] += 1
        elif op in SALU_EXEC:
            c["exec"] += 1
            tot["exec"] += 1
    cols = ["valu", "nonarith", "v_mov", "mov_inline", "mov_literal", "mov_vgpr", "mov_sgpr", "v_cndmask", "v_cmp", "bit_lane", "exec"]
    print("%-28s" % "total" + "".join("%11s" % k for k in cols))
    print("%-28s" % "" + "".join("%11d" % tot[k] for k in cols))
    print()
    print("%-28s" % "source line (top by non-arith)" + "".join("%11s" % k for k in cols))
    for loc, c in sorted(per.items(), key=lambda kv: -kv[1]["nonarith"])[:top]:
        print("%-28s" % ("%s:%d" % loc) + "".join("%11d" % c[k] for k in cols))


if __name__ == "__main__":
    main()
