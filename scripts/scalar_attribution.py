"""Per-source-line attribution of a kernel's scalar stream -- scalar ALU, branches, exec-save regions -- from a line-table assembly
listing: the sibling of scripts/valu_attribution.py for the instructions it leaves out.

    hipcc <the Makefile's HIPFLAGS> -gline-tables-only --cuda-device-only -S -o k.s <unit that instantiates the kernel>
    python scripts/scalar_attribution.py k.s [kernel symbol prefix] [--top N] [--by-file]

Every instruction is charged to the `.loc` in force where it stands (the innermost inlined source line; what the compiler puts at
a join -- the mask merges of a divergent if -- carries the line of the join, often line 0).  Columns:
  salu     scalar ALU: every s_* that is no branch, no scalar load, no wait / nop / sleep / barrier / message;
  mask     of those, 64-bit lane-mask logic and moves (s_and / or / xor / andn2 / orn2 / not / mov / cselect _b64, saveexec included);
  saveexec s_*_saveexec_b64: one per exec-save region;
  branch   s_branch / s_cbranch_*;
  execbr   of those, s_cbranch_execz / s_cbranch_execnz;
  valu     vector instructions on the same line, for scale.
Static counts: what the compiler emitted, not what runs.  Scalar ALU and branches both take scalar issue
(profiles/scalar_issue_microbench.txt), so `salu + branch` is what the ranking sorts by; --by-file adds the totals per source file."""
import collections
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from valu_attribution import HEADLINE, kernel_lines  # noqa: E402

NOT_ALU = ("s_load", "s_buffer_load", "s_waitcnt", "s_nop", "s_sleep", "s_barrier", "s_endpgm", "s_memtime", "s_memrealtime", "s_setprio", "s_sendmsg",
           "s_icache", "s_setreg", "s_getreg", "s_code_end", "s_trap", "s_sethalt")
MASK = re.compile(r"^s_(and|or|xor|andn2|orn2|nand|nor|xnor|not|mov|cselect|wqm)_b64$|^s_\w+_saveexec_b64$")
SAVEEXEC = re.compile(r"^s_\w+_saveexec_b64$")
COLS = ["salu", "mask", "saveexec", "branch", "execbr", "valu"]


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    top = 40
    if "--top" in sys.argv:
        top = int(sys.argv[sys.argv.index("--top") + 1])
        args.remove(str(top))
    by_file = "--by-file" in sys.argv
    path = args[0]
    prefix = args[1] if len(args) > 1 else HEADLINE
    tot, per = collections.Counter(), collections.defaultdict(collections.Counter)
    for loc, op, _ in kernel_lines(path, prefix):
        keys = []
        if op.startswith("v_"):
            keys = ["valu"]
        elif op.startswith(("s_cbranch", "s_branch")):
            keys = ["branch"] + (["execbr"] if op in ("s_cbranch_execz", "s_cbranch_execnz") else [])
        elif op.startswith("s_") and not op.startswith(NOT_ALU):
            keys = ["salu"] + (["mask"] if MASK.match(op) else []) + (["saveexec"] if SAVEEXEC.match(op) else [])
        for k in keys:
            per[loc][k] += 1
            tot[k] += 1
            if by_file:
                per[(loc[0], -1)][k] += 1
    print("%-28s" % "total" + "".join("%10s" % k for k in COLS))
    print("%-28s" % "" + "".join("%10d" % tot[k] for k in COLS))
    if by_file:
        print()
        print("%-28s" % "source file" + "".join("%10s" % k for k in COLS))
        for loc, c in sorted(((l, c) for l, c in per.items() if l[1] == -1), key=lambda kv: -(kv[1]["salu"] + kv[1]["branch"])):
            print("%-28s" % loc[0] + "".join("%10d" % c[k] for k in COLS))
    print()
    print("%-28s" % "source line (top by salu + branch)" + "".join("%10s" % k for k in COLS))
    lines = sorted(((l, c) for l, c in per.items() if l[1] != -1), key=lambda kv: -(kv[1]["salu"] + kv[1]["branch"]))
    for loc, c in lines[:top]:
        print("%-28s" % ("%s:%d" % loc) + "".join("%10d" % c[k] for k in COLS))


if __name__ == "__main__":
    main()
