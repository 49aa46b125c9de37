"""Static census of the benchmark kernel's scalar stream as a whole -- scalar ALU instructions and branches --, read from the built
library's code object (no GPU needed); the sibling of tests/test_headline_scalar_census.py, which pins the exec-mask part of it.

The kernel issues two scalar or branch instructions for every three vector ones and a scalar instruction is not free at that ratio
(profiles/scalar_issue_microbench.txt).  The any-hit walk in two stages (csrc/vspg_device.h, rects_any_planes) ADDS static text --
the pre-pass stands in front of the walk it usually replaces: 1730 -> 1843 scalar ALU instructions and 371 -> 395 branches in the
pinned k_render_wave_wg3 instantiation -- while what runs falls (profiles/anyhit_table_static.txt, anyhit_table_ab.txt: per shadow
ray 185 -> 90 scalar instructions on the path where no lane is a candidate; SQ_INSTS_SALU -4.9 %, SQ_INSTS_BRANCH -8.8 % per launch).
So these pins do not say the stream is short; they keep further text from arriving unseen.  The ceilings are the counts plus 1 %,
rounded up; they only ever go down.  Scalar ALU is what scripts/scalar_attribution.py calls it: every s_* that is no branch, no
scalar load and no wait / nop / sleep / barrier / message.  The carry entry point's surplus stays pinned where it is, in
tests/test_headline_scalar_census.py and tests/test_wg3_carry_kernel.py."""
import math

from test_headline_scalar_census import PINNED, ops   # noqa: F401  (the fixture: the opcodes of the pinned kernel and its carry twin)

NOT_ALU = ("s_load", "s_buffer_load", "s_waitcnt", "s_nop", "s_sleep", "s_barrier", "s_endpgm", "s_memtime", "s_memrealtime", "s_setprio",
           "s_sendmsg", "s_icache", "s_setreg", "s_getreg", "s_code_end", "s_trap", "s_sethalt")
BRANCH = ("s_branch", "s_cbranch")
SCALAR_ALU_NOW, BRANCHES_NOW = 1843, 395                   # the pinned kernel when the ceilings were set
MAX_SCALAR_ALU = math.ceil(SCALAR_ALU_NOW * 1.01)          # 1862; ceilings to lower, never to raise
MAX_BRANCHES = math.ceil(BRANCHES_NOW * 1.01)              # 399


def test_headline_kernel_scalar_alu_stays_down(ops):
    n = sum(op.startswith("s_") and not op.startswith(NOT_ALU) and not op.startswith(BRANCH) for op in ops[PINNED])
    print("pinned kernel: %d scalar ALU instructions (ceiling %d)" % (n, MAX_SCALAR_ALU))
    assert n <= MAX_SCALAR_ALU


def test_headline_kernel_branches_stay_down(ops):
    n = sum(op.startswith(BRANCH) for op in ops[PINNED])
    print("pinned kernel: %d branches (ceiling %d)" % (n, MAX_BRANCHES))
    assert n <= MAX_BRANCHES
