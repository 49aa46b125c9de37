"""Static census of what k_render_wave_wg3's scheduler issues, read from the built library's code object (no GPU needed) the way
tests/test_wg3_carry_kernel.py reads it: the pinned instantiation and its carry twin.

Two counts stand for the scheduler (csrc/vspg_wg3.h) because almost nothing else in the kernel issues them:
  * v_readfirstlane_b32 + v_readlane_b32 -- making scalars of the queue words.  The decision used to scalarise seventeen words a poll;
    now lane q computes queue q's `avail`, two ballots carry the four to the scalar side and only the chosen queue's head is read
    from its lane (parent 51 / carry 54; now 42 / 45, the tile cursor's, the claims' results and ring_push_all's four bases among them).
  * LDS atomics (ds_add_*, ds_sub_*, ds_cmpst_*, ds_wrxchg_*) -- the claims, the pushes and the counters.  A chunk's tail was three
    atomics from lane 0 and is one from three lanes; a fresh claim's two counters are one atomic from two lanes (parent 40 / carry
    42; now 23 / 23, the seven of the launch's counters at the kernel's end included).
Ceilings: the first clean build's counts plus 2; to lower, never to raise."""
from test_wg3_carry_kernel import CARRY, PINNED, kernels   # noqa: F401  (the fixture: metadata and opcodes of the two kernels)

LANE_READS = ("v_readfirstlane_b32", "v_readlane_b32")
LDS_ATOMICS = ("ds_add_", "ds_sub_", "ds_cmpst_", "ds_wrxchg_")
MAX_LANE_READS = {PINNED: 42 + 2, CARRY: 45 + 2}
MAX_LDS_ATOMICS = {PINNED: 23 + 2, CARRY: 23 + 2}


def test_scheduler_scalarises_few_words(kernels):
    for key in (PINNED, CARRY):
        n = sum(op in LANE_READS for op in kernels[key][1])
        print("%s: %d lane reads (ceiling %d)" % ("carry" if key == CARRY else "pinned", n, MAX_LANE_READS[key]))
        assert n <= MAX_LANE_READS[key], key


def test_scheduler_issues_few_lds_atomics(kernels):
    for key in (PINNED, CARRY):
        n = sum(op.startswith(LDS_ATOMICS) for op in kernels[key][1])
        print("%s: %d LDS atomics (ceiling %d)" % ("carry" if key == CARRY else "pinned", n, MAX_LDS_ATOMICS[key]))
        assert n <= MAX_LDS_ATOMICS[key], key
