// wg3_policy_check.cpp -- k_render_wave_wg3's chunk policy (csrc/vspg_wg3.h: w3_policy, w3_policy_of) on the CPU, against a
// transcription of the `if` chain the kernel held before the policy became a function of two 4-bit masks: every combination of
//   avail of each of the four queues in {0, 1, 63, 64, 65, 128}, busyS, busyV in {0, 1}, exh in {0, 1}, live in {0, 64},
//   old in {0, 1, the drain bit},
// for CARRY and non-CARRY.  Same kind, same first and second queue, same requested counts.  Built and run by tests/test_wg3_policy.py.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "vspg_wg3.h"

using namespace vspg;

struct Ref {
    unsigned kind = W3_NONE, q0 = Q_VV, n0 = 0, q1 = Q_VS, n1 = 0;
};

// The chain as it stood in the kernel's loop, claims taken as won: `claim_vertex`, `claim_segment` and the branches, in their order.
template <bool CARRY>
static Ref chain(const unsigned a[Q_COUNT], unsigned busyS, unsigned busyV, bool exh, unsigned live, unsigned old_in) {
    Ref r;
    const unsigned old_word = CARRY ? old_in : 1u;
    const int aVV = (int)a[Q_VV], aVS = (int)a[Q_VS], aA = (int)a[Q_A], aF = exh ? 0 : (int)a[Q_F];
    const auto claim_vertex = [&](int a_first, unsigned q_first, int a_second, unsigned q_second) {
        const unsigned na = (unsigned)(a_first < 64 ? a_first : 64);
        if (na > 0u) {
            r.kind = W3_VERTEX; r.q0 = q_first; r.n0 = na;
            const unsigned nb = (unsigned)(a_second < 64 - (int)na ? a_second : 64 - (int)na);
            if (nb > 0u) { r.q1 = q_second; r.n1 = nb; }
        }
    };
    const auto claim_segment = [&]() {
        r.kind = W3_SEGMENT; r.q0 = Q_A; r.n0 = (unsigned)(aA < 64 ? aA : 64);
    };
    const int aV = aVV + aVS;
    if (CARRY && exh && old_word == 0u) r.kind = W3_EXIT;
    else if (aVV >= 64) claim_vertex(aVV, Q_VV, 0, Q_VS);
    else if (aVS >= 64) claim_vertex(aVS, Q_VS, 0, Q_VV);
    else if (aA >= 64) claim_segment();
    else if (aF >= 64) { r.kind = W3_FRESH; r.q0 = Q_F; r.n0 = 64u; }
    else if (aV >= 64 || (aV > 0 && busyS == 0u)) {
        if (aVV >= aVS) claim_vertex(aVV, Q_VV, aVS, Q_VS);
        else claim_vertex(aVS, Q_VS, aVV, Q_VV);
    } else if (aA > 0 && busyV == 0u) {
        claim_segment();
    } else if (exh && live == 0u) {
        r.kind = W3_EXIT;
    }
    return r;
}

template <bool CARRY>
static long check(long *cases, long kinds[5]) {
    static const unsigned kAvail[6] = {0u, 1u, 63u, 64u, 65u, 128u};
    static const unsigned kOld[3] = {0u, 1u, kCarryDrainBit};
    long bad = 0;
    for (int i = 0; i < 6 * 6 * 6 * 6; ++i) {
        const unsigned a[Q_COUNT] = {kAvail[i % 6], kAvail[i / 6 % 6], kAvail[i / 36 % 6], kAvail[i / 216]};
        for (int j = 0; j < 2 * 2 * 2 * 2 * 3; ++j) {
            const unsigned busyS = j & 1, busyV = j >> 1 & 1, live = (j >> 3 & 1) * 64u, old_word = kOld[j >> 4];
            const bool exh = (j >> 2 & 1) != 0;
            const Ref want = chain<CARRY>(a, busyS, busyV, exh, live, old_word);
            const W3Pick got = w3_policy_of<CARRY>(a, busyS, busyV, exh, live, old_word);
            ++*cases;
            ++kinds[want.kind];
            bool same = got.kind == want.kind;
            if (same && (want.kind == W3_VERTEX || want.kind == W3_SEGMENT || want.kind == W3_FRESH))
                same = got.q0 == want.q0 && got.n0 == want.n0 && got.n1 == want.n1 && (want.n1 == 0u || (got.q0 ^ 1u) == want.q1);
            if (!same && bad++ < 10)
                std::printf("CARRY %d avail {%u %u %u %u} busyS %u busyV %u exh %d live %u old %#x: chain {%u q%u %u q%u %u}, policy {%u q%u %u %u}\n",
                            (int)CARRY, a[0], a[1], a[2], a[3], busyS, busyV, (int)exh, live, old_word, want.kind, want.q0, want.n0, want.q1, want.n1,
                            got.kind, got.q0, got.n0, got.n1);
        }
    }
    return bad;
}

int main() {
    long cases = 0, kinds[5] = {0, 0, 0, 0, 0};
    const long bad = check<false>(&cases, kinds) + check<true>(&cases, kinds);
    std::printf("%ld cases (none %ld, vertex %ld, segment %ld, fresh %ld, exit %ld), %ld differ\n", cases, kinds[W3_NONE], kinds[W3_VERTEX], kinds[W3_SEGMENT],
                kinds[W3_FRESH], kinds[W3_EXIT], bad);
    for (int k = 0; k < 5; ++k)
        if (kinds[k] == 0) return 2;  // (every kind is reached, or the enumeration shows nothing about it)
    return bad == 0 ? 0 : 1;
}
