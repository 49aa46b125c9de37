// vspg_wg3.h -- k_render_wave_wg3: the workgroup kernel of vspg_wg_kernel.h WITHOUT workgroup barriers (round 5).
//
// k_render_wave_wg2 advances its pool in lock step -- [segment phase] barrier [vertex phase] barrier -- and the per-phase table of
// round 4 (profiles/r04_phase_profile_fog.txt) put 18 % of the wavefronts' time at those two barriers and 14 % in the scheduler
// between them: a phase lasts as long as its slowest 64-entry chunk, and the vertex phase has work for six of the eight
// wavefronts.  Here the lists are RING QUEUES in LDS and every wavefront is its own scheduler:
//
//   Q_VV / Q_VS  paths standing at a volume / surface vertex         -> vertex chunk  (NEE, Russian roulette, new direction)
//   Q_A          paths with a ray to follow (bit 15: the slot's pixel starts its next sample: multi-sample launches)
//                                                                     -> segment chunk (intersection, SampleDistance, event)
//   Q_F          free slots; 64 of them + one 8x8 pixel tile from the global tile head -> a chunk of camera rays
//
// A wavefront pops up to 64 entries from one queue (reserve with a compare-and-swap on the queue's head), runs the chunk, pushes
// every slot of it into the queue its path now belongs to (ballot + prefix count, one reserving atomic per queue, entries, one
// committing atomic) and looks for the next chunk -- it never waits for its seven siblings.  A consumer trusts entries only
// up to a commit count it has seen EQUAL to the reserve count (every reservation below it has then been written).
//
// Chunks stay FULL: a queue is served once it holds 64 entries; a partial chunk is taken only when the queue's producers are
// idle (vertex queues: no segment chunk in flight; Q_A: no vertex chunk in flight).  The pool holds MORE paths than the
// workgroup has lanes (the grey instantiations: 640 for 512 lanes; what k_render_wave_wg2 could not use -- its pool had to be
// a whole number of rounds of eight chunks) so that a wavefront that finishes a chunk finds a full one waiting: with seven
// siblings busy on 64 slots each, 640 - 448 = 192 slots sit in three kinds of queue, so one kind holds 64 (the two vertex
// queues count as one kind: a vertex chunk may take the rest of the smaller one and fill up from the other).
// Termination: the tile head has run dry and no slot holds a path (`live`, raised by 64 BEFORE a tile is claimed).
//
// Per path nothing changes: the operations, their order and the sampler dimensions are li_segment_a's and li_segment_b's, a
// finished path parks {L, ISG code} exactly as under k_render_wave_wg2 (deferred resolve, vspg_wg_sched.h): the three schedulers
// give the same film bit for bit (tests: test_workgroup_schedulers_are_bit_identical).
#pragma once
#include <type_traits>

#include "vspg_guided_wg.h"
#include "vspg_path.h"
#include "vspg_wg_kernel.h"

VSPG_NS_BEGIN

enum { Q_VV = 0, Q_VS = 1, Q_A = 2, Q_F = 3, Q_COUNT = 4 };
enum { QC_RES = 0, QC_COM = 1, QC_HEAD = 2, QC_STRIDE = 4 };
// (one 16-byte group behind the queues'.  The order serves the chunk's tail, see ring_push_all: OLD, BUSY_S, LIVE are three words in a
//  row and OLD, LIVE, BUSY_V three words two apart)
enum { W3_BUSY_S = Q_COUNT * QC_STRIDE, W3_LIVE, W3_EXH, W3_BUSY_V, W3_COUNT };
// CARRY, the spare words of the queue groups: resumed paths still in flight (+ kCarryDrainBit in a launch that suspends nothing: the
// word then never reads 0), and the suspend buffer's address -- parked in LDS over the persistent loop, whose SGPRs are all spoken for
enum { W3_OLD = Q_F * QC_STRIDE + 3, W3_SUSP_LO = Q_VS * QC_STRIDE + 3, W3_SUSP_HI = Q_A * QC_STRIDE + 3 };
static_assert(W3_BUSY_S == W3_OLD + 1 && W3_LIVE == W3_OLD + 2 && W3_BUSY_V == W3_OLD + 4, "the tail's three lanes reach their words by lane << shift");
constexpr unsigned kCarryDrainBit = 0x80000000u;
enum { W3_NONE = 0, W3_VERTEX = 1, W3_SEGMENT = 2, W3_FRESH = 3, W3_EXIT = 4 };
constexpr unsigned kRestartBit = 0x8000u;

// ---- the policy: which chunk a wavefront takes next --------------------------------------------------------------------------------
// Order: a FULL chunk of one kind (volume vertices, surface vertices, segments, a fresh tile) before a vertex chunk mixed from both
// vertex queues, before partial chunks (only while their producers idle), before the exit.  A queue's `avail` is its committed
// entries nobody has claimed, 0 while a push is between its reservation and its commit, and 0 for Q_F once the tile cursors are dry.
// The kernel does not hold the four `avail` as scalars: lane q computes queue q's, two ballots give `full` (bit q: avail >= 64) and
// `any` (bit q: avail > 0), and everything else is FETCHED where a branch needs it -- avail(q) only for a queue whose `any` bit is
// set, the shared words only by the partial, exit and suspend branches.  A host test walks the same function over plain arrays
// (tests/test_wg3_policy.py).
struct W3Pick {
    unsigned kind, q0, n0, n1;  // ask n0 entries of queue q0; a vertex chunk asks n1 more of the other vertex queue, q0 ^ 1
};
enum { W3S_BUSY_S = 0, W3S_BUSY_V, W3S_LIVE, W3S_OLD };
template <bool CARRY, class Avail, class Shared>
VSPG_HD W3Pick w3_policy(unsigned full, unsigned any, bool exh, Avail avail, Shared shared) {
    // CARRY: the cursors are dry and every resumed path has ended -- the workgroup suspends what it holds (behind the loop)
    if (CARRY && exh && shared(W3S_OLD) == 0u) return W3Pick{W3_EXIT, Q_VV, 0u, 0u};
    // a full chunk: the queues' numbers are their rank here (Q_VV, Q_VS, Q_A, Q_F), so the lowest set bit names the one to serve
    if (full != 0u) {
        const unsigned q = (unsigned)__builtin_ctz(full);
        return W3Pick{q <= (unsigned)Q_VS ? (unsigned)W3_VERTEX : q == (unsigned)Q_A ? (unsigned)W3_SEGMENT : (unsigned)W3_FRESH, q, 64u, 0u};
    }
    if (any & (1u << Q_VV | 1u << Q_VS)) {
        // (both below 64 here) the larger queue first; a chunk it cannot fill takes the rest from the other one
        const unsigned aVV = any & (1u << Q_VV) ? avail(Q_VV) : 0u, aVS = any & (1u << Q_VS) ? avail(Q_VS) : 0u;
        if (aVV + aVS >= 64u || shared(W3S_BUSY_S) == 0u) {
            const unsigned first = aVV >= aVS ? aVV : aVS, second = aVV >= aVS ? aVS : aVV;
            return W3Pick{W3_VERTEX, aVV >= aVS ? (unsigned)Q_VV : (unsigned)Q_VS, first, second < 64u - first ? second : 64u - first};
        }
    }
    if ((any & (1u << Q_A)) && shared(W3S_BUSY_V) == 0u) return W3Pick{W3_SEGMENT, Q_A, avail(Q_A), 0u};
    if (exh && shared(W3S_LIVE) == 0u) return W3Pick{W3_EXIT, Q_VV, 0u, 0u};
    return W3Pick{W3_NONE, Q_VV, 0u, 0u};
}
// ... from the four `avail` and the five shared words as plain values (the form a test can enumerate)
template <bool CARRY>
VSPG_HD W3Pick w3_policy_of(const unsigned a[Q_COUNT], unsigned busyS, unsigned busyV, bool exh, unsigned live, unsigned old_word) {
    unsigned full = 0u, any = 0u;
    for (int q = 0; q < Q_COUNT; ++q) {
        const unsigned aq = q == Q_F && exh ? 0u : a[q];
        full |= (aq >= 64u ? 1u : 0u) << q;
        any |= (aq > 0u ? 1u : 0u) << q;
    }
    const unsigned words[4] = {busyS, busyV, live, old_word};
    return w3_policy<CARRY>(full, any, exh, [&](int q) { return a[q]; }, [&](int w) { return words[w]; });
}

// ISG code of a finished sample, one float: 0 = no ISG record, +q = volume event, -q = surface event, q = the VSP the primary
// segment used (or 0.5): q lies in [0.001, 0.999], so the sign is free and nothing is rounded
VDEV float isg_code(const IsgSample &isg) {
    if (!isg.valid) return 0.f;
    const float q = isg.vsp_used >= 0.f ? isg.vsp_used : 0.5f;
    return isg.surface_event ? -q : q;
}
// one parked sample {L, ISG code} into the film and the image-space statistics (RGBFilm::AddSample + ISG AddSample, the
// read-modify-write forms: one writer per pixel)
__device__ __forceinline__ void resolve_sample(float4 s, float4 *film_px, float *isg_px) {
    const Spec L = Spec{s.x, s.y, s.z};
    film_add_sample_rmw(film_px, L);
    IsgSample isg;
    isg.valid = s.w != 0.f;
    isg.surface_event = s.w < 0.f;
    isg.vsp_used = __builtin_fabsf(s.w);
    isg_add_sample_rmw(isg_px, L, isg);
}
// ... given the film pixel and the statistics already loaded (a FRESH chunk loads them with the parked sample, in one round trip):
// the additions, their operands and their order are film_add_sample_rmw's and isg_add_sample_rmw's
__device__ __forceinline__ void resolve_sample_loaded(float4 s, float4 fpx, float4 st03, float2 st45, float4 *film_px, float *isg_px) {
    const Spec L = Spec{s.x, s.y, s.z};
    film_store_sample(film_px, fpx, L);
    IsgSample isg;
    isg.valid = s.w != 0.f;
    isg.surface_event = s.w < 0.f;
    isg.vsp_used = __builtin_fabsf(s.w);
    isg_store_sample(isg_px, st03, st45, L, isg);
}
// Every load issued so far has arrived behind this point: the values are named as inputs, so the compiler can neither sink a load
// into the branch that uses it (a second round trip behind the first) nor wait for them one by one.
__device__ __forceinline__ void w3_loads_arrived(float4 a, float4 b, float4 c, float2 d, float e) {
    asm volatile("" ::"v"(a.x), "v"(a.y), "v"(a.z), "v"(a.w), "v"(b.x), "v"(b.y), "v"(b.z), "v"(b.w), "v"(c.x), "v"(c.y), "v"(c.z), "v"(c.w), "v"(d.x),
                 "v"(d.y), "v"(e));
}
// An opaque copy of a kernel argument at its point of use.  A wave-uniform flag tested inside the persistent loop is otherwise
// turned into a 64-bit lane mask once, before the loop, and held there (one pair per test: `single_sample` took two); with more live
// values than SGPRs those pairs are spilled to VGPR lanes and read back at every use.  The opaque copy keeps the 32-bit argument
// live instead and forms the mask where it is used.  Integers and pointers only: no float passes through it.
template <class T>
__device__ __forceinline__ T w3_at_use(T v) {
    asm volatile("" : "+s"(v));
    return v;
}
// The lane index, opaque in the same way: a compare of it (`lane == 0`, `lane < Q_COUNT`) is a lane mask, an SGPR pair, which the
// compiler would otherwise form once before the persistent loop and hold for the whole kernel.
__device__ __forceinline__ int w3_lane() {
    int l = (int)(threadIdx.x & 63u);
    asm volatile("" : "+v"(l));
    return l;
}
// ---- CARRY: in-flight paths cross the boundary between two one-sample launches -----------------------------------------------
// A self-contained launch ends with every workgroup draining its pool through ever thinner chunks on a chip that empties
// (profiles/carry_drain_profile.txt: the last exit comes ~118 us after the median wavefront sees the cursors dry, of a 639 us
// launch), and the next one starts from empty pools.  In CARRY mode (k_render_wave_wg3_carry, launched by vspg_render_window where
// the deferred resolve applies) a workgroup whose cursors are dry SUSPENDS instead: it writes pool, rings and queue words -- its
// image -- to global memory, and the same workgroup of the next launch RESUMES from it, with a full pool and the scheduler's state as
// it was.  The contract is the parked samples': nothing reads the film between two such launches; whoever does drains first
// (vspg_capi.hip: drain_carried_paths, a CARRY launch without tiles and without a suspend buffer; flush_parked_samples runs it first).
//   * a resumed path is told by its sample index (SAMPLE != first_sample); when it ends it adds its sample to the film and the
//     statistics itself (resolve_sample) and lowers `old_live`.  In the drain launch (first_sample < 0) it PARKS the sample
//     instead, over its pixel's sentinel: what the drain leaves is the state a self-contained launch leaves, parked samples and
//     nothing else, for whoever resolves them next;
//   * for every path it suspends, a workgroup writes kCarrySentinel into the pixel's entry of this launch's wave_samples plane: the
//     next launch does not resolve that entry at the start of the pixel (k_film_resolve skips it too) -- the resumed path will.
//     So sample N of a pixel enters the film in launch N + 1 either way, once, and sample N + 1 no earlier than launch N + 2: the
//     additions per pixel keep their order and the film its bits;
//   * a workgroup suspends only once `old_live` is 0 (until then it serves every queue as ever): a path is carried at most once,
//     whatever the frame size, and every slot in flight at the suspension belongs to this launch.
//   * a launch whose step ends in an update of the VSP buffer (vspg_capi.hip predicts it) would be drained at once: it gets `resume`
//     and its tiles but NO suspend buffer.  The drain bit in `old_live` keeps the carry exit from firing, resumed paths add their
//     samples, new ones run to their ends and park, workgroups leave by the ordinary `exh && live == 0`: behind it nothing is
//     pending and the parked plane is complete.  What tells the drain launch (no tiles) is first_sample < 0, not the missing buffer.
// The image lies in global memory as it lies in LDS -- pool, rings, queue words -- and moves in 16-byte pieces, every load of the
// prologue in flight before the first LDS write (profiles/wave_boundary_static.txt).
// The free ring and the claimed-unread hazard (see the FRESH claim below): a resumed ring is no longer "full from index 0", it is a
// ring on a later lap, which the same argument already covers -- the claimed entries are read right behind the CAS, and a sibling
// would have to claim, run a chunk and push within those few instructions.  The queue words are rebased on resume (HEAD < NP), so
// ring positions never come near 2^32 however many launches pass between two drains.
constexpr float kCarrySentinel = 2.f;  // (a legal ISG code lies in [-0.999, 0.999])
__device__ __forceinline__ bool carry_sentinel(float w) { return w > 1.f; }
template <class LY, int NP> constexpr int kWg3ImagePool = LY::COUNT * NP;                 // dwords: the pool,
template <class LY, int NP> constexpr int kWg3ImageWords = LY::COUNT * NP + Q_COUNT * NP / 2;  // ... the four rings, then the queue words
template <class LY, int NP> constexpr int kWg3ImageStride = kWg3ImageWords<LY, NP> + 32;  // per workgroup
static_assert(W3_COUNT <= 32, "the image's queue words");
// piece i of an image of N 16-byte pieces, or the last one for a lane past the end: its load stays inside the image, nothing is stored
template <int N> __device__ __forceinline__ int w3_image_piece(int i) { return i < N ? i : N - 1; }

constexpr int kWg3Heads = 8, kWg3HeadSetBytes = kWg3Heads * 128;  // k_render_wave_wg3's tile cursors (see the kernel)
// The global work head is a PAIR of counters used by alternate launches: a launch zeroes the one the NEXT launch will use
// (nobody reads it meanwhile, launches of a renderer are stream-ordered), so no memset sits between two waves.
__device__ __forceinline__ void reset_sibling_head(unsigned int *work_head) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *reinterpret_cast<unsigned int *>(reinterpret_cast<uintptr_t>(work_head) ^ 4u) = 0u;
}

// The scheduler's words in LDS: per queue {reserved, committed, head, -} and {segment chunks in flight, slots holding a path, tile
// head dry, vertex chunks in flight}, each group 16 bytes.  A deciding wavefront reads them with TWO back-to-back 128-bit LDS reads and
// one wait: lane q (and q + 4, ...) its queue's group, every lane the shared one.  A 128-bit read is one LDS instruction:
// {reserved, committed, head} are a snapshot.
typedef unsigned int w3_u32x4 __attribute__((ext_vector_type(4)));
typedef const volatile __attribute__((address_space(3))) w3_u32x4 *w3_lds_v4;
typedef __attribute__((address_space(1))) w3_u32x4 *w3_glb_v4;
// Every lane hands its slot to the queue its path now belongs to (dq in [0, Q_COUNT), or -1: none): the four reservations are ONE
// returning LDS atomic (lane q reserves for queue q), then the entries, then the four commits as one atomic -- and then the chunk's
// tail, ONE more: lanes 0-2 lower {OLD, BUSY_S, LIVE} (a segment chunk, tail_shift 0) or {OLD, LIVE, BUSY_V} (a vertex chunk,
// tail_shift 1) by {n_old, 1, slots freed}.  The slots freed are the lanes that push to Q_F: nobody else does.
//
// Why the tail may be one instruction, and why it stays BEHIND the commits.  LDS serves a wavefront's instructions in order, so a
// sibling that sees any of the tail's new values can see the commits too; but a sibling READS the queue groups before (never after)
// the shared group, so it may pair a queue's words from before this push with counters from after it.  Each such pairing makes it
// take less, never more:
//   * old queue words, read before the reservation: RES == COM, every entry it counts is an older, committed one;
//   * read between reservation and commit: RES != COM, the queue counts as empty;
//   * BUSY_S / BUSY_V lower than the entries it sees justify: it takes a partial chunk that could have been fuller;
//   * LIVE == 0 or OLD == 0 are seen only behind the commits of the last pushes (this order), so a wavefront that exits or
//     suspends on them leaves no push outstanding -- its own is committed before it polls, a sibling's before that sibling
//     lowers the word.  Words that lag (the tail's lanes need not land together) only delay the exit: all three only fall.
// Riding in the commit atomic itself (lanes 4-6) would be as safe by the same argument but needs a per-lane select of address and
// operand, more vector instructions than the second atomic's two.
template <int NP>
VDEV void ring_push_all(int dq, unsigned entry, unsigned short (*ring)[NP], unsigned int *s_w, unsigned n_old, int tail_shift) {
    const int lane = w3_lane();
    const unsigned lane8 = (unsigned)lane << 3;
    asm volatile("" : "+v"(dq));  // (one register, four compares: the compiler would otherwise rebuild each predicate from the callers' flags)
    // (the ballot of a predicate, not of an integer: the four masks are the compares' own results, no select-and-compare in between)
    // (a vertex chunk pushes to Q_A and Q_F only: tail_shift is a constant where this is inlined, and the vertex queues' half drops out)
    const unsigned long long m0 = tail_shift ? 0ull : __builtin_amdgcn_ballot_w64(dq == 0), m1 = tail_shift ? 0ull : __builtin_amdgcn_ballot_w64(dq == 1);
    const unsigned long long m2 = __builtin_amdgcn_ballot_w64(dq == 2), m3 = __builtin_amdgcn_ballot_w64(dq == 3);
    // the four counts (<= 64 each) in the bytes of one scalar: lane q picks its own with one bit-field extract.  A queue that gets
    // nothing is reserved and committed by 0 -- the atomics run for four lanes either way, and `myn > 0` was a compare and a mask more.
    const unsigned n3 = (unsigned)__popcll(m3);
    const unsigned counts = (unsigned)__popcll(m0) | (unsigned)__popcll(m1) << 8 | (unsigned)__popcll(m2) << 16 | n3 << 24;
    const unsigned myn = __builtin_amdgcn_ubfe(counts, lane8, 8u);
    unsigned base = 0;
    if (lane < Q_COUNT) base = atomicAdd(s_w + lane * QC_STRIDE + QC_RES, myn);
    // reserved base + the lane's rank among its queue's lanes: v_mbcnt takes the ballot from scalar registers and the base as its addend,
    // two instructions per queue; the lane's own queue picks one of the four sums (the ballots again, as the selects' masks)
    const auto at = [&](unsigned long long m, int q) {
        const unsigned b = (unsigned)__builtin_amdgcn_readlane((int)base, q);
        return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, b));
    };
    const unsigned p2 = at(m2, 2), p3 = at(m3, 3);
    unsigned pos = dq == 2 ? p2 : p3;
    if (!tail_shift) {
        const unsigned p0 = at(m0, 0), p1 = at(m1, 1);
        pos = dq == 0 ? p0 : dq == 1 ? p1 : pos;
    }
    if (dq >= 0) (&ring[0][0])[__umul24((unsigned)dq, (unsigned)NP) + pos % (unsigned)NP] = (unsigned short)entry;  // ring[dq][pos % NP]
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // the entries (and the pool records behind them) before the commits
    if (lane < Q_COUNT) atomicAdd(s_w + lane * QC_STRIDE + QC_COM, myn);
    const unsigned tail = tail_shift ? n_old | n3 << 8 | 1u << 16 : n_old | 1u << 8 | n3 << 16;
    // (a subtracting atomic by name: atomicSub adds the negated operand, one more instruction)
    if (lane < 3) (void)__hip_atomic_fetch_sub(s_w + W3_OLD + (lane << tail_shift), __builtin_amdgcn_ubfe(tail, lane8, 8u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

#ifndef VSPG_WG3_IDLE_SLEEP
#define VSPG_WG3_IDLE_SLEEP 8   // s_sleep argument (x 64 clocks) of a wavefront that found no chunk twice in a row
#endif
#ifndef VSPG_WG3_NP_CAP
#define VSPG_WG3_NP_CAP 768
#endif
#ifndef VSPG_WG3_LDS_BUDGET
#define VSPG_WG3_LDS_BUDGET 81920
#endif
#ifndef VSPG_WG3_OTHER
#define VSPG_WG3_OTHER 5200   // scene records, libm tables, counters, queue words beside the pool and the rings (5104 B measured)
#endif
// paths per pool: what fits the LDS a workgroup may use when two share a CU -- the record, four ring entries per path, `other`
// bytes (scene records, counters, staged kd nodes); a multiple of 32
template <class LY>
constexpr int wg3_pool_paths(int other_bytes) {
    const int n = (VSPG_WG3_LDS_BUDGET - other_bytes) / (LY::COUNT * 4 + Q_COUNT * 2) / 32 * 32;
    return n < VSPG_WG3_NP_CAP ? n : VSPG_WG3_NP_CAP;
}

// Diagnostic build only (-DVSPG_W3_TIMELINE, csrc/Makefile target `timeline`; scripts/carry_drain_profile.py reads it): per wavefront
// of the last launch, 100 MHz stamps of {loop entry, first full vertex chunk, cursors first seen dry, exit} and, for each of the three
// phases these stamps bound (ramp, steady, drain) and each chunk kind (vertex, segment, fresh), {chunks, lanes, ticks in chunks}.
// The shipped library contains none of this.
#ifdef VSPG_W3_TIMELINE
enum { W3T_BEGIN = 0, W3T_FULL, W3T_EXH, W3T_EXIT, W3T_SUMS, W3T_WORDS = W3T_SUMS + 27, W3T_MAX_BLOCKS = 2048 };
__device__ unsigned long long g_w3_timeline[W3T_MAX_BLOCKS][8][32];
struct W3Timeline {
    unsigned long long *rec, t0;
    unsigned phase;
    __device__ __forceinline__ bool mine() const { return (threadIdx.x & 63u) == 0u && blockIdx.x < (unsigned)W3T_MAX_BLOCKS; }
    __device__ __forceinline__ W3Timeline() : rec(&g_w3_timeline[blockIdx.x % W3T_MAX_BLOCKS][(threadIdx.x >> 6) & 7u][0]), t0(0), phase(0) { stamp(W3T_BEGIN); }
    __device__ __forceinline__ void stamp(int i) { const unsigned long long t = __builtin_amdgcn_s_memrealtime(); if (mine()) rec[i] = t; }
    __device__ __forceinline__ void enter(unsigned p, int i) { if (phase < p) { phase = p; stamp(i); } }
    __device__ __forceinline__ void chunk_begin() { t0 = __builtin_amdgcn_s_memrealtime(); }
    __device__ __forceinline__ void chunk_end(unsigned kind, unsigned lanes) {
        const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
        if (mine()) {
            unsigned long long *r = rec + W3T_SUMS + (phase * 3u + kind) * 3u;
            atomicAdd(r, 1ull); atomicAdd(r + 1, (unsigned long long)lanes); atomicAdd(r + 2, t1 - t0);
        }
    }
};
#define VSPG_W3T(x) x
#else
#define VSPG_W3T(x)
#endif

// The kernel's body.  WINDOW: the launch covers the pixel window `win` (vspg_render_window) instead of the frame.  The 8x8 tile grid stays
// anchored to the frame; the launch enumerates the tile rectangle that covers the window (tile index -> window-local row / column, plus
// the rectangle's origin) and masks the lanes outside the window the way the full-frame launch masks lanes past W / H.  The full-frame
// instantiation takes none of it: `win` is unused there and its code is what it was (it is pinned at its SGPR limit and within five
// selects / compares of its ceiling, tests/test_headline_kernel_census.py).
template <class Medium, bool GUIDED, int NP, int kWgBlock, int kWgWavesPerSimd, bool TRAIN, bool WINDOW, bool CARRY = false>
__device__ __forceinline__ void wg3_render(
    const DScene *__restrict__ Sp, float4 *__restrict__ film, float *__restrict__ isg_stats, const float *__restrict__ vsp_buf,
    int vsp_ready, int wave_end, int first_sample, int single_sample, PcgJump jump, unsigned int tiles_magic,
    unsigned int *__restrict__ work_head, const float4 *__restrict__ prev_samples,
    float4 *__restrict__ wave_samples, unsigned long long *__restrict__ counters, TrainArgs train, const PixelWindow win,
    const unsigned int *__restrict__ resume = nullptr, unsigned int *__restrict__ suspend = nullptr) {
    static_assert(!CARRY || (!TRAIN && !GUIDED), "CARRY serves the unguided one-sample launches");
    // (each argument its own register from here on: the four ints arrive as one 128-bit load, and a tuple is spilled as a unit)
    vsp_ready = w3_at_use(vsp_ready), wave_end = w3_at_use(wave_end), first_sample = w3_at_use(first_sample);
    single_sample = w3_at_use(single_sample);
    const DScene &S = *Sp;
    const int W = S.xres, H = S.yres;
    const int tilesX = WINDOW ? win_tiles_x(win) : (W + 7) >> 3, tilesY = WINDOW ? win_tiles_y(win) : (H + 7) >> 3;
    // (CARRY with first_sample < 0 is the drain launch: no tiles, the resumed paths run to their ends)
    const unsigned n_tiles = CARRY && w3_at_use(first_sample) < 0 ? 0u : (unsigned)(tilesX * tilesY);
    // is pixel (px, py) of a claimed tile part of the launch?  (tile padding past the frame / outside the window)
    const auto in_launch = [&](int px, int py) {
        if constexpr (WINDOW) return win_has(win, px, py);
        else return px < W && py < H;
    };
    const int lane = threadIdx.x & 63;
    const int sample_step = S.shard_count > 1 ? S.shard_count : 1;
    // The tile head: kWg3Heads cursors, each on a 128-byte line of its own, cursor k handing out tiles k, k + kWg3Heads, ...  One cursor
    // was a returning atomic per 8x8 tile on ONE address -- 32 400 of them per 1080p launch, at the ~88 per microsecond a hot word
    // serves more than half the kernel's time in the atomic unit's queue.  A wavefront starts at its workgroup's cursor (workgroups go
    // round the XCDs) and moves on when one has run out (it looks before it asks: cursors only grow).  The heads are a PAIR of sets
    // used by alternate launches, 1 KB apart: a launch zeroes the set the next one will use (reset_sibling_head's scheme).
    if (blockIdx.x == 0 && threadIdx.x < (unsigned)kWg3Heads)
        reinterpret_cast<unsigned int *>(reinterpret_cast<uintptr_t>(work_head) ^ (uintptr_t)kWg3HeadSetBytes)[threadIdx.x * 32u] = 0u;
    unsigned wseg = blockIdx.x % (unsigned)kWg3Heads, wtried = 0u;

    constexpr bool FULL = !Medium::kSimpleScene;
    static_assert(!FULL || !GUIDED, "the workgroup kernel's guided vertex (vspg_guided_wg.h) is built for rectangle scenes");
    static_assert(NP < (int)kRestartBit, "a ring entry is the slot plus the restart bit");
    using LY = PoolLayout<GUIDED, Medium::kGrey, TRAIN, FULL>;
    constexpr int NF = LY::COUNT;
    static_assert(!TRAIN || GUIDED, "segment recording belongs to the guided instantiations");
    static_assert(Medium::kSingleSegment, "k_render_wave_wg3 serves homogeneous media (grid media: the wavefront pipeline)");
    __shared__ __attribute__((aligned(16))) float s_pool[NF * NP];                  // (16 bytes: CARRY copies both in 128-bit pieces)
    __shared__ __attribute__((aligned(16))) unsigned short s_ring[Q_COUNT][NP];
    __shared__ __attribute__((aligned(16))) unsigned int s_w[W3_COUNT];
    const Pool P{s_pool, NP};
    const Medium medium = MediumMaker<Medium>::make(S, nullptr);
    float *glds = nullptr;
    if constexpr (GUIDED && kKdLdsNodes > 0) {  // the upper levels of the two kd-trees (north star: "LDS-staged kd-tree nodes")
        __shared__ VspgKdNode s_kd[2][kKdLdsNodes > 0 ? kKdLdsNodes : 1];
        for (int f = 0; f < 2; ++f) {
            const int nl = S.field[f].n_nodes < kKdLdsNodes ? S.field[f].n_nodes : kKdLdsNodes;
            for (int i = threadIdx.x; i < nl; i += kWgBlock) s_kd[f][i] = S.field[f].nodes[i];
        }
        glds = reinterpret_cast<float *>(&s_kd[0][0]);
    }
    __shared__ unsigned int s_counters[CNT_COUNT];
    struct LaneCounters : PathCounters { uint32_t paths; VDEV void path() { paths++; } };
    using Rec = typename std::conditional<TRAIN, PathRecorder, NullRecorder>::type;
    typename std::conditional<GUIDED, WaveCountersT<Rec>, LaneCounters>::type pc = [&] {
        if constexpr (GUIDED) { WaveCountersT<Rec> c; c.c = s_counters; return c; }
        else { LaneCounters c; c.segments = c.volume_scatters = c.surface_hits = c.density_queries = c.shadow_rays = c.shadow_queries = c.paths = 0; return c; }
    }();
    // a18, training launches (one sample per pixel): a path's records go to ITS column of the wave's record buffer -- the
    // column of its work item, which the pixel names (tile-ordered items: vspg_render_wave sizes the buffer by them)
    const auto rec_bind = [&](int pxy) {
        if constexpr (TRAIN) {
            const unsigned px = (unsigned)pxy & 0xffffu, py = (unsigned)pxy >> 16;
            const unsigned tcol = WINDOW ? (px >> 3) - (unsigned)win_tile_x0(win) : px >> 3, trow = WINDOW ? (py >> 3) - (unsigned)win_tile_y0(win) : py >> 3;
            const unsigned item = (trow * (unsigned)tilesX + tcol) * 64u + ((py & 7u) << 3) + (px & 7u);
            pc.rec.base = train.segbuf + item;
            pc.rec.stride = (int)train.n_items;
            pc.rec.max_seg = train_rec_capacity(S.prm.maxdepth);
            return item;
        } else {
            (void)pxy;
            return 0u;
        }
    };

    stage_scene_lds(S);
    if (threadIdx.x < CNT_COUNT) s_counters[threadIdx.x] = 0;
    constexpr int kImgPool = kWg3ImagePool<LY, NP>, kImgWords = kWg3ImageWords<LY, NP>, kImgStride = kWg3ImageStride<LY, NP>;
    // the image moves in 16-byte pieces, pool then rings: kImgRounds per lane, the last round partly past the end
    constexpr int kImgPieces = kImgWords / 4, kImgRounds = (kImgPieces + kWgBlock - 1) / kWgBlock;
    static_assert(kImgPool % 4 == 0 && (Q_COUNT * NP / 2) % 4 == 0 && kImgStride % 4 == 0, "pool, ring block and stride of an image: multiples of 16 bytes");
    w3_u32x4 *const pool4 = reinterpret_cast<w3_u32x4 *>(s_pool), *const ring4 = reinterpret_cast<w3_u32x4 *>(&s_ring[0][0]);
    const int img_lane = (int)threadIdx.x;
    __builtin_assume(img_lane >= 0 && img_lane < kWgBlock);  // (the launch bounds: only the last round of the copies tests its index)
    bool resumed = false;
    if constexpr (CARRY) {
        // RESUME: the workgroup's image of the previous launch, verbatim, if it holds paths
        const unsigned int *const img = resume + (size_t)blockIdx.x * kImgStride;
        resumed = resume != nullptr && img[kImgWords + W3_LIVE] != 0u;
        if (resumed) {
            // (pool and rings lie in the image as they lie in LDS: 16-byte pieces, every load in flight before the first LDS write)
            const w3_u32x4 *const img4 = reinterpret_cast<const w3_u32x4 *>(img);
            w3_u32x4 piece[kImgRounds];
#pragma unroll
            for (int k = 0; k < kImgRounds; ++k) piece[k] = img4[w3_image_piece<kImgPieces>(img_lane + k * kWgBlock)];
            const unsigned qword = img[kImgWords + (img_lane < W3_COUNT ? img_lane : 0)];  // (the queue words, the same way)
            asm volatile("" ::"v"(piece[kImgRounds - 1]), "v"(qword));  // (the partial round's loads leave with the others, not inside their branches)
#pragma unroll
            for (int k = 0; k < kImgRounds; ++k) {
                const int i = img_lane + k * kWgBlock;
                if (i < kImgPieces) *(i < kImgPool / 4 ? pool4 + i : ring4 + (i - kImgPool / 4)) = piece[k];
            }
            if (threadIdx.x < W3_COUNT) s_w[threadIdx.x] = qword;
            __syncthreads();
            // what belongs to the launch: every resumed path is an old one, the cursors are this launch's (a drain launch has none),
            // no chunk is in flight; ring positions rebased below NP
            if (threadIdx.x < Q_COUNT) {
                const unsigned h = s_w[threadIdx.x * QC_STRIDE + QC_HEAD], n = s_w[threadIdx.x * QC_STRIDE + QC_COM] - h, h2 = h % (unsigned)NP;
                s_w[threadIdx.x * QC_STRIDE + QC_HEAD] = h2;
                s_w[threadIdx.x * QC_STRIDE + QC_RES] = h2 + n;
                s_w[threadIdx.x * QC_STRIDE + QC_COM] = h2 + n;
            }
            if (threadIdx.x == 0) {
                s_w[W3_OLD] = s_w[W3_LIVE];
                s_w[W3_EXH] = 0u;
                s_w[W3_BUSY_S] = 0u;
                s_w[W3_BUSY_V] = 0u;
            }
        }
    }
    if (!resumed) {
        if (threadIdx.x < W3_COUNT) s_w[threadIdx.x] = 0;
        for (int i = threadIdx.x; i < NP; i += kWgBlock) s_ring[Q_F][i] = (unsigned short)i;
        __syncthreads();
        if (threadIdx.x == 0) {
            s_w[Q_F * QC_STRIDE + QC_RES] = NP; s_w[Q_F * QC_STRIDE + QC_COM] = NP;
        }
    }
    if constexpr (CARRY) {
        __syncthreads();
        if (threadIdx.x == 0) {
            // nothing is suspended: the drain launch (no tiles either), and the launch an update of the VSP buffer follows -- its
            // tiles as ever, the resumed paths to their ends, every workgroup out by the ordinary `exh && live == 0`
            if (suspend == nullptr) s_w[W3_OLD] |= kCarryDrainBit;
            if (first_sample < 0) s_w[W3_EXH] = 1u;
            s_w[W3_SUSP_LO] = (unsigned)reinterpret_cast<uintptr_t>(suspend);
            s_w[W3_SUSP_HI] = (unsigned)(reinterpret_cast<uintptr_t>(suspend) >> 32);
        }
    }
    __syncthreads();

    // a path ends: its sample leaves the kernel
    // (CARRY, `old`: a resumed path -- its sample goes where the next launch would have put it, see the header)
    auto emit = [&](int pxy, Spec Lraw, const IsgSample &isg, bool old) {
        const Spec L = finish_radiance(Lraw);
        const size_t pidx = (size_t)((unsigned)pxy >> 16) * W + (pxy & 0xffff);
        if (CARRY && old && w3_at_use(first_sample) >= 0) {
            resolve_sample(make_float4(L.r, L.g, L.b, isg_code(isg)), film + pidx, isg_stats + pidx * VSPG_ISG_STATS);
        } else if (w3_at_use(single_sample)) {
            wave_samples[pidx] = make_float4(L.r, L.g, L.b, isg_code(isg));
        } else {
            film_add_sample(film + pidx, L);
            isg_add_sample_atomic(isg_stats + pidx * VSPG_ISG_STATS, L, isg);
        }
    };

    VSPG_PROF(PS_WG_TOTAL);
    VSPG_PROF_ACC(prof_decide, PS_WG_R);      // diagnostic build: the scheduler (decisions that found a chunk)
    VSPG_PROF_ACC(prof_idle, PS_WG_BAR_A);    // ... and the polls that found none, the sleep included
    unsigned idle_polls = 0;
    VSPG_W3T(W3Timeline tl);
    while (true) {
        VSPG_PROF_ACC_BEGIN(prof_decide);
        VSPG_PROF_ACC_BEGIN(prof_idle);
        // ---- this wavefront's next chunk -----------------------------------------------------------------
        // Lane q reads queue q's 16-byte group and every lane the shared one: two LDS reads, one wait.  Lane q computes its queue's
        // `avail` in vector code, two ballots turn the four into two 4-bit scalar masks, and the policy (w3_policy, above) is scalar
        // bit tests -- the kernel is bound by vector issue, and a wavefront polls here while its siblings compute.  Making scalars of
        // all seventeen words first was sixteen v_readfirstlane a poll; now the policy fetches what its branch needs.
        // Lane 0 performs the claims.
        unsigned kind = W3_NONE, pos0 = 0, n0 = 0, pos1 = 0, n1 = 0, q0 = Q_VV, tile = 0;
        unsigned fresh_entry = 0;  // a FRESH chunk's free-ring entry of this lane
        {
            const auto U = [](unsigned v) { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); };
            const w3_lds_v4 qw = (w3_lds_v4)(s_w);
            const auto L = [](unsigned v, unsigned l) { return (unsigned)__builtin_amdgcn_readlane((int)v, (int)l); };
            // (both addresses in registers before the first read: built behind it, the second one landed in a register of the first read's
            //  result and waited for it -- two round trips)
            w3_lds_v4 pq = qw + (lane & 3), pm = qw + Q_COUNT;
            asm volatile("" : "+v"(pq), "+v"(pm));
            const w3_u32x4 wq = *pq, wM = *pm;  // (the queue groups BEFORE the shared one: ring_push_all's argument rests on it)
            const bool exh = U(wM.z) != 0u;
            VSPG_W3T(if (exh) tl.enter(2u, W3T_EXH));
            // lane q: queue q's committed entries nobody has claimed; they count only while no push stands between its reservation and
            // its commit.  Q_F is not served once the tile cursors are dry.
            // (one select, then each ballot is ONE compare's own mask: a ballot of `whole && ...` is built from a 0 / 1 value instead)
            const int a = wq.x == wq.y ? (int)(wq.y - wq.z) : 0;
            const unsigned served = exh ? (1u << Q_F) - 1u : (1u << Q_COUNT) - 1u;
            const unsigned full = (unsigned)__builtin_amdgcn_ballot_w64(a >= 64) & served;
            const unsigned any = (unsigned)__builtin_amdgcn_ballot_w64(a > 0) & served;
            const W3Pick pick = w3_policy<CARRY>(
                full, any, exh, [&](int q) { return L((unsigned)a, (unsigned)q); },
                [&](int w) { return w == W3S_OLD ? L(wq.w, Q_F) : U(w == W3S_BUSY_S ? wM.x : w == W3S_BUSY_V ? wM.w : wM.y); });
            const auto claim = [&](unsigned q, unsigned head, unsigned n) {  // compare-and-swap on the queue's head: this wavefront owns [head, head + n)
                unsigned old = head + 1u;
                if (w3_lane() == 0) old = atomicCAS(s_w + q * QC_STRIDE + QC_HEAD, head, head + n);
                return U(old) == head;
            };
            const auto bump = [&](int w, int d) { if (w3_lane() == 0) atomicAdd(s_w + w, (unsigned)d); };
            // a fresh claim's two words, BUSY_S by 1 and LIVE by 64, neighbours in LDS: one atomic with two lanes, either way
            const auto bump_fresh = [&](bool up) {
                const int l = w3_lane();
                if (l < 2) {
                    const unsigned d = __umul24((unsigned)l, 63u) + 1u;  // 1, 64
                    if (up) atomicAdd(s_w + W3_BUSY_S + l, d);
                    else atomicSub(s_w + W3_BUSY_S + l, d);
                }
            };
            // (only the chosen queue's head becomes a scalar: the claims' compare value and the chunk's ring position)
            if (pick.kind == W3_EXIT) {
                kind = W3_EXIT;
            } else if (pick.kind == W3_VERTEX) {
                bump(W3_BUSY_V, 1);
                // (both vertex heads from constant lanes and a scalar select: a lane index held in a register goes through a VGPR)
                const unsigned hVV = L(wq.z, Q_VV), hVS = L(wq.z, Q_VS);
                const unsigned h_first = pick.q0 == Q_VV ? hVV : hVS, h_second = pick.q0 == Q_VV ? hVS : hVV;
                if (claim(pick.q0, h_first, pick.n0)) {
                    kind = W3_VERTEX; q0 = pick.q0; pos0 = h_first; n0 = pick.n0;
                    if (pick.n1 > 0u && claim(pick.q0 ^ 1u, h_second, pick.n1)) { pos1 = h_second; n1 = pick.n1; }
                } else {
                    bump(W3_BUSY_V, -1);
                }
            } else if (pick.kind == W3_SEGMENT) {
                bump(W3_BUSY_S, 1);
                const unsigned hA = L(wq.z, Q_A);
                if (claim(Q_A, hA, pick.n0)) { kind = W3_SEGMENT; pos0 = hA; n0 = pick.n0; }
                else bump(W3_BUSY_S, -1);
            } else if (pick.kind == W3_FRESH) {
                bump_fresh(true);  // LIVE BEFORE the tile is claimed: `live == 0` then says nobody can still start a path
                const unsigned hF = L(wq.z, Q_F);
                if (claim(Q_F, hF, 64u)) {
                    kind = W3_FRESH; pos0 = hF; n0 = 64u;
                    // The claimed entries are read HERE, before the tile cursors are asked.  The free ring starts full (RES = COM = NP), so a
                    // sibling that claims the next 64 entries, ends paths and pushes their slots writes at index NP % NP = 0 onwards: over
                    // entries claimed but not read yet, if the reader is still going round dry cursors (small images and small windows: the
                    // cursors run dry in the first lap; on a later lap a claimed-unread chunk plus NP - 64 outstanding pushes reaches it the
                    // same way).  A slot would then be handed out twice.  Read at once, the window shrinks from the whole cursor loop to
                    // the few instructions between the CAS and this LDS read, in which a sibling would have to claim, run a segment and
                    // push.  That is a timing argument, not an ordering guarantee: rings 2 * NP deep or a producer-side RES - HEAD < NP
                    // check would exclude it by construction (DESIGN.md 4.5 says what they cost).
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                    fresh_entry = s_ring[Q_F][(hF + (unsigned)lane) % (unsigned)NP];
                    tile = n_tiles;
                    while (wtried < (unsigned)kWg3Heads) {
                        unsigned c = 0xffffffffu;
                        if (w3_lane() == 0 && __hip_atomic_load(work_head + wseg * 32u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) * (unsigned)kWg3Heads + wseg < n_tiles)
                            c = atomicAdd(work_head + wseg * 32u, 1u);
                        c = U(c);
                        if (c != 0xffffffffu && c * (unsigned)kWg3Heads + wseg < n_tiles) {
                            tile = c * (unsigned)kWg3Heads + wseg;
                            break;
                        }
                        wseg = (wseg + 1u) % (unsigned)kWg3Heads;
                        ++wtried;
                    }
                } else {
                    bump_fresh(false);
                }
            }
        }
        if (kind == W3_EXIT) break;
        if (kind == W3_NONE) {
            if (idle_polls < 2u) __builtin_amdgcn_s_sleep(2);
            else __builtin_amdgcn_s_sleep(VSPG_WG3_IDLE_SLEEP);
            // (safety valve: a wavefront that has found nothing for ~10^7 polls -- seconds -- leaves instead of hanging the device;
            //  the launch's counters and film then show the loss)
            VSPG_PROF_ACC_END(prof_idle);
            if (++idle_polls > (1u << 23)) break;
            continue;
        }
        VSPG_PROF_ACC_END(prof_decide);
        idle_polls = 0;
        VSPG_W3T(if (kind == W3_VERTEX && n0 + n1 == 64u) tl.enter(1u, W3T_FULL); tl.chunk_begin());
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

        if (kind == W3_VERTEX) {
            // ---- V: vertex processing (NEE, Russian roulette, new direction) ----------------------------
            VSPG_PROF(PS_WG_B);
            bool cont = false, restart = false, freed = false, old_done = false;
            int slot = 0;
            if ((unsigned)lane < n0 + n1) {
                slot = (unsigned)lane < n0 ? s_ring[q0][(pos0 + (unsigned)lane) % (unsigned)NP]
                                           : s_ring[q0 ^ 1u][(pos1 + ((unsigned)lane - n0)) % (unsigned)NP];
                Sampler sampler;
                PathState st;
                IsgSample isg;
                int ch;
                bool alive;
                if constexpr (GUIDED) {  // the guided vertex works on the pool record directly (vspg_guided_wg.h)
                    const uint32_t fl = P.u(LY::FLAGS, slot);
                    if constexpr (TRAIN) { (void)rec_bind(P.i(LY::PIXEL, slot)); pool_load_rec<LY>(P, slot, pc.rec); }
                    alive = li_vertex_guided_wg<Medium>(S, medium, P, slot, fl, pc, reinterpret_cast<const VspgKdNode *>(glds), &st.L, &isg);
                    if constexpr (TRAIN) { if (alive) pool_store_rec<LY>(P, slot, pc.rec); }
                    if (!alive) {
                        isg.valid = (fl & FL_ISG_VALID) != 0;
                        isg.surface_event = (fl & FL_ISG_SURF) != 0;
                        isg.vsp_used = P.f(LY::VSP, slot);  // (depth >= 1 at a vertex: the slot holds isg.vsp_used)
                    }
                } else {
                    const uint32_t fl = pool_load<GUIDED, Medium::kGrey, FULL>(P, slot, S, st, sampler, &ch, isg);
                    const Vertex vx = pool_load_vertex<GUIDED, Medium::kGrey, FULL>(P, slot, fl);
                    alive = li_segment_b<Medium, GUIDED, GUIDED>(S, medium, st, ch, sampler, pc, vx, glds, kWgBlock);
                    if (alive) pool_store_full<GUIDED, Medium::kGrey, FULL>(P, slot, st, sampler, ch, isg, FL_LIVE);
                }
                if (alive) {
                    cont = true;
                } else {
                    if constexpr (CARRY) old_done = P.i(LY::SAMPLE, slot) != first_sample;
                    emit(P.i(LY::PIXEL, slot), st.L, isg, old_done);
                    if constexpr (TRAIN) train.seg_count[rec_bind(P.i(LY::PIXEL, slot))] = pc.rec.n;
                    pc.path();
                    const int s2 = P.i(LY::SAMPLE, slot) + sample_step;
                    P.i(LY::SAMPLE, slot) = s2;
                    restart = !w3_at_use(single_sample) && s2 < wave_end;
                    freed = !restart;
                }
            }
            // (the chunk's tail -- OLD, LIVE, BUSY_V -- rides behind the push's commits; the slots freed are its Q_F lanes)
            const unsigned n_old = CARRY ? (unsigned)__popcll(__builtin_amdgcn_ballot_w64(old_done)) : 0u;
            ring_push_all<NP>(cont || restart ? Q_A : (freed ? Q_F : -1), (unsigned)slot | (restart ? kRestartBit : 0u), s_ring, s_w, n_old, 1);
            VSPG_W3T(tl.chunk_end(0u, n0 + n1));
            continue;
        }

        // ---- S: camera ray + primary segment for new paths, one secondary segment for the others ------
        {
            VSPG_PROF(PS_WG_A);
            bool toVV = false, toVS = false, toA = false, restart = false, freed = false, old_done = false;
            int slot = 0;
            const bool fresh = kind == W3_FRESH;
            const bool tile_ok = !fresh || tile < n_tiles;  // (the head has run dry: the 64 slots go back)
            if (fresh && !tile_ok) {
                slot = (int)fresh_entry;
                freed = true;
            } else if ((unsigned)lane < n0) {
                const unsigned e = fresh ? fresh_entry : s_ring[Q_A][(pos0 + (unsigned)lane) % (unsigned)NP];
                slot = (int)(e & (kRestartBit - 1u));
                const bool primary = fresh || (e & kRestartBit) != 0u;
                Sampler sampler;
                PathState st;
                IsgSample isg;
                int ch = 0, pxy = 0;
                Vertex vx;
                bool alive = false, valid = true;
                int seg = LI_END;
                if (primary) {
                    int px, py, smp;
                    float vsp0 = 0.5f;  // the pixel's entry of the VSP buffer once the buffer counts (start_path)
                    if (fresh) {
                        unsigned ty = w3_at_use(tilesX) == 1 ? tile : __umulhi(tile, tiles_magic);
                        unsigned tx = tile - ty * (unsigned)tilesX;
                        while (tx >= (unsigned)tilesX) { tx -= (unsigned)tilesX; ty++; }
                        if constexpr (WINDOW) { tx += (unsigned)win_tile_x0(win); ty += (unsigned)win_tile_y0(win); }
                        px = (int)(tx * 8u + ((unsigned)lane & 7u));
                        py = (int)(ty * 8u + ((unsigned)lane >> 3));
                        pxy = px | (py << 16);
                        smp = first_sample;
                        // the PREVIOUS one-sample launch parked this pixel's sample (vspg_render_wave: deferred resolve): it enters
                        // the film now, before this launch's sample of the pixel can (same order of additions as ever)
                        // Everything the pixel's start reads from global memory leaves together and is waited for once: the parked sample, the
                        // film pixel and the statistics it goes into, and the pixel's VSP -- four dependent round trips before.  The loads are
                        // speculative (the sentinel and the ISG code decide what is stored); they stay behind in_launch: a padding lane's
                        // pixel lies outside the buffers.
                        if (in_launch(px, py)) {
                            const size_t pidx = (size_t)py * W + px;
                            if (w3_at_use(vsp_ready) & VSP_READY) vsp0 = vsp_buf[pidx];
                            if (w3_at_use(prev_samples) != nullptr) {
                                float *const isg_px = isg_stats + pidx * VSPG_ISG_STATS;
                                const float4 parked = prev_samples[pidx];
                                float4 fpx = film[pidx], st03 = *reinterpret_cast<const float4 *>(isg_px);
                                float2 st45 = *reinterpret_cast<const float2 *>(isg_px + 4);
                                w3_loads_arrived(parked, fpx, st03, st45, vsp0);
                                if (!(CARRY && carry_sentinel(parked.w)))  // (... unless its path is still in flight: it resumed in this launch)
                                    resolve_sample_loaded(parked, fpx, st03, st45, film + pidx, isg_px);
                            }
                        }
                    } else {
                        pxy = P.i(LY::PIXEL, slot);
                        smp = P.i(LY::SAMPLE, slot);
                        px = pxy & 0xffff;
                        py = (int)((unsigned)pxy >> 16);
                    }
                    valid = in_launch(px, py) && smp < wave_end;  // tile padding: the slot stays free
                    if (valid) {
                        if (!fresh && (w3_at_use(vsp_ready) & VSP_READY)) vsp0 = vsp_buf[(size_t)py * W + px];
                        if (w3_at_use(single_sample))
                            start_path<false>(S, vsp0, px, py, jump, sampler, st, &ch, isg);
                        else
                            start_path<false>(S, vsp0, px, py, smp, sampler, st, &ch, isg);
                        P.i(LY::PIXEL, slot) = pxy;
                        P.i(LY::SAMPLE, slot) = smp;
                        if constexpr (TRAIN) { (void)rec_bind(pxy); pc.rec.reset(); }
                        seg = li_segment_a<Medium, GUIDED, SEG_PRIMARY>(S, medium, vsp_buf, w3_at_use(vsp_ready), px, py, st, ch, sampler,
                                                                        isg, pc, vx);
                        alive = seg != LI_END;
                        if (alive) {
                            pool_store_full<GUIDED, Medium::kGrey, FULL>(P, slot, st, sampler, ch, isg, FL_LIVE | (seg == LI_VERTEX && vx.volume ? (uint32_t)FL_VX_VOLUME : 0u));
                            if (seg == LI_VERTEX) pool_store_vertex<GUIDED, Medium::kGrey>(P, slot, vx);
                            if constexpr (TRAIN) pool_store_rec<LY>(P, slot, pc.rec);
                        }
                    } else {
                        freed = true;
                    }
                } else {
                    const uint32_t fl = pool_load<GUIDED, Medium::kGrey, FULL>(P, slot, S, st, sampler, &ch, isg);
                    pxy = P.i(LY::PIXEL, slot);
                    const int px = pxy & 0xffff, py = (int)((unsigned)pxy >> 16);
                    if constexpr (TRAIN) { (void)rec_bind(pxy); pool_load_rec<LY>(P, slot, pc.rec); }
                    // (full scenes: a path that crossed a medium boundary on its camera segment is still at depth 0 here)
                    seg = li_segment_a<Medium, GUIDED, FULL ? SEG_ANY : SEG_SECONDARY>(S, medium, vsp_buf, w3_at_use(vsp_ready), px, py, st, ch, sampler,
                                                                                      isg, pc, vx);
                    alive = seg != LI_END;
                    if (seg == LI_SKIP) {
                        pool_store_full<GUIDED, Medium::kGrey, FULL>(P, slot, st, sampler, ch, isg, fl & (FL_LIVE | FL_GS_SCATTER | FL_GS_FIELD));
                    } else if (alive) {
                        pool_store_a<Medium::kGrey, GUIDED, FULL>(P, slot, st, sampler, ch, isg, vx, fl & (FL_LIVE | FL_GS_SCATTER | FL_GS_FIELD | FL_INMED));
                        if constexpr (TRAIN) pool_store_rec<LY>(P, slot, pc.rec);
                    }
                }
                if (seg == LI_SKIP) {        // a medium boundary was crossed (:399-404): no vertex, the next segment starts behind it
                    toA = true;
                } else if (alive) {
                    toVV = vx.volume;
                    toVS = !vx.volume;
                } else if (valid) {
                    if constexpr (CARRY) old_done = !primary && P.i(LY::SAMPLE, slot) != first_sample;
                    emit(pxy, st.L, isg, old_done);
                    if constexpr (TRAIN) train.seg_count[rec_bind(pxy)] = pc.rec.n;  // PropagateSamples (:627) follows in k_propagate
                    pc.path();
                    const int s2 = P.i(LY::SAMPLE, slot) + sample_step;
                    P.i(LY::SAMPLE, slot) = s2;
                    restart = !w3_at_use(single_sample) && s2 < wave_end;
                    freed = !restart;
                }
            }
            // (the chunk's tail -- OLD, BUSY_S, LIVE -- rides behind the push's commits; EXH before them, where it stood: a sibling
            //  that sees LIVE == 0 sees the cursors dry)
            const unsigned n_old = CARRY ? (unsigned)__popcll(__builtin_amdgcn_ballot_w64(old_done)) : 0u;
            if (fresh && !tile_ok) {
                if (w3_lane() == 0) atomicExch(s_w + W3_EXH, 1u);
            }
            ring_push_all<NP>(toVV ? Q_VV : toVS ? Q_VS : (toA || restart) ? Q_A : (freed ? Q_F : -1), (unsigned)slot | (restart ? kRestartBit : 0u), s_ring, s_w, n_old, 0);
            VSPG_W3T(tl.chunk_end(fresh ? 2u : 1u, tile_ok ? n0 : 0u));
        }
    }
    VSPG_W3T(tl.stamp(W3T_EXIT));
    if constexpr (!GUIDED) {
        atomicAdd(&s_counters[CNT_PATHS], pc.paths); atomicAdd(&s_counters[CNT_SEGMENTS], pc.segments);
        atomicAdd(&s_counters[CNT_VOLUME_SCATTERS], pc.volume_scatters); atomicAdd(&s_counters[CNT_SURFACE_HITS], pc.surface_hits);
        atomicAdd(&s_counters[CNT_DENSITY_QUERIES], pc.density_queries); atomicAdd(&s_counters[CNT_SHADOW_RAYS], pc.shadow_rays);
        atomicAdd(&s_counters[CNT_SHADOW_QUERIES], pc.shadow_queries);
    }
    __syncthreads();
    if (threadIdx.x < CNT_COUNT) atomicAdd(&counters[threadIdx.x], (unsigned long long)s_counters[threadIdx.x]);
    if constexpr (CARRY) {
        // SUSPEND (every wavefront has left the loop: no chunk in flight, every push committed): the image, and the sentinel of every
        // path it holds -- the entries of the three path queues
        unsigned int *const susp = reinterpret_cast<unsigned int *>((uintptr_t)s_w[W3_SUSP_LO] | ((uintptr_t)s_w[W3_SUSP_HI] << 32));
        if (susp != nullptr) {
            unsigned int *const img = susp + (size_t)blockIdx.x * kImgStride;
            if (threadIdx.x < W3_COUNT) ((__attribute__((address_space(1))) unsigned int *)img)[kImgWords + threadIdx.x] = s_w[threadIdx.x];
            if (s_w[W3_LIVE] != 0u) {
                // (the address came back from LDS as two integers: said to be global memory here, or the stores are flat ones, which
                //  count as LDS traffic too and wait for each other's reads)
                const w3_glb_v4 img4 = (w3_glb_v4)img;
                w3_u32x4 piece[kImgRounds];
#pragma unroll
                for (int k = 0; k < kImgRounds; ++k) {
                    const int i = w3_image_piece<kImgPieces>(img_lane + k * kWgBlock);
                    piece[k] = *(i < kImgPool / 4 ? pool4 + i : ring4 + (i - kImgPool / 4));
                }
#pragma unroll
                for (int k = 0; k < kImgRounds; ++k) {
                    const int i = img_lane + k * kWgBlock;
                    if (i < kImgPieces) img4[i] = piece[k];
                }
                for (int q = 0; q < Q_F; ++q) {
                    const unsigned h = s_w[q * QC_STRIDE + QC_HEAD], n = s_w[q * QC_STRIDE + QC_COM] - h;
                    for (unsigned i = threadIdx.x; i < n && i < (unsigned)NP; i += kWgBlock) {
                        const int pxy = P.i(LY::PIXEL, (int)(s_ring[q][(h + i) % (unsigned)NP] & (kRestartBit - 1u)) % NP);
                        const unsigned px = (unsigned)pxy & 0xffffu, py = (unsigned)pxy >> 16;
                        if (in_launch((int)px, (int)py)) wave_samples[(size_t)py * W + px].w = kCarrySentinel;
                    }
                }
            }
        }
    }
}

template <class Medium, bool GUIDED, int NP, int kWgBlock, int kWgWavesPerSimd, bool TRAIN = false>
__global__ __launch_bounds__(kWgBlock, kWgWavesPerSimd) void k_render_wave_wg3(
    const DScene *__restrict__ Sp, float4 *__restrict__ film, float *__restrict__ isg_stats, const float *__restrict__ vsp_buf,
    int vsp_ready, int wave_end, int first_sample, int single_sample, PcgJump jump, unsigned int tiles_magic,
    unsigned int *__restrict__ work_head, const float4 *__restrict__ prev_samples,
    float4 *__restrict__ wave_samples, unsigned long long *__restrict__ counters, TrainArgs train = TrainArgs{nullptr, nullptr, nullptr, nullptr, 0, 0}) {
    wg3_render<Medium, GUIDED, NP, kWgBlock, kWgWavesPerSimd, TRAIN, false>(Sp, film, isg_stats, vsp_buf, vsp_ready, wave_end, first_sample, single_sample, jump,
                                                                            tiles_magic, work_head, prev_samples, wave_samples, counters, train, PixelWindow{0, 0, 0, 0});
}
// the same kernel over a pixel window (a kernel name of its own: the full-frame instantiations stay the only ones of theirs);
// tiles_magic = ceil(2^32 / the window's tile columns)
template <class Medium, bool GUIDED, int NP, int kWgBlock, int kWgWavesPerSimd, bool TRAIN = false>
__global__ __launch_bounds__(kWgBlock, kWgWavesPerSimd) void k_render_wave_wg3_window(
    const DScene *__restrict__ Sp, float4 *__restrict__ film, float *__restrict__ isg_stats, const float *__restrict__ vsp_buf,
    int vsp_ready, int wave_end, int first_sample, int single_sample, PcgJump jump, unsigned int tiles_magic,
    unsigned int *__restrict__ work_head, const float4 *__restrict__ prev_samples,
    float4 *__restrict__ wave_samples, unsigned long long *__restrict__ counters, TrainArgs train, PixelWindow win) {
    wg3_render<Medium, GUIDED, NP, kWgBlock, kWgWavesPerSimd, TRAIN, true>(Sp, film, isg_stats, vsp_buf, vsp_ready, wave_end, first_sample, single_sample, jump,
                                                                           tiles_magic, work_head, prev_samples, wave_samples, counters, train, win);
}

// the same kernel in CARRY mode (see the header of this file): `resume` / `suspend` are per-workgroup images, either may be null
template <class Medium, bool GUIDED, int NP, int kWgBlock, int kWgWavesPerSimd, bool WINDOW>
__global__ __launch_bounds__(kWgBlock, kWgWavesPerSimd) void k_render_wave_wg3_carry(
    const DScene *__restrict__ Sp, float4 *__restrict__ film, float *__restrict__ isg_stats, const float *__restrict__ vsp_buf,
    int vsp_ready, int wave_end, int first_sample, int single_sample, PcgJump jump, unsigned int tiles_magic,
    unsigned int *__restrict__ work_head, const float4 *__restrict__ prev_samples,
    float4 *__restrict__ wave_samples, unsigned long long *__restrict__ counters, PixelWindow win,
    const unsigned int *__restrict__ resume, unsigned int *__restrict__ suspend) {
    wg3_render<Medium, GUIDED, NP, kWgBlock, kWgWavesPerSimd, false, WINDOW, true>(Sp, film, isg_stats, vsp_buf, vsp_ready, wave_end, first_sample, single_sample, jump,
                                                                                   tiles_magic, work_head, prev_samples, wave_samples, counters,
                                                                                   TrainArgs{nullptr, nullptr, nullptr, nullptr, 0, 0}, win, resume, suspend);
}

// ---- host side: the unguided rectangle-scene instantiations behind one call (what vspg_capi.hip launches for them, and what the
// fast-arithmetic translation units export: vspg_fast.hip, vspg_arith.h) -------------------------------------------------------
#ifndef VSPG_WG_WAVES
#define VSPG_WG_WAVES 4
#endif
#ifndef VSPG_WG_BLOCK
#define VSPG_WG_BLOCK 512
#endif
struct Wg3Launch {
    const DScene *dscene;
    float4 *film;
    float *isg_stats;
    const float *vsp;
    int vsp_ready, wave_end, first_sample, single_sample;
    PcgJump jump;
    unsigned int tiles_magic;
    unsigned int *work_head;
    const float4 *ws_prev;
    float4 *ws_out;
    unsigned long long *counters;
    unsigned int blocks;
    hipStream_t stream;
    int grey;          // 0: chromatic; 1: grey medium; 2: grey medium and grey surfaces (HomogeneousMediumT)
    int null_zero;     // ... whose null-collision coefficient is exactly 0
    int windowed;      // the launch covers `win`, not the frame (vspg_render_window): k_render_wave_wg3_window
    PixelWindow win;
    int carry;         // k_render_wave_wg3_carry: resume from / suspend into the per-workgroup images (either may be null)
    const unsigned int *resume;
    unsigned int *suspend;
};
template <int GREY> constexpr int kWg3PoolHomogT = wg3_pool_paths<PoolLayout<false, GREY>>(VSPG_WG3_OTHER);
// dwords of a workgroup's image, the largest of the instantiations below (what the host allocates per workgroup)
template <int GREY> constexpr int kWg3ImageStrideT = kWg3ImageStride<PoolLayout<false, GREY>, kWg3PoolHomogT<GREY>>;
constexpr int kWg3ImageStrideMax = kWg3ImageStrideT<0> > kWg3ImageStrideT<1> ? (kWg3ImageStrideT<0> > kWg3ImageStrideT<2> ? kWg3ImageStrideT<0> : kWg3ImageStrideT<2>)
                                                                             : (kWg3ImageStrideT<1> > kWg3ImageStrideT<2> ? kWg3ImageStrideT<1> : kWg3ImageStrideT<2>);
// (a template: a plain inline host function that names kernels instantiates them in every translation unit that includes this
// header, even where nothing calls it -- the exact ones belong to vspg_wg3_exact.hip alone)
template <int = 0>
inline int wg3_launch_unguided(const Wg3Launch &L) {
#define VSPG_WG3_GO(M, NPOOL)                                                                                                                \
    do {                                                                                                                                     \
        if (L.carry && L.windowed)                                                                                                           \
            hipLaunchKernelGGL((k_render_wave_wg3_carry<M, false, NPOOL, VSPG_WG_BLOCK, VSPG_WG_WAVES, true>), dim3(L.blocks), dim3(VSPG_WG_BLOCK), 0, \
                               L.stream, L.dscene, L.film, L.isg_stats, L.vsp, L.vsp_ready, L.wave_end, L.first_sample, L.single_sample, L.jump, \
                               L.tiles_magic, L.work_head, L.ws_prev, L.ws_out, L.counters, L.win, L.resume, L.suspend);                    \
        else if (L.carry)                                                                                                                    \
            hipLaunchKernelGGL((k_render_wave_wg3_carry<M, false, NPOOL, VSPG_WG_BLOCK, VSPG_WG_WAVES, false>), dim3(L.blocks), dim3(VSPG_WG_BLOCK), 0, \
                               L.stream, L.dscene, L.film, L.isg_stats, L.vsp, L.vsp_ready, L.wave_end, L.first_sample, L.single_sample, L.jump, \
                               L.tiles_magic, L.work_head, L.ws_prev, L.ws_out, L.counters, PixelWindow{0, 0, 0, 0}, L.resume, L.suspend);   \
        else if (L.windowed)                                                                                                                      \
            hipLaunchKernelGGL((k_render_wave_wg3_window<M, false, NPOOL, VSPG_WG_BLOCK, VSPG_WG_WAVES, false>), dim3(L.blocks), dim3(VSPG_WG_BLOCK), 0, \
                               L.stream, L.dscene, L.film, L.isg_stats, L.vsp, L.vsp_ready, L.wave_end, L.first_sample, L.single_sample, L.jump, \
                               L.tiles_magic, L.work_head, L.ws_prev, L.ws_out, L.counters, TrainArgs{nullptr, nullptr, nullptr, nullptr, 0, 0}, L.win); \
        else                                                                                                                                 \
            hipLaunchKernelGGL((k_render_wave_wg3<M, false, NPOOL, VSPG_WG_BLOCK, VSPG_WG_WAVES, false>), dim3(L.blocks), dim3(VSPG_WG_BLOCK), 0, L.stream, \
                               L.dscene, L.film, L.isg_stats, L.vsp, L.vsp_ready, L.wave_end, L.first_sample, L.single_sample, L.jump, L.tiles_magic, \
                               L.work_head, L.ws_prev, L.ws_out, L.counters, TrainArgs{nullptr, nullptr, nullptr, nullptr, 0, 0});          \
    } while (0)
    if (L.grey >= 2 && L.null_zero) VSPG_WG3_GO(HomogeneousMediumGreySceneNullZero, kWg3PoolHomogT<2>);
    else if (L.grey >= 2) VSPG_WG3_GO(HomogeneousMediumGreyScene, kWg3PoolHomogT<2>);
    else if (L.grey == 1) VSPG_WG3_GO(HomogeneousMediumGrey, kWg3PoolHomogT<1>);
    else VSPG_WG3_GO(HomogeneousMediumSimple, kWg3PoolHomogT<0>);
#undef VSPG_WG3_GO
    return (int)hipGetLastError();
}
// the exact-arithmetic instantiations, compiled in vspg_wg3_exact.hip (flags of their own, csrc/Makefile)
int wg3_launch_exact(const Wg3Launch &L);

VSPG_NS_END  // namespace vspg
