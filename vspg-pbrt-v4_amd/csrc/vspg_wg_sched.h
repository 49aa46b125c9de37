// vspg_wg_sched.h -- the two older workgroup schedulers, k_render_wave_wg and k_render_wave_wg2, with their pool sizes and the
// C_* / D_* counter slots (the design: vspg_wg_kernel.h; the current scheduler, k_render_wave_wg3: vspg_wg3.h).
//
// Text of vspg_capi.hip, included there once at the place where it stood: it is part of that translation unit, uses the constants
// defined above it (kNumCounters) and is not meant for any other unit.
#pragma once

namespace {

// Workgroup-level wavefront kernel (see vspg_wg_kernel.h for the design): a persistent workgroup
// advances a pool of NP paths parked in LDS, phase by phase, over compacted lists.  Iteration k
// (parity par = k & 1, nxt = par ^ 1):
//   assign  wavefront 0 maps the free slots of s_free[par] to work items (s_item), claiming chunks of
//           kWgChunk items from the global head;
//   S       "segment" phase over one dense index space
//             [0, nAssign)           fresh slots: camera ray + PRIMARY segment (VSP-guided distance sampling)
//             [.., + A0[par])        slots whose pixel starts its next sample (multi-sample launches): same
//             [.., + A1[par])        continuing paths: one SECONDARY segment (plain delta tracking)
//           survivors go to the vertex list (volume vertices from the front of s_listB, surface vertices
//           from the back), finished paths are splatted and their slot goes to s_free[nxt] or, when the
//           pixel has samples left, to the front of s_listA[nxt];
//   V       vertex phase over s_listB: NEE, Russian roulette, new direction; survivors go to the back of
//           s_listA[nxt].
// Fusing the camera ray with the primary segment keeps the heaviest code (optical-depth-space sampling)
// where the path state is still compile-time constant (beta = r_u = r_l = 1, L = 0), and keeping it out
// of the secondary phase is what lets the whole kernel fit the 128-VGPR budget of 4 waves per SIMD.
// Launch shapes.  Homogeneous media: the segment code has no loops left (see HomogeneousMedium::
// kAlwaysRealCollision) and the kernel fits 128 VGPRs: 512-thread workgroups, 4 waves per SIMD, two
// workgroups per CU, 512 paths each.  Grid media keep the DDA / null-collision loops (about 250 live
// VGPRs): 256-thread workgroups at 2 waves per SIMD, 368 paths beside the 16 KB majorant grid in LDS.
#ifndef VSPG_WG_WAVES
#define VSPG_WG_WAVES 4
#endif
#ifndef VSPG_WG_BLOCK
#define VSPG_WG_BLOCK 512
#endif
#ifndef VSPG_WG_NP
#define VSPG_WG_NP 512
#endif
constexpr int kWgWavesHomog = VSPG_WG_WAVES, kWgBlockHomog = VSPG_WG_BLOCK, kWgPoolHomog = VSPG_WG_NP;
constexpr int kWgWavesGrid = 2, kWgBlockGrid = 256, kWgPoolGrid = 384;
#ifndef VSPG_WGG_NP
#define VSPG_WGG_NP 320
#endif
#ifndef VSPG_WGG_WAVES
#define VSPG_WGG_WAVES 4
#endif
#ifndef VSPG_WGG_BLOCK
#define VSPG_WGG_BLOCK 512
#endif
// guided vertices on the workgroup kernel (round 3, vspg_guided_wg.h): 128 registers, four waves per SIMD like the unguided kernel
constexpr int kWgWavesGuided = VSPG_WGG_WAVES, kWgBlockGuided = VSPG_WGG_BLOCK, kWgPoolGuided = VSPG_WGG_NP;
// Paths per pool: what fits the 80 KB a workgroup may use when two share a CU -- the record (PoolLayout::COUNT dwords), the
// lists' entries per path, and `other` bytes of fixed LDS (scene records, tables, counters, staged kd nodes); a multiple of 32.
#ifndef VSPG_WG_LDS_BUDGET
#define VSPG_WG_LDS_BUDGET 81920
#endif
#ifndef VSPG_WG_NP_CAP
#define VSPG_WG_NP_CAP 512
#endif
template <class LY>
constexpr int wg_pool_paths(int list_bytes_per_path, int other_bytes) {
    return (VSPG_WG_LDS_BUDGET - other_bytes) / (LY::COUNT * 4 + list_bytes_per_path) / 32 * 32;
}
#ifndef VSPG_WG_OTHER
#define VSPG_WG_OTHER 5500
#endif
// The unguided kernels run eight waves per workgroup over 64-entry chunks: 512 paths give every wave one chunk per phase, and a
// pool that is not a multiple of that leaves a second round of partly filled chunks behind (608 paths: 0.849 against 0.804 ms per
// 1080p wave) -- so the records the grey instantiations save are not spent on more paths there.
template <int GREY> constexpr int kWgPoolHomogT = wg_pool_paths<PoolLayout<false, GREY>>(14, VSPG_WG_OTHER) < 512 ? wg_pool_paths<PoolLayout<false, GREY>>(14, VSPG_WG_OTHER) : 512;  // k_render_wave_wg: + s_item
template <int GREY> constexpr int kWg2PoolHomogT = wg_pool_paths<PoolLayout<false, GREY>>(10, VSPG_WG_OTHER) < VSPG_WG_NP_CAP ? wg_pool_paths<PoolLayout<false, GREY>>(10, VSPG_WG_OTHER) : VSPG_WG_NP_CAP;
// full scenes (triangles, spheres, infinite lights, medium boundaries): the generic record + isg.vsp_used; the stage_scene_lds copy is the same
constexpr int kWg2PoolFull = wg_pool_paths<PoolLayout<false, 0, false, true>>(10, VSPG_WG_OTHER) < VSPG_WG_NP_CAP ? wg_pool_paths<PoolLayout<false, 0, false, true>>(10, VSPG_WG_OTHER) : VSPG_WG_NP_CAP;
// guided: every path counts (320 -> 384 -> 416 paths: 2.14 -> 1.86 -> 1.78 ms per trained 1080p wave)
#ifndef VSPG_WGG_NP_G0
#define VSPG_WGG_NP_G0 wg_pool_paths<PoolLayout<true, 0>>(10, VSPG_WG_OTHER + 2 * kKdLdsNodes * 8)
#endif
#ifndef VSPG_WGG_NP_G2
#define VSPG_WGG_NP_G2 wg_pool_paths<PoolLayout<true, 2>>(10, VSPG_WG_OTHER + 2 * kKdLdsNodes * 8)
#endif
template <int GREY> constexpr int kWg2PoolGuidedT = GREY >= 2 ? (VSPG_WGG_NP_G2) : (VSPG_WGG_NP_G0);
template <int GREY> constexpr int kWg2PoolTrainT = wg_pool_paths<PoolLayout<true, GREY, true>>(10, VSPG_WG_OTHER + 2 * kKdLdsNodes * 8);  // + the recorder's state
constexpr int kWgChunk = 256;  // work items (4 pixel tiles) a workgroup claims per global atomic
enum { C_A0 = 0, C_A1 = 2, C_CURA = 4, C_BV = 6, C_BS = 7, C_CURB = 8, C_NFREE = 9, C_NASSIGN = 11, C_RNEXT = 12, C_REND = 13,
       C_EXH = 14, C_RTX = 15, C_RTY = 16, C_COUNT = 17 };

template <class Medium, bool GUIDED, int NP, int kWgBlock, int kWgWavesPerSimd>
__global__ __launch_bounds__(kWgBlock, kWgWavesPerSimd) void k_render_wave_wg(
    const DScene *__restrict__ Sp, float4 *__restrict__ film, float *__restrict__ isg_stats, const float *__restrict__ vsp_buf,
    int vsp_ready, int wave_end, int first_sample, int single_sample, PcgJump jump, unsigned int tiles_magic,
    unsigned int *__restrict__ work_head, unsigned long long *__restrict__ counters, PixelWindow win) {
    // win: the pixels the launch covers (see k_render_wave); tilesX / tilesY are the window's tile rectangle
    // tiles_magic = ceil(2^32 / tilesX): the one integer division of the kernel (tile index -> tile row, once
    // per claimed chunk) is a multiply-high by it plus a fix-up; pixels travel as packed (x | y << 16)
    const DScene &S = *Sp;
    const int W = S.xres;
    const int tilesX = win_tiles_x(win), tilesY = win_tiles_y(win);
    const unsigned total_items = (unsigned)(tilesX * tilesY) * 64u;
    const int lane = threadIdx.x & 63;
    const int sample_step = S.shard_count > 1 ? S.shard_count : 1;
    reset_sibling_head(work_head);

    using LY = PoolLayout<GUIDED, Medium::kGrey>;
    constexpr int NF = LY::COUNT;
    // (Tried in round 2 and dropped: the pool in the workgroup's own piece of GLOBAL memory instead of LDS -- the segment-streaming
    // layout SURVEY 8d's byte model describes -- 0.82 ms (LDS, 512 paths) -> 2.49 / 3.39 / 2.95 ms with 1024 / 2048 / 4096 paths.)
    __shared__ float s_pool[NF * NP];
    float *const pool_base = s_pool;
    __shared__ unsigned short s_listA[2][NP], s_listB[NP], s_free[2][NP];
    __shared__ unsigned int s_item[NP];
    __shared__ unsigned int s_cnt[C_COUNT];
    const Pool P{pool_base, NP};
    // Heterogeneous media: a tracking walk visits every tentative collision of its ray, and the rays of one list chunk
    // have wildly different expected counts (0 for a ray that misses the cloud, tens through its core): a chunk lasts
    // as long as its longest walk.  Before the segment phase the continuing paths are therefore counting-sorted by the
    // majorant optical depth of their ray (the traversals' own pre-pass quantity), thickest first, so that the lanes of
    // a chunk walk about equally long and the dynamic chunk queue starts with the long chunks.
    constexpr bool kSortWalks = !Medium::kSingleSegment;
    constexpr int kWalkBuckets = 32;
    __shared__ unsigned short s_order[kSortWalks ? NP : 1];
    __shared__ unsigned char s_key[kSortWalks ? NP : 1];
    __shared__ unsigned int s_hist[kSortWalks ? kWalkBuckets : 1];

    const float *maj_ptr = nullptr;
    if constexpr (std::is_same<Medium, GridMedium>::value || std::is_same<Medium, GridMediumGrey>::value) {
        __shared__ float s_maj[kMajRes * kMajRes * kMajRes];
        const float4 *src = reinterpret_cast<const float4 *>(S.majorant);
        float4 *dst = reinterpret_cast<float4 *>(s_maj);
        for (int i = threadIdx.x; i < kMajRes * kMajRes * kMajRes / 4; i += kWgBlock) dst[i] = src[i];
        maj_ptr = s_maj;
    }
    const Medium medium = MediumMaker<Medium>::make(S, maj_ptr);
    // guided builds keep the mixture scratch in registers here (GStoreReg): the LDS belongs to the pool -- and to a copy of
    // the upper levels of the two kd-trees (north star: "LDS-staged kd-tree nodes"), which `glds` then points at
    float *glds = nullptr;
    if constexpr (GUIDED) {
        __shared__ VspgKdNode s_kd[2][kKdLdsNodes];
        for (int f = 0; f < 2; ++f) {
            const int nl = S.field[f].n_nodes < kKdLdsNodes ? S.field[f].n_nodes : kKdLdsNodes;
            for (int i = threadIdx.x; i < nl; i += kWgBlock) s_kd[f][i] = S.field[f].nodes[i];
        }
        glds = reinterpret_cast<float *>(&s_kd[0][0]);
    }
    __shared__ unsigned int s_counters[CNT_COUNT];
#ifdef VSPG_WG_WAVE_COUNTERS  // alternative sink: no per-lane registers, ~2 % slower (measured)
    const WaveCounters pc{s_counters};
#else
    struct LaneCounters : PathCounters { uint32_t paths; VDEV void path() { paths++; } } pc;
    pc.segments = pc.volume_scatters = pc.surface_hits = pc.density_queries = pc.shadow_rays = pc.shadow_queries = pc.paths = 0;
#endif

    stage_scene_lds(S);
    if (threadIdx.x < CNT_COUNT) s_counters[threadIdx.x] = 0;
    if (threadIdx.x < C_COUNT) s_cnt[threadIdx.x] = 0;
    for (int i = threadIdx.x; i < NP; i += kWgBlock) {
        s_free[0][i] = (unsigned short)i;
        P.u(LY::FLAGS, i) = 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) s_cnt[C_NFREE] = NP;
    __syncthreads();

    VSPG_PROF(PS_WG_TOTAL);
    for (int k = 0;; ++k) {
        const int par = k & 1, nxt = par ^ 1;
        // ---- assign: work items for the free slots ---------------------------------------------------
        if (threadIdx.x < 64) {
            const unsigned n_free = s_cnt[C_NFREE + par];
            unsigned rnext = s_cnt[C_RNEXT], rend = s_cnt[C_REND], exh = s_cnt[C_EXH];
            unsigned rtx = s_cnt[C_RTX], rty = s_cnt[C_RTY];  // tile column / row of item rnext
            unsigned filled = 0;
            while (filled < n_free) {
                if (rnext >= rend) {
                    if (exh) break;
                    unsigned base = 0;
                    if (lane == 0) base = atomicAdd(work_head, (unsigned)kWgChunk);
                    base = __builtin_amdgcn_readfirstlane(base);
                    if (base >= total_items) { exh = 1; break; }
                    rnext = base;
                    rend = base + (unsigned)kWgChunk < total_items ? base + (unsigned)kWgChunk : total_items;
                    const unsigned tile = base >> 6;
                    rty = tilesX == 1 ? tile : __umulhi(tile, tiles_magic);
                    rtx = tile - rty * (unsigned)tilesX;
                    while (rtx >= (unsigned)tilesX) { rtx -= (unsigned)tilesX; rty++; }
                }
                const unsigned n = rend - rnext < n_free - filled ? rend - rnext : n_free - filled;
                for (unsigned j = (unsigned)lane; j < n; j += 64u) {
                    const unsigned it = (rnext & 63u) + j;
                    unsigned tx = rtx + (it >> 6), ty = rty;
                    while (tx >= (unsigned)tilesX) { tx -= (unsigned)tilesX; ty++; }
                    s_item[filled + j] = ((tx + (unsigned)win_tile_x0(win)) * 8u + (it & 7u)) | (((ty + (unsigned)win_tile_y0(win)) * 8u + ((it >> 3) & 7u)) << 16);
                }
                rtx += ((rnext & 63u) + n) >> 6;
                while (rtx >= (unsigned)tilesX) { rtx -= (unsigned)tilesX; rty++; }
                rnext += n;
                filled += n;
            }
            if (lane == 0) {
                s_cnt[C_RNEXT] = rnext; s_cnt[C_REND] = rend; s_cnt[C_EXH] = exh; s_cnt[C_RTX] = rtx; s_cnt[C_RTY] = rty;
                s_cnt[C_NASSIGN] = filled;  // free slots beyond `filled` stay empty: the work has run out
                s_cnt[C_BV] = 0; s_cnt[C_BS] = 0; s_cnt[C_CURB] = 0;
                s_cnt[C_A0 + nxt] = 0; s_cnt[C_A1 + nxt] = 0; s_cnt[C_CURA + nxt] = 0;
            }
        } else if (single_sample) {
            // ---- film flush, by the waves the assignment leaves idle ----------------------------------
            // Paths that ended in the previous iteration parked their radiance in their (now free) slot.  In a
            // launch of ONE sample per pixel nobody else touches the pixel, so the film and the ISG statistics take a
            // plain 16-byte load / add / store: the same single IEEE addition per channel as the ten no-return float
            // atomics this replaces, which were L2-atomic-unit bound (0.28 ms of a 0.42 ms maxdepth-0 wave at 1080p).
            // Done here in bulk, every lane busy, the load latency is paid once per 64 finished paths.
            // (Tried: reading the parked record here and doing the global read-modify-write after the barrier, so that
            //  its latency overlaps segment work -- the registers live across the barrier cost more than the overlap won.)
            const unsigned n_free = s_cnt[C_NFREE + par];
            for (unsigned base = (threadIdx.x >> 6) * 64u - 64u; base < n_free; base += (unsigned)kWgBlock - 64u) {
                const unsigned i = base + (unsigned)lane;
                if (i < n_free) {
                    const int slot = s_free[par][i];
                    const uint32_t fl = P.u(LY::FLAGS, slot);
                    if (fl & FL_DONE) {
                        const int pxy = P.i(LY::PIXEL, slot);
                        const size_t pidx = (size_t)((unsigned)pxy >> 16) * W + (pxy & 0xffff);
                        const Spec L = P.sp3(LY::L, slot);
                        IsgSample isg;
                        isg.valid = (fl & FL_ISG_VALID) != 0;
                        isg.surface_event = (fl & FL_ISG_SURF) != 0;
                        isg.vsp_used = P.f(LY::VSP, slot);
                        film_add_sample_rmw(film + pidx, L);
                        isg_add_sample_rmw(isg_stats + pidx * VSPG_ISG_STATS, L, isg);
                        P.u(LY::FLAGS, slot) = 0;
                    }
                }
            }
        }
        { VSPG_PROF(PS_WG_BAR_R); __syncthreads(); }
        if (threadIdx.x == 0) s_cnt[C_NFREE + par] = 0;  // (read by the flush above; refilled from the next iteration on)
        const unsigned nFresh = s_cnt[C_NASSIGN], nA0 = s_cnt[C_A0 + par], nA1 = s_cnt[C_A1 + par];
        const unsigned nPrim = nFresh + nA0, nA = nPrim + nA1;
        if (nA == 0 && s_cnt[C_EXH]) break;  // nothing in flight and nothing left to start

        if constexpr (kSortWalks) {  // ---- order the continuing paths by expected walk length -----------------------
            if (threadIdx.x < kWalkBuckets) s_hist[threadIdx.x] = 0;
            __syncthreads();
            for (unsigned j = threadIdx.x; j < nA1; j += (unsigned)kWgBlock) {
                const int slot = s_listA[par][NP - 1 - (int)j];
                const V3 ro = P.v3(LY::RO, slot), rd = P.v3(LY::RD, slot);
                const int ch = (int)((P.u(LY::FLAGS, slot) >> FL_CH_SHIFT) & 3u);
                const Isect si = scene_intersect(S, ro, rd, kInf);
                float tau = 0.f;
                if (si.hit && S.medium_type != VSPG_MEDIUM_NONE) tau = majorant_optical_depth(medium, ro, rd, si.t, ch);
                int b = tau > 0.f ? 1 + (int)(tau * 0.75f) : 0;
                b = b > kWalkBuckets - 1 ? kWalkBuckets - 1 : b;
                s_key[j] = (unsigned char)b;
                atomicAdd(&s_hist[b], 1u);
            }
            __syncthreads();
            if (threadIdx.x == 0) {  // exclusive offsets, thickest bucket first
                unsigned run = 0;
                for (int b = kWalkBuckets - 1; b >= 0; --b) { const unsigned c = s_hist[b]; s_hist[b] = run; run += c; }
            }
            __syncthreads();
            for (unsigned j = threadIdx.x; j < nA1; j += (unsigned)kWgBlock) {
                const unsigned pos = atomicAdd(&s_hist[s_key[j]], 1u);
                s_order[pos] = s_listA[par][NP - 1 - (int)j];
            }
            __syncthreads();
        }
        // ---- S: camera ray + primary segment for new paths, one secondary segment for the others ------
        while (true) {
            unsigned base = 0;
            if (lane == 0) base = atomicAdd(&s_cnt[C_CURA + par], 64u);
            base = __builtin_amdgcn_readfirstlane(base);
            if (base >= nA) break;
            VSPG_PROF(PS_WG_A);
            const unsigned i = base + (unsigned)lane;
            bool toV = false, toS = false, restart = false, freed = false;
            int slot = 0;
            if (i < nA) {
                Sampler sampler;
                PathState st;
                IsgSample isg;
                int ch = 0, pxy = 0;
                Vertex vx;
                bool alive = false, valid = true;
                if (i < nPrim) {
                    int px, py, smp;
                    if (i < nFresh) {
                        slot = s_free[par][i];
                        pxy = (int)s_item[i];
                        smp = first_sample;
                    } else {
                        slot = s_listA[par][i - nFresh];
                        pxy = P.i(LY::PIXEL, slot);
                        smp = P.i(LY::SAMPLE, slot);
                    }
                    px = pxy & 0xffff;
                    py = (int)((unsigned)pxy >> 16);
                    valid = win_has(win, px, py) && smp < wave_end;  // tile padding: the slot stays free
                    if (valid) {
                        if (single_sample)
                            start_path<!Medium::kSimpleScene>(S, vsp_buf, vsp_ready, px, py, jump, sampler, st, &ch, isg);
                        else
                            start_path<!Medium::kSimpleScene>(S, vsp_buf, vsp_ready, px, py, smp, sampler, st, &ch, isg);
                        P.i(LY::PIXEL, slot) = pxy;
                        P.i(LY::SAMPLE, slot) = smp;
                        alive = li_segment_a<Medium, GUIDED, SEG_PRIMARY>(S, medium, vsp_buf, vsp_ready, px, py, st, ch, sampler,
                                                                          isg, pc, vx);
                        if (alive) {
                            pool_store_full<GUIDED, Medium::kGrey>(P, slot, st, sampler, ch, isg, FL_LIVE | (vx.volume ? (uint32_t)FL_VX_VOLUME : 0u));
                            pool_store_vertex<GUIDED, Medium::kGrey>(P, slot, vx);
                        }
                    } else {
                        freed = true;
                    }
                } else {
                    if constexpr (kSortWalks) slot = s_order[i - nPrim];
                    else slot = s_listA[par][NP - 1 - (int)(i - nPrim)];
                    const uint32_t fl = pool_load<GUIDED, Medium::kGrey>(P, slot, S, st, sampler, &ch, isg);
                    pxy = P.i(LY::PIXEL, slot);
                    const int px = pxy & 0xffff, py = (int)((unsigned)pxy >> 16);
                    alive = li_segment_a<Medium, GUIDED, SEG_SECONDARY>(S, medium, vsp_buf, vsp_ready, px, py, st, ch, sampler,
                                                                        isg, pc, vx);
                    if (alive) pool_store_a<Medium::kGrey, GUIDED>(P, slot, st, sampler, ch, isg, vx, fl & (FL_LIVE | FL_GS_SCATTER | FL_GS_FIELD));
                }
                if (alive) {
                    toV = vx.volume;
                    toS = !vx.volume;
                } else if (valid) {
                    const Spec L = finish_radiance(st.L);
                    const size_t pidx = (size_t)((unsigned)pxy >> 16) * W + (pxy & 0xffff);
                    if (single_sample) {  // parked for the film flush at the top of the next iteration
                        P.sets(LY::L, slot, L);
                        P.i(LY::PIXEL, slot) = pxy;
                        P.f(LY::VSP, slot) = isg.vsp_used;
                        P.u(LY::FLAGS, slot) = (uint32_t)FL_DONE | (isg.valid ? (uint32_t)FL_ISG_VALID : 0u) | (isg.surface_event ? (uint32_t)FL_ISG_SURF : 0u);
                    } else {
                        film_add_sample(film + pidx, L);
                        isg_add_sample_atomic(isg_stats + pidx * VSPG_ISG_STATS, L, isg);
                    }
                    pc.path();
                    const int s2 = P.i(LY::SAMPLE, slot) + sample_step;
                    P.i(LY::SAMPLE, slot) = s2;
                    restart = s2 < wave_end;
                    freed = !restart;
                }
            }
            list_push(toV, slot, s_listB, &s_cnt[C_BV]);
            list_push_back(toS, slot, s_listB + NP - 1, &s_cnt[C_BS]);
            list_push(restart, slot, s_listA[nxt], &s_cnt[C_A0 + nxt]);
            list_push(freed, slot, s_free[nxt], &s_cnt[C_NFREE + nxt]);
        }
        { VSPG_PROF(PS_WG_BAR_A); __syncthreads(); }

        // ---- V: vertex processing (NEE, Russian roulette, new direction) ----------------------------
        const unsigned nBV = s_cnt[C_BV], nB = nBV + s_cnt[C_BS];
        while (true) {
            unsigned base = 0;
            if (lane == 0) base = atomicAdd(&s_cnt[C_CURB], 64u);
            base = __builtin_amdgcn_readfirstlane(base);
            if (base >= nB) break;
            VSPG_PROF(PS_WG_B);
            const unsigned i = base + (unsigned)lane;
            bool cont = false, restart = false, freed = false;
            int slot = 0;
            if (i < nB) {
                slot = i < nBV ? s_listB[i] : s_listB[NP - 1 - (int)(i - nBV)];
                Sampler sampler;
                PathState st;
                IsgSample isg;
                int ch;
                const uint32_t fl = pool_load<GUIDED, Medium::kGrey>(P, slot, S, st, sampler, &ch, isg);
                const Vertex vx = pool_load_vertex<GUIDED, Medium::kGrey>(P, slot, fl);
                if (li_segment_b<Medium, GUIDED, GUIDED>(S, medium, st, ch, sampler, pc, vx, glds, kWgBlock)) {
                    pool_store_full<GUIDED, Medium::kGrey>(P, slot, st, sampler, ch, isg, FL_LIVE);
                    cont = true;
                } else {
                    const int pxy = P.i(LY::PIXEL, slot);
                    const size_t pidx = (size_t)((unsigned)pxy >> 16) * W + (pxy & 0xffff);
                    const Spec L = finish_radiance(st.L);
                    if (single_sample) {  // parked for the film flush at the top of the next iteration
                        P.sets(LY::L, slot, L);
                        P.i(LY::PIXEL, slot) = pxy;
                        P.f(LY::VSP, slot) = isg.vsp_used;
                        P.u(LY::FLAGS, slot) = (uint32_t)FL_DONE | (isg.valid ? (uint32_t)FL_ISG_VALID : 0u) | (isg.surface_event ? (uint32_t)FL_ISG_SURF : 0u);
                    } else {
                        film_add_sample(film + pidx, L);
                        isg_add_sample_atomic(isg_stats + pidx * VSPG_ISG_STATS, L, isg);
                    }
                    pc.path();
                    const int s2 = P.i(LY::SAMPLE, slot) + sample_step;
                    P.i(LY::SAMPLE, slot) = s2;
                    restart = s2 < wave_end;
                    freed = !restart;
                }
            }
            list_push_back(cont, slot, s_listA[nxt] + NP - 1, &s_cnt[C_A1 + nxt]);
            list_push(restart, slot, s_listA[nxt], &s_cnt[C_A0 + nxt]);
            list_push(freed, slot, s_free[nxt], &s_cnt[C_NFREE + nxt]);
        }
        { VSPG_PROF(PS_WG_BAR_B); __syncthreads(); }
    }
    static_assert(CNT_COUNT == kNumCounters, "counter layout");
#ifndef VSPG_WG_WAVE_COUNTERS
    atomicAdd(&s_counters[CNT_PATHS], pc.paths); atomicAdd(&s_counters[CNT_SEGMENTS], pc.segments);
    atomicAdd(&s_counters[CNT_VOLUME_SCATTERS], pc.volume_scatters); atomicAdd(&s_counters[CNT_SURFACE_HITS], pc.surface_hits);
    atomicAdd(&s_counters[CNT_DENSITY_QUERIES], pc.density_queries); atomicAdd(&s_counters[CNT_SHADOW_RAYS], pc.shadow_rays);
    atomicAdd(&s_counters[CNT_SHADOW_QUERIES], pc.shadow_queries);
    __syncthreads();
#endif
    if (threadIdx.x < CNT_COUNT) atomicAdd(&counters[threadIdx.x], (unsigned long long)s_counters[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------------------------------
// k_render_wave_wg2 (round 3): the same pool / phase design with the scheduler's serial pieces taken out.
//   * work assignment: whole pixel tiles for the pool's free slots, claimed from a GLOBAL tile head with one returning atomic per
//     claim (up to NP / 64 tiles at once); a fresh item's pixel is index arithmetic on the claimed tile -- no assignment phase, no
//     s_item array.  (First version: static interleaved shares, workgroup b owning tiles b, b + G, ... -- every workgroup then
//     ended on its own slowest tiles; handing the frame out from the head took the unguided wave from 0.887 to 0.775 ms and the
//     reference-default guided one from 1.59 to 1.45.  VSPG_WG2_TAIL keeps the split adjustable: the share of the frame that
//     comes from the head, in 64ths.)
//   * a finished path of a one-sample-per-pixel launch PARKS {L, ISG code} in a per-pixel buffer with one 16-byte fire-and-forget
//     store; the NEXT launch adds it to the film and the ISG statistics as it starts that pixel's new path (or k_film_resolve
//     does, when something else wants the film first: flush_parked_samples).  The film flush of k_render_wave_wg -- a
//     read-modify-write whose load latency sat between two workgroup barriers of every iteration -- is gone, and with it the
//     third barrier: [segment] barrier [vertex] barrier.  Per pixel and channel it is still the one IEEE addition `film += L` of
//     RGBFilm::AddSample, in the same order: same bits.
//   Measured (profiles/r03_*): per-section wave timers of k_render_wave_wg showed 28 % of the wave cycles in the three
//   barriers and ~20 % in assignment / flush; the SIMDs issued 44 % of the time (scripts/microbench/issue.hip prices).
// Multi-sample launches keep the no-return atomics at the point where a path ends (several samples of a pixel per launch).
enum { D_NFREE = 0, D_A0 = 2, D_A1 = 4, D_CURA = 6, D_BV = 8, D_BS = 10, D_CURB = 12, D_LNEXT = 14, D_COUNT = 15 };
// (isg_code, resolve_sample: vspg_wg3.h)
#ifndef VSPG_WG2_UNIT_SHIFT
#define VSPG_WG2_UNIT_SHIFT 6
#endif
template <class Medium, bool GUIDED, int NP, int kWgBlock, int kWgWavesPerSimd, bool TRAIN = false>
__global__ __launch_bounds__(kWgBlock, kWgWavesPerSimd) void k_render_wave_wg2(
    const DScene *__restrict__ Sp, float4 *__restrict__ film, float *__restrict__ isg_stats, const float *__restrict__ vsp_buf,
    int vsp_ready, int wave_end, int first_sample, int single_sample, PcgJump jump, unsigned int tiles_magic,
    unsigned int static_tiles, unsigned int *__restrict__ work_head, const float4 *__restrict__ prev_samples,
    float4 *__restrict__ wave_samples, unsigned long long *__restrict__ counters, TrainArgs train, PixelWindow win) {
    // win: the pixels the launch covers (see k_render_wave); tiles, static shares and training columns count inside its tile rectangle
    const DScene &S = *Sp;
    const int W = S.xres;
    const int tilesX = win_tiles_x(win), tilesY = win_tiles_y(win);
    const unsigned n_tiles = (unsigned)(tilesX * tilesY);
    const int lane = threadIdx.x & 63;
    const int sample_step = S.shard_count > 1 ? S.shard_count : 1;
    // this workgroup's items: local item j = pixel (j & 63) of tile (j >> 6) * gridDim.x + blockIdx.x, over the first static_tiles
    // tiles; the REST of the frame is handed out tile by tile from a global head once a workgroup has started all of its own --
    // the workgroups finish their static shares at different times (a share's cost follows what its pixels see), and without the
    // shared tail every one of them ended on its own slowest tiles
    const unsigned n_static = static_tiles < n_tiles ? static_tiles : n_tiles;
    constexpr unsigned kUnitShift = VSPG_WG2_UNIT_SHIFT, kUnit = 1u << kUnitShift;
    const unsigned local_tiles = blockIdx.x < n_static ? (n_static - blockIdx.x + gridDim.x - 1) / gridDim.x : 0u;
    const unsigned local_total = local_tiles * 64u;
    reset_sibling_head(work_head);

    // FULL: a scene beyond rectangles and area lights -- triangles (BVH), spheres, infinite lights, non-uniform light samplers, medium
    // boundaries (round 4: these used to fall to the per-lane kernel).  The phases are the same; a segment may end on an interface
    // (LI_SKIP: the path goes round again without a vertex) and a path beyond the camera segment may still be at depth 0.
    constexpr bool FULL = !Medium::kSimpleScene;
    static_assert(!FULL || !GUIDED, "the workgroup kernel's guided vertex (vspg_guided_wg.h) is built for rectangle scenes");
    using LY = PoolLayout<GUIDED, Medium::kGrey, TRAIN, FULL>;
    constexpr int NF = LY::COUNT;
    static_assert(!TRAIN || GUIDED, "segment recording belongs to the guided instantiations");
    __shared__ float s_pool[NF * NP];
    __shared__ unsigned short s_listA[2][NP], s_listB[NP], s_free[2][NP];
    __shared__ unsigned int s_cnt[D_COUNT + 1];
    __shared__ unsigned int s_dyn[2], s_dyn_done[2];  // the tiles claimed for this iteration (first tile, items); the shared tail has run out
    const Pool P{s_pool, NP};
    static_assert(Medium::kSingleSegment, "k_render_wave_wg2 serves homogeneous media (grid media: the wavefront pipeline)");
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
    // counters: per lane in registers (six of them; the unguided instantiations have them to spare), per workgroup in LDS through
    // a ballot and one atomic per count in the guided instantiation, whose vertex phase needs every register it can get
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
            const unsigned item = (((py >> 3) - (unsigned)win_tile_y0(win)) * (unsigned)tilesX + ((px >> 3) - (unsigned)win_tile_x0(win))) * 64u + ((py & 7u) << 3) + (px & 7u);
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
    if (threadIdx.x <= D_COUNT) s_cnt[threadIdx.x] = 0;
    if (threadIdx.x < 2) { s_dyn[threadIdx.x] = 0; s_dyn_done[threadIdx.x] = 0; }
    for (int i = threadIdx.x; i < NP; i += kWgBlock) s_free[0][i] = (unsigned short)i;
    __syncthreads();
    if (threadIdx.x == 0) s_cnt[D_NFREE] = NP;
    __syncthreads();

    // a path ends: its sample leaves the kernel
    auto emit = [&](int pxy, Spec Lraw, const IsgSample &isg) {
        const Spec L = finish_radiance(Lraw);
        const size_t pidx = (size_t)((unsigned)pxy >> 16) * W + (pxy & 0xffff);
        if (single_sample) {
            wave_samples[pidx] = make_float4(L.r, L.g, L.b, isg_code(isg));
        } else {
            film_add_sample(film + pidx, L);
            isg_add_sample_atomic(isg_stats + pidx * VSPG_ISG_STATS, L, isg);
        }
    };

    VSPG_PROF(PS_WG_TOTAL);
    for (int k = 0;; ++k) {
        const int par = k & 1, nxt = par ^ 1;
        const unsigned nFree = s_cnt[D_NFREE + par], nA0 = s_cnt[D_A0 + par], nA1 = s_cnt[D_A1 + par], lnext = s_cnt[D_LNEXT];
        const unsigned left = local_total - lnext;
        // the vertex-list counters of the PREVIOUS iteration (other parity) are free again: nobody reads them before the
        // segment phase of the next iteration pushes into them, two barriers from here
        if (threadIdx.x == 0) { s_cnt[D_BV + nxt] = 0; s_cnt[D_BS + nxt] = 0; s_cnt[D_CURB + nxt] = 0; s_dyn_done[nxt] = s_dyn_done[par]; }
        // own share started: whole tiles from the shared tail for the free slots (one returning atomic per claim).  Every thread
        // takes this branch or none: its condition reads values written at least one barrier ago (the done flag travels by parity).
        unsigned dynBase = 0, nDyn = 0;
        // (the head counts UNITS of 2^kUnitShift work items -- a tile, or half / a quarter of one: smaller units leave fewer slots idle)
        if (left == 0u && nFree >= kUnit && n_static < n_tiles && !s_dyn_done[par]) {
            if (threadIdx.x == 0) {
                const unsigned m = nFree >> kUnitShift, n_dyn = (n_tiles - n_static) << (6 - kUnitShift);
                const unsigned b = atomicAdd(work_head, m);
                const unsigned got = b < n_dyn ? (m < n_dyn - b ? m : n_dyn - b) : 0u;
                s_dyn[0] = (n_static << (6 - kUnitShift)) + b;
                s_dyn[1] = got << kUnitShift;
                if (got < m) s_dyn_done[nxt] = 1u;
            }
            __syncthreads();
            dynBase = s_dyn[0];
            nDyn = s_dyn[1];
        }
        const unsigned nFresh = left > 0u ? (nFree < left ? nFree : left) : nDyn;
        const unsigned nPrim = nFresh + nA0, nA = nPrim + nA1;
        if (nA == 0) break;  // nothing in flight and nothing left to start (free slots exist whenever nothing is in flight)
        const unsigned nSpare = nFree - nFresh;  // carried over to the next iteration's free list (the shared tail will want them)

        // ---- S: camera ray + primary segment for new paths, one secondary segment for the others ------
        while (true) {
            unsigned base = 0;
            if (lane == 0) base = atomicAdd(&s_cnt[D_CURA + par], 64u);
            base = __builtin_amdgcn_readfirstlane(base);
            if (base >= nA + nSpare) break;
            VSPG_PROF(PS_WG_A);
            const unsigned i = base + (unsigned)lane;
            bool toV = false, toS = false, restart = false, freed = false, skipped = false;
            int slot = 0;
            if (i >= nA && i < nA + nSpare) {  // a free slot no new path took this iteration: it stays free
                slot = s_free[par][nFresh + (i - nA)];
                freed = true;
            }
            if (i < nA) {
                Sampler sampler;
                PathState st;
                IsgSample isg;
                int ch = 0, pxy = 0;
                Vertex vx;
                bool alive = false, valid = true;
                int seg = LI_END;
                if (i < nPrim) {
                    int px, py, smp;
                    if (i < nFresh) {
                        slot = s_free[par][i];
                        const unsigned item = lnext + i;
                        const unsigned unit = dynBase + (i >> kUnitShift);  // (claimed items only)
                        const unsigned tile = left > 0u ? (item >> 6) * gridDim.x + blockIdx.x : unit >> (6 - kUnitShift);
                        const unsigned l = left > 0u ? item & 63u : ((unit & ((1u << (6 - kUnitShift)) - 1u)) << kUnitShift) + (i & (kUnit - 1u));
                        unsigned ty = tilesX == 1 ? tile : __umulhi(tile, tiles_magic);
                        unsigned tx = tile - ty * (unsigned)tilesX;
                        while (tx >= (unsigned)tilesX) { tx -= (unsigned)tilesX; ty++; }
                        px = (int)((tx + (unsigned)win_tile_x0(win)) * 8u + (l & 7u));
                        py = (int)((ty + (unsigned)win_tile_y0(win)) * 8u + (l >> 3));
                        pxy = px | (py << 16);
                        smp = first_sample;
                        valid = tile < (left > 0u ? n_static : n_tiles);
                        // the PREVIOUS one-sample launch parked this pixel's sample (vspg_render_wave: deferred resolve): it enters
                        // the film now, before this launch's sample of the pixel can (same order of additions as ever)
                        if (prev_samples != nullptr && valid && win_has(win, px, py)) {
                            const size_t pidx = (size_t)py * W + px;
                            resolve_sample(prev_samples[pidx], film + pidx, isg_stats + pidx * VSPG_ISG_STATS);
                        }
                    } else {
                        slot = s_listA[par][i - nFresh];
                        pxy = P.i(LY::PIXEL, slot);
                        smp = P.i(LY::SAMPLE, slot);
                        px = pxy & 0xffff;
                        py = (int)((unsigned)pxy >> 16);
                    }
                    valid = valid && win_has(win, px, py) && smp < wave_end;  // tile padding: the slot stays free
                    if (valid) {
                        if (single_sample)
                            start_path<!Medium::kSimpleScene>(S, vsp_buf, vsp_ready, px, py, jump, sampler, st, &ch, isg);
                        else
                            start_path<!Medium::kSimpleScene>(S, vsp_buf, vsp_ready, px, py, smp, sampler, st, &ch, isg);
                        P.i(LY::PIXEL, slot) = pxy;
                        P.i(LY::SAMPLE, slot) = smp;
                        if constexpr (TRAIN) { (void)rec_bind(pxy); pc.rec.reset(); }
                        seg = li_segment_a<Medium, GUIDED, SEG_PRIMARY>(S, medium, vsp_buf, vsp_ready, px, py, st, ch, sampler,
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
                    slot = s_listA[par][NP - 1 - (int)(i - nPrim)];
                    const uint32_t fl = pool_load<GUIDED, Medium::kGrey, FULL>(P, slot, S, st, sampler, &ch, isg);
                    pxy = P.i(LY::PIXEL, slot);
                    const int px = pxy & 0xffff, py = (int)((unsigned)pxy >> 16);
                    if constexpr (TRAIN) { (void)rec_bind(pxy); pool_load_rec<LY>(P, slot, pc.rec); }
                    // (full scenes: a path that crossed a medium boundary on its camera segment is still at depth 0 here)
                    seg = li_segment_a<Medium, GUIDED, FULL ? SEG_ANY : SEG_SECONDARY>(S, medium, vsp_buf, vsp_ready, px, py, st, ch, sampler,
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
                    skipped = true;
                } else if (alive) {
                    toV = vx.volume;
                    toS = !vx.volume;
                } else if (valid) {
                    emit(pxy, st.L, isg);
                    if constexpr (TRAIN) train.seg_count[rec_bind(pxy)] = pc.rec.n;  // PropagateSamples (:627) follows in k_propagate
                    pc.path();
                    const int s2 = P.i(LY::SAMPLE, slot) + sample_step;
                    P.i(LY::SAMPLE, slot) = s2;
                    restart = s2 < wave_end;
                    freed = !restart;
                }
            }
            list_push(toV, slot, s_listB, &s_cnt[D_BV + par]);
            list_push_back(toS, slot, s_listB + NP - 1, &s_cnt[D_BS + par]);
            list_push(restart, slot, s_listA[nxt], &s_cnt[D_A0 + nxt]);
            list_push(freed, slot, s_free[nxt], &s_cnt[D_NFREE + nxt]);
            if constexpr (FULL) list_push_back(skipped, slot, s_listA[nxt] + NP - 1, &s_cnt[D_A1 + nxt]);  // joins the paths the vertex phase sends on
        }
        { VSPG_PROF(PS_WG_BAR_A); __syncthreads(); }
        // the segment phase's inputs are consumed (every wave read the counts before it entered the phase)
        if (threadIdx.x == 0) {
            s_cnt[D_LNEXT] = lnext + (left > 0u ? nFresh : 0u);
            s_cnt[D_NFREE + par] = 0; s_cnt[D_A0 + par] = 0; s_cnt[D_A1 + par] = 0; s_cnt[D_CURA + par] = 0;
        }

        // ---- V: vertex processing (NEE, Russian roulette, new direction) ----------------------------
        const unsigned nBV = s_cnt[D_BV + par], nB = nBV + s_cnt[D_BS + par];
        while (true) {
            unsigned base = 0;
            if (lane == 0) base = atomicAdd(&s_cnt[D_CURB + par], 64u);
            base = __builtin_amdgcn_readfirstlane(base);
            if (base >= nB) break;
            VSPG_PROF(PS_WG_B);
            const unsigned i = base + (unsigned)lane;
            bool cont = false, restart = false, freed = false;
            int slot = 0;
            if (i < nB) {
                slot = i < nBV ? s_listB[i] : s_listB[NP - 1 - (int)(i - nBV)];
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
                    emit(P.i(LY::PIXEL, slot), st.L, isg);
                    if constexpr (TRAIN) train.seg_count[rec_bind(P.i(LY::PIXEL, slot))] = pc.rec.n;
                    pc.path();
                    const int s2 = P.i(LY::SAMPLE, slot) + sample_step;
                    P.i(LY::SAMPLE, slot) = s2;
                    restart = s2 < wave_end;
                    freed = !restart;
                }
            }
            list_push_back(cont, slot, s_listA[nxt] + NP - 1, &s_cnt[D_A1 + nxt]);
            list_push(restart, slot, s_listA[nxt], &s_cnt[D_A0 + nxt]);
            list_push(freed, slot, s_free[nxt], &s_cnt[D_NFREE + nxt]);
        }
        { VSPG_PROF(PS_WG_BAR_B); __syncthreads(); }
    }
    if constexpr (!GUIDED) {
        atomicAdd(&s_counters[CNT_PATHS], pc.paths); atomicAdd(&s_counters[CNT_SEGMENTS], pc.segments);
        atomicAdd(&s_counters[CNT_VOLUME_SCATTERS], pc.volume_scatters); atomicAdd(&s_counters[CNT_SURFACE_HITS], pc.surface_hits);
        atomicAdd(&s_counters[CNT_DENSITY_QUERIES], pc.density_queries); atomicAdd(&s_counters[CNT_SHADOW_RAYS], pc.shadow_rays);
    atomicAdd(&s_counters[CNT_SHADOW_QUERIES], pc.shadow_queries);
    }
    __syncthreads();
    if (threadIdx.x < CNT_COUNT) atomicAdd(&counters[threadIdx.x], (unsigned long long)s_counters[threadIdx.x]);
}

}  // namespace
