// vspg_train_kernels.h -- the kernels of the guiding-field update (definitions: vspg_train.h / oracle "Field::Update"): k_propagate,
// k_field_aux and k_train_* with the counting sort between them.  vspg_capi.hip launches them (train_update, upload_field).
//
// Text of vspg_capi.hip, included there once at the place where it stood: it is part of that translation unit, uses the constants
// defined above it (kBlock) and is not meant for any other unit.
#pragma once

namespace {

// PathSegmentStorage::PropagateSamples (:627) for every path of a training wave: one thread per work item
constexpr int kStagePerLane = 3;  // samples staged per lane on average (2.5 at the defaults); a wavefront that collects more flushes early (StageSink)
__global__ __launch_bounds__(kBlock) void k_propagate(TrainArgs train, int max_seg) {
    __shared__ VspgTrainSample s_stage[kBlock * kStagePerLane];  // 31 KB: five workgroups per CU
    __shared__ unsigned int s_wcount[kBlock / 64], s_wzero[kBlock / 64];
    __shared__ unsigned long long s_base;
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    PathRecorder rec;
    rec.base = train.segbuf + (i < train.n_items ? i : 0u);
    rec.stride = (int)train.n_items;
    rec.max_seg = max_seg;
    rec.reset();
    rec.n = i < train.n_items ? train.seg_count[i] : 0;
    StageSink sink{s_stage + wave * 64 * kStagePerLane, 64u * kStagePerLane, 0u, train.samples, train.counters, train.capacity};
    unsigned int zero = propagate_samples(rec, rec.n > 0, sink);
    for (int off = 32; off > 0; off >>= 1) zero += __shfl_xor(zero, off);  // (one atomic per workgroup: the counters are single words)
    if (lane == 0) { s_wcount[wave] = sink.count; s_wzero[wave] = zero; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int total = 0, zeros = 0;
        for (int w = 0; w < kBlock / 64; ++w) { total += s_wcount[w]; zeros += s_wzero[w]; }
        s_base = total ? atomicAdd(&train.counters[0], (unsigned long long)total) : 0ull;
        if (zeros) atomicAdd(&train.counters[1], (unsigned long long)zeros);
    }
    __syncthreads();
    unsigned long long base = s_base;
    for (int w = 0; w < wave; ++w) base += s_wcount[w];
    for (unsigned int j = (unsigned int)lane; j < sink.count; j += 64u)
        if (base + j < train.capacity) train.samples[base + j] = sink.stage[j];
}

// DField::aux / DField::lobes of regions [0, n_regions): the per-lobe constants every mixture evaluation needs, and the
// region records re-laid as arrays of lobes (vspg_guided_wg.h)
__global__ __launch_bounds__(kBlock) void k_field_aux(const DScene *__restrict__ Sp, int f, const VspgFieldRegion *__restrict__ regs,
                                                      float *__restrict__ aux, float4 *__restrict__ lobes) {
    const int n = Sp->field[f].n_regions * GK;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const int r = i / GK, k = i - r * GK;
        const VspgFieldRegion &R = regs[r];
        const float kc = kappa_clamp(R.kappa[k]);
        const float b = R.weight[k] * vmf_norm(kc);  // b_k (vspg_guiding.h)
        aux[(size_t)r * (2 * GK) + k] = b;
        aux[(size_t)r * (2 * GK) + GK + k] = kc;
        float4 *L = lobes + (size_t)r * kRegionLobeQuads;
        if (k == 0) L[0] = make_float4(R.pivot[0], R.pivot[1], R.pivot[2], __builtin_bit_cast(float, (int)R.n_lobes));
        L[1 + 2 * k] = make_float4(R.mu[0][k], R.mu[1][k], R.mu[2][k], R.distance[k]);
        L[2 + 2 * k] = make_float4(R.weight[k], b, kc, R.vsp[k]);
    }
}

// ---- a18: Field::Update stand-in (definitions in vspg_train.h / oracle "Field::Update") --------------
// The surface (0) and the volume (1) field are updated TOGETHER: a sample belongs to exactly one of them (its VOLUME flag),
// the two updates are independent, and every pass over the batch is bound by reading the samples -- so each pass serves both
// fields under the sort key  field * kTrainCapRegions + region  (vspg_train.h: kTrainKeys).
struct TrainFields {
    RegionStats *stats[2];
    VspgFieldRegion *regs[2];
    VspgKdNode *nodes[2];
};
__global__ __launch_bounds__(kBlock) void k_train_decay(const DScene *__restrict__ Sp, TrainFields tf) {
    for (int f = 0; f < 2; ++f) {
        const int n = Sp->field[f].n_regions * kStatFloats;
        for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
            const int r = i / kStatFloats, k = i - r * kStatFloats;
            (&tf.stats[f][r].n)[k] *= kTrainDecay;
        }
    }
}
// ---- counting sort of the batch by key -----------------------------------------------------------------
// Histograms are built per workgroup in LDS over a contiguous chunk of the batch and flushed with one global
// atomic per non-empty bin: device-scope atomics on a handful of hot addresses (few regions in the first
// iterations) cost ~300 ns each when issued per wavefront.
constexpr int kSortBlock = 1024;  // one workgroup per CU: half the flushes of two 512-thread ones at the same occupancy
__device__ __forceinline__ void train_chunk(unsigned long long n, unsigned long long *lo, unsigned long long *hi) {
    unsigned long long per = (n + gridDim.x - 1) / gridDim.x;
    per = (per + kSortBlock - 1) / kSortBlock * kSortBlock;
    *lo = (unsigned long long)blockIdx.x * per < n ? (unsigned long long)blockIdx.x * per : n;
    *hi = *lo + per < n ? *lo + per : n;
}
// s_bins[key] += 1 for every lane with key >= 0; returns the bin's value before the lane's own add.
// A few ballot rounds serve the popular bins with one LDS atomic each, the tail goes lane by lane.
__device__ __forceinline__ unsigned int lds_bin_add(unsigned int *s_bins, int key) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(key >= 0);
    unsigned int rank = 0;
    for (int round = 0; todo != 0ull && round < 4; ++round) {
        const int leader = __ffsll((long long)todo) - 1;
        const int lkey = __shfl(key, leader);
        const unsigned long long same = __ballot(key == lkey) & todo;
        unsigned int base = 0;
        if (lane == leader) base = atomicAdd(&s_bins[lkey], (unsigned int)__popcll(same));
        base = __shfl(base, leader);
        if ((same >> lane) & 1ull) rank = base + (unsigned int)__popcll(same & ((1ull << lane) - 1ull));
        todo &= ~same;
    }
    if ((todo >> lane) & 1ull) rank = atomicAdd(&s_bins[key], 1u);
    return rank;
}
// key of every sample (-1: outside its field's tree) + histogram; the first of an update's two sorts also sums the sample
// weights (sumw != nullptr).  `redo`: the second sort runs only if the split pass changed a tree (*redo != 0); otherwise
// key_of / order / n_sorted of the first sort still stand.
constexpr int kTrainLdsNodes = 512;  // upper kd-tree levels per field staged in LDS for the descent (field_lookup)
__global__ __launch_bounds__(kSortBlock) void k_train_lookup(const DScene *__restrict__ Sp, const VspgTrainSample *__restrict__ samples,
                                                         unsigned long long n, int *__restrict__ key_of, unsigned int *__restrict__ hist,
                                                         float *__restrict__ sumw, const int *__restrict__ redo) {
    __shared__ unsigned int s_hist[kTrainKeys];
    __shared__ VspgKdNode s_nodes[2 * kTrainLdsNodes];
    if (redo && *redo == 0) return;
    const DScene &S = *Sp;
    int nl[2];
    for (int f = 0; f < 2; ++f) {
        nl[f] = S.field[f].n_nodes < kTrainLdsNodes ? S.field[f].n_nodes : kTrainLdsNodes;
        for (int i = threadIdx.x; i < nl[f]; i += kSortBlock) s_nodes[f * kTrainLdsNodes + i] = S.field[f].nodes[i];
    }
    for (int b = threadIdx.x; b < kTrainKeys; b += kSortBlock) s_hist[b] = 0;
    __syncthreads();
    unsigned long long lo, hi;
    train_chunk(n, &lo, &hi);
    float wsum = 0;
    for (unsigned long long i0 = lo; i0 < hi; i0 += kSortBlock) {
        const unsigned long long i = i0 + threadIdx.x;
        int key = -1;
        if (i < hi) {
            const VspgTrainSample sm = samples[i];
            const int f = (sm.flags & VSPG_SAMPLE_VOLUME) ? 1 : 0;
            const int region = field_lookup(S.field[f], ld3(sm.p), s_nodes + f * kTrainLdsNodes, nl[f]);
            if (region >= 0) key = f * kTrainCapRegions + region;
            key_of[i] = key;
            wsum += sm.weight;
        }
        lds_bin_add(s_hist, key);
    }
    if (sumw) {
        for (int off = 32; off > 0; off >>= 1) wsum += __shfl_xor(wsum, off);
        if ((threadIdx.x & 63) == 0 && wsum != 0.f) atomicAdd(sumw, wsum);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < kTrainKeys; b += kSortBlock)
        if (s_hist[b]) atomicAdd(&hist[b], s_hist[b]);
}
// exclusive scan of the histogram -> start offsets (one block); cursor = copy for the scatter; total -> *n_sorted
__global__ __launch_bounds__(kBlock) void k_train_scan(const unsigned int *__restrict__ hist, unsigned int *__restrict__ cursor,
                                                       unsigned int *__restrict__ n_sorted, const int *__restrict__ redo) {
    __shared__ unsigned int s_part[kBlock];
    if (redo && *redo == 0) return;
    constexpr int per = (kTrainKeys + kBlock - 1) / kBlock;
    const int lo = threadIdx.x * per < kTrainKeys ? threadIdx.x * per : kTrainKeys, hi = lo + per < kTrainKeys ? lo + per : kTrainKeys;
    unsigned int sum = 0;
    for (int i = lo; i < hi; ++i) sum += hist[i];
    s_part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int run = 0;
        for (int t = 0; t < kBlock; ++t) { const unsigned int v = s_part[t]; s_part[t] = run; run += v; }
        *n_sorted = run;
    }
    __syncthreads();
    unsigned int run = s_part[threadIdx.x];
    for (int i = lo; i < hi; ++i) { cursor[i] = run; run += hist[i]; }
}
// a workgroup recounts its chunk, reserves one range per non-empty bin, then places its samples
__global__ __launch_bounds__(kSortBlock) void k_train_scatter(const int *__restrict__ key_of, unsigned long long n, unsigned int *__restrict__ cursor,
                                                          unsigned int *__restrict__ order, const int *__restrict__ redo) {
    __shared__ unsigned int s_cur[kTrainKeys];
    if (redo && *redo == 0) return;
    for (int b = threadIdx.x; b < kTrainKeys; b += kSortBlock) s_cur[b] = 0;
    __syncthreads();
    unsigned long long lo, hi;
    train_chunk(n, &lo, &hi);
    for (unsigned long long i0 = lo; i0 < hi; i0 += kSortBlock) {
        const unsigned long long i = i0 + threadIdx.x;
        lds_bin_add(s_cur, i < hi ? key_of[i] : -1);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < kTrainKeys; b += kSortBlock) {
        const unsigned int c = s_cur[b];
        s_cur[b] = c ? atomicAdd(&cursor[b], c) : 0u;  // from a count to the chunk's first slot of the bin
    }
    __syncthreads();
    for (unsigned long long i0 = lo; i0 < hi; i0 += kSortBlock) {
        const unsigned long long i = i0 + threadIdx.x;
        const int key = i < hi ? key_of[i] : -1;
        const unsigned int slot = lds_bin_add(s_cur, key);
        if (key >= 0) order[slot] = (unsigned int)i;
    }
}
// every wavefront takes a contiguous piece of the sorted order
__device__ __forceinline__ void train_piece(unsigned int n_sorted, unsigned int *lo, unsigned int *hi) {
    const unsigned int waves = gridDim.x * (kBlock / 64), w = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    unsigned int per = (n_sorted + waves - 1) / waves;
    per = (per + 63u) & ~63u;
    *lo = w * per < n_sorted ? w * per : n_sorted;
    *hi = *lo + per < n_sorted ? *lo + per : n_sorted;
}
// position statistics {n, sum p, [sum p^2]} of the batch per key -> acc
// (`need`: the pass after the split serves k_train_init_regions only -- it runs when a region without lobes exists, flags[1] of k_train_split)
template <bool WITH_P2>
__global__ __launch_bounds__(kBlock) void k_train_pos(const VspgTrainSample *__restrict__ samples, const int *__restrict__ key_of,
                                                      const unsigned int *__restrict__ order, const unsigned int *__restrict__ n_sorted,
                                                      float *__restrict__ acc, const int *__restrict__ need) {
    if (need && *need == 0) return;
    unsigned int lo, hi;
    train_piece(*n_sorted, &lo, &hi);
    constexpr int NV = WITH_P2 ? 7 : 4;
    RunAccumulator<NV> R;
    R.init(acc, 0);
    for (unsigned int j0 = lo; j0 < hi; j0 += 64u) {
        const unsigned int j = j0 + (threadIdx.x & 63);
        const bool valid = j < hi;
        float v[RunAccumulator<NV>::P];
        int key = -1;
        for (int k = 0; k < RunAccumulator<NV>::P; ++k) v[k] = 0.f;
        if (valid) {
            const unsigned int i = order[j];
            key = key_of[i];
            const VspgTrainSample sm = samples[i];
            v[0] = 1.f; v[1] = sm.p[0]; v[2] = sm.p[1]; v[3] = sm.p[2];
            if constexpr (WITH_P2) { v[4] = sm.p[0] * sm.p[0]; v[5] = sm.p[1] * sm.p[1]; v[6] = sm.p[2] * sm.p[2]; }
        }
        R.add(valid, key, v);
    }
    R.flush();
}
// spatial refinement: one workgroup per field, sequential in meaning like the CPU definition so node / region numbering is the same
constexpr int kSplitBlock = 1024;
// flags[0] += regions created (the second sort runs only then), flags[1] |= a region without lobes exists (k_train_init_regions has work)
__global__ __launch_bounds__(kSplitBlock) void k_train_split(DScene *Sp, TrainFields tf, const float *acc_all, int *flags) {
    // The definition is sequential over the nodes (oracle/vspg_oracle.c:field_update_one): a leaf that wants to
    // split takes the next two node slots and the next region slot, until a capacity runs out.  Slots only grow,
    // so "rank among the wanting leaves" (a prefix sum) reproduces the sequential numbering exactly.
    __shared__ unsigned int s_wave[kSplitBlock / 64];
    __shared__ int s_n_nodes, s_n_regions;
    const int f = blockIdx.x;
    DField &F = Sp->field[f];
    RegionStats *stats = tf.stats[f];
    VspgFieldRegion *regs = tf.regs[f];
    VspgKdNode *nodes = tf.nodes[f];
    const float *acc = acc_all + (size_t)f * kTrainCapRegions * kStatFloats;
    const int n_reg0 = F.n_regions, n_nodes0 = F.n_nodes;
    bool bare = false;
    for (int i = threadIdx.x; i < n_reg0; i += kSplitBlock) {
        const float *a = acc + (size_t)i * kStatFloats;
        stats[i].n += a[0];
        for (int k = 0; k < 3; ++k) { stats[i].sum_p[k] += a[1 + k]; stats[i].sum_p2[k] += a[4 + k]; }
        bare = bare || regs[i].n_lobes == 0;  // (the regions a split creates are copies of these)
    }
    if (__ballot(bare) != 0ull && (threadIdx.x & 63) == 0) atomicOr(&flags[1], 1);
    __syncthreads();
    constexpr int kPer = (kTrainCapNodes + kSplitBlock - 1) / kSplitBlock;
    const int first = threadIdx.x * kPer;
    unsigned int want = 0;
    int axis_of[kPer];
    float split_of[kPer];
    for (int j = 0; j < kPer; ++j) {
        const int nd = first + j;
        axis_of[j] = 0; split_of[j] = 0;
        if (nd >= n_nodes0 || (nodes[nd].packed & 3u) != 3u) continue;
        const RegionStats &s0 = stats[nodes[nd].packed >> 2];
        if (!(s0.n > kTrainSplitCount) || s0.depth >= kTrainMaxDepth) continue;
        float mean[3], var[3];
        for (int k = 0; k < 3; ++k) {
            mean[k] = s0.sum_p[k] / s0.n;
            var[k] = s0.sum_p2[k] / s0.n - mean[k] * mean[k];
        }
        const int axis = var[0] >= var[1] ? (var[0] >= var[2] ? 0 : 2) : (var[1] >= var[2] ? 1 : 2);
        if (!(var[axis] > 0)) continue;
        want |= 1u << j;
        axis_of[j] = axis;
        split_of[j] = mean[axis];
    }
    // exclusive prefix sum of popc(want) over the threads: within the wavefront by shuffles, across wavefronts through LDS
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned int mine = (unsigned int)__popc(want);
    unsigned int incl = mine;
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned int up = __shfl_up(incl, off);
        if (lane >= off) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    unsigned int before = 0, total = 0;
    for (int w = 0; w < kSplitBlock / 64; ++w) {
        const unsigned int c = s_wave[w];
        if (w < wave) before += c;
        total += c;
    }
    if (threadIdx.x == 0) {
        // how many of the `total` candidates fit: both capacities
        int fit = (int)total;
        if (fit > (kTrainCapNodes - n_nodes0) / 2) fit = (kTrainCapNodes - n_nodes0) / 2;
        if (fit > kTrainCapRegions - n_reg0) fit = kTrainCapRegions - n_reg0;
        if (fit < 0) fit = 0;
        s_n_nodes = n_nodes0 + 2 * fit;
        s_n_regions = n_reg0 + fit;
        if (fit) atomicAdd(&flags[0], fit);
    }
    int rank = (int)(before + incl - mine);
    for (int j = 0; j < kPer; ++j) {
        if (!((want >> j) & 1u)) continue;
        const int left = n_nodes0 + 2 * rank, newreg = n_reg0 + rank;
        ++rank;
        if (left + 2 > kTrainCapNodes || newreg + 1 > kTrainCapRegions) continue;
        const int nd = first + j;
        const int reg = (int)(nodes[nd].packed >> 2);
        RegionStats &s0 = stats[reg];
        float *v = &s0.n;
        for (int k = 0; k < kStatFloats; ++k) v[k] *= 0.5f;
        s0.depth += 1;
        stats[newreg] = s0;
        regs[newreg] = regs[reg];
        nodes[left].split = 0; nodes[left].packed = ((uint32_t)reg << 2) | 3u;
        nodes[left + 1].split = 0; nodes[left + 1].packed = ((uint32_t)newreg << 2) | 3u;
        nodes[nd].split = split_of[j];
        nodes[nd].packed = ((uint32_t)left << 2) | (uint32_t)axis_of[j];
    }
    __syncthreads();
    if (threadIdx.x == 0) { F.n_nodes = s_n_nodes; F.n_regions = s_n_regions; }
}
__global__ __launch_bounds__(kBlock) void k_train_init_regions(const DScene *__restrict__ Sp, TrainFields tf, const float *__restrict__ acc) {
    const int key = blockIdx.x * kBlock + threadIdx.x;
    if (key >= kTrainKeys) return;
    const int f = key >= kTrainCapRegions ? 1 : 0, i = key - f * kTrainCapRegions;
    if (i >= Sp->field[f].n_regions) return;
    const float *a = acc + (size_t)key * kStatFloats;
    VspgFieldRegion &R = tf.regs[f][i];
    if (R.n_lobes == 0 && a[0] > 0) {
        for (int k = 0; k < 3; ++k) R.pivot[k] = a[1 + k] / a[0];
        region_init_lobes(R);
    }
}
__global__ __launch_bounds__(kBlock) void k_train_estep(const DScene *__restrict__ Sp, const VspgTrainSample *__restrict__ samples,
                                                        const int *__restrict__ key_of, const unsigned int *__restrict__ order,
                                                        const unsigned int *__restrict__ n_sorted, const float *__restrict__ sumw,
                                                        float *__restrict__ acc) {
    const DScene &S = *Sp;
    vspg_libm::stage_logf_tab_lds();
    __syncthreads();
    const float wmax = kTrainWeightClamp * (sumw[0] / sumw[1]);  // mean sample weight: sum / count, both over ALL ranks' samples (train_update)
    unsigned int lo, hi;
    train_piece(*n_sorted, &lo, &hi);
    RunAccumulator<8 * GK> R;
    R.init(acc, 7);
    for (unsigned int j0 = lo; j0 < hi; j0 += 64u) {
        const unsigned int j = j0 + (threadIdx.x & 63);
        bool valid = j < hi;
        int key = -1;
        float vals[8 * GK];  // S, R0, R1, R2, D, V, Qv, Qs -- the order of RegionStats
        for (int k = 0; k < 8 * GK; ++k) vals[k] = 0.f;
        if (valid) {
            const unsigned int i = order[j];
            key = key_of[i];
            const VspgTrainSample sm = samples[i];
            const int f = key >= kTrainCapRegions ? 1 : 0;
            const VspgFieldRegion &Rg = S.field[f].regions[key - f * kTrainCapRegions];
            const int nl = Rg.n_lobes < GK ? Rg.n_lobes : GK;
            valid = nl > 0;
            if (valid) {
                const float w = sm.weight < wmax ? sm.weight : wmax;
                const V3 om = train_reaim(Rg, ld3(sm.p), ld3(sm.dir), sm.distance);
                float g[GK], gs = 0;
                for (int k = 0; k < GK; ++k) {
                    g[k] = k < nl ? Rg.weight[k] * vmf_eval(V3{Rg.mu[0][k], Rg.mu[1][k], Rg.mu[2][k]}, kappa_clamp(Rg.kappa[k]), om) : 0.f;
                    gs += g[k];
                }
                valid = gs > 0 && !isinf_(gs);
                if (valid) {
                    const bool nextvol = (sm.flags & VSPG_SAMPLE_NEXT_VOLUME) != 0;
                    const bool hasd = sm.distance > 0 && !isinf_(sm.distance);
                    for (int k = 0; k < GK; ++k) {
                        const float wg = w * (g[k] / gs);
                        vals[0 * GK + k] = wg;
                        vals[1 * GK + k] = wg * om.x; vals[2 * GK + k] = wg * om.y; vals[3 * GK + k] = wg * om.z;
                        vals[4 * GK + k] = hasd ? wg / sm.distance : 0.f;
                        vals[5 * GK + k] = nextvol ? wg : 0.f;
                        vals[6 * GK + k] = nextvol ? wg * w : 0.f;
                        vals[7 * GK + k] = nextvol ? 0.f : wg * w;
                    }
                }
            }
        }
        R.add(valid, key, vals);
    }
    R.flush();
}
__global__ __launch_bounds__(kBlock) void k_train_mstep(const DScene *__restrict__ Sp, TrainFields tf, const float *__restrict__ acc) {
    const int key = blockIdx.x * kBlock + threadIdx.x;
    if (key >= kTrainKeys) return;
    const int f = key >= kTrainCapRegions ? 1 : 0, i = key - f * kTrainCapRegions;
    if (i >= Sp->field[f].n_regions) return;
    VspgFieldRegion &R = tf.regs[f][i];
    if (R.n_lobes <= 0) return;
    const int nl = R.n_lobes < GK ? R.n_lobes : GK;
    RegionStats &s1 = tf.stats[f][i];
    const float *a = acc + (size_t)key * kStatFloats + 7;
    float Stot = 0;
    for (int k = 0; k < nl; ++k) {
        s1.S[k] += a[0 * GK + k];
        s1.R[0][k] += a[1 * GK + k]; s1.R[1][k] += a[2 * GK + k]; s1.R[2][k] += a[3 * GK + k];
        s1.D[k] += a[4 * GK + k]; s1.V[k] += a[5 * GK + k]; s1.Qv[k] += a[6 * GK + k]; s1.Qs[k] += a[7 * GK + k];
        Stot += s1.S[k];
    }
    if (!(Stot > 0)) return;
    const float floorw = 1e-3f / GK;
    float wsum = 0;
    for (int k = 0; k < nl; ++k) {
        float wk = s1.S[k] / Stot;
        wk = wk < floorw ? floorw : wk;
        R.weight[k] = wk;
        wsum += wk;
        const float rl = sqrtf(s1.R[0][k] * s1.R[0][k] + s1.R[1][k] * s1.R[1][k] + s1.R[2][k] * s1.R[2][k]);
        if (s1.S[k] > 0 && rl > 0) {
            R.mu[0][k] = s1.R[0][k] / rl; R.mu[1][k] = s1.R[1][k] / rl; R.mu[2][k] = s1.R[2][k] / rl;
            float rbar = rl / s1.S[k];
            rbar = rbar > 0.9999f ? 0.9999f : rbar;
            R.kappa[k] = kappa_clamp(rbar * (3 - rbar * rbar) / (1 - rbar * rbar));
            R.distance[k] = s1.D[k] > 0 ? s1.S[k] / s1.D[k] : kInf;
            if (Sp->prm.vspcriterion == VSPG_VSP_VARIANCE) {
                const float qv = sqrtf(s1.Qv[k]), qs = sqrtf(s1.Qs[k]);
                R.vsp[k] = qv + qs > 0 ? qv / (qv + qs) : 0.5f;
            } else {
                R.vsp[k] = s1.V[k] / s1.S[k];
            }
        }
    }
    for (int k = 0; k < nl; ++k) R.weight[k] = R.weight[k] / wsum;
}

}  // namespace
