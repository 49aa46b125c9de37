// What a scalar (lane-mask) instruction costs a vector-issue-bound kernel on gfx950 -- a sibling of issue.hip, same method: every
// wave stamps s_memtime / s_memrealtime around its loop, the streams are inline assembly, a launch lasts milliseconds and follows
// warm-up launches, the figure is the median over waves.
//   hipcc --offload-arch=gfx950 -O3 -o scalar_issue scalar_issue.hip && ./scalar_issue
//
// Mixed rows: issue.hip's path-kernel-like mix of 32 vector instructions per iteration, with 0, 10, 20 or 32 scalar instructions
// interleaved (0, 0.31, 0.62, 1.0 per vector instruction), at the headline kernel's occupancy: 512-thread workgroups, two per CU
// (each holds 80 000 B of LDS, so a CU takes two and no more), four waves per SIMD -- checked, not assumed: the occupancy query's
// answer and the waves found resident on a SIMD (HW_REG_HW_ID, s_memrealtime) are printed with every row.  Two flavours:
//   logic : s_and_b64 / s_or_b64 / s_andn2_b64 on SGPR pairs, four independent chains;
//   exec  : s_and_saveexec_b64 before a vector instruction and s_or_b64 exec, exec, saved behind it (the mask is all ones, so the
//           vector work is unchanged; two scalar instructions per region).
// Figure: SIMD-cycles per vector wave-instruction = the SIMD's own time (first of its waves into the loop to the last out of it, in
// s_memrealtime ticks x the clock) / (N x 32 x waves it held); the median of the waves' own d memtime / 4 is printed beside it.  The
// price of a scalar instruction is the difference of two rows over the difference of their scalar counts.  The same rows run in
// issue.hip's launch shape (256-thread workgroups, four per CU), and the 20-instruction row in three placements.
//
// Scalar-only rows: 32 lane-mask logic instructions per iteration and nothing else, one workgroup of 1, 4 or 16 waves per CU (100 000 B
// of LDS: one workgroup per CU).  If every SIMD issued scalar instructions on its own, 4 waves (one per SIMD) would take the time of 1
// and 16 four times that; if the CU's four SIMDs share one scalar issue port, the time grows with the waves per CU throughout.
//
// Only register-to-register instructions of the scalar ALU are used: lane-mask logic, moves, exec save / restore.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#define N (1 << 15)

struct Stamp {
    unsigned long long cyc, real, begin;   // shader cycles and 100 MHz ticks of the loop, the tick it began at
    unsigned int hw_id, xcc_id;            // where the wave ran (HW_REG_HW_ID: wave 3:0, SIMD 5:4, CU 11:8, SH 12, SE 15:13; HW_REG_XCC_ID 3:0)
};
// Every row checks the occupancy it claims from these stamps: for each wave, how many waves of the launch were in their loops on the
// same SIMD (same XCC, SE, SH, CU, SIMD) at the middle of its own loop, itself included; the median over waves is printed beside the
// figure as "resident".  The ticks are one free-running counter, compared only between waves of one SIMD.
#define STAMP(t_, r_, r0_) Stamp{t_, r_, r0_, (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4), (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 20)}

// the 32 vector instructions of issue.hip's M_MIX, one per slot; operand numbers as in MIX's constraint lists
#define V00 "v_fma_f32 %0, %0, %12, %13\n\t"
#define V01 "v_mul_f32 %1, %1, %12\n\t"
#define V02 "v_add_f32 %2, %2, %13\n\t"
#define V03 "v_fma_f32 %3, %3, %12, %13\n\t"
#define V04 "v_add_u32 %4, %4, %5\n\t"
#define V05 "v_mul_f32 %0, %0, %12\n\t"
#define V06 "v_cmp_lt_f32 vcc, %0, %1\n\t"
#define V07 "v_cndmask_b32 %2, %2, %3, vcc\n\t"
#define V08 "v_mad_u64_u32 %6, vcc, %4, %5, %6\n\t"
#define V09 "v_fma_f32 %1, %1, %12, %13\n\t"
#define V10 "v_add_f32 %3, %3, %13\n\t"
#define V11 "v_mul_lo_u32 %5, %5, %4\n\t"
#define V12 "v_fma_f64 %7, %7, %14, %15\n\t"
#define V13 "v_fma_f32 %0, %0, %12, %13\n\t"
#define V14 "v_mul_f32 %2, %2, %12\n\t"
#define V15 "v_xor_b32 %4, %4, %5\n\t"
#define V16 "v_rcp_f32 %3, %3\n\t"
#define V17 "v_fma_f32 %1, %1, %12, %13\n\t"
#define V18 "v_add_f32 %0, %0, %13\n\t"
#define V19 "v_lshrrev_b32 %5, 3, %5\n\t"
#define V20 "v_mad_u64_u32 %6, vcc, %5, %4, %6\n\t"
#define V21 "v_mul_f32 %2, %2, %12\n\t"
#define V22 "v_cmp_gt_f32 vcc, %2, %0\n\t"
#define V23 "v_cndmask_b32 %1, %1, %0, vcc\n\t"
#define V24 "v_fma_f64 %7, %7, %14, %15\n\t"
#define V25 "v_fma_f32 %3, %3, %12, %13\n\t"
#define V26 "v_ldexp_f32 %0, %0, %16\n\t"
#define V27 "v_add_u32 %4, %4, %5\n\t"
#define V28 "v_fma_f32 %2, %2, %12, %13\n\t"
#define V29 "v_add_f32 %1, %1, %13\n\t"
#define V30 "v_and_b32 %5, %5, %4\n\t"
#define V31 "v_mul_f32 %3, %3, %12\n\t"
// scalar slots: nothing; lane-mask logic on the pairs %8..%11 (four chains, %17 = a constant mask); an exec region's two ends
#define __ ""
#define LA "s_and_b64 %8, %8, %17\n\t"
#define LB "s_or_b64 %9, %9, %17\n\t"
#define LC "s_andn2_b64 %10, %10, %17\n\t"
#define LD "s_or_b64 %11, %11, %8\n\t"
#define XO "s_and_saveexec_b64 %8, %18\n\t"   // %18 = all ones: exec stays what it was
#define XC "s_or_b64 exec, exec, %8\n\t"
// the mix with one scalar slot behind every vector instruction
#define MIX(s00, s01, s02, s03, s04, s05, s06, s07, s08, s09, s10, s11, s12, s13, s14, s15, s16, s17, s18, s19, s20, s21, s22, s23, s24, s25, s26, s27, \
            s28, s29, s30, s31)                                                                                                                       \
    asm volatile(V00 s00 V01 s01 V02 s02 V03 s03 V04 s04 V05 s05 V06 s06 V07 s07 V08 s08 V09 s09 V10 s10 V11 s11 V12 s12 V13 s13 V14 s14 V15 s15 V16 s16   \
                     V17 s17 V18 s18 V19 s19 V20 s20 V21 s21 V22 s22 V23 s23 V24 s24 V25 s25 V26 s26 V27 s27 V28 s28 V29 s29 V30 s30 V31 s31            \
                 : "+v"(f0), "+v"(f1), "+v"(f2), "+v"(f3), "+v"(a0), "+v"(a1), "+v"(q0), "+v"(d0), "+s"(m0), "+s"(m1), "+s"(m2), "+s"(m3)             \
                 : "v"(c0), "v"(c1), "v"(dc0), "v"(dc1), "v"(0), "s"(mk), "s"(ones)                                                                   \
                 : "vcc", "scc")

enum { R_BASE = 0, R_LOGIC_10, R_LOGIC_20, R_LOGIC_32, R_EXEC_10, R_EXEC_20, R_EXEC_32, R_LOGIC_20_RUNS, R_LOGIC_20_BLOCK, R_COUNT };
static const char *kRowName[R_COUNT] = {"mix alone", "mix + 10 mask-logic", "mix + 20 mask-logic", "mix + 32 mask-logic",
                                        "mix + 5 exec regions (10 scalar)", "mix + 10 exec regions (20 scalar)", "mix + 16 exec regions (32 scalar)",
                                        "mix + 20 mask-logic in runs of 5", "mix + 20 mask-logic in one block"};
static const int kRowScalar[R_COUNT] = {0, 10, 20, 32, 10, 20, 32, 20, 20};
#define L5 LA LB LC LD LA

constexpr int kPadTwoPerCu = 80000, kPadFourPerCu = 40000, kPadOnePerCu = 100000, kNoPad = 2048;

template <int ROW, int THREADS, int PAD>
__global__ __launch_bounds__(THREADS) void k_mixed(Stamp *out, float *sink, uint32_t seed) {
    __shared__ float pad[PAD / 4];   // LDS that lets a CU take so many workgroups and no more
    pad[threadIdx.x] = (float)seed;
    float f0 = 1.0f + (float)(threadIdx.x & 7) * 0.125f + seed * 1e-9f, f1 = f0 + 0.25f, f2 = f0 + 0.5f, f3 = f0 + 0.75f;
    const float c0 = 0.999999f, c1 = 1e-7f;
    uint32_t a0 = seed + threadIdx.x, a1 = a0 * 3 + 1;
    uint64_t q0 = a0;
    double d0 = f0;
    const double dc0 = 0.999999, dc1 = 1e-7;
    unsigned long long m0 = __builtin_amdgcn_read_exec(), m1 = m0 >> 1, m2 = m0 >> 2, m3 = m0 >> 3;
    const unsigned long long mk = 0x5555aaaa3333ccccull, ones = ~0ull;
    asm volatile("" : "+s"(m0), "+s"(m1), "+s"(m2), "+s"(m3));
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    for (int i = 0; i < N; ++i) {
        if (ROW == R_BASE) MIX(__, __, __, __, __, __, __, __, __, __, __, __, __, __, __, __, __, __, __, __, __, __, __, __, __, __, __, __, __, __, __, __);
        if (ROW == R_LOGIC_10) MIX(LA, __, __, LB, __, __, LC, __, __, LD, __, __, LA, __, __, __, LB, __, __, LC, __, __, LD, __, __, LA, __, __, LB, __, __, __);
        if (ROW == R_LOGIC_20) MIX(LA, LB, __, LC, LD, __, LA, __, LB, LC, __, LD, LA, __, LB, __, LC, LD, __, LA, LB, __, LC, __, LD, LA, __, LB, LC, __, LD, __);
        if (ROW == R_LOGIC_32) MIX(LA, LB, LC, LD, LA, LB, LC, LD, LA, LB, LC, LD, LA, LB, LC, LD, LA, LB, LC, LD, LA, LB, LC, LD, LA, LB, LC, LD, LA, LB, LC, LD);
        if (ROW == R_EXEC_10) MIX(XO, XC, __, __, __, __, XO, XC, __, __, __, __, XO, XC, __, __, __, __, __, XO, XC, __, __, __, __, XO, XC, __, __, __, __, __);
        if (ROW == R_EXEC_20) MIX(XO, XC, __, XO, XC, __, XO, XC, __, XO, XC, __, XO, XC, __, __, XO, XC, __, XO, XC, __, XO, XC, __, XO, XC, __, XO, XC, __, __);
        if (ROW == R_EXEC_32) MIX(XO, XC, XO, XC, XO, XC, XO, XC, XO, XC, XO, XC, XO, XC, XO, XC, XO, XC, XO, XC, XO, XC, XO, XC, XO, XC, XO, XC, XO, XC, XO, XC);
        // the same 20 scalar instructions placed differently: four runs of five, one block of twenty
        if (ROW == R_LOGIC_20_RUNS) MIX(__, __, __, L5, __, __, __, __, __, __, __, L5, __, __, __, __, __, __, __, L5, __, __, __, __, __, __, __, L5, __, __, __, __);
        if (ROW == R_LOGIC_20_BLOCK) MIX(__, __, __, __, __, __, __, __, __, __, __, __, __, __, __, L5 L5 L5 L5, __, __, __, __, __, __, __, __, __, __, __, __, __, __, __, __);
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    if ((threadIdx.x & 63) == 0) out[blockIdx.x * 16 + (threadIdx.x >> 6)] = STAMP(t1 - t0, r1 - r0, r0);
    sink[blockIdx.x * blockDim.x + threadIdx.x] = f0 + f1 + f2 + f3 + (float)(a0 + a1) + (float)q0 + (float)d0 + (float)(unsigned)(m0 ^ m1 ^ m2 ^ m3) + pad[(threadIdx.x * 7) & 255];
}

// 32 lane-mask logic instructions per iteration and nothing else
__global__ __launch_bounds__(1024) void k_scalar(Stamp *out, float *sink, uint32_t seed) {
    __shared__ float pad[kPadOnePerCu / 4];   // one workgroup per CU
    pad[threadIdx.x] = (float)seed;
    unsigned long long m0 = __builtin_amdgcn_read_exec(), m1 = m0 >> 1, m2 = m0 >> 2, m3 = m0 >> 3, mk = 0x5555aaaa3333ccccull + seed;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    for (int i = 0; i < N; ++i) {
#define S4 "s_and_b64 %0, %0, %4\n\ts_or_b64 %1, %1, %4\n\ts_andn2_b64 %2, %2, %4\n\ts_or_b64 %3, %3, %0\n\t"
        asm volatile(S4 S4 S4 S4 S4 S4 S4 S4 : "+s"(m0), "+s"(m1), "+s"(m2), "+s"(m3) : "s"(mk) : "scc");
#undef S4
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    if ((threadIdx.x & 63) == 0) out[blockIdx.x * 16 + (threadIdx.x >> 6)] = STAMP(t1 - t0, r1 - r0, r0);
    sink[blockIdx.x * blockDim.x + threadIdx.x] = (float)(unsigned)(m0 ^ m1 ^ m2 ^ m3) + pad[(threadIdx.x * 7) & 63];
}

static void median(const std::vector<Stamp> &h, double *cycles, double *ghz) {
    std::vector<double> cyc, clk;
    for (auto &s : h) {
        cyc.push_back((double)s.cyc);
        clk.push_back((double)s.cyc / (double)s.real * 0.1);
    }
    std::sort(cyc.begin(), cyc.end());
    std::sort(clk.begin(), clk.end());
    *cycles = cyc[cyc.size() / 2];
    *ghz = clk[clk.size() / 2];
}
// waves in their loops on the same SIMD at the middle of a wave's own loop (itself included), median over waves; CUs seen; and the
// SIMD's own time: from the first of its waves entering the loop to the last leaving it, in 100 MHz ticks per wave it held, median
// over SIMDs.  The waves of a SIMD do not advance evenly (with vector instructions alone some finish long before others, and the
// median of the waves' own times moves by 20 % from launch to launch); what the SIMD took for all of them does not depend on that.
static void residency(const std::vector<Stamp> &h, int *per_simd, int *cus_seen, double *ticks_per_wave) {
    const auto simd_key = [](const Stamp &s) { return ((unsigned long long)(s.xcc_id & 15u) << 16) | (s.hw_id & 0xff30u); };
    std::vector<size_t> order(h.size());
    for (size_t i = 0; i < h.size(); ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return simd_key(h[a]) < simd_key(h[b]); });
    std::vector<int> counts;
    std::vector<double> spans;
    std::vector<unsigned long long> cu_keys;
    for (size_t a = 0; a < order.size();) {
        size_t b = a;
        while (b < order.size() && simd_key(h[order[b]]) == simd_key(h[order[a]])) ++b;
        cu_keys.push_back(simd_key(h[order[a]]) & ~0x30ull);
        unsigned long long first = ~0ull, last = 0;
        for (size_t i = a; i < b; ++i) {
            first = std::min(first, h[order[i]].begin);
            last = std::max(last, h[order[i]].begin + h[order[i]].real);
        }
        spans.push_back((double)(last - first) / (double)(b - a));
        for (size_t i = a; i < b; ++i) {
            const Stamp &w = h[order[i]];
            const unsigned long long mid = w.begin + w.real / 2;
            int n = 0;
            for (size_t j = a; j < b; ++j) n += h[order[j]].begin <= mid && mid <= h[order[j]].begin + h[order[j]].real;
            counts.push_back(n);
        }
        a = b;
    }
    std::sort(counts.begin(), counts.end());
    std::sort(cu_keys.begin(), cu_keys.end());
    std::sort(spans.begin(), spans.end());
    *ticks_per_wave = spans[spans.size() / 2];
    *per_simd = counts[counts.size() / 2];
    *cus_seen = (int)(std::unique(cu_keys.begin(), cu_keys.end()) - cu_keys.begin());
}

#define CHECK(x)                                                                          \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess) {                                                           \
            printf("%s: %s\n", #x, hipGetErrorString(e_));                                \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)

// THREADS-wide workgroups, PER_CU of them per CU: PER_CU x THREADS / 256 waves per SIMD
template <int ROW, int THREADS, int PAD, int PER_CU>
int run_mixed(Stamp *d, float *sink, int cus, double *per_vector) {
    constexpr int kWaves = THREADS / 64, kPerSimd = PER_CU * THREADS / 256;
    const int blocks = cus * PER_CU;
    int fit = 0;
    CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&fit, k_mixed<ROW, THREADS, PAD>, THREADS, 0));
    for (int r = 0; r < 4; ++r) hipLaunchKernelGGL((k_mixed<ROW, THREADS, PAD>), dim3(blocks), dim3(THREADS), 0, 0, d, sink, 1u + r);
    CHECK(hipDeviceSynchronize());   // the measured launch starts on an empty chip: its workgroups enter their loops together
    hipLaunchKernelGGL((k_mixed<ROW, THREADS, PAD>), dim3(blocks), dim3(THREADS), 0, 0, d, sink, 17u);
    CHECK(hipDeviceSynchronize());
    std::vector<Stamp> h((size_t)blocks * 16);
    CHECK(hipMemcpy(h.data(), d, (size_t)blocks * 16 * sizeof(Stamp), hipMemcpyDeviceToHost));
    std::vector<Stamp> used;
    for (int b = 0; b < blocks; ++b) used.insert(used.end(), h.begin() + b * 16, h.begin() + b * 16 + kWaves);
    double cyc, ghz, ticks;
    int resident, cus_seen;
    median(used, &cyc, &ghz);
    residency(used, &resident, &cus_seen, &ticks);
    *per_vector = ticks * 10.0 * ghz / ((double)N * 32);   // the SIMD's time per wave it held, in shader cycles, per vector instruction
    printf("%-36s %dx%d LDS %6d  scalar/vector %.3f  %7.3f SIMD-cycles per vector wave-instruction (median of the waves' own times / %d: %6.3f)  resident %d of %d per SIMD on %d CUs, %d workgroups fit a CU  clock %.3f GHz  loop %.1f ms%s\n",
           kRowName[ROW], PER_CU, THREADS, PAD, kRowScalar[ROW] / 32.0, *per_vector, kPerSimd, cyc / ((double)N * 32 * kPerSimd), resident, kPerSimd, cus_seen, fit, ghz,
           cyc / ghz * 1e-6, resident == kPerSimd ? "" : "  (fewer at a wave's middle: the waves did not advance evenly)");
    return 0;
}

int run_scalar(Stamp *d, float *sink, int cus, int waves) {
    for (int r = 0; r < 4; ++r) hipLaunchKernelGGL(k_scalar, dim3(cus), dim3(64 * waves), 0, 0, d, sink, 1u + r);
    CHECK(hipDeviceSynchronize());
    hipLaunchKernelGGL(k_scalar, dim3(cus), dim3(64 * waves), 0, 0, d, sink, 17u);
    CHECK(hipDeviceSynchronize());
    std::vector<Stamp> h((size_t)cus * 16);
    CHECK(hipMemcpy(h.data(), d, (size_t)cus * 16 * sizeof(Stamp), hipMemcpyDeviceToHost));
    std::vector<Stamp> used;
    for (int b = 0; b < cus; ++b) used.insert(used.end(), h.begin() + b * 16, h.begin() + b * 16 + waves);
    double cyc, ghz, ticks;
    int resident, cus_seen;
    median(used, &cyc, &ghz);
    residency(used, &resident, &cus_seen, &ticks);
    printf("scalar only, %2d waves per CU: %7.3f cycles per scalar instruction of one wave, %6.3f cycles of the CU per scalar instruction, %6.3f of a SIMD by its own time  resident %d per SIMD on %d CUs  clock %.3f GHz  loop %.1f ms\n",
           waves, cyc / ((double)N * 32), cyc / ((double)N * 32 * waves), ticks * 10.0 * ghz / ((double)N * 32), resident, cus_seen, ghz, cyc / ghz * 1e-6);
    return 0;
}

int main() {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    printf("device %s, %d CUs; cycles are s_memtime ticks (shader clock); rows: workgroups per CU x threads, LDS bytes per workgroup\n", prop.gcnArchName, cus);
    Stamp *d;
    float *sink;
    CHECK(hipMalloc(&d, (size_t)cus * 4 * 16 * sizeof(Stamp)));
    CHECK(hipMalloc(&sink, (size_t)cus * 4 * 1024 * sizeof(float)));
    double v[R_COUNT], w[R_COUNT], x;
#define HEADLINE(row) run_mixed<row, 512, kPadTwoPerCu, 2>(d, sink, cus, &v[row])
#define FOURS(row) run_mixed<row, 256, kPadFourPerCu, 4>(d, sink, cus, &w[row])
    // the headline kernel's shape: 512-thread workgroups, two per CU
    if (HEADLINE(R_BASE) || HEADLINE(R_LOGIC_10) || HEADLINE(R_LOGIC_20) || HEADLINE(R_LOGIC_32) || HEADLINE(R_EXEC_10) || HEADLINE(R_EXEC_20) ||
        HEADLINE(R_EXEC_32) || HEADLINE(R_LOGIC_20_RUNS) || HEADLINE(R_LOGIC_20_BLOCK) || HEADLINE(R_BASE))
        return 1;
    // issue.hip's shape: 256-thread workgroups, four per CU -- held there by LDS, and as issue.hip launches them (nothing holds them)
    if (FOURS(R_BASE) || FOURS(R_LOGIC_10) || FOURS(R_LOGIC_20) || FOURS(R_LOGIC_32) || FOURS(R_LOGIC_20_RUNS) || FOURS(R_LOGIC_20_BLOCK) ||
        run_mixed<R_BASE, 256, kNoPad, 4>(d, sink, cus, &x))
        return 1;
    // SIMD-cycles per scalar instruction: (cycles per vector instruction, row b - row a) x 32 / (scalar count b - a)
    for (int shape = 0; shape < 2; ++shape) {
        const double *t = shape ? w : v;
        const auto price = [&](int a, int b) { return (t[b] - t[a]) * 32.0 / (kRowScalar[b] - kRowScalar[a]); };
        printf("%s: SIMD-cycles per scalar instruction, mask logic spread: 0 -> 0.31: %.3f, 0.31 -> 0.62: %.3f, 0.62 -> 1.0: %.3f, 0 -> 0.62: %.3f; "
               "0 -> 0.62 in runs of 5: %.3f, in one block: %.3f\n", shape ? "4x256" : "2x512",
               price(R_BASE, R_LOGIC_10), price(R_LOGIC_10, R_LOGIC_20), price(R_LOGIC_20, R_LOGIC_32), price(R_BASE, R_LOGIC_20),
               price(R_BASE, R_LOGIC_20_RUNS), price(R_BASE, R_LOGIC_20_BLOCK));
        if (!shape)
            printf("2x512: SIMD-cycles per scalar instruction, exec save/restore: 0 -> 0.31: %.3f, 0.31 -> 0.62: %.3f, 0.62 -> 1.0: %.3f, 0 -> 0.62: %.3f\n",
                   price(R_BASE, R_EXEC_10), price(R_EXEC_10, R_EXEC_20), price(R_EXEC_20, R_EXEC_32), price(R_BASE, R_EXEC_20));
    }
    if (run_scalar(d, sink, cus, 1) || run_scalar(d, sink, cus, 4) || run_scalar(d, sink, cus, 16)) return 1;
    return 0;
}
