// rgb_octet_fill.hip -- k_rgb_octet_build (csrc/vspg_rgb_update_kernels.h: the brick's voxels staged in LDS, stores in memory order)
// against the per-lane fill it was chosen over (lane = octet, as k_brick_fill: eight 16-byte stores per lane, 128 bytes apart across
// lanes) and against hipMemsetAsync over the same image in the same process: the write-only streaming rate of that machine on that day.
// The per-lane variant lives here only, for the comparison.  Both images are compared on the device before anything is timed.
//
//   hipcc $(make -s -C vspg-pbrt-v4_amd/csrc print-HIPFLAGS) -I vspg-pbrt-v4_amd/csrc -o rgb_octet_fill scripts/microbench/rgb_octet_fill.hip
//   ./rgb_octet_fill N [reps]      -> one JSON line (scripts/rgbgrid_update_timing.py runs it)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vspg_rgbgrid.h"
using namespace vspg;
namespace {
constexpr int kBlock = 256;     // vspg_capi.hip's
constexpr int kMajBlock = 256;  // vspg_probe_kernels.h's
}  // namespace
#include "vspg_rgb_update_kernels.h"

namespace {
__device__ __forceinline__ float4 rgb_raw_at(const float *d, int nx, int ny, int nz, int x, int y, int z) {
    if (x < 0 || y < 0 || z < 0 || x >= nx || y >= ny || z >= nz) return make_float4(0.f, 0.f, 0.f, 0.f);
    const float *v = d + (((size_t)z * ny + y) * nx + x) * 3u;
    return make_float4(v[0], v[1], v[2], 0.f);
}
__global__ __launch_bounds__(512) void k_rgb_octet_build_lane(const float *__restrict__ rgb, int nx, int ny, int nz, int bnx, int bny,
                                                              float4 *__restrict__ oct) {
    const int b = blockIdx.x;
    const int bx = b % bnx, by = (b / bnx) % bny, bz = b / (bnx * bny);
    const int l = threadIdx.x, ox = 8 * bx + (l & 7), oy = 8 * by + ((l >> 3) & 7), oz = 8 * bz + (l >> 6);
    const bool used = ox <= nx && oy <= ny && oz <= nz;
    float4 *q = oct + ((size_t)b * 512u + (size_t)l) * 8u;
#pragma unroll
    for (int c = 0; c < 8; ++c)
        q[c] = used ? rgb_raw_at(rgb, nx, ny, nz, ox - 1 + (c & 1), oy - 1 + ((c >> 1) & 1), oz - 1 + (c >> 2)) : make_float4(0.f, 0.f, 0.f, 0.f);
}
__global__ __launch_bounds__(kBlock) void k_count_differences(const uint4 *__restrict__ a, const uint4 *__restrict__ b, size_t n, unsigned long long *out) {
    unsigned long long bad = 0;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
        const uint4 x = a[i], y = b[i];
        bad += (x.x != y.x) + (x.y != y.y) + (x.z != y.z) + (x.w != y.w);
    }
    if (bad) atomicAdd(out, bad);
}
}  // namespace

#define CK(expr)                                                                                  \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            std::fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e_));                       \
            return 1;                                                                             \
        }                                                                                         \
    } while (0)

int main(int argc, char **argv) {
    const int n = argc > 1 ? std::atoi(argv[1]) : 64, reps = argc > 2 ? std::atoi(argv[2]) : 9;
    if (n < 1 || n > 512 || reps < 1) return 2;
    const int bn = (n + 8) / 8;
    const size_t nb = (size_t)bn * bn * bn, nq = nb * 4096u, n3 = (size_t)n * n * n * 3;
    std::vector<float> host(n3);
    unsigned s = 12345u;
    for (float &v : host) { s = s * 1664525u + 1013904223u; v = (float)(s >> 8) * (1.f / 16777216.f); }
    float *rgb = nullptr;
    float4 *img[2] = {nullptr, nullptr};
    unsigned long long *dbad = nullptr, bad = 0;
    CK(hipMalloc(&rgb, n3 * sizeof(float)));
    CK(hipMalloc(&img[0], nq * sizeof(float4)));
    CK(hipMalloc(&img[1], nq * sizeof(float4)));
    CK(hipMalloc(&dbad, sizeof bad));
    CK(hipMemcpy(rgb, host.data(), n3 * sizeof(float), hipMemcpyHostToDevice));
    CK(hipMemset(dbad, 0, sizeof bad));
    CK(hipMemset(img[0], 0xff, nq * sizeof(float4)));   // (both kernels write every byte: no memset stands behind the images)
    CK(hipMemset(img[1], 0x7f, nq * sizeof(float4)));
    hipLaunchKernelGGL(k_rgb_octet_build, dim3((unsigned)nb), dim3(512), 0, 0, rgb, n, n, n, bn, bn, img[0]);
    hipLaunchKernelGGL(k_rgb_octet_build_lane, dim3((unsigned)nb), dim3(512), 0, 0, rgb, n, n, n, bn, bn, img[1]);
    hipLaunchKernelGGL(k_count_differences, dim3(4096), dim3(kBlock), 0, 0, (const uint4 *)img[0], (const uint4 *)img[1], nq, dbad);
    CK(hipGetLastError());
    CK(hipMemcpy(&bad, dbad, sizeof bad, hipMemcpyDeviceToHost));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    double med[3];
    for (int which = 0; which < 3; ++which) {
        std::vector<float> ms;
        for (int r = 0; r <= reps; ++r) {  // (repetition 0 warms up)
            CK(hipEventRecord(e0, 0));
            if (which == 0) hipLaunchKernelGGL(k_rgb_octet_build, dim3((unsigned)nb), dim3(512), 0, 0, rgb, n, n, n, bn, bn, img[0]);
            else if (which == 1) hipLaunchKernelGGL(k_rgb_octet_build_lane, dim3((unsigned)nb), dim3(512), 0, 0, rgb, n, n, n, bn, bn, img[1]);
            else CK(hipMemsetAsync(img[1], 0, nq * sizeof(float4), 0));
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            float t = 0.f;
            CK(hipEventElapsedTime(&t, e0, e1));
            if (r) ms.push_back(t);
        }
        std::sort(ms.begin(), ms.end());
        med[which] = ms[ms.size() / 2];
    }
    const double gb = (double)nq * sizeof(float4) / 1e9;
    std::printf("{\"n\": %d, \"image_bytes\": %zu, \"reps\": %d, \"differences\": %llu, \"staged_ms\": %.4f, \"per_lane_ms\": %.4f, \"memset_ms\": %.4f, "
                "\"staged_GBps\": %.1f, \"per_lane_GBps\": %.1f, \"memset_GBps\": %.1f}\n",
                n, nq * sizeof(float4), reps, bad, med[0], med[1], med[2], gb / (med[0] * 1e-3), gb / (med[1] * 1e-3), gb / (med[2] * 1e-3));
    (void)hipFree(rgb); (void)hipFree(img[0]); (void)hipFree(img[1]); (void)hipFree(dbad);
    return bad ? 1 : 0;
}
