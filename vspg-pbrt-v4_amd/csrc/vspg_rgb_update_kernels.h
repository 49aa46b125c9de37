// vspg_rgb_update_kernels.h -- the device side of vspg_renderer_update_rgb_grids: an RGB grid medium's storage (vspg_rgbgrid.h) rebuilt
// from raw RGB voxels that lie ON THE DEVICE.  Three kernels: the value check of a device source (k_rgb_validate), the octet image of
// one sigma grid (k_rgb_octet_build) and the majorant grid (k_majorant_build_rgb).  Included by vspg_capi.hip next to
// vspg_probe_kernels.h, whose k_brick_fill / k_majorant_build do the same for the scalar grids.  Create keeps the host builders
// (build_rgb_octets, build_majorant_grid_rgb in vspg_scene_build.hip): they are the independent statement these kernels are held to,
// byte for byte (tests/test_rgbgrid_update_gpu.py).
#pragma once
#include "vspg_rgbgrid.h"

namespace {

// ---- the value check of a device source ------------------------------------------------------------------------------------------------
// One read pass over the n floats of a grid; *flag becomes non-zero when a value is negative or not finite (-0.0 passes, as it passes
// the host loop check_rgb_grid_values: -0.0 < 0 is false).  Runs, and is read back, before anything of the renderer is written.
__global__ __launch_bounds__(kBlock) void k_rgb_validate(const float *__restrict__ v, size_t n, int *__restrict__ flag) {
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
        const float x = v[i];
        bad = bad || !(x >= 0.f && x <= 3.402823466e+38f);  // NaN fails both comparisons
    }
    if (bad) atomicOr(flag, 1);
}

// ---- the octet image of one sigma grid -------------------------------------------------------------------------------------------------
// One 512-thread workgroup per brick, every brick stored (brick number = slot: rgb_octet_slot).  A brick holds the octets o = 8b .. 8b + 7
// per axis, i.e. base voxels 8b - 1 .. 8b + 6, whose corners are the 9^3 raw voxels 8b - 1 .. 8b + 7.  Those are staged in LDS first, rows
// of 9 voxels = 27 consecutive floats read by consecutive lanes, zero outside the grid (SampledGrid::Lookup(Point3i)'s bounds test).
// Then the brick's 4096 float4 (512 octets x 8 corners = 64 KB) are written in memory order: the i-th store of lane l is float4 number
// j = 512 i + l of the brick -- octet j >> 3, corner j & 7 -- so one store instruction of a wavefront covers 1 KB of consecutive memory.
// EVERY slot is written: .w = 0, zeros for corners outside the grid and for the octets behind o = n on an axis (a brick's unused slots),
// which makes the image equal build_rgb_octets' in every byte without a memset.
constexpr int kRgbStage = 9 * 9 * 27;  // floats: 8748 bytes of LDS
__global__ __launch_bounds__(512) void k_rgb_octet_build(const float *__restrict__ rgb, int nx, int ny, int nz, int bnx, int bny,
                                                         float4 *__restrict__ oct) {
    __shared__ float s_v[kRgbStage];
    const int b = blockIdx.x;
    const int bx = b % bnx, by = (b / bnx) % bny, bz = b / (bnx * bny);
    const int l = threadIdx.x;
    for (int i = l; i < kRgbStage; i += 512) {
        const int f = i % 27, row = i / 27;
        const int x = 8 * bx - 1 + f / 3, y = 8 * by - 1 + row % 9, z = 8 * bz - 1 + row / 9;
        float v = 0.f;
        if (x >= 0 && y >= 0 && z >= 0 && x < nx && y < ny && z < nz) v = rgb[(((size_t)z * ny + y) * nx + x) * 3u + (size_t)(f % 3)];
        s_v[i] = v;
    }
    __syncthreads();
    float4 *q = oct + (size_t)b * 4096u;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int j = 512 * i + l, o = j >> 3, c = j & 7;
        const int ox = o & 7, oy = (o >> 3) & 7, oz = o >> 6;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (8 * bx + ox <= nx && 8 * by + oy <= ny && 8 * bz + oz <= nz) {  // (a corner outside the grid is a staged zero)
            const float *s = s_v + ((oz + (c >> 2)) * 9 + oy + ((c >> 1) & 1)) * 27 + (ox + (c & 1)) * 3;
            v.x = s[0]; v.y = s[1]; v.z = s[2];
        }
        q[j] = v;
    }
}

// ---- the majorant grid -------------------------------------------------------------------------------------------------------------
// One 256-thread workgroup per majorant cell, the per-axis box tables from the host (majorant_axis_ranges), as k_majorant_build.  One
// launch covers both sigma grids: per grid convert = max(R, G, B) per voxel (RGBUnboundedSpectrum::MaxValue in the RGB build), the
// maximum over the box started from the low-corner voxel's value (0 outside the grid) as SampledGrid::MaxValue starts, an absent grid
// counting as 1; the cell gets sigma_scale * (ma + ms), one rounding per operation (build_majorant_grid_rgb).
// A grid's voxels come from `raw` (the grid being replaced: 3 floats per voxel) or, for a grid that stays, from its own octets: corner 0
// of octet (x + 1, y + 1, z + 1) is voxel (x, y, z) -- no raw copy of the sigma grids is kept on the device.  Both null: absent.
struct RgbMajSource {
    const float *raw;
    const float4 *oct;
};
__device__ __forceinline__ float rgb_max_at(const RgbMajSource &g, int nx, int ny, int nz, int bnx, int bny, int x, int y, int z) {
    if (x < 0 || y < 0 || z < 0 || x >= nx || y >= ny || z >= nz) return 0.f;
    float r, gg, bb;
    if (g.raw) {
        const float *v = g.raw + (((size_t)z * ny + y) * nx + x) * 3u;
        r = v[0]; gg = v[1]; bb = v[2];
    } else {
        const float4 q = g.oct[rgb_octet_slot(x + 1, y + 1, z + 1, bnx, bny) * 8u];
        r = q.x; gg = q.y; bb = q.z;
    }
    const float m = r < gg ? gg : r;  // std::max(std::max(v[0], v[1]), v[2])
    return m < bb ? bb : m;
}
__global__ __launch_bounds__(kMajBlock) void k_majorant_build_rgb(RgbMajSource ga, RgbMajSource gs, int nx, int ny, int nz, int bnx, int bny,
                                                                 int R, const int2 *__restrict__ ranges, float sigma_scale,
                                                                 float *__restrict__ maj) {
    const int c = blockIdx.x;
    const int2 rx = ranges[c % R], ry = ranges[R + (c / R) % R], rz = ranges[2 * R + c / (R * R)];
    const int bx = rx.y - rx.x + 1, by = ry.y - ry.x + 1, bz = rz.y - rz.x + 1;
    // (a box lies inside the grid, and a grid holds at most 2^31 voxels: unsigned arithmetic holds the count and the strided index)
    const unsigned n = (bx > 0 && by > 0 && bz > 0) ? (unsigned)bx * (unsigned)by * (unsigned)bz : 0u;
    __shared__ float s_max[2][kMajBlock / 64];
    float m[2];
    for (int k = 0; k < 2; ++k) {
        const RgbMajSource g = k ? gs : ga;
        float mx = 1.f;
        if (g.raw || g.oct) {  // (workgroup-uniform)
            mx = rgb_max_at(g, nx, ny, nz, bnx, bny, rx.x, ry.x, rz.x);
            for (unsigned i = threadIdx.x; i < n; i += kMajBlock) {
                const unsigned row = i / (unsigned)bx, zz = row / (unsigned)by;
                const int x = rx.x + (int)(i - row * (unsigned)bx), y = ry.x + (int)(row - zz * (unsigned)by), z = rz.x + (int)zz;
                const float v = rgb_max_at(g, nx, ny, nz, bnx, bny, x, y, z);
                mx = mx < v ? v : mx;
            }
            for (int o = 32; o > 0; o >>= 1) {
                const float v = __shfl_down(mx, o, 64);
                mx = mx < v ? v : mx;
            }
        }
        if ((threadIdx.x & 63) == 0) s_max[k][threadIdx.x >> 6] = mx;
        m[k] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 0; k < 2; ++k)
            for (int w = 1; w < kMajBlock / 64; ++w) m[k] = m[k] < s_max[k][w] ? s_max[k][w] : m[k];
        const float sum = m[0] + m[1];
        maj[c] = sigma_scale * sum;
    }
}

}  // namespace
