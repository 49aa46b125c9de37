// vspg_film_error.h -- film error against a reference image, reduced on the device (include/vspg.h: VspgFilmError).
//
// What ImageTileIntegrator::Render computes after every wave under --mse-reference-image (src/pbrt/cpu/integrators.cpp:243-262):
// Image::MSE (src/pbrt/util/image.cpp:575-607) and Image::MRSE (:609-639) of the film against the reference image, here as the six
// sums before the division, over a pixel window.
//
// Two launches, no atomics, no dependence on the grid or on which block runs where:
//   k_film_error_rows    one workgroup per row of the window.  Lane t of the 256 adds the row's pixels x0 + t, x0 + t + 256, ...
//                        in that order into six double accumulators; the 64 lanes of a wavefront are folded by the fixed
//                        shuffle tree (offsets 32, 16, .. 1), the four wavefronts' results are added in wavefront order.  Six doubles
//                        per row go to `partials`.
//   k_film_error_finish  one workgroup.  Lane t adds the rows t, t + 256, ... in that order, the same fold follows, lane 0 writes the
//                        record and stamps it with the device's constant-rate clock.
// So the association order of every sum is a function of (x1 - x0, y1 - y0) alone: the same film and window give the same bits.
//
// Traffic: the film is float4 {sum w*r, sum w*g, sum w*b, sum w}, the reference image is kept as a padded float4 too, so a pixel is
// two 16-byte loads: 32 bytes per pixel (66.4 MB for a 1920 x 1080 window), plus 48 bytes per row written and read once.
// The kernels read the film, the reference image and `partials`; they write `partials` and one log record.
#ifndef VSPG_FILM_ERROR_H
#define VSPG_FILM_ERROR_H
#include <hip/hip_runtime.h>

#include "../../include/vspg.h"
#include "vspg_device.h"

constexpr int kFilmErrorBlock = 256;

// the fold of one value over the workgroup; the result is valid in thread 0.  `lds` holds kFilmErrorBlock / 64 doubles.
__device__ __forceinline__ double film_error_fold(double v, double *lds) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    const int wave = threadIdx.x >> 6;
    __syncthreads();  // (the previous fold's reads of lds are done)
    if ((threadIdx.x & 63) == 0) lds[wave] = v;
    __syncthreads();
    double s = lds[0];
#pragma unroll
    for (int w = 1; w < kFilmErrorBlock / 64; ++w) s += lds[w];
    return s;
}

__global__ void __launch_bounds__(kFilmErrorBlock) k_film_error_rows(int xres, vspg::PixelWindow win, const float4 *__restrict__ film,
                                                                      const float4 *__restrict__ ref, double *__restrict__ partials) {
    __shared__ double lds[kFilmErrorBlock / 64];
    const int row = blockIdx.x;
    const size_t base = (size_t)(win.y0 + row) * (size_t)xres;
    double acc[6] = {0., 0., 0., 0., 0., 0.};
#pragma unroll 4
    for (int x = win.x0 + (int)threadIdx.x; x < win.x1; x += kFilmErrorBlock) {
        const float4 f = film[base + x];
        const float4 q = ref[base + x];
        const float rgb[3] = {f.x, f.y, f.z}, rc[3] = {q.x, q.y, q.z};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = f.w != 0.f ? rgb[c] / f.w : rgb[c];  // RGBFilm::GetPixelRGB (film.h:269-287): one float division
            const double d = (double)v - (double)rc[c];
            const double se = d * d;                              // image.cpp:594
            const double den = (double)rc[c] + 0.01;
            const double rse = se / (den * den);                  // image.cpp:626
            if (!__builtin_isinf(se)) acc[c] += se;               // :595-597 (a NaN is added)
            if (!__builtin_isinf(rse)) acc[3 + c] += rse;         // :627-629
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double s = film_error_fold(acc[k], lds);
        if (threadIdx.x == 0) partials[(size_t)row * 6 + k] = s;
    }
}

__global__ void __launch_bounds__(kFilmErrorBlock) k_film_error_finish(vspg::PixelWindow win, int tag, const double *__restrict__ partials,
                                                                        VspgFilmError *__restrict__ rec) {
    __shared__ double lds[kFilmErrorBlock / 64];
    const int rows = win.y1 - win.y0;
    double acc[6] = {0., 0., 0., 0., 0., 0.};
    for (int row = (int)threadIdx.x; row < rows; row += kFilmErrorBlock) {
#pragma unroll
        for (int k = 0; k < 6; ++k) acc[k] += partials[(size_t)row * 6 + k];
    }
    double sum[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) sum[k] = film_error_fold(acc[k], lds);
    if (threadIdx.x == 0) {
        rec->x0 = win.x0; rec->y0 = win.y0; rec->x1 = win.x1; rec->y1 = win.y1;
        rec->tag = tag;
        rec->tick_khz = 0;  // (filled in by vspg_film_error_read)
        rec->n_pixels = (uint64_t)(win.x1 - win.x0) * (uint64_t)rows;
#pragma unroll
        for (int c = 0; c < 3; ++c) { rec->sum_se[c] = sum[c]; rec->sum_rse[c] = sum[3 + c]; }
        rec->device_ticks = wall_clock64();
    }
}
#endif  // VSPG_FILM_ERROR_H
