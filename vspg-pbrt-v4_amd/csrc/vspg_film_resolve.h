// vspg_film_resolve.h -- the film resolved to pixel values on the device (include/vspg.h: vspg_film_resolve).
//
// What RGBFilm::GetImage does before RGBFilm::WriteImage hands the image to the EXR writer (src/pbrt/film.cpp:531-569), over a pixel
// window: per pixel RGBFilm::GetPixelRGB (film.h:269-287: w != 0 ? rgbSum_c / w : rgbSum_c, one float division, no colour transform
// here as in the film-error kernels), then -- for half output -- the clamp of :544-556 and Half(float) of util/float.h:417-463.
//
// Two launches: k_film_pixels_zero clears the clamp counter (a launch, not a memset node, so the sequence can sit inside a captured
// graph), k_film_pixels<T, layout> writes the window's pixels to a staging buffer the host then copies out in one piece.
// One lane per pixel: a 16-byte load of the film's float4, three stores of T.  The clamp count is reduced per wavefront (ballot +
// popcount) and added by one lane of each.
//
// Traffic: 16 bytes read and 6 (half) or 12 (float) written per pixel -- 33.2 MB and 12.4 MB for a 1920 x 1080 half image, 10.4 us
// (4.39 TB/s) -- and the same 6 (12) bytes per pixel copied to the host afterwards, 223 us for those 12.4 MB: the copy is 21 times
// the kernel (profiles/film_resolve_timing.txt), so nothing is packed into wider stores.
// The kernels read the film; they write the staging buffer and the counter.
// (Not k_film_resolve of vspg_capi.hip: that one adds PARKED SAMPLES to the film; vspg_film_resolve runs it first when any are parked.)
#ifndef VSPG_FILM_RESOLVE_H
#define VSPG_FILM_RESOLVE_H
#include <hip/hip_runtime.h>

#include "../../include/vspg.h"
#include "vspg_device.h"

constexpr int kFilmResolveBlock = 256;

// Half(float) (util/float.h:417-463): round to nearest even, subnormal halves, >= 65520 to +-inf -- the conversion instruction's
// own behaviour -- and ANY NaN to 0x7e00 | sign, which it is not (the instruction keeps payload bits).
__device__ __forceinline__ unsigned short film_resolve_half_bits(float v) {
    if (v != v) return (unsigned short)(0x7e00u | ((__float_as_uint(v) >> 16) & 0x8000u));
    const _Float16 h = (_Float16)v;  // v_cvt_f16_f32, round to nearest even
    unsigned short bits;
    __builtin_memcpy(&bits, &h, sizeof(bits));
    return bits;
}

__global__ void k_film_pixels_zero(unsigned int *__restrict__ n_clamped) { *n_clamped = 0u; }

// T = float: the values unchanged.  T = unsigned short: the clamped values' half bits.
// layout VSPG_RESOLVE_RGB: out[(row * w + col) * 3 + {0,1,2}] = r, g, b.  VSPG_RESOLVE_SCANLINE_BGR: out[row * 3 * w + {0,1,2} * w + col] = b, g, r.
template <typename T, int kLayout>
__global__ void __launch_bounds__(kFilmResolveBlock) k_film_pixels(int xres, vspg::PixelWindow win, const float4 *__restrict__ film,
                                                                    T *__restrict__ out, unsigned int *__restrict__ n_clamped) {
    const int w = win.x1 - win.x0;
    const size_t n = (size_t)w * (size_t)(win.y1 - win.y0);
    const size_t i = (size_t)blockIdx.x * kFilmResolveBlock + threadIdx.x;
    const bool live = i < n;
    bool clamped = false;
    if (live) {
        const int row = (int)(i / (size_t)w), col = (int)(i - (size_t)row * (size_t)w);
        const float4 f = film[(size_t)(win.y0 + row) * (size_t)xres + (size_t)(win.x0 + col)];
        float r = f.w != 0.f ? f.x / f.w : f.x;  // RGBFilm::GetPixelRGB (film.h:269-287)
        float g = f.w != 0.f ? f.y / f.w : f.y;
        float b = f.w != 0.f ? f.z / f.w : f.z;
        T vr, vg, vb;
        if constexpr (sizeof(T) == 2) {
            float m = r;  // std::max({r, g, b}) with its NaN behaviour (film.cpp:547)
            if (m < g) m = g;
            if (m < b) m = b;
            if (m > 65504.f) {
                if (r > 65504.f) r = 65504.f;
                if (g > 65504.f) g = 65504.f;
                if (b > 65504.f) b = 65504.f;
                clamped = true;
            }
            vr = film_resolve_half_bits(r); vg = film_resolve_half_bits(g); vb = film_resolve_half_bits(b);
        } else {
            vr = r; vg = g; vb = b;
        }
        if constexpr (kLayout == VSPG_RESOLVE_RGB) {
            T *p = out + i * 3;
            p[0] = vr; p[1] = vg; p[2] = vb;
        } else {
            T *p = out + (size_t)row * 3 * (size_t)w + (size_t)col;
            p[0] = vb; p[(size_t)w] = vg; p[2 * (size_t)w] = vr;
        }
    }
    if constexpr (sizeof(T) == 2) {
        const unsigned long long mask = __ballot(clamped);  // (every lane of the wavefront is here: no early return above)
        if ((threadIdx.x & 63) == 0 && mask != 0ull) atomicAdd(n_clamped, (unsigned int)__popcll(mask));
    }
}

// the launch of one instantiation: a lane per pixel of the window
template <typename T>
inline void film_resolve_launch(int xres, const vspg::PixelWindow &win, int layout, const float4 *film, void *stage, unsigned int *n_clamped,
                                hipStream_t s) {
    const size_t n = (size_t)(win.x1 - win.x0) * (size_t)(win.y1 - win.y0);
    const dim3 grid((unsigned)((n + kFilmResolveBlock - 1) / kFilmResolveBlock)), block(kFilmResolveBlock);
    if (layout == VSPG_RESOLVE_RGB)
        hipLaunchKernelGGL((k_film_pixels<T, VSPG_RESOLVE_RGB>), grid, block, 0, s, xres, win, film, (T *)stage, n_clamped);
    else
        hipLaunchKernelGGL((k_film_pixels<T, VSPG_RESOLVE_SCANLINE_BGR>), grid, block, 0, s, xres, win, film, (T *)stage, n_clamped);
}
#endif  // VSPG_FILM_RESOLVE_H
