// vspg_envlight.h -- ImageInfiniteLight for the RGB build (src/pbrt/lights.h:607-697, lights.cpp:1072-1142): an importance-sampled
// equal-area octahedral environment map.  Three entry points, used by sample_light and li_surface_pre (vspg_path.h) and pinned
// through vspg_envlight_batch against tests/envlight_model.py:
//   env_Le         ImageInfiniteLight::Le        (lights.h:643-647)
//   env_sample_li  ImageInfiniteLight::SampleLi  (lights.h:650-674), allowIncompletePDF = true
//   env_pdf_li     ImageInfiniteLight::PDF_Li    (lights.cpp:1113-1123), allowIncompletePDF = true
// The tables (DEnvLight, vspg_device.h) are built on the host by vspg_renderer_set_environment_image; only the compensated
// distribution exists (every call site of the integrator passes allowIncompletePDF = true).
//
// Loads: in li_surface_pre the light index is the loop counter -- wave-uniform, the record's fields are scalar loads; what is indexed
// by the direction (texels, func) or by the search (cdf) differs per lane and is a vector load.  In sample_light the light itself is
// the lane's pick.  The two searches are FindInterval's own loop (util/math.h:508-519): its body is two selects, no branch, and its
// trip count is ceil(log2(res + 1)) or one less depending on the lane's path through it, so the lanes of a wave leave it within one
// iteration of each other; each step is one dependent 4-byte load.
#pragma once
#include "vspg_device.h"
// env_xform, env_sphere_to_square and env_remap_octahedral live in vspg_envmap.h (shared with the host builders; vspg_path.h includes it)

// EqualAreaSquareToSphere (util/math.cpp:292-314)
VDEV V3 env_square_to_sphere(float px, float py) {
    const float u = 2 * px - 1, v = 2 * py - 1;
    const float up = __builtin_fabsf(u), vp = __builtin_fabsf(v);
    const float signedDistance = 1 - (up + vp);
    const float d = __builtin_fabsf(signedDistance);
    const float r = 1 - d;
    const float phi = (r == 0 ? 1 : (vp - up) / r + 1) * kPi / 4;
    const float z = __builtin_copysignf(1 - sqr(r), signedDistance);
    float sinPhi, cosPhi;
    sincosf_(phi, &sinPhi, &cosPhi);
    cosPhi = __builtin_copysignf(cosPhi, u);
    sinPhi = __builtin_copysignf(sinPhi, v);
    return V3{cosPhi * r * safe_sqrt(2 - sqr(r)), sinPhi * r * safe_sqrt(2 - sqr(r)), z};
}

// ImageLe (lights.h:681-687): Image::LookupNearestChannel under WrapMode::OctahedralSphere (util/image.h:352-356, RemapPixelCoords
// :100-125), ClampZero, times the multiplier.  u == 1 gives index res: it mirrors across u = 1 and flips v.
VDEV Spec env_image_le(const DScene &S, int k, float u, float v) {
    const DEnvLight &E = S.env[k];
    const int res = E.res;
    int px = (int)(u * (float)res), py = (int)(v * (float)res);
    env_remap_octahedral(&px, &py, res);
    // (u, v) of a finite direction lie in [0, 1] and the remap lands inside the image; a NaN direction must not index outside it
    px = px < 0 ? 0 : (px > res - 1 ? res - 1 : px);
    py = py < 0 ? 0 : (py > res - 1 ? res - 1 : py);
    const float *t = E.texels + 3 * ((size_t)py * (size_t)res + (size_t)px);
    return clamp_zero(Spec{t[0], t[1], t[2]}) * lds(S.inf_L[k]);
}

VDEV Spec env_Le(const DScene &S, int k, V3 d, float *uv = nullptr) {
    const V3 wLight = normalize(env_xform(S.env[k].mi, d));
    float u, v;
    env_sphere_to_square(wLight, &u, &v);
    if (uv) { uv[0] = u; uv[1] = v; }
    return env_image_le(S, k, u, v);
}

// PiecewiseConstant2D::PDF over the unit square (util/sampling.h:773-779), / (4 Pi).  The direction is NOT normalised
// (lights.cpp:1115).
VDEV float env_pdf_li(const DScene &S, int k, V3 w) {
    const DEnvLight &E = S.env[k];
    const V3 wLight = env_xform(E.mi, w);
    float u, v;
    env_sphere_to_square(wLight, &u, &v);
    const int res = E.res;
    int iu = (int)(u * (float)res), iv = (int)(v * (float)res);
    iu = iu < 0 ? 0 : (iu > res - 1 ? res - 1 : iu);
    iv = iv < 0 ? 0 : (iv > res - 1 ? res - 1 : iv);
    const float pdf = E.func[(size_t)iv * (size_t)res + (size_t)iu] / E.integral;
    return pdf / (4 * kPi);
}

// FindInterval(sz, [&](int i) { return cdf[i] <= u; }) (util/math.h:508-519): indices 1 .. sz - 2 are read
VDEV int env_find_interval(const float *cdf, int sz, float u) {
    int size = sz - 2, first = 1;
    while (size > 0) {
        const int half = size >> 1, middle = first + half;
        const bool pred = cdf[middle] <= u;
        first = pred ? middle + 1 : first;
        size = pred ? size - (half + 1) : half;
    }
    const int o = first - 1;
    return o < 0 ? 0 : (o > sz - 2 ? sz - 2 : o);
}
// PiecewiseConstant1D::Sample over [0, 1] (util/sampling.h:657-675); Lerp(x, 0, 1) = (1 - x) * 0 + x * 1 is x for 0 <= x <= 1
VDEV float env_sample_1d(const float *func, const float *cdf, int n, float funcInt, float u, float *pdf, int *offset) {
    const int o = env_find_interval(cdf, n + 1, u);
    *offset = o;
    const float c0 = cdf[o], c1 = cdf[o + 1];
    float du = u - c0;
    if (c1 - c0 > 0) du /= c1 - c0;
    *pdf = funcInt > 0 ? func[o] / funcInt : 0.f;
    return ((float)o + du) / (float)n;
}

VDEV bool env_sample_li(const DScene &S, int k, V3 ctxp, float u0, float u1, LightLi *ls, float *uv = nullptr) {
    const DEnvLight &E = S.env[k];
    const int res = E.res;
    // PiecewiseConstant2D::Sample (util/sampling.h:760-770): the marginal with u[1], then that row with u[0]
    float pdf0, pdf1;
    int iv, iu;
    const float d1 = env_sample_1d(E.mfunc, E.mcdf, res, E.integral, u1, &pdf1, &iv);
    const float d0 = env_sample_1d(E.func + (size_t)iv * (size_t)res, E.cdf + (size_t)iv * (size_t)(res + 1), res, E.mfunc[iv], u0, &pdf0, &iu);
    const float mapPDF = pdf0 * pdf1;
    if (uv) { uv[0] = d0; uv[1] = d1; }
    if (mapPDF == 0) return false;
    const V3 wLight = env_square_to_sphere(d0, d1);
    const V3 wi = env_xform(E.m, wLight);
    ls->L = env_image_le(S, k, d0, d1);
    ls->wi = wi;
    ls->pdf = mapPDF / (4 * kPi);
    ls->pLight = p3i_exact(ctxp + wi * (2 * S.scene_radius));
    ls->nLight = mk(0, 0, 0);
    return true;
}
