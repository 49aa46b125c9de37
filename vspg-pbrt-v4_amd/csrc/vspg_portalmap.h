// vspg_portalmap.h -- the arithmetic of PortalImageInfiniteLight (src/pbrt/lights.h:699-808, lights.cpp:1287-1345) and of its
// WindowedPiecewiseConstant2D over a SummedAreaTable (util/sampling.h:829-983), on one DPortalLight record.  Host and device: the
// kernels reach it through vspg_portallight.h, the host builder (vspg_scene_build.hip) takes RenderFromImage from here, and the
// stand-alone check (tests/portallight_build_check.cpp) runs the sampling on the CPU against tests/portallight_model.py bit for bit.
// Every operation is one IEEE float operation in the reference's order; tan and atan2 are the project's own (vspg_trig.h).
//
// What this text DEFINES where the reference's is undefined or unbounded:
//   * float -> int of a table coordinate (SummedAreaTable::Lookup, Eval, ImageLookup) goes through portal_idx: a NaN or negative
//     coordinate gives 0, one past the table gives the table's size.  For coordinates in [0, size] -- all a finite query produces --
//     that is the reference's (int)x; a NaN direction or variate therefore reads inside the tables.  (The reference converts NaN to
//     int, which is undefined.)
//   * ImageFromRender refuses unless w.z > 0, so a NaN direction is "outside" (the reference's `w.z <= 0` lets NaN through).
//   * SampleBisection's loop is capped at kPortalBisectCap iterations.  The reference's loop has no bound: with a resolution that is no
//     power of two, n * max and n * min are rounded products and two adjacent floats can straddle a texel edge for ever.  The bound:
//     the window starts no wider than 1 and each iteration halves it; it goes on only while the window contains a texel edge k / n
//     with k >= 1, which is >= 2^-12 (n <= 4096), where floats are spaced >= 2^-36 apart: after 36 halvings the two ends are equal
//     or adjacent and no iteration changes them any more.  40 leaves room for the roundings of (min + max) / 2.  A run that reaches
//     the cap goes on to the interpolation with the bracket it has; tests/test_portallight_model.py proves no fixture reaches it.
//   * a non-finite interpolation parameter t = (u - P(min)) / (P(max) - P(min)) gives "no sample" (the reference clamps a NaN).
//
// The bisection is the hot loop: per iteration the reference's Px / Py evaluates Integral() = four bilinear lookups = sixteen table
// loads.  Across the iterations only one coordinate of one corner moves.  A lookup is a pure function of its two PortalAxis
// records (index pair and weights of one coordinate), so the two lookups on the fixed side and the axis record of the fixed
// coordinate are formed once per bisection: eight loads per iteration, and the same bits (the mirror evaluates every lookup in full).
#pragma once
#include "vspg_device.h"
#include "vspg_envmap.h"  // the __host__ twins of the vector helpers
#include "vspg_trig.h"

VSPG_NS_BEGIN

constexpr int kPortalBisectCap = 40;
enum { PORTAL_OK = 0, PORTAL_NO_BOUNDS = 1, PORTAL_ZERO_WINDOW = 2, PORTAL_ZERO_COLUMN = 3, PORTAL_BAD_T = 4, PORTAL_ZERO_JACOBIAN = 5 };

VHD V3 portal_to_local(const DPortalLight &P, V3 v) { return V3{dot(v, ld3(P.fx)), dot(v, ld3(P.fy)), dot(v, ld3(P.fz))}; }  // Frame::ToLocal
VHD V3 portal_from_local(const DPortalLight &P, V3 v) { return v.x * ld3(P.fx) + v.y * ld3(P.fy) + v.z * ld3(P.fz); }       // Frame::FromLocal
// the Jacobian d(u, v) / d(omega) of both directions of the map (lights.h:762, :779)
VHD float portal_duv_dw(V3 w) { return (kPi * kPi) * (1 - sqr(w.x)) * (1 - sqr(w.y)) / w.z; }

// ImageFromRender (lights.h:754-768)
VHD bool portal_image_from_render(const DPortalLight &P, V3 wRender, float *pu, float *pv, float *duv_dw = nullptr) {
    const V3 w = portal_to_local(P, wRender);
    if (!(w.z > 0)) return false;
    if (duv_dw) *duv_dw = portal_duv_dw(w);
    const float alpha = vspg_libm::portal_atan2f(w.x, w.z), beta = vspg_libm::portal_atan2f(w.y, w.z);
    *pu = clampf((alpha + kPiOver2) / kPi, 0.f, 1.f);
    *pv = clampf((beta + kPiOver2) / kPi, 0.f, 1.f);
    return true;
}
// RenderFromImage (lights.h:771-782)
VHD V3 portal_render_from_image(const DPortalLight &P, float u, float v, float *duv_dw = nullptr) {
    const float alpha = -kPiOver2 + u * kPi, beta = -kPiOver2 + v * kPi;
    const float x = vspg_libm::portal_tanf(alpha), y = vspg_libm::portal_tanf(beta);
    const V3 w = normalize(V3{x, y, 1.f});
    if (duv_dw) *duv_dw = portal_duv_dw(w);
    return portal_from_local(P, w);
}
// ImageBounds (lights.h:785-791): b = {pMin.x, pMin.y, pMax.x, pMax.y}
VHD bool portal_image_bounds(const DPortalLight &P, V3 p, float *b) {
    float u0, v0, u1, v1;
    const bool ok0 = portal_image_from_render(P, normalize(ld3(P.p0) - p), &u0, &v0);
    const bool ok1 = portal_image_from_render(P, normalize(ld3(P.p2) - p), &u1, &v1);
    if (!ok0 || !ok1) return false;
    b[0] = fmin_(u0, u1);
    b[1] = fmin_(v0, v1);
    b[2] = fmax_(u0, u1);
    b[3] = fmax_(v0, v1);
    return true;
}

VHD int portal_idx(float x, int n) { return x >= 0 ? (x < (float)n ? (int)x : n) : 0; }
// One coordinate of a SummedAreaTable::Lookup (util/sampling.h:864-876): the table indices LookupInt reads for x0 and x0 + 1
// (i0 < 0: the zero of the lower boundary) and the two bilinear weights
struct PortalAxis {
    int i0, i1;
    float d, omd;
};
VHD PortalAxis portal_axis(float c, int res) {
    const float s = c * (float)res;
    const int i = portal_idx(s, res);
    PortalAxis a;
    a.i0 = i == 0 ? -1 : (i - 1 < res - 1 ? i - 1 : res - 1);
    a.i1 = i < res - 1 ? i : res - 1;
    a.d = s - (float)i;
    a.omd = 1 - a.d;
    return a;
}
VHD float portal_lookup(const DPortalLight &P, const PortalAxis &ax, const PortalAxis &ay) {
    const size_t res = (size_t)P.res;
    const float *r0 = P.sat + (size_t)(ay.i0 < 0 ? 0 : ay.i0) * res, *r1 = P.sat + (size_t)ay.i1 * res;
    const float v00 = ax.i0 < 0 || ay.i0 < 0 ? 0.f : r0[ax.i0], v10 = ay.i0 < 0 ? 0.f : r0[ax.i1];
    const float v01 = ax.i0 < 0 ? 0.f : r1[ax.i0], v11 = r1[ax.i1];
    return ax.omd * ay.omd * v00 + ax.omd * ay.d * v01 + ax.d * ay.omd * v10 + ax.d * ay.d * v11;
}
// SummedAreaTable::Integral (util/sampling.h:851-857) of four lookups: (maxx, maxy), (minx, maxy), (minx, miny), (maxx, miny)
VHD float portal_integral4(const DPortalLight &P, float l11, float l01, float l00, float l10) {
    const double s = ((double)l11 - (double)l01) + ((double)l00 - (double)l10);
    const float q = (float)(s / (double)(P.res * P.res));
    return q < 0.f ? 0.f : q;  // std::max<Float>(q, 0)
}
VHD float portal_integral(const DPortalLight &P, const float *b) {
    const PortalAxis x0 = portal_axis(b[0], P.res), y0 = portal_axis(b[1], P.res), x1 = portal_axis(b[2], P.res), y1 = portal_axis(b[3], P.res);
    return portal_integral4(P, portal_lookup(P, x1, y1), portal_lookup(P, x0, y1), portal_lookup(P, x0, y0), portal_lookup(P, x1, y0));
}
// WindowedPiecewiseConstant2D::Eval (util/sampling.h:974-978)
VHD float portal_eval(const DPortalLight &P, float u, float v) {
    const int res = P.res;
    int iu = portal_idx(u * (float)res, res), iv = portal_idx(v * (float)res, res);
    iu = iu < res - 1 ? iu : res - 1;
    iv = iv < res - 1 ? iv : res - 1;
    return P.func[(size_t)iv * (size_t)res + (size_t)iu];
}
// WindowedPiecewiseConstant2D::PDF (util/sampling.h:945-950)
VHD float portal_map_pdf(const DPortalLight &P, float u, float v, const float *b) {
    const float funcInt = portal_integral(P, b);
    if (funcInt == 0) return 0.f;
    return portal_eval(P, u, v) / funcInt;
}

// SampleBisection (util/sampling.h:955-971) of the CDF  c -> Integral(window with one pMax coordinate set to c) / norm.  ALONG_X: the
// moving coordinate is pMax.x and (f0, f1) are the axis records of pMin.y and pMax.y; else it is pMax.y and they are those of pMin.x
// and pMax.x.  lo_axis: the axis record of the window's fixed LOWER end of the moving coordinate.
template <bool ALONG_X>
VHD float portal_bisect(const DPortalLight &P, const PortalAxis &lo_axis, const PortalAxis &f0, const PortalAxis &f1, float norm, float u,
                        float lo, float hi, int *trips, bool *bad_t) {
    const int n = P.res;
    // the two lookups at the fixed lower end: Integral's (minx, maxy) and (minx, miny) along x, its (minx, miny) and (maxx, miny) along y
    const float fixA = ALONG_X ? portal_lookup(P, lo_axis, f1) : portal_lookup(P, f0, lo_axis);
    const float fixB = ALONG_X ? portal_lookup(P, lo_axis, f0) : portal_lookup(P, f1, lo_axis);
    auto cdf = [&](float c) -> float {
        const PortalAxis m = portal_axis(c, n);
        float integral;
        if (ALONG_X) integral = portal_integral4(P, portal_lookup(P, m, f1), fixA, fixB, portal_lookup(P, m, f0));
        else integral = portal_integral4(P, portal_lookup(P, f1, m), portal_lookup(P, f0, m), fixA, fixB);
        return integral / norm;
    };
    int it = 0;
    while (__builtin_ceilf((float)n * hi) - __builtin_floorf((float)n * lo) > 1 && it < kPortalBisectCap) {
        const float mid = (lo + hi) / 2;
        if (cdf(mid) > u) hi = mid;
        else lo = mid;
        ++it;
    }
    *trips = it;
    const float plo = cdf(lo), phi = cdf(hi);
    const float t = (u - plo) / (phi - plo);
    *bad_t = !(__builtin_fabsf(t) <= kFltMax);
    return clampf((1 - t) * lo + t * hi, lo, hi);
}

// PortalImageInfiniteLight::ImageLookup (lights.cpp:1296-1303) without the scale: Image::LookupNearestChannel under WrapMode::Clamp,
// ClampZero
VHD void portal_image_lookup(const DPortalLight &P, float u, float v, float *rgb) {
    const int res = P.res;
    int iu = portal_idx(u * (float)res, res), iv = portal_idx(v * (float)res, res);
    iu = iu < res - 1 ? iu : res - 1;
    iv = iv < res - 1 ? iv : res - 1;
    const float *t = P.image + 3 * ((size_t)iv * (size_t)res + (size_t)iu);
    for (int c = 0; c < 3; ++c) rgb[c] = t[c] > 0.f ? t[c] : 0.f;
}

// What SampleLi forms on its way (lights.cpp:1305-1329); the probe (vspg_portallight_batch) reports all of it
struct PortalSample {
    float u, v, mapPDF, duv_dw, pdf;
    V3 wi;
    float rgb[3];  // ClampZero(texel), without the light's scale
    int trips_x, trips_y, why;
};
// WindowedPiecewiseConstant2D::Sample (util/sampling.h:903-942) inside PortalImageInfiniteLight::SampleLi
VHD bool portal_sample(const DPortalLight &P, V3 ctxp, float u0, float u1, PortalSample *o) {
    const int res = P.res;
    o->trips_x = o->trips_y = 0;
    float b[4];
    if (!portal_image_bounds(P, ctxp, b)) { o->why = PORTAL_NO_BOUNDS; return false; }
    const PortalAxis bx0 = portal_axis(b[0], res), by0 = portal_axis(b[1], res), bx1 = portal_axis(b[2], res), by1 = portal_axis(b[3], res);
    const float bInt = portal_integral4(P, portal_lookup(P, bx1, by1), portal_lookup(P, bx0, by1), portal_lookup(P, bx0, by0), portal_lookup(P, bx1, by0));
    if (bInt == 0) { o->why = PORTAL_ZERO_WINDOW; return false; }
    bool bad_x, bad_y;
    const float px = portal_bisect<true>(P, bx0, by0, by1, bInt, u0, b[0], b[2], &o->trips_x, &bad_x);
    o->u = px;
    if (bad_x) { o->why = PORTAL_BAD_T; return false; }
    // bCond (util/sampling.h:922-926)
    const float nx = (float)res;
    const float cx0 = __builtin_floorf(px * nx) / nx;
    float cx1 = __builtin_ceilf(px * nx) / nx;
    if (cx0 == cx1) cx1 += 1.f / nx;
    const PortalAxis ax0 = portal_axis(cx0, res), ax1 = portal_axis(cx1, res);
    const float condInt = portal_integral4(P, portal_lookup(P, ax1, by1), portal_lookup(P, ax0, by1), portal_lookup(P, ax0, by0), portal_lookup(P, ax1, by0));
    if (condInt == 0) { o->why = PORTAL_ZERO_COLUMN; return false; }
    const float py = portal_bisect<false>(P, by0, ax0, ax1, condInt, u1, b[1], b[3], &o->trips_y, &bad_y);
    o->v = py;
    if (bad_y) { o->why = PORTAL_BAD_T; return false; }
    o->mapPDF = portal_eval(P, px, py) / bInt;
    o->wi = portal_render_from_image(P, px, py, &o->duv_dw);
    if (o->duv_dw == 0) { o->why = PORTAL_ZERO_JACOBIAN; return false; }
    o->pdf = o->mapPDF / o->duv_dw;
    portal_image_lookup(P, px, py, o->rgb);
    o->why = PORTAL_OK;
    return true;
}
// PortalImageInfiniteLight::PDF_Li (lights.cpp:1331-1345)
VHD float portal_pdf(const DPortalLight &P, V3 ctxp, V3 w) {
    float u, v, duv_dw, b[4];
    if (!portal_image_from_render(P, w, &u, &v, &duv_dw) || duv_dw == 0) return 0.f;
    if (!portal_image_bounds(P, ctxp, b)) return 0.f;
    return portal_map_pdf(P, u, v, b) / duv_dw;
}
// PortalImageInfiniteLight::Le (lights.cpp:1287-1294) without the scale; false: zero radiance.  uv (optional): the direction's image
// point where it has one, for the probe
VHD bool portal_radiance(const DPortalLight &P, V3 ro, V3 rd, float *rgb, float *uv = nullptr) {
    float u, v, b[4];
    const bool has_uv = portal_image_from_render(P, normalize(rd), &u, &v);
    if (uv && has_uv) { uv[0] = u; uv[1] = v; }
    const bool has_b = portal_image_bounds(P, ro, b);
    if (!has_uv || !has_b || !(u >= b[0] && u <= b[2] && v >= b[1] && v <= b[3])) return false;
    portal_image_lookup(P, u, v, rgb);
    return true;
}

VSPG_NS_END
