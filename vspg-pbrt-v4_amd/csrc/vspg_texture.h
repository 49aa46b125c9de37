// vspg_texture.h -- image textures on diffuse reflectance: SpectrumImageTexture ("imagemap") under UVMapping, evaluated as the reference
// does with every ray differential zero (`Option "bool disabletexturefiltering" true`), pinned through vspg_texture_eval_batch against
// tests/texture_model.py bit for bit.
// (reference: src/pbrt/textures.h:86-106 UVMapping::Map, textures.cpp:359-387 SpectrumImageTexture::Evaluate, util/mipmap.cpp:229-298
// MIPMap::Filter / Bilerp / Texel, util/image.h:93-146 RemapPixelCoords and :279-292 Image::BilerpChannel, interaction.cpp:43-47)
//
// With zero differentials MIPMap::Filter's `level = nLevels - 1 + Log2(1e-8)` is negative for any image that fits in memory: every
// filter reads level 0, "bilinear" / "trilinear" / "ewa" as Bilerp(0, st), "point" as Texel(0, round(st * res - 0.5)).
//
// The (u, v) of a hit.  A vertex travels as (primitive, three floats):
//   rectangle   the three floats are the re-projected point p;  d = p - p00,
//                 u = (d.x e1.x + d.y e1.y + d.z e1.z) * inv_l1      inv_l1 = 1 / |e1|^2 (DQuad)
//                 v = (d.x e2.x + d.y e2.y + d.z e2.z) * inv_l2      inv_l2 = 1 / |e2|^2
//               sums left to right, no contraction: the rectangle test's own (u, v), pbrt's default patch uv
//               (0,0) (1,0) (0,1) (1,1) of a bilinear patch p00, p10 = p00 + e1, p01 = p00 + e2, p11
//   triangle    the three floats are the barycentrics;  uv = b0 uv0 + b1 uv1 + b2 uv2 per component, summed left to right
//               (Triangle::InteractionFromIntersection, shapes.h `uvHit`), uv0..2 from DScene::tri_uv
//
// The lookup, in float with no contraction (the project's rule: -ffp-contract=off, a fused operation only where the reference calls FMA):
//   1  st = (su u + du, sv v + dv);  st[1] = 1 - st[1]
//   2  bilinear: x = st[0] xres - 0.5f, xi = floor(x), dx = x - xi, likewise y; texels (xi, yi) (xi+1, yi) (xi, yi+1) (xi+1, yi+1) through
//      the wrap; ((1-dx)(1-dy) v0 + dx(1-dy) v1 + (1-dx)dy v2 + dx dy v3) per channel, in that order
//   3  point: texel (round(x), round(y)), halves away from zero, through the wrap
//   4  rgb = scale * filtered          5  rgb = ClampZero(invert ? 1 - rgb : rgb)          6  R = Clamp(rgb, 0, 1)
//   7  has_lobes = some component of R is non-zero (DiffuseBxDF::Flags)
// x and y are held to [-1e9, 1e9] (NaN: 0) before they become integers: the parameters only have to be finite, and a float beyond the
// range of int has no defined conversion; no image has a texel there, and the mirror does the same.
// The wrap (RemapPixelCoords) per coordinate: repeat = pbrt's Mod, which is non-negative -- for the power-of-two resolutions the
// library accepts that is `p & (res - 1)` in two's complement, no integer division --; clamp; black = a texel with a coordinate outside
// the image counts as 0.
//
// Layout and cost.  One float4 per texel, row-major: a bilinear lookup is four independent 16-byte loads whose addresses are all
// computed before the first one is issued, and all four are issued before the first use; under the black wrap the load goes to the
// clamped address and the value is replaced by a select -- no branch around a load.  The loads are gathers (a lane's four texels are
// two pairs of neighbours, lanes of a wavefront are wherever their paths hit): they sit behind the dependent load of the texture's
// record, at a vertex that has just fetched its primitive anyway.
//
// Out of scope: filtered lookups (ray differentials, levels above 0, EWA), resolutions that are no power of two, 8-bit images and
// colour encodings, spheres, float textures, alpha, bump or displacement, textures on Le or on anything but diffuse reflectance,
// procedural textures.
#pragma once
#include "vspg_device.h"

VSPG_NS_BEGIN

struct TexUv { float u, v; };
VDEV TexUv tex_uv_quad(const DQuad &q, V3 p) {
    const V3 d = p - ld3(q.p00);
    return TexUv{dot(d, ld3(q.e1)) * q.inv_l1, dot(d, ld3(q.e2)) * q.inv_l2};
}
// uv6: the triangle's (uv0, uv1, uv2); b: the hit's barycentrics
VDEV TexUv tex_uv_tri(const float *uv6, V3 b) {  // (uv6 is 8-byte aligned: three float2)
    const float2 a0 = *reinterpret_cast<const float2 *>(uv6), a1 = *reinterpret_cast<const float2 *>(uv6 + 2), a2 = *reinterpret_cast<const float2 *>(uv6 + 4);
    return TexUv{b.x * a0.x + b.y * a1.x + b.z * a2.x, b.x * a0.y + b.y * a1.y + b.z * a2.y};
}
// one coordinate through RemapPixelCoords: the address to load from (always inside the image) and whether the texel counts
VDEV int tex_wrap(int p, int res, int wrap, bool *counts) {
    const bool inside = p >= 0 && p < res;
    *counts = inside || wrap != VSPG_TEXWRAP_BLACK;
    const int clamped = p < 0 ? 0 : (p > res - 1 ? res - 1 : p);
    return wrap == VSPG_TEXWRAP_REPEAT ? (p & (res - 1)) : clamped;
}
// a continuous texel coordinate held to what converts to int (and xi + 1 with it)
VDEV float tex_coord(float x) { return x < -1e9f ? -1e9f : (x > 1e9f ? 1e9f : (x == x ? x : 0.f)); }
// steps 1-6; *s, *t: st after the flip
VDEV Spec texture_lookup(const DTexture &T, float u, float v, float *s, float *t) {
    const float4 *__restrict__ texels = T.texels;
    const int xres = T.xres, yres = T.yres, wrap = T.wrap;
    const float s0 = T.su * u + T.du;
    const float t0 = 1 - (T.sv * v + T.dv);
    *s = s0;
    *t = t0;
    const float x = tex_coord(s0 * (float)xres - 0.5f), y = tex_coord(t0 * (float)yres - 0.5f);
    Spec f;
    if (T.filter == VSPG_TEXFILTER_POINT) {
        bool cx, cy;
        const int xi = tex_wrap((int)__builtin_roundf(x), xres, wrap, &cx), yi = tex_wrap((int)__builtin_roundf(y), yres, wrap, &cy);
        const float4 a = texels[(size_t)yi * xres + xi];
        const bool c = cx && cy;
        f = Spec{c ? a.x : 0.f, c ? a.y : 0.f, c ? a.z : 0.f};
    } else {
        const float fx = __builtin_floorf(x), fy = __builtin_floorf(y);
        const int xi = (int)fx, yi = (int)fy;
        const float dx = x - (float)xi, dy = y - (float)yi;
        bool cx0, cx1, cy0, cy1;
        const int x0 = tex_wrap(xi, xres, wrap, &cx0), x1 = tex_wrap(xi + 1, xres, wrap, &cx1);
        const int y0 = tex_wrap(yi, yres, wrap, &cy0), y1 = tex_wrap(yi + 1, yres, wrap, &cy1);
        const size_t r0 = (size_t)y0 * xres, r1 = (size_t)y1 * xres;
        const float4 a0 = texels[r0 + x0], a1 = texels[r0 + x1], a2 = texels[r1 + x0], a3 = texels[r1 + x1];  // four loads in flight
        const bool c0 = cx0 && cy0, c1 = cx1 && cy0, c2 = cx0 && cy1, c3 = cx1 && cy1;
        const float w0 = (1 - dx) * (1 - dy), w1 = dx * (1 - dy), w2 = (1 - dx) * dy, w3 = dx * dy;
        auto bilerp = [&](float v0, float v1, float v2, float v3) {
            return ((w0 * (c0 ? v0 : 0.f) + w1 * (c1 ? v1 : 0.f)) + w2 * (c2 ? v2 : 0.f)) + w3 * (c3 ? v3 : 0.f);
        };
        f = Spec{bilerp(a0.x, a1.x, a2.x, a3.x), bilerp(a0.y, a1.y, a2.y, a3.y), bilerp(a0.z, a1.z, a2.z, a3.z)};
    }
    Spec rgb = Spec{T.scale * f.r, T.scale * f.g, T.scale * f.b};
    if (T.invert) rgb = Spec{1 - rgb.r, 1 - rgb.g, 1 - rgb.b};
    rgb = clamp_zero(rgb);
    return Spec{clampf(rgb.r, 0.f, 1.f), clampf(rgb.g, 0.f, 1.f), clampf(rgb.b, 0.f, 1.f)};
}
// The texture of the surface a hit names: 0 = none, k = S.tex[k - 1].  Rectangles and triangles only.
VDEV int tex_of_prim(const DScene &S, int prim) {
    if (is_tri(prim)) return S.tris[tri_of(prim)].flags >> TRI_TEX_SHIFT;
    if (is_sphere(prim)) return 0;
    return S.quad_tex[prim];
}
// What vertex_setup<FULL> and vspg_texture_eval_batch run for a textured hit (k = tex_of_prim != 0): steps 1-7
struct TexEval { TexUv uv; float s, t; Spec R; bool has_lobes; };
VDEV TexEval texture_eval(const DScene &S, int k, int prim, V3 hit) {
    TexEval e;
    e.uv = is_tri(prim) ? tex_uv_tri(S.tri_uv + 6 * (size_t)tri_of(prim), hit) : tex_uv_quad(quad_at(prim), hit);
    e.R = texture_lookup(S.tex[k - 1], e.uv.u, e.uv.v, &e.s, &e.t);
    e.has_lobes = e.R.r != 0 || e.R.g != 0 || e.R.b != 0;
    return e;
}

VSPG_NS_END
