// vspg_scene_build.hip -- host-side scene preprocessing (vspg_scene_build.h): validation, the device scene record, the light
// samplers, the triangle BVH, the majorant grids and the environment-map tables.  No kernel is defined or launched here and no HIP
// function is called: the unit carries no device code, and links and runs without a GPU (tests/scene_build_check.cpp).
#include "vspg_scene_build.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>

#include "vspg_envmap.h"
#include "vspg_error.h"
#include "vspg_portalmap.h"

namespace vspg_host {

// (accMult, G) of RNG::Advance(delta) (src/pbrt/util/rng.h:137-150), see PcgJump
PcgJump pcg_jump(unsigned long long delta) {
    unsigned long long curMult = 0x5851f42d4c957f2dULL, curPlus = 1u, accMult = 1u, accPlus = 0u;
    while (delta > 0) {
        if (delta & 1) {
            accMult *= curMult;
            accPlus = accPlus * curMult + curPlus;
        }
        curPlus = (curMult + 1) * curPlus;
        curMult *= curMult;
        delta /= 2;
    }
    return PcgJump{accMult, accPlus};
}

// ---- light samplers: host-side build (lightsamplers.cpp:76-99 PowerLightSampler, :108-262 BVHLightSampler::buildBVH) ----------
// The reference's construction restated: LightBounds of every bounded light (DiffuseAreaLight::Bounds on a rectangle), the
// modified-SAH split over 12 buckets per axis, CompactLightBounds' quantisation.  The CPU checker states the same thing in C
// (oracle/vspg_oracle.c, "light samplers"); both run the same float operations on the same libm, so the trees are equal.
namespace lsb {
struct v3 { float x, y, z; };
static inline v3 V3(float x, float y, float z) { return v3{x, y, z}; }
static inline v3 v_add(v3 a, v3 b) { return v3{a.x + b.x, a.y + b.y, a.z + b.z}; }
static inline v3 v_sub(v3 a, v3 b) { return v3{a.x - b.x, a.y - b.y, a.z - b.z}; }
static inline v3 v_scale(v3 a, float s) { return v3{a.x * s, a.y * s, a.z * s}; }
static inline v3 v_neg(v3 a) { return v3{-a.x, -a.y, -a.z}; }
static inline float v_dot(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static inline float v_len2(v3 a) { return v_dot(a, a); }
static inline float v_len(v3 a) { return sqrtf(v_len2(a)); }
static inline v3 v_normalize(v3 a) { float l = v_len(a); return v3{a.x / l, a.y / l, a.z / l}; }
static inline float dop(float a, float b, float c, float d) { return hostmath::dop(a, b, c, d); }
static inline v3 v_cross(v3 v, v3 w) { return v3{dop(v.y, w.z, v.z, w.y), dop(v.z, w.x, v.x, w.z), dop(v.x, w.y, v.y, w.x)}; }
static inline float sqr(float x) { return x * x; }
static inline float clampf(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }
static inline float safe_sqrt(float x) { return sqrtf(x > 0 ? x : 0.f); }
constexpr float PI_F = 3.14159265358979323846f;
constexpr int LBVH_MAX_LIGHTS = kMaxLights;
struct lightbounds_t { v3 bmin, bmax; float phi; v3 w; float cosTheta_o, cosTheta_e; int twoSided; };
static float safe_asin_f(float x) { return asinf(clampf(x, -1, 1)); }
static float safe_acos_f(float x) { return acosf(clampf(x, -1, 1)); }
static float angle_between(v3 a, v3 b) { /* vecmath.h:972-977 */
    if (v_dot(a, b) < 0) return PI_F - 2 * safe_asin_f(v_len(v_add(a, b)) / 2);
    return 2 * safe_asin_f(v_len(v_sub(b, a)) / 2);
}
typedef struct { v3 w; float cosTheta; } dircone_t; /* DirectionCone (vecmath.h:1785-1808); cosTheta == INFINITY: empty */
static dircone_t dircone(v3 w, float c) { dircone_t d; d.w = v_normalize(w); d.cosTheta = c; return d; }
static dircone_t dircone_union(dircone_t a, dircone_t b) { /* vecmath.cpp:56-83 */
    if (std::isinf(a.cosTheta)) return b;
    if (std::isinf(b.cosTheta)) return a;
    float theta_a = safe_acos_f(a.cosTheta), theta_b = safe_acos_f(b.cosTheta);
    float theta_d = angle_between(a.w, b.w);
    if (fminf(theta_d + theta_b, PI_F) <= theta_a) return a;
    if (fminf(theta_d + theta_a, PI_F) <= theta_b) return b;
    float theta_o = (theta_a + theta_d + theta_b) / 2;
    if (theta_o >= PI_F) return dircone(V3(0, 0, 1), -1);
    float theta_r = theta_o - theta_a;
    v3 wr = v_cross(a.w, b.w);
    if (v_len2(wr) == 0) return dircone(V3(0, 0, 1), -1);
    /* Rotate(Degrees(theta_r), wr)(a.w) (transform.h:220-247): sin / cos of Radians(Degrees(theta_r)) */
    float deg = (180 / PI_F) * theta_r, rad = (PI_F / 180) * deg;
    float sinT = sinf(rad), cosT = cosf(rad);
    v3 ax = v_normalize(wr);
    float m[3][3];
    m[0][0] = ax.x * ax.x + (1 - ax.x * ax.x) * cosT; m[0][1] = ax.x * ax.y * (1 - cosT) - ax.z * sinT; m[0][2] = ax.x * ax.z * (1 - cosT) + ax.y * sinT;
    m[1][0] = ax.x * ax.y * (1 - cosT) + ax.z * sinT; m[1][1] = ax.y * ax.y + (1 - ax.y * ax.y) * cosT; m[1][2] = ax.y * ax.z * (1 - cosT) - ax.x * sinT;
    m[2][0] = ax.x * ax.z * (1 - cosT) - ax.y * sinT; m[2][1] = ax.y * ax.z * (1 - cosT) + ax.x * sinT; m[2][2] = ax.z * ax.z + (1 - ax.z * ax.z) * cosT;
    v3 w = V3(m[0][0] * a.w.x + m[0][1] * a.w.y + m[0][2] * a.w.z, m[1][0] * a.w.x + m[1][1] * a.w.y + m[1][2] * a.w.z,
              m[2][0] * a.w.x + m[2][1] * a.w.y + m[2][2] * a.w.z); /* Transform::operator()(Vector3f), transform.h:351-356 */
    return dircone(w, cosf(theta_o));
}
static lightbounds_t lb_empty(void) { lightbounds_t b; std::memset(&b, 0, sizeof b); b.bmin = V3(INFINITY, INFINITY, INFINITY); b.bmax = V3(-INFINITY, -INFINITY, -INFINITY); return b; }
static v3 v_min3(v3 a, v3 b) { return V3(fminf(a.x, b.x), fminf(a.y, b.y), fminf(a.z, b.z)); }
static v3 v_max3(v3 a, v3 b) { return V3(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z)); }
static lightbounds_t lb_union(lightbounds_t a, lightbounds_t b) { /* lights.h:137-153 */
    if (a.phi == 0) return b;
    if (b.phi == 0) return a;
    dircone_t ca, cb; ca.w = a.w; ca.cosTheta = a.cosTheta_o; cb.w = b.w; cb.cosTheta = b.cosTheta_o;
    ca.w = v_normalize(ca.w); cb.w = v_normalize(cb.w); /* DirectionCone(w, cosTheta) normalises */
    dircone_t cone = dircone_union(ca, cb);
    lightbounds_t r;
    r.bmin = v_min3(a.bmin, b.bmin); r.bmax = v_max3(a.bmax, b.bmax);
    r.w = v_normalize(cone.w);
    r.phi = a.phi + b.phi;
    r.cosTheta_o = cone.cosTheta;
    r.cosTheta_e = fminf(a.cosTheta_e, b.cosTheta_e);
    r.twoSided = a.twoSided | b.twoSided;
    return r;
}
static v3 lb_centroid(const lightbounds_t *b) { return v_scale(v_add(b->bmin, b->bmax), 0.5f); } /* (pMin + pMax) / 2 */
static float vcomp(v3 v, int d) { return d == 0 ? v.x : (d == 1 ? v.y : v.z); }
/* CompactLightBounds(lb, allb) and back through its accessors (lightsamplers.h:100-142, 212-242; vecmath.h:1733-1782) */
static float quantize_bounds(float c, float mn, float mx) { return mn == mx ? 0.f : 65535.f * clampf((c - mn) / (mx - mn), 0, 1); }
static float lerpf(float t, float a, float b) { return (1 - t) * a + t * b; }
static uint16_t oct_encode(float f) { return (uint16_t)std::round(clampf((f + 1) / 2, 0, 1) * 65535.f); }
static void compact_node(DLightNode *nd, const lightbounds_t *lb, v3 amin, v3 amax) {
    /* OctahedralVector(Normalize(lb.w)) -> Vector3f */
    v3 v = v_normalize(lb->w);
    float l1 = fabsf(v.x) + fabsf(v.y) + fabsf(v.z);
    v = V3(v.x / l1, v.y / l1, v.z / l1);
    uint16_t ox, oy;
    if (v.z >= 0) { ox = oct_encode(v.x); oy = oct_encode(v.y); }
    else { ox = oct_encode((1 - fabsf(v.y)) * copysignf(1.f, v.x)); oy = oct_encode((1 - fabsf(v.x)) * copysignf(1.f, v.y)); }
    v3 d;
    d.x = -1 + 2 * (ox / 65535.f);
    d.y = -1 + 2 * (oy / 65535.f);
    d.z = 1 - (fabsf(d.x) + fabsf(d.y));
    if (d.z < 0) { float xo = d.x; d.x = (1 - fabsf(d.y)) * copysignf(1.f, xo); d.y = (1 - fabsf(xo)) * copysignf(1.f, d.y); }
    { const v3 wn = v_normalize(d); nd->w[0] = wn.x; nd->w[1] = wn.y; nd->w[2] = wn.z; }
    nd->phi = lb->phi;
    unsigned qo = (unsigned)floorf(32767.f * ((lb->cosTheta_o + 1) / 2)), qe = (unsigned)floorf(32767.f * ((lb->cosTheta_e + 1) / 2));
    nd->cosTheta_o = 2 * (qo / 32767.f) - 1;
    nd->cosTheta_e = 2 * (qe / 32767.f) - 1;
    nd->twoSided = lb->twoSided;
    float lo[3], hi[3];
    for (int c = 0; c < 3; ++c) {
        uint16_t q0 = (uint16_t)floorf(quantize_bounds(vcomp(lb->bmin, c), vcomp(amin, c), vcomp(amax, c)));
        uint16_t q1 = (uint16_t)ceilf(quantize_bounds(vcomp(lb->bmax, c), vcomp(amin, c), vcomp(amax, c)));
        lo[c] = lerpf(q0 / 65535.f, vcomp(amin, c), vcomp(amax, c));
        hi[c] = lerpf(q1 / 65535.f, vcomp(amin, c), vcomp(amax, c));
    }
    for (int c = 0; c < 3; ++c) { nd->bmin[c] = lo[c]; nd->bmax[c] = hi[c]; }
}
static float lb_evaluate_cost(const lightbounds_t *b, v3 bdiag, int dim) { /* lightsamplers.h:398-411 */
    float theta_o = acosf(b->cosTheta_o), theta_e = acosf(b->cosTheta_e);
    float theta_w = fminf(theta_o + theta_e, PI_F);
    float sinTheta_o = safe_sqrt(1 - sqr(b->cosTheta_o));
    float M_omega = 2 * PI_F * (1 - b->cosTheta_o) +
                    PI_F / 2 * (2 * theta_w * sinTheta_o - cosf(theta_o - 2 * theta_w) - 2 * theta_o * sinTheta_o + b->cosTheta_o);
    float Kr = fmaxf(bdiag.x, fmaxf(bdiag.y, bdiag.z)) / vcomp(bdiag, dim);
    v3 d = v_sub(b->bmax, b->bmin);
    float area = 2 * (d.x * d.y + d.x * d.z + d.y * d.z); /* Bounds3::SurfaceArea */
    return b->phi * M_omega * Kr * area;
}
typedef struct { int light; lightbounds_t lb; } lbvh_item_t;
static int lbvh_bucket(const lightbounds_t *lb, v3 cmin, v3 cmax, int dim) { /* nBuckets * centroidBounds.Offset(pc)[dim], 12 buckets */
    float pc = vcomp(lb_centroid(lb), dim), mn = vcomp(cmin, dim), mx = vcomp(cmax, dim);
    float o = pc - mn;
    if (mx > mn) o /= mx - mn;
    int b = (int)(12 * o);
    return b == 12 ? 11 : b;
}
static int lbvh_build(DLightSampler *ls, lbvh_item_t *it, int start, int end, uint32_t bitTrail, int depth, v3 amin, v3 amax, lightbounds_t *out) {
    if (end - start == 1) {
        int nodeIndex = ls->n_nodes++;
        compact_node(&ls->nodes[nodeIndex], &it[start].lb, amin, amax);
        ls->nodes[nodeIndex].child_or_light = (uint32_t)it[start].light;
        ls->nodes[nodeIndex].is_leaf = 1;
        ls->bit_trail[it[start].light] = bitTrail;
        *out = it[start].lb;
        return nodeIndex;
    }
    v3 bmin = V3(INFINITY, INFINITY, INFINITY), bmax = V3(-INFINITY, -INFINITY, -INFINITY), cmin = bmin, cmax = bmax;
    for (int i = start; i < end; ++i) {
        bmin = v_min3(bmin, it[i].lb.bmin); bmax = v_max3(bmax, it[i].lb.bmax);
        v3 c = lb_centroid(&it[i].lb);
        cmin = v_min3(cmin, c); cmax = v_max3(cmax, c);
    }
    float minCost = INFINITY;
    int minCostSplitBucket = -1, minCostSplitDim = -1;
    const v3 bdiag = v_sub(bmax, bmin);
    for (int dim = 0; dim < 3; ++dim) {
        if (vcomp(cmax, dim) == vcomp(cmin, dim)) continue;
        lightbounds_t bucket[12];
        for (int b = 0; b < 12; ++b) bucket[b] = lb_empty();
        for (int i = start; i < end; ++i) {
            int b = lbvh_bucket(&it[i].lb, cmin, cmax, dim);
            bucket[b] = lb_union(bucket[b], it[i].lb);
        }
        float cost[11];
        for (int i = 0; i < 11; ++i) {
            lightbounds_t b0 = lb_empty(), b1 = lb_empty();
            for (int j = 0; j <= i; ++j) b0 = lb_union(b0, bucket[j]);
            for (int j = i + 1; j < 12; ++j) b1 = lb_union(b1, bucket[j]);
            cost[i] = lb_evaluate_cost(&b0, bdiag, dim) + lb_evaluate_cost(&b1, bdiag, dim);
        }
        for (int i = 1; i < 11; ++i)
            if (cost[i] > 0 && cost[i] < minCost) { minCost = cost[i]; minCostSplitBucket = i; minCostSplitDim = dim; }
    }
    int mid;
    if (minCostSplitDim == -1) mid = (start + end) / 2;
    else {
        /* std::partition (libstdc++, forward-iterator form is not used for pointers: the bidirectional algorithm) */
        int first = start, last = end;
        while (1) {
            while (1) {
                if (first == last) goto done;
                if (lbvh_bucket(&it[first].lb, cmin, cmax, minCostSplitDim) <= minCostSplitBucket) ++first; else break;
            }
            --last;
            while (1) {
                if (first == last) goto done;
                if (!(lbvh_bucket(&it[last].lb, cmin, cmax, minCostSplitDim) <= minCostSplitBucket)) --last; else break;
            }
            lbvh_item_t t = it[first]; it[first] = it[last]; it[last] = t;
            ++first;
        }
    done:
        mid = first;
        if (mid == start || mid == end) mid = (start + end) / 2;
    }
    int nodeIndex = ls->n_nodes++;
    lightbounds_t l0, l1;
    lbvh_build(ls, it, start, mid, bitTrail, depth + 1, amin, amax, &l0);
    int child1 = lbvh_build(ls, it, mid, end, bitTrail | (1u << depth), depth + 1, amin, amax, &l1);
    lightbounds_t lb = lb_union(l0, l1);
    compact_node(&ls->nodes[nodeIndex], &lb, amin, amax);
    ls->nodes[nodeIndex].child_or_light = (uint32_t)child1;
    ls->nodes[nodeIndex].is_leaf = 0;
    *out = lb;
    return nodeIndex;
}
static lightbounds_t quad_light_bounds(const DQuad &q, int reverse_orientation) {  // lights.cpp:845-864; shapes.cpp:1070-1126
    const v3 p00 = V3(q.p00[0], q.p00[1], q.p00[2]), p10 = V3(q.p10[0], q.p10[1], q.p10[2]), p01 = V3(q.p01[0], q.p01[1], q.p01[2]),
             p11 = V3(q.p11[0], q.p11[1], q.p11[2]);
    lightbounds_t lb;
    lb.bmin = v_min3(v_min3(p00, p01), v_min3(p10, p11));
    lb.bmax = v_max3(v_max3(p00, p01), v_max3(p10, p11));
    v3 n00 = v_normalize(v_cross(v_sub(p10, p00), v_sub(p01, p00)));
    v3 n10 = v_normalize(v_cross(v_sub(p11, p10), v_sub(p00, p10)));
    v3 n01 = v_normalize(v_cross(v_sub(p00, p01), v_sub(p11, p01)));
    v3 n11 = v_normalize(v_cross(v_sub(p01, p11), v_sub(p10, p11)));
    if (reverse_orientation) { n00 = v_neg(n00); n10 = v_neg(n10); n01 = v_neg(n01); n11 = v_neg(n11); }
    v3 n = v_normalize(v_add(v_add(n00, n10), v_add(n01, n11)));
    float cosTheta = fminf(fminf(v_dot(n, n00), v_dot(n, n01)), fminf(v_dot(n, n10), v_dot(n, n11)));
    dircone_t nb = dircone(n, clampf(cosTheta, -1, 1));
    float phi = fmaxf(q.Le[0], fmaxf(q.Le[1], q.Le[2]));  // Lemit->MaxValue(), RGB rendering mode (spectrum.h:772-779)
    phi *= 1.f * q.area * PI_F;                           // scale * area * Pi
    lb.w = v_normalize(nb.w);
    lb.phi = phi;
    lb.cosTheta_o = nb.cosTheta;
    lb.cosTheta_e = cosf(PI_F / 2);
    lb.twoSided = q.two_sided;
    return lb;
}
// PointLight::Bounds (lights.cpp:200-205) / SpotLight::Bounds (:1457-1467): a degenerate box at the light's position
// DiffuseAreaLight::Bounds (lights.cpp:845-864) over a sphere: Sphere::Bounds (shapes.cpp:33-36) = the object box carried to render space
// corner by corner (Transform::operator()(Bounds3f), transform.cpp:134-139; Point3f operator() transform.h:310-319), NormalBounds =
// DirectionCone::EntireSphere() (shapes.h:134; w = (0, 0, 1), cosTheta = -1), phi = Lemit->MaxValue() * scale * area * Pi
static lightbounds_t sphere_light_bounds(const DSphere &S, const DSphereLight &E) {
    lightbounds_t lb;
    lb.bmin = V3(INFINITY, INFINITY, INFINITY);
    lb.bmax = V3(-INFINITY, -INFINITY, -INFINITY);
    const float r = S.radius;
    for (int c = 0; c < 8; ++c) {  // Bounds3::Corner: bit 0 -> x, bit 1 -> y, bit 2 -> z
        const float x = (c & 1) ? r : -r, y = (c & 2) ? r : -r, z = (c & 4) ? r : -r;
        float q[3];
        for (int k = 0; k < 3; ++k) {
            volatile float a = S.m[4 * k] * x;  // volatile: one rounding per operation, no contraction
            volatile float b = S.m[4 * k + 1] * y;
            volatile float c2 = S.m[4 * k + 2] * z;
            volatile float sum = a + b;
            sum = sum + c2;
            sum = sum + S.m[4 * k + 3];
            q[k] = sum;
        }
        const v3 p = V3(q[0], q[1], q[2]);  // (affine: wp == 1)
        lb.bmin = v_min3(lb.bmin, p);
        lb.bmax = v_max3(lb.bmax, p);
    }
    float phi = fmaxf(E.Le[0], fmaxf(E.Le[1], E.Le[2]));
    volatile float dz = r - (-r);
    volatile float a = S.phiMax * r;
    a = a * dz;
    phi *= 1.f * a * PI_F;  // scale * area * Pi
    lb.w = V3(0, 0, 1);
    lb.phi = phi;
    lb.cosTheta_o = -1;
    lb.cosTheta_e = cosf(PI_F / 2);
    lb.twoSided = E.two_sided;
    return lb;
}
// ProjectionLight::Bounds (lights.cpp:426-441): phi = scale * sum of max(R, G, B) / (width * height), the cone of the screen window's corner
// around Normalize(renderFromLight(Vector3f(0, 0, 1))); GoniometricLight::Bounds (:612-624): "Bound it as an isotropic point light", phi =
// scale * Iemit->MaxValue() * 4 * Pi * sumY / (width * height).  Where the reference has a scalar scale the record has an RGB I: its
// largest component, as PointLight::Bounds takes MaxValue.
static lightbounds_t point_light_bounds(const DPointLight &P, const DImageLight &G) {
    lightbounds_t lb;
    lb.bmin = lb.bmax = V3(P.pos[0], P.pos[1], P.pos[2]);
    const float maxI = fmaxf(P.I[0], fmaxf(P.I[1], P.I[2]));  // scale * I->MaxValue()
    lb.twoSided = 0;
    if (P.type == VSPG_LIGHT_PROJECTION) {
        lb.w = V3(P.axis[0], P.axis[1], P.axis[2]);
        lb.phi = maxI * G.sum_bounds / (float)(G.xres * G.yres);
        lb.cosTheta_o = cosf(0.f);
        lb.cosTheta_e = G.cosTotalWidth;
    } else if (P.type == VSPG_LIGHT_GONIOMETRIC) {
        lb.w = V3(0, 0, 1);
        lb.phi = maxI * 4 * PI_F * G.sum_bounds / (float)(G.xres * G.yres);
        lb.cosTheta_o = cosf(PI_F);
        lb.cosTheta_e = cosf(PI_F / 2);
    } else if (P.type == VSPG_LIGHT_SPOT) {
        lb.w = V3(P.axis[0], P.axis[1], P.axis[2]);
        lb.phi = maxI * 4 * PI_F;
        lb.cosTheta_o = P.cosFalloffStart;
        float cosTheta_e = cosf(acosf(P.cosFalloffEnd) - acosf(P.cosFalloffStart));
        // "Allow a little slop here to deal with fp round-off error in the computation of cosTheta_p in the importance function."
        if (cosTheta_e == 1 && P.cosFalloffEnd != P.cosFalloffStart) cosTheta_e = 0.999f;
        lb.cosTheta_e = cosTheta_e;
    } else {
        lb.w = V3(0, 0, 1);
        lb.phi = 4 * PI_F * maxI;
        lb.cosTheta_o = cosf(PI_F);
        lb.cosTheta_e = cosf(PI_F / 2);
    }
    return lb;
}
// (called again by vspg_renderer_set_environment_image and vspg_renderer_set_light_image: the power sampler's table depends on an image
// light's Phi, the BVH on a projection / goniometric light's LightBounds)
void build(const VspgScene &sc, const VspgIntegratorParams &prm, DScene *D) {
    DLightSampler *ls = &D->lsamp;
    std::memset(ls, 0, sizeof *ls);
    const int n_all = light_list_size(*D), first_point = D->n_lights + D->n_inf, first_sphere = first_point + D->n_point;
    for (int i = 0; i < kMaxLights; ++i) ls->bit_trail[i] = 0xffffffffu;
    for (int i = 0; i < VSPG_MAX_QUADS; ++i) ls->light_of_quad[i] = -1;
    for (int i = 0; i < D->n_lights; ++i) ls->light_of_quad[D->light_quads[i]] = i;
    for (int i = 0; i < VSPG_MAX_SPHERES; ++i) ls->light_of_sphere[i] = -1;
    for (int i = 0; i < D->n_sphere_lights; ++i) ls->light_of_sphere[D->light_spheres[i]] = first_sphere + i;
    // every sampler picks a scene's only light with pmf 1: the two-line uniform pick serves (and keeps the workgroup kernels)
    ls->mode = n_all > 1 ? prm.lightsampler : VSPG_LIGHTSAMPLER_UNIFORM;
    lbvh_item_t items[LBVH_MAX_LIGHTS];
    int n_items = 0;
    v3 amin = V3(INFINITY, INFINITY, INFINITY), amax = V3(-INFINITY, -INFINITY, -INFINITY);
    for (int i = 0; i < n_all; ++i) {
        if (i >= D->n_lights && i < first_point) { ls->inf_light[ls->n_inf++] = i; continue; }  // Bounds() == {}
        lightbounds_t lb;
        if (i >= first_sphere) lb = sphere_light_bounds(D->spheres[D->light_spheres[i - first_sphere]], D->sphere_light[D->light_spheres[i - first_sphere]]);
        else if (i >= first_point) lb = point_light_bounds(D->point[i - first_point], D->image_light[i - first_point]);
        else {
            const int qi = D->light_quads[i];
            lb = quad_light_bounds(D->quads[qi], sc.quads[qi].reverse_orientation);
        }
        if (lb.phi > 0) {
            items[n_items].light = i; items[n_items].lb = lb; n_items++;
            amin = v_min3(amin, lb.bmin); amax = v_max3(amax, lb.bmax);
        }
    }
    if (n_items > 0) { lightbounds_t root; lbvh_build(ls, items, 0, n_items, 0, 0, amin, amax, &root); }
    // PowerLightSampler: phi = SafeDiv(light.Phi(lambda), lambda.PDF()).Average(), lambda = SampledWavelengths::SampleVisible(0.5f)
    if (n_all > 0) {
        float pdf[3], power[LBVH_MAX_LIGHTS], acc0 = 0.f;
        for (int i = 0; i < 3; ++i) {
            float up = 0.5f + (float)i / 3;
            if (up > 1) up -= 1;
            float lambda = 538 - 138.888889f * atanhf(0.85691062f - 1.82750197f * up);
            pdf[i] = lambda < 360 || lambda > 830 ? 0.f : 0.0039398042f / sqr(coshf(0.0072f * (lambda - 538)));
        }
        for (int i = 0; i < n_all; ++i) {
            float L[3], k, phi[3] = {0.f, 0.f, 0.f};
            bool have_phi = false;
            if (i < D->n_lights) {
                const DQuad &q = D->quads[D->light_quads[i]];
                for (int c = 0; c < 3; ++c) L[c] = q.Le[c];
                k = PI_F * (q.two_sided ? 2 : 1) * q.area;  // DiffuseAreaLight::Phi (lights.cpp:826-843)
            } else if (i >= first_sphere) {
                const int si = D->light_spheres[i - first_sphere];
                const DSphereLight &E = D->sphere_light[si];
                for (int c = 0; c < 3; ++c) L[c] = E.Le[c];
                volatile float dz = D->spheres[si].radius - (-D->spheres[si].radius);
                volatile float area = D->spheres[si].phiMax * D->spheres[si].radius;
                area = area * dz;
                k = PI_F * (E.two_sided ? 2 : 1) * area;  // DiffuseAreaLight::Phi (lights.cpp:826-843)
            } else if (i >= first_point) {
                const DPointLight &P = D->point[i - first_point];
                for (int c = 0; c < 3; ++c) L[c] = P.I[c];
                k = 4 * PI_F;  // PointLight::Phi = 4 * Pi * scale * I (lights.cpp:196-198)
                if (P.type == VSPG_LIGHT_SPOT) {
                    // SpotLight::Phi (lights.cpp:1452-1455) in its order: scale * Iemit * 2 * Pi * ((1 - cosStart) + (cosStart - cosEnd) / 2)
                    const float cone = (1 - P.cosFalloffStart) + (P.cosFalloffStart - P.cosFalloffEnd) / 2;
                    for (int c = 0; c < 3; ++c) phi[c] = L[c] * 2 * PI_F * cone;
                    have_phi = true;
                } else if (P.type == VSPG_LIGHT_PROJECTION) {
                    // ProjectionLight::Phi (lights.cpp:404-424) in its order: scale * A * sum / (width * height), per channel of I
                    const DImageLight &G = D->image_light[i - first_point];
                    for (int c = 0; c < 3; ++c) phi[c] = L[c] * G.A * G.sum_phi[c] / (float)(G.xres * G.yres);
                    have_phi = true;
                } else if (P.type == VSPG_LIGHT_GONIOMETRIC) {
                    // GoniometricLight::Phi (lights.cpp:603-610) in its order: scale * Iemit * 4 * Pi * sumY / (width * height)
                    const DImageLight &G = D->image_light[i - first_point];
                    for (int c = 0; c < 3; ++c) phi[c] = L[c] * 4 * PI_F * G.sum_phi[0] / (float)(G.xres * G.yres);
                    have_phi = true;
                }
            } else {
                const int j = i - D->n_lights;
                for (int c = 0; c < 3; ++c) L[c] = D->inf_L[j][c];
                k = D->inf_type[j] == VSPG_LIGHT_DISTANT ? PI_F * sqr(D->scene_radius) : 4 * PI_F * PI_F * sqr(D->scene_radius);
                if (D->inf_type[j] == VSPG_LIGHT_IMAGE_INFINITE) {
                    // ImageInfiniteLight::Phi (lights.cpp:1141) in its order: 4 * Pi * Pi * Sqr(sceneRadius) * scale * sumL / (width * height)
                    const DEnvLight &E = D->env[j];
                    for (int c = 0; c < 3; ++c) phi[c] = k * L[c] * E.sum_L[c] / (float)(E.res * E.res);
                    // PortalImageInfiniteLight::Phi (lights.cpp:1284) in its order: scale * Area() * sumL / (width * height)
                    const DPortalLight &Q = D->portal[j];
                    if (Q.res > 0)
                        for (int c = 0; c < 3; ++c) phi[c] = L[c] * Q.area * Q.sum_phi[c] / (float)(Q.res * Q.res);
                    have_phi = true;
                }
            }
            float s = 0.f;
            for (int c = 0; c < 3; ++c) s += pdf[c] != 0 ? (have_phi ? phi[c] : k * L[c]) / pdf[c] : 0.f;
            power[i] = s / 3;
            acc0 += power[i];
        }
        if (acc0 == 0.f) for (int i = 0; i < n_all; ++i) power[i] = 1.f;
        double sum = 0.;  // AliasTable (util/sampling.cpp:563-618)
        for (int i = 0; i < n_all; ++i) sum += power[i];
        const float fsum = (float)sum;
        ls->n_alias = n_all;
        struct { float pHat; int index; } under[LBVH_MAX_LIGHTS], over[LBVH_MAX_LIGHTS];
        int nu = 0, no = 0;
        for (int i = 0; i < n_all; ++i) {
            ls->alias_p[i] = power[i] / fsum;
            float pHat = ls->alias_p[i] * n_all;
            if (pHat < 1) { under[nu].pHat = pHat; under[nu].index = i; nu++; } else { over[no].pHat = pHat; over[no].index = i; no++; }
        }
        while (nu > 0 && no > 0) {
            float upH = under[nu - 1].pHat, ovH = over[no - 1].pHat;
            int ui = under[nu - 1].index, oi = over[no - 1].index;
            nu--; no--;
            ls->alias_q[ui] = upH; ls->alias_i[ui] = oi;
            float pExcess = upH + ovH - 1;
            if (pExcess < 1) { under[nu].pHat = pExcess; under[nu].index = oi; nu++; } else { over[no].pHat = pExcess; over[no].index = oi; no++; }
        }
        while (no > 0) { no--; ls->alias_q[over[no].index] = 1; ls->alias_i[over[no].index] = -1; }
        while (nu > 0) { nu--; ls->alias_q[under[nu].index] = 1; ls->alias_i[under[nu].index] = -1; }
    }
}
}  // namespace lsb

// ---- image infinite light: the host side of vspg_envlight.h (EnvTables: vspg_scene_build.h) ---------------------------------------
// PiecewiseConstant1D's constructor over [0, 1] (util/sampling.h:625-649): func (made absolute) and cdf[n + 1], sequential float sums
static float env_build_1d(float *func, float *cdf, int n) {
    for (int i = 0; i < n; ++i) func[i] = std::fabs(func[i]);
    cdf[0] = 0;
    for (int i = 1; i < n + 1; ++i) cdf[i] = cdf[i - 1] + func[i - 1] * (1.f - 0.f) / (float)n;
    const float funcInt = cdf[n];
    if (funcInt == 0)
        for (int i = 1; i < n + 1; ++i) cdf[i] = (float)i / (float)n;
    else
        for (int i = 1; i < n + 1; ++i) cdf[i] /= funcInt;
    return funcInt;
}
// What ImageInfiniteLight's constructor derives from the image (lights.cpp:1100-1110), compensated distribution only
void env_build_tables(const float *rgb, int res, EnvTables *T) {
    const size_t n = (size_t)res * res;
    T->res = res;
    T->o_func = 3 * n;
    T->o_cdf = T->o_func + n;
    T->o_mfunc = T->o_cdf + (size_t)res * (res + 1);
    T->o_mcdf = T->o_mfunc + res;
    T->buf.assign(T->o_mcdf + res + 1, 0.f);
    std::memcpy(T->buf.data(), rgb, 3 * n * sizeof(float));
    float *d = T->buf.data() + T->o_func;
    float sumL[3] = {0.f, 0.f, 0.f};  // Phi (lights.cpp:1127-1138): ClampZero(rgb) summed per channel, rows then columns
    for (size_t i = 0; i < n; ++i) {
        float sum = 0;  // ImageChannelValues::Average (util/image.h:205-210); dxdA = 1 (GetSamplingDistribution, image.h:338-339, 450-469)
        for (int c = 0; c < 3; ++c) sum += rgb[3 * i + c];
        d[i] = sum / 3;
        for (int c = 0; c < 3; ++c) sumL[c] += rgb[3 * i + c] > 0.f ? rgb[3 * i + c] : 0.f;
    }
    for (int c = 0; c < 3; ++c) T->sum_L[c] = sumL[c];
    double acc = 0.;  // std::accumulate(d.begin(), d.end(), 0.) / d.size() (lights.cpp:1105)
    for (size_t i = 0; i < n; ++i) acc += d[i];
    const float average = (float)(acc / (double)n);  // `Float average`: the double quotient rounded to float once
    bool all_zero = true;
    for (size_t i = 0; i < n; ++i) {
        const float v = d[i] - average;                    // std::max<Float>(v - average, 0): a float subtraction
        d[i] = v < 0.f ? 0.f : v;                          // (std::max(a, b) = a < b ? b : a; a NaN cannot occur: the texels are finite)
        all_zero = all_zero && d[i] == 0;
    }
    if (all_zero) for (size_t i = 0; i < n; ++i) d[i] = 1.f;
    // PiecewiseConstant2D (util/sampling.h:737-754): a 1-D distribution per row, then the marginal over the rows' integrals
    float *cdf = T->buf.data() + T->o_cdf, *mfunc = T->buf.data() + T->o_mfunc, *mcdf = T->buf.data() + T->o_mcdf;
    for (int v = 0; v < res; ++v) mfunc[v] = env_build_1d(d + (size_t)v * res, cdf + (size_t)v * (res + 1), res);
    T->integral = env_build_1d(mfunc, mcdf, res);
}
// The linear part of render_from_light (3 x 4 row-major, NULL = identity) and its inverse: cofactors over the determinant in double,
// each entry rounded to float once.  false: a non-finite entry or a singular matrix.
bool env_matrices(const float *m34, float *m, float *mi) {
    static const float ident[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    const float *s = m34 ? m34 : ident;
    double A[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            m[3 * r + c] = s[4 * r + c];
            A[3 * r + c] = (double)s[4 * r + c];
            if (!std::isfinite(s[4 * r + c])) return false;
        }
    const double a = A[0], b = A[1], c = A[2], d = A[3], e = A[4], f = A[5], g = A[6], h = A[7], i = A[8];
    const double c00 = e * i - f * h, c01 = f * g - d * i, c02 = d * h - e * g;
    const double det = (a * c00 + b * c01) + c * c02;
    if (!(det != 0) || !std::isfinite(det)) return false;
    const double adj[9] = {c00, c * h - b * i, b * f - c * e, c01, a * i - c * g, c * d - a * f, c02, b * g - a * h, a * e - b * d};
    for (int k = 0; k < 9; ++k) {
        mi[k] = (float)(adj[k] / det);
        if (!std::isfinite(mi[k])) return false;
    }
    return true;
}
// ---- portal image infinite light: the host side of vspg_portallight.h (PortalTables: vspg_scene_build.h) ---------------------------
int portal_refusal(const float *q) {
    if (!q) return fail(VSPG_EINVAL, "null argument");
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(q[i])) return fail(VSPG_EINVAL, "a portal vertex is not finite");
    const V3 p[4] = {ld3(q), ld3(q + 3), ld3(q + 6), ld3(q + 9)};
    const V3 e[4] = {p[1] - p[0], p[2] - p[1], p[2] - p[3], p[3] - p[0]};
    for (int i = 0; i < 4; ++i)
        if (!(len2(e[i]) > 0) || !std::isfinite(len2(e[i]))) return fail(VSPG_EINVAL, "the portal has a degenerate edge");
    // lights.cpp:1218-1228: float dot products of the normalised edges, the differences and .001 compared in double
    const V3 p01 = normalize(e[0]), p12 = normalize(e[1]), p32 = normalize(e[2]), p03 = normalize(e[3]);
    if (!(std::abs((double)(dot(p01, p32) - 1)) <= .001) || !(std::abs((double)(dot(p12, p03) - 1)) <= .001))
        return fail(VSPG_EINVAL, "Infinite light portal isn't a planar quadrilateral (opposite edges are not parallel)");
    if (!(std::abs((double)dot(p01, p12)) <= .001) || !(std::abs((double)dot(p12, p32)) <= .001) || !(std::abs((double)dot(p32, p03)) <= .001) ||
        !(std::abs((double)dot(p03, p01)) <= .001))
        return fail(VSPG_EINVAL, "Infinite light portal isn't a planar quadrilateral (sides are not perpendicular)");
    return 0;
}
void portal_build_tables(const float *rgb, int res, const float *mi, const float *q, PortalTables *T) {
    static const float white[3] = {1.f, 1.f, 1.f};
    env_build_tables(white, 1, &T->env);
    const size_t n = (size_t)res * res;
    T->o_image = T->env.buf.size();
    T->o_func = T->o_image + 3 * n;
    T->o_sat = T->o_func + n;
    T->env.buf.resize(T->o_sat + n, 0.f);
    DPortalLight &P = T->rec;
    P = DPortalLight{};
    P.res = res;
    const V3 p0 = ld3(q), p1 = ld3(q + 3), p2 = ld3(q + 6), p3 = ld3(q + 9);
    const V3 fx = normalize(p3 - p0), fy = normalize(p1 - p0), fz = cross(fx, fy);  // Frame::FromXY(p03, p01)
    for (int c = 0; c < 3; ++c) {
        P.p0[c] = q[c];
        P.p2[c] = q[6 + c];
        P.fx[c] = (&fx.x)[c];
        P.fy[c] = (&fy.x)[c];
        P.fz[c] = (&fz.x)[c];
    }
    P.area = len(p1 - p0) * len(p3 - p0);  // Area() (lights.h:794-796)
    float *image = T->env.buf.data() + T->o_image, *func = T->env.buf.data() + T->o_func, *sat = T->env.buf.data() + T->o_sat;
    // the rectified image (lights.cpp:1232-1250): Image::BilerpChannel (util/image.h:279-292) of the equal-area image under the
    // octahedral wrap; then d = Average(R, G, B) * duv_dw(centre) (Image::GetSamplingDistribution, util/image.h:450-469) and Phi's
    // sums (lights.cpp:1262-1285), all in image order
    float sum_phi[3] = {0.f, 0.f, 0.f};
    for (int y = 0; y < res; ++y)
        for (int x = 0; x < res; ++x) {
            const float u = ((float)x + 0.5f) / (float)res, v = ((float)y + 0.5f) / (float)res;
            float duv_dw;
            V3 w = portal_render_from_image(P, u, v, &duv_dw);
            w = normalize(env_xform(mi, w));
            float ue, ve;
            env_sphere_to_square(w, &ue, &ve);
            const float fxp = ue * (float)res - 0.5f, fyp = ve * (float)res - 0.5f;
            const int xi = (int)std::floor(fxp), yi = (int)std::floor(fyp);
            const float dx = fxp - (float)xi, dy = fyp - (float)yi;
            const float *t[4];
            for (int j = 0; j < 4; ++j) {
                int px = xi + (j & 1), py = yi + (j >> 1);
                env_remap_octahedral(&px, &py, res);
                px = px < 0 ? 0 : (px > res - 1 ? res - 1 : px);  // (a finite direction lands inside the image)
                py = py < 0 ? 0 : (py > res - 1 ? res - 1 : py);
                t[j] = rgb + 3 * ((size_t)py * res + px);
            }
            float *o = image + 3 * ((size_t)y * res + x);
            float sum = 0.f;
            for (int c = 0; c < 3; ++c) {
                o[c] = (1 - dx) * (1 - dy) * t[0][c] + dx * (1 - dy) * t[1][c] + (1 - dx) * dy * t[2][c] + dx * dy * t[3][c];
                sum += o[c];
                sum_phi[c] += (o[c] > 0.f ? o[c] : 0.f) / duv_dw;
            }
            func[(size_t)y * res + x] = sum / 3 * duv_dw;
        }
    for (int c = 0; c < 3; ++c) P.sum_phi[c] = sum_phi[c];
    // SummedAreaTable (util/sampling.h:834-848): double sums in its order, each rounded to float once at the end
    std::vector<double> s(n);
    s[0] = func[0];
    for (int x = 1; x < res; ++x) s[x] = (double)func[x] + s[x - 1];
    for (int y = 1; y < res; ++y) s[(size_t)y * res] = (double)func[(size_t)y * res] + s[(size_t)(y - 1) * res];
    for (int y = 1; y < res; ++y)
        for (int x = 1; x < res; ++x) {
            const size_t i = (size_t)y * res + x;
            s[i] = (double)func[i] + s[i - 1] + s[i - res] - s[i - res - 1];
        }
    for (size_t i = 0; i < n; ++i) sat[i] = (float)s[i];
}
// ---- projection and goniometric lights: the host side of vspg_imagelight.h (ImageLightTables: vspg_scene_build.h) -------------------
// The refusals of vspg_renderer_set_light_image that need no renderer, in its order; 0 or VSPG_EINVAL with the message set
int image_light_refusal(int type, const float *pixels, int xres, int yres, int channels) {
    if (!pixels) return fail(VSPG_EINVAL, "null argument");
    if (type != VSPG_LIGHT_PROJECTION && type != VSPG_LIGHT_GONIOMETRIC) return fail(VSPG_EINVAL, "the point light is neither a projection nor a goniometric light");
    if (channels != (type == VSPG_LIGHT_PROJECTION ? 3 : 1))
        return fail(VSPG_EINVAL, type == VSPG_LIGHT_PROJECTION ? "a projection light's image has 3 channels (R, G, B)" : "a goniometric light's image has 1 channel (Y)");
    if (xres < 1 || xres > VSPG_LIGHT_IMAGE_MAX_RES || yres < 1 || yres > VSPG_LIGHT_IMAGE_MAX_RES)
        return fail(VSPG_EINVAL, "light image resolution outside 1 .. VSPG_LIGHT_IMAGE_MAX_RES (4096)");
    if (type == VSPG_LIGHT_GONIOMETRIC && xres != yres) return fail(VSPG_EINVAL, "goniometric image resolution is non-square: it's unlikely this is an equal-area environment map");
    const size_t n = (size_t)xres * yres * channels;
    for (size_t i = 0; i < n; ++i) {
        if (pixels[i] != pixels[i]) return fail(VSPG_EINVAL, "light image has not-a-number pixel values and so is not suitable as a light");
        if (std::isinf(pixels[i])) return fail(VSPG_EINVAL, "light image has infinite pixel values and so is not suitable as a light");
    }
    return 0;
}
// What the two constructors, Phi() and Bounds() derive from the image (and, for a projection light, the field of view), in the
// reference's order of operations.  The arguments have passed image_light_refusal; fov_deg lies in (0, 180).
void image_light_build(int type, const float *pixels, int xres, int yres, float fov_deg, ImageLightTables *T) {
    using namespace hostmath;
    const size_t n = (size_t)xres * yres;
    T->type = type;
    T->xres = xres;
    T->yres = yres;
    T->hither = 1e-3f;
    T->A = 0.f;
    T->cosTotalWidth = 0.f;
    for (int k = 0; k < 4; ++k) T->sb[k] = 0.f;
    for (int k = 0; k < 12; ++k) T->sfl[k] = 0.f;
    for (int c = 0; c < 3; ++c) T->sum_phi[c] = 0.f;
    if (type == VSPG_LIGHT_GONIOMETRIC) {
        T->buf.assign(pixels, pixels + n);
        float sumY = 0;  // Phi (lights.cpp:604-607) and Bounds (:613-616): the same sum, rows then columns
        for (size_t i = 0; i < n; ++i) sumY += pixels[i];
        T->sum_phi[0] = sumY;
        T->sum_bounds = sumY;
        return;
    }
    // the constructor (lights.cpp:334-344): the screen window, screenFromLight = Perspective(fov, hither, 1e30), its inverse, A
    const float aspect = (float)xres / (float)yres;
    if (aspect > 1) { T->sb[0] = -aspect; T->sb[1] = -1; T->sb[2] = aspect; T->sb[3] = 1; }
    else { T->sb[0] = -1; T->sb[1] = -1 / aspect; T->sb[2] = 1; T->sb[3] = 1 / aspect; }
    // Perspective (transform.cpp:119-131): persp = {1 0 0 0; 0 1 0 0; 0 0 f/(f-n) -f*n/(f-n); 0 0 1 0}, then Scale(invTanAng, invTanAng, 1) *
    // Transform(persp).  The product accumulates by FMA from 0 (SquareMatrix::operator*): next to exact zeros and ones every entry is one
    // factor as it stands.
    const float nn = T->hither, ff = 1e30f;
    const float pa = ff / (ff - nn), pb = -ff * nn / (ff - nn);
    const float deg2rad = 3.14159265358979323846f / 180;  // Radians (math.h:261-263)
    const float half = (deg2rad * fov_deg) / 2;
    const float invTanAng = 1 / std::tan(half);
    T->sfl[0] = invTanAng;   // row 0: {invTanAng, 0, 0, 0}
    T->sfl[5] = invTanAng;   // row 1: {0, invTanAng, 0, 0}
    T->sfl[10] = 1.f;        // row 3: {0, 0, 1, 0}
    // Transform(persp)'s mInv = Inverse(persp) (util/math.h:1571-1624): of the 2 x 2 sub-determinants only s0 = 1 and c5 = -pb are not
    // zero (DifferenceOfProducts is exact there), determinant = -pb, s = 1 / determinant, and the entries that are not zero are
    //   [0][0] = [1][1] = [2][3] = s * -pb   [3][2] = s * -1   [3][3] = s * pa
    // lightFromScreen = Inverse(screenFromLight): m = Inverse(persp) * Scale's minv = diag(1 / invTanAng, 1 / invTanAng, 1, 1).
    const float det = -pb, si = 1 / det;
    const float one = si * -pb;
    const float l00 = one * (1 / invTanAng), l23 = one, l33 = si * pa;
    // lightFromScreen(Point3f(x, y, 0)) (transform.h:310-319), then Vector3f, Normalize: the direction through a screen point
    auto dir = [&](float x, float y) {
        const float xp = l00 * x + 0.f * y + 0.f * 0.f + 0.f, yp = 0.f * x + l00 * y + 0.f * 0.f + 0.f, zp = 0.f * x + 0.f * y + 0.f * 0.f + l23;
        const float wp = 0.f * x + 0.f * y + -si * 0.f + l33;
        const H3 v = wp == 1 ? H3{xp, yp, zp} : H3{xp / wp, yp / wp, zp / wp};
        return normv(v);
    };
    const float opposite = std::tan(half);
    T->A = 4 * (opposite * opposite) * (aspect > 1 ? aspect : (1 / aspect));
    T->cosTotalWidth = dir(T->sb[2], T->sb[3]).z;  // Bounds (lights.cpp:434-436)
    // the device image: ClampZero(rgb) and a zero pad per texel; Phi's sum (lights.cpp:405-421) and Bounds' (:427-431) on the way
    T->buf.assign(4 * n, 0.f);
    float sum[3] = {0.f, 0.f, 0.f}, sum_max = 0;
    for (int y = 0; y < yres; ++y)
        for (int x = 0; x < xres; ++x) {
            const float tx = (x + 0.5f) / xres, ty = (y + 0.5f) / yres;
            // screenBounds.Lerp (vecmath.h:1228-1231): Lerp(t, a, b) = (1 - t) * a + t * b (math.h:210-212)
            const float px = (1 - tx) * T->sb[0] + tx * T->sb[2], py = (1 - ty) * T->sb[1] + ty * T->sb[3];
            const float c = dir(px, py).z;
            const float dwdA = c * c * c;  // Pow<3>
            const float *t = pixels + 3 * ((size_t)y * xres + x);
            float *o = T->buf.data() + 4 * ((size_t)y * xres + x);
            for (int k = 0; k < 3; ++k) {
                o[k] = 0.f < t[k] ? t[k] : 0.f;  // ClampZero: std::max<Float>(0, v)
                sum[k] += o[k] * dwdA;
            }
            float m = t[0];  // std::max({R, G, B})
            if (m < t[1]) m = t[1];
            if (m < t[2]) m = t[2];
            sum_max += m;
        }
    for (int k = 0; k < 3; ++k) T->sum_phi[k] = sum[k];
    T->sum_bounds = sum_max;
}
// ... into a slot's record; the texel pointer is the renderer's to set
void image_light_apply(const ImageLightTables &T, DImageLight *G) {
    G->xres = T.xres;
    G->yres = T.yres;
    for (int k = 0; k < 4; ++k) G->sb[k] = T.sb[k];
    for (int k = 0; k < 12; ++k) G->sfl[k] = T.sfl[k];
    G->hither = T.hither;
    G->A = T.A;
    for (int k = 0; k < 3; ++k) G->sum_phi[k] = T.sum_phi[k];
    G->sum_bounds = T.sum_bounds;
    G->cosTotalWidth = T.cosTotalWidth;
}
// SURF_* flags from the C-ABI's material / medium_interface pair: a MediumInterface only counts when it is a TRANSITION
// (inside != outside, base/medium.h:124)
static int32_t surf_flags_of(int material, int medium_interface) {
    const int b = medium_interface & (VSPG_IFACE_INSIDE | VSPG_IFACE_OUTSIDE);
    const int iface = (b == VSPG_IFACE_INSIDE || b == VSPG_IFACE_OUTSIDE) ? b : 0;
    return (material == VSPG_MATERIAL_INTERFACE ? SURF_INTERFACE : 0) | (iface << SURF_IFACE_SHIFT);
}
void build_dscene(const VspgScene &sc, const VspgIntegratorParams &prm, const VspgRenderConfig &cfg, DScene *D) {
    using namespace hostmath;
    memset(D, 0, sizeof *D);
    D->n_quads = sc.n_quads;
    int frame = 0;   // the axis frame the rectangle tests are in after record i - 1 (IsectRec)
    for (int i = 0; i < sc.n_quads; ++i) {
        const VspgQuad &in = sc.quads[i];
        DQuad &q = D->quads[i];
        H3 p00 = ld(in.p00), e1 = ld(in.e1), e2 = ld(in.e2);
        H3 p10 = add(p00, e1), p01 = add(p00, e2), p11 = add(p10, e2);
        stv(q.p00, p00); stv(q.p10, p10); stv(q.p01, p01); stv(q.p11, p11); stv(q.e1, e1); stv(q.e2, e2);
        H3 c = crossv(e1, e2);
        q.area = std::sqrt(len2v(c));
        H3 n = normv(c);
        if (in.reverse_orientation) n = H3{-n.x, -n.y, -n.z};
        stv(q.n, n);
        stv(q.dpdu_n, normv(e1));
        const float eps = 0x1p-24f;
        float g6 = (6 * eps) / (1 - 6 * eps);  // gamma(6) (util/float.h:195)
        H3 s = add(add(absv(p00), absv(p01)), add(absv(p10), absv(p11)));
        stv(q.perr, H3{s.x * g6, s.y * g6, s.z * g6});
        q.inv_l1 = 1.f / len2v(e1);
        q.inv_l2 = 1.f / len2v(e2);
        bool lobes = false, light = false;
        for (int k = 0; k < 3; ++k) {
            float kd = in.Kd[k];
            kd = kd < 0 ? 0 : (kd > 1 ? 1 : kd);  // DiffuseMaterial clamps reflectance to [0,1]
            q.Kd[k] = kd;
            q.Le[k] = in.Le[k];
            lobes = lobes || kd != 0;
            light = light || in.Le[k] != 0;
        }
        q.two_sided = in.two_sided;
        q.is_light = light;
        q.has_lobes = lobes;
        q.flags = surf_flags_of(in.material, in.medium_interface);
        frame = isect_rec_build(&D->irec[i], q.n, q.p00, q.e1, q.e2, q.inv_l1, q.inv_l2, frame);
        if (light) D->light_quads[D->n_lights++] = i;
    }
    rect_twins_mark(D->irec, D->n_quads);
    rect_planes_build(&D->planes, D->irec, D->n_quads);
    D->n_inf = sc.n_infinite_lights;
    for (int i = 0; i < sc.n_infinite_lights && i < VSPG_MAX_INFINITE_LIGHTS; ++i) {
        D->inf_type[i] = sc.infinite_lights[i].type;
        for (int k = 0; k < 3; ++k) { D->inf_L[i][k] = sc.infinite_lights[i].L[k]; D->inf_w[i][k] = sc.infinite_lights[i].w_light[k]; }
        if (D->inf_type[i] == VSPG_LIGHT_IMAGE_INFINITE) {  // the 1 x 1 white image under the identity; vspg_renderer_create uploads its tables
            DEnvLight &E = D->env[i];
            E.res = 1;
            for (int k = 0; k < 3; ++k) { E.m[4 * k] = E.mi[4 * k] = 1.f; E.sum_L[k] = 1.f; }
        }
    }
    // point and spot lights (vspg_pointlight.h): what the constructors and SampleLi's first line derive from the transform
    D->n_point = sc.n_point_lights;
    for (int i = 0; i < sc.n_point_lights && i < VSPG_MAX_POINT_LIGHTS; ++i) {
        const VspgPointLight &in = sc.point_lights[i];
        DPointLight &P = D->point[i];
        P.type = in.type;
        const float *m = in.render_from_light;
        // renderFromLight(Point3f(0, 0, 0)), Transform::operator()(Point3f) (transform.h:310-319): the sums as written, then `wp == 1`
        float q[4];
        for (int k = 0; k < 4; ++k) {
            volatile float a = m[4 * k] * 0.f;  // volatile: one rounding per operation, no contraction
            volatile float b = m[4 * k + 1] * 0.f;
            volatile float c2 = m[4 * k + 2] * 0.f;
            volatile float sum = a + b;
            sum = sum + c2;
            sum = sum + m[4 * k + 3];
            q[k] = sum;
        }
        for (int k = 0; k < 3; ++k) P.pos[k] = q[3] == 1 ? q[k] : q[k] / q[3];
        for (int k = 0; k < 3; ++k) P.I[k] = in.I[k];
        for (int k = 0; k < 12; ++k) P.mi[k] = in.light_from_render[k];
        P.cosFalloffEnd = P.cosFalloffStart = 0.f;
        P.axis[0] = P.axis[1] = 0.f; P.axis[2] = 1.f;
        if (in.type == VSPG_LIGHT_PROJECTION || in.type == VSPG_LIGHT_GONIOMETRIC) {
            // the 1 x 1 image of ones (include/vspg.h): the light is valid from creation on; vspg_renderer_create uploads the texel
            const float ones[3] = {1.f, 1.f, 1.f};
            ImageLightTables T;
            image_light_build(in.type, ones, 1, 1, in.cone_angle_deg, &T);
            image_light_apply(T, &D->image_light[i]);
        }
        if (in.type == VSPG_LIGHT_SPOT) {
            // the constructor's cosines (lights.cpp:1438-1439): totalWidth = coneangle, falloffStart = coneangle - conedelta; Radians (math.h:261-263)
            volatile float start_deg = in.cone_angle_deg - in.cone_delta_deg;
            const float deg2rad = 3.14159265358979323846f / 180;
            volatile float rad_end = deg2rad * in.cone_angle_deg, rad_start = deg2rad * start_deg;
            P.cosFalloffEnd = std::cos((float)rad_end);
            P.cosFalloffStart = std::cos((float)rad_start);
        }
        if (in.type == VSPG_LIGHT_SPOT || in.type == VSPG_LIGHT_PROJECTION) {
            // Normalize(renderFromLight(Vector3f(0, 0, 1))) (transform.h:351-356), the w of SpotLight::Bounds and of ProjectionLight::Bounds (lights.cpp:439)
            float w[3];
            for (int k = 0; k < 3; ++k) {
                volatile float a = m[4 * k] * 0.f;
                volatile float b = m[4 * k + 1] * 0.f;
                volatile float c2 = m[4 * k + 2] * 1.f;
                volatile float sum = a + b;
                sum = sum + c2;
                w[k] = sum;
            }
            stv(P.axis, normv(H3{w[0], w[1], w[2]}));
        }
    }
    {   // scene bounds = union of the primitives' bounds; light.Preprocess: BoundingSphere (integrators.h:74-81, vecmath.h:1335-1338)
        float lo[3] = {kInf, kInf, kInf}, hi[3] = {-kInf, -kInf, -kInf};
        auto grow = [&](const float *q) { for (int k = 0; k < 3; ++k) { lo[k] = q[k] < lo[k] ? q[k] : lo[k]; hi[k] = q[k] > hi[k] ? q[k] : hi[k]; } };
        for (int i = 0; i < D->n_quads; ++i) { grow(D->quads[i].p00); grow(D->quads[i].p10); grow(D->quads[i].p01); grow(D->quads[i].p11); }
        for (int i = 0; i < sc.n_triangles && sc.tri_p; ++i) {
            DTri T;
            if (derive_triangle(sc.tri_p + 9 * (size_t)i, nullptr, i, &T)) { grow(T.p0); grow(T.p1); grow(T.p2); }
        }
        for (int i = 0; i < sc.n_spheres; ++i) {  // Sphere::Bounds (shapes.cpp:33-36): the corners of the object-space box, transformed
            const float *m = sc.spheres[i].render_from_object, rr = sc.spheres[i].radius;
            for (int c = 0; c < 8; ++c) {
                const float x = (c & 1) ? rr : -rr, y = (c & 2) ? rr : -rr, z = (c & 4) ? rr : -rr;
                float q[3];
                for (int k = 0; k < 3; ++k) {
                    volatile float a = m[4 * k] * x;  // volatile: one rounding per operation, as the oracle's -ffp-contract=off build
                    volatile float b = m[4 * k + 1] * y;
                    volatile float c2 = m[4 * k + 2] * z;
                    volatile float sum = a + b;
                    sum = sum + c2;
                    sum = sum + m[4 * k + 3];
                    q[k] = sum;
                }
                grow(q);
            }
        }
        D->scene_radius = 0.f;
        if (lo[0] <= hi[0]) {
            volatile float cx = (lo[0] + hi[0]) / 2, cy = (lo[1] + hi[1]) / 2, cz = (lo[2] + hi[2]) / 2;
            volatile float dx = cx - hi[0], dy = cy - hi[1], dz = cz - hi[2];
            volatile float l2 = dx * dx;
            l2 = l2 + dy * dy;
            l2 = l2 + dz * dz;
            D->scene_radius = std::sqrt(l2);
        }
    }
    // Shape "sphere": the constants the Sphere constructor derives (shapes.h:117-128), full sphere
    D->n_spheres = sc.n_spheres;
    for (int i = 0; i < sc.n_spheres; ++i) {
        const VspgSphere &in = sc.spheres[i];
        DSphere &sp = D->spheres[i];
        for (int k = 0; k < 12; ++k) { sp.m[k] = in.render_from_object[k]; sp.mi[k] = in.object_from_render[k]; }
        sp.radius = in.radius;
        const float *m = in.render_from_object;  // Transform::SwapsHandedness: Determinant(SquareMatrix<3>) < 0 (transform.cpp:145-152, math.h:1419-1425)
        const float minor12 = dop(m[5], m[10], m[6], m[9]), minor02 = dop(m[4], m[10], m[6], m[8]), minor01 = dop(m[4], m[9], m[5], m[8]);
        const bool swaps = std::fmaf(m[2], minor01, dop(m[0], minor12, m[1], minor02)) < 0;
        sp.flip = (in.reverse_orientation ? 1 : 0) ^ (swaps ? 1 : 0);
        auto clamp1 = [](float v) { return v < -1.f ? -1.f : (v > 1.f ? 1.f : v); };
        sp.thetaZMin = std::acos(clamp1(-in.radius / in.radius));  // zMin = -radius, zMax = radius (the "sphere" defaults, shapes.cpp:231-237)
        sp.thetaZMax = std::acos(clamp1(in.radius / in.radius));
        {
            volatile float rad = 3.14159265358979323846f / 180;  // Radians(360) (math.h:261-263) == fl(2 pi): no phi clipping
            rad = rad * 360.f;
            sp.phiMax = rad;
        }
        bool lobes = false;
        for (int k = 0; k < 3; ++k) {
            float kd = in.Kd[k];
            kd = kd < 0 ? 0 : (kd > 1 ? 1 : kd);
            sp.Kd[k] = kd;
            lobes = lobes || kd != 0;
        }
        sp.has_lobes = lobes;
        sp.flags = surf_flags_of(in.material, in.medium_interface);
    }
    // DiffuseAreaLight on a sphere (vspg_spherelight.h): the emissive spheres, in sphere order, are the last range of the light list
    D->n_sphere_lights = 0;
    for (int i = 0; i < VSPG_MAX_SPHERES; ++i) {
        DSphereLight &E = D->sphere_light[i];
        std::memset(&E, 0, sizeof E);
        E.light = -1;
        D->light_spheres[i] = 0;
    }
    for (int i = 0; i < sc.n_spheres; ++i) {
        const VspgSphere &in = sc.spheres[i];
        DSphereLight &E = D->sphere_light[i];
        for (int k = 0; k < 3; ++k) E.Le[k] = sc.sphere_Le[i][k];
        E.two_sided = sc.sphere_two_sided[i] ? 1 : 0;
        E.reverse = in.reverse_orientation ? 1 : 0;
        {   // Area() = phiMax * radius * (zMax - zMin) (shapes.h:131), zMin = -radius, zMax = radius: object space
            volatile float dz = in.radius - (-in.radius);  // volatile: one rounding per operation, no contraction
            volatile float a = D->spheres[i].phiMax * in.radius;
            a = a * dz;
            E.inv_area = 1 / a;
        }
        // renderFromObject(Point3f(0, 0, 0)), Transform::operator()(Point3f) (transform.h:310-319): the sums as written, then `wp == 1`
        const float *m = in.render_from_object;
        float q[4];
        for (int k = 0; k < 4; ++k) {
            volatile float a = m[4 * k] * 0.f;
            volatile float b = m[4 * k + 1] * 0.f;
            volatile float c2 = m[4 * k + 2] * 0.f;
            volatile float sum = a + b;
            sum = sum + c2;
            sum = sum + m[4 * k + 3];
            q[k] = sum;
        }
        for (int k = 0; k < 3; ++k) E.center[k] = q[3] == 1 ? q[k] : q[k] / q[3];
        if (E.Le[0] != 0 || E.Le[1] != 0 || E.Le[2] != 0) {
            E.light = D->n_lights + D->n_inf + D->n_point + D->n_sphere_lights;
            D->light_spheres[D->n_sphere_lights++] = i;
        }
    }
    // medium boundaries: anything that makes "the medium fills the scene" false
    D->camera_in_medium = sc.medium.type != VSPG_MEDIUM_NONE && !sc.camera_outside_medium;
    D->has_boundaries = sc.camera_outside_medium != 0;
    for (int i = 0; i < D->n_quads; ++i) D->has_boundaries |= D->quads[i].flags != 0;
    for (int i = 0; i < D->n_spheres; ++i) D->has_boundaries |= D->spheres[i].flags != 0;
    for (int i = 0; i < sc.n_triangles && sc.tri_flags; ++i)
        D->has_boundaries |= surf_flags_of(sc.tri_flags[i] & VSPG_TRI_INTERFACE, sc.tri_flags[i] >> VSPG_TRI_IFACE_SHIFT) != 0;
    D->cam = sc.camera;
    D->medium_type = sc.medium.type;
    for (int k = 0; k < 3; ++k) {
        D->sigma_a[k] = sc.medium.sigma_a[k];
        D->sigma_s[k] = sc.medium.sigma_s[k];
        {
            volatile float st = D->sigma_s[k] + D->sigma_a[k];  // volatile: one rounding per operation, no contraction
            volatile float sn = st - D->sigma_a[k];
            sn = sn - D->sigma_s[k];
            D->sigma_t[k] = st;
            D->sigma_n_raw[k] = sn;
        }
        D->Le[k] = sc.medium.Le[k];
    }
    D->g = sc.medium.g;
    for (int k = 0; k < 3; ++k) {
        D->index_min[k] = sc.medium.index_min[k];
        D->inv_voxel[k] = sc.medium.type == VSPG_MEDIUM_NANOVDB ? 1.0f / sc.medium.voxel_size[k] : 0.f;
        D->grid_origin[k] = sc.medium.grid_origin[k];
    }
    D->density_offset = sc.medium.density_offset;
    D->has_xform = sc.medium.has_transform ? 1 : 0;
    for (int k = 0; k < 12; ++k) D->minv[k] = sc.medium.has_transform ? sc.medium.medium_from_render[k] : ((k % 5) == 0 ? 1.f : 0.f);
    D->nx = sc.medium.nx;
    D->ny = sc.medium.ny;
    D->nz = sc.medium.nz;
    for (int k = 0; k < 3; ++k) {
        D->bounds_min[k] = sc.medium.bounds_min[k];
        D->bounds_max[k] = sc.medium.bounds_max[k];
    }
    D->prm = prm;
    D->xres = cfg.xres;
    D->yres = cfg.yres;
    D->seed = cfg.seed;
    D->shard_index = cfg.shard_index;
    D->shard_count = cfg.shard_count < 1 ? 1 : cfg.shard_count;
    // RGB grid medium: the scales; create points the grids at their device storage
    D->rgb_oct_a = D->rgb_oct_s = nullptr;
    D->rgb_Le = nullptr;
    D->rgb_sigma_scale = sc.medium.type == VSPG_MEDIUM_RGBGRID ? sc.rgb_sigma_scale : 0.f;
    D->rgb_le_scale = sc.medium.type == VSPG_MEDIUM_RGBGRID ? sc.rgb_le_scale : 0.f;
    lsb::build(sc, prm, D);  // LightSampler::Create(prm.lightsampler, lights) (lightsamplers.cpp:49-64)
}

// The voxel box of a majorant cell separates per axis: ranges[axis * R + c] = {lo, hi} of cell coordinate c, in ARRAY coordinates
// (the NANOVDB index range minus index_min), clipped to the grid; hi < lo is an empty range.  Both host builders below and the device
// builder (k_majorant_build, vspg_renderer_update_grid) read these tables, so the three agree on every box.
//   GRID:    SampledGrid::MaxValue(VoxelBounds(x,y,z)) (media.cpp:262-269, containers.h:838-854)
//   NANOVDB: "Initialize majorantGrid" (media.cpp:600-671): the cell's world bounds to index space (float Lerp, double division),
//            widened by one voxel (the trilinear filter slop), truncated, clipped to the index bounding box
int majorant_res(const VspgMedium &m) { return m.type == VSPG_MEDIUM_NANOVDB ? kMajResNvdb : kMajRes; }
std::vector<int2> majorant_axis_ranges(const VspgMedium &m) {
    const int R = majorant_res(m);
    const int n[3] = {m.nx, m.ny, m.nz};
    std::vector<int2> ranges((size_t)3 * R);
    auto lerp = [](float t, float a, float b) { return (1 - t) * a + t * b; };  // pbrt::Lerp (math.h)
    for (int k = 0; k < 3; ++k)
        for (int c = 0; c < R; ++c) {
            int lo, hi;
            if (m.type == VSPG_MEDIUM_NANOVDB) {
                const int imin = m.index_min[k], imax = m.index_min[k] + n[k] - 1;
                const float w0 = lerp((float)c / R, m.bounds_min[k], m.bounds_max[k]);
                const float w1 = lerp((float)(c + 1) / R, m.bounds_min[k], m.bounds_max[k]);
                const double i0 = ((double)w0 - (double)m.grid_origin[k]) / (double)m.voxel_size[k];  // worldToIndexF(Vec3R)
                const double i1 = ((double)w1 - (double)m.grid_origin[k]) / (double)m.voxel_size[k];
                const float delta = 1.f;
                lo = std::max((int)(i0 - delta), imin) - imin;
                hi = std::min((int)(i1 + delta), imax) - imin;
            } else {
                float p0 = (float)c / R, p1 = (float)(c + 1) / R;
                int a = (int)std::floor(p0 * n[k] - .5f), b = (int)std::floor(p1 * n[k] - .5f) + 1;
                lo = std::max(a, 0);
                hi = std::min(b, n[k] - 1);
            }
            ranges[(size_t)k * R + c] = make_int2(lo, hi);
        }
    return ranges;
}

// GridMedium constructor: majorantGrid.Set(x,y,z, densityGrid.MaxValue(VoxelBounds(x,y,z)))
// (src/pbrt/media.cpp:262-269; SampledGrid::MaxValue src/pbrt/util/containers.h:838-854)
std::vector<float> build_majorant_grid(const VspgMedium &m) {
    const int R = kMajRes;
    std::vector<float> maj((size_t)R * R * R);
    const std::vector<int2> ranges = majorant_axis_ranges(m);
    auto at = [&](int x, int y, int z) -> float {
        if (x < 0 || y < 0 || z < 0 || x >= m.nx || y >= m.ny || z >= m.nz) return 0.f;
        return m.density[((size_t)z * m.ny + y) * m.nx + x];
    };
    for (int z = 0; z < R; ++z)
        for (int y = 0; y < R; ++y)
            for (int x = 0; x < R; ++x) {
                const int2 rx = ranges[x], ry = ranges[R + y], rz = ranges[2 * R + z];
                float mx = at(rx.x, ry.x, rz.x);
                for (int zz = rz.x; zz <= rz.y; ++zz)
                    for (int yy = ry.x; yy <= ry.y; ++yy)
                        for (int xx = rx.x; xx <= rx.y; ++xx) mx = std::max(mx, at(xx, yy, zz));
                maj[x + R * (y + R * z)] = mx;
            }
    return maj;
}

// ---- f1: BVH over the triangle soup (own builder: binned SAH on centroids, leaves of <= 4 triangles, depth-first
// layout with skip links -- see DBvhNode).  cpu/aggregates.cpp:529-640 is what it stands in for; WHICH triangles a ray
// tests never changes a result (vspg_device.h: bvh_closest), so the builder is free.
namespace bvhbuild {
// the binary tree the builder grows first, depth-first: an inner node's first child is the next node, `skip` is the index behind
// its subtree (so its second child sits at nodes[first child].skip)
struct DBvhNode {
    float bmin[3];
    int32_t skip;
    float bmax[3];
    int32_t leaf;    // >= 0: first triangle * 8 + count (1..7); -1: inner node
};
struct Box { float lo[3], hi[3]; };
static Box empty_box() { return Box{{kInf, kInf, kInf}, {-kInf, -kInf, -kInf}}; }
static void grow(Box &b, const float *p) { for (int k = 0; k < 3; ++k) { b.lo[k] = std::min(b.lo[k], p[k]); b.hi[k] = std::max(b.hi[k], p[k]); } }
static void merge(Box &b, const Box &o) { for (int k = 0; k < 3; ++k) { b.lo[k] = std::min(b.lo[k], o.lo[k]); b.hi[k] = std::max(b.hi[k], o.hi[k]); } }
static float area(const Box &b) {
    const float dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
    return dx < 0 ? 0.f : 2 * (dx * dy + dy * dz + dz * dx);
}
struct Builder {
    const float *p = nullptr;       // 9 floats per triangle
    std::vector<int> order;         // triangle indices, permuted in place
    std::vector<Box> tbox;
    std::vector<float> cen;         // 3 per triangle
    std::vector<DBvhNode> nodes;
    std::vector<signed char> split_axis;   // per node: the axis its children were separated along (inner nodes)
    // The device tree (DBvh4Node): an inner node takes its two children and, while it holds fewer than four, replaces the inner child
    // of the largest surface area by that child's two children.  Returns the node's index; *depth: levels below and including it.
    bool balanced = false;          // median splits only: the fallback that bounds the depth for the traversal's stack
    std::vector<DBvh4Node> nodes4;
    int collapse(int node, int *depth) {
        const int me = (int)nodes4.size();
        nodes4.push_back(DBvh4Node{});
        int kids[4], nk = 0;
        if (nodes[node].leaf >= 0) {
            kids[nk++] = node;  // (a soup that fits one leaf: a root with one child)
        } else {
            kids[nk++] = node + 1;
            kids[nk++] = nodes[node + 1].skip;
            while (nk < 4) {
                int pick = -1;
                float pa = -1.f;
                for (int k = 0; k < nk; ++k)
                    if (nodes[kids[k]].leaf < 0) {
                        const Box b{{nodes[kids[k]].bmin[0], nodes[kids[k]].bmin[1], nodes[kids[k]].bmin[2]}, {nodes[kids[k]].bmax[0], nodes[kids[k]].bmax[1], nodes[kids[k]].bmax[2]}};
                        const float ar = area(b);
                        if (ar > pa) { pa = ar; pick = k; }
                    }
                if (pick < 0) break;
                const int c = kids[pick];
                kids[pick] = c + 1;
                kids[nk++] = nodes[c + 1].skip;
            }
        }
        int dmax = 0;
        for (int k = 0; k < 4; ++k) {
            DBvh4Node &N = nodes4[me];  // (re-taken every round: the recursion below grows the vector)
            if (k >= nk) {
                N.lox[k] = N.loy[k] = N.loz[k] = kInf; N.hix[k] = N.hiy[k] = N.hiz[k] = -kInf;
                N.child[k] = kBvhAbsent;
                continue;
            }
            const DBvhNode &c = nodes[kids[k]];
            N.lox[k] = c.bmin[0]; N.loy[k] = c.bmin[1]; N.loz[k] = c.bmin[2];
            N.hix[k] = c.bmax[0]; N.hiy[k] = c.bmax[1]; N.hiz[k] = c.bmax[2];
            if (c.leaf >= 0) {
                N.child[k] = -c.leaf - 1;
            } else {
                int dk = 0;
                const int idx = collapse(kids[k], &dk);
                nodes4[me].child[k] = idx;
                dmax = dk > dmax ? dk : dmax;
            }
        }
        for (int k = 0; k < 4; ++k) nodes4[me].pad[k] = 0;
        *depth = dmax + 1;
        return me;
    }
#ifndef VSPG_BVH_LEAF
#define VSPG_BVH_LEAF 2
#endif
    // a range of at most this many triangles is not split further (a leaf holds <= 7).  Measured (scripts/tri_timing.py, fog box + 100 k
    // triangles, ms per 1080p wave): 6: 8.0, 4: 7.4, 2: 6.4, 1: 6.5 -- the watertight triangle test is the expensive part of a visit
    static constexpr int kLeafMax = VSPG_BVH_LEAF;
    int bin_of(int t, int ax, float lo_a, float ext, int nb) const {
        const int k = (int)(nb * ((cen[3 * t + ax] - lo_a) / ext));
        return k < 0 ? 0 : (k >= nb ? nb - 1 : k);
    }
    void build(int lo, int hi) {
        const int me = (int)nodes.size();
        nodes.push_back(DBvhNode{});
        split_axis.push_back(0);
        Box b = empty_box(), cb = empty_box();
        for (int i = lo; i < hi; ++i) { merge(b, tbox[order[i]]); grow(cb, &cen[3 * order[i]]); }
        for (int k = 0; k < 3; ++k) { nodes[me].bmin[k] = b.lo[k]; nodes[me].bmax[k] = b.hi[k]; }
        const int n = hi - lo;
        int axis = 0;
        for (int k = 1; k < 3; ++k) if (cb.hi[k] - cb.lo[k] > cb.hi[axis] - cb.lo[axis]) axis = k;
        int mid = -1;
        if (n > kLeafMax && !balanced) {  // binned SAH over all three axes: the cheapest of the 3 x (NB - 1) candidate planes
            constexpr int NB = 16;
            float best = kInf; int bs = -1, baxis = -1;
            for (int ax = 0; ax < 3; ++ax) {
                const float ext = cb.hi[ax] - cb.lo[ax];
                if (!(ext > 0)) continue;
                Box bb[NB]; int cnt[NB];
                for (int i = 0; i < NB; ++i) { bb[i] = empty_box(); cnt[i] = 0; }
                for (int i = lo; i < hi; ++i) { const int k = bin_of(order[i], ax, cb.lo[ax], ext, NB); cnt[k]++; merge(bb[k], tbox[order[i]]); }
                for (int s = 0; s < NB - 1; ++s) {
                    Box l = empty_box(), rr = empty_box(); int nl = 0, nr = 0;
                    for (int i = 0; i <= s; ++i) { merge(l, bb[i]); nl += cnt[i]; }
                    for (int i = s + 1; i < NB; ++i) { merge(rr, bb[i]); nr += cnt[i]; }
                    if (!nl || !nr) continue;
                    const float c = nl * area(l) + nr * area(rr);
                    if (c < best) { best = c; bs = s; baxis = ax; }
                }
            }
            if (bs >= 0) {
                axis = baxis;
                const float lo_a = cb.lo[axis], ext = cb.hi[axis] - cb.lo[axis];
                auto it = std::partition(order.begin() + lo, order.begin() + hi, [&](int t) { return bin_of(t, axis, lo_a, ext, NB) <= bs; });
                mid = (int)(it - order.begin());
            }
        }
        if ((n > 7 || (balanced && n > kLeafMax)) && (mid <= lo || mid >= hi)) {  // no useful split but too many for a leaf (or the balanced fallback): median by index
            mid = lo + n / 2;
            std::nth_element(order.begin() + lo, order.begin() + mid, order.begin() + hi,
                             [&](int a, int c) { return cen[3 * a + axis] < cen[3 * c + axis]; });
        }
        if (mid > lo && mid < hi) {
            nodes[me].leaf = -1;
            split_axis[me] = (signed char)axis;
            build(lo, mid);
            build(mid, hi);
        } else {
            nodes[me].leaf = lo * 8 + n;  // n <= 7
        }
        nodes[me].skip = (int)nodes.size();
    }
};
}  // namespace bvhbuild

// what Triangle::InteractionFromIntersection derives from the vertices alone (shapes.h:888-938), same float operations
bool derive_triangle(const float *p9, const float *kd, int id, DTri *T, const int32_t *flags, const int32_t *tex) {
    using namespace hostmath;
    const H3 p0 = ld(p9), p1 = ld(p9 + 3), p2 = ld(p9 + 6);
    auto sub = [](H3 a, H3 b) { return H3{a.x - b.x, a.y - b.y, a.z - b.z}; };
    if (len2v(crossv(sub(p2, p0), sub(p1, p0))) == 0) return false;  // IntersectTriangle: degenerate -> never hit (shapes.cpp:172-173)
    const H3 dp02 = sub(p0, p2), dp12 = sub(p1, p2);
    // default (u,v) = (0,0), (1,0), (1,1): duv02 = (-1,-1), duv12 = (0,-1)
    const float duv02[2] = {0.f - 1.f, 0.f - 1.f}, duv12[2] = {1.f - 1.f, 0.f - 1.f};
    const float determinant = dop(duv02[0], duv12[1], duv02[1], duv12[0]);
    H3 dpdu{0, 0, 0}, dpdv{0, 0, 0};
    const bool degenerateUV = std::fabs(determinant) < 1e-9f;
    if (!degenerateUV) {
        const float invdet = 1 / determinant;
        dpdu = H3{dop(duv12[1], dp02.x, duv02[1], dp12.x) * invdet, dop(duv12[1], dp02.y, duv02[1], dp12.y) * invdet, dop(duv12[1], dp02.z, duv02[1], dp12.z) * invdet};
        dpdv = H3{dop(duv02[0], dp12.x, duv12[0], dp02.x) * invdet, dop(duv02[0], dp12.y, duv12[0], dp02.y) * invdet, dop(duv02[0], dp12.z, duv12[0], dp02.z) * invdet};
    }
    if (degenerateUV || len2v(crossv(dpdu, dpdv)) == 0) return false;  // (the reference falls back to CoordinateSystem(ng); such slivers are dropped here)
    const H3 n = normv(crossv(dp02, dp12));
    memset(T, 0, sizeof *T);
    stv(T->p0, p0); stv(T->p1, p1); stv(T->p2, p2);
    T->nx = n.x; T->ny = n.y; T->nz = n.z;
    stv(T->dpdu_n, normv(dpdu));
    T->id = id;
    for (int k = 0; k < 3; ++k) { float v = kd ? kd[3 * id + k] : 0.5f; T->Kd[k] = v < 0 ? 0 : (v > 1 ? 1 : v); }
    const int fl = flags ? flags[id] : 0;
    T->flags = surf_flags_of(fl & VSPG_TRI_INTERFACE, fl >> VSPG_TRI_IFACE_SHIFT);
    if (tex && tex[id] > 0) T->flags |= tex[id] << TRI_TEX_SHIFT;  // (validate_textures: 1 .. n_textures, never on an interface triangle)
    if (fl & VSPG_TRI_FLIP_NORMAL) { T->nx = -T->nx; T->ny = -T->ny; T->nz = -T->nz; }  // reverseOrientation ^ transformSwapsHandedness (shapes.h:934-936)
    return true;
}

// The soup as the device reads it: derive the triangles, build the binary tree and collapse it to four-wide nodes, fall back to
// median splits when that tree is too deep for the traversal's stack, then put the triangles in the final tree's leaf order.
int build_triangle_bvh(const VspgScene &sc, std::vector<DTri> *tris, std::vector<DBvh4Node> *nodes4, const int32_t *tri_texture) {
    tris->clear();
    nodes4->clear();
    std::vector<DTri> all;
    all.reserve(sc.n_triangles);
    for (int i = 0; i < sc.n_triangles; ++i) {
        DTri T;
        if (derive_triangle(sc.tri_p + 9 * (size_t)i, sc.tri_kd, i, &T, sc.tri_flags, tri_texture)) all.push_back(T);
    }
    if (all.empty()) return 0;
    bvhbuild::Builder B;
    B.order.resize(all.size());
    B.tbox.resize(all.size());
    B.cen.resize(3 * all.size());
    for (size_t i = 0; i < all.size(); ++i) {
        B.order[i] = (int)i;
        bvhbuild::Box b = bvhbuild::empty_box();
        bvhbuild::grow(b, all[i].p0); bvhbuild::grow(b, all[i].p1); bvhbuild::grow(b, all[i].p2);
        B.tbox[i] = b;
        for (int k = 0; k < 3; ++k) B.cen[3 * i + k] = 0.5f * (b.lo[k] + b.hi[k]);
    }
    B.nodes.reserve(2 * all.size());
    B.build(0, (int)all.size());
    int depth4 = 0;
    B.collapse(0, &depth4);
    if (3 * depth4 + 1 > kBvhStack) {  // a degenerate soup made the SAH tree too deep for the traversal's stack: median splits
        bvhbuild::Builder B2;
        B2.balanced = true;
        B2.p = B.p; B2.tbox = B.tbox; B2.cen = B.cen;
        B2.order.resize(all.size());
        for (size_t i = 0; i < all.size(); ++i) B2.order[i] = (int)i;
        B2.nodes.reserve(2 * all.size());
        B2.build(0, (int)all.size());
        B2.collapse(0, &depth4);
        if (3 * depth4 + 1 > kBvhStack) return fail(VSPG_ESCOPE, "triangle soup too large for the BVH traversal's stack");
        B.order = B2.order;
        B.nodes4 = B2.nodes4;
    }
    tris->resize(all.size());
    for (size_t i = 0; i < all.size(); ++i) (*tris)[i] = all[B.order[i]];
    *nodes4 = B.nodes4;
    return 0;
}

// ---- image textures on diffuse reflectance (vspg_texture.h; include/vspg.h VspgTexture) ----
static bool power_of_two(int v) { return v > 0 && (v & (v - 1)) == 0; }
int texture_image_refusal(const float *pixels, int xres, int yres, int channels) {
    if (!pixels) return fail(VSPG_EINVAL, "a texture without an image (null pixels)");
    if (xres < 1 || xres > VSPG_TEXTURE_MAX_RES || yres < 1 || yres > VSPG_TEXTURE_MAX_RES)
        return fail(VSPG_EINVAL, "texture resolution outside 1 .. VSPG_TEXTURE_MAX_RES (4096)");
    if (channels != 1 && channels != 3) return fail(VSPG_EINVAL, "a texture image has 1 or 3 channels");
    if (!power_of_two(xres) || !power_of_two(yres))
        return fail(VSPG_ESCOPE, "texture resolution is not a power of two: the reference resamples such an image before level 0 exists, and that resampling is not built");
    const size_t n = (size_t)xres * yres * channels;
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(pixels[i])) return fail(VSPG_EINVAL, "a texture image holds a texel that is not-a-number or infinite");
    return 0;
}
int validate_textures(const VspgScene &sc, const VspgSceneTextures &tx) {
    if (tx.n_textures < 0 || tx.n_textures > VSPG_MAX_TEXTURES) return fail(VSPG_EINVAL, "n_textures out of range");
    for (int k = 0; k < tx.n_textures; ++k) {
        const VspgTexture &t = tx.textures[k];
        if (t.wrap != VSPG_TEXWRAP_REPEAT && t.wrap != VSPG_TEXWRAP_CLAMP && t.wrap != VSPG_TEXWRAP_BLACK) return fail(VSPG_EINVAL, "unknown texture wrap mode");
        if (t.filter != VSPG_TEXFILTER_POINT && t.filter != VSPG_TEXFILTER_BILINEAR) return fail(VSPG_EINVAL, "unknown texture filter");
        if (t.invert != 0 && t.invert != 1) return fail(VSPG_EINVAL, "a texture's invert must be 0 or 1");
        const float prm[5] = {t.scale, t.su, t.sv, t.du, t.dv};
        for (int j = 0; j < 5; ++j)
            if (!std::isfinite(prm[j])) return fail(VSPG_EINVAL, "a texture's scale, uscale, vscale, udelta or vdelta is not finite");
        if (const int rc = texture_image_refusal(t.pixels, t.xres, t.yres, t.channels)) return rc;
    }
    for (int i = 0; i < sc.n_quads && i < VSPG_MAX_QUADS; ++i) {
        const int k = tx.quad_texture[i];
        if (k < 0 || k > tx.n_textures) return fail(VSPG_EINVAL, "a rectangle's texture index names no texture of the scene");
        if (k != 0 && sc.quads[i].material == VSPG_MATERIAL_INTERFACE) return fail(VSPG_EINVAL, "a texture on a rectangle whose material is \"interface\"");
    }
    if (tx.tri_texture)
        for (int i = 0; i < sc.n_triangles; ++i) {
            const int k = tx.tri_texture[i];
            if (k < 0 || k > tx.n_textures) return fail(VSPG_EINVAL, "a triangle's texture index names no texture of the scene");
            if (k != 0 && sc.tri_flags && (sc.tri_flags[i] & VSPG_TRI_INTERFACE)) return fail(VSPG_EINVAL, "a texture on a triangle whose material is \"interface\"");
        }
    if (tx.tri_uv)
        for (size_t i = 0; i < 6 * (size_t)sc.n_triangles; ++i)
            if (!std::isfinite(tx.tri_uv[i])) return fail(VSPG_EINVAL, "a triangle's uv is not finite");
    return 0;
}
std::vector<float> texture_image_build(const float *pixels, int xres, int yres, int channels) {
    const size_t n = (size_t)xres * yres;
    std::vector<float> img(4 * n);
    for (size_t i = 0; i < n; ++i) {
        for (int c = 0; c < 3; ++c) img[4 * i + c] = channels == 3 ? pixels[3 * i + c] : pixels[i];
        img[4 * i + 3] = 0.f;
    }
    return img;
}
void texture_apply(const VspgTexture &in, DTexture *T) {
    T->xres = in.xres; T->yres = in.yres;
    T->wrap = in.wrap; T->filter = in.filter; T->invert = in.invert;
    T->scale = in.scale; T->su = in.su; T->sv = in.sv; T->du = in.du; T->dv = in.dv;
    T->pad = 0;
}
void apply_scene_textures(const VspgScene &sc, const VspgSceneTextures &tx, DScene *D) {
    for (int k = 0; k < tx.n_textures && k < VSPG_MAX_TEXTURES; ++k) texture_apply(tx.textures[k], &D->tex[k]);
    for (int i = 0; i < sc.n_quads && i < VSPG_MAX_QUADS; ++i) D->quad_tex[i] = tx.quad_texture[i];
}
int count_textured(const VspgScene &sc, const VspgSceneTextures &tx, const std::vector<DTri> &tris) {
    int n = 0;
    for (int i = 0; i < sc.n_quads && i < VSPG_MAX_QUADS; ++i) n += tx.quad_texture[i] != 0;
    for (const DTri &T : tris) n += (T.flags >> TRI_TEX_SHIFT) != 0;
    return n;
}
std::vector<float> build_tri_uv(const float *tri_uv, const std::vector<DTri> &tris) {
    bool any = false;
    for (const DTri &T : tris) any = any || (T.flags >> TRI_TEX_SHIFT) != 0;
    std::vector<float> uv;
    if (!any) return uv;
    static const float def[6] = {0.f, 0.f, 1.f, 0.f, 1.f, 1.f};  // Triangle::InteractionFromIntersection's default uv (shapes.h)
    uv.resize(6 * tris.size());
    for (size_t i = 0; i < tris.size(); ++i)
        for (int j = 0; j < 6; ++j) uv[6 * i + j] = tri_uv ? tri_uv[6 * (size_t)tris[i].id + j] : def[j];
    return uv;
}

bool wants_guiding(const VspgIntegratorParams &p) {
    return p.surfaceguiding || p.volumeguiding || (p.vspguiding && p.vspsecondaryguiding) || p.rrguiding;  // guided kernels
}
bool wants_training(const VspgIntegratorParams &p) {  // the field is queried
    return p.surfaceguiding || p.volumeguiding || (p.vspguiding && p.vspsecondaryguiding);
}

// NanoVDBMedium constructor, "Initialize majorantGrid" (media.cpp:600-671) over the dense copy: 64^3 cells; a
// cell's majorant is the largest voxel value in the cell's index-space footprint widened by one voxel (the
// trilinear filter slop), clipped to the index bounding box (majorant_axis_ranges), then (max + densityOffset) * majorantScale.
std::vector<float> build_majorant_grid_nvdb(const VspgMedium &m) {
    const int R = kMajResNvdb;
    std::vector<float> maj((size_t)R * R * R);
    const std::vector<int2> ranges = majorant_axis_ranges(m);
    auto value = [&](int x, int y, int z) -> float {  // accessor.getValue: background outside the tree (array coordinates)
        if (x < 0 || y < 0 || z < 0 || x >= m.nx || y >= m.ny || z >= m.nz) return 0.f;
        return m.density[((size_t)z * m.ny + y) * m.nx + x];
    };
    for (int z = 0; z < R; ++z)
        for (int y = 0; y < R; ++y)
            for (int x = 0; x < R; ++x) {
                const int2 rx = ranges[x], ry = ranges[R + y], rz = ranges[2 * R + z];
                float mx = 0;
                for (int kk = rz.x; kk <= rz.y; ++kk)
                    for (int jj = ry.x; jj <= ry.y; ++jj)
                        for (int ii = rx.x; ii <= rx.y; ++ii) mx = std::max(mx, value(ii, jj, kk));
                maj[x + R * (y + R * z)] = (mx + m.density_offset) * m.majorant_scale;
            }
    return maj;
}

// ---- RGBGridMedium ("rgbgrid", media.h:391-467): what create derives on the host -- the refusals, the majorants, the storage image.
// Create's error triggers (media.cpp:418-445) as far as they survive in a record of pointers: the sample counts are nx * ny * nz by
// contract, so what is left is "sigma_a and/or sigma_s" (:418-420) and "sigma_a if Le" (:433-434, the constructor's CHECK :386-387).
// the value check of one grid (HOST values), shared by create and vspg_renderer_update_rgb_grids: -0.0 passes (it is not < 0)
static const char *rgb_grid_name(int which) { return which == 0 ? "sigma_a" : which == 1 ? "sigma_s" : "Le"; }
int rgb_grid_value_refusal(int which) {
    return fail(VSPG_EINVAL, std::string("RGB grid medium: \"") + rgb_grid_name(which) + "\" holds a value that is negative or not finite");
}
int check_rgb_grid_values(const float *values, size_t n_floats, int which) {
    for (size_t i = 0; i < n_floats; ++i)
        if (!std::isfinite(values[i]) || values[i] < 0) return rgb_grid_value_refusal(which);
    return 0;
}
int validate_rgb_grid(const VspgScene &sc) {
    const VspgMedium &m = sc.medium;
    if (m.nx <= 0 || m.ny <= 0 || m.nz <= 0) return fail(VSPG_EINVAL, "RGB grid medium needs nx, ny, nz > 0");
    if ((long long)m.nx * m.ny * m.nz > (1ll << 31)) return fail(VSPG_EINVAL, "RGB grid too large");
    if (!sc.rgb_sigma_a && !sc.rgb_sigma_s) return fail(VSPG_EINVAL, "RGB grid requires \"sigma_a\" and/or \"sigma_s\" parameter values.");
    if (sc.rgb_Le && !sc.rgb_sigma_a) return fail(VSPG_EINVAL, "RGB grid requires \"sigma_a\" if \"Le\" value provided.");
    if (m.temperature) return fail(VSPG_EINVAL, "an RGB grid medium has no temperature grid");
    if (!std::isfinite(sc.rgb_sigma_scale) || !std::isfinite(sc.rgb_le_scale)) return fail(VSPG_EINVAL, "RGB grid medium: \"scale\" / \"Lescale\" is not finite");
    for (int k = 0; k < 3; ++k)
        if (!(m.bounds_max[k] > m.bounds_min[k])) return fail(VSPG_EINVAL, "grid medium bounds must have positive extent");
    if (m.has_transform) {
        const float *a = m.render_from_medium, *b = m.medium_from_render;
        if (a[12] != 0 || a[13] != 0 || a[14] != 0 || a[15] != 1 || b[12] != 0 || b[13] != 0 || b[14] != 0 || b[15] != 1)
            return fail(VSPG_EINVAL, "renderFromMedium must be affine (last row 0 0 0 1)");
        for (int k = 0; k < 16; ++k)
            if (!(a[k] == a[k]) || !(b[k] == b[k])) return fail(VSPG_EINVAL, "renderFromMedium holds a NaN");
    }
    const size_t n3 = (size_t)m.nx * m.ny * m.nz * 3;
    const float *grids[3] = {sc.rgb_sigma_a, sc.rgb_sigma_s, sc.rgb_Le};
    for (int gk = 0; gk < 3; ++gk)
        if (grids[gk])
            if (const int rc = check_rgb_grid_values(grids[gk], n3, gk)) return rc;
    return 0;
}

// RGBGridMedium constructor, "Initialize majorantGrid" (media.cpp:395-408): per cell sigmaScale * (MaxValue(sigma_a box, max) +
// MaxValue(sigma_s box, max)) with SampledGrid::MaxValue(bounds, convert) (containers.h:837-854) -- maxValue starts at Lookup(pi[0])
// and the box is GridMedium's (majorant_axis_ranges) -- convert = the largest of R, G, B; an absent grid counts as 1.
std::vector<float> build_majorant_grid_rgb(const VspgScene &sc) {
    const VspgMedium &m = sc.medium;
    const int R = kMajRes;
    std::vector<float> maj((size_t)R * R * R);
    const std::vector<int2> ranges = majorant_axis_ranges(m);
    auto at = [&](const float *g, int x, int y, int z) -> float {  // Lookup(Point3i, convert): RGB{} outside the grid
        if (x < 0 || y < 0 || z < 0 || x >= m.nx || y >= m.ny || z >= m.nz) return 0.f;
        const float *v = g + (((size_t)z * m.ny + y) * m.nx + x) * 3;
        return std::max(std::max(v[0], v[1]), v[2]);  // RGBUnboundedSpectrum::MaxValue in the RGB build
    };
    auto max_value = [&](const float *g, int2 rx, int2 ry, int2 rz) -> float {
        float mx = at(g, rx.x, ry.x, rz.x);
        for (int zz = rz.x; zz <= rz.y; ++zz)
            for (int yy = ry.x; yy <= ry.y; ++yy)
                for (int xx = rx.x; xx <= rx.y; ++xx) mx = std::max(mx, at(g, xx, yy, zz));
        return mx;
    };
    for (int z = 0; z < R; ++z)
        for (int y = 0; y < R; ++y)
            for (int x = 0; x < R; ++x) {
                const int2 rx = ranges[x], ry = ranges[R + y], rz = ranges[2 * R + z];
                const float ma = sc.rgb_sigma_a ? max_value(sc.rgb_sigma_a, rx, ry, rz) : 1.f;
                const float ms = sc.rgb_sigma_s ? max_value(sc.rgb_sigma_s, rx, ry, rz) : 1.f;
                volatile float sum = ma + ms;  // volatile: one rounding per operation, as the kernels' flags give
                maj[x + R * (y + R * z)] = sc.rgb_sigma_scale * sum;
            }
    return maj;
}

// The device image of one RGB grid (vspg_rgbgrid.h): per base voxel in [-1, n - 1]^3 its eight RGB corners as float4, in brick order;
// bn = (n + 8) / 8 bricks per axis, every brick stored, zeros outside the grid and in a brick's unused slots.
void rgb_brick_counts(const VspgMedium &m, int *bnx, int *bny, int *bnz) {
    *bnx = (m.nx + 1 + 7) / 8;
    *bny = (m.ny + 1 + 7) / 8;
    *bnz = (m.nz + 1 + 7) / 8;
}
std::vector<float> build_rgb_octets(const float *rgb, const VspgMedium &m) {
    int bnx, bny, bnz;
    rgb_brick_counts(m, &bnx, &bny, &bnz);
    std::vector<float> img((size_t)bnx * bny * bnz * 512u * 32u, 0.f);
    for (int oz = 0; oz <= m.nz; ++oz)
        for (int oy = 0; oy <= m.ny; ++oy)
            for (int ox = 0; ox <= m.nx; ++ox) {
                float *o = img.data() + rgb_octet_slot(ox, oy, oz, bnx, bny) * 32u;
                for (int c = 0; c < 8; ++c) {
                    const int x = ox - 1 + (c & 1), y = oy - 1 + ((c >> 1) & 1), z = oz - 1 + (c >> 2);
                    if (x < 0 || y < 0 || z < 0 || x >= m.nx || y >= m.ny || z >= m.nz) continue;
                    const float *v = rgb + (((size_t)z * m.ny + y) * m.nx + x) * 3;
                    o[4 * c] = v[0]; o[4 * c + 1] = v[1]; o[4 * c + 2] = v[2];
                }
            }
    return img;
}

int validate(const VspgScene *scene, const VspgIntegratorParams *p, const VspgRenderConfig *cfg) {
    if (!scene || !p || !cfg) return fail(VSPG_EINVAL, "null argument");
    if (cfg->xres <= 0 || cfg->yres <= 0) return fail(VSPG_EINVAL, "film resolution must be positive");
    if (cfg->xres > 32768 || cfg->yres > 32768) return fail(VSPG_EINVAL, "film resolution above 32768 (pixels travel as packed 16-bit pairs)");
    if (scene->n_quads < 0 || scene->n_quads > VSPG_MAX_QUADS) return fail(VSPG_EINVAL, "n_quads out of range");
    if (scene->n_spheres < 0 || scene->n_spheres > VSPG_MAX_SPHERES) return fail(VSPG_EINVAL, "n_spheres out of range");
    for (int i = 0; i < scene->n_spheres; ++i) {
        const VspgSphere &sp = scene->spheres[i];
        if (!(sp.radius > 0)) return fail(VSPG_EINVAL, "sphere radius must be positive");
        const float *a = sp.render_from_object, *b = sp.object_from_render;
        if (a[12] != 0 || a[13] != 0 || a[14] != 0 || a[15] != 1 || b[12] != 0 || b[13] != 0 || b[14] != 0 || b[15] != 1)
            return fail(VSPG_EINVAL, "a sphere's renderFromObject must be affine (last row 0 0 0 1)");
        const float *Le = scene->sphere_Le[i];
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(Le[k]) || Le[k] < 0) return fail(VSPG_EINVAL, "a sphere light's Le must be finite and >= 0");
        if (scene->sphere_two_sided[i] != 0 && scene->sphere_two_sided[i] != 1) return fail(VSPG_EINVAL, "a sphere light's two_sided must be 0 or 1");
        if ((Le[0] != 0 || Le[1] != 0 || Le[2] != 0) && sp.material == VSPG_MATERIAL_INTERFACE)
            return fail(VSPG_ESCOPE, "an emissive sphere with Material \"interface\": the reference allows it, this library does not (a shadow ray's end "
                                     "point would lie on a surface its segments walk through)");
    }
    if (cfg->shard_count > 1 && (cfg->shard_index < 0 || cfg->shard_index >= cfg->shard_count))
        return fail(VSPG_EINVAL, "shard_index out of range");
    if (p->maxdepth < 0) return fail(VSPG_EINVAL, "maxdepth must be >= 0");
    if (p->maxdepth > 254) return fail(VSPG_EINVAL, "maxdepth above 254 (the path depth travels in 8 bits of the packed path flags)");
    if (!(p->vspmisratio >= 0.f && p->vspmisratio <= 1.f)) return fail(VSPG_EINVAL, "vspmisratio must be in [0,1]");
    if (scene->medium.type == VSPG_MEDIUM_GRID || scene->medium.type == VSPG_MEDIUM_NANOVDB) {
        const VspgMedium &m = scene->medium;
        if (m.nx <= 0 || m.ny <= 0 || m.nz <= 0 || !m.density) return fail(VSPG_EINVAL, "grid medium needs nx,ny,nz > 0 and a density array");
        if (m.type == VSPG_MEDIUM_NANOVDB) {
            for (int k = 0; k < 3; ++k)
                if (!(m.voxel_size[k] > 0)) return fail(VSPG_EINVAL, "nanovdb medium needs a positive voxel_size");
            if (!(m.majorant_scale > 0)) return fail(VSPG_EINVAL, "nanovdb medium needs majorant_scale > 0 (reference default 1)");
        }
        if ((long long)m.nx * m.ny * m.nz > (1ll << 31)) return fail(VSPG_EINVAL, "density grid too large");
        for (int k = 0; k < 3; ++k)
            if (!(m.bounds_max[k] > m.bounds_min[k])) return fail(VSPG_EINVAL, "grid medium bounds must have positive extent");
        if (m.has_transform) {
            const float *a = m.render_from_medium, *b = m.medium_from_render;
            if (a[12] != 0 || a[13] != 0 || a[14] != 0 || a[15] != 1 || b[12] != 0 || b[13] != 0 || b[14] != 0 || b[15] != 1)
                return fail(VSPG_EINVAL, "renderFromMedium must be affine (last row 0 0 0 1)");
            for (int k = 0; k < 16; ++k)
                if (!(a[k] == a[k]) || !(b[k] == b[k])) return fail(VSPG_EINVAL, "renderFromMedium holds a NaN");
        }
        if (m.Le[0] != 0 || m.Le[1] != 0 || m.Le[2] != 0) {
            if (m.type == VSPG_MEDIUM_NANOVDB)
                return fail(VSPG_EINVAL, "NanoVDBMedium has no Le spectrum: it emits through its temperature grid (VspgMedium.temperature)");
            if (m.temperature) return fail(VSPG_EINVAL, "Both \"Le\" and \"temperature\" values were provided.");  // media.cpp:307-308
        }
        // temperature grids (media.h:333-341, :724-735): blackbody volume emission, sampled by the delta-tracking routine only
        // (guidedvolpathvspgintegrator.cpp:895-906) -- under "resampling" a heterogeneous medium never evaluates it
        if (m.type == VSPG_MEDIUM_GRID && (m.temperature || m.Le[0] != 0 || m.Le[1] != 0 || m.Le[2] != 0))
            if (m.le_scale && (m.le_nx <= 0 || m.le_ny <= 0 || m.le_nz <= 0 || (long long)m.le_nx * m.le_ny * m.le_nz > (1ll << 31)))
                return fail(VSPG_EINVAL, "emissive grid medium: bad Lescale grid size");
    } else if (scene->medium.type == VSPG_MEDIUM_RGBGRID) {
        if (const int rc = validate_rgb_grid(*scene)) return rc;
    } else if (scene->medium.type != VSPG_MEDIUM_NONE && scene->medium.type != VSPG_MEDIUM_HOMOGENEOUS)
        return fail(VSPG_EINVAL, "unknown medium type");
    if (scene->n_triangles < 0 || scene->n_triangles > (1 << 27)) return fail(VSPG_EINVAL, "n_triangles out of range");
    if (scene->n_triangles > 0 && !scene->tri_p) return fail(VSPG_EINVAL, "triangles without vertex data");
    if (scene->n_infinite_lights < 0 || scene->n_infinite_lights > VSPG_MAX_INFINITE_LIGHTS) return fail(VSPG_EINVAL, "n_infinite_lights out of range");
    for (int i = 0; i < scene->n_infinite_lights; ++i)
        if (scene->infinite_lights[i].type != VSPG_LIGHT_UNIFORM_INFINITE && scene->infinite_lights[i].type != VSPG_LIGHT_DISTANT &&
            scene->infinite_lights[i].type != VSPG_LIGHT_IMAGE_INFINITE)
            return fail(VSPG_EINVAL, "unknown infinite light type");
    if (scene->n_point_lights < 0 || scene->n_point_lights > VSPG_MAX_POINT_LIGHTS) return fail(VSPG_EINVAL, "n_point_lights out of range");
    for (int i = 0; i < scene->n_point_lights; ++i) {
        const VspgPointLight &pl = scene->point_lights[i];
        if (pl.type != VSPG_LIGHT_POINT && pl.type != VSPG_LIGHT_SPOT && pl.type != VSPG_LIGHT_PROJECTION && pl.type != VSPG_LIGHT_GONIOMETRIC)
            return fail(VSPG_EINVAL, "unknown point light type");
        const float *a = pl.render_from_light, *b = pl.light_from_render;
        for (int k = 0; k < 16; ++k)
            if (!std::isfinite(a[k]) || !std::isfinite(b[k])) return fail(VSPG_EINVAL, "a point light's renderFromLight is not finite");
        if (a[12] != 0 || a[13] != 0 || a[14] != 0 || a[15] != 1 || b[12] != 0 || b[13] != 0 || b[14] != 0 || b[15] != 1)
            return fail(VSPG_EINVAL, "a point light's renderFromLight must be affine (last row 0 0 0 1)");
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(pl.I[k])) return fail(VSPG_EINVAL, "a point light's I is not finite");
        if (pl.type == VSPG_LIGHT_SPOT) {
            if (!(pl.cone_angle_deg > 0 && pl.cone_angle_deg <= 180)) return fail(VSPG_EINVAL, "a spot light's cone_angle_deg must be in (0, 180]");
            if (!(pl.cone_delta_deg >= 0)) return fail(VSPG_EINVAL, "a spot light's cone_delta_deg must be >= 0");
            if (!(pl.cone_delta_deg <= pl.cone_angle_deg)) return fail(VSPG_EINVAL, "a spot light's cone_delta_deg exceeds cone_angle_deg");
        }
        if (pl.type == VSPG_LIGHT_PROJECTION) {
            const float fov = pl.cone_angle_deg;  // a projection slot's field of view
            if (!(fov > 0 && fov < 180)) return fail(VSPG_EINVAL, "a projection light's field of view (cone_angle_deg) must be in (0, 180)");
        }
        if (pl.type == VSPG_LIGHT_GONIOMETRIC) {
            // EqualAreaSphereToSquare is defined for unit vectors, and ApplyInverse(-wi) is not normalised: R R^T = 1 within 1e-4 (include/vspg.h)
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) {
                    double d = 0;
                    for (int k = 0; k < 3; ++k) d += (double)b[4 * r + k] * (double)b[4 * c + k];
                    if (!(std::fabs(d - (r == c ? 1.0 : 0.0)) <= 1e-4))
                        return fail(VSPG_ESCOPE, "a goniometric light's transform must be orthonormal (rotations and reflections only): the equal-area mapping takes unit vectors");
                }
        }
    }
    int nl = scene->n_infinite_lights;
    for (int i = 0; i < scene->n_quads; ++i)
        if (scene->quads[i].Le[0] != 0 || scene->quads[i].Le[1] != 0 || scene->quads[i].Le[2] != 0) nl++;
    (void)nl;  // (round 3: "power" and "bvh" serve any number of lights -- vspg_lightsampler.h)
    return 0;
}

}  // namespace vspg_host
