"""The axis-aligned rectangle test in the frame of its axis (csrc/vspg_device.h: isect_rec_build, rect_frame, rect_hit_uv,
rects_closest) decides and reports what the tests it replaces did, bit for bit.

The record builder, the frame step, the test and the loop over the records are cut out of the header as they stand and compiled for
the host (the one instruction of swap_regs restated as a plain exchange; -ffp-contract=off as the device build).  Two references sit
beside them: the generic plane / edge formula quad_hit_uv, cut from the header too, and the axis-aligned test as it was before
(components picked by the record's axes, both terms times nsign, four compares as the sign pre-test), kept in the driver.

Case 1, one rectangle: 3 axes x both e1 / e2 orders x reverse_orientation x both signs of the extents, ~10^6 random rays each, then
rays with d[a] = +-0, origins on the plane, (u, v) exactly 0 or 1, every combination of zeros / infinities / NaNs / denormals in o
and d, and tMax equal to the hit distance (rejected) and one ulp above it (accepted).  hit, t, u, v must agree with BOTH references.
Two things set the GENERIC formula apart from the axis-aligned arithmetic, old and new alike, so they are no part of this claim:
its dot products add the +0 products of the normal's and the edges' zero components, which turns a u or v of -0 into +0 -- against
it a zero's sign is not compared, every other bit is --, and with an infinite or NaN component in the ray 0 * inf makes those dot
products NaN where the axis-aligned text never forms the product -- such rays are left out against it, counted and printed.
Against the earlier axis-aligned text every ray and every bit counts.

Case 2, the frame bookkeeping: a 16-record list with every transition between axes and two tilted (kind-0) records in the middle,
walked by rects_closest / rects_any, against a plain loop of per-record evaluations in the scene frame: winner index and bits."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "vspg-pbrt-v4_amd", "csrc", "vspg_device.h")

DRIVER = r"""
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#define VDEV static inline
@TYPES@
VDEV void swap_regs(float &a, float &b) { const float t = a; a = b; b = t; }   // v_swap_b32
@FUNCTIONS@

// ---- the axis-aligned test as it was: record and text ----
namespace old {
struct Rec { float f[14]; int32_t kind, axes; };
static void build(Rec *rec, const float *n, const float *p00, const float *e1, const float *e2, float inv_l1, float inv_l2) {
    auto single_axis = [](const float *v) {
        int nz = 0, ax = -1;
        for (int k = 0; k < 3; ++k)
            if (v[k] != 0) { nz++; ax = k; }
        return nz == 1 ? ax : -1;
    };
    int an = single_axis(n), a1 = single_axis(e1), a2 = single_axis(e2);
    std::memset(rec, 0, sizeof *rec);
    if (an >= 0 && a1 >= 0 && a2 >= 0 && an != a1 && an != a2 && a1 != a2 && std::fabs(n[an]) == 1.0f) {
        rec->kind = 1;
        rec->axes = an | (a1 << 2) | (a2 << 4);
        rec->f[0] = n[an]; rec->f[1] = p00[an]; rec->f[2] = p00[a1]; rec->f[3] = p00[a2];
        rec->f[4] = e1[a1]; rec->f[5] = e2[a2]; rec->f[6] = inv_l1; rec->f[7] = inv_l2;
    } else {
        rec->kind = 0;
        for (int k = 0; k < 3; ++k) { rec->f[k] = n[k]; rec->f[3 + k] = p00[k]; rec->f[6 + k] = e1[k]; rec->f[9 + k] = e2[k]; }
        rec->f[12] = inv_l1; rec->f[13] = inv_l2;
    }
}
static bool rect_hit_uv(const Rec &r, V3 o, V3 d, float tMax, float *tHit, float *uHit, float *vHit) {
    float num, denom, u, v, t;
    if (r.kind == 1) {
        const int a = r.axes & 3, ua = (r.axes >> 2) & 3, va = (r.axes >> 4) & 3;
        denom = r.f[0] * comp(d, a);
        num = r.f[0] * (r.f[1] - comp(o, a));
        bool cand = (num > 0 && denom > 0) || (num < 0 && denom < 0);
        if (!cand) return false;
        if (beyond(num, denom, tMax)) return false;
        t = num / denom;
        if (!(t > 0) || !(t < tMax)) return false;
        float pu = comp(o, ua) + comp(d, ua) * t, pv = comp(o, va) + comp(d, va) * t;
        u = ((pu - r.f[2]) * r.f[4]) * r.f[6];
        v = ((pv - r.f[3]) * r.f[5]) * r.f[7];
    } else {
        V3 n = V3{r.f[0], r.f[1], r.f[2]}, p00 = V3{r.f[3], r.f[4], r.f[5]};
        denom = dot(n, d);
        num = dot(n, p00 - o);
        bool cand = (num > 0 && denom > 0) || (num < 0 && denom < 0);
        if (!cand) return false;
        if (beyond(num, denom, tMax)) return false;
        t = num / denom;
        if (!(t > 0) || !(t < tMax)) return false;
        V3 p = o + d * t;
        V3 rel = p - p00;
        u = dot(rel, V3{r.f[6], r.f[7], r.f[8]}) * r.f[12];
        v = dot(rel, V3{r.f[9], r.f[10], r.f[11]}) * r.f[13];
    }
    if (u < 0 || u > 1 || v < 0 || v > 1) return false;
    *tHit = t; *uHit = u; *vHit = v;
    return true;
}
}  // namespace old

static inline uint32_t f2b(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static inline float b2f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static inline uint32_t rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_state >> 32); }
static inline float unif(float lo, float hi) { return lo + (hi - lo) * (float)((rnd() >> 8) * (1.0 / 16777216.0)); }
static const float kInf = std::numeric_limits<float>::infinity();

// what build_dscene derives of a rectangle (n = +-unit vector of e1 x e2: exact for one-axis edges)
struct Rect { DQuad q; IsectRec rec; old::Rec orec; };
static void cross(const float *a, const float *b, float *c) {
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
static int make_rect(Rect *R, const float *p00, const float *e1, const float *e2, bool reverse, int cur) {
    std::memset(R, 0, sizeof *R);
    float c[3];
    cross(e1, e2, c);
    const float len = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    for (int k = 0; k < 3; ++k) {
        R->q.p00[k] = p00[k]; R->q.e1[k] = e1[k]; R->q.e2[k] = e2[k];
        R->q.n[k] = c[k] / len;
        if (reverse) R->q.n[k] = -R->q.n[k];
    }
    R->q.inv_l1 = 1.f / (e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
    R->q.inv_l2 = 1.f / (e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
    old::build(&R->orec, R->q.n, R->q.p00, R->q.e1, R->q.e2, R->q.inv_l1, R->q.inv_l2);
    return isect_rec_build(&R->rec, R->q.n, R->q.p00, R->q.e1, R->q.e2, R->q.inv_l1, R->q.inv_l2, cur);
}

struct Hit { bool hit; float t, u, v; };
static bool same(const Hit &a, const Hit &b) {
    if (a.hit != b.hit) return false;
    return !a.hit || (f2b(a.t) == f2b(b.t) && f2b(a.u) == f2b(b.u) && f2b(a.v) == f2b(b.v));
}
// against the generic formula: the same, but -0 and +0 are one value of u or v (its dot products end in `+ 0`)
static bool same_but_zero_sign(const Hit &a, const Hit &b) {
    if (a.hit != b.hit) return false;
    auto eq = [](float x, float y) { return f2b(x) == f2b(y) || (x == 0 && y == 0); };
    return !a.hit || (f2b(a.t) == f2b(b.t) && eq(a.u, b.u) && eq(a.v, b.v));
}
// the new test as the loops use it: the ray turned into the record's frame, the swapped (u, v) traded back
static Hit hit_new(const IsectRec &r, V3 o, V3 d, float tMax) {
    Hit h{false, 0, 0, 0};
    float u = 0, v = 0;
    rect_frame(o, d, r.axes);
    h.hit = rect_hit_uv(r, o, d, tMax, &h.t, &u, &v);
    const bool swapped = (r.axes & kIsectUvSwapped) != 0;
    h.u = swapped ? v : u;
    h.v = swapped ? u : v;
    return h;
}
static Hit hit_old(const old::Rec &r, V3 o, V3 d, float tMax) {
    Hit h{false, 0, 0, 0};
    h.hit = old::rect_hit_uv(r, o, d, tMax, &h.t, &h.u, &h.v);
    return h;
}
static Hit hit_generic(const DQuad &q, V3 o, V3 d, float tMax) {
    Hit h{false, 0, 0, 0};
    h.hit = quad_hit_uv(q, o, d, tMax, &h.t, &h.u, &h.v);
    return h;
}

struct Tally { unsigned long long rays = 0, hits = 0, bad_old = 0, bad_generic = 0, generic_left_out = 0, generic_left_out_differ = 0; };
static bool finite3(V3 a) { return std::isfinite(a.x) && std::isfinite(a.y) && std::isfinite(a.z); }
static void report(const char *what, V3 o, V3 d, float tMax, const Hit &a, const Hit &b) {
    printf("  %s: o %08x %08x %08x d %08x %08x %08x tMax %08x: new %d %08x %08x %08x ref %d %08x %08x %08x\n", what, f2b(o.x), f2b(o.y),
           f2b(o.z), f2b(d.x), f2b(d.y), f2b(d.z), f2b(tMax), a.hit, f2b(a.t), f2b(a.u), f2b(a.v), b.hit, f2b(b.t), f2b(b.u), f2b(b.v));
}
static Hit check(const Rect &R, V3 o, V3 d, float tMax, Tally *T) {
    const Hit a = hit_new(R.rec, o, d, tMax), b = hit_old(R.orec, o, d, tMax), c = hit_generic(R.q, o, d, tMax);
    T->rays++;
    T->hits += a.hit;
    if (!same(a, b) && T->bad_old++ < 4) report("old", o, d, tMax, a, b);
    if (finite3(o) && finite3(d)) {
        if (!same_but_zero_sign(a, c) && T->bad_generic++ < 4) report("generic", o, d, tMax, a, c);
    } else {
        T->generic_left_out++;
        T->generic_left_out_differ += !same_but_zero_sign(a, c);
    }
    return a;
}
static float &at(V3 &v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }

static int one_rectangle() {
    Tally T;
    unsigned long long n_u_edge = 0, n_tmax_edge = 0, n_cases = 0;
    const float specials[] = {0.f, -0.f, kInf, -kInf, std::numeric_limits<float>::quiet_NaN(), b2f(1), b2f(0x80000001u), b2f(0x00400000u),
                              1.f, -0.5f};
    for (int a = 0; a < 3; ++a)
        for (int order = 0; order < 2; ++order)
            for (int reverse = 0; reverse < 2; ++reverse)
                for (int sgn = 0; sgn < 2; ++sgn) {
                    n_cases++;
                    const int a1 = order ? (a + 2) % 3 : (a + 1) % 3, a2 = order ? (a + 1) % 3 : (a + 2) % 3;
                    // power-of-two extents in the first sign case (u and v reach exactly 1), odd ones in the second
                    const float l1 = sgn ? -1.7f : 2.f, l2 = sgn ? 0.9f : -0.5f;
                    float p00[3] = {0, 0, 0}, e1[3] = {0, 0, 0}, e2[3] = {0, 0, 0};
                    p00[a] = 0.375f; p00[a1] = sgn ? 0.3f : -0.75f; p00[a2] = sgn ? -0.2f : 0.25f;
                    e1[a1] = l1; e2[a2] = l2;
                    Rect R;
                    const int frame = make_rect(&R, p00, e1, e2, reverse != 0, 0);
                    if (R.rec.kind != 1 || R.orec.kind != 1 || frame != a || ((R.rec.axes & kIsectUvSwapped) != 0) != (order != 0) ||
                        (R.rec.axes & kIsectStepsMask) != a) {
                        printf("record of case axis %d order %d: kind %d axes %x frame %d\n", a, order, R.rec.kind, R.rec.axes, frame);
                        return 1;
                    }
                    // random rays: origins around the rectangle, directions of every sign, a tenth with a finite tMax near the hit
                    for (int i = 0; i < 1000000; ++i) {
                        V3 o{unif(-2, 2), unif(-2, 2), unif(-2, 2)}, d{unif(-1, 1), unif(-1, 1), unif(-1, 1)};
                        float tMax = kInf;
                        if (i % 10 == 0) tMax = unif(0.f, 4.f);
                        const Hit h = check(R, o, d, tMax, &T);
                        if (h.hit && i % 4 == 0) {   // tMax equal to the hit distance: rejected by all; one ulp above: accepted by all
                            const Hit h0 = check(R, o, d, h.t, &T), h1 = check(R, o, d, std::nextafter(h.t, kInf), &T);
                            if (h0.hit || !h1.hit) { printf("tMax at the hit distance: %d %d\n", h0.hit, h1.hit); return 1; }
                            n_tmax_edge++;
                        }
                    }
                    // d[a] = +-0, the origin exactly on the plane, both
                    for (int i = 0; i < 20000; ++i) {
                        V3 o{unif(-2, 2), unif(-2, 2), unif(-2, 2)}, d{unif(-1, 1), unif(-1, 1), unif(-1, 1)};
                        V3 o1 = o, d1 = d;
                        at(d1, a) = (i & 1) ? 0.f : -0.f;
                        check(R, o, d1, kInf, &T);
                        at(o1, a) = p00[a];
                        check(R, o1, d, kInf, &T);
                        check(R, o1, d1, (i & 2) ? kInf : 1.f, &T);
                    }
                    // (u, v) exactly 0 or 1: the origin over an edge or a corner, no motion along that edge's axis
                    for (int i = 0; i < 20000; ++i) {
                        V3 o{unif(-2, 2), unif(-2, 2), unif(-2, 2)}, d{unif(-1, 1), unif(-1, 1), unif(-1, 1)};
                        const int eu = i % 3, ev = (i / 3) % 3;   // 0: free, 1: parameter 0, 2: parameter 1
                        if (eu) { at(o, a1) = p00[a1] + (eu == 2 ? l1 : 0.f); at(d, a1) = (i & 8) ? 0.f : -0.f; }
                        if (ev) { at(o, a2) = p00[a2] + (ev == 2 ? l2 : 0.f); at(d, a2) = (i & 16) ? 0.f : -0.f; }
                        const Hit h = check(R, o, d, kInf, &T);
                        if (h.hit && ((eu && (h.u == 0.f || h.u == 1.f)) || (ev && (h.v == 0.f || h.v == 1.f)))) n_u_edge++;
                    }
                    // zeros, infinities, NaNs, denormals and ordinary values in every slot of o and d
                    const int ns = (int)(sizeof specials / sizeof specials[0]);
                    for (int i = 0; i < ns * ns * ns * ns * ns * ns; ++i) {
                        int k = i;
                        float c[6];
                        for (int j = 0; j < 6; ++j) { c[j] = specials[k % ns]; k /= ns; }
                        const float tMax = (i % 3 == 0) ? kInf : ((i % 3 == 1) ? 1.f : 0.375f);
                        check(R, V3{c[0], c[1], c[2]}, V3{c[3], c[4], c[5]}, tMax, &T);
                    }
                }
    printf("one rectangle: %llu cases, %llu rays, %llu hits, %llu hits with u or v exactly 0 or 1, %llu with tMax at the hit distance\n",
           n_cases, T.rays, T.hits, n_u_edge, n_tmax_edge);
    printf("one rectangle: mismatches against the earlier axis-aligned test %llu, against the generic formula %llu "
           "(rays with an infinite or NaN component, not held against the generic formula: %llu, of which it answers differently %llu)\n",
           T.bad_old, T.bad_generic, T.generic_left_out, T.generic_left_out_differ);
    if (T.hits < 1000000 || n_u_edge < 1000 || n_tmax_edge < 50000) { printf("too few rays reach the cases they are meant for\n"); return 1; }
    return T.bad_old != 0 || T.bad_generic != 0;
}

// 16 records: every ordered pair of axes as a transition (x x y y z z x z | two tilted | y x z y z x), both e1 / e2 orders,
// reversed or not, and rectangles that overlap so that the winner depends on the ray
static int record_list() {
    const int N = 16;
    const int axis_of[N] = {0, 0, 1, 1, 2, 2, 0, 2, -1, -1, 1, 0, 2, 1, 2, 0};
    bool seen[3][3] = {};
    Rect R[N];
    IsectRec recs[N];
    int cur = 0;
    for (int i = 0; i < N; ++i) {
        float p00[3], e1[3] = {0, 0, 0}, e2[3] = {0, 0, 0};
        const int a = axis_of[i];
        if (a >= 0) {
            const int order = (i * 7 / 3) & 1, a1 = order ? (a + 2) % 3 : (a + 1) % 3, a2 = order ? (a + 1) % 3 : (a + 2) % 3;
            p00[a] = -1.2f + 0.16f * i;
            p00[a1] = unif(-1.5f, -0.5f);
            p00[a2] = unif(-1.5f, -0.5f);
            e1[a1] = unif(1.2f, 2.4f);
            e2[a2] = unif(1.2f, 2.4f);
            if (i % 5 == 0) { p00[a1] += e1[a1]; e1[a1] = -e1[a1]; }
        } else {
            p00[0] = -0.8f; p00[1] = -0.9f; p00[2] = i == 8 ? -0.3f : 0.4f;
            e1[0] = 1.5f; e1[1] = 0.2f; e1[2] = i == 8 ? 0.6f : -0.5f;
            e2[0] = -0.1f; e2[1] = 1.7f; e2[2] = 0.3f;
        }
        const int frame = make_rect(&R[i], p00, e1, e2, (i % 3) == 1, cur);
        if (frame != (a >= 0 ? a : 0) || R[i].rec.kind != (a >= 0 ? 1 : 0) || (R[i].rec.axes & kIsectStepsMask) != (frame - cur + 3) % 3) {
            printf("record %d: kind %d axes %x frame %d after %d\n", i, R[i].rec.kind, R[i].rec.axes, frame, cur);
            return 1;
        }
        seen[cur][frame] = true;
        cur = frame;
        recs[i] = R[i].rec;
    }
    for (int p = 0; p < 3; ++p)
        for (int q = 0; q < 3; ++q)
            if (!seen[p][q]) { printf("transition %d -> %d missing\n", p, q); return 1; }
    unsigned long long bad = 0, hits = 0, wins[N] = {}, anys = 0;
    for (int i = 0; i < 1000000; ++i) {
        V3 o{unif(-2, 2), unif(-2, 2), unif(-2, 2)}, d{unif(-1, 1), unif(-1, 1), unif(-1, 1)};
        const float tMax = (i % 4 == 0) ? unif(0.f, 3.f) : kInf;
        // plain evaluation, every record in the scene frame with the earlier / generic text
        bool hit = false, any = false;
        float bt = tMax, bu = 0, bv = 0;
        int bi = 0;
        for (int k = 0; k < N; ++k) {
            const Hit h = R[k].orec.kind == 1 ? hit_old(R[k].orec, o, d, bt) : hit_generic(R[k].q, o, d, bt);
            if (h.hit) { hit = true; bt = h.t; bi = k; bu = h.u; bv = h.v; }
            any = any || (R[k].orec.kind == 1 ? hit_old(R[k].orec, o, d, tMax) : hit_generic(R[k].q, o, d, tMax)).hit;
        }
        float t, u, v;
        int idx;
        const bool nhit = rects_closest(recs, N, o, d, tMax, &t, &idx, &u, &v);
        const bool nany = rects_any(recs, N, o, d, tMax);
        const bool ok = nhit == hit && nany == any && idx == bi && f2b(t) == f2b(bt) && f2b(u) == f2b(bu) && f2b(v) == f2b(bv);
        if (!ok && bad++ < 4)
            printf("  list: ray %d: new %d %d %d %08x %08x %08x plain %d %d %d %08x %08x %08x\n", i, nhit, nany, idx, f2b(t), f2b(u), f2b(v),
                   hit, any, bi, f2b(bt), f2b(bu), f2b(bv));
        hits += hit;
        anys += any;
        if (hit) wins[bi]++;
    }
    int winners = 0;
    for (int k = 0; k < N; ++k) winners += wins[k] > 0;
    printf("record list: 1000000 rays, %llu hits, %llu any-hits, %d of %d records win some ray, mismatches %llu\n", hits, anys, winners, N, bad);
    if (winners != N || hits < 100000) { printf("the list does not exercise every record\n"); return 1; }
    return bad != 0;
}

int main() {
    const int a = one_rectangle(), b = record_list();
    printf("result %s\n", (a || b) ? "MISMATCH" : "identical");
    return a || b;
}
"""


def _cut(src, pattern, what):
    m = re.search(pattern, src, re.S | re.M)
    assert m, "%s not found in vspg_device.h" % what
    return m.group(0)


def _function(src, name):
    return _cut(src, r"^(?:VDEV|inline) \w+ %s\(.*?^}\n" % name, name)


def _line(src, start):
    return _cut(src, r"^%s[^\n]*\n" % re.escape(start), start)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.fail("no host C++ compiler")
    src = open(HDR).read()
    types = "".join([_cut(src, r"^struct V3 \{.*?^};\n", "struct V3"),
                     _line(src, "VDEV V3 ld3("), _line(src, "VDEV V3 operator+(V3 a, V3 b)"), _line(src, "VDEV V3 operator-(V3 a, V3 b)"),
                     _line(src, "VDEV V3 operator*(V3 a, float s)"), _line(src, "VDEV float dot(V3 a, V3 b)"),
                     _cut(src, r"^struct DQuad \{.*?^};\n", "struct DQuad"),
                     _cut(src, r"^enum \{ kIsectStepsMask.*?\n", "the record's flag bits"),
                     _cut(src, r"^struct IsectRec \{.*?^};\n", "struct IsectRec")])
    body = "".join([_function(src, "isect_rec_build"), _function(src, "beyond"), _line(src, "VDEV float comp(V3 v, int axis)"),
                    _function(src, "rect_frame"), _function(src, "rect_hit_uv"), _function(src, "rects_closest"), _function(src, "rects_any"),
                    _function(src, "quad_hit_uv")])
    assert "asm" not in body, "only swap_regs may hold an instruction by name; the driver restates that one function"
    d = tmp_path_factory.mktemp("rect_frame")
    (d / "check.cpp").write_text(DRIVER.replace("@TYPES@", types).replace("@FUNCTIONS@", body))
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-o", str(d / "check"), str(d / "check.cpp")], check=True)
    return str(d / "check")


def test_axis_frame_rectangle_tests_keep_every_bit(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "result identical" in r.stdout
