"""The rectangle walks with one lane mask and one wave vote per record (csrc/vspg_device.h: rect_hit_uv, rects_closest, rects_any)
decide and report what the walks with four nested early returns per record did, bit for bit.

The header's text of the three functions is cut out as it stands and compiled for the host next to a frozen copy of the text they
replace (namespace parent below; the record builder, beyond, rect_frame and the types come from the header for both).  On the
device the vote is a ballot over the wavefront; the host has no wavefront, so the driver is built twice:

  * vote = the lane itself: a lane whose wavefront holds no other candidate -- it leaves at the vote exactly where the parent left;
  * vote = always taken (-DVSPG_RECT_VOTE_TAKEN): a lane whose neighbour is a candidate -- it runs the whole predicated body,
    divides by whatever denom it has, and must still reject what the parent rejected and keep the earlier winner untouched.

Every lane of a real wavefront is in one of these two states at each record, and nothing else of the wavefront reaches it.

Compared bit for bit: rects_closest's (hit, t, index, u, v) -- all five defined with or without a hit --, rects_any's flag, and
rect_hit_uv's flag with (t, u, v) where it says hit; what it leaves in (t, u, v) where it says no hit was never defined, in the
parent text or the new one, and is not read.

Case 1, one record (rect_hit_uv direct, and as a list of one): axis-aligned records on 3 axes x both e1 / e2 orders (the swapped
(u, v)) x reverse_orientation x both signs of the extents, one of them with its plane through 0 so that num takes the ray's own zeros,
denormals, infinities and NaNs; two tilted (generic) records.  Random rays, rays with d[a] = +-0 and origins on the plane, then every
combination of zeros / denormals / infinities / NaNs / ordinary values in all six ray components, each with tMax = infinity, tiny
(1e-30 and a denormal), 0, NaN, an ordinary value, exactly the parent's hit distance (rejected) and one ulp above it (accepted).

Case 2, lists: no record, one record, and the 16-record list with every transition between frames and two tilted records in the
middle; random rays (every record must win some) and the special-value rays again."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "vspg-pbrt-v4_amd", "csrc", "vspg_device.h")

# rect_hit_uv / rects_closest / rects_any as they were before the vote (frozen: this text is the reference and does not follow the header)
PARENT = r"""
namespace parent {
VDEV bool rect_hit_uv(const IsectRec &r, V3 o, V3 d, float tMax, float *tHit, float *uHit, float *vHit) {
    float num, denom, u, v, t;
    if (r.axes & kIsectAxisAligned) {
        denom = d.x;
        num = r.f[1] - o.x;
        if ((int32_t)(__builtin_bit_cast(uint32_t, num) ^ __builtin_bit_cast(uint32_t, denom)) < 0) return false;
        if (beyond(num, denom, tMax)) return false;
        t = num / denom;
        if (!(t > 0) || !(t < tMax)) return false;
        float pu = o.y + d.y * t, pv = o.z + d.z * t;
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
    *tHit = t;
    *uHit = u;
    *vHit = v;
    return true;
}
VDEV bool rects_closest(const IsectRec *recs, int n, V3 o, V3 d, float tMax, float *tBest, int *iBest, float *uBest, float *vBest) {
    bool hit = false;
    float bt = tMax, bu = 0, bv = 0;
    int bi = 0;
    V3 fo = o, fd = d;
    for (int i = 0; i < n; ++i) {
        const IsectRec &r = recs[i];
        float t, u, v;
        rect_frame(fo, fd, r.axes);
        if (rect_hit_uv(r, fo, fd, bt, &t, &u, &v)) {
            const bool swapped = (r.axes & kIsectUvSwapped) != 0;
            hit = true;
            bt = t;
            bi = i;
            bu = swapped ? v : u;
            bv = swapped ? u : v;
        }
    }
    *tBest = bt;
    *iBest = bi;
    *uBest = bu;
    *vBest = bv;
    return hit;
}
VDEV bool rects_any(const IsectRec *recs, int n, V3 o, V3 d, float tMax) {
    bool any = false;
    V3 fo = o, fd = d;
    for (int i = 0; i < n; ++i) {
        const IsectRec &r = recs[i];
        float t, u, v;
        rect_frame(fo, fd, r.axes);
        any = any || rect_hit_uv(r, fo, fd, tMax, &t, &u, &v);
    }
    return any;
}
}  // namespace parent
"""

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
@SHARED@
@PARENT@
@FUNCTIONS@

static inline uint32_t f2b(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static inline float b2f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static uint64_t g_state = 0x2545F4914F6CDD1Dull;
static inline uint32_t rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_state >> 32); }
static inline float unif(float lo, float hi) { return lo + (hi - lo) * (float)((rnd() >> 8) * (1.0 / 16777216.0)); }
static const float kInf = std::numeric_limits<float>::infinity();
static const float kNaN = std::numeric_limits<float>::quiet_NaN();

static void cross(const float *a, const float *b, float *c) {
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
// what build_dscene derives of a rectangle (n = +-unit vector of e1 x e2: exact for one-axis edges)
static int make_rec(IsectRec *rec, const float *p00, const float *e1, const float *e2, bool reverse, int cur) {
    float c[3], n[3];
    cross(e1, e2, c);
    const float len = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    for (int k = 0; k < 3; ++k) n[k] = reverse ? -(c[k] / len) : c[k] / len;
    const float inv_l1 = 1.f / (e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
    const float inv_l2 = 1.f / (e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
    std::memset(rec, 0, sizeof *rec);
    return isect_rec_build(rec, n, p00, e1, e2, inv_l1, inv_l2, cur);
}

struct Tally { unsigned long long rays = 0, hits = 0, anys = 0, bad = 0, tmax_edge = 0; };
struct Closest { bool hit; float t; int i; float u, v; };
static Closest closest_new(const IsectRec *recs, int n, V3 o, V3 d, float tMax) {
    Closest c;
    c.hit = rects_closest(recs, n, o, d, tMax, &c.t, &c.i, &c.u, &c.v);
    return c;
}
static Closest closest_parent(const IsectRec *recs, int n, V3 o, V3 d, float tMax) {
    Closest c;
    c.hit = parent::rects_closest(recs, n, o, d, tMax, &c.t, &c.i, &c.u, &c.v);
    return c;
}
static void report(const char *what, V3 o, V3 d, float tMax, const Closest &a, const Closest &b, bool anyA, bool anyB) {
    printf("  %s: o %08x %08x %08x d %08x %08x %08x tMax %08x: new %d %08x %d %08x %08x any %d parent %d %08x %d %08x %08x any %d\n", what,
           f2b(o.x), f2b(o.y), f2b(o.z), f2b(d.x), f2b(d.y), f2b(d.z), f2b(tMax), a.hit, f2b(a.t), a.i, f2b(a.u), f2b(a.v), anyA, b.hit,
           f2b(b.t), b.i, f2b(b.u), f2b(b.v), anyB);
}
// one ray against a list: the closest hit's five values and the any-hit flag, every bit; returns the parent's closest hit
static Closest check_list(const char *what, const IsectRec *recs, int n, V3 o, V3 d, float tMax, Tally *T) {
    const Closest a = closest_new(recs, n, o, d, tMax), b = closest_parent(recs, n, o, d, tMax);
    const bool anyA = rects_any(recs, n, o, d, tMax), anyB = parent::rects_any(recs, n, o, d, tMax);
    T->rays++;
    T->hits += b.hit;
    T->anys += anyB;
    const bool ok = a.hit == b.hit && f2b(a.t) == f2b(b.t) && a.i == b.i && f2b(a.u) == f2b(b.u) && f2b(a.v) == f2b(b.v) && anyA == anyB;
    if (!ok && T->bad++ < 6) report(what, o, d, tMax, a, b, anyA, anyB);
    return b;
}
// one ray against one record, the test itself in the record's frame (as the walks call it) and the record as a list of one
static Closest check_one(const IsectRec &r, V3 o, V3 d, float tMax, Tally *T) {
    V3 fo = o, fd = d;
    rect_frame(fo, fd, r.axes);
    float ta = 0, ua = 0, va = 0, tb = 0, ub = 0, vb = 0;
    const bool ha = rect_hit_uv(r, fo, fd, tMax, &ta, &ua, &va), hb = parent::rect_hit_uv(r, fo, fd, tMax, &tb, &ub, &vb);
    const bool ok = ha == hb && (!hb || (f2b(ta) == f2b(tb) && f2b(ua) == f2b(ub) && f2b(va) == f2b(vb)));
    if (!ok && T->bad++ < 6)
        printf("  test: o %08x %08x %08x d %08x %08x %08x tMax %08x: new %d %08x %08x %08x parent %d %08x %08x %08x\n", f2b(o.x), f2b(o.y),
               f2b(o.z), f2b(d.x), f2b(d.y), f2b(d.z), f2b(tMax), ha, f2b(ta), f2b(ua), f2b(va), hb, f2b(tb), f2b(ub), f2b(vb));
    return check_list("one", &r, 1, o, d, tMax, T);
}
// a ray at every tMax of interest: infinity, tiny, 0, NaN, ordinary, and around the parent's own hit distance
static void check_tmaxes(const IsectRec *recs, int n, V3 o, V3 d, Tally *T) {
    const float tm[] = {kInf, 1e-30f, b2f(3), 0.f, kNaN, 1.f, 0.375f};
    for (float t : tm) {
        if (n == 1) check_one(recs[0], o, d, t, T); else check_list("list", recs, n, o, d, t, T);
    }
    const Closest h = closest_parent(recs, n, o, d, kInf);
    if (h.hit) {
        const Closest h0 = n == 1 ? check_one(recs[0], o, d, h.t, T) : check_list("list", recs, n, o, d, h.t, T);
        const Closest h1 = n == 1 ? check_one(recs[0], o, d, std::nextafter(h.t, kInf), T) : check_list("list", recs, n, o, d, std::nextafter(h.t, kInf), T);
        // at exactly the hit distance that record is rejected (another, farther one cannot win either); one ulp above it is accepted
        if (!(h0.hit == false || h0.i != h.i) || !h1.hit) T->bad++;
        T->tmax_edge++;
    }
}
static const float kSpecials[] = {0.f, -0.f, kInf, -kInf, kNaN, b2f(1), b2f(0x80400000u), 1.f, -0.5f};
static const int kNs = (int)(sizeof kSpecials / sizeof kSpecials[0]);
// the combinations of the special values in the six ray components: every one with step = 1, else every step-th (a step prime to the
// number of values walks all six slots through all values); `stride` thins the tMax sweep (every ray still runs at tMax = inf and one more)
static void special_rays(const IsectRec *recs, int n, Tally *T, int stride, int step) {
    int total = 1;
    for (int j = 0; j < 6; ++j) total *= kNs;
    for (int i = 0; i < total; i += step) {
        int k = i;
        float c[6];
        for (int j = 0; j < 6; ++j) { c[j] = kSpecials[k % kNs]; k /= kNs; }
        const V3 o{c[0], c[1], c[2]}, d{c[3], c[4], c[5]};
        if ((i / step) % stride == 0) {
            check_tmaxes(recs, n, o, d, T);
        } else {
            const float tMax = (i % 3 == 0) ? 1e-30f : ((i % 3 == 1) ? 1.f : 0.375f);
            if (n == 1) { check_one(recs[0], o, d, kInf, T); check_one(recs[0], o, d, tMax, T); }
            else { check_list("list", recs, n, o, d, kInf, T); check_list("list", recs, n, o, d, tMax, T); }
        }
    }
}
static float &at(V3 &v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }

static int one_record() {
    Tally T;
    int n_cases = 0, n_swapped = 0, n_generic = 0;
    for (int c = 0; c < 26; ++c) {
        IsectRec R;
        float p00[3] = {0, 0, 0}, e1[3] = {0, 0, 0}, e2[3] = {0, 0, 0};
        int a = -1;
        if (c < 24) {
            a = c % 3;
            const int order = (c / 3) & 1, reverse = (c / 6) & 1, sgn = (c / 12) & 1;
            const int a1 = order ? (a + 2) % 3 : (a + 1) % 3, a2 = order ? (a + 1) % 3 : (a + 2) % 3;
            // power-of-two extents in the first sign case (u and v reach exactly 1), odd ones in the second; the plane of the
            // reversed records of the first sign case goes through 0: num = -o[a], with every special value the ray brings
            const float l1 = sgn ? -1.7f : 2.f, l2 = sgn ? 0.9f : -0.5f;
            p00[a] = (reverse && !sgn) ? 0.f : 0.375f; p00[a1] = sgn ? 0.3f : -0.75f; p00[a2] = sgn ? -0.2f : 0.25f;
            e1[a1] = l1; e2[a2] = l2;
            const int frame = make_rec(&R, p00, e1, e2, reverse != 0, 0);
            if (R.kind != 1 || frame != a || ((R.axes & kIsectUvSwapped) != 0) != (order != 0)) { printf("record of case %d: kind %d axes %x\n", c, R.kind, R.axes); return 1; }
            n_swapped += order;
        } else {
            p00[0] = -0.8f; p00[1] = -0.9f; p00[2] = c == 24 ? -0.3f : 0.4f;
            e1[0] = 1.5f; e1[1] = 0.2f; e1[2] = c == 24 ? 0.6f : -0.5f;
            e2[0] = -0.1f; e2[1] = 1.7f; e2[2] = 0.3f;
            make_rec(&R, p00, e1, e2, c == 25, 0);
            if (R.kind != 0) { printf("record of case %d is not generic\n", c); return 1; }
            n_generic++;
        }
        n_cases++;
        for (int i = 0; i < 40000; ++i) {
            V3 o{unif(-2, 2), unif(-2, 2), unif(-2, 2)}, d{unif(-1, 1), unif(-1, 1), unif(-1, 1)};
            const Closest h = check_one(R, o, d, (i % 10 == 0) ? unif(0.f, 4.f) : kInf, &T);
            if (i % 16 == 0) check_tmaxes(&R, 1, o, d, &T);
            if (a >= 0 && i % 8 == 0) {   // d[a] = +-0, the origin exactly on the plane, both
                V3 o1 = o, d1 = d;
                at(d1, a) = (i & 8) ? 0.f : -0.f;
                check_one(R, o, d1, kInf, &T);
                at(o1, a) = p00[a];
                check_one(R, o1, d, kInf, &T);
                check_one(R, o1, d1, (i & 16) ? kInf : 1.f, &T);
            }
            (void)h;
        }
        special_rays(&R, 1, &T, 11, (c < 3 || c == 9 || c == 24) ? 1 : 13);   // in full: each axis, a swapped record with its plane through 0, a generic one
    }
    printf("one record: %d records (%d with (u, v) swapped, %d generic), %llu rays, %llu hits, %llu with tMax at the hit distance, mismatches %llu\n",
           n_cases, n_swapped, n_generic, T.rays, T.hits, T.tmax_edge, T.bad);
    if (T.hits < 100000 || T.tmax_edge < 5000 || n_swapped != 12 || n_generic != 2) { printf("too few rays reach the cases they are meant for\n"); return 1; }
    return T.bad != 0;
}

// 16 records: every ordered pair of axes as a transition (x x y y z z x z | two tilted | y x z y z x), both e1 / e2 orders, reversed
// or not, and rectangles that overlap so that the winner depends on the ray
static int record_lists() {
    const int N = 16;
    const int axis_of[N] = {0, 0, 1, 1, 2, 2, 0, 2, -1, -1, 1, 0, 2, 1, 2, 0};
    bool seen[3][3] = {};
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
        const int frame = make_rec(&recs[i], p00, e1, e2, (i % 3) == 1, cur);
        if (frame != (a >= 0 ? a : 0) || recs[i].kind != (a >= 0 ? 1 : 0) || (recs[i].axes & kIsectStepsMask) != (frame - cur + 3) % 3) {
            printf("record %d: kind %d axes %x frame %d after %d\n", i, recs[i].kind, recs[i].axes, frame, cur);
            return 1;
        }
        seen[cur][frame] = true;
        cur = frame;
    }
    for (int p = 0; p < 3; ++p)
        for (int q = 0; q < 3; ++q)
            if (!seen[p][q]) { printf("transition %d -> %d missing\n", p, q); return 1; }
    // two copies of one record in a row: equal distances, the first keeps winning
    IsectRec twins[2];
    {
        const float p00[3] = {0.25f, -1.f, -1.f}, e1[3] = {0, 2.f, 0}, e2[3] = {0, 0, 2.f};
        const int f = make_rec(&twins[0], p00, e1, e2, false, 0);
        make_rec(&twins[1], p00, e1, e2, true, f);
    }
    Tally T16, T1, T0, T2;
    unsigned long long wins[N] = {}, twin_second = 0;
    for (int i = 0; i < 200000; ++i) {
        V3 o{unif(-2, 2), unif(-2, 2), unif(-2, 2)}, d{unif(-1, 1), unif(-1, 1), unif(-1, 1)};
        const float tMax = (i % 4 == 0) ? unif(0.f, 3.f) : kInf;
        const Closest h = check_list("list16", recs, N, o, d, tMax, &T16);
        if (h.hit) wins[h.i]++;
        if (i % 8 == 0) check_tmaxes(recs, N, o, d, &T16);
        if (i % 4 == 0) {
            const Closest e = check_list("list0", recs, 0, o, d, tMax, &T0);
            if (e.hit || f2b(e.t) != f2b(tMax) || e.i != 0 || f2b(e.u) != 0 || f2b(e.v) != 0) T0.bad++;
            check_list("list1", recs + (i / 4) % N, 1, o, d, tMax, &T1);
            const Closest w = check_list("twins", twins, 2, o, d, tMax, &T2);
            twin_second += w.hit && w.i == 1;
        }
    }
    special_rays(recs, N, &T16, 53, 5);
    special_rays(recs, 0, &T0, 1009, 49);
    special_rays(twins, 2, &T2, 211, 7);
    int winners = 0;
    for (int k = 0; k < N; ++k) winners += wins[k] > 0;
    printf("lists: 16 records %llu rays (%llu hits, %llu any-hits, %d of %d records win some ray, %llu with tMax at the hit distance) mismatches %llu; "
           "1 record %llu rays mismatches %llu; 0 records %llu rays mismatches %llu; twin records %llu rays (%llu hits, second wins %llu) mismatches %llu\n",
           T16.rays, T16.hits, T16.anys, winners, N, T16.tmax_edge, T16.bad, T1.rays, T1.bad, T0.rays, T0.bad, T2.rays, T2.hits, twin_second, T2.bad);
    if (winners != N || T16.hits < 30000 || T16.tmax_edge < 2000 || T2.hits < 5000) { printf("the lists do not exercise every record\n"); return 1; }
    if (twin_second != 0) { printf("the second of two equal records won\n"); return 1; }
    return (T16.bad | T1.bad | T0.bad | T2.bad) != 0;
}

int main() {
    const int a = one_record(), b = record_lists();
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
def source(tmp_path_factory):
    src = open(HDR).read()
    types = "".join([_cut(src, r"^struct V3 \{.*?^};\n", "struct V3"),
                     _line(src, "VDEV V3 ld3("), _line(src, "VDEV V3 operator+(V3 a, V3 b)"), _line(src, "VDEV V3 operator-(V3 a, V3 b)"),
                     _line(src, "VDEV V3 operator*(V3 a, float s)"), _line(src, "VDEV float dot(V3 a, V3 b)"),
                     _cut(src, r"^enum \{ kIsectStepsMask.*?\n", "the record's flag bits"),
                     _cut(src, r"^struct IsectRec \{.*?^};\n", "struct IsectRec")])
    shared = "".join([_function(src, "isect_rec_build"), _function(src, "beyond"), _function(src, "rect_frame")])
    body = "".join([_function(src, "rect_hit_uv"), _function(src, "rects_closest"), _function(src, "rects_any")])
    assert "asm" not in body
    # the vote is the only thing the device build has and the host build has not, and VSPG_RECT_VOTE_TAKEN the only host switch
    assert body.count("#if defined(__HIP_DEVICE_COMPILE__)") == body.count("#elif defined(VSPG_RECT_VOTE_TAKEN)") == body.count("#endif") >= 1
    assert body.count("__ballot(") == body.count("#if")
    d = tmp_path_factory.mktemp("rect_vote")
    (d / "check.cpp").write_text(DRIVER.replace("@TYPES@", types).replace("@SHARED@", shared).replace("@PARENT@", PARENT)
                                 .replace("@FUNCTIONS@", body))
    return d


def _run(source, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.fail("no host C++ compiler")
    exe = str(source / name)
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"] + flags + ["-o", exe, str(source / "check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "result identical" in r.stdout


def test_lane_alone_in_its_wavefront_keeps_every_bit(source):
    _run(source, "check_identity", [])


def test_lane_beside_a_candidate_keeps_every_bit(source):
    _run(source, "check_taken", ["-DVSPG_RECT_VOTE_TAKEN"])
