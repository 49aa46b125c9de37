"""The closest-hit walk that tests the two walls of a twin pair in one pass (csrc/vspg_device.h: rect_twins_mark, rect_hit_uv_twins,
rects_closest_twins) reports what the plain walk (rects_closest) reports: hit, t, index, u and v, bit for bit, no tolerance.

The header's own text is compiled stand-alone for the host, as tests/test_rect_vote_bits.py does.  On the device the two votes of a
pair are ballots; the host has no wavefront, so three builds stand for what a lane can see:
  * both votes are the lane itself: a lane alone in its wavefront;
  * -DVSPG_RECT_TWIN_VOTE=1, `some` always taken: a lane beside a candidate -- it runs the merged body though it is no candidate;
  * -DVSPG_RECT_TWIN_VOTE=2, the both-candidates vote always taken: every pair falls back, which is the plain walk by construction.
VSPG_RECT_VOTE_TAKEN stays reserved for its own test.  The plain walk runs over records that were never marked.

Scenes: the fog box (vspg_scene_fog_box's seven rectangles); the same box seen from outside; a pair that differs in one in-plane
field and opposite walls that are not adjacent in the list (neither may be marked); two coplanar identical records (marked: every
candidate is a candidate of both, the second never wins); 16 records with a pair on every frame transition, both (u, v) orders
and a generic record between pairs.  Rays: origins inside, outside and exactly on planes; direction and origin components +-0,
+-inf, NaN, denormal; tMax finite, infinite, tiny, 0, NaN and at the hit distance; rays through the box's edges and corners with
dyadic coordinates, where two or three walls give exactly the same t and the lower index has to win.  More than 10^7 rays per build.

Neither path may hide behind the other (asserted by the driver where the votes are the lane's own or `some` is taken): on origins
strictly inside the box with finite non-zero directions at least 99 % of the (ray, pair) evaluations take the merged path, and on
origins uniform in [-3, 3]^3 with tMax = inf at least 10 % take the fallback.

rect_twins_mark is held against pairs found here in Python from the unmarked records, and against the pairs each scene's geometry
dictates."""
import os
import re
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "vspg-pbrt-v4_amd", "csrc", "vspg_device.h")

DRIVER = r"""
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#define VDEV static inline
static unsigned long long g_path[2];   // (ray, pair) evaluations: [0] merged, [1] fallback
#define VSPG_RECT_TWIN_PATH(fallback) g_path[(fallback) ? 1 : 0]++
#ifndef VSPG_RECT_TWIN_VOTE
#define VSPG_RECT_TWIN_VOTE 0
#endif
@TYPES@
VDEV void swap_regs(float &a, float &b) { const float t = a; a = b; b = t; }   // v_swap_b32
@FUNCTIONS@

static inline uint32_t f2b(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static inline float b2f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static inline uint32_t rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_state >> 32); }
static inline float unif(float lo, float hi) { return lo + (hi - lo) * (float)((rnd() >> 8) * (1.0 / 16777216.0)); }
static const float kInf = std::numeric_limits<float>::infinity();
static const float kNaN = std::numeric_limits<float>::quiet_NaN();

struct Quad { float p00[3], e1[3], e2[3]; bool reverse; };
struct Scene { const char *name; int n; IsectRec plain[16], recs[16], solo[16]; float lo, hi; };
static void cross(const float *a, const float *b, float *c) {
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
// what build_dscene derives of a rectangle (n = +-unit vector of e1 x e2: exact for one-axis edges)
static int make_rec(IsectRec *rec, const Quad &q, int cur) {
    float c[3], n[3];
    cross(q.e1, q.e2, c);
    const float len = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    for (int k = 0; k < 3; ++k) n[k] = q.reverse ? -(c[k] / len) : c[k] / len;
    const float inv_l1 = 1.f / (q.e1[0] * q.e1[0] + q.e1[1] * q.e1[1] + q.e1[2] * q.e1[2]);
    const float inv_l2 = 1.f / (q.e2[0] * q.e2[0] + q.e2[1] * q.e2[1] + q.e2[2] * q.e2[2]);
    std::memset(rec, 0, sizeof *rec);
    return isect_rec_build(rec, n, q.p00, q.e1, q.e2, inv_l1, inv_l2, cur);
}
static void print_rec(const char *scene, const char *when, int i, const IsectRec &r) {
    printf("rec %s %s %d %d %d", scene, when, i, r.kind, r.axes);
    for (int k = 0; k < 14; ++k) printf(" %08x", f2b(r.f[k]));
    printf("\n");
}
static void build(Scene *S, const char *name, const Quad *q, int n, float lo, float hi) {
    S->name = name; S->n = n; S->lo = lo; S->hi = hi;
    int cur = 0;
    for (int i = 0; i < n; ++i) { cur = make_rec(&S->plain[i], q[i], cur); make_rec(&S->solo[i], q[i], 0); }
    std::memcpy(S->recs, S->plain, sizeof S->plain);
    rect_twins_mark(S->recs, n);
    IsectRec again[16];
    std::memcpy(again, S->recs, sizeof again);
    rect_twins_mark(again, n);
    if (std::memcmp(again, S->recs, sizeof(IsectRec) * n) != 0) { printf("marking %s twice changed it\n", name); std::exit(1); }
    for (int i = 0; i < n; ++i) { print_rec(name, "before", i, S->plain[i]); print_rec(name, "after", i, S->recs[i]); }
}

struct Tally { unsigned long long rays = 0, hits = 0, bad = 0, ties = 0, second = 0, wins[16] = {}; };
struct Closest { bool hit; float t; int i; float u, v; };
static bool same(const Closest &a, const Closest &b) {
    return a.hit == b.hit && f2b(a.t) == f2b(b.t) && a.i == b.i && f2b(a.u) == f2b(b.u) && f2b(a.v) == f2b(b.v);
}
// one ray: the twin walk over the marked records against the plain walk over the unmarked ones, and the plain walk over the marked
// ones (it reads none of the new bits); returns the plain walk's answer
static Closest check(const Scene &S, V3 o, V3 d, float tMax, Tally *T) {
    Closest a, b, c;
    a.hit = rects_closest_twins(S.recs, S.n, o, d, tMax, &a.t, &a.i, &a.u, &a.v);
    b.hit = rects_closest(S.plain, S.n, o, d, tMax, &b.t, &b.i, &b.u, &b.v);
    c.hit = rects_closest(S.recs, S.n, o, d, tMax, &c.t, &c.i, &c.u, &c.v);
    T->rays++;
    T->hits += b.hit;
    if (b.hit) { T->wins[b.i]++; T->second += (S.recs[b.i > 0 ? b.i - 1 : 0].axes & kIsectTwin) != 0 && b.i > 0; }
    if ((!same(a, b) || !same(c, b)) && T->bad++ < 6)
        printf("  %s: o %08x %08x %08x d %08x %08x %08x tMax %08x: twins %d %08x %d %08x %08x plain %d %08x %d %08x %08x\n", S.name, f2b(o.x), f2b(o.y),
               f2b(o.z), f2b(d.x), f2b(d.y), f2b(d.z), f2b(tMax), a.hit, f2b(a.t), a.i, f2b(a.u), f2b(a.v), b.hit, f2b(b.t), b.i, f2b(b.u), f2b(b.v));
    return b;
}
// a ray at every tMax of interest: infinity, tiny, 0, NaN, ordinary, and around the plain walk's own hit distance
static void check_tmaxes(const Scene &S, V3 o, V3 d, Tally *T) {
    const float tm[] = {kInf, 1e-30f, b2f(3), 0.f, kNaN, 1.f, 0.375f, 2.5f};
    for (float t : tm) check(S, o, d, t, T);
    Closest h;
    h.hit = rects_closest(S.plain, S.n, o, d, kInf, &h.t, &h.i, &h.u, &h.v);
    if (h.hit) { check(S, o, d, h.t, T); check(S, o, d, std::nextafter(h.t, kInf), T); }
}
static float &at(V3 &v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }
static const float kSpecials[] = {0.f, -0.f, kInf, -kInf, kNaN, b2f(1), b2f(0x80400000u), 1.f, -0.5f};
static const int kNs = (int)(sizeof kSpecials / sizeof kSpecials[0]);
// the combinations of the special values in the six ray components, every step-th (a step prime to 9 walks all six slots through
// all values), at tMax = inf and one finite value
static void special_rays(const Scene &S, Tally *T, int step) {
    int total = 1;
    for (int j = 0; j < 6; ++j) total *= kNs;
    for (int i = 0; i < total; i += step) {
        int k = i;
        float c[6];
        for (int j = 0; j < 6; ++j) { c[j] = kSpecials[k % kNs]; k /= kNs; }
        const V3 o{c[0], c[1], c[2]}, d{c[3], c[4], c[5]};
        check(S, o, d, kInf, T);
        check(S, o, d, (i % 3 == 0) ? 1e-30f : ((i % 3 == 1) ? 1.f : 2.5f), T);
        if ((i / step) % 64 == 0) check_tmaxes(S, o, d, T);
    }
}
// the plane coordinates of the axis-aligned records, to put origins exactly on them
static int planes_of(const Scene &S, int *axis, float *coord) {
    int m = 0;
    for (int i = 0; i < S.n; ++i)
        if (S.plain[i].kind == 1) { axis[m] = (S.plain[i].axes >> kIsectAxisShift) & 3; coord[m++] = S.plain[i].f[1]; }
    return m;
}
// random rays: `inside` origins in (lo, hi)^3 of the scene (strictly: unif never returns hi, and lo is moved up), else in [-3, 3]^3
static void random_rays(const Scene &S, Tally *T, int count, bool inside) {
    int axis[16];
    float coord[16];
    const int m = planes_of(S, axis, coord);
    const float lo = inside ? std::nextafter(S.lo, kInf) : -3.f, hi = inside ? S.hi : 3.f;
    for (int i = 0; i < count; ++i) {
        V3 o{unif(lo, hi), unif(lo, hi), unif(lo, hi)}, d{unif(-1, 1), unif(-1, 1), unif(-1, 1)};
        const float tMax = (i % 4 == 3) ? unif(0.f, 4.f) : kInf;
        check(S, o, d, tMax, T);
        if (i % 32 == 0) check_tmaxes(S, o, d, T);
        if (i % 8 == 0 && m > 0) {   // the origin exactly on a plane, d[a] = +-0, both, a denormal and an infinite component
            const int k = (i / 8) % m;
            V3 o1 = o, d1 = d, d2 = d;
            at(o1, axis[k]) = coord[k];
            at(d1, axis[k]) = (i & 8) ? 0.f : -0.f;
            at(d2, (axis[k] + 1 + ((i >> 4) & 1)) % 3) = (i & 64) ? b2f(0x00000005u) : ((i & 128) ? kInf : -kInf);
            check(S, o1, d, tMax, T);
            check(S, o, d1, tMax, T);
            check(S, o1, d1, tMax, T);
            check(S, o, d2, tMax, T);
            check(S, o1, d2, kInf, T);
        }
    }
}
// rays through edges and corners of a box [-1, 1]^3 from dyadic origins: d = target - o is exact and every wall the target lies on
// gives t = 1 exactly (num == denom), so two or three walls tie and the lower index must win
static void edge_and_corner_rays(const Scene &S, Tally *T, int count, bool inside) {
    for (int i = 0; i < count; ++i) {
        V3 o, g;
        for (int k = 0; k < 3; ++k) {
            const float q = (float)((int)(rnd() % 255u) - 127) / 128.f;   // dyadic, strictly inside (-1, 1)
            at(o, k) = inside ? q : 3.f * q;
            at(g, k) = (rnd() & 1u) ? 1.f : -1.f;
        }
        if (i % 3 != 0) at(g, rnd() % 3u) = (float)((int)(rnd() % 255u) - 127) / 128.f;   // two in three lie on an edge, the others in a corner
        const V3 d = g - o;
        const float tm[] = {kInf, 2.f, std::nextafter(1.f, kInf), 1.f};
        for (float tMax : tm) {
            const Closest h = check(S, o, d, tMax, T);
            if (tMax != kInf) continue;
            int tied = 0, first = -1;
            for (int k = 0; k < S.n; ++k) {
                Closest s;
                s.hit = rects_closest(&S.solo[k], 1, o, d, kInf, &s.t, &s.i, &s.u, &s.v);
                if (s.hit && h.hit && f2b(s.t) == f2b(h.t)) { tied++; if (first < 0) first = k; }
            }
            if (tied >= 2) { T->ties++; if (h.i != first) T->bad++; }
        }
    }
}
static int report(const Scene &S, const Tally &T, unsigned long long *total) {
    int winners = 0;
    for (int k = 0; k < S.n; ++k) winners += T.wins[k] > 0;
    printf("scene %s: %llu rays, %llu hits, %d of %d records win some ray, a pair's second wall wins %llu, ties %llu, mismatches %llu\n", S.name, T.rays,
           T.hits, winners, S.n, T.second, T.ties, T.bad);
    *total += T.rays;
    return T.bad != 0;
}
static int paths(const char *what, unsigned long long before[2], double least_merged, double least_fallback) {
    const unsigned long long m = g_path[0] - before[0], f = g_path[1] - before[1];
    const double fm = (m + f) ? (double)m / (double)(m + f) : 0., ff = (m + f) ? (double)f / (double)(m + f) : 0.;
    printf("paths %s: merged %llu, fallback %llu (%.4f / %.4f)\n", what, m, f, fm, ff);
    if (VSPG_RECT_TWIN_VOTE == 2) return (m != 0);   // every pair falls back
    return fm < least_merged || ff < least_fallback;
}

int main() {
    int bad = 0;
    unsigned long long total = 0;
    // ---- the fog box: floor, ceiling, back, front, left, right, the ceiling light
    const Quad box[7] = {{{-1, -1, -1}, {0, 0, 2}, {2, 0, 0}, false}, {{-1, 1, -1}, {2, 0, 0}, {0, 0, 2}, false}, {{-1, -1, 1}, {0, 2, 0}, {2, 0, 0}, false},
                         {{-1, -1, -1}, {2, 0, 0}, {0, 2, 0}, false}, {{-1, -1, -1}, {0, 2, 0}, {0, 0, 2}, false}, {{1, -1, -1}, {0, 0, 2}, {0, 2, 0}, false},
                         {{-0.25f, 0.999f, -0.25f}, {0.5f, 0, 0}, {0, 0, 0.5f}, false}};
    Scene B;
    build(&B, "box", box, 7, -1.f, 1.f);
    {
        Tally T;
        unsigned long long p0[2] = {g_path[0], g_path[1]};
        for (int i = 0; i < 2000000; ++i) {   // strictly inside, finite non-zero directions, tMax = inf: the merged path's case
            V3 o{unif(std::nextafter(-1.f, 0.f), 1.f), unif(std::nextafter(-1.f, 0.f), 1.f), unif(std::nextafter(-1.f, 0.f), 1.f)}, d{unif(-1, 1), unif(-1, 1), unif(-1, 1)};
            if (d.x == 0) d.x = 0.5f;
            if (d.y == 0) d.y = 0.5f;
            if (d.z == 0) d.z = 0.5f;
            check(B, o, d, kInf, &T);
        }
        bad |= paths("box, origins inside, tMax inf", p0, 0.99, 0.);
        random_rays(B, &T, 600000, true);
        edge_and_corner_rays(B, &T, 100000, true);
        special_rays(B, &T, 1);
        bad |= report(B, T, &total);
        if (T.ties < 50000 || T.second < 500000 || T.hits < 2000000) { printf("the box's rays miss the cases they are meant for\n"); bad = 1; }
    }
    // ---- the same box seen from outside
    {
        Scene O = B;
        O.name = "outside";
        Tally T;
        unsigned long long p0[2] = {g_path[0], g_path[1]};
        for (int i = 0; i < 1000000; ++i) {
            V3 o{unif(-3, 3), unif(-3, 3), unif(-3, 3)}, d{unif(-1, 1), unif(-1, 1), unif(-1, 1)};
            check(O, o, d, kInf, &T);
        }
        bad |= paths("box, origins in [-3,3]^3, tMax inf", p0, 0., 0.10);
        for (int i = 0; i < 400000; ++i) {   // a camera outside, looking at the box
            V3 o{unif(-0.5f, 0.5f), unif(-0.5f, 0.5f), unif(-6.f, -2.f)}, g{unif(-1.2f, 1.2f), unif(-1.2f, 1.2f), unif(-1.2f, 1.2f)};
            check(O, o, g - o, (i % 4 == 3) ? unif(0.f, 2.f) : kInf, &T);
        }
        random_rays(O, &T, 300000, false);
        edge_and_corner_rays(O, &T, 50000, false);
        bad |= report(O, T, &total);
        if (T.hits < 300000 || T.ties < 10000) { printf("the outside view's rays miss the cases they are meant for\n"); bad = 1; }
    }
    // ---- a pair that differs in one in-plane field (the ceiling is shorter along x): not to be marked
    {
        const Quad q[2] = {box[0], {{-1, 1, -1}, {1.5f, 0, 0}, {0, 0, 2}, false}};
        Scene S;
        build(&S, "differs", q, 2, -1.f, 1.f);
        Tally T;
        random_rays(S, &T, 300000, true);
        random_rays(S, &T, 100000, false);
        special_rays(S, &T, 7);
        bad |= report(S, T, &total);
    }
    // ---- identical opposite walls that are not adjacent in the list: not to be marked
    {
        const Quad q[6] = {box[0], box[2], box[1], box[4], box[3], box[5]};
        Scene S;
        build(&S, "apart", q, 6, -1.f, 1.f);
        Tally T;
        random_rays(S, &T, 300000, true);
        random_rays(S, &T, 100000, false);
        edge_and_corner_rays(S, &T, 30000, true);
        special_rays(S, &T, 7);
        bad |= report(S, T, &total);
    }
    // ---- two coplanar identical records (one reversed, one with e1 and e2 traded): a candidate is a candidate of both, the first wins
    {
        const Quad q[3] = {{{0.25f, -1, -1}, {0, 2, 0}, {0, 0, 2}, false}, {{0.25f, -1, -1}, {0, 0, 2}, {0, 2, 0}, false}, box[0]};
        Scene S;
        build(&S, "coplanar", q, 3, -1.f, 1.f);
        Tally T;
        unsigned long long p0[2] = {g_path[0], g_path[1]};
        random_rays(S, &T, 300000, true);
        random_rays(S, &T, 100000, false);
        special_rays(S, &T, 7);
        bad |= report(S, T, &total);
        paths("coplanar", p0, 0., 0.);
        if (T.wins[1] != 0 || T.wins[0] < 50000) { printf("the second of two equal records won, or the first too rarely\n"); bad = 1; }
    }
    // ---- 16 records: pairs x G y z x G z y x -- every transition between two different frames, 0 -> 0 with and without a generic
    //      record in between; nested slabs of different sizes, every other pair with one wall's e1 / e2 traded, reversed or not
    {
        const int axis_of[9] = {0, -1, 1, 2, 0, -1, 2, 1, 0};
        Quad q[16];
        int n = 0, pair = 0;
        for (int e = 0; e < 9; ++e) {
            const int a = axis_of[e];
            if (a < 0) {
                const Quad g = {{-0.8f, -0.9f, n < 4 ? -0.3f : 0.4f}, {1.5f, 0.2f, n < 4 ? 0.6f : -0.5f}, {-0.1f, 1.7f, 0.3f}, n >= 4};
                q[n++] = g;
                continue;
            }
            const int a1 = (a + 1) % 3, a2 = (a + 2) % 3;
            const float half = 0.45f + 0.11f * pair, c1 = unif(-1.4f, -0.9f), c2 = unif(-1.4f, -0.9f), l1 = unif(1.9f, 2.6f), l2 = unif(1.9f, 2.6f);
            for (int w = 0; w < 2; ++w) {
                Quad r = {};
                const bool traded = ((pair + w) & 1) != 0 && (pair % 3 != 0 || w == 1);
                r.p00[a] = w ? half : -half - 0.02f * pair;
                r.p00[a1] = c1; r.p00[a2] = c2;
                if (traded) { r.e1[a2] = l2; r.e2[a1] = l1; } else { r.e1[a1] = l1; r.e2[a2] = l2; }
                r.reverse = ((pair >> 1) & 1) != w;
                q[n++] = r;
            }
            pair++;
        }
        if (n != 16) { printf("the list has %d records\n", n); return 1; }
        Scene S;
        build(&S, "list16", q, 16, -0.45f, 0.45f);
        Tally T;
        unsigned long long p0[2] = {g_path[0], g_path[1]};
        random_rays(S, &T, 1200000, true);
        random_rays(S, &T, 500000, false);
        special_rays(S, &T, 2);
        bad |= report(S, T, &total);
        paths("list16", p0, 0., 0.);
        int winners = 0;
        for (int k = 0; k < 16; ++k) winners += T.wins[k] > 0;
        if (winners != 16 || T.second < 100000) { printf("the list does not exercise every record\n"); bad = 1; }
    }
    printf("total %llu rays\n", total);
    if (total < 10000000ull) { printf("fewer than 10^7 rays\n"); bad = 1; }
    printf("result %s\n", bad ? "MISMATCH" : "identical");
    return bad;
}
"""

AXIS_ALIGNED, UV_SWAPPED, STEPS, TWIN, TWIN_SWAPPED = 8, 4, 3, 64, 128
# the first records of the pairs each scene's geometry dictates
EXPECTED = {"box": [0, 2, 4], "differs": [], "apart": [], "coplanar": [0], "list16": [0, 3, 5, 7, 10, 12, 14]}


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
    hook = _cut(src, r"^#if defined\(__HIP_DEVICE_COMPILE__\) \|\| !defined\(VSPG_RECT_TWIN_PATH\)\n.*?^#endif\n", "the path hook's default")
    twins = "".join([_function(src, "rect_twins_mark"), hook, _function(src, "rect_hit_uv_twins"), _function(src, "rects_closest_twins")])
    body = "".join([_function(src, "isect_rec_build"), _function(src, "beyond"), _function(src, "rect_frame"), _function(src, "rect_hit_uv"),
                    _function(src, "rects_closest"), twins])
    assert "asm" not in body
    # the two votes are all the device build has and the host build has not, and VSPG_RECT_TWIN_VOTE is the only host switch of the twin walk
    assert twins.count("__builtin_amdgcn_ballot_w64(") == twins.count("#elif VSPG_RECT_TWIN_VOTE == ") == 2
    assert "VSPG_RECT_VOTE_TAKEN" not in twins
    # every kernel family's closest hit goes through the twin walk, and the records are marked where they are built
    assert "rects_closest_twins(S.irec, S.n_quads, o, d, tMax" in _cut(src, r"^VLEAF Isect scene_intersect\(.*?^}\n", "scene_intersect")
    build_src = open(os.path.join(os.path.dirname(HDR), "vspg_scene_build.hip")).read()
    assert build_src.index("isect_rec_build(") < build_src.index("rect_twins_mark(D->irec, D->n_quads)") < build_src.index("rect_planes_build(")
    d = tmp_path_factory.mktemp("rect_twins")
    (d / "check.cpp").write_text(DRIVER.replace("@TYPES@", types).replace("@FUNCTIONS@", body))
    return d


def _run(source, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.fail("no host C++ compiler")
    exe = str(source / name)
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"] + flags + ["-o", exe, str(source / "check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print("\n".join(line for line in r.stdout.split("\n") if not line.startswith("rec ")))
    assert r.returncode == 0, r.stdout[-4000:]
    assert "result identical" in r.stdout
    return r.stdout


@pytest.fixture(scope="module")
def lane_run(source):
    """the output of the build whose votes are the lane itself: run once, read by two tests"""
    return _run(source, "check_lane", [])


def test_lane_alone_in_its_wavefront_keeps_every_bit(lane_run):
    assert "result identical" in lane_run


def test_lane_beside_a_candidate_keeps_every_bit(source):
    _run(source, "check_some", ["-DVSPG_RECT_TWIN_VOTE=1"])


def test_every_pair_falling_back_keeps_every_bit(source):
    out = _run(source, "check_both", ["-DVSPG_RECT_TWIN_VOTE=2"])
    assert re.search(r"paths box, origins inside, tMax inf: merged 0, fallback [1-9]", out)


def _records(out):
    """{scene: {"before": [(kind, axes, [14 words])], "after": [...]}} from the driver's `rec` lines"""
    scenes = {}
    for line in out.split("\n"):
        w = line.split()
        if len(w) == 20 and w[0] == "rec":
            lst = scenes.setdefault(w[1], {"before": [], "after": []})[w[2]]
            assert int(w[3]) == len(lst)
            lst.append((int(w[4]), int(w[5]), [int(x, 16) for x in w[6:]]))
    return scenes


def test_marked_pairs_are_the_pairs_found_independently(lane_run):
    scenes = _records(lane_run)
    assert sorted(scenes) == sorted(EXPECTED)
    for name, recs in scenes.items():
        before, after = recs["before"], recs["after"]
        assert len(before) == len(after) >= 2
        firsts, i = [], 0
        while i + 1 < len(before):
            (ka, xa, fa), (kb, xb, fb) = before[i], before[i + 1]
            assert xa < TWIN and xb < TWIN, "isect_rec_build's output is as it was: no new bit"
            if (ka == kb == 1 and xa & AXIS_ALIGNED and xb & AXIS_ALIGNED and (xa >> 4) & 3 == (xb >> 4) & 3 and xb & STEPS == 0
                    and fa[2:8] == fb[2:8]):
                firsts.append(i)
                i += 2
            else:
                i += 1
        assert firsts == EXPECTED[name], (name, firsts)
        for i, ((k0, x0, f0), (k1, x1, f1)) in enumerate(zip(before, after)):
            assert k0 == k1
            if i in firsts:
                partner = before[i + 1]
                assert x1 == x0 | TWIN | (TWIN_SWAPPED if partner[1] & UV_SWAPPED else 0), (name, i)
                assert f1[8] == partner[2][1] and f1[:8] == f0[:8] and f1[9:] == f0[9:], (name, i)
                assert struct.pack("<I", f1[8]) != struct.pack("<I", f0[1]) or name == "coplanar"
            else:
                assert (x1, f1) == (x0, f0), (name, i)   # the second of a pair and every other record: complete and unchanged
    # both (u, v) orders among the selected walls
    box = scenes["box"]["after"]
    assert any(x & TWIN and bool(x & TWIN_SWAPPED) != bool(x & UV_SWAPPED) for _, x, _ in box)
