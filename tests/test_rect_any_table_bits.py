"""The any-hit walk in two stages (csrc/vspg_device.h: RectPlanes, rect_planes_build, rects_any_planes) answers what the plain walk
over every record answered, for every ray; and the plane table holds what it is said to hold.

The header's text of the table, its builder and the two-stage walk is cut out as it stands and compiled for the host next to a frozen
copy of the walk it replaces (namespace parent below: rects_any and the rect_hit_uv it calls, with the host's vote written out as "the
lane itself" -- a lane's answer never depended on its neighbours, tests/test_rect_vote_bits.py).  The record builder, beyond,
rect_frame and the types come from the header for both.  On the device the votes are ballots; the host has no wavefront, so the
driver is built twice, as that test's is:

  * vote = the lane itself: a lane alone in its wavefront -- the pre-pass drops every record whose plane the lane cannot reach, and
    the answer must be the parent's all the same;
  * vote = always taken (-DVSPG_RECT_VOTE_TAKEN): a lane whose neighbours are candidates of everything -- every record is walked,
    in the table's order and not in index order, each test running its whole predicated body.

Rays (more than 10^7 per build): shadow rays inside the room towards points near and on the walls with tMax = 1 - eps, random rays
with random, infinite and tiny tMax, rays that start exactly on a record's plane (with d[a] = +-0 too), rays with zeros of both signs,
infinities, NaNs and denormals thrown into origin, direction and tMax, and for the small scenes every combination of nine special
values in the six ray components.  Scenes: the fog box (7 records, all axis-aligned); 16 records with planes on all three axes --
more than kPlaneChunk on two of them, whose last records are therefore walked without a pre-test --, two records on one plane and two
tilted (generic) records in the middle; one axis-aligned record; one generic record; two generic records and no axis-aligned one; no record.

The table test compares the lists, the listed and always-walked bits and the order with lists made independently from the scene's description, and
rebuilds a used table for another scene: it must equal the table built from scratch.  (Records are built in one place, build_dscene
at renderer creation, and the table right behind them; no call updates a scene's rectangles, so a second build over a used table is
all of "rebuilt after an update" that exists to test.)"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "vspg-pbrt-v4_amd", "csrc", "vspg_device.h")
API = os.path.join(ROOT, "include", "vspg.h")

# rects_any and its rect_hit_uv as they were before the plane table (frozen: this text is the reference and does not follow the header)
PARENT = r"""
namespace parent {
VDEV bool rect_hit_uv(const IsectRec &r, V3 o, V3 d, float tMax, float *tHit, float *uHit, float *vHit) {
    float num, denom, u, v, t;
    bool cand;
    if (r.axes & kIsectAxisAligned) {
        denom = d.x;
        num = r.f[1] - o.x;
        cand = (int32_t)(__builtin_bit_cast(uint32_t, num) ^ __builtin_bit_cast(uint32_t, denom)) >= 0;
        cand = cand & !beyond(num, denom, tMax);
        const bool some = cand;
        if (!some) return false;
        t = num / denom;
        cand = cand & (t > 0) & (t < tMax);
        float pu = o.y + d.y * t, pv = o.z + d.z * t;
        u = ((pu - r.f[2]) * r.f[4]) * r.f[6];
        v = ((pv - r.f[3]) * r.f[5]) * r.f[7];
    } else {
        V3 n = V3{r.f[0], r.f[1], r.f[2]}, p00 = V3{r.f[3], r.f[4], r.f[5]};
        denom = dot(n, d);
        num = dot(n, p00 - o);
        cand = ((num > 0) & (denom > 0)) | ((num < 0) & (denom < 0));
        cand = cand & !beyond(num, denom, tMax);
        const bool some = cand;
        if (!some) return false;
        t = num / denom;
        cand = cand & (t > 0) & (t < tMax);
        V3 p = o + d * t;
        V3 rel = p - p00;
        u = dot(rel, V3{r.f[6], r.f[7], r.f[8]}) * r.f[12];
        v = dot(rel, V3{r.f[9], r.f[10], r.f[11]}) * r.f[13];
    }
    cand = cand & !((u < 0) | (u > 1) | (v < 0) | (v > 1));
    *tHit = t;
    *uHit = u;
    *vHit = v;
    return cand;
}
VDEV bool rects_any(const IsectRec *recs, int n, V3 o, V3 d, float tMax) {
    bool any = false;
    V3 fo = o, fd = d;
    for (int i = 0; i < n; ++i) {
        const IsectRec &r = recs[i];
        float t, u, v;
        rect_frame(fo, fd, r.axes);
        any = any | rect_hit_uv(r, fo, fd, tMax, &t, &u, &v);
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
#define VSPG_MAX_QUADS @MAX_QUADS@
@TYPES@
VDEV void swap_regs(float &a, float &b) { const float t = a; a = b; b = t; }   // v_swap_b32
VDEV void here(float, float, float, float) {}                              // (where a scalar load stands: no arithmetic)
@SHARED@
@PARENT@
@FUNCTIONS@

static inline uint32_t f2b(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static inline float b2f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static inline uint32_t rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_state >> 32); }
static inline float unif(float lo, float hi) { return lo + (hi - lo) * (float)((rnd() >> 8) * (1.0 / 16777216.0)); }
static const float kInf = std::numeric_limits<float>::infinity();
static const float kNaN = std::numeric_limits<float>::quiet_NaN();
static float &at(V3 &v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }

// a scene as the renderer would build it: rectangles {p00, e1, e2, reverse} -> records in index order, then the table
struct Rect { float p00[3], e1[3], e2[3]; bool reverse; };
struct Scene {
    const char *name;
    std::vector<Rect> rects;
    IsectRec recs[VSPG_MAX_QUADS];
    RectPlanes planes;
    int n;
};
static void cross(const float *a, const float *b, float *c) {
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
static void finish(Scene &S) {
    S.n = (int)S.rects.size();
    int cur = 0;
    for (int i = 0; i < S.n; ++i) {
        const Rect &q = S.rects[i];
        float c[3], n[3];
        cross(q.e1, q.e2, c);
        const float len = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        for (int k = 0; k < 3; ++k) n[k] = q.reverse ? -(c[k] / len) : c[k] / len;
        const float inv_l1 = 1.f / (q.e1[0] * q.e1[0] + q.e1[1] * q.e1[1] + q.e1[2] * q.e1[2]);
        const float inv_l2 = 1.f / (q.e2[0] * q.e2[0] + q.e2[1] * q.e2[1] + q.e2[2] * q.e2[2]);
        std::memset(&S.recs[i], 0, sizeof S.recs[i]);
        cur = isect_rec_build(&S.recs[i], n, q.p00, q.e1, q.e2, inv_l1, inv_l2, cur);
    }
    std::memset(&S.planes, 0xAB, sizeof S.planes);   // the builder owes every byte
    rect_planes_build(&S.planes, S.recs, S.n);
}
static Rect rect(float px, float py, float pz, float ax, float ay, float az, float bx, float by, float bz, bool reverse = false) {
    return Rect{{px, py, pz}, {ax, ay, az}, {bx, by, bz}, reverse};
}
static Scene fog_box() {
    Scene S;
    S.name = "fog box";
    S.rects = {rect(-1, -1, -1, 0, 0, 2, 2, 0, 0), rect(-1, 1, -1, 2, 0, 0, 0, 0, 2), rect(-1, -1, 1, 0, 2, 0, 2, 0, 0),
               rect(-1, -1, -1, 2, 0, 0, 0, 2, 0), rect(-1, -1, -1, 0, 2, 0, 0, 0, 2), rect(1, -1, -1, 0, 0, 2, 0, 2, 0),
               rect(-0.25f, 0.999f, -0.25f, 0.5f, 0, 0, 0, 0, 0.5f)};
    finish(S);
    return S;
}
// the axes of the sixteen: x x y y z z x z | two tilted | y x z y z x; records 6 and 11 lie on one plane
static const int kAxisOf16[16] = {0, 0, 1, 1, 2, 2, 0, 2, -1, -1, 1, 0, 2, 1, 2, 0};
static Scene sixteen() {
    Scene S;
    S.name = "sixteen records";
    for (int i = 0; i < 16; ++i) {
        Rect q = rect(0, 0, 0, 0, 0, 0, 0, 0, 0, (i % 3) == 1);
        const int a = kAxisOf16[i];
        if (a >= 0) {
            const int order = (i * 7 / 3) & 1, a1 = order ? (a + 2) % 3 : (a + 1) % 3, a2 = order ? (a + 1) % 3 : (a + 2) % 3;
            q.p00[a] = (i == 11) ? -1.2f + 0.16f * 6 : -1.2f + 0.16f * i;
            q.p00[a1] = unif(-1.5f, -0.5f);
            q.p00[a2] = unif(-1.5f, -0.5f);
            q.e1[a1] = unif(1.2f, 2.4f);
            q.e2[a2] = unif(1.2f, 2.4f);
            if (i % 5 == 0) { q.p00[a1] += q.e1[a1]; q.e1[a1] = -q.e1[a1]; }
        } else {
            q = rect(-0.8f, -0.9f, i == 8 ? -0.3f : 0.4f, 1.5f, 0.2f, i == 8 ? 0.6f : -0.5f, -0.1f, 1.7f, 0.3f, i == 9);
        }
        S.rects.push_back(q);
    }
    finish(S);
    return S;
}
static Scene small(const char *name, int n_aligned, int n_generic) {
    Scene S;
    S.name = name;
    for (int i = 0; i < n_aligned; ++i) S.rects.push_back(rect(-1, 0.25f, -1, 2, 0, 0, 0, 0, 2));
    for (int i = 0; i < n_generic; ++i) S.rects.push_back(rect(-0.8f, -0.9f, i ? 0.4f : -0.3f, 1.5f, 0.2f, i ? -0.5f : 0.6f, -0.1f, 1.7f, 0.3f, i == 1));
    finish(S);
    return S;
}

struct Tally { unsigned long long rays = 0, anys = 0, bad = 0; };
static void check(const Scene &S, V3 o, V3 d, float tMax, Tally *T) {
    const bool a = rects_any_planes(S.planes, S.recs, o, d, tMax), b = parent::rects_any(S.recs, S.n, o, d, tMax);
    T->rays++;
    T->anys += b;
    if (a != b && T->bad++ < 6)
        printf("  %s: o %08x %08x %08x d %08x %08x %08x tMax %08x: new %d parent %d\n", S.name, f2b(o.x), f2b(o.y), f2b(o.z), f2b(d.x),
               f2b(d.y), f2b(d.z), f2b(tMax), a, b);
}
static const float kSpecials[] = {0.f, -0.f, kInf, -kInf, kNaN, b2f(1), b2f(0x80400000u), 1.f, -0.5f};
static const int kNs = (int)(sizeof kSpecials / sizeof kSpecials[0]);
static const float kTMaxes[] = {kInf, 1.f - 1e-4f, 1e-30f, b2f(3), 0.f, -0.f, kNaN, 0.375f, -1.f};
static const int kNt = (int)(sizeof kTMaxes / sizeof kTMaxes[0]);
static float special_or(float v, unsigned one_in) { return (rnd() % one_in) ? v : kSpecials[rnd() % 7]; }   // the seven non-ordinary ones

static Tally run(const Scene &S, long n_random, int combo_step) {
    Tally T;
    std::vector<int> aligned;
    for (int i = 0; i < S.n; ++i)
        if (S.recs[i].axes & kIsectAxisAligned) aligned.push_back(i);
    for (long i = 0; i < n_random; ++i) {
        V3 o{unif(-0.999f, 0.999f), unif(-0.999f, 0.999f), unif(-0.999f, 0.999f)}, d;
        float tMax;
        const int kind = (int)(i % 8);
        if (kind < 3) {   // a shadow ray: d = (a point near or on the room's walls) - o, tMax = 1 - eps
            V3 p{unif(-1.1f, 1.1f), unif(-1.1f, 1.1f), unif(-1.1f, 1.1f)};
            if (kind == 1) at(p, rnd() % 3) = (rnd() & 1) ? 1.f : -1.f;
            if (kind == 2) p = V3{unif(-0.25f, 0.25f), 0.999f, unif(-0.25f, 0.25f)};
            d = V3{p.x - o.x, p.y - o.y, p.z - o.z};
            tMax = 1.f - 1e-4f;
        } else {
            o = V3{unif(-2, 2), unif(-2, 2), unif(-2, 2)};
            d = V3{unif(-1, 1), unif(-1, 1), unif(-1, 1)};
            tMax = (i % 5 == 0) ? unif(0.f, 4.f) : ((i % 5 == 1) ? kTMaxes[rnd() % kNt] : kInf);
        }
        if (kind == 4 && !aligned.empty()) {   // the origin exactly on a record's plane; every fourth with d[a] = +-0
            const IsectRec &r = S.recs[aligned[rnd() % aligned.size()]];
            const int a = (r.axes >> kIsectAxisShift) & 3;
            at(o, a) = r.f[1];
            if (i % 32 == 4) at(d, a) = (i & 32) ? 0.f : -0.f;
        }
        if (kind == 5) {   // zeros, infinities, NaNs, denormals in some components
            o = V3{special_or(o.x, 4), special_or(o.y, 4), special_or(o.z, 4)};
            d = V3{special_or(d.x, 4), special_or(d.y, 4), special_or(d.z, 4)};
            tMax = (rnd() & 1) ? tMax : kTMaxes[rnd() % kNt];
        }
        check(S, o, d, tMax, &T);
    }
    if (combo_step > 0) {   // the special values in all six components: every combo_step-th combination, each at two tMax
        long total = 1;
        for (int j = 0; j < 6; ++j) total *= kNs;
        for (long i = 0; i < total; i += combo_step) {
            long k = i;
            float c[6];
            for (int j = 0; j < 6; ++j) { c[j] = kSpecials[k % kNs]; k /= kNs; }
            check(S, V3{c[0], c[1], c[2]}, V3{c[3], c[4], c[5]}, kTMaxes[i % kNt], &T);
            check(S, V3{c[0], c[1], c[2]}, V3{c[3], c[4], c[5]}, kTMaxes[(i / kNt) % kNt], &T);
        }
    }
    printf("%s: %d records, %llu rays, %llu any-hits, mismatches %llu\n", S.name, S.n, T.rays, T.anys, T.bad);
    return T;
}

static int rays() {
    const Scene box = fog_box(), many = sixteen(), one = small("one record", 1, 0), tilted = small("one tilted record", 0, 1),
                generic = small("no axis-aligned record", 0, 2), none = small("no record", 0, 0);
    unsigned long long total = 0, bad = 0;
    bool thin = false;
    Tally t = run(box, 4000000, 1);
    total += t.rays; bad += t.bad; thin = thin || t.anys < 200000 || t.anys > t.rays / 2;
    t = run(many, 4000000, 3);
    total += t.rays; bad += t.bad; thin = thin || t.anys < 200000;
    t = run(one, 1000000, 7);
    total += t.rays; bad += t.bad; thin = thin || t.anys < 20000;
    t = run(tilted, 500000, 49);
    total += t.rays; bad += t.bad; thin = thin || t.anys < 10000;
    t = run(generic, 500000, 49);
    total += t.rays; bad += t.bad; thin = thin || t.anys < 10000;
    t = run(none, 200000, 49);
    total += t.rays; bad += t.bad; thin = thin || t.anys != 0;
    printf("rays %llu mismatches %llu\n", total, bad);
    if (total < 10000000ull) { printf("fewer than 10^7 rays\n"); return 1; }
    if (thin) { printf("the rays do not exercise hits and misses as meant\n"); return 1; }
    return bad != 0;
}

// ---- the table ----------------------------------------------------------------------------------------------------------
static int expect_table(const Scene &S, const int *axis_of) {
    int bad = 0;
    int at_pos[32];   // the record each position should name, -1: none
    for (int p = 0; p < 32; ++p) at_pos[p] = -1;
    std::vector<bool> is_listed(S.n, false);
    uint32_t listed = 0, always = 0;
    for (int a = 0; a < 3; ++a) {
        int k = 0;
        for (int i = 0; i < S.n && k < kPlaneChunk; ++i)
            if (axis_of[i] == a) {
                if (f2b(S.planes.c[a][k]) != f2b(S.rects[i].p00[a])) { printf("  %s: plane %d of axis %d is %g, record %d lies at %g\n", S.name, k, a, S.planes.c[a][k], i, S.rects[i].p00[a]); bad++; }
                at_pos[kPlaneChunk * a + k + 1] = i;
                listed |= 1u << (kPlaneChunk * a + k + 1);
                is_listed[i] = true;
                k++;
            }
        for (; k < kPlaneChunk; ++k)
            if (f2b(S.planes.c[a][k]) != 0) { printf("  %s: unused slot %d of axis %d is not 0\n", S.name, k, a); bad++; }
    }
    int pos = 3 * kPlaneChunk + 1;   // the generic records and those past a full list, in index order
    for (int i = 0; i < S.n; ++i)
        if (!is_listed[i]) { always |= 1u << pos; at_pos[pos++] = i; }
    if (S.planes.listed != listed) { printf("  %s: listed bits %x, expected %x\n", S.name, S.planes.listed, listed); bad++; }
    if (S.planes.always != always) { printf("  %s: always-walked bits %x, expected %x\n", S.name, S.planes.always, always); bad++; }
    for (int p = 1; p < 32; ++p) {
        const int want = at_pos[p] < 0 ? 0 : at_pos[p], got = (int)((S.planes.order[(p - 1) >> 3] >> (4 * ((p - 1) & 7))) & 15);
        if (got != want) { printf("  %s: position %d names record %d, expected %d\n", S.name, p, got, want); bad++; }
    }
    return bad;
}
static int table() {
    int bad = 0;
    const Scene box = fog_box(), many = sixteen(), generic = small("no axis-aligned record", 0, 2), none = small("no record", 0, 0);
    const int box_axes[7] = {1, 1, 2, 2, 0, 0, 1}, generic_axes[2] = {-1, -1};
    bad += expect_table(box, box_axes);
    bad += expect_table(many, kAxisOf16);
    bad += expect_table(generic, generic_axes);
    bad += expect_table(none, generic_axes);
    // x and z hold five planes each (records 15 and 14 do not fit their lists), y exactly a full list, and two records are generic
    if (many.planes.listed != 0x1FFEu || many.planes.always != 0x1E000u) { printf("the sixteen do not overflow the lists as meant\n"); bad++; }
    if (f2b(many.planes.c[0][2]) != f2b(many.planes.c[0][3])) { printf("records 6 and 11 do not share a plane\n"); bad++; }
    // a scene update: the used table of one scene rebuilt for another equals that scene's own
    const Scene *seq[] = {&many, &box, &none, &generic, &many};
    RectPlanes T = many.planes;
    for (const Scene *S : seq) {
        rect_planes_build(&T, S->recs, S->n);
        if (std::memcmp(&T, &S->planes, sizeof T) != 0) { printf("  rebuilt for '%s': differs from the table built from scratch\n", S->name); bad++; }
    }
    printf("table: %d mismatches\n", bad);
    return bad != 0;
}

int main(int argc, char **argv) {
    const int r = (argc > 1 && !std::strcmp(argv[1], "table")) ? table() : rays();
    printf("result %s\n", r ? "MISMATCH" : "identical");
    return r;
}
"""


def _cut(src, pattern, what):
    m = re.search(pattern, src, re.S | re.M)
    assert m, "%s not found" % what
    return m.group(0)


def _function(src, name):
    return _cut(src, r"^(?:VDEV|inline) \w+ %s\(.*?^}\n" % name, name)


def _line(src, start):
    return _cut(src, r"^%s[^\n]*\n" % re.escape(start), start)


@pytest.fixture(scope="module")
def source(tmp_path_factory):
    src = open(HDR).read()
    max_quads = _cut(open(API).read(), r"^#define VSPG_MAX_QUADS (\d+)$", "VSPG_MAX_QUADS").split()[-1]
    types = "".join([_cut(src, r"^struct V3 \{.*?^};\n", "struct V3"),
                     _line(src, "VDEV V3 ld3("), _line(src, "VDEV V3 operator+(V3 a, V3 b)"), _line(src, "VDEV V3 operator-(V3 a, V3 b)"),
                     _line(src, "VDEV V3 operator*(V3 a, float s)"), _line(src, "VDEV float dot(V3 a, V3 b)"),
                     _cut(src, r"^enum \{ kIsectStepsMask.*?\n", "the record's flag bits"),
                     _cut(src, r"^struct IsectRec \{.*?^};\n", "struct IsectRec"),
                     _line(src, "constexpr int kPlaneChunk"),
                     _cut(src, r"^struct RectPlanes \{.*?^};\n", "struct RectPlanes")])
    shared = "".join([_function(src, "isect_rec_build"), _function(src, "beyond"), _function(src, "rect_frame")])
    body = "".join([_function(src, "rect_planes_build"), _function(src, "rect_hit_uv"), _function(src, "plane_vote"), _function(src, "axis_votes"),
                    _function(src, "rects_any_planes")])
    assert "asm" not in body
    # the votes are the only thing the device build has and the host build has not, and VSPG_RECT_VOTE_TAKEN the only host switch
    assert body.count("#if defined(__HIP_DEVICE_COMPILE__)") == body.count("#elif defined(VSPG_RECT_VOTE_TAKEN)") == body.count("#endif") >= 1
    assert body.count("__ballot(") + body.count("__builtin_amdgcn_ballot_w64(same) & __builtin_amdgcn_ballot_w64(within)") == body.count("#if")
    # the kernels' any-hit query goes through the two-stage walk
    assert "rects_any_planes(S.planes, S.irec, o, d, tMax)" in _cut(src, r"^VLEAF bool scene_intersect_any\(.*?^}\n", "scene_intersect_any")
    d = tmp_path_factory.mktemp("rect_any_table")
    (d / "check.cpp").write_text(DRIVER.replace("@MAX_QUADS@", max_quads).replace("@TYPES@", types).replace("@SHARED@", shared)
                                 .replace("@PARENT@", PARENT).replace("@FUNCTIONS@", body))
    return d


def _build(source, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.fail("no host C++ compiler")
    exe = str(source / name)
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"] + flags + ["-o", exe, str(source / "check.cpp")], check=True)
    return exe


def _run(exe, *args):
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "result identical" in r.stdout


def test_lane_alone_in_its_wavefront_gets_the_plain_walks_answer(source):
    _run(_build(source, "check_identity", []))


def test_lane_beside_candidates_of_everything_gets_the_plain_walks_answer(source):
    _run(_build(source, "check_taken", ["-DVSPG_RECT_VOTE_TAKEN"]))


def test_plane_table_lists_order_and_rebuilt_over_a_used_table(source):
    _run(_build(source, "check_table", []), "table")
