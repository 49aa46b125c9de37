"""Work the path kernels no longer do, held bit for bit against the text that did it (csrc/vspg_path.h, csrc/vspg_device.h).

The functions are cut out of the headers as they stand and compiled for the host (-ffp-contract=off as the device build, the bit
casts as memcpy, the one instruction of swap_regs restated as a plain exchange).

1. light_pdf_li_hit against light_pdf_li.  An emitter hit by a non-specular path used to intersect the light again from an origin
   rebuilt out of the previous vertex; the rectangles-only kernels now take the hit point scene_intersect delivered.  The driver
   walks what the kernel walks -- previous vertex, the ray origin vertex_tail stores (offset_ray_origin after a surface vertex,
   the vertex itself after a medium vertex), the record test rect_hit_uv in the record's frame, quad_point -- and compares the
   two pdfs on every triple that hits: >= 10^7 of them over axis-aligned lights on every axis and in both edge orders, a light
   in the plane x = 0 (perr.x == 0: a zero's sign survives the interval), tilted lights, surface and medium previous vertices,
   both faces of one- and two-sided lights, and rays with +-0 components from vertices with +-0 components.
2. medium_ray_origin against offset_ray_origin(p3i_exact(p), 0, w): every combination of +-0, denormals, +-FLT_MAX, +-inf, NaN and
   ordinary values in p, with ordinary and special w, and 10^7 random (p, w).  The plain `mid() + 0` is held against it as well:
   it must agree on every finite p and is counted where it does not on the others (it misses the NaN an infinity makes of err).
3. sincosf_host_exact (csrc/vspg_libm.h, included as it stands) against sinf_host_exact and cosf_host_exact: every float in [0, 8]
   and its negative -- the range tests/test_libm_model.py::test_sincos_exhaustive pins the two against the host's libm on -- plus
   a stride through every other bit pattern (the out-of-scope arguments among them, which take the host branch here)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vspg-pbrt-v4_amd", "csrc")

PRELUDE = r"""
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#define VDEV static inline
static inline uint32_t f2b(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static inline float b2f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static const float kInf = std::numeric_limits<float>::infinity();
static inline bool isinf_(float x) { return std::isinf(x); }
static inline float wrcp(float b) { return 1 / b; }
static inline float wdiv(float a, float b) { return a / b; }
@TYPES@
VDEV void swap_regs(float &a, float &b) { const float t = a; a = b; b = t; }   // v_swap_b32
@FUNCTIONS@
static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static inline uint32_t rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_state >> 32); }
static inline float unif(float lo, float hi) { return lo + (hi - lo) * (float)((rnd() >> 8) * (1.0 / 16777216.0)); }
static inline bool same3(V3 a, V3 b) { return f2b(a.x) == f2b(b.x) && f2b(a.y) == f2b(b.y) && f2b(a.z) == f2b(b.z); }
"""

EMITTER_DRIVER = PRELUDE + r"""
// what build_dscene derives of a rectangle
struct Light { DQuad q; IsectRec rec; };
static void crossf(const float *a, const float *b, float *c) {
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
static void make_quad(Light *L, const float *p00, const float *e1, const float *e2, bool reverse, bool two_sided) {
    std::memset(L, 0, sizeof *L);
    float c[3];
    crossf(e1, e2, c);
    const float len = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    const float g6 = (6 * 0x1p-24f) / (1 - 6 * 0x1p-24f);
    for (int k = 0; k < 3; ++k) {
        L->q.p00[k] = p00[k]; L->q.e1[k] = e1[k]; L->q.e2[k] = e2[k];
        L->q.p10[k] = p00[k] + e1[k]; L->q.p01[k] = p00[k] + e2[k]; L->q.p11[k] = L->q.p10[k] + e2[k];
        L->q.n[k] = c[k] / len;
        if (reverse) L->q.n[k] = -L->q.n[k];
        L->q.perr[k] = (std::fabs(L->q.p00[k]) + std::fabs(L->q.p01[k]) + std::fabs(L->q.p10[k]) + std::fabs(L->q.p11[k])) * g6;
    }
    L->q.area = len;
    L->q.inv_l1 = 1.f / (e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
    L->q.inv_l2 = 1.f / (e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
    L->q.two_sided = two_sided;
    L->q.is_light = 1;
    isect_rec_build(&L->rec, L->q.n, L->q.p00, L->q.e1, L->q.e2, L->q.inv_l1, L->q.inv_l2, 0);
}
struct Tally { unsigned long long triples = 0, hits = 0, bad = 0, ref_zero = 0, zero_sign_points = 0, front = 0, back = 0; };
// one (previous vertex, direction, light) triple as the kernel walks it.  prev: the rectangle of a surface vertex, or null
static void triple(const Light &L, const Light *prev, V3 pp, V3 wi, Tally *T) {
    LsCtx ctx;
    V3 ro;
    if (prev) {  // PrevCtx::expand / vertex_tail: the same p3i_from_err(p, perr), the same n
        ctx.pi = p3i_from_err(pp, ld3(prev->q.perr));
        ctx.n = ld3(prev->q.n);
        ro = offset_ray_origin(ctx.pi, ctx.n, wi);
    } else {
        ctx.pi = p3i_exact(pp);
        ctx.n = V3{0, 0, 0};
        ro = pp;
    }
    T->triples++;
    V3 fo = ro, fd = wi;
    float t, u, v;
    rect_frame(fo, fd, L.rec.axes);
    if (!rect_hit_uv(L.rec, fo, fd, kInf, &t, &u, &v)) return;
    const bool swapped = (L.rec.axes & kIsectUvSwapped) != 0;
    const V3 pHit = quad_point(L.q, swapped ? v : u, swapped ? u : v);   // scene_intersect: Isect::p
    T->hits++;
    (dot(ld3(L.q.n), wi) < 0 ? T->front : T->back)++;
    const float a = light_pdf_li_hit(L.q, ctx, wi, pHit), b = light_pdf_li(L.q, ctx, wi);
    T->ref_zero += b == 0;
    {   // how often the point light_pdf_li finds differs from pHit (in a zero's sign only, or the pdfs below differ)
        float t2;
        V3 p2;
        if (quad_intersect(L.q, offset_ray_origin(ctx.pi, ctx.n, wi), wi, kInf, &t2, &p2) && !same3(p2, pHit)) T->zero_sign_points++;
    }
    if (f2b(a) != f2b(b) && T->bad++ < 8)
        printf("  pdf %08x against %08x: prev %s p %08x %08x %08x wi %08x %08x %08x\n", f2b(a), f2b(b), prev ? "surface" : "medium", f2b(pp.x),
               f2b(pp.y), f2b(pp.z), f2b(wi.x), f2b(wi.y), f2b(wi.z));
}
static V3 norm3(V3 a) { const float l = std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z); return V3{a.x / l, a.y / l, a.z / l}; }
static float &at(V3 &v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }

int main() {
    // the lights: axis-aligned on each axis in both edge orders (the second of each pair reversed), one in the plane x = 0, two tilted
    Light lights[9];
    int nl = 0;
    for (int a = 0; a < 3; ++a)
        for (int order = 0; order < 2; ++order) {
            const int a1 = order ? (a + 2) % 3 : (a + 1) % 3, a2 = order ? (a + 1) % 3 : (a + 2) % 3;
            float p00[3], e1[3] = {0, 0, 0}, e2[3] = {0, 0, 0};
            p00[a] = order ? 0.98f : -0.375f; p00[a1] = -0.3f; p00[a2] = 0.2f;
            e1[a1] = order ? 0.47f : -0.5f; e2[a2] = 0.6f;
            make_quad(&lights[nl++], p00, e1, e2, order != 0, ((a + order) & 1) != 0);
        }
    {
        // p00.x = -0 and both extents negative: at the corner u = v = -0 the record test's point has x = -0 where the plane formula's
        // (u = v = +0) has +0 -- the one place the two hit points differ
        const float p00[3] = {-0.f, 0.25f, 0.5f}, e1[3] = {0, -0.5f, 0}, e2[3] = {0, 0, -1.f};
        make_quad(&lights[nl++], p00, e1, e2, false, true);
    }
    {
        const float p00[3] = {-0.3f, 0.9f, -0.2f}, e1[3] = {0.5f, 0.1f, 0.05f}, e2[3] = {-0.02f, 0.12f, 0.45f};
        make_quad(&lights[nl++], p00, e1, e2, false, false);
        const float q00[3] = {0.4f, -0.1f, 0.3f}, f1[3] = {0.3f, 0.3f, 0.f}, f2[3] = {0.f, 0.f, -0.7f};
        make_quad(&lights[nl++], q00, f1, f2, true, true);
    }
    for (int i = 0; i < nl; ++i) {
        const bool aligned = (lights[i].rec.axes & kIsectAxisAligned) != 0;
        if (aligned != (i < 7)) { printf("light %d: record kind %d\n", i, lights[i].rec.kind); return 1; }
    }
    // the surfaces previous vertices lie on: the walls of a box around the lights and a tilted one
    Light walls[4];
    {
        const float a00[3] = {-1, -1, -1}, a1[3] = {2, 0, 0}, a2[3] = {0, 0, 2};         // floor y = -1
        make_quad(&walls[0], a00, a1, a2, true, false);
        const float b00[3] = {-1, -1, -1}, b1[3] = {0, 2, 0}, b2[3] = {0, 0, 2};         // wall x = -1
        make_quad(&walls[1], b00, b1, b2, false, false);
        const float c00[3] = {-1, -1, 0}, c1[3] = {2, 0, 0}, c2[3] = {0, 2, 0};          // wall z = 0: perr.z == 0
        make_quad(&walls[2], c00, c1, c2, false, false);
        const float d00[3] = {-0.9f, -0.8f, 0.7f}, d1[3] = {1.5f, 0.2f, 0.3f}, d2[3] = {-0.1f, 1.4f, 0.2f};
        make_quad(&walls[3], d00, d1, d2, false, false);
    }
    Tally T;
    unsigned long long hits_of[9][2] = {};
    for (int i = 0; i < nl; ++i) {
        const Light &L = lights[i];
        for (int it = 0; it < 1800000; ++it) {
            const int kind = it & 1;   // 0: medium vertex, 1: surface vertex
            const Light *prev = kind ? &walls[(it >> 1) & 3] : nullptr;
            V3 pp;
            if (prev) pp = quad_point(prev->q, unif(0, 1), unif(0, 1));
            else pp = V3{unif(-1, 1), unif(-1, 1), unif(-1, 1)};
            V3 wi;
            if (it % 8 == 7) {
                wi = norm3(V3{unif(-1, 1), unif(-1, 1), unif(-1, 1)});   // anywhere
            } else {
                const V3 target = quad_point(L.q, unif(-0.05f, 1.05f), unif(-0.05f, 1.05f));
                wi = target - pp;
                if (it % 8 < 6) wi = norm3(wi);   // (a quarter of the aimed rays keep their length)
            }
            const unsigned long long h0 = T.hits;
            triple(L, prev, pp, wi, &T);
            hits_of[i][kind] += T.hits - h0;
        }
        // zeros: medium vertices with +-0 components, rays along an axis with +-0 in the other two components
        for (int it = 0; it < 60000; ++it) {
            V3 pp{unif(-1, 1), unif(-1, 1), unif(-1, 1)};
            // (a target on an edge or a corner now and then: u or v exactly 0 or 1)
            V3 target = quad_point(L.q, (it & 512) ? (float)((it >> 10) & 1) : unif(0, 1), (it & 2048) ? (float)((it >> 12) & 1) : unif(0, 1));
            V3 wi = target - pp;
            const int ax = it % 3;
            for (int k = 0; k < 3; ++k)
                if (k != ax) {
                    at(pp, k) = (it & (8 << k)) ? -0.f : 0.f;
                    if (it & 4) { at(pp, k) = at(target, k); at(wi, k) = (it & (64 << k)) ? -0.f : 0.f; }
                    else at(wi, k) = at(target, k) - at(pp, k);
                }
            if (it & 1) wi = norm3(wi);
            triple(L, nullptr, pp, wi, &T);
        }
    }
    printf("emitter hits: %llu triples, %llu hit (%llu on the front face, %llu on the back), reference pdf 0 on %llu, "
           "hit points that differ from the re-intersection's (a zero's sign) %llu, pdf mismatches %llu\n",
           T.triples, T.hits, T.front, T.back, T.ref_zero, T.zero_sign_points, T.bad);
    for (int i = 0; i < nl; ++i) {
        printf("  light %d (%s, %s): hits after a medium vertex %llu, after a surface vertex %llu\n", i, i < 7 ? "axis-aligned" : "tilted",
               lights[i].q.two_sided ? "two-sided" : "one-sided", hits_of[i][0], hits_of[i][1]);
        if (hits_of[i][0] < 100000 || hits_of[i][1] < 100000) { printf("too few hits on light %d\n", i); return 1; }
    }
    if (T.hits < 10000000ull || T.front < 1000000ull || T.back < 1000000ull) { printf("too few hits\n"); return 1; }
    if (T.zero_sign_points == 0) { printf("no hit point differs from the re-intersection's in a zero's sign: the case the light at x = -0 is there for\n"); return 1; }
    printf("result %s\n", T.bad ? "MISMATCH" : "identical");
    return T.bad != 0;
}
"""

ORIGIN_DRIVER = PRELUDE + r"""
static V3 plain(P3i pi) { return pi.mid() + V3{0.f, 0.f, 0.f}; }
struct Tally { unsigned long long n = 0, bad = 0, plain_bad_finite = 0, plain_bad_other = 0; };
static void check(V3 p, V3 w, Tally *T) {
    const P3i pi = p3i_exact(p);
    const V3 ref = offset_ray_origin(pi, V3{0.f, 0.f, 0.f}, w), got = medium_ray_origin(pi), pl = plain(pi);
    T->n++;
    if (!same3(ref, got) && T->bad++ < 8)
        printf("  p %08x %08x %08x w %08x %08x %08x: %08x %08x %08x against %08x %08x %08x\n", f2b(p.x), f2b(p.y), f2b(p.z), f2b(w.x), f2b(w.y),
               f2b(w.z), f2b(got.x), f2b(got.y), f2b(got.z), f2b(ref.x), f2b(ref.y), f2b(ref.z));
    if (!same3(ref, pl)) {
        if (std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z)) T->plain_bad_finite++;
        else T->plain_bad_other++;
    }
}
int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), fmax = std::numeric_limits<float>::max();
    const float specials[] = {0.f, -0.f, b2f(1), b2f(0x80000001u), b2f(0x007fffffu), b2f(0x807fffffu), b2f(0x00800000u), fmax, -fmax,
                              fmax / 2, b2f(0x7f000001u), kInf, -kInf, nan, -nan, b2f(0x7f800001u), 1.f, -0.3f};
    const int ns = (int)(sizeof specials / sizeof specials[0]);
    const V3 ws[] = {{0.3f, -0.5f, 0.8f}, {0.f, -0.f, 1.f}, {-1.f, -2.f, -3.f}, {kInf, 1.f, -kInf}, {nan, 0.f, 1.f}, {-0.f, -0.f, -0.f},
                     {fmax, -fmax, b2f(1)}};
    Tally T;
    for (int i = 0; i < ns * ns * ns; ++i)
        for (const V3 &w : ws) check(V3{specials[i % ns], specials[(i / ns) % ns], specials[i / (ns * ns)]}, w, &T);
    const unsigned long long n_special = T.n;
    for (int i = 0; i < 10000000; ++i) {
        V3 p, w;
        if (i % 4 == 0) {   // any bit pattern in p: every exponent, NaNs and infinities among them
            p = V3{b2f(rnd()), b2f(rnd()), b2f(rnd())};
            w = V3{b2f(rnd()), b2f(rnd()), b2f(rnd())};
        } else {
            p = V3{unif(-2, 2), unif(-2, 2), unif(-2, 2)};
            w = V3{unif(-1, 1), unif(-1, 1), unif(-1, 1)};
        }
        check(p, w, &T);
    }
    printf("medium ray origin: %llu special and %llu random (p, w), mismatches %llu; the plain mid() + 0 differs on %llu finite p "
           "and on %llu p with an infinite or NaN component\n", n_special, T.n - n_special, T.bad, T.plain_bad_finite, T.plain_bad_other);
    if (T.plain_bad_finite) { printf("the plain form must hold on finite points\n"); return 1; }
    printf("result %s\n", T.bad ? "MISMATCH" : "identical");
    return T.bad != 0;
}
"""


SINCOS_DRIVER = r"""
#include <math.h>
#include <stdint.h>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>
#include "vspg_libm.h"
static inline uint32_t f2b(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static inline float b2f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static bool same(float a, float b) { return f2b(a) == f2b(b) || (a != a && b != b); }   // (a NaN of the host's sin / cos: any NaN)
static unsigned long long check(uint32_t bits) {
    const float y = b2f(bits);
    float s, c;
    vspg_libm::sincosf_host_exact(y, &s, &c);
    return !same(s, vspg_libm::sinf_host_exact(y)) || !same(c, vspg_libm::cosf_host_exact(y));
}
int main() {
    const uint32_t hi = f2b(8.0f);
    const unsigned hc = std::thread::hardware_concurrency();
    const int nt = hc < 1 ? 1 : (hc > 16 ? 16 : (int)hc);
    std::vector<unsigned long long> bad(nt, 0), n(nt, 0);
    std::vector<std::thread> th;
    for (int k = 0; k < nt; ++k)
        th.emplace_back([&, k] {
            for (uint64_t u = k; u <= hi; u += nt) { bad[k] += check((uint32_t)u) + check((uint32_t)u | 0x80000000u); n[k] += 2; }
            for (uint64_t u = k * 997; u < (1ull << 32); u += 997 * nt) { bad[k] += check((uint32_t)u); n[k]++; }
        });
    for (auto &t : th) t.join();
    unsigned long long b = 0, m = 0;
    for (int k = 0; k < nt; ++k) { b += bad[k]; m += n[k]; }
    printf("sin / cos pair: %llu arguments, mismatches %llu\n", m, b);
    printf("result %s\n", b ? "MISMATCH" : "identical");
    return b != 0;
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


def _struct(src, name):
    return _cut(src, r"^struct %s \{.*?^};\n" % name, "struct " + name)


def _device_text():
    dev = open(os.path.join(CSRC, "vspg_device.h")).read()
    types = "".join([_struct(dev, "V3"), _line(dev, "VDEV V3 ld3("), _line(dev, "VDEV V3 operator+(V3 a, V3 b)"),
                     _line(dev, "VDEV V3 operator-(V3 a, V3 b)"), _line(dev, "VDEV V3 operator-(V3 a)"), _line(dev, "VDEV V3 operator*(V3 a, float s)"),
                     _line(dev, "VDEV V3 vabs("), _line(dev, "VDEV float sqr("), _line(dev, "VDEV float dot(V3 a, V3 b)"),
                     _line(dev, "VDEV float absdot("), _line(dev, "VDEV float len2("),
                     _struct(dev, "DQuad"), _cut(dev, r"^enum \{ kIsectStepsMask.*?\n", "the record's flag bits"), _struct(dev, "IsectRec")])
    body = "".join([_function(dev, "next_float_up"), _function(dev, "next_float_down"), _struct(dev, "P3i").replace("VDEV ", ""), _line(dev, "VDEV P3i p3i_exact("),
                    _function(dev, "interval_ve"), _function(dev, "p3i_from_err"), _function(dev, "offset_axis"), _function(dev, "offset_ray_origin"),
                    _function(dev, "medium_ray_origin")])
    return dev, types, body


def _build(tmp_path_factory, name, driver, types, body):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.fail("no host C++ compiler")
    assert "asm" not in body, "only swap_regs may hold an instruction by name; the driver restates that one function"
    d = tmp_path_factory.mktemp(name)
    (d / "check.cpp").write_text(driver.replace("@TYPES@", types).replace("@FUNCTIONS@", body))
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-o", str(d / "check"), str(d / "check.cpp")], check=True)
    return str(d / "check")


def _run(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "result identical" in r.stdout


@pytest.fixture(scope="module")
def emitter_checker(tmp_path_factory):
    dev, types, body = _device_text()
    path = open(os.path.join(CSRC, "vspg_path.h")).read()
    body += "".join([_function(dev, "isect_rec_build"), _function(dev, "beyond"), _line(dev, "VDEV float comp(V3 v, int axis)"),
                     _function(dev, "rect_frame"), _function(dev, "rect_hit_uv"), _function(dev, "quad_hit_uv"), _line(dev, "VDEV V3 quad_point("),
                     _function(dev, "quad_intersect"), _struct(path, "LsCtx"), _function(path, "light_pdf_li"), _function(path, "light_pdf_li_hit")])
    return _build(tmp_path_factory, "emitter_hit", EMITTER_DRIVER, types, body)


@pytest.fixture(scope="module")
def origin_checker(tmp_path_factory):
    _, types, body = _device_text()
    return _build(tmp_path_factory, "medium_origin", ORIGIN_DRIVER, types, body)


def test_emitter_hit_pdf_from_the_hit_point_keeps_every_bit(emitter_checker):
    _run(emitter_checker)


def test_medium_ray_origin_is_offset_ray_origin_with_a_zero_normal(origin_checker):
    _run(origin_checker)


@pytest.fixture(scope="module")
def sincos_checker(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("sincos_pair")
    (d / "check.cpp").write_text(SINCOS_DRIVER)
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-I", CSRC, "-o", str(d / "check"), str(d / "check.cpp")],
                   check=True)
    return str(d / "check")


def test_sin_cos_pair_is_the_two_functions(sincos_checker):
    _run(sincos_checker)
