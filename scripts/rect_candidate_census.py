"""How many rectangle records a closest-hit walk of the fog box really tests, per ray and per 64-ray group, with and without twin
pairs merged (csrc/vspg_device.h: rects_closest, rect_twins_mark, rects_closest_twins):
    python scripts/rect_candidate_census.py > profiles/rect_twins_census.txt
No GPU.  The header's own text (isect_rec_build, rect_twins_mark, beyond, rect_frame, rect_hit_uv) is compiled for the host, as
tests/test_rect_twins_bits.py does, into a driver that walks paths through vspg_scene_fog_box's seven rectangles and counts, for
every path segment's closest-hit walk:
  - the records the ray is a candidate of (rect_hit_uv's sign and range pre-tests, with the running closest distance);
  - the record bodies a 64-ray group runs in the plain walk (a body runs as soon as one lane is a candidate);
  - the bodies it runs with twins merged (one per pair unless some lane is a candidate of both walls), and how often a pair falls back.
The oracle hands out radiances, not segments, so the paths are the driver's own: the benchmark's camera (eye (0, 0, -0.95), 60
degrees, 1920 x 1080), the fog box's medium (sigma_t 0.5, isotropic), free flights sampled from the exponential, cosine-weighted
bounces off the walls, the App.-F depth limit, no Russian roulette; a path ends on the light.  Their mean length is printed next to
the benchmark's mean_segments_per_path so the two can be compared.  A group is 64 consecutive segments of an 8 x 8 pixel tile
(segments ordered by depth, then pixel): what a wavefront holds once finished lanes are refilled from the same tile."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

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
@TYPES@
VDEV void swap_regs(float &a, float &b) { const float t = a; a = b; b = t; }
@FUNCTIONS@
static uint64_t g_state = 0x853C49E6748FEA9Bull;
static inline uint32_t rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_state >> 32); }
static inline float u01() { return (float)((rnd() >> 8) * (1.0 / 16777216.0)); }
static const float kInf = std::numeric_limits<float>::infinity();
struct Quad { float p00[3], e1[3], e2[3]; };
struct Seg { V3 o, d; int depth; };
static bool pretest(float plane, V3 o, V3 d, float bt) {
    const float num = plane - o.x;
    uint32_t a, b;
    std::memcpy(&a, &num, 4); std::memcpy(&b, &d.x, 4);
    return (int32_t)(a ^ b) >= 0 && !beyond(num, d.x, bt);
}
struct Count { double rays = 0, cands = 0, groups = 0, plain = 0, twins = 0, entries = 0, pairs = 0, fallbacks = 0; };
int main(int argc, char **argv) {
    const int maxdepth = argc > 1 ? atoi(argv[1]) : 5, tiles = argc > 2 ? atoi(argv[2]) : 64;
    const Quad box[7] = {{{-1, -1, -1}, {0, 0, 2}, {2, 0, 0}}, {{-1, 1, -1}, {2, 0, 0}, {0, 0, 2}}, {{-1, -1, 1}, {0, 2, 0}, {2, 0, 0}},
                         {{-1, -1, -1}, {2, 0, 0}, {0, 2, 0}}, {{-1, -1, -1}, {0, 2, 0}, {0, 0, 2}}, {{1, -1, -1}, {0, 0, 2}, {0, 2, 0}},
                         {{-0.25f, 0.999f, -0.25f}, {0.5f, 0, 0}, {0, 0, 0.5f}}};
    const int N = 7;
    IsectRec recs[N];
    V3 normal[N];
    int cur = 0;
    for (int i = 0; i < N; ++i) {
        const float *a = box[i].e1, *b = box[i].e2;
        float n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
        const float len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        for (int k = 0; k < 3; ++k) n[k] /= len;
        normal[i] = V3{n[0], n[1], n[2]};
        std::memset(&recs[i], 0, sizeof recs[i]);
        cur = isect_rec_build(&recs[i], n, box[i].p00, a, b, 1.f / (a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), 1.f / (b[0] * b[0] + b[1] * b[1] + b[2] * b[2]), cur);
    }
    rect_twins_mark(recs, N);
    int n_pairs = 0;
    for (int i = 0; i < N; ++i) n_pairs += (recs[i].axes & kIsectTwin) != 0;
    printf("records %d, twin pairs %d: a walk has %d entries with every pair merged\n", N, n_pairs, N - n_pairs);
    const float sigma_t = 0.5f, W = 1920, H = 1080, tanh = std::tan(30.f * 3.14159265f / 180.f);
    Count C[2];   // [0] groups of primary rays only, [1] every other group
    double n_paths = 0, n_segs = 0;
    for (int tile = 0; tile < tiles; ++tile) {
        const int tx = (int)(u01() * (W / 8)), ty = (int)(u01() * (H / 8));
        std::vector<Seg> segs;
        for (int lane = 0; lane < 64; ++lane) {
            const float px = 8 * tx + lane % 8 + u01(), py = 8 * ty + lane / 8 + u01();
            V3 o{0, 0, -0.95f}, d{(2 * px / W - 1) * tanh * (W / H), (1 - 2 * py / H) * tanh, 1.f};
            n_paths++;
            for (int depth = 0; depth < maxdepth; ++depth) {
                segs.push_back(Seg{o, d, depth});
                float t, u, v;
                int prim;
                const bool hit = rects_closest(recs, N, o, d, kInf, &t, &prim, &u, &v);
                const float len = std::sqrt(d.x * d.x + d.y * d.y + d.z * d.z), s = -std::log(1.f - u01()) / sigma_t / len;
                const float u1 = u01(), u2 = u01();
                if (hit && s >= t) {   // a wall: cosine-weighted bounce, the origin a little off the wall; the light ends the path
                    if (prim == 6) break;
                    const V3 p = o + d * t, n = normal[prim];
                    const float r = std::sqrt(u1), phi = 6.2831853f * u2, z = std::sqrt(1.f - u1);
                    const V3 a = std::fabs(n.x) > 0.5f ? V3{0, 1, 0} : V3{1, 0, 0};
                    V3 b{n.y * a.z - n.z * a.y, n.z * a.x - n.x * a.z, n.x * a.y - n.y * a.x};
                    const V3 c{n.y * b.z - n.z * b.y, n.z * b.x - n.x * b.z, n.x * b.y - n.y * b.x};
                    o = p + n * 1e-4f;
                    d = b * (r * std::cos(phi)) + c * (r * std::sin(phi)) + n * z;
                } else if (!hit) {
                    break;
                } else {               // a scattering event in the fog: isotropic
                    o = o + d * s;
                    const float z = 1.f - 2.f * u1, r = std::sqrt(1.f - z * z), phi = 6.2831853f * u2;
                    d = V3{r * std::cos(phi), r * std::sin(phi), z};
                }
            }
        }
        n_segs += segs.size();
        std::vector<Seg> order;
        for (int depth = 0; depth < maxdepth; ++depth)
            for (const Seg &s : segs) if (s.depth == depth) order.push_back(s);
        for (size_t g0 = 0; g0 < order.size(); g0 += 64) {
            const int n = (int)std::min<size_t>(64, order.size() - g0);
            bool primary = true;
            V3 fo[64], fd[64];
            float bt[64];
            for (int l = 0; l < n; ++l) { fo[l] = order[g0 + l].o; fd[l] = order[g0 + l].d; bt[l] = kInf; primary = primary && order[g0 + l].depth == 0; }
            Count &K = C[primary ? 0 : 1];
            K.groups++;
            K.rays += n;
            bool anyA_first = false, anyAB = false, both = false;
            for (int i = 0; i < N; ++i) {
                const IsectRec &r = recs[i];
                const bool twin = (r.axes & kIsectTwin) != 0, second = i > 0 && (recs[i - 1].axes & kIsectTwin) != 0;
                bool any = false, anyB = false, anyBoth = false;
                for (int l = 0; l < n; ++l) {
                    rect_frame(fo[l], fd[l], r.axes);
                    const bool a = pretest(r.f[1], fo[l], fd[l], bt[l]), b = twin && pretest(r.f[8], fo[l], fd[l], bt[l]);
                    any |= a; anyB |= b; anyBoth |= a && b;
                    K.cands += a;
                    float t, u, v;
                    if (rect_hit_uv(r, fo[l], fd[l], bt[l], &t, &u, &v)) bt[l] = t;
                }
                K.plain += any;
                if (twin) { anyA_first = any; anyAB = any || anyB; both = anyBoth; K.pairs++; K.fallbacks += both; }
                else if (second) { K.twins += both ? (anyA_first + any) : anyAB; K.entries += both ? 2 : 1; }
                else { K.twins += any; K.entries++; }
            }
        }
    }
    printf("%d tiles of 8 x 8 pixels, %.0f paths, %.0f segments: %.2f segments per path (depth limit %d)\n", tiles, n_paths, n_segs, n_segs / n_paths, maxdepth);
    const char *name[2] = {"groups of primary rays", "every other group"};
    for (int k = 0; k < 2; ++k) {
        const Count &K = C[k];
        if (K.groups == 0) continue;
        printf("%s: %.0f groups, %.0f rays\n", name[k], K.groups, K.rays);
        printf("  candidate records per ray                          %.2f of %d\n", K.cands / K.rays, N);
        printf("  record bodies per walk of a group, plain walk      %.2f of %d\n", K.plain / K.groups, N);
        printf("  entries visited per walk with twins merged         %.2f (%d with every pair merged)\n", K.entries / K.groups, N - n_pairs);
        printf("  record bodies per walk of a group, twins merged    %.2f\n", K.twins / K.groups);
        printf("  bodies saved per walk                              %.2f\n", (K.plain - K.twins) / K.groups);
        printf("  pairs that fall back (some lane a candidate of both walls)  %.0f of %.0f\n", K.fallbacks, K.pairs);
    }
    const double all = C[0].groups + C[1].groups, saved = (C[0].plain + C[1].plain - C[0].twins - C[1].twins) / all;
    printf("all groups: %.2f bodies per walk plain, %.2f with twins merged, %.2f saved per walk: %s\n", (C[0].plain + C[1].plain) / all,
           (C[0].twins + C[1].twins) / all, saved, saved >= 2. ? "two or more, go on" : "FEWER THAN TWO, STOP");
    return 0;
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


def main():
    src = open(HDR).read()
    types = "".join([_cut(src, r"^struct V3 \{.*?^};\n", "struct V3"),
                     _line(src, "VDEV V3 operator+(V3 a, V3 b)"), _line(src, "VDEV V3 operator-(V3 a, V3 b)"),
                     _line(src, "VDEV V3 operator*(V3 a, float s)"), _line(src, "VDEV float dot(V3 a, V3 b)"),
                     _cut(src, r"^enum \{ kIsectStepsMask.*?\n", "the record's flag bits"),
                     _cut(src, r"^struct IsectRec \{.*?^};\n", "struct IsectRec")])
    body = "".join(_function(src, f) for f in ("isect_rec_build", "rect_twins_mark", "beyond", "rect_frame", "rect_hit_uv", "rects_closest"))
    maxdepth = 5
    try:   # the App.-F depth limit from the library's own parameters where it is built
        sys.path.insert(0, ROOT)
        import __graft_entry__ as g
        maxdepth = int(g.load_package().app_f_params().maxdepth)
    except Exception as e:   # noqa: BLE001
        print("(library not loaded: %s; depth limit %d assumed)" % (e, maxdepth))
    cxx = shutil.which("g++") or shutil.which("c++")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "census.cpp"), "w").write(DRIVER.replace("@TYPES@", types).replace("@FUNCTIONS@", body))
        exe = os.path.join(d, "census")
        subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-o", exe, os.path.join(d, "census.cpp")], check=True)
        print("Closest-hit walks of the fog box: candidate records per ray and record bodies per 64-ray group (scripts/rect_candidate_census.py)")
        sys.stdout.flush()
        subprocess.run([exe, str(maxdepth), "64"], check=True)


if __name__ == "__main__":
    main()
