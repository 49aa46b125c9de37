// bvh_traverse_check.cpp -- the triangle traversal's own text (csrc/vspg_device.h: TriHit ... bvh_any) on the CPU, against a
// brute-force walk over all triangles.
//
// tests/test_bvh_traverse_bits.py cuts that text out of the header as it stands (bvh_traverse_text.inc, with two counters inserted
// by textual replacement), compiles this program with the library's flags plus AddressSanitizer and UndefinedBehaviorSanitizer,
// links it with csrc/vspg_scene_build.hip and csrc/vspg_scene_api.hip (build_triangle_bvh builds every tree) and runs it.  The
// reference answer of a ray is a loop over all accepted triangles with the same tri_intersect against the RAY's tMax, the closest
// hit decided by (t, id); bvh_closest must give the same found / id / bits of t, b0, b1, b2 and bvh_any the same boolean, for every
// ray of every family.  Usage: bvh_traverse_check [substring of the family names to run].
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "vspg_scene_build.h"

using namespace vspg;
using namespace vspg_host;

// what the inserted counters write: the stack's high-water mark, and the nodes and leaves one query has visited (a query that
// visits more than the tree has is stopped and reported: the traversal visits each at most once, so it terminates)
static int g_high_water = 0;
static long g_steps = 0, g_step_cap = 0;
static bool g_runaway = false;

namespace cut {
#undef VDEV
#define VDEV static inline
#include "bvh_traverse_text.inc"
}  // namespace cut

static inline uint32_t f2b(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static inline float b2f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static inline uint32_t rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_state >> 32); }
static inline float unif(float lo, float hi) { return lo + (hi - lo) * (float)((rnd() >> 8) * (1.0 / 16777216.0)); }
static const float kNaN = std::numeric_limits<float>::quiet_NaN();
static const float kZero[2] = {0.f, -0.f};

static int g_failed = 0;
#define CHECK(cond, ...)                                                        \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond);     \
            std::printf(__VA_ARGS__);                                           \
            std::printf("\n");                                                  \
            ++g_failed;                                                         \
        }                                                                       \
    } while (0)

struct P3 { float x, y, z; };
struct Ray { P3 o, d; float tMax; };
static float &at(P3 &v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }
// (u, v) in a plane, c along `axis`: each axis takes the flat role
static P3 in_plane(int axis, float u, float v, float c) { return axis == 2 ? P3{u, v, c} : (axis == 0 ? P3{c, u, v} : P3{v, c, u}); }

// ---- a soup and its tree ------------------------------------------------------------------------------------------------------
struct Soup {
    std::vector<float> p;   // 9 floats per triangle; the position in this array is the triangle's id
    std::vector<DTri> tris;
    std::vector<DBvh4Node> nodes;
    int depth = 0, leaves = 0, largest_leaf = 0;
    DScene S;
    void add(P3 a, P3 b, P3 c) { const float v[9] = {a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z}; p.insert(p.end(), v, v + 9); }
    int count() const { return (int)(p.size() / 9); }
};
static int tree_depth(const Soup &s, int node, int *leaves, int *largest_leaf) {
    int depth = 0;
    for (int k = 0; k < 4; ++k) {
        const int32_t c = s.nodes[node].child[k];
        if (c == kBvhAbsent) continue;
        if (c >= 0) { const int d = tree_depth(s, c, leaves, largest_leaf); depth = d > depth ? d : depth; }
        else { ++*leaves; const int n = (-c - 1) & 7; *largest_leaf = n > *largest_leaf ? n : *largest_leaf; }
    }
    return depth + 1;
}
static void finish(Soup &s) {
    static VspgScene sc;
    std::memset(&sc, 0, sizeof sc);
    sc.n_triangles = s.count();
    sc.tri_p = s.p.data();
    CHECK(build_triangle_bvh(sc, &s.tris, &s.nodes) == 0, "%s", vspg_last_error());
    std::memset(&s.S, 0, sizeof s.S);
    s.S.n_tris = (int32_t)s.tris.size();
    s.S.n_bvh_nodes = (int32_t)s.nodes.size();
    s.S.tris = s.tris.data();
    s.S.bvh = s.nodes.data();
    s.leaves = s.largest_leaf = 0;
    s.depth = s.nodes.empty() ? 0 : tree_depth(s, 0, &s.leaves, &s.largest_leaf);
}

// ---- one family: every ray through both, the tallies printed in one line ---------------------------------------------------------
struct Tally { long rays = 0, hits = 0, closest_bad = 0, hit_miss_bad = 0, any_bad = 0; int high_water = 0; };
static long g_total_bad = 0, g_total_rays = 0;
static int g_max_high_water = 0;
static const char *g_filter = "";

static bool brute(const Soup &s, const Ray &r, int *id, cut::TriHit *best) {
    const cut::V3 o{r.o.x, r.o.y, r.o.z};
    const cut::TriRay R = cut::tri_ray(cut::V3{r.d.x, r.d.y, r.d.z});
    bool found = false;
    for (const DTri &T : s.tris) {
        cut::TriHit h;
        if (cut::tri_intersect(o, R, r.tMax, cut::ld3(T.p0), cut::ld3(T.p1), cut::ld3(T.p2), &h) && h.t < r.tMax)
            if (!found || h.t < best->t || (h.t == best->t && T.id < *id)) { found = true; *best = h; *id = T.id; }
    }
    return found;
}
static void check(const Soup &s, const Ray &r, Tally *T, const char *name) {
    int ref_id = -1, tp = -1;
    cut::TriHit ref{0, 0, 0, 0}, got{0, 0, 0, 0};
    const bool ref_found = brute(s, r, &ref_id, &ref);
    const cut::V3 o{r.o.x, r.o.y, r.o.z}, d{r.d.x, r.d.y, r.d.z};
    g_high_water = 0;
    g_steps = 0;
    const bool found = s.tris.empty() ? false : cut::bvh_closest(s.S, o, d, r.tMax, &tp, &got);
    g_steps = 0;
    const bool any = s.tris.empty() ? false : cut::bvh_any(s.S, o, d, r.tMax);
    T->rays++;
    T->hits += ref_found;
    T->high_water = g_high_water > T->high_water ? g_high_water : T->high_water;
    bool bad = found != ref_found;
    if (bad) T->hit_miss_bad++;
    if (!bad && found) {
        CHECK(tp >= 0 && tp < (int)s.tris.size(), "%s: triangle position %d of %zu", name, tp, s.tris.size());
        bad = tp < 0 || tp >= (int)s.tris.size() || s.tris[tp].id != ref_id || f2b(got.t) != f2b(ref.t) || f2b(got.b0) != f2b(ref.b0) ||
              f2b(got.b1) != f2b(ref.b1) || f2b(got.b2) != f2b(ref.b2);
    }
    if (bad) T->closest_bad++;
    if (any != ref_found) T->any_bad++;
    if ((bad || any != ref_found) && T->closest_bad + T->any_bad <= 4)
        std::printf("  %s: o %08x %08x %08x d %08x %08x %08x tMax %08x: brute force %d id %d t %08x, traversal %d id %d t %08x, any %d\n", name,
                    f2b(r.o.x), f2b(r.o.y), f2b(r.o.z), f2b(r.d.x), f2b(r.d.y), f2b(r.d.z), f2b(r.tMax), ref_found, ref_id, f2b(ref.t), found,
                    (found && tp >= 0 && tp < (int)s.tris.size()) ? s.tris[tp].id : -1, f2b(got.t), any);
}
static bool wanted(const char *name) { return std::strstr(name, g_filter) != nullptr; }
static Tally run(const char *name, Soup &s, const std::vector<Ray> &rays) {
    Tally T;
    g_step_cap = (long)s.nodes.size() + s.leaves;
    for (const Ray &r : rays) check(s, r, &T, name);
    std::printf("family %s: triangles %zu nodes %zu depth %d rays %ld hits %ld high-water %d closest-mismatches %ld hit-miss-mismatches %ld any-mismatches %ld\n",
                name, s.tris.size(), s.nodes.size(), s.depth, T.rays, T.hits, T.high_water, T.closest_bad, T.hit_miss_bad, T.any_bad);
    CHECK(T.high_water <= 3 * s.depth && T.high_water <= kBvhStack, "%s: %d stack entries at depth %d (the stack has %d)", name, T.high_water, s.depth, kBvhStack);
    g_total_bad += T.closest_bad + T.any_bad;
    g_total_rays += T.rays;
    g_max_high_water = T.high_water > g_max_high_water ? T.high_water : g_max_high_water;
    return T;
}

// ---- soups ---------------------------------------------------------------------------------------------------------------------
// n x n cells over [0, 1]^2 of the plane `axis` = c, vertices at multiples of 1 / n, two triangles per cell; `other` takes the
// other diagonal; height(i, j) is added to c at vertex (i, j)
static void add_grid(Soup &s, int axis, int n, float c, bool other = false, float (*height)(int, int) = nullptr) {
    auto vtx = [&](int i, int j) { return in_plane(axis, (float)i / n, (float)j / n, c + (height ? height(i, j) : 0.f)); };
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) {
            if (!other) { s.add(vtx(i, j), vtx(i + 1, j), vtx(i + 1, j + 1)); s.add(vtx(i, j), vtx(i + 1, j + 1), vtx(i, j + 1)); }
            else { s.add(vtx(i, j), vtx(i + 1, j), vtx(i, j + 1)); s.add(vtx(i + 1, j), vtx(i + 1, j + 1), vtx(i, j + 1)); }
        }
}
static float steps_of_eighths(int i, int j) { return (float)((3 * i + 5 * j) % 4) / 8.f; }

// rays along `axis` through the (2n + 1)^2 vertices, edge midpoints and cell centres of an n x n grid over [0, 1]^2, from c + dist
// downwards and from c - dist upwards; the two zero components of d take the signs of `signs` (bit 0, bit 1: negative)
static void perpendicular(std::vector<Ray> &rays, int axis, int n, float c, float dist, unsigned sign_mask, float tMax) {
    for (unsigned signs = 0; signs < 4; ++signs) {
        if (!((sign_mask >> signs) & 1u)) continue;
        for (int side = 0; side < 2; ++side)
            for (int j = 0; j <= 2 * n; ++j)
                for (int i = 0; i <= 2 * n; ++i) {
                    Ray r;
                    r.o = in_plane(axis, (float)i / (2 * n), (float)j / (2 * n), side ? c - dist : c + dist);
                    r.d = in_plane(axis, kZero[signs & 1], kZero[signs >> 1], side ? 1.f : -1.f);
                    r.tMax = tMax;
                    rays.push_back(r);
                }
    }
}
// the same rays with tMax exactly the hit distance (a miss: h.t < tMax is strict) and with the next float above it
static std::vector<Ray> at_the_hit_distance(const Soup &s, const std::vector<Ray> &rays) {
    std::vector<Ray> out;
    for (Ray r : rays) {
        int id;
        cut::TriHit h;
        r.tMax = kInf;
        if (!brute(s, r, &id, &h)) continue;
        r.tMax = h.t; out.push_back(r);
        r.tMax = std::nextafterf(h.t, kInf); out.push_back(r);
    }
    return out;
}
static Ray random_ray(float extent, int i) {
    Ray r;
    r.o = P3{unif(-extent, extent), unif(-extent, extent), unif(-extent, extent)};
    r.d = P3{unif(-1, 1), unif(-1, 1), unif(-1, 1)};
    r.tMax = (i % 4 == 0) ? unif(0.f, 2 * extent) : ((i % 4 == 1) ? unif(0.f, 1e-3f * extent) : kInf);
    return r;
}
// a ray from a random origin towards a random point of a random triangle
static Ray aimed_ray(const Soup &s, float extent) {
    const float *p = &s.p[9 * (rnd() % (unsigned)s.count())];
    float b0 = unif(0, 1), b1 = unif(0, 1);
    if (b0 + b1 > 1) { b0 = 1 - b0; b1 = 1 - b1; }
    const float b2 = 1 - b0 - b1;
    Ray r;
    r.o = P3{unif(-extent, extent), unif(-extent, extent), unif(-extent, extent)};
    r.d = P3{b0 * p[0] + b1 * p[3] + b2 * p[6] - r.o.x, b0 * p[1] + b1 * p[4] + b2 * p[7] - r.o.y, b0 * p[2] + b1 * p[5] + b2 * p[8] - r.o.z};
    r.tMax = kInf;
    return r;
}

// ---- the families -----------------------------------------------------------------------------------------------------------------
static const float kPlaneOf[3] = {0.5f, -0.25f, 0.f};   // the flat grids: x = 0.5, y = -0.25, z = 0
static void flat_grids() {
    for (int axis = 2; axis >= 0; --axis) {
        const char ax = "xyz"[axis];
        char name[96];
        Soup s;
        add_grid(s, axis, 8, kPlaneOf[axis]);
        finish(s);
        std::vector<Ray> rays, all;
        // both zeros of one sign: the 1156 rays of the first report (brute force hits on every one)
        std::snprintf(name, sizeof name, "flat grid %c, perpendicular, zeros of one sign", ax);
        if (wanted(name)) {
            perpendicular(rays, axis, 8, kPlaneOf[axis], 1.f, 0x9u, kInf);
            const Tally T = run(name, s, rays);
            CHECK(T.rays == 1156 && T.hits == T.rays, "%s: %ld of %ld rays hit", name, T.hits, T.rays);
        }
        std::snprintf(name, sizeof name, "flat grid %c, perpendicular, zeros of two signs", ax);
        if (wanted(name)) {
            rays.clear();
            perpendicular(rays, axis, 8, kPlaneOf[axis], 1.f, 0x6u, kInf);
            perpendicular(rays, axis, 8, kPlaneOf[axis], 0.7f, 0xFu, kInf);
            const Tally T = run(name, s, rays);
            CHECK(T.hits == T.rays, "%s: %ld of %ld rays hit", name, T.hits, T.rays);
        }
        std::snprintf(name, sizeof name, "flat grid %c, tMax at the hit distance", ax);
        if (wanted(name)) {
            perpendicular(all, axis, 8, kPlaneOf[axis], 1.f, 0xFu, kInf);
            perpendicular(all, axis, 8, kPlaneOf[axis], 0.7f, 0xFu, kInf);
            const Tally T = run(name, s, at_the_hit_distance(s, all));
            CHECK(T.rays == 2 * (long)all.size() && 2 * T.hits == T.rays, "%s: %ld of %ld rays hit", name, T.hits, T.rays);
        }
        std::snprintf(name, sizeof name, "flat grid %c, rays in its plane", ax);
        if (wanted(name)) {
            rays.clear();
            const float dirs[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {-1, 1}, {0.25f, -1}, {-1, -0.375f}};
            for (int k = 0; k < 8; ++k)
                for (int z = 0; z < 2; ++z)
                    for (int j = -1; j <= 17; j += 1)
                        for (int i = -1; i <= 17; i += 3) {   // origins on vertices, edges and outside the grid
                            Ray r;
                            r.o = in_plane(axis, (float)i / 16, (float)j / 16, kPlaneOf[axis]);
                            r.d = in_plane(axis, dirs[k][0], dirs[k][1], kZero[z]);
                            r.tMax = kInf;
                            rays.push_back(r);
                        }
            const Tally T = run(name, s, rays);
            CHECK(T.hits == 0, "%s: %ld rays hit", name, T.hits);
        }
    }
}
static void tilted_triangles() {
    const char *name = "tilted triangles, axis-parallel rays";
    if (!wanted(name)) return;
    Soup s;
    add_grid(s, 2, 8, 0.f, false, steps_of_eighths);   // a heightfield with steps of 1/8: a box face holds a vertex or an edge only
    finish(s);
    std::vector<Ray> rays;
    perpendicular(rays, 2, 8, 0.f, 1.f, 0xFu, kInf);
    // along x and along y through the lattice of sixteenths (heights included): such rays run along the faces of the boxes
    for (int axis = 0; axis < 2; ++axis)
        for (unsigned signs = 0; signs < 4; ++signs)
            for (int side = 0; side < 2; ++side)
                for (int k = -1; k <= 8; ++k)
                    for (int j = 0; j <= 16; ++j) {
                        Ray r;
                        const float u = (float)j / 16, h = (float)k / 16;
                        r.o = axis == 0 ? P3{side ? -1.f : 2.f, u, h} : P3{u, side ? -1.f : 2.f, h};
                        r.d = axis == 0 ? P3{side ? 1.f : -1.f, kZero[signs & 1], kZero[signs >> 1]} : P3{kZero[signs & 1], side ? 1.f : -1.f, kZero[signs >> 1]};
                        r.tMax = kInf;
                        rays.push_back(r);
                    }
    const Tally T = run(name, s, rays);
    CHECK(T.hits > T.rays / 2, "%s: %ld of %ld rays hit", name, T.hits, T.rays);
    std::vector<Ray> exact = at_the_hit_distance(s, rays);
    run("tilted triangles, tMax at the hit distance", s, exact);
}
static void two_layers() {
    const char *name = "two layers";
    if (!wanted(name)) return;
    Soup s;
    add_grid(s, 2, 8, 0.f);
    add_grid(s, 2, 8, -0.5f);
    finish(s);
    std::vector<Ray> rays;
    perpendicular(rays, 2, 8, 0.f, 1.f, 0xFu, kInf);     // from above: layer 0 first; from below (c - 1 = -1): layer 1 first
    perpendicular(rays, 2, 8, -0.25f, 0.125f, 0x9u, kInf);   // from between the layers
    perpendicular(rays, 2, 8, 0.f, 1.f, 0x9u, 1.25f);    // tMax between the layers' distances
    for (int i = 0; i < 4000; ++i) {   // oblique rays through both layers
        Ray r;
        r.o = P3{unif(-0.5f, 1.5f), unif(-0.5f, 1.5f), (i & 1) ? 1.f : -1.5f};
        r.d = P3{unif(0, 1) - r.o.x, unif(0, 1) - r.o.y, -0.25f - r.o.z};
        r.tMax = kInf;
        rays.push_back(r);
    }
    const Tally T = run(name, s, rays);
    CHECK(T.hits > T.rays * 3 / 4, "%s: %ld of %ld rays hit", name, T.hits, T.rays);
    run("two layers, tMax at the hit distance", s, at_the_hit_distance(s, rays));
}
// `copies` coincident copies of each triangle of a 2 x 2 grid, the ids shuffled: equal t goes to the smallest id.  The copies share
// a centroid, so no plane separates them: nine are split at the median into leaves of 4 and 5, fourteen into two full leaves of 7
static void coincident_copies(int copies, int leaf) {
    char name[64];
    std::snprintf(name, sizeof name, "ties, %d coincident copies", copies);
    if (!wanted(name)) return;
    Soup g, s;
    add_grid(g, 2, 2, 0.f);
    const int n = 8 * copies;
    std::vector<int> slot(n);
    for (int i = 0; i < n; ++i) slot[i] = i % 8;   // which of the 8 triangles the soup's triangle i is a copy of
    for (int i = n - 1; i > 0; --i) { const int j = (int)(rnd() % (unsigned)(i + 1)), t = slot[i]; slot[i] = slot[j]; slot[j] = t; }
    int smallest[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
    for (int i = 0; i < n; ++i) {
        s.p.insert(s.p.end(), &g.p[9 * slot[i]], &g.p[9 * slot[i]] + 9);
        if (smallest[slot[i]] < 0) smallest[slot[i]] = i;
    }
    finish(s);
    CHECK(s.largest_leaf == leaf, "%s: the largest leaf holds %d triangles, not %d", name, s.largest_leaf, leaf);
    std::vector<Ray> rays;
    perpendicular(rays, 2, 2, 0.f, 1.f, 0xFu, kInf);
    perpendicular(rays, 2, 4, 0.f, 0.7f, 0x9u, kInf);
    for (int i = 0; i < 4000; ++i) rays.push_back(aimed_ray(s, 2.f));
    const Tally T = run(name, s, rays);
    CHECK(T.hits > T.rays * 3 / 4, "%s: %ld of %ld rays hit", name, T.hits, T.rays);
    long not_smallest = 0;   // independently of the brute-force loop: the winner is the smallest id of its copies
    for (const Ray &r : rays) {
        int tp = -1;
        cut::TriHit h;
        g_steps = 0;
        if (cut::bvh_closest(s.S, cut::V3{r.o.x, r.o.y, r.o.z}, cut::V3{r.d.x, r.d.y, r.d.z}, r.tMax, &tp, &h) && tp >= 0 && tp < n)
            not_smallest += s.tris[tp].id != smallest[slot[s.tris[tp].id]];
    }
    std::printf("  %s: %ld winners are not the smallest id of their copies\n", name, not_smallest);
    g_total_bad += not_smallest;
}
static void ties() {
    coincident_copies(9, 5);
    coincident_copies(14, 7);
    const char *name = "ties, two triangulations of one plane";
    if (wanted(name)) {
        Soup s;
        add_grid(s, 2, 8, 0.f);
        add_grid(s, 2, 8, 0.f, true);
        add_grid(s, 2, 5, 0.f);
        finish(s);
        std::vector<Ray> rays;
        perpendicular(rays, 2, 8, 0.f, 1.f, 0xFu, kInf);
        perpendicular(rays, 2, 5, 0.f, 0.7f, 0x9u, kInf);
        for (int i = 0; i < 4000; ++i) rays.push_back(aimed_ray(s, 2.f));
        const Tally T = run(name, s, rays);
        CHECK(T.hits > T.rays * 3 / 4, "%s: %ld of %ld rays hit", name, T.hits, T.rays);
    }
}
static void random_triangles(Soup &s, int n, float extent, float size) {
    for (int t = 0; t < n; ++t) {
        const P3 c{unif(-extent, extent), unif(-extent, extent), unif(-extent, extent)};
        P3 v[3];
        for (int k = 0; k < 3; ++k) v[k] = P3{c.x + unif(-size, size), c.y + unif(-size, size), c.z + unif(-size, size)};
        s.add(v[0], v[1], v[2]);
    }
}
static void tree_shapes() {
    const int small[6] = {1, 2, 3, 7, 8, 9};
    for (int k = 0; k < 6; ++k) {
        char name[64];
        std::snprintf(name, sizeof name, "tree shapes, soup of %d", small[k]);
        if (!wanted(name)) continue;
        Soup s;
        random_triangles(s, small[k], 0.5f, 0.5f);
        finish(s);
        std::vector<Ray> rays;
        for (int i = 0; i < 6000; ++i) rays.push_back((i & 1) ? aimed_ray(s, 2.f) : random_ray(1.5f, i >> 1));
        const Tally T = run(name, s, rays);
        CHECK(T.hits > T.rays / 4 && T.hits < T.rays, "%s: %ld of %ld rays hit", name, T.hits, T.rays);
    }
    const char *name = "tree shapes, 1000 triangles in one box";
    if (wanted(name)) {
        Soup s;
        for (int t = 0; t < 1000; ++t) {   // per coordinate one vertex at 0, one at 1 and one between: every triangle's box is [0, 1]^3
            float v[3][3];
            for (int c = 0; c < 3; ++c) {
                const int lo = (int)(rnd() % 3u), hi = (lo + 1 + (int)(rnd() % 2u)) % 3;
                for (int k = 0; k < 3; ++k) v[k][c] = k == lo ? 0.f : (k == hi ? 1.f : unif(0, 1));
            }
            s.add(P3{v[0][0], v[0][1], v[0][2]}, P3{v[1][0], v[1][1], v[1][2]}, P3{v[2][0], v[2][1], v[2][2]});
        }
        finish(s);
        std::vector<Ray> rays;
        for (int i = 0; i < 6000; ++i) rays.push_back((i & 1) ? aimed_ray(s, 2.f) : random_ray(1.5f, i >> 1));
        for (int i = 0; i < 600; ++i) {   // along the box's faces and through its corners, with zeros of both signs
            Ray r;
            const int a = i % 3;
            r.o = P3{(float)(rnd() % 3u) * 0.5f, (float)(rnd() % 3u) * 0.5f, (float)(rnd() % 3u) * 0.5f};
            r.d = P3{kZero[rnd() & 1], kZero[rnd() & 1], kZero[rnd() & 1]};
            at(r.o, a) = (i & 1) ? 2.f : -1.f;
            at(r.d, a) = (i & 1) ? -1.f : 1.f;
            r.tMax = kInf;
            rays.push_back(r);
        }
        const Tally T = run(name, s, rays);
        CHECK(T.hits > T.rays / 4, "%s: %ld of %ld rays hit", name, T.hits, T.rays);
    }
    const int sheets[4] = {7, 8, 60, 2000};
    for (int k = 0; k < 4; ++k) {
        char nm[64];
        std::snprintf(nm, sizeof nm, "tree shapes, %d stacked sheets", sheets[k]);
        if (!wanted(nm)) continue;
        Soup s;
        for (int t = 0; t < sheets[k]; ++t) {
            const float z = (float)t / 64;
            s.add(P3{0, 0, z}, P3{1, 0, z}, P3{0, 1, z});
        }
        finish(s);
        std::vector<Ray> rays;
        perpendicular(rays, 2, 2, 0.f, 40.f, 0xFu, kInf);
        for (int i = 0; i < 2000; ++i) {
            Ray r = aimed_ray(s, 1.5f);
            if (i & 1) r.o.z = unif(0.f, (float)sheets[k] / 64);   // from between the sheets
            if (i % 8 == 0) r.tMax = unif(0.f, 2.f);
            rays.push_back(r);
        }
        const Tally T = run(nm, s, rays);
        CHECK(T.hits > T.rays / 4, "%s: %ld of %ld rays hit", nm, T.hits, T.rays);
    }
    const int cascade[2] = {48, 126};
    for (int k = 0; k < 2; ++k) {
        char nm[64];
        std::snprintf(nm, sizeof nm, "tree shapes, cascade of %d", cascade[k]);
        if (!wanted(nm)) continue;
        Soup s;
        for (int t = 1; t <= cascade[k]; ++t) {   // the unit triangle in the plane z = 0 with its corner at x = 2^-t
            const float x = std::ldexp(1.f, -t);
            s.add(P3{x, 0, 0}, P3{x + 1, 0, 0}, P3{x, 1, 0});
        }
        finish(s);
        std::vector<Ray> rays;
        for (int t = 0; t <= cascade[k] + 1; ++t)
            for (int j = 0; j < 5; ++j)
                for (unsigned signs = 0; signs < 4; ++signs)
                    for (int side = 0; side < 2; ++side) {
                        Ray r;
                        r.o = P3{t == 0 ? 0.f : std::ldexp(1.f, -t), (float)j / 4, side ? -1.f : 1.f};
                        r.d = P3{kZero[signs & 1], kZero[signs >> 1], side ? 1.f : -1.f};
                        r.tMax = kInf;
                        rays.push_back(r);
                    }
        for (int i = 0; i < 4000; ++i) rays.push_back(aimed_ray(s, 2.f));
        const Tally T = run(nm, s, rays);
        CHECK(T.hits > T.rays / 4, "%s: %ld of %ld rays hit", nm, T.hits, T.rays);
    }
}
static const float kOdd[] = {0.f, -0.f, b2f(1), b2f(0x80000001u), b2f(0x00400000u), b2f(0x807fffffu)};   // zeros and denormals
static const float kNonFinite[] = {kInf, -kInf, kNaN, -kNaN};
static void random_soup() {
    Soup s;
    g_state = 0x2545F4914F6CDD1Dull;
    random_triangles(s, 2000, 1.f, 0.08f);
    finish(s);
    const char *name = "random soup, random rays";
    if (wanted(name)) {
        std::vector<Ray> rays;
        for (int i = 0; i < 12000; ++i) rays.push_back((i % 3 == 0) ? aimed_ray(s, 2.f) : random_ray(1.5f, i));
        for (int i = 0; i < 4000; ++i) {   // origins inside boxes: on a triangle's vertex, or just off a point of a triangle
            Ray r = random_ray(1.f, i);
            const float *p = &s.p[9 * (rnd() % 2000u)];
            r.o = P3{p[0], p[1], p[2]};
            if (i & 1) r.o = P3{(p[0] + p[3] + p[6]) / 3 - 1e-3f * r.d.x, (p[1] + p[4] + p[7]) / 3 - 1e-3f * r.d.y, (p[2] + p[5] + p[8]) / 3 - 1e-3f * r.d.z};
            rays.push_back(r);
        }
        const Tally T = run(name, s, rays);
        CHECK(T.hits > T.rays / 8 && T.hits < T.rays, "%s: %ld of %ld rays hit", name, T.hits, T.rays);
    }
    name = "random soup, zeros and denormals in d";
    if (wanted(name)) {
        std::vector<Ray> rays;
        for (int i = 0; i < 12000; ++i) {
            Ray r = (i & 1) ? aimed_ray(s, 2.f) : random_ray(1.2f, i);
            const int n = 1 + (int)(rnd() % 2u), first = (int)(rnd() % 3u);
            for (int k = 0; k < n; ++k) at(r.d, (first + k) % 3) = kOdd[rnd() % 6u];
            if (i % 4 == 0) {   // the origin on a triangle's box face: a vertex's coordinate
                const float *p = &s.p[9 * (rnd() % 2000u)];
                at(r.o, first) = p[first];
            }
            rays.push_back(r);
        }
        const Tally T = run(name, s, rays);
        CHECK(T.hits > T.rays / 16, "%s: %ld of %ld rays hit", name, T.hits, T.rays);
    }
    name = "random soup, infinities and NaNs";
    if (wanted(name)) {
        std::vector<Ray> rays;
        for (int i = 0; i < 8000; ++i) {
            Ray r = (i & 1) ? aimed_ray(s, 2.f) : random_ray(1.2f, i);
            const int n = 1 + (int)(rnd() % 3u);
            for (int k = 0; k < n; ++k) {
                const unsigned w = rnd() % 7u;
                const float v = kNonFinite[rnd() % 4u];
                if (w < 3) at(r.o, (int)w) = v; else if (w < 6) at(r.d, (int)w - 3) = v; else r.tMax = v;
            }
            rays.push_back(r);
        }
        run(name, s, rays);
    }
}
static void slivers_and_wide_range() {
    const char *name = "slivers at grazing angles";
    if (wanted(name)) {
        Soup s;
        g_state = 0xD1B54A32D192ED03ull;
        for (int t = 0; t < 500; ++t) {   // long thin triangles close to the plane z = 0
            const P3 a{unif(-1, 1), unif(-1, 1), unif(-0.01f, 0.01f)};
            const float ang = unif(0.f, 6.2831853f), l = unif(0.5f, 2.f), w = unif(1e-5f, 1e-3f);
            const P3 b{a.x + l * std::cos(ang), a.y + l * std::sin(ang), a.z + unif(-0.01f, 0.01f)};
            const P3 c{a.x - w * std::sin(ang), a.y + w * std::cos(ang), a.z + unif(-1e-4f, 1e-4f)};
            s.add(a, b, c);
        }
        finish(s);
        std::vector<Ray> rays;
        for (int i = 0; i < 40000; ++i) {
            Ray r = aimed_ray(s, 3.f);
            const float z = unif(-0.05f, 0.05f);   // grazing: the origin close to the plane, the target as aimed
            r.d.z = r.d.z + r.o.z - z;
            r.o.z = z;
            rays.push_back(r);
        }
        const Tally T = run(name, s, rays);
        CHECK(T.hits > T.rays / 8, "%s: %ld of %ld rays hit", name, T.hits, T.rays);
    }
    name = "wide-range soup, aimed rays";
    if (wanted(name)) {
        Soup s;
        g_state = 0x94D049BB133111EBull;
        auto wide = [] { const float m = std::pow(10.f, unif(-4.f, 4.f)); return (rnd() & 1) ? m : -m; };
        for (int t = 0; t < 1000; ++t) s.add(P3{wide(), wide(), wide()}, P3{wide(), wide(), wide()}, P3{wide(), wide(), wide()});
        finish(s);
        std::vector<Ray> rays;
        for (int i = 0; i < 20000; ++i) {
            Ray r = aimed_ray(s, 1.f);
            const float m = std::pow(10.f, unif(-4.f, 4.f));
            const P3 o{r.o.x * m, r.o.y * m, r.o.z * m};
            r.d = P3{r.d.x + r.o.x - o.x, r.d.y + r.o.y - o.y, r.d.z + r.o.z - o.z};
            r.o = o;
            rays.push_back(r);
        }
        const Tally T = run(name, s, rays);
        CHECK(T.hits > T.rays / 2, "%s: %ld of %ld rays hit", name, T.hits, T.rays);
    }
}

int main(int argc, char **argv) {
    if (argc > 1) g_filter = argv[1];
    flat_grids();
    tilted_triangles();
    two_layers();
    ties();
    tree_shapes();
    random_soup();
    slivers_and_wide_range();
    CHECK(!g_runaway, "a query visited more nodes and leaves than its tree has");
    std::printf("rays %ld mismatches %ld highest stack occupancy %d of %d\n", g_total_rays, g_total_bad, g_max_high_water, kBvhStack);
    if (!*g_filter) CHECK(g_max_high_water >= 16, "no family fills the stack beyond %d entries", g_max_high_water);
    if (g_failed) std::printf("%d checks failed\n", g_failed);
    std::printf("result %s\n", (g_total_bad || g_failed) ? "MISMATCH" : "identical");
    return (g_total_bad || g_failed) ? 1 : 0;
}
