// scene_build_check.cpp -- the host-side scene preprocessing (csrc/vspg_scene_build.hip, csrc/vspg_scene_api.hip) run on the CPU.
//
// tests/test_scene_build.py compiles those two units and this program with the library's flags plus AddressSanitizer and
// UndefinedBehaviorSanitizer, links them WITHOUT the HIP runtime and runs the result: exit status 0 and no sanitizer report.
// Every check below is a structural fact of any correct result (sums, ranges, containment, reachability), none is a recorded output.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "vspg_scene_build.h"

using namespace vspg;
using namespace vspg_host;

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

// the fixed-seed generator of every case: a 64-bit LCG (Knuth's MMIX constants), the top 24 bits as a float in [0, 1)
struct Lcg {
    uint64_t s;
    explicit Lcg(uint64_t seed) : s(seed) {}
    float next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (float)(s >> 40) * 0x1p-24f;
    }
};

static VspgRenderConfig config(int xres, int yres) {
    VspgRenderConfig cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.xres = xres; cfg.yres = yres; cfg.spp = 1; cfg.shard_count = 1;
    return cfg;
}
static void emissive_quad(VspgQuad *q, const float p[3], const float e1[3], const float e2[3], float le, int two_sided) {
    std::memset(q, 0, sizeof *q);
    for (int k = 0; k < 3; ++k) { q->p00[k] = p[k]; q->e1[k] = e1[k]; q->e2[k] = e2[k]; q->Le[k] = le * (float)(k + 1); }
    q->two_sided = two_sided;
}

// ---- 1. fog box ----------------------------------------------------------------------------------------------------------------
static void check_light_of_quad(const DScene &D) {
    for (int i = 0; i < D.n_lights; ++i) {
        const int q = D.light_quads[i];
        CHECK(q >= 0 && q < D.n_quads, "light %d names rectangle %d", i, q);
        if (q >= 0 && q < D.n_quads) CHECK(D.lsamp.light_of_quad[q] == i, "light_of_quad[%d] = %d, light %d", q, D.lsamp.light_of_quad[q], i);
    }
    int lights = 0;
    for (int q = 0; q < VSPG_MAX_QUADS; ++q) {
        const int l = D.lsamp.light_of_quad[q];
        if (l < 0) { CHECK(l == -1, "light_of_quad[%d] = %d", q, l); continue; }
        ++lights;
        CHECK(l < D.n_lights && D.light_quads[l] == q, "light_of_quad[%d] = %d does not map back", q, l);
    }
    CHECK(lights == D.n_lights, "%d rectangles are lights, n_lights %d", lights, D.n_lights);
}
static void test_fog_box() {
    static VspgScene sc;
    static DScene D;
    VspgIntegratorParams prm;
    vspg_integrator_params_default(&prm);
    const VspgRenderConfig cfg = config(16, 16);
    CHECK(vspg_scene_fog_box(&sc, 16, 16) == 0, "%s", vspg_last_error());
    CHECK(validate(&sc, &prm, &cfg) == 0, "%s", vspg_last_error());
    build_dscene(sc, prm, cfg, &D);
    CHECK(D.n_lights == 1, "n_lights %d", D.n_lights);
    CHECK(D.lsamp.mode == VSPG_LIGHTSAMPLER_UNIFORM, "mode %d", D.lsamp.mode);
    check_light_of_quad(D);
    // RectPlanes (vspg_device.h): "the fog box has 2, 3 and 2"; plane k of axis a has position kPlaneChunk * a + k + 1
    const int want[3] = {2, 3, 2};
    for (int a = 0; a < 3; ++a) {
        int n = 0;
        for (int k = 0; k < kPlaneChunk; ++k) n += (D.planes.listed >> (kPlaneChunk * a + k + 1)) & 1u;
        CHECK(n == want[a], "axis %d lists %d planes", a, n);
    }
    CHECK(D.planes.always == 0u, "always %08x: every rectangle of the fog box is axis aligned", D.planes.always);
}

// ---- 2. many lights --------------------------------------------------------------------------------------------------------------
static void test_many_lights(int lightsampler) {
    static VspgScene sc;
    static DScene D;
    VspgIntegratorParams prm;
    vspg_integrator_params_default(&prm);
    prm.lightsampler = lightsampler;
    const VspgRenderConfig cfg = config(16, 16);
    CHECK(vspg_scene_fog_box(&sc, 16, 16) == 0, "%s", vspg_last_error());
    {
        const float p0[3] = {-0.9f, -0.2f, 0.3f}, a0[3] = {0.f, 0.3f, 0.f}, b0[3] = {0.f, 0.f, 0.2f};        // on the left wall's side, faces +x
        const float p1[3] = {0.2f, -0.9f, -0.4f}, a1[3] = {0.25f, 0.1f, 0.f}, b1[3] = {0.f, 0.1f, 0.35f};    // tilted, near the floor
        const float p2[3] = {0.5f, 0.1f, 0.6f}, a2[3] = {0.f, 0.2f, 0.f}, b2[3] = {0.2f, 0.f, 0.f};          // two-sided, in mid air
        emissive_quad(&sc.quads[sc.n_quads++], p0, a0, b0, 3.f, 0);
        emissive_quad(&sc.quads[sc.n_quads++], p1, a1, b1, 0.5f, 0);
        emissive_quad(&sc.quads[sc.n_quads++], p2, a2, b2, 8.f, 1);
    }
    sc.n_infinite_lights = 2;
    sc.infinite_lights[0].type = VSPG_LIGHT_UNIFORM_INFINITE;
    sc.infinite_lights[1].type = VSPG_LIGHT_IMAGE_INFINITE;
    for (int k = 0; k < 3; ++k) { sc.infinite_lights[0].L[k] = 0.1f * (float)(k + 1); sc.infinite_lights[1].L[k] = 0.4f; }
    sc.n_point_lights = 2;
    {
        const float from0[3] = {0.3f, 0.5f, -0.2f}, from1[3] = {-0.6f, 0.7f, 0.4f}, to1[3] = {0.1f, -1.f, 0.f};
        VspgPointLight &P = sc.point_lights[0], &S = sc.point_lights[1];
        std::memset(&P, 0, sizeof P);
        std::memset(&S, 0, sizeof S);
        P.type = VSPG_LIGHT_POINT;
        S.type = VSPG_LIGHT_SPOT;
        for (int k = 0; k < 3; ++k) { P.I[k] = 2.f; S.I[k] = 5.f + (float)k; }
        S.cone_angle_deg = 30.f;
        S.cone_delta_deg = 5.f;
        CHECK(vspg_point_light_at(&P, from0, nullptr) == 0, "%s", vspg_last_error());
        CHECK(vspg_spot_light_look_at(&S, from1, to1, nullptr) == 0, "%s", vspg_last_error());
    }
    CHECK(validate(&sc, &prm, &cfg) == 0, "%s", vspg_last_error());
    build_dscene(sc, prm, cfg, &D);
    const DLightSampler &ls = D.lsamp;
    const int n_all = D.n_lights + D.n_inf + D.n_point, first_point = D.n_lights + D.n_inf;
    CHECK(D.n_lights == 4 && D.n_inf == 2 && D.n_point == 2, "%d rectangle, %d infinite, %d point lights", D.n_lights, D.n_inf, D.n_point);
    CHECK(ls.mode == lightsampler, "mode %d, asked for %d", ls.mode, lightsampler);
    check_light_of_quad(D);
    // the power sampler's alias table
    CHECK(ls.n_alias == n_all, "n_alias %d, %d lights", ls.n_alias, n_all);
    double sum = 0;
    for (int i = 0; i < ls.n_alias; ++i) {
        sum += (double)ls.alias_p[i];
        CHECK(ls.alias_q[i] >= 0.f && ls.alias_q[i] <= 1.f, "alias_q[%d] = %g", i, ls.alias_q[i]);
        CHECK(ls.alias_i[i] == -1 || (ls.alias_i[i] >= 0 && ls.alias_i[i] < ls.n_alias), "alias_i[%d] = %d", i, ls.alias_i[i]);
    }
    CHECK(std::fabs(sum - 1.) <= ls.n_alias * 0x1p-23, "alias_p sums to 1 %+g", sum - 1.);
    // the BVH sampler's tree: bit d of a light's trail says which child to take at depth d (0: node + 1, 1: child_or_light)
    CHECK(ls.n_inf == D.n_inf, "n_inf %d", ls.n_inf);
    for (int i = 0; i < n_all; ++i) {
        const bool infinite = i >= D.n_lights && i < first_point;
        if (infinite) {
            int listed = 0;
            for (int k = 0; k < ls.n_inf; ++k) listed += ls.inf_light[k] == i;
            CHECK(listed == 1, "infinite light %d is in inf_light %d times", i, listed);
            CHECK(ls.bit_trail[i] == 0xffffffffu, "infinite light %d has the bit trail %08x", i, ls.bit_trail[i]);
            continue;
        }
        float power = 0.f;  // what LightBounds::phi is positive with: the largest channel of Le or I
        if (i < D.n_lights) for (int k = 0; k < 3; ++k) power = std::fmax(power, D.quads[D.light_quads[i]].Le[k]);
        else for (int k = 0; k < 3; ++k) power = std::fmax(power, D.point[i - first_point].I[k]);
        if (!(power > 0)) continue;
        CHECK(ls.bit_trail[i] != 0xffffffffu, "bounded light %d has no bit trail", i);
        int node = 0, depth = 0;
        while (node >= 0 && node < ls.n_nodes && !ls.nodes[node].is_leaf && depth < 32) {
            node = (ls.bit_trail[i] >> depth) & 1u ? (int)ls.nodes[node].child_or_light : node + 1;
            ++depth;
        }
        CHECK(node >= 0 && node < ls.n_nodes && ls.nodes[node].is_leaf && (int)ls.nodes[node].child_or_light == i,
              "the trail %08x of light %d ends at node %d after %d steps", ls.bit_trail[i], i, node, depth);
    }
    int leaves = 0;
    for (int n = 0; n < ls.n_nodes; ++n) {
        if (!ls.nodes[n].is_leaf) {
            CHECK((int)ls.nodes[n].child_or_light > n + 1 && (int)ls.nodes[n].child_or_light < ls.n_nodes, "node %d: second child %u", n, ls.nodes[n].child_or_light);
            continue;
        }
        ++leaves;
        const int l = (int)ls.nodes[n].child_or_light;
        CHECK(l >= 0 && l < n_all && !(l >= D.n_lights && l < first_point), "leaf %d names light %d", n, l);
    }
    CHECK(leaves == D.n_lights + D.n_point && ls.n_nodes == 2 * leaves - 1, "%d leaves, %d nodes", leaves, ls.n_nodes);
}

// ---- 3. triangle soup --------------------------------------------------------------------------------------------------------------
struct Box3 { float lo[3], hi[3]; };
static Box3 child_box(const DBvh4Node &N, int k) { return Box3{{N.lox[k], N.loy[k], N.loz[k]}, {N.hix[k], N.hiy[k], N.hiz[k]}}; }
static bool contains(const Box3 &b, const float *p) {
    for (int k = 0; k < 3; ++k) if (!(p[k] >= b.lo[k] && p[k] <= b.hi[k])) return false;
    return true;
}
// levels below and including `node`; counts how often each triangle slot sits in a leaf
static int walk_bvh(const std::vector<DBvh4Node> &nodes, const std::vector<DTri> &tris, int node, std::vector<int> &seen, std::vector<int> &visits) {
    if (node < 0 || node >= (int)nodes.size()) { CHECK(false, "child index %d of %zu nodes", node, nodes.size()); return 0; }
    if (++visits[node] > 1) { CHECK(false, "node %d has two parents", node); return 0; }
    const DBvh4Node &N = nodes[node];
    int depth = 0;
    for (int k = 0; k < 4; ++k) {
        const int32_t c = N.child[k];
        if (c == kBvhAbsent) continue;
        const Box3 b = child_box(N, k);
        if (c >= 0) {
            if (c < (int)nodes.size())
                for (int j = 0; j < 4; ++j) {
                    if (nodes[c].child[j] == kBvhAbsent) continue;
                    const Box3 cb = child_box(nodes[c], j);
                    CHECK(contains(b, cb.lo) && contains(b, cb.hi), "node %d child %d: its box does not contain box %d of node %d", node, k, j, c);
                }
            const int d = walk_bvh(nodes, tris, c, seen, visits);
            depth = d > depth ? d : depth;
        } else {
            const int leaf = -(c + 1), first = leaf / 8, count = leaf % 8;
            CHECK(count >= 1 && count <= 7 && first >= 0 && first + count <= (int)tris.size(), "node %d child %d: leaf of %d triangles from %d", node, k, count, first);
            for (int t = first; t < first + count && t < (int)tris.size(); ++t) {
                if (t < 0) continue;
                ++seen[t];
                CHECK(contains(b, tris[t].p0) && contains(b, tris[t].p1) && contains(b, tris[t].p2), "node %d child %d: triangle slot %d sticks out of its leaf's box", node, k, t);
            }
        }
    }
    return depth + 1;
}
static void test_triangle_soup() {
    Lcg rng(0x7261796cull);
    std::vector<float> p;
    for (int t = 0; t < 96; ++t) {
        float c[3];
        for (int k = 0; k < 3; ++k) c[k] = 2.f * rng.next() - 1.f;
        for (int v = 0; v < 3; ++v)
            for (int k = 0; k < 3; ++k) p.push_back(c[k] + 0.2f * (rng.next() - 0.5f));
    }
    const float one[9] = {0.1f, 0.2f, 0.3f, 0.4f, 0.25f, 0.3f, 0.2f, 0.5f, 0.35f};
    for (int t = 0; t < 200; ++t) p.insert(p.end(), one, one + 9);  // identical centroids: no plane separates them
    static VspgScene sc;
    std::memset(&sc, 0, sizeof sc);
    sc.n_triangles = (int)(p.size() / 9);
    sc.tri_p = p.data();
    std::vector<DTri> tris;
    std::vector<DBvh4Node> nodes;
    CHECK(build_triangle_bvh(sc, &tris, &nodes) == 0, "%s", vspg_last_error());
    std::set<int> accepted;
    for (int t = 0; t < sc.n_triangles; ++t) {
        DTri T;
        if (derive_triangle(sc.tri_p + 9 * (size_t)t, nullptr, t, &T)) accepted.insert(t);
    }
    CHECK(accepted.size() == 296u, "%zu of 296 triangles accepted (none of them is degenerate)", accepted.size());
    CHECK(tris.size() == accepted.size(), "%zu triangles in leaf order, %zu accepted", tris.size(), accepted.size());
    CHECK(!nodes.empty(), "no nodes");
    if (nodes.empty()) return;
    std::vector<int> seen(tris.size(), 0), visits(nodes.size(), 0);
    const int depth = walk_bvh(nodes, tris, 0, seen, visits);
    std::set<int> ids;
    for (size_t t = 0; t < tris.size(); ++t) {
        CHECK(seen[t] == 1, "triangle slot %zu is in %d leaves", t, seen[t]);
        CHECK(accepted.count(tris[t].id) == 1, "slot %zu holds triangle %d, which derive_triangle refuses", t, tris[t].id);
        ids.insert(tris[t].id);
    }
    CHECK(ids == accepted, "%zu different triangles in the leaves, %zu accepted", ids.size(), accepted.size());
    for (size_t n = 0; n < nodes.size(); ++n) CHECK(visits[n] == 1, "node %zu is reached %d times", n, visits[n]);
    CHECK(3 * depth + 1 <= kBvhStack, "depth %d needs %d stack entries, the traversal has %d", depth, 3 * depth + 1, kBvhStack);
    std::printf("triangle soup: %zu triangles, %zu nodes, depth %d\n", tris.size(), nodes.size(), depth);
}

// ---- 4. majorants ------------------------------------------------------------------------------------------------------------------
static void test_majorants(int type, int nx, int ny, int nz, uint64_t seed) {
    Lcg rng(seed);
    std::vector<float> d((size_t)nx * ny * nz);
    for (float &v : d) v = rng.next() < 0.3f ? 0.f : 4.f * rng.next();
    VspgMedium m;
    std::memset(&m, 0, sizeof m);
    m.type = type;
    m.nx = nx; m.ny = ny; m.nz = nz;
    m.density = d.data();
    m.density_offset = 0.25f;
    m.majorant_scale = 1.5f;
    const int n[3] = {nx, ny, nz};
    for (int k = 0; k < 3; ++k) {
        m.index_min[k] = -3 + 2 * k;
        m.voxel_size[k] = 0.125f;
        m.grid_origin[k] = 0.05f * (float)k;
        // the world box of the index box, as a .nvdb's bounding box is: [index_min, index_min + n] * voxel_size + origin
        m.bounds_min[k] = m.grid_origin[k] + (float)m.index_min[k] * m.voxel_size[k];
        m.bounds_max[k] = m.grid_origin[k] + (float)(m.index_min[k] + n[k]) * m.voxel_size[k];
    }
    // GridMedium has neither a density offset nor a majorant scale (media.cpp:262-269): its majorant bounds the samples themselves
    const float offset = type == VSPG_MEDIUM_NANOVDB ? m.density_offset : 0.f, scale = type == VSPG_MEDIUM_NANOVDB ? m.majorant_scale : 1.f;
    const int R = majorant_res(m);
    CHECK(R == (type == VSPG_MEDIUM_NANOVDB ? kMajResNvdb : kMajRes), "majorant_res %d", R);
    const std::vector<float> maj = type == VSPG_MEDIUM_NANOVDB ? build_majorant_grid_nvdb(m) : build_majorant_grid(m);
    const std::vector<int2> ranges = majorant_axis_ranges(m);
    CHECK(maj.size() == (size_t)R * R * R, "%zu majorants, R = %d", maj.size(), R);
    CHECK(ranges.size() == (size_t)3 * R, "%zu axis ranges", ranges.size());
    if (maj.size() != (size_t)R * R * R || ranges.size() != (size_t)3 * R) return;
    for (int k = 0; k < 3; ++k) {  // the cells' ranges stay inside the grid and leave no voxel out
        std::vector<int> covered(n[k], 0);
        for (int c = 0; c < R; ++c) {
            const int2 r = ranges[(size_t)k * R + c];
            CHECK(r.x >= 0 && r.y <= n[k] - 1, "axis %d cell %d: range [%d, %d] of %d voxels", k, c, r.x, r.y, n[k]);
            for (int v = r.x < 0 ? 0 : r.x; v <= r.y && v < n[k]; ++v) covered[v] = 1;
        }
        for (int v = 0; v < n[k]; ++v) CHECK(covered[v], "axis %d: voxel %d is in no cell's range", k, v);
    }
    long long bad = 0, pairs = 0;
    for (int z = 0; z < R; ++z)
        for (int y = 0; y < R; ++y)
            for (int x = 0; x < R; ++x) {
                const int2 rx = ranges[x], ry = ranges[R + y], rz = ranges[2 * R + z];
                const float mj = maj[x + (size_t)R * (y + (size_t)R * z)];
                for (int zz = rz.x; zz <= rz.y; ++zz)
                    for (int yy = ry.x; yy <= ry.y; ++yy)
                        for (int xx = rx.x; xx <= rx.y; ++xx) {
                            if (xx < 0 || yy < 0 || zz < 0 || xx >= nx || yy >= ny || zz >= nz) continue;  // (reported above)
                            ++pairs;
                            if (!(mj >= (d[((size_t)zz * ny + yy) * nx + xx] + offset) * scale)) ++bad;
                        }
            }
    CHECK(bad == 0, "%lld of %lld (cell, voxel) pairs have a majorant below the voxel's value", bad, pairs);
    CHECK(pairs >= (long long)d.size(), "only %lld (cell, voxel) pairs for %zu voxels", pairs, d.size());
}

// ---- 5. environment tables ---------------------------------------------------------------------------------------------------------
static void check_cdf(const float *cdf, int n, const char *what, int row) {
    CHECK(cdf[0] == 0.f && cdf[n] == 1.f, "%s %d runs from %g to %g", what, row, cdf[0], cdf[n]);
    for (int i = 0; i < n; ++i) CHECK(cdf[i + 1] >= cdf[i], "%s %d decreases at %d: %g then %g", what, row, i, cdf[i], cdf[i + 1]);
}
static void test_env_tables(int res, int black_row) {
    Lcg rng(0x656e76ull + (uint64_t)res);
    std::vector<float> rgb((size_t)3 * res * res);
    for (float &v : rgb) v = 0.05f + 3.f * rng.next();
    if (black_row >= 0)
        for (int i = 0; i < 3 * res; ++i) rgb[(size_t)3 * res * black_row + i] = 0.f;
    EnvTables T;
    env_build_tables(rgb.data(), res, &T);
    CHECK(T.res == res, "res %d", T.res);
    CHECK(T.buf.size() == T.o_mcdf + (size_t)res + 1 && T.o_func == (size_t)3 * res * res && T.o_cdf == T.o_func + (size_t)res * res &&
              T.o_mfunc == T.o_cdf + (size_t)res * (res + 1) && T.o_mcdf == T.o_mfunc + (size_t)res,
          "layout: %zu floats, offsets %zu %zu %zu %zu", T.buf.size(), T.o_func, T.o_cdf, T.o_mfunc, T.o_mcdf);
    if (T.buf.size() != T.o_mcdf + (size_t)res + 1) return;
    CHECK(std::memcmp(T.buf.data(), rgb.data(), rgb.size() * sizeof(float)) == 0, "the texels are not the image");
    for (int v = 0; v < res; ++v) check_cdf(T.buf.data() + T.o_cdf + (size_t)v * (res + 1), res, "the conditional CDF of row", v);
    check_cdf(T.buf.data() + T.o_mcdf, res, "the marginal CDF", 0);
    CHECK(T.integral > 0.f && std::isfinite(T.integral), "integral %g", T.integral);
}
static void test_env_matrices() {
    float m[9], mi[9];
    CHECK(env_matrices(nullptr, m, mi), "nullptr refused");
    for (int k = 0; k < 9; ++k) CHECK(m[k] == (k % 4 == 0 ? 1.f : 0.f) && mi[k] == m[k], "nullptr: m[%d] = %g, mi[%d] = %g", k, m[k], k, mi[k]);
    const float singular[12] = {1, 2, 3, 9, 2, 4, 6, 9, 0, 1, 0, 9};  // row 1 = 2 * row 0
    CHECK(!env_matrices(singular, m, mi), "a singular matrix accepted");
    float nan[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    nan[5] = std::nanf("");
    CHECK(!env_matrices(nan, m, mi), "a NaN matrix accepted");
    const float rot[12] = {0, -2, 0, 5, 1, 0, 0, 6, 0, 0, 4, 7};  // regular: m * mi = 1
    CHECK(env_matrices(rot, m, mi), "a regular matrix refused");
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            float s = 0;
            for (int k = 0; k < 3; ++k) s += m[3 * r + k] * mi[3 * k + c];
            CHECK(std::fabs(s - (r == c ? 1.f : 0.f)) <= 1e-6f, "(m * mi)[%d][%d] = %g", r, c, s);
        }
}

// ---- 6. validate's refusals --------------------------------------------------------------------------------------------------------
static void refused(const VspgScene &sc, const VspgIntegratorParams &prm, const char *message) {
    const VspgRenderConfig cfg = config(16, 16);
    const int rc = validate(&sc, &prm, &cfg);
    CHECK(rc == VSPG_EINVAL, "returned %d, expected VSPG_EINVAL for: %s", rc, message);
    CHECK(std::string(vspg_last_error()) == message, "message \"%s\", expected \"%s\"", vspg_last_error(), message);
}
static void test_validate_refusals() {
    static VspgScene base, sc;
    VspgIntegratorParams prm0, prm;
    vspg_integrator_params_default(&prm0);
    CHECK(vspg_scene_fog_box(&base, 16, 16) == 0, "%s", vspg_last_error());
    prm = prm0;
    prm.maxdepth = 255;
    refused(base, prm, "maxdepth above 254 (the path depth travels in 8 bits of the packed path flags)");
    sc = base;
    sc.n_quads = VSPG_MAX_QUADS + 1;
    refused(sc, prm0, "n_quads out of range");
    sc = base;
    sc.n_point_lights = 1;
    {
        const float from[3] = {0.f, 0.5f, 0.f}, to[3] = {0.f, -1.f, 0.f};
        VspgPointLight &S = sc.point_lights[0];
        S.type = VSPG_LIGHT_SPOT;
        S.I[0] = S.I[1] = S.I[2] = 1.f;
        S.cone_angle_deg = 20.f;
        S.cone_delta_deg = 25.f;
        CHECK(vspg_spot_light_look_at(&S, from, to, nullptr) == 0, "%s", vspg_last_error());
    }
    refused(sc, prm0, "a spot light's cone_delta_deg exceeds cone_angle_deg");
    sc = base;
    sc.medium.type = VSPG_MEDIUM_GRID;
    sc.medium.nx = sc.medium.ny = sc.medium.nz = 4;
    sc.medium.density = nullptr;
    for (int k = 0; k < 3; ++k) { sc.medium.bounds_min[k] = -1.f; sc.medium.bounds_max[k] = 1.f; }
    refused(sc, prm0, "grid medium needs nx,ny,nz > 0 and a density array");
}

int main() {
    test_fog_box();
    test_many_lights(VSPG_LIGHTSAMPLER_POWER);
    test_many_lights(VSPG_LIGHTSAMPLER_BVH);
    test_triangle_soup();
    test_majorants(VSPG_MEDIUM_GRID, 5, 4, 3, 0x67726964ull);
    test_majorants(VSPG_MEDIUM_NANOVDB, 9, 7, 5, 0x6e766462ull);
    test_env_tables(1, -1);
    test_env_tables(4, 2);
    test_env_matrices();
    test_validate_refusals();
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("scene_build_check: all checks passed\n");
    return 0;
}
