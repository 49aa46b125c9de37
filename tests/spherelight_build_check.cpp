// spherelight_build_check.cpp -- the host side of sphere area lights (csrc/vspg_scene_build.hip: build_dscene, lsb::build, validate)
// run on the CPU.
//
// tests/test_spherelight_model.py compiles the two host-only units and this program with the library's flags plus AddressSanitizer
// and UndefinedBehaviorSanitizer, links them WITHOUT the HIP runtime and runs the result: exit status 0 and no sanitizer report.
// The known answers are derived by hand beside each check.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

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

static VspgRenderConfig config(int xres, int yres) {
    VspgRenderConfig cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.xres = xres; cfg.yres = yres; cfg.spp = 1; cfg.shard_count = 1;
    return cfg;
}
static void sphere_at(VspgScene *sc, float x, float y, float z, float radius) {
    VspgSphere &sp = sc->spheres[sc->n_spheres++];
    std::memset(&sp, 0, sizeof sp);
    for (int k = 0; k < 4; ++k) sp.render_from_object[5 * k] = sp.object_from_render[5 * k] = 1.f;
    sp.render_from_object[3] = x; sp.render_from_object[7] = y; sp.render_from_object[11] = z;
    sp.object_from_render[3] = -x; sp.object_from_render[7] = -y; sp.object_from_render[11] = -z;
    sp.radius = radius;
    sp.Kd[0] = sp.Kd[1] = sp.Kd[2] = 0.5f;
}

// Two sphere lights and nothing else that emits.  Sphere 0: radius 1, L = 1, one-sided: Phi = Pi * area * L = Pi * 4 Pi = 4 Pi^2.  Sphere 2
// (sphere 1 is not a light): radius 2, L = 0.5, two-sided: Phi = Pi * 2 * 16 Pi * 0.5 = 16 Pi^2.  The power sampler's pmfs are 1 / 5 and
// 4 / 5 whatever lambda.PDF() is (the lights are grey: the same factor on both); the alias table of (1 / 5, 4 / 5): pHat = (2 / 5, 8 / 5),
// so q[0] = 2 / 5 with alias 1 and q[1] = 1.
static void test_two_sphere_lights(int lightsampler) {
    static VspgScene sc;
    static DScene D;
    std::memset(&sc, 0, sizeof sc);
    VspgIntegratorParams prm;
    vspg_integrator_params_default(&prm);
    prm.lightsampler = lightsampler;
    const VspgRenderConfig cfg = config(16, 16);
    const float eye[3] = {0, 0, -20}, look[3] = {0, 0, 0}, up[3] = {0, 1, 0};
    CHECK(vspg_camera_look_at(&sc.camera, eye, look, up, 40.f, 16, 16) == 0, "%s", vspg_last_error());
    sphere_at(&sc, -3.f, 0.f, 0.f, 1.f);
    sphere_at(&sc, 0.f, 5.f, 0.f, 0.25f);
    sphere_at(&sc, 4.f, 1.f, 2.f, 2.f);
    for (int k = 0; k < 3; ++k) { sc.sphere_Le[0][k] = 1.f; sc.sphere_Le[2][k] = 0.5f; }
    sc.sphere_two_sided[2] = 1;
    CHECK(validate(&sc, &prm, &cfg) == 0, "%s", vspg_last_error());
    build_dscene(sc, prm, cfg, &D);
    const DLightSampler &ls = D.lsamp;
    CHECK(D.n_lights == 0 && D.n_inf == 0 && D.n_point == 0 && D.n_sphere_lights == 2 && light_list_size(D) == 2, "%d %d %d %d", D.n_lights, D.n_inf, D.n_point, D.n_sphere_lights);
    CHECK(D.light_spheres[0] == 0 && D.light_spheres[1] == 2, "light_spheres %d %d", D.light_spheres[0], D.light_spheres[1]);
    CHECK(D.sphere_light[0].light == 0 && D.sphere_light[1].light == -1 && D.sphere_light[2].light == 1, "light indices %d %d %d", D.sphere_light[0].light,
          D.sphere_light[1].light, D.sphere_light[2].light);
    CHECK(ls.light_of_sphere[0] == 0 && ls.light_of_sphere[1] == -1 && ls.light_of_sphere[2] == 1, "light_of_sphere %d %d %d", ls.light_of_sphere[0], ls.light_of_sphere[1],
          ls.light_of_sphere[2]);
    for (int i = 3; i < VSPG_MAX_SPHERES; ++i) CHECK(ls.light_of_sphere[i] == -1 && D.sphere_light[i].light == -1, "slot %d", i);
    CHECK(ls.mode == lightsampler, "mode %d", ls.mode);
    const double pi = 3.14159265358979323846;
    CHECK(std::fabs(1. / D.sphere_light[0].inv_area / (4 * pi) - 1) <= 4 * 0x1p-24 && std::fabs(1. / D.sphere_light[2].inv_area / (16 * pi) - 1) <= 4 * 0x1p-24,
          "areas %g %g", 1. / D.sphere_light[0].inv_area, 1. / D.sphere_light[2].inv_area);
    CHECK(D.sphere_light[2].center[0] == 4.f && D.sphere_light[2].center[1] == 1.f && D.sphere_light[2].center[2] == 2.f, "centre");
    CHECK(D.sphere_light[2].two_sided == 1 && D.sphere_light[0].two_sided == 0 && D.sphere_light[0].reverse == 0, "flags");
    // the alias table
    CHECK(ls.n_alias == 2, "n_alias %d", ls.n_alias);
    CHECK(std::fabs(ls.alias_p[0] - 0.2) <= 16 * 0x1p-24 && std::fabs(ls.alias_p[1] - 0.8) <= 16 * 0x1p-24, "alias_p %g %g", ls.alias_p[0], ls.alias_p[1]);
    CHECK(std::fabs(ls.alias_q[0] - 0.4) <= 32 * 0x1p-24 && ls.alias_i[0] == 1 && ls.alias_q[1] == 1.f && ls.alias_i[1] == -1, "alias q %g -> %d, %g -> %d", ls.alias_q[0],
          ls.alias_i[0], ls.alias_q[1], ls.alias_i[1]);
    // the BVH sampler's tree: both lights are bounded, two leaves under one root; a leaf's box (after CompactLightBounds' 16-bit
    // quantisation against the union box [-4, 6] x [-1, 3] x [-2, 4], whose cell is at most 10 / 65535) contains the sphere's box
    // centre +- radius; EntireSphere: cosTheta_o = -1; cosTheta_e = cos(Pi / 2); phi = max(L) * area * Pi
    CHECK(ls.n_nodes == 3 && ls.n_inf == 0, "%d nodes, %d infinite", ls.n_nodes, ls.n_inf);
    int leaves = 0;
    for (int n = 0; n < ls.n_nodes; ++n) {
        const DLightNode &N = ls.nodes[n];
        if (!N.is_leaf) continue;
        ++leaves;
        const int l = (int)N.child_or_light;
        CHECK(l == 0 || l == 1, "leaf %d names light %d", n, l);
        if (l != 0 && l != 1) continue;
        const int si = D.light_spheres[l];
        const float r = D.spheres[si].radius, tol = 2.f * 10.f / 65535.f;
        for (int k = 0; k < 3; ++k) {
            const float c = D.sphere_light[si].center[k];
            CHECK(N.bmin[k] <= c - r + 1e-6f && N.bmin[k] >= c - r - tol && N.bmax[k] >= c + r - 1e-6f && N.bmax[k] <= c + r + tol, "light %d axis %d: [%g, %g] around %g +- %g", l, k,
                  N.bmin[k], N.bmax[k], c, r);
        }
        const double phi = (l == 0 ? 1. * 4 * pi : 0.5 * 16 * pi) * pi;
        CHECK(std::fabs(N.phi / phi - 1) <= 8 * 0x1p-24, "light %d: phi %g, expected %g", l, N.phi, phi);
        CHECK(N.cosTheta_o <= -0.999f && std::fabs(N.cosTheta_e) <= 1e-3f && N.twoSided == (l == 1), "light %d: cosTheta_o %g cosTheta_e %g twoSided %d", l, N.cosTheta_o,
              N.cosTheta_e, N.twoSided);
        // the light's bit trail leads to this leaf
        int node = 0, depth = 0;
        while (node >= 0 && node < ls.n_nodes && !ls.nodes[node].is_leaf && depth < 32) {
            node = (ls.bit_trail[l] >> depth) & 1u ? (int)ls.nodes[node].child_or_light : node + 1;
            ++depth;
        }
        CHECK(node == n, "the trail %08x of light %d ends at node %d, its leaf is %d", ls.bit_trail[l], l, node, n);
    }
    CHECK(leaves == 2, "%d leaves", leaves);
}

// every light kind at once: the fourth range starts behind the point lights
static void test_light_list_order() {
    static VspgScene sc;
    static DScene D;
    VspgIntegratorParams prm;
    vspg_integrator_params_default(&prm);
    prm.lightsampler = VSPG_LIGHTSAMPLER_BVH;
    const VspgRenderConfig cfg = config(16, 16);
    CHECK(vspg_scene_fog_box(&sc, 16, 16) == 0, "%s", vspg_last_error());      // one emissive rectangle
    sc.n_infinite_lights = 1;
    sc.infinite_lights[0].type = VSPG_LIGHT_UNIFORM_INFINITE;
    sc.infinite_lights[0].L[0] = sc.infinite_lights[0].L[1] = sc.infinite_lights[0].L[2] = 0.1f;
    sc.n_point_lights = 1;
    std::memset(&sc.point_lights[0], 0, sizeof sc.point_lights[0]);
    sc.point_lights[0].type = VSPG_LIGHT_POINT;
    sc.point_lights[0].I[0] = sc.point_lights[0].I[1] = sc.point_lights[0].I[2] = 1.f;
    const float from[3] = {0.1f, 0.2f, 0.3f};
    CHECK(vspg_point_light_at(&sc.point_lights[0], from, nullptr) == 0, "%s", vspg_last_error());
    for (int i = 0; i < VSPG_MAX_SPHERES; ++i) {      // every sphere slot in use, every second one a light
        sphere_at(&sc, -0.7f + 0.2f * (float)i, -0.5f, 0.2f, 0.05f);
        if (i % 2) sc.sphere_Le[i][1] = 2.f;
    }
    CHECK(validate(&sc, &prm, &cfg) == 0, "%s", vspg_last_error());
    build_dscene(sc, prm, cfg, &D);
    CHECK(D.n_lights == 1 && D.n_inf == 1 && D.n_point == 1 && D.n_sphere_lights == VSPG_MAX_SPHERES / 2, "%d %d %d %d", D.n_lights, D.n_inf, D.n_point, D.n_sphere_lights);
    for (int k = 0; k < D.n_sphere_lights; ++k) {
        const int si = D.light_spheres[k];
        CHECK(si == 2 * k + 1 && D.sphere_light[si].light == 3 + k && D.lsamp.light_of_sphere[si] == 3 + k, "emissive sphere %d: sphere %d, light %d / %d", k, si,
              D.sphere_light[si].light, D.lsamp.light_of_sphere[si]);
    }
    const int n_all = light_list_size(D);
    CHECK(n_all == 3 + VSPG_MAX_SPHERES / 2 && D.lsamp.n_alias == n_all && n_all <= kMaxLights, "%d lights", n_all);
    int leaves = 0;
    for (int n = 0; n < D.lsamp.n_nodes; ++n) leaves += D.lsamp.nodes[n].is_leaf ? 1 : 0;
    CHECK(leaves == n_all - 1 && D.lsamp.n_nodes == 2 * leaves - 1 && D.lsamp.n_nodes <= 2 * kMaxLights, "%d leaves, %d nodes", leaves, D.lsamp.n_nodes);
    double sum = 0;
    for (int i = 0; i < n_all; ++i) sum += (double)D.lsamp.alias_p[i];
    CHECK(std::fabs(sum - 1.) <= n_all * 0x1p-23, "alias_p sums to 1 %+g", sum - 1.);
}

static void refused(const VspgScene &sc, int code, const char *needle) {
    VspgIntegratorParams prm;
    vspg_integrator_params_default(&prm);
    const VspgRenderConfig cfg = config(16, 16);
    const int rc = validate(&sc, &prm, &cfg);
    CHECK(rc == code, "returned %d, expected %d for: %s", rc, code, needle);
    CHECK(std::string(vspg_last_error()).find(needle) != std::string::npos, "message \"%s\" does not name \"%s\"", vspg_last_error(), needle);
}
static void test_validate_refusals() {
    static VspgScene base, sc;
    CHECK(vspg_scene_fog_box(&base, 16, 16) == 0, "%s", vspg_last_error());
    sphere_at(&base, 0.f, 0.f, 0.f, 0.2f);
    base.sphere_Le[0][0] = 1.f;
    VspgIntegratorParams prm;
    vspg_integrator_params_default(&prm);
    const VspgRenderConfig cfg = config(16, 16);
    CHECK(validate(&base, &prm, &cfg) == 0, "%s", vspg_last_error());
    sc = base; sc.sphere_Le[0][1] = -0.5f;            refused(sc, VSPG_EINVAL, "Le must be finite and >= 0");
    sc = base; sc.sphere_Le[0][2] = std::nanf("");    refused(sc, VSPG_EINVAL, "Le must be finite and >= 0");
    sc = base; sc.sphere_Le[0][0] = INFINITY;         refused(sc, VSPG_EINVAL, "Le must be finite and >= 0");
    sc = base; sc.sphere_two_sided[0] = 3;            refused(sc, VSPG_EINVAL, "two_sided must be 0 or 1");
    sc = base; sc.spheres[0].material = VSPG_MATERIAL_INTERFACE;  refused(sc, VSPG_ESCOPE, "an emissive sphere with Material \"interface\"");
    sc = base; sc.spheres[0].material = VSPG_MATERIAL_INTERFACE; sc.sphere_Le[0][0] = 0.f;      // not emissive: legal
    CHECK(validate(&sc, &prm, &cfg) == 0, "%s", vspg_last_error());
    sc = base; sc.sphere_Le[5][0] = -1.f;             // beyond n_spheres: not looked at
    CHECK(validate(&sc, &prm, &cfg) == 0, "%s", vspg_last_error());
}

int main() {
    test_two_sphere_lights(VSPG_LIGHTSAMPLER_POWER);
    test_two_sphere_lights(VSPG_LIGHTSAMPLER_BVH);
    test_light_list_order();
    test_validate_refusals();
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("spherelight_build_check: all checks passed\n");
    return 0;
}
