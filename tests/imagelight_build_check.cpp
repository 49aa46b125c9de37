// imagelight_build_check.cpp -- the host side of projection and goniometric lights (csrc/vspg_scene_build.hip: image_light_refusal,
// image_light_build, build_dscene, lsb::build, validate; csrc/vspg_scene_api.hip: the two transform helpers) run on the CPU.
//
// tests/test_imagelight_model.py compiles the two host-only units and this program with the library's flags plus AddressSanitizer
// and UndefinedBehaviorSanitizer, links them WITHOUT the HIP runtime and runs the result on case files it wrote from the NumPy model
// (tests/imagelight_model.py): exit status 0 and no sanitizer report.  A case file holds, little-endian:
//   int32 type, xres, yres; float fov; the pixels (xres * yres * channels floats); int32 n; the device image the model expects (n floats);
//   then the model's screen window (4), screenFromLight rows 0, 1, 3 (12), A, Phi's sums (3), Bounds' sum, cosTotalWidth, and the
//   LightBounds phi of a light with I = (0.5, 2, 1) holding that image
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
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

static bool same_bits(const float *a, const float *b, size_t n) { return std::memcmp(a, b, n * sizeof(float)) == 0; }

static VspgRenderConfig config(int xres, int yres) {
    VspgRenderConfig cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.xres = xres; cfg.yres = yres; cfg.spp = 1; cfg.shard_count = 1;
    return cfg;
}

// a scene with one light of `type` under the helper's own transform and nothing else
static void one_light_scene(VspgScene *sc, int type, float fov) {
    std::memset(sc, 0, sizeof *sc);
    const float eye[3] = {0, 0, -5}, look[3] = {0, 0, 0}, up[3] = {0, 1, 0};
    CHECK(vspg_camera_look_at(&sc->camera, eye, look, up, 40.f, 16, 16) == 0, "%s", vspg_last_error());
    sc->n_point_lights = 1;
    VspgPointLight &l = sc->point_lights[0];
    l.type = type;
    l.I[0] = 0.5f; l.I[1] = 2.f; l.I[2] = 1.f;
    const float ctm[16] = {0, -1, 0, 0.5f, 1, 0, 0, -0.25f, 0, 0, 1, 2.f, 0, 0, 0, 1};  // a quarter turn about z, then a translation
    CHECK((type == VSPG_LIGHT_PROJECTION ? vspg_projection_light_at(&l, ctm) : vspg_goniometric_light_at(&l, ctm)) == 0, "%s", vspg_last_error());
    l.cone_angle_deg = fov;  // a projection slot's field of view
}

static void test_case_file(const char *path) {
    std::FILE *f = std::fopen(path, "rb");
    CHECK(f != nullptr, "cannot open %s", path);
    if (!f) return;
    int32_t head[3];
    float fov;
    bool ok = std::fread(head, 4, 3, f) == 3 && std::fread(&fov, 4, 1, f) == 1;
    const int type = head[0], xres = head[1], yres = head[2], channels = type == VSPG_LIGHT_PROJECTION ? 3 : 1;
    std::vector<float> pixels((size_t)xres * yres * channels), want_buf;
    ok = ok && std::fread(pixels.data(), 4, pixels.size(), f) == pixels.size();
    int32_t n = 0;
    ok = ok && std::fread(&n, 4, 1, f) == 1;
    want_buf.resize(ok ? (size_t)n : 0);
    ok = ok && std::fread(want_buf.data(), 4, want_buf.size(), f) == want_buf.size();
    float want[23];
    ok = ok && std::fread(want, 4, 23, f) == 23;
    std::fclose(f);
    CHECK(ok, "short case file %s", path);
    if (!ok) return;
    CHECK(image_light_refusal(type, pixels.data(), xres, yres, channels) == 0, "%s: %s", path, vspg_last_error());
    ImageLightTables T;
    image_light_build(type, pixels.data(), xres, yres, fov, &T);
    CHECK(T.xres == xres && T.yres == yres && T.buf.size() == want_buf.size(), "%s: %d x %d, %zu floats", path, T.xres, T.yres, T.buf.size());
    if (T.buf.size() == want_buf.size()) CHECK(same_bits(T.buf.data(), want_buf.data(), want_buf.size()), "%s: the device image differs from the model's", path);
    if (type == VSPG_LIGHT_PROJECTION) {
        CHECK(same_bits(T.sb, want, 4), "%s: screenBounds %g %g %g %g, model %g %g %g %g", path, T.sb[0], T.sb[1], T.sb[2], T.sb[3], want[0], want[1], want[2], want[3]);
        CHECK(same_bits(T.sfl, want + 4, 12), "%s: screenFromLight rows", path);
        CHECK(same_bits(&T.A, want + 16, 1), "%s: A %.9g, model %.9g", path, T.A, want[16]);
        CHECK(same_bits(T.sum_phi, want + 17, 3), "%s: Phi sums %.9g %.9g %.9g, model %.9g %.9g %.9g", path, T.sum_phi[0], T.sum_phi[1], T.sum_phi[2], want[17], want[18], want[19]);
        CHECK(same_bits(&T.cosTotalWidth, want + 21, 1), "%s: cosTotalWidth %.9g, model %.9g", path, T.cosTotalWidth, want[21]);
        CHECK(T.hither == 1e-3f, "hither %g", T.hither);
    } else {
        CHECK(same_bits(T.sum_phi, want + 17, 1), "%s: sumY %.9g, model %.9g", path, T.sum_phi[0], want[17]);
    }
    CHECK(same_bits(&T.sum_bounds, want + 20, 1), "%s: Bounds sum %.9g, model %.9g", path, T.sum_bounds, want[20]);
    // through the scene build: the light's leaf in the BVH holds the model's LightBounds phi once the image is in the record
    static VspgScene sc;
    static DScene D;
    one_light_scene(&sc, type, fov);
    VspgIntegratorParams prm;
    vspg_integrator_params_default(&prm);
    prm.lightsampler = VSPG_LIGHTSAMPLER_BVH;
    const VspgRenderConfig cfg = config(16, 16);
    CHECK(validate(&sc, &prm, &cfg) == 0, "%s", vspg_last_error());
    build_dscene(sc, prm, cfg, &D);
    CHECK(D.n_point == 1 && light_list_size(D) == 1 && D.image_light[0].xres == 1 && D.image_light[0].yres == 1 && D.image_light[0].texels == nullptr,
          "%d lights, image %d x %d", light_list_size(D), D.image_light[0].xres, D.image_light[0].yres);
    image_light_apply(T, &D.image_light[0]);
    lsb::build(sc, prm, &D);
    CHECK(D.lsamp.n_nodes == 1 && D.lsamp.nodes[0].is_leaf, "%d nodes", D.lsamp.n_nodes);
    CHECK(same_bits(&D.lsamp.nodes[0].phi, want + 22, 1), "%s: LightBounds phi %.9g, model %.9g", path, D.lsamp.nodes[0].phi, want[22]);
    CHECK(D.lsamp.nodes[0].bmin[0] == 0.5f && D.lsamp.nodes[0].bmin[1] == -0.25f && D.lsamp.nodes[0].bmin[2] == 2.f, "the light's position");
}

static void test_refusals() {
    float px[3 * 4] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12};
    const int P = VSPG_LIGHT_PROJECTION, G = VSPG_LIGHT_GONIOMETRIC;
    CHECK(image_light_refusal(P, nullptr, 2, 2, 3) == VSPG_EINVAL, "null pixels");
    CHECK(image_light_refusal(VSPG_LIGHT_SPOT, px, 2, 2, 3) == VSPG_EINVAL && std::strstr(vspg_last_error(), "neither"), "%s", vspg_last_error());
    CHECK(image_light_refusal(P, px, 2, 2, 1) == VSPG_EINVAL && std::strstr(vspg_last_error(), "3 channels"), "%s", vspg_last_error());
    CHECK(image_light_refusal(G, px, 2, 2, 3) == VSPG_EINVAL && std::strstr(vspg_last_error(), "1 channel"), "%s", vspg_last_error());
    CHECK(image_light_refusal(P, px, 0, 2, 3) == VSPG_EINVAL && std::strstr(vspg_last_error(), "resolution"), "%s", vspg_last_error());
    CHECK(image_light_refusal(P, px, 2, VSPG_LIGHT_IMAGE_MAX_RES + 1, 3) == VSPG_EINVAL && std::strstr(vspg_last_error(), "resolution"), "%s", vspg_last_error());
    CHECK(image_light_refusal(G, px, 4, 3, 1) == VSPG_EINVAL && std::strstr(vspg_last_error(), "non-square"), "%s", vspg_last_error());
    CHECK(image_light_refusal(P, px, 2, 2, 3) == 0 && image_light_refusal(G, px, 3, 3, 1) == 0 && image_light_refusal(P, px, 4, 1, 3) == 0, "%s", vspg_last_error());
    px[7] = NAN;
    CHECK(image_light_refusal(P, px, 2, 2, 3) == VSPG_EINVAL && std::strstr(vspg_last_error(), "not-a-number"), "%s", vspg_last_error());
    CHECK(image_light_refusal(G, px, 3, 3, 1) == VSPG_EINVAL && std::strstr(vspg_last_error(), "not-a-number"), "%s", vspg_last_error());
    px[7] = -INFINITY;
    CHECK(image_light_refusal(P, px, 2, 2, 3) == VSPG_EINVAL && std::strstr(vspg_last_error(), "infinite"), "%s", vspg_last_error());
    // create's refusals: the field of view of a projection slot, the transform of a goniometric slot
    static VspgScene sc;
    VspgIntegratorParams prm;
    vspg_integrator_params_default(&prm);
    const VspgRenderConfig cfg = config(16, 16);
    const float bad_fov[] = {0.f, 180.f, -30.f, NAN};
    for (float fov : bad_fov) {
        one_light_scene(&sc, P, fov);
        CHECK(validate(&sc, &prm, &cfg) == VSPG_EINVAL && std::strstr(vspg_last_error(), "field of view"), "fov %g: %s", fov, vspg_last_error());
    }
    one_light_scene(&sc, G, 0.f);  // (a goniometric slot's fov is not read)
    CHECK(validate(&sc, &prm, &cfg) == 0, "%s", vspg_last_error());
    sc.point_lights[0].light_from_render[0] = 1.001f;  // row 0 = (1.001, 1, 0) after the quarter turn's: not a unit vector
    CHECK(validate(&sc, &prm, &cfg) == VSPG_ESCOPE && std::strstr(vspg_last_error(), "orthonormal"), "%s", vspg_last_error());
    one_light_scene(&sc, G, 0.f);
    for (int k = 0; k < 12; ++k) sc.point_lights[0].light_from_render[k] *= 0.5f;  // a uniform scale
    for (int k = 0; k < 12; ++k) sc.point_lights[0].render_from_light[k] *= (k % 4 == 3 ? 1.f : 2.f);
    CHECK(validate(&sc, &prm, &cfg) == VSPG_ESCOPE, "%s", vspg_last_error());
    sc.point_lights[0].type = 7;
    CHECK(validate(&sc, &prm, &cfg) == VSPG_EINVAL && std::strstr(vspg_last_error(), "unknown point light type"), "%s", vspg_last_error());
}

int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) test_case_file(argv[i]);
    test_refusals();
    if (g_failed) {
        std::printf("%d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("imagelight_build_check: %d case files, all checks passed\n", argc - 1);
    return 0;
}
