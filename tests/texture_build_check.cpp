// texture_build_check.cpp -- the host side of image textures (csrc/vspg_scene_build.hip: texture_image_refusal, validate_textures,
// texture_image_build, texture_apply, derive_triangle's texture bits, build_tri_uv, count_textured, build_dscene, validate) run on the CPU.
//
// tests/test_texture_model.py compiles the two host-only units and this program with the library's flags plus AddressSanitizer and
// UndefinedBehaviorSanitizer, links them WITHOUT the HIP runtime and runs the result on case files it wrote from the NumPy model
// (tests/texture_model.py): exit status 0 and no sanitizer report.  A case file holds, little-endian:
//   int32 xres, yres, channels; the pixels (xres * yres * channels floats); the device image the model expects (4 * xres * yres floats)
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

static VspgRenderConfig config() {
    VspgRenderConfig cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.xres = 16; cfg.yres = 16; cfg.spp = 1; cfg.shard_count = 1;
    return cfg;
}

// the fog box with one texture on its back wall (rectangle 2) and on the second of two triangles
static const float kTris[18] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0.5f, -0.9f, 0.5f, 0.5f, -0.9f, 0.75f, 0.75f, -0.9f, 0.5f};
static const int32_t kTriTex[2] = {0, 1};
static const float kTriUv[12] = {0, 0, 1, 0, 1, 1, 0.25f, 0.5f, 2.f, -1.f, 0.75f, 3.f};
static void textured_box(VspgScene *sc, VspgSceneTextures *tx, const float *pixels, int xres, int yres, int channels) {
    CHECK(vspg_scene_fog_box(sc, 16, 16) == 0, "%s", vspg_last_error());
    std::memset(tx, 0, sizeof *tx);
    tx->n_textures = 1;
    VspgTexture &t = tx->textures[0];
    t.pixels = pixels; t.xres = xres; t.yres = yres; t.channels = channels;
    t.wrap = VSPG_TEXWRAP_CLAMP; t.filter = VSPG_TEXFILTER_BILINEAR; t.invert = 1;
    t.scale = 0.5f; t.su = 2.f; t.sv = 3.f; t.du = 0.25f; t.dv = -0.5f;
    tx->quad_texture[2] = 1;
    sc->n_triangles = 2;
    sc->tri_p = kTris;
    tx->tri_texture = kTriTex;
    tx->tri_uv = kTriUv;
}

static void test_case_file(const char *path) {
    std::FILE *f = std::fopen(path, "rb");
    CHECK(f != nullptr, "cannot open %s", path);
    if (!f) return;
    int32_t head[3];
    CHECK(std::fread(head, 4, 3, f) == 3, "%s: short header", path);
    const int xres = head[0], yres = head[1], ch = head[2];
    const size_t n = (size_t)xres * yres;
    std::vector<float> pixels(n * ch), want(4 * n);
    CHECK(std::fread(pixels.data(), 4, pixels.size(), f) == pixels.size(), "%s: short pixels", path);
    CHECK(std::fread(want.data(), 4, want.size(), f) == want.size(), "%s: short image", path);
    std::fclose(f);
    CHECK(texture_image_refusal(pixels.data(), xres, yres, ch) == 0, "%s: %s", path, vspg_last_error());
    const std::vector<float> img = texture_image_build(pixels.data(), xres, yres, ch);
    CHECK(img.size() == want.size() && std::memcmp(img.data(), want.data(), want.size() * 4) == 0, "%s: the device image differs from the model's", path);

    static VspgScene sc;
    static VspgSceneTextures tx;
    textured_box(&sc, &tx, pixels.data(), xres, yres, ch);
    VspgIntegratorParams prm;
    vspg_integrator_params_default(&prm);
    const VspgRenderConfig cfg = config();
    CHECK(validate(&sc, &prm, &cfg) == 0 && validate_textures(sc, tx) == 0, "%s: %s", path, vspg_last_error());
    static DScene D;
    build_dscene(sc, prm, cfg, &D);
    apply_scene_textures(sc, tx, &D);
    const DTexture &T = D.tex[0];
    CHECK(T.texels == nullptr && T.xres == xres && T.yres == yres && T.wrap == VSPG_TEXWRAP_CLAMP && T.filter == VSPG_TEXFILTER_BILINEAR && T.invert == 1,
          "%s: the texture record", path);
    CHECK(T.scale == 0.5f && T.su == 2.f && T.sv == 3.f && T.du == 0.25f && T.dv == -0.5f, "%s: the texture's parameters", path);
    for (int i = 0; i < VSPG_MAX_QUADS; ++i) CHECK(D.quad_tex[i] == (i == 2 ? 1 : 0), "%s: quad_tex[%d] = %d", path, i, D.quad_tex[i]);
    for (int i = 0; i < D.n_quads; ++i) CHECK(D.quads[i].flags == 0, "a texture must not look like a medium boundary");
    CHECK(D.has_boundaries == 0, "a textured scene has no boundaries");
    CHECK(sizeof(DTri) == 80, "DTri keeps its 80 bytes");

    std::vector<DTri> tris;
    std::vector<DBvh4Node> nodes;
    CHECK(build_triangle_bvh(sc, &tris, &nodes, tx.tri_texture) == 0 && tris.size() == 2, "%s: the triangles", path);
    CHECK(count_textured(sc, tx, tris) == 2, "one rectangle and one triangle carry the texture");
    const std::vector<float> uv = build_tri_uv(tx.tri_uv, tris);
    CHECK(uv.size() == 12, "six floats per triangle");
    for (size_t i = 0; i < tris.size() && uv.size() == 12; ++i) {
        const int id = tris[i].id;
        CHECK((tris[i].flags >> TRI_TEX_SHIFT) == kTriTex[id] && (tris[i].flags & SURF_FLAG_MASK) == 0, "triangle %d: flags %d", id, tris[i].flags);
        CHECK(std::memcmp(&uv[6 * i], &kTriUv[6 * id], 24) == 0, "triangle %d: its uv travels in leaf order", id);
    }
    const std::vector<float> def = build_tri_uv(nullptr, tris);  // the default uv
    const float want_def[6] = {0, 0, 1, 0, 1, 1};
    CHECK(def.size() == 12 && std::memcmp(&def[0], want_def, 24) == 0 && std::memcmp(&def[6], want_def, 24) == 0, "the default uv (0,0) (1,0) (1,1)");
    tx.tri_texture = nullptr;  // no triangle textured: no side array
    CHECK(build_triangle_bvh(sc, &tris, &nodes, nullptr) == 0 && build_tri_uv(tx.tri_uv, tris).empty() && count_textured(sc, tx, tris) == 1, "no side array without a textured triangle");
}

static void refused(const VspgScene &sc, const VspgSceneTextures &tx, int code, const char *needle) {
    const int rc = validate_textures(sc, tx);
    CHECK(rc == code && std::strstr(vspg_last_error(), needle), "wanted %d \"%s\", got %d \"%s\"", code, needle, rc, vspg_last_error());
}

static void test_refusals() {
    static VspgScene base, sc;
    static VspgSceneTextures tb, tx;
    static float px[4 * 4 * 3];
    for (float &v : px) v = 0.5f;
    textured_box(&base, &tb, px, 4, 4, 3);
    VspgIntegratorParams prm;
    vspg_integrator_params_default(&prm);
    const VspgRenderConfig cfg = config();
    CHECK(validate(&base, &prm, &cfg) == 0 && validate_textures(base, tb) == 0, "%s", vspg_last_error());
    sc = base; tx = tb; tx.n_textures = -1; refused(sc, tx, VSPG_EINVAL, "n_textures");
    sc = base; tx = tb; tx.n_textures = VSPG_MAX_TEXTURES + 1; refused(sc, tx, VSPG_EINVAL, "n_textures");
    sc = base; tx = tb; tx.quad_texture[0] = 2; refused(sc, tx, VSPG_EINVAL, "names no texture");
    sc = base; tx = tb; tx.quad_texture[0] = -3; refused(sc, tx, VSPG_EINVAL, "names no texture");
    sc = base; tx = tb; sc.quads[2].material = VSPG_MATERIAL_INTERFACE; refused(sc, tx, VSPG_EINVAL, "interface");
    static const int32_t bad_tex[2] = {0, 5}, iface_flags[2] = {0, VSPG_TRI_INTERFACE};
    sc = base; tx = tb; tx.tri_texture = bad_tex; refused(sc, tx, VSPG_EINVAL, "triangle's texture index");
    sc = base; tx = tb; sc.tri_flags = iface_flags; refused(sc, tx, VSPG_EINVAL, "interface");
    static float bad_uv[12];
    std::memcpy(bad_uv, kTriUv, sizeof bad_uv);
    bad_uv[7] = std::numeric_limits<float>::quiet_NaN();
    sc = base; tx = tb; tx.tri_uv = bad_uv; refused(sc, tx, VSPG_EINVAL, "uv is not finite");
    sc = base; tx = tb; tx.textures[0].pixels = nullptr; refused(sc, tx, VSPG_EINVAL, "null pixels");
    sc = base; tx = tb; tx.textures[0].xres = 0; refused(sc, tx, VSPG_EINVAL, "resolution outside");
    sc = base; tx = tb; tx.textures[0].yres = VSPG_TEXTURE_MAX_RES + 1; refused(sc, tx, VSPG_EINVAL, "resolution outside");
    sc = base; tx = tb; tx.textures[0].channels = 4; refused(sc, tx, VSPG_EINVAL, "1 or 3 channels");
    sc = base; tx = tb; tx.textures[0].xres = 3; refused(sc, tx, VSPG_ESCOPE, "power of two");
    sc = base; tx = tb; tx.textures[0].yres = 3; refused(sc, tx, VSPG_ESCOPE, "power of two");
    sc = base; tx = tb; tx.textures[0].wrap = 3; refused(sc, tx, VSPG_EINVAL, "wrap");
    sc = base; tx = tb; tx.textures[0].filter = -1; refused(sc, tx, VSPG_EINVAL, "filter");
    sc = base; tx = tb; tx.textures[0].invert = 2; refused(sc, tx, VSPG_EINVAL, "invert");
    sc = base; tx = tb; tx.textures[0].scale = std::numeric_limits<float>::infinity(); refused(sc, tx, VSPG_EINVAL, "not finite");
    sc = base; tx = tb; tx.textures[0].dv = std::numeric_limits<float>::quiet_NaN(); refused(sc, tx, VSPG_EINVAL, "not finite");
    static float bad_px[4 * 4 * 3];
    std::memcpy(bad_px, px, sizeof px);
    bad_px[47] = std::numeric_limits<float>::quiet_NaN();   // the last float of the image
    sc = base; tx = tb; tx.textures[0].pixels = bad_px; refused(sc, tx, VSPG_EINVAL, "not-a-number or infinite");
    bad_px[47] = -std::numeric_limits<float>::infinity();
    refused(sc, tx, VSPG_EINVAL, "not-a-number or infinite");
    // a zeroed tail holds no texture
    static VspgScene plain;
    CHECK(vspg_scene_fog_box(&plain, 16, 16) == 0, "%s", vspg_last_error());
    static VspgSceneTextures none;
    CHECK(validate(&plain, &prm, &cfg) == 0 && validate_textures(plain, none) == 0, "%s", vspg_last_error());
    static DScene D;
    build_dscene(plain, prm, cfg, &D);
    apply_scene_textures(plain, none, &D);
    CHECK(D.n_textured == 0 && D.tri_uv == nullptr, "an untextured scene");
}

int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) test_case_file(argv[i]);
    test_refusals();
    if (g_failed) {
        std::printf("texture_build_check: %d checks FAILED\n", g_failed);
        return 1;
    }
    std::printf("texture_build_check: %d case files, all checks passed\n", argc - 1);
    return 0;
}
