// rgbgrid_build_check.cpp -- the host side of the RGB grid medium (csrc/vspg_scene_build.hip: validate_rgb_grid through validate,
// build_majorant_grid_rgb, build_rgb_octets, build_dscene) run on the CPU.
//
// tests/test_rgbgrid_model.py compiles the two host-only units and this program with the library's flags plus AddressSanitizer and
// UndefinedBehaviorSanitizer, links them WITHOUT the HIP runtime and runs the result: exit status 0 and no sanitizer report.  The
// known answers are derived by hand beside each check.
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

static VspgRenderConfig config(int xres, int yres) {
    VspgRenderConfig cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.xres = xres; cfg.yres = yres; cfg.spp = 1; cfg.shard_count = 1;
    return cfg;
}
static void rgb_medium(VspgScene *sc, int nx, int ny, int nz, const float *a, const float *s, const float *le, float scale, float lescale) {
    VspgMedium &m = sc->medium;
    std::memset(&m, 0, sizeof m);
    m.type = VSPG_MEDIUM_RGBGRID;
    m.nx = nx; m.ny = ny; m.nz = nz;
    for (int k = 0; k < 3; ++k) { m.bounds_min[k] = -0.5f; m.bounds_max[k] = 0.5f; }
    sc->rgb_sigma_a = a; sc->rgb_sigma_s = s; sc->rgb_Le = le;
    sc->rgb_sigma_scale = scale; sc->rgb_le_scale = lescale;
}

// Two voxels along x (nx = 2, ny = nz = 1).  sigma_a = {(1, 5, 2), (3, 0, 4)}, sigma_s = {(7, 1, 1), (2, 2, 6)}, scale 2.
// Per axis MaxValue's range of cell c is floor(c / 16 * n - .5) .. floor((c + 1) / 16 * n - .5) + 1 clipped to [0, n - 1]: along x with
// n = 2: lo = max(floor(c / 8 - .5), 0) is 0 up to cell 11 and 1 from cell 12 on; hi = min(floor((c + 1) / 8 - .5) + 1, 1) is 0 for
// cells 0..2 and 1 from cell 3 on.  Cells 0..2 see voxel 0 alone, cells 3..11 both voxels, cells 12..15 voxel 1 alone.
// max over voxels and channels per grid, then summed: voxel 0 alone 5 + 7 = 12, both 5 + 7 = 12, voxel 1 alone 4 + 6 = 10; times 2.
// (The maximum of the per-voxel sum would give 8, 8 and 10 in the red channel -- another number.)
static void test_two_voxel_majorant() {
    static VspgScene sc;
    std::memset(&sc, 0, sizeof sc);
    const float a[6] = {1, 5, 2, 3, 0, 4}, s[6] = {7, 1, 1, 2, 2, 6};
    rgb_medium(&sc, 2, 1, 1, a, s, nullptr, 2.f, 0.f);
    const std::vector<float> maj = build_majorant_grid_rgb(sc);
    CHECK(maj.size() == 16 * 16 * 16, "%zu", maj.size());
    for (int z = 0; z < 16; ++z)
        for (int y = 0; y < 16; ++y)
            for (int x = 0; x < 16; ++x) {
                const float want = x < 12 ? 24.f : 20.f;
                CHECK(maj[x + 16 * (y + 16 * z)] == want, "cell %d %d %d: %g, expected %g", x, y, z, maj[x + 16 * (y + 16 * z)], want);
            }
    // an absent grid counts as 1: only sigma_s -> (1 + 7) * 2 = 16 up to cell 11, (1 + 6) * 2 = 14 behind it
    rgb_medium(&sc, 2, 1, 1, nullptr, s, nullptr, 2.f, 0.f);
    const std::vector<float> m2 = build_majorant_grid_rgb(sc);
    CHECK(m2[0] == 16.f && m2[11] == 16.f && m2[12] == 14.f && m2[15 + 16 * (15 + 16 * 15)] == 14.f, "%g %g %g", m2[0], m2[11], m2[12]);
}

// The storage image of a 2 x 1 x 1 grid: one brick (bn = (n + 8) / 8 = 1 per axis) of 512 octets of 8 float4.  Base voxel (ix, iy, iz)
// lives at slot (ix + 1) + 8 ((iy + 1) + 8 (iz + 1)); its corner c = dx + 2 dy + 4 dz is voxel (ix + dx, iy + dy, iz + dz) or 0.
static void test_octet_image() {
    static VspgScene sc;
    std::memset(&sc, 0, sizeof sc);
    const float a[6] = {1, 5, 2, 3, 0, 4};
    rgb_medium(&sc, 2, 1, 1, a, nullptr, nullptr, 1.f, 0.f);
    int bnx, bny, bnz;
    rgb_brick_counts(sc.medium, &bnx, &bny, &bnz);
    CHECK(bnx == 1 && bny == 1 && bnz == 1, "%d %d %d", bnx, bny, bnz);
    const std::vector<float> img = build_rgb_octets(a, sc.medium);
    CHECK(img.size() == 512u * 32u, "%zu", img.size());
    auto corner = [&](int ix, int iy, int iz, int c) { return img.data() + rgb_octet_slot(ix + 1, iy + 1, iz + 1, bnx, bny) * 32u + 4 * c; };
    CHECK(rgb_octet_slot(1, 1, 1, 1, 1) == 1 + 8 + 64, "slot");
    // base voxel (0, 0, 0): corner 0 = voxel 0, corner 1 = voxel 1, the rest outside
    CHECK(corner(0, 0, 0, 0)[0] == 1 && corner(0, 0, 0, 0)[1] == 5 && corner(0, 0, 0, 0)[2] == 2 && corner(0, 0, 0, 0)[3] == 0, "corner 0");
    CHECK(corner(0, 0, 0, 1)[0] == 3 && corner(0, 0, 0, 1)[1] == 0 && corner(0, 0, 0, 1)[2] == 4, "corner 1");
    for (int c = 2; c < 8; ++c) CHECK(corner(0, 0, 0, c)[0] == 0 && corner(0, 0, 0, c)[1] == 0 && corner(0, 0, 0, c)[2] == 0, "corner %d", c);
    // base voxel (-1, -1, -1): only corner 7 = voxel (0, 0, 0); base voxel (1, 0, -1): only corner 4 = voxel (1, 0, 0)
    CHECK(corner(-1, -1, -1, 7)[1] == 5 && corner(-1, -1, -1, 0)[1] == 0, "rim");
    CHECK(corner(1, 0, -1, 4)[2] == 4 && corner(1, 0, -1, 5)[2] == 0, "rim 2");
    double sum = 0;   // every voxel appears in exactly eight octets
    for (float v : img) sum += v;
    CHECK(sum == 8 * (1 + 5 + 2 + 3 + 0 + 4), "%g", sum);
}

static void refused(const VspgScene &sc, const char *needle) {
    VspgIntegratorParams prm;
    vspg_integrator_params_default(&prm);
    const VspgRenderConfig cfg = config(16, 16);
    const int rc = validate(&sc, &prm, &cfg);
    CHECK(rc == VSPG_EINVAL, "returned %d for: %s", rc, needle);
    CHECK(std::string(vspg_last_error()).find(needle) != std::string::npos, "message \"%s\" does not name \"%s\"", vspg_last_error(), needle);
}
static void test_validate_and_dscene() {
    static VspgScene base, sc;
    static DScene D;
    CHECK(vspg_scene_fog_box(&base, 16, 16) == 0, "%s", vspg_last_error());
    static float a[2 * 3 * 5 * 3], s[2 * 3 * 5 * 3], le[2 * 3 * 5 * 3], bad[2 * 3 * 5 * 3];
    for (int i = 0; i < 90; ++i) { a[i] = 0.25f * (float)(i % 7); s[i] = 0.5f * (float)(i % 5); le[i] = (float)(i % 3); }
    rgb_medium(&base, 2, 3, 5, a, s, le, 1.5f, 2.f);
    VspgIntegratorParams prm;
    vspg_integrator_params_default(&prm);
    const VspgRenderConfig cfg = config(16, 16);
    CHECK(validate(&base, &prm, &cfg) == 0, "%s", vspg_last_error());
    build_dscene(base, prm, cfg, &D);
    CHECK(D.medium_type == VSPG_MEDIUM_RGBGRID && D.nx == 2 && D.ny == 3 && D.nz == 5 && D.rgb_sigma_scale == 1.5f && D.rgb_le_scale == 2.f, "dscene");
    CHECK(D.rgb_oct_a == nullptr && D.rgb_oct_s == nullptr && D.rgb_Le == nullptr, "device pointers are create's to fill");
    sc = base; sc.rgb_sigma_a = nullptr; sc.rgb_sigma_s = nullptr; sc.rgb_Le = nullptr;   refused(sc, "requires \"sigma_a\" and/or \"sigma_s\"");
    sc = base; sc.rgb_sigma_a = nullptr;                                                refused(sc, "requires \"sigma_a\" if \"Le\"");
    sc = base; sc.rgb_sigma_a = nullptr; sc.rgb_Le = nullptr;                           // only sigma_s: legal
    CHECK(validate(&sc, &prm, &cfg) == 0, "%s", vspg_last_error());
    sc = base; sc.rgb_sigma_s = nullptr;                                                // only sigma_a (with Le): legal
    CHECK(validate(&sc, &prm, &cfg) == 0, "%s", vspg_last_error());
    const float spoil[3] = {-1.f, std::nanf(""), INFINITY};
    for (int g = 0; g < 3; ++g)
        for (int k = 0; k < 3; ++k) {
            std::memcpy(bad, a, sizeof bad);
            bad[89 - 7 * k] = spoil[k];
            sc = base;
            (g == 0 ? sc.rgb_sigma_a : g == 1 ? sc.rgb_sigma_s : sc.rgb_Le) = bad;
            refused(sc, "negative or not finite");
        }
    sc = base; sc.medium.nx = 0;                       refused(sc, "nx, ny, nz > 0");
    sc = base; sc.medium.nz = -3;                      refused(sc, "nx, ny, nz > 0");
    sc = base; sc.rgb_sigma_scale = std::nanf("");     refused(sc, "is not finite");
    sc = base; sc.rgb_le_scale = INFINITY;             refused(sc, "is not finite");
    sc = base; sc.medium.temperature = a;              refused(sc, "no temperature grid");
    sc = base; sc.medium.sigma_a[0] = -5.f; sc.medium.density = nullptr;   // ignored fields
    CHECK(validate(&sc, &prm, &cfg) == 0, "%s", vspg_last_error());
    // a zeroed tail holds no RGB grid: the fog box is what it was
    std::memset(&sc, 0, sizeof sc);
    CHECK(vspg_scene_fog_box(&sc, 16, 16) == 0 && sc.rgb_sigma_a == nullptr && sc.medium.type == VSPG_MEDIUM_HOMOGENEOUS && validate(&sc, &prm, &cfg) == 0, "fog box");
}

int main() {
    test_two_voxel_majorant();
    test_octet_image();
    test_validate_and_dscene();
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("rgbgrid_build_check: all checks passed\n");
    return 0;
}
