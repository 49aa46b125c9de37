// rgbgrid_update_check.cpp -- the host statements the RGB grid update is held to (csrc/vspg_scene_build.hip), run on the CPU:
// build_rgb_octets for the sizes tests/test_rgbgrid_update_model.py names, dumped for the comparison with the NumPy model
// (tests/rgbgrid_update_model.py octets32), and check_rgb_grid_values -- the loop factored out of validate_rgb_grid, which
// vspg_renderer_update_rgb_grids reuses -- on clean, negative, NaN, infinite and -0.0 inputs.
//
// usage: rgbgrid_update_check DIR nx ny nz [nx ny nz ...]   reads DIR/in_<nx>x<ny>x<nz>.bin (3 nx ny nz float32), writes DIR/out_<...>.bin
// The test compiles the two host-only units and this program with the library's flags plus AddressSanitizer and
// UndefinedBehaviorSanitizer, links them WITHOUT the HIP runtime and runs the result: exit status 0 and no sanitizer report.
#include <cmath>
#include <cstdio>
#include <cstdlib>
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

static void test_value_check() {
    const char *names[3] = {"sigma_a", "sigma_s", "Le"};
    std::vector<float> v(3 * 5 * 7 * 3);
    for (size_t i = 0; i < v.size(); ++i) v[i] = 0.125f * (float)(i % 9);
    for (int which = 0; which < 3; ++which) {
        CHECK(check_rgb_grid_values(v.data(), v.size(), which) == 0, "clean values refused: %s", vspg_last_error());
        const float spoil[3] = {-1e-30f, std::nanf(""), INFINITY};
        const size_t at[3] = {0, v.size() / 2 + 1, v.size() - 1};   // first, middle, last
        for (int k = 0; k < 3; ++k)
            for (int p = 0; p < 3; ++p) {
                std::vector<float> bad = v;
                bad[at[p]] = spoil[k];
                CHECK(check_rgb_grid_values(bad.data(), bad.size(), which) == VSPG_EINVAL, "spoil %d at %zu accepted", k, at[p]);
                const std::string msg = vspg_last_error();
                CHECK(msg.find(std::string("\"") + names[which] + "\"") != std::string::npos && msg.find("negative or not finite") != std::string::npos,
                      "message \"%s\"", msg.c_str());
            }
        std::vector<float> neg0 = v;
        neg0[3] = -0.f;
        neg0.back() = -0.f;
        CHECK(check_rgb_grid_values(neg0.data(), neg0.size(), which) == 0, "-0.0 refused: %s", vspg_last_error());
        CHECK(check_rgb_grid_values(v.data(), 0, which) == 0, "an empty range");
    }
    CHECK(rgb_grid_value_refusal(1) == VSPG_EINVAL && std::string(vspg_last_error()).find("\"sigma_s\"") != std::string::npos, "%s", vspg_last_error());
}

static int dump_octets(const std::string &dir, int nx, int ny, int nz) {
    const std::string tag = std::to_string(nx) + "x" + std::to_string(ny) + "x" + std::to_string(nz);
    std::vector<float> rgb((size_t)nx * ny * nz * 3);
    std::FILE *f = std::fopen((dir + "/in_" + tag + ".bin").c_str(), "rb");
    if (!f || std::fread(rgb.data(), sizeof(float), rgb.size(), f) != rgb.size()) {
        std::printf("cannot read the input of %s\n", tag.c_str());
        if (f) std::fclose(f);
        return 1;
    }
    std::fclose(f);
    VspgMedium m;
    std::memset(&m, 0, sizeof m);
    m.type = VSPG_MEDIUM_RGBGRID;
    m.nx = nx; m.ny = ny; m.nz = nz;
    int bnx, bny, bnz;
    rgb_brick_counts(m, &bnx, &bny, &bnz);
    const std::vector<float> img = build_rgb_octets(rgb.data(), m);
    CHECK(img.size() == (size_t)bnx * bny * bnz * 512u * 32u, "%zu", img.size());
    f = std::fopen((dir + "/out_" + tag + ".bin").c_str(), "wb");
    if (!f || std::fwrite(img.data(), sizeof(float), img.size(), f) != img.size()) {
        std::printf("cannot write the image of %s\n", tag.c_str());
        if (f) std::fclose(f);
        return 1;
    }
    std::fclose(f);
    std::printf("%s: %d x %d x %d bricks, %zu floats\n", tag.c_str(), bnx, bny, bnz, img.size());
    return 0;
}

int main(int argc, char **argv) {
    test_value_check();
    if (argc >= 2 && (argc - 2) % 3 != 0) {
        std::printf("usage: rgbgrid_update_check DIR nx ny nz [nx ny nz ...]\n");
        return 2;
    }
    for (int i = 2; i + 2 < argc; i += 3)
        if (dump_octets(argv[1], std::atoi(argv[i]), std::atoi(argv[i + 1]), std::atoi(argv[i + 2]))) return 1;
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("rgbgrid_update_check: all checks passed\n");
    return 0;
}
