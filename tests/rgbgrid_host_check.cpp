// rgbgrid_host_check.cpp -- the host adapter's CreateMedium("rgbgrid", ...) (RGBGridMedium::Create, media.cpp:411-484: parameter
// names, defaults, error triggers) and the scene-file reader's MakeNamedMedium "string type" "rgbgrid" (CTM -> renderFromMedium), on
// the CPU.  tests/test_rgbgrid_host.py builds it against libvspg_host.so and runs it twice: with "create", and with tests/scenes/rgb_smoke.pbrt.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "vspg_scenefile.h"

using namespace vspg;

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

// the Error's text, or "" when nothing was thrown
static std::string error_of(const std::function<void()> &f) {
    try { f(); } catch (const Error &e) { return e.what(); }
    return "";
}
static void expect_error(const char *params, const char *needle) {
    RgbGridStorage st;
    const std::string msg = error_of([&] { CreateMedium("rgbgrid", ParameterDictionary::Parse(params), nullptr, nullptr, nullptr, &st); });
    CHECK(msg.find(needle) != std::string::npos, "parameters %s: message \"%s\" does not name \"%s\"", params, msg.c_str(), needle);
}

static void test_create_medium() {
    // two voxels along x, every parameter given
    RgbGridStorage st;
    VspgMedium m = CreateMedium("rgbgrid", ParameterDictionary::Parse("\"integer nx\" 2 \"rgb sigma_a\" [1 2 3 4 5 6] \"rgb sigma_s\" [.5 .25 .125 0 0 1] \"rgb Le\" [0 0 0 1 1 2] "
                                                                       "\"point3 p0\" [-1 -2 -3] \"point3 p1\" [1 2 3] \"float g\" .5 \"float scale\" 4 \"float Lescale\" .25"),
                                nullptr, nullptr, nullptr, &st);
    CHECK(m.type == VSPG_MEDIUM_RGBGRID && m.nx == 2 && m.ny == 1 && m.nz == 1 && m.g == .5f, "%d %d %d %d %g", m.type, m.nx, m.ny, m.nz, m.g);
    CHECK(m.bounds_min[1] == -2.f && m.bounds_max[2] == 3.f && m.density == nullptr && m.temperature == nullptr && m.has_transform == 0, "bounds");
    CHECK(st.sigma_a == std::vector<float>({1, 2, 3, 4, 5, 6}) && st.sigma_s == std::vector<float>({.5f, .25f, .125f, 0, 0, 1}) && st.Le == std::vector<float>({0, 0, 0, 1, 1, 2}), "grids");
    CHECK(st.scale == 4.f && st.Lescale == .25f, "scales %g %g", st.scale, st.Lescale);
    VspgScene sc;
    std::memset(&sc, 0, sizeof sc);
    st.Attach(&sc);
    CHECK(sc.rgb_sigma_a == st.sigma_a.data() && sc.rgb_sigma_s == st.sigma_s.data() && sc.rgb_Le == st.Le.data() && sc.rgb_sigma_scale == 4.f && sc.rgb_le_scale == .25f, "Attach");
    // the defaults: nx = ny = nz = 1, p0 = 0, p1 = 1, g = 0, scale = Lescale = 1; a single "rgb" is a one-voxel grid; absent grids stay absent
    RgbGridStorage d;
    m = CreateMedium("rgbgrid", ParameterDictionary().RGB("sigma_s", 1, 2, 3), nullptr, nullptr, nullptr, &d);
    CHECK(m.nx == 1 && m.ny == 1 && m.nz == 1 && m.g == 0.f && m.bounds_min[0] == 0.f && m.bounds_max[0] == 1.f && m.bounds_max[2] == 1.f, "defaults");
    CHECK(d.sigma_a.empty() && d.Le.empty() && d.sigma_s.size() == 3 && d.scale == 1.f && d.Lescale == 1.f, "default storage");
    d.Attach(&sc);
    CHECK(sc.rgb_sigma_a == nullptr && sc.rgb_Le == nullptr && sc.rgb_sigma_s == d.sigma_s.data(), "Attach with absent grids");
    // the error triggers of media.cpp:418-445, with the reference's words
    expect_error("\"integer nx\" 1", "RGB grid requires \"sigma_a\" and/or \"sigma_s\" parameter values.");
    expect_error("\"integer nx\" 2 \"rgb sigma_a\" [1 1 1 2 2 2] \"rgb sigma_s\" [1 1 1]", "Different number of samples (2 vs 1) provided for \"sigma_a\" and \"sigma_s\".");
    expect_error("\"rgb sigma_s\" [1 1 1] \"rgb Le\" [1 1 1]", "RGB grid requires \"sigma_a\" if \"Le\" value provided.");
    expect_error("\"integer nx\" 2 \"rgb sigma_a\" [1 1 1 2 2 2] \"rgb Le\" [1 1 1]", "Expected 2 values for \"Le\" parameter but were given 1.");
    expect_error("\"integer nx\" 3 \"rgb sigma_a\" [1 1 1 2 2 2]", "RGB grid medium has 2 density values; expected nx*ny*nz = 3");
    expect_error("\"rgb sigma_a\" [1 1 1] \"float bogus\" 1", "\"bogus\": unused parameter.");
    expect_error("\"rgb sigma_a\" [1 1 1 2]", "come in threes");
    expect_error("\"float sigma_a\" [1 1 1]", "wrong type");
    const std::string none = error_of([] { CreateMedium("rgbgrid", ParameterDictionary().RGB("sigma_a", 1, 1, 1)); });
    CHECK(none.find("needs an RgbGridStorage") != std::string::npos, "%s", none.c_str());
}

static void test_scene_file(const char *path) {
    std::unique_ptr<SceneDescription> sd = ParseSceneFile(path);
    const VspgScene &s = sd->scene;
    const VspgMedium &m = s.medium;
    CHECK(m.type == VSPG_MEDIUM_RGBGRID && m.nx == 2 && m.ny == 2 && m.nz == 3 && m.g == .25f, "%d %d %d %d %g", m.type, m.nx, m.ny, m.nz, m.g);
    for (int k = 0; k < 3; ++k) CHECK(m.bounds_min[k] == -.5f && m.bounds_max[k] == .5f, "bounds axis %d", k);
    CHECK(s.rgb_sigma_scale == 2.f && s.rgb_le_scale == .5f, "scales %g %g", s.rgb_sigma_scale, s.rgb_le_scale);
    CHECK(s.rgb_sigma_a == sd->rgb.sigma_a.data() && s.rgb_sigma_s == sd->rgb.sigma_s.data() && s.rgb_Le == sd->rgb.Le.data(), "the record points at the description's grids");
    CHECK(sd->rgb.sigma_a.size() == 36 && sd->rgb.sigma_s.size() == 36 && sd->rgb.Le.size() == 36, "%zu %zu %zu", sd->rgb.sigma_a.size(), sd->rgb.sigma_s.size(), sd->rgb.Le.size());
    // voxel-major, x fastest, R G B per voxel: voxel (x 1, y 0, z 0) is the file's second triple, voxel (0, 1, 2) its eleventh
    CHECK(s.rgb_sigma_a[3] == .25f && s.rgb_sigma_a[4] == .125f && s.rgb_sigma_a[5] == 0.f, "sigma_a voxel 1");
    CHECK(s.rgb_sigma_s[30] == 0.f && s.rgb_sigma_s[31] == 1.f && s.rgb_sigma_s[32] == .5f, "sigma_s voxel 10");
    CHECK(s.rgb_Le[12] == 2.f && s.rgb_Le[13] == 1.f && s.rgb_Le[14] == .5f, "Le voxel 4");
    double sums[3] = {0, 0, 0};
    for (int i = 0; i < 36; ++i) { sums[0] += s.rgb_sigma_a[i]; sums[1] += s.rgb_sigma_s[i]; sums[2] += s.rgb_Le[i]; }
    CHECK(sums[0] == 7.375 && sums[1] == 32.75 && sums[2] == 11., "sums %g %g %g", sums[0], sums[1], sums[2]);
    // renderFromMedium = the CTM at MakeNamedMedium: Translate(.125, -.125, 0) * Scale(1.5, 1.25, 1.5); its inverse is exact here too
    const float want[16] = {1.5f, 0, 0, .125f, 0, 1.25f, 0, -.125f, 0, 0, 1.5f, 0, 0, 0, 0, 1};
    CHECK(m.has_transform == 1, "has_transform %d", m.has_transform);
    for (int k = 0; k < 16; ++k) CHECK(m.render_from_medium[k] == want[k], "render_from_medium[%d] = %g, expected %g", k, m.render_from_medium[k], want[k]);
    CHECK(std::fabs(m.medium_from_render[0] * 1.5f - 1.f) <= 1e-6f && std::fabs(m.medium_from_render[5] - .8f) <= 1e-6f &&
              std::fabs(m.medium_from_render[3] + .125f / 1.5f) <= 1e-6f && std::fabs(m.medium_from_render[7] - .1f) <= 1e-6f && m.medium_from_render[15] == 1.f,
          "medium_from_render");
    CHECK(s.n_quads == 7 && s.camera_outside_medium == 0 && sd->xres == 24 && sd->yres == 16 && sd->pixelSamples == 4, "scene %d %d", s.n_quads, s.camera_outside_medium);
    VspgIntegratorParams prm = ParseIntegratorParams(sd->integratorParams);
    CHECK(prm.vspsamplingmethod == VSPG_VSP_NDS, "vspsamplingmethod %d", prm.vspsamplingmethod);
    // the reader passes the adapter's errors on, and an rgbgrid next to a second medium is refused like any other
    const std::string head = "LookAt 0 0 -1 0 0 0 0 1 0\nMediumInterface \"\" \"m\"\nCamera \"perspective\"\nFilm \"rgb\"\nIntegrator \"guidedvolpathvspg\"\nWorldBegin\n";
    const std::string msg = error_of([&] { (void)ParseSceneString(head + "MakeNamedMedium \"m\" \"string type\" \"rgbgrid\" \"rgb Le\" [1 1 1] \"rgb sigma_s\" [1 1 1]\n"); });
    CHECK(msg.find("requires \"sigma_a\" if \"Le\"") != std::string::npos, "%s", msg.c_str());
}

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: rgbgrid_host_check create | scene.pbrt\n"); return 2; }
    try {
        if (std::string(argv[1]) == "create") test_create_medium();
        else test_scene_file(argv[1]);
    } catch (const std::exception &e) {
        std::printf("FAILED: unexpected exception: %s\n", e.what());
        return 1;
    }
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("rgbgrid_host_check: all checks passed\n");
    return 0;
}
