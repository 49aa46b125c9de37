// Stand-alone driver of tests/test_camera_model.py: the host-only camera code -- vspg_camera_look_at_window and the refusals of
// vspg_renderer_set_camera (vspg_host::camera_refusal, camera_model_record, camera_model_general; csrc/vspg_scene_api.hip) -- linked
// with the two host-only units and without the HIP runtime, built with AddressSanitizer and UndefinedBehaviorSanitizer and run on
// the CPU.  Prints one line per group and "camera_build_check: ok"; exit status 1 and a message at the first failed check.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "vspg_scene_build.h"

using namespace vspg_host;

static int g_failed = 0;
#define CHECK(cond)                                                               \
    do {                                                                          \
        if (!(cond)) {                                                            \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            g_failed = 1;                                                         \
        }                                                                         \
    } while (0)

static VspgCamera good_camera(int model = VSPG_CAMERA_PERSPECTIVE) {
    VspgCamera c;
    const float eye[3] = {0, 0, -0.95f}, look[3] = {0, 0, 0}, up[3] = {0, 1, 0};
    CHECK(vspg_camera_look_at_window(&c, model, eye, look, up, 60.f, nullptr, 0.f, 33, 17) == 0);
    return c;
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float eye[3] = {0.5f, 0.25f, -2.f}, look[3] = {0, 0.5f, 1}, up[3] = {0.1f, 1, 0};
    {   // the default case equals vspg_camera_look_at byte for byte, at both aspects
        for (int k = 0; k < 2; ++k) {
            const int w = k ? 17 : 33, h = k ? 33 : 17;
            VspgCamera a, b;
            std::memset(&a, 0x5a, sizeof a);
            std::memset(&b, 0xa5, sizeof b);
            CHECK(vspg_camera_look_at(&a, eye, look, up, 37.5f, w, h) == 0);
            CHECK(vspg_camera_look_at_window(&b, VSPG_CAMERA_PERSPECTIVE, eye, look, up, 37.5f, nullptr, 0.f, w, h) == 0);
            CHECK(std::memcmp(&a, &b, sizeof a) == 0);
        }
        std::printf("look_at_window == look_at in the default case\n");
    }
    {   // windows: orthographic takes the window as it is, perspective scales it by tan(fov / 2) = 1 at 90 degrees; raster y points down
        const float sw[4] = {-2.f, 6.f, -1.f, 3.f};
        VspgCamera o, p, s;
        CHECK(vspg_camera_look_at_window(&o, VSPG_CAMERA_ORTHOGRAPHIC, eye, look, up, 0.f, sw, 0.f, 32, 16) == 0);
        CHECK(o.sx == 0.25f && o.ox == -2.f && o.sy == -0.25f && o.oy == 3.f);
        CHECK(vspg_camera_look_at_window(&p, VSPG_CAMERA_PERSPECTIVE, eye, look, up, 90.f, sw, 0.f, 32, 16) == 0);
        CHECK(std::fabs(p.sx - 0.25f) < 1e-7f && std::fabs(p.ox + 2.f) < 1e-6f && std::fabs(p.sy + 0.25f) < 1e-7f && std::fabs(p.oy - 3.f) < 1e-6f);
        // frameaspectratio on both sides of 1: [-a, a] x [-1, 1] and [-1, 1] x [-1/a, 1/a]
        CHECK(vspg_camera_look_at_window(&o, VSPG_CAMERA_ORTHOGRAPHIC, eye, look, up, 0.f, nullptr, 2.f, 32, 16) == 0);
        CHECK(o.sx == 0.125f && o.ox == -2.f && o.sy == -0.125f && o.oy == 1.f);
        CHECK(vspg_camera_look_at_window(&o, VSPG_CAMERA_ORTHOGRAPHIC, eye, look, up, 0.f, nullptr, 0.5f, 32, 16) == 0);
        CHECK(o.sx == 0.0625f && o.ox == -1.f && o.sy == -0.25f && o.oy == 2.f);
        CHECK(vspg_camera_look_at_window(&s, VSPG_CAMERA_SPHERICAL_EQUALAREA, eye, look, up, 0.f, sw, 0.f, 32, 16) == 0);
        CHECK(s.sx == 0.f && s.ox == 0.f && s.sy == 0.f && s.oy == 0.f && s.origin[0] == 0.5f && s.origin[2] == -2.f);
        CHECK(std::memcmp(s.fwd, p.fwd, sizeof s.fwd) == 0 && std::memcmp(s.right, o.right, sizeof s.right) == 0);
        std::printf("screen windows and frame aspect ratios\n");
    }
    {   // vspg_camera_look_at_window's refusals leave the record alone
        VspgCamera c;
        std::memset(&c, 0x11, sizeof c);
        VspgCamera before = c;
        const float bad_sw[4] = {-1.f, nan, -1.f, 1.f};
        CHECK(vspg_camera_look_at_window(nullptr, 0, eye, look, up, 60.f, nullptr, 0.f, 8, 8) == VSPG_EINVAL);
        CHECK(vspg_camera_look_at_window(&c, 4, eye, look, up, 60.f, nullptr, 0.f, 8, 8) == VSPG_EINVAL);
        CHECK(vspg_camera_look_at_window(&c, -1, eye, look, up, 60.f, nullptr, 0.f, 8, 8) == VSPG_EINVAL);
        CHECK(vspg_camera_look_at_window(&c, 0, eye, look, up, 60.f, nullptr, -1.f, 8, 8) == VSPG_EINVAL);
        CHECK(vspg_camera_look_at_window(&c, 0, eye, look, up, 60.f, nullptr, inf, 8, 8) == VSPG_EINVAL);
        CHECK(vspg_camera_look_at_window(&c, 1, eye, look, up, 60.f, bad_sw, 0.f, 8, 8) == VSPG_EINVAL);
        CHECK(vspg_camera_look_at_window(&c, 0, eye, eye, up, 60.f, nullptr, 0.f, 8, 8) == VSPG_EINVAL);
        CHECK(vspg_camera_look_at_window(&c, 0, eye, look, up, 60.f, nullptr, 0.f, 0, 8) == VSPG_EINVAL);
        CHECK(std::memcmp(&c, &before, sizeof c) == 0);
        std::printf("look_at_window refusals\n");
    }
    {   // the refusals of vspg_renderer_set_camera, in the header's order, and what passes
        const VspgCamera c = good_camera();
        VspgCameraModel m = {VSPG_CAMERA_PERSPECTIVE, 0.f, 0.f};
        CHECK(camera_refusal(nullptr, &m) == VSPG_EINVAL);
        CHECK(camera_refusal(&c, nullptr) == 0);
        CHECK(camera_refusal(&c, &m) == 0);
        for (int bad : {-1, 4, 1000}) { m.model = bad; CHECK(camera_refusal(&c, &m) == VSPG_EINVAL && std::strstr(vspg_last_error(), "unknown camera model")); }
        m.model = VSPG_CAMERA_PERSPECTIVE;
        for (int k = 0; k < 16; ++k) {  // every float of the record, NaN and infinity
            for (const float v : {nan, inf, -inf}) {
                VspgCamera b = c;
                reinterpret_cast<float *>(&b)[k] = v;
                CHECK(camera_refusal(&b, &m) == VSPG_EINVAL && std::strstr(vspg_last_error(), "not finite"));
                CHECK(camera_refusal(&b, nullptr) == VSPG_EINVAL);
            }
        }
        static_assert(sizeof(VspgCamera) == 16 * sizeof(float), "origin, right, up, fwd and the four affine terms");
        for (const int model : {VSPG_CAMERA_PERSPECTIVE, VSPG_CAMERA_ORTHOGRAPHIC}) {
            for (const float r : {-1.f, -0.f - 1e-30f, nan, inf}) { VspgCameraModel b = {model, r, 1.f}; CHECK(camera_refusal(&c, &b) == VSPG_EINVAL && std::strstr(vspg_last_error(), "lens_radius")); }
            for (const float f : {0.f, -1.f, nan, inf}) { VspgCameraModel b = {model, 0.1f, f}; CHECK(camera_refusal(&c, &b) == VSPG_EINVAL && std::strstr(vspg_last_error(), "focal_distance")); }
            for (const float f : {0.f, -1.f, nan, inf}) { VspgCameraModel b = {model, 0.f, f}; CHECK(camera_refusal(&c, &b) == 0); }  // (no lens: not read)
            VspgCameraModel ok = {model, 0.05f, 1.95f};
            CHECK(camera_refusal(&c, &ok) == 0);
            const VspgCameraModel rec = camera_model_record(&ok);
            CHECK(rec.model == model && rec.lens_radius == 0.05f && rec.focal_distance == 1.95f && camera_model_general(rec));
        }
        for (const int model : {VSPG_CAMERA_SPHERICAL_EQUALAREA, VSPG_CAMERA_SPHERICAL_EQUIRECT}) {  // a spherical model ignores both lens fields
            VspgCameraModel b = {model, nan, -inf};
            CHECK(camera_refusal(&c, &b) == 0);
            const VspgCameraModel rec = camera_model_record(&b);
            CHECK(rec.model == model && rec.lens_radius == 0.f && rec.focal_distance == 0.f && camera_model_general(rec));
        }
        {   // the pinhole: a null model, a zeroed one, perspective with lens_radius 0 and any focal distance
            VspgCameraModel z = {0, 0.f, 0.f}, f = {VSPG_CAMERA_PERSPECTIVE, 0.f, 1e6f};
            for (const VspgCameraModel *p : {(const VspgCameraModel *)nullptr, (const VspgCameraModel *)&z, (const VspgCameraModel *)&f}) {
                const VspgCameraModel rec = camera_model_record(p);
                CHECK(rec.model == 0 && rec.lens_radius == 0.f && rec.focal_distance == 0.f && !camera_model_general(rec));
            }
            VspgCameraModel o = {VSPG_CAMERA_ORTHOGRAPHIC, 0.f, 0.f};
            CHECK(camera_model_general(camera_model_record(&o)));
        }
        std::printf("set_camera refusals and acceptances\n");
    }
    if (g_failed) return 1;
    std::printf("camera_build_check: ok\n");
    return 0;
}
