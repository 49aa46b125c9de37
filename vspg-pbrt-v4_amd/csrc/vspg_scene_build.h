// vspg_scene_build.h -- host-side scene preprocessing: what vspg_renderer_create and the update entry points derive from a
// VspgScene before anything is uploaded.  Host code only (vspg_scene_build.hip): no kernel, no HIP call, no renderer.  Built with
// the kernels' flags (-ffp-contract=off -fno-fast-math): the floats computed here are the ones the kernels consume bit for bit.
#pragma once
#include <vector>

#include "vspg_device.h"
#include "vspg_lightsampler.h"
#include "vspg_rgbgrid.h"

#pragma GCC visibility push(hidden)  // shared between the library's units, not part of its ABI
namespace vspg_host {
using namespace vspg;

// ---- host float helpers for scene preprocessing (same formulas as the kernels use) ----
namespace hostmath {
struct H3 { float x, y, z; };
static H3 ld(const float *p) { return H3{p[0], p[1], p[2]}; }
static void stv(float *d, H3 v) { d[0] = v.x; d[1] = v.y; d[2] = v.z; }
static H3 add(H3 a, H3 b) { return H3{a.x + b.x, a.y + b.y, a.z + b.z}; }
static H3 absv(H3 a) { return H3{std::fabs(a.x), std::fabs(a.y), std::fabs(a.z)}; }
static float dop(float a, float b, float c, float d) {
    float cd = c * d;
    float r = std::fmaf(a, b, -cd);
    float e = std::fmaf(-c, d, cd);
    return r + e;
}
static H3 crossv(H3 v, H3 w) { return H3{dop(v.y, w.z, v.z, w.y), dop(v.z, w.x, v.x, w.z), dop(v.x, w.y, v.y, w.x)}; }
static float len2v(H3 a) { return a.x * a.x + a.y * a.y + a.z * a.z; }
static H3 normv(H3 a) { float l = std::sqrt(len2v(a)); return H3{a.x / l, a.y / l, a.z / l}; }
}  // namespace hostmath

// 0, or VSPG_EINVAL with the message set (vspg_error.h)
int validate(const VspgScene *scene, const VspgIntegratorParams *p, const VspgRenderConfig *cfg);
// everything of the device scene that needs no device memory, light sampler included
void build_dscene(const VspgScene &sc, const VspgIntegratorParams &prm, const VspgRenderConfig &cfg, DScene *D);
namespace lsb {
void build(const VspgScene &sc, const VspgIntegratorParams &prm, DScene *D);  // the light sampler alone (a light's power changed)
}
PcgJump pcg_jump(unsigned long long delta);
// ---- camera models (vspg_camera.h; vspg_scene_api.hip): the refusals of vspg_renderer_set_camera in the header's order (0, or
// VSPG_EINVAL with the message set), the record an accepted model leaves in DScene, and ChoiceFacts::camera_general of that record
int camera_refusal(const VspgCamera *cam, const VspgCameraModel *model);
VspgCameraModel camera_model_record(const VspgCameraModel *model);
bool camera_model_general(const VspgCameraModel &rec);
bool wants_guiding(const VspgIntegratorParams &p);
bool wants_training(const VspgIntegratorParams &p);

// false: a degenerate triangle, which no ray hits.  tex: VspgSceneTextures::tri_texture (the triangle's texture goes above the SURF_* bits)
bool derive_triangle(const float *p9, const float *kd, int id, DTri *T, const int32_t *flags = nullptr, const int32_t *tex = nullptr);
// The triangle soup as the kernels read it: the accepted triangles in leaf order and the four-wide BVH over them (both empty when no
// triangle is accepted).  tri_texture: VspgSceneTextures::tri_texture or null.  0, or VSPG_ESCOPE when even median splits leave the tree too deep for the traversal's stack (kBvhStack).
int build_triangle_bvh(const VspgScene &sc, std::vector<DTri> *tris, std::vector<DBvh4Node> *nodes, const int32_t *tri_texture = nullptr);

// ---- image textures on diffuse reflectance: the host side of vspg_texture.h ---------------------------------------------------
// The refusals of one image, shared by create and vspg_renderer_set_texture_image, in the header's order; 0, VSPG_EINVAL or
// VSPG_ESCOPE with the message set
int texture_image_refusal(const float *pixels, int xres, int yres, int channels);
// ... of the record beside the scene (vspg_renderer_create_textured calls it behind validate): the textures, their parameters and
// every surface's index
int validate_textures(const VspgScene &sc, const VspgSceneTextures &tx);
// the device image: one float4 {R, G, B, 0} per texel (a grey image broadcast), row-major, top row first; 4 * xres * yres floats
std::vector<float> texture_image_build(const float *pixels, int xres, int yres, int channels);
// everything of a DTexture but the image pointer
void texture_apply(const VspgTexture &in, DTexture *T);
// the textures' records and the rectangles' indices into a DScene that build_dscene made (the images, the triangles' uv and
// n_textured are vspg_renderer_create_textured's)
void apply_scene_textures(const VspgScene &sc, const VspgSceneTextures &tx, DScene *D);
// the surfaces that carry a texture: rectangles, and triangles the build keeps
int count_textured(const VspgScene &sc, const VspgSceneTextures &tx, const std::vector<DTri> &tris);
// DScene::tri_uv for `tris` (build_triangle_bvh's leaf order): 6 floats per triangle, the caller's or the default (0,0) (1,0) (1,1);
// empty when no triangle of `tris` is textured
std::vector<float> build_tri_uv(const float *tri_uv, const std::vector<DTri> &tris);

int majorant_res(const VspgMedium &m);
std::vector<int2> majorant_axis_ranges(const VspgMedium &m);
std::vector<float> build_majorant_grid(const VspgMedium &m);
std::vector<float> build_majorant_grid_nvdb(const VspgMedium &m);
// RGBGridMedium (VSPG_MEDIUM_RGBGRID, vspg_rgbgrid.h): the refusals of create (validate calls it), the 16^3 majorants, and the device
// image of one RGB grid -- bnx * bny * bnz bricks of 512 octets of 8 float4 (32 floats)
int validate_rgb_grid(const VspgScene &sc);
// ... its per-value loop over one grid's n_floats HOST values (`which`: 0 sigma_a, 1 sigma_s, 2 Le -- the name in the message), which
// vspg_renderer_update_rgb_grids reuses; rgb_grid_value_refusal sets that message alone (a device source is checked by a kernel)
int check_rgb_grid_values(const float *values, size_t n_floats, int which);
int rgb_grid_value_refusal(int which);
std::vector<float> build_majorant_grid_rgb(const VspgScene &sc);
void rgb_brick_counts(const VspgMedium &m, int *bnx, int *bny, int *bnz);
std::vector<float> build_rgb_octets(const float *rgb, const VspgMedium &m);

// ---- image infinite light: the host side of vspg_envlight.h ----------------------------------------------------------------
// The arrays of one DEnvLight, laid out in one buffer: texels | func | cdf | mfunc | mcdf
struct EnvTables {
    int res = 0;
    float integral = 0.f, sum_L[3] = {0.f, 0.f, 0.f};
    std::vector<float> buf;
    size_t o_func = 0, o_cdf = 0, o_mfunc = 0, o_mcdf = 0;
};
void env_build_tables(const float *rgb, int res, EnvTables *T);
bool env_matrices(const float *m34, float *m, float *mi);

// ---- portal image infinite light: the host side of vspg_portallight.h (PortalImageInfiniteLight's constructor, lights.cpp:1181-1260) --
// The slot's one buffer: the DEnvLight arrays of the 1 x 1 white image (what the slot's plain image-light probes keep reading), then
// rectified image | func | summed-area table.  `rec` holds everything of the DPortalLight but the three pointers.
struct PortalTables {
    EnvTables env;  // env.buf is the whole buffer
    size_t o_image = 0, o_func = 0, o_sat = 0;
    DPortalLight rec = {};
};
// The constructor's tests on the quadrilateral (lights.cpp:1218-1228, thresholds compared in double) and a finite, non-degenerate
// outline; 0, or VSPG_EINVAL with the message set.  The reference prints an error and goes on with a broken frame: the library refuses.
int portal_refusal(const float *portal12);
// mi: the linear part of the inverse of render_from_light (env_matrices).  Sequential by construction (the table's running sums).
void portal_build_tables(const float *rgb, int res, const float *mi, const float *portal12, PortalTables *T);

// ---- projection and goniometric lights: the host side of vspg_imagelight.h ------------------------------------------------------
// What one light's image becomes: the device image (projection: a float4 per texel, clamped at zero, pad 0; goniometric: the texels as
// given) and the host-side fields of its DImageLight
struct ImageLightTables {
    int type = 0, xres = 0, yres = 0;
    std::vector<float> buf;
    float sb[4], sfl[12], hither = 0.f, A = 0.f, sum_phi[3], sum_bounds = 0.f, cosTotalWidth = 0.f;
};
int image_light_refusal(int type, const float *pixels, int xres, int yres, int channels);
void image_light_build(int type, const float *pixels, int xres, int yres, float fov_deg, ImageLightTables *T);
void image_light_apply(const ImageLightTables &T, DImageLight *G);

}  // namespace vspg_host
#pragma GCC visibility pop
