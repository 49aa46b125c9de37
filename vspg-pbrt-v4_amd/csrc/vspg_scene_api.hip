// vspg_scene_api.hip -- the entry points of include/vspg.h that touch neither a renderer nor the GPU: version and last error,
// default parameters, camera and transform helpers, point and spot light transforms, the fog-box scene.  Host code only.
#include <cmath>
#include <cstring>
#include <string>

#include "vspg_error.h"
#include "vspg_scene_build.h"

using namespace vspg_host;

static thread_local std::string g_err;
int vspg_host::fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

// The refusals of vspg_renderer_set_camera, in the header's order (no renderer, no HIP call: tests/camera_build_check.cpp links it)
int vspg_host::camera_refusal(const VspgCamera *cam, const VspgCameraModel *model) {
    if (!cam) return fail(VSPG_EINVAL, "null camera");
    const int m = model ? model->model : VSPG_CAMERA_PERSPECTIVE;
    if (m < VSPG_CAMERA_PERSPECTIVE || m > VSPG_CAMERA_SPHERICAL_EQUIRECT) return fail(VSPG_EINVAL, "unknown camera model " + std::to_string(m));
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(cam->origin[k]) || !std::isfinite(cam->right[k]) || !std::isfinite(cam->up[k]) || !std::isfinite(cam->fwd[k]))
            return fail(VSPG_EINVAL, "camera origin or frame is not finite");
    if (!std::isfinite(cam->sx) || !std::isfinite(cam->ox) || !std::isfinite(cam->sy) || !std::isfinite(cam->oy))
        return fail(VSPG_EINVAL, "camera affine term is not finite");
    if (model && m <= VSPG_CAMERA_ORTHOGRAPHIC) {  // (a spherical camera ignores both lens fields)
        if (!(model->lens_radius >= 0) || !std::isfinite(model->lens_radius)) return fail(VSPG_EINVAL, "lens_radius is negative or not finite");
        if (model->lens_radius > 0 && (!(model->focal_distance > 0) || !std::isfinite(model->focal_distance)))
            return fail(VSPG_EINVAL, "focal_distance must be finite and positive under a lens");
    }
    return 0;
}
// What the scene record holds for an accepted model: a spherical camera carries no lens, a lens of radius 0 no focal distance worth reading
VspgCameraModel vspg_host::camera_model_record(const VspgCameraModel *model) {
    VspgCameraModel o = {VSPG_CAMERA_PERSPECTIVE, 0.f, 0.f};
    if (!model) return o;
    o.model = model->model;
    if (o.model <= VSPG_CAMERA_ORTHOGRAPHIC && model->lens_radius > 0) { o.lens_radius = model->lens_radius; o.focal_distance = model->focal_distance; }
    return o;
}
bool vspg_host::camera_model_general(const VspgCameraModel &rec) { return rec.model != VSPG_CAMERA_PERSPECTIVE || rec.lens_radius > 0; }

extern "C" {

int vspg_abi_version(void) { return VSPG_ABI_VERSION; }
const char *vspg_last_error(void) { return g_err.c_str(); }

void vspg_integrator_params_default(VspgIntegratorParams *p) {
    // GuidedVolPathVSPGIntegrator::Create defaults (guidedvolpathvspgintegrator.cpp:1263-1319)
    memset(p, 0, sizeof *p);
    p->maxdepth = 5;
    p->minrrdepth = 1;
    p->usenee = 1;
    p->surfaceguiding = 1;
    p->volumeguiding = 1;
    p->surfaceguidingtype = VSPG_GUIDE_RIS;
    p->volumeguidingtype = VSPG_GUIDE_MIS;
    p->vspguiding = 1;
    p->vspprimaryguiding = 1;
    p->vspsecondaryguiding = 1;
    p->vspmisratio = 0.5f;
    p->vspcriterion = VSPG_VSP_VARIANCE;
    p->vspsamplingmethod = VSPG_VSP_RESAMPLING;
    p->lightsampler = VSPG_LIGHTSAMPLER_BVH;
    p->guide_num_training_waves = 128;
    p->surfacerrguiding = 1;
    p->volumerrguiding = 1;
}

// LookAt's frame (pbrt LookAt: right = Normalize(Cross(Normalize(up), dir)); newUp = Cross(dir, right)), in double, rounded once
static int look_at_frame(VspgCamera *cam, const float eye[3], const float look[3], const float up[3]) {
    double e[3], f[3], u[3];
    for (int i = 0; i < 3; ++i) { e[i] = eye[i]; f[i] = (double)look[i] - eye[i]; u[i] = up[i]; }
    double fl = std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    double ul = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    if (fl == 0 || ul == 0) return fail(VSPG_EINVAL, "degenerate LookAt");
    for (int i = 0; i < 3; ++i) { f[i] /= fl; u[i] /= ul; }
    double r[3] = {u[1] * f[2] - u[2] * f[1], u[2] * f[0] - u[0] * f[2], u[0] * f[1] - u[1] * f[0]};
    double rl = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    if (rl == 0) return fail(VSPG_EINVAL, "up vector parallel to view direction");
    for (int i = 0; i < 3; ++i) r[i] /= rl;
    double nu[3] = {f[1] * r[2] - f[2] * r[1], f[2] * r[0] - f[0] * r[2], f[0] * r[1] - f[1] * r[0]};
    for (int i = 0; i < 3; ++i) {
        cam->origin[i] = (float)e[i];
        cam->right[i] = (float)r[i];
        cam->up[i] = (float)nu[i];
        cam->fwd[i] = (float)f[i];
    }
    return 0;
}

int vspg_camera_look_at_window(VspgCamera *cam, int model, const float eye[3], const float look[3], const float up[3], float fov_degrees,
                               const float screen_window[4], float frame_aspect, int xres, int yres) {
    if (!cam || !eye || !look || !up || xres <= 0 || yres <= 0) return fail(VSPG_EINVAL, "bad camera arguments");
    if (model < VSPG_CAMERA_PERSPECTIVE || model > VSPG_CAMERA_SPHERICAL_EQUIRECT) return fail(VSPG_EINVAL, "unknown camera model");
    if (!(frame_aspect >= 0) || !std::isfinite(frame_aspect)) return fail(VSPG_EINVAL, "frame_aspect is negative or not finite");
    if (screen_window)
        for (int k = 0; k < 4; ++k)
            if (!std::isfinite(screen_window[k])) return fail(VSPG_EINVAL, "screen_window is not finite");
    VspgCamera c;
    memset(&c, 0, sizeof c);
    if (const int rc = look_at_frame(&c, eye, look, up)) return rc;
    if (model == VSPG_CAMERA_PERSPECTIVE || model == VSPG_CAMERA_ORTHOGRAPHIC) {
        // the screen window spans [-1,1] on the shorter axis (cameras.cpp:375-389, :474-489), "screenwindow" replaces it
        // (:390-404); raster y points down
        const double aspect = frame_aspect != 0 ? (double)frame_aspect : (double)xres / (double)yres;
        const double wx = aspect > 1 ? aspect : 1.0, wy = aspect > 1 ? 1.0 : 1.0 / aspect;
        double x0 = -wx, x1 = wx, y0 = -wy, y1 = wy;
        if (screen_window) { x0 = screen_window[0]; x1 = screen_window[1]; y0 = screen_window[2]; y1 = screen_window[3]; }
        // perspective: the window lies on the plane z = 1 of a 90-degree frustum scaled by tan(fov / 2) (Perspective's Scale(1 / tan),
        // transform.cpp); orthographic: camera-space units, fov is not read
        const double th = model == VSPG_CAMERA_PERSPECTIVE ? std::tan(fov_degrees * 3.14159265358979323846 / 360.0) : 1.0;
        c.sx = (float)((x1 - x0) * th / xres);
        c.ox = (float)(x0 * th);
        c.sy = (float)(-((y1 - y0) * th / yres));
        c.oy = (float)(y1 * th);
    }
    *cam = c;
    return 0;
}

int vspg_camera_look_at(VspgCamera *cam, const float eye[3], const float look[3], const float up[3], float fov_degrees,
                        int xres, int yres) {
    return vspg_camera_look_at_window(cam, VSPG_CAMERA_PERSPECTIVE, eye, look, up, fov_degrees, nullptr, 0.f, xres, yres);
}

int vspg_transform_inverse(const float m[16], float inv[16]) {
    if (!m || !inv) return fail(VSPG_EINVAL, "null argument");
    if (m[12] != 0 || m[13] != 0 || m[14] != 0 || m[15] != 1) return fail(VSPG_EINVAL, "affine matrices only (last row 0 0 0 1)");
    const double a = m[0], b = m[1], c = m[2], d = m[4], e = m[5], f = m[6], g = m[8], h = m[9], i = m[10];
    const double A = e * i - f * h, B = -(d * i - f * g), Cc = d * h - e * g;
    const double det = a * A + b * B + c * Cc;
    if (det == 0 || det != det) return fail(VSPG_EINVAL, "singular matrix");
    double r[9] = {A / det, -(b * i - c * h) / det, (b * f - c * e) / det, B / det, (a * i - c * g) / det, -(a * f - c * d) / det,
                   Cc / det, -(a * h - b * g) / det, (a * e - b * d) / det};
    const double t[3] = {m[3], m[7], m[11]};
    for (int row = 0; row < 3; ++row) {
        for (int col = 0; col < 3; ++col) inv[4 * row + col] = (float)r[3 * row + col];
        inv[4 * row + 3] = (float)-(r[3 * row] * t[0] + r[3 * row + 1] * t[1] + r[3 * row + 2] * t[2]);
    }
    inv[12] = inv[13] = inv[14] = 0.f;
    inv[15] = 1.f;
    return 0;
}

// ---- transforms of point and spot lights (PointLight::Create lights.cpp:240-242, SpotLight::Create :1531-1536) ------------------
// SquareMatrix<4> product (util/math.h: FMA accumulation from 0), row-major
static void mat4_mul(const float a[16], const float b[16], float out[16]) {
    float r[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            float s = 0.f;
            for (int k = 0; k < 4; ++k) s = std::fmaf(a[4 * i + k], b[4 * k + j], s);
            r[4 * i + j] = s;
        }
    memcpy(out, r, sizeof r);
}
static void mat4_identity(float m[16]) { for (int i = 0; i < 16; ++i) m[i] = i % 5 == 0 ? 1.f : 0.f; }
// m = ctm * t, inv = t_inv * ctm^-1 (Transform::operator*, transform.cpp:305-307); ctm NULL = identity (t as it stands)
static int light_compose(VspgPointLight *l, const float *ctm, const float t[16], const float t_inv[16]) {
    if (!ctm) {
        memcpy(l->render_from_light, t, 64);
        memcpy(l->light_from_render, t_inv, 64);
        return 0;
    }
    for (int k = 0; k < 16; ++k)
        if (!std::isfinite(ctm[k])) return fail(VSPG_EINVAL, "ctm is not finite");
    float ci[16];
    if (const int rc = vspg_transform_inverse(ctm, ci)) return rc;
    mat4_mul(ctm, t, l->render_from_light);
    mat4_mul(t_inv, ci, l->light_from_render);
    return 0;
}
int vspg_point_light_at(VspgPointLight *l, const float from[3], const float ctm[16]) {
    if (!l || !from) return fail(VSPG_EINVAL, "null argument");
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(from[k])) return fail(VSPG_EINVAL, "from is not finite");
    float t[16], ti[16];
    mat4_identity(t);
    mat4_identity(ti);
    for (int k = 0; k < 3; ++k) { t[4 * k + 3] = from[k]; ti[4 * k + 3] = -from[k]; }  // Translate (transform.cpp:38-43)
    return light_compose(l, ctm, t, ti);
}
// ProjectionLight::Create (lights.cpp:555-556): ctm * Scale(1, -1, 1); Scale's minv holds 1 / y = -1 (transform.cpp:35-45)
int vspg_projection_light_at(VspgPointLight *l, const float ctm[16]) {
    if (!l) return fail(VSPG_EINVAL, "null argument");
    float t[16];
    mat4_identity(t);
    t[5] = -1.f;
    return light_compose(l, ctm, t, t);
}
// GoniometricLight::Create (lights.cpp:724-726): ctm * Transform(swapYZ); the swap is its own inverse
int vspg_goniometric_light_at(VspgPointLight *l, const float ctm[16]) {
    if (!l) return fail(VSPG_EINVAL, "null argument");
    const float t[16] = {1, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 1};
    return light_compose(l, ctm, t, t);
}
int vspg_spot_light_look_at(VspgPointLight *l, const float from[3], const float to[3], const float ctm[16]) {
    if (!l || !from || !to) return fail(VSPG_EINVAL, "null argument");
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(from[k]) || !std::isfinite(to[k])) return fail(VSPG_EINVAL, "from / to is not finite");
    using namespace hostmath;
    const H3 dv = H3{to[0] - from[0], to[1] - from[1], to[2] - from[2]};
    if (!(len2v(dv) > 0)) return fail(VSPG_EINVAL, "spot light: from == to");
    const H3 z = normv(dv);
    // Frame::FromZ: CoordinateSystem (util/vecmath.h:1007-1013)
    const float sign = std::copysign(1.f, z.z);
    const float a = -1 / (sign + z.z);
    const float b = z.x * z.y * a;
    const H3 x = H3{1 + sign * (z.x * z.x) * a, sign * b, -sign * z.x};
    const H3 y = H3{b, sign + (z.y * z.y) * a, -z.y};
    // dirToZ = Transform(Frame): rows x, y, z; its inverse through the library's own helper
    float f[16], fi[16];
    mat4_identity(f);
    f[0] = x.x; f[1] = x.y; f[2] = x.z;
    f[4] = y.x; f[5] = y.y; f[6] = y.z;
    f[8] = z.x; f[9] = z.y; f[10] = z.z;
    if (const int rc = vspg_transform_inverse(f, fi)) return rc;
    // t = Translate(from) * Inverse(dirToZ): m = T * fi, mInv = f * T^-1
    float T[16], Ti[16], t[16], t_inv[16];
    mat4_identity(T);
    mat4_identity(Ti);
    for (int k = 0; k < 3; ++k) { T[4 * k + 3] = from[k]; Ti[4 * k + 3] = -from[k]; }
    mat4_mul(T, fi, t);
    mat4_mul(f, Ti, t_inv);
    return light_compose(l, ctm, t, t_inv);
}

static void quad(VspgQuad *q, float px, float py, float pz, float ax, float ay, float az, float bx, float by, float bz,
                 float kd, float lr, float lg, float lb) {
    memset(q, 0, sizeof *q);
    q->p00[0] = px; q->p00[1] = py; q->p00[2] = pz;
    q->e1[0] = ax; q->e1[1] = ay; q->e1[2] = az;
    q->e2[0] = bx; q->e2[1] = by; q->e2[2] = bz;
    q->Kd[0] = q->Kd[1] = q->Kd[2] = kd;
    q->Le[0] = lr; q->Le[1] = lg; q->Le[2] = lb;
}

int vspg_scene_fog_box(VspgScene *s, int xres, int yres) {
    if (!s) return fail(VSPG_EINVAL, "null scene");
    memset(s, 0, sizeof *s);
    const float k = 0.73f;
    s->n_quads = 7;  // normals e1 x e2 face into the box
    quad(&s->quads[0], -1, -1, -1, 0, 0, 2, 2, 0, 0, k, 0, 0, 0);   // floor
    quad(&s->quads[1], -1, 1, -1, 2, 0, 0, 0, 0, 2, k, 0, 0, 0);    // ceiling
    quad(&s->quads[2], -1, -1, 1, 0, 2, 0, 2, 0, 0, k, 0, 0, 0);    // back  z=+1
    quad(&s->quads[3], -1, -1, -1, 2, 0, 0, 0, 2, 0, k, 0, 0, 0);   // front z=-1
    quad(&s->quads[4], -1, -1, -1, 0, 2, 0, 0, 0, 2, k, 0, 0, 0);   // left
    quad(&s->quads[5], 1, -1, -1, 0, 0, 2, 0, 2, 0, k, 0, 0, 0);    // right
    quad(&s->quads[6], -0.25f, 0.999f, -0.25f, 0.5f, 0, 0, 0, 0, 0.5f, 0, 17, 12, 4);  // ceiling light, faces -y
    const float eye[3] = {0, 0, -0.95f}, look[3] = {0, 0, 0}, up[3] = {0, 1, 0};
    int rc = vspg_camera_look_at(&s->camera, eye, look, up, 60.f, xres, yres);
    if (rc) return rc;
    s->medium.type = VSPG_MEDIUM_HOMOGENEOUS;
    for (int i = 0; i < 3; ++i) { s->medium.sigma_a[i] = 0.05f; s->medium.sigma_s[i] = 0.45f; }
    s->medium.g = 0.f;
    return 0;
}

}  // extern "C"
