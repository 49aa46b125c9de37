// vspg_camera.h -- the camera ray of the full-scene kernels: GenerateRay of PerspectiveCamera, OrthographicCamera and SphericalCamera
// (src/pbrt/cameras.cpp:410-433, :290-312, :616-636), pinned through vspg_camera_ray_batch against tests/camera_model.py bit for bit.
// One function, camera_generate_ray; start_path_common<true> (vspg_path.h) and the probe kernel k_camera_ray call it, nothing copies it.
// (included inside vspg_path.h's namespace block, behind vspg_envlight.h: env_square_to_sphere is EqualAreaSquareToSphere)
//
// The record: DScene::cam (VspgCamera: the raster-to-camera affine map sx, ox, sy, oy and the render-space frame) and, at the very
// end of DScene, cam_model (VSPG_CAMERA_*), cam_lens_radius and cam_focal_distance.  All wave-uniform: scalar loads, one branch on the
// model and one on the lens, no divergence inside a wavefront.
//
// Statement order, in float with no contraction (-ffp-contract=off; no product-sum below is fused, the reference calls no FMA here):
//   perspective   pCamera = (sx pfx + ox, sy pfy + oy, 1);  o = 0;  d = pCamera / sqrt(x^2 + y^2 + z^2), one division per component
//   orthographic  o = (sx pfx + ox, sy pfy + oy, 0);  d = (0, 0, 1)
//   lens (both, lens_radius > 0)
//                 (x, y) = 2 u - 1;  the concentric map of cos_hemi_pre: r, theta;  disk = (r cos theta, r sin theta), (0, 0) at the centre
//                 pLens = (lens_radius disk.x, lens_radius disk.y)
//                 ft = focal_distance / d.z;  pFocus = o + d ft (per component: product, then sum)
//                 o = (pLens.x, pLens.y, 0)  -- the lens point itself, for the orthographic camera too: the reference's text
//                 d = Normalize(pFocus - o)
//   spherical     uv = (pfx / xres, pfy / yres), two true divisions
//                 equirectangular  theta = Pi uv[1];  phi = (2 Pi) uv[0];  SphericalDirection(sin theta, cos theta, phi) =
//                                  (Clamp(sin theta, -1, 1) cos phi, Clamp(sin theta, -1, 1) sin phi, Clamp(cos theta, -1, 1))
//                 equal-area       uv = WrapEqualAreaSquare(uv);  dir = EqualAreaSquareToSphere(uv)
//                 swap(dir.y, dir.z);  o = 0;  d = dir, not normalised; no lens
//   render space  ro = origin + ((o.x right + o.y up) + o.z fwd), and `origin` itself where o is the camera-space origin (a pinhole
//                 perspective, a spherical camera);  rd = (d.x right + d.y up) + d.z fwd   (Frame::from_local, per component)
#pragma once
#include "vspg_device.h"

// anything but the pinhole perspective (the host holds ChoiceFacts::camera_general to the same rule: vspg_camera_model_general)
VDEV bool camera_is_general(const DScene &S) { return S.cam_model != VSPG_CAMERA_PERSPECTIVE || S.cam_lens_radius > 0; }

// WrapEqualAreaSquare (util/math.cpp:363-379)
VDEV void wrap_equal_area_square(float *pu, float *pv) {
    float u = *pu, v = *pv;
    if (u < 0) {
        u = -u;
        v = 1 - v;
    } else if (u > 1) {
        u = 2 - u;
        v = 1 - v;
    }
    if (v < 0) {
        u = 1 - u;
        v = -v;
    } else if (v > 1) {
        u = 1 - u;
        v = 2 - v;
    }
    *pu = u;
    *pv = v;
}

// the thin lens of PerspectiveCamera / OrthographicCamera::GenerateRay: (o, d) in camera space, replaced
VDEV void camera_thin_lens(float lens_radius, float focal_distance, float uLensX, float uLensY, V3 *o, V3 *d) {
    float r, sinT, cosT;
    bool degenerate;
    const float theta = cos_hemi_pre(uLensX, uLensY, &r, &degenerate);  // SampleUniformDiskConcentric (sampling.h:325-341)
    sincosf_(theta, &sinT, &cosT);
    const float lx = lens_radius * (degenerate ? 0.f : r * cosT), ly = lens_radius * (degenerate ? 0.f : r * sinT);
    const float ft = focal_distance / d->z;
    const V3 pFocus = *o + *d * ft;
    *o = mk(lx, ly, 0.f);
    *d = normalize(pFocus - *o);
}

VDEV void camera_generate_ray(const DScene &S, float pfx, float pfy, float uLensX, float uLensY, V3 *ro, V3 *rd) {
    const int model = S.cam_model;
    V3 o = mk(0.f, 0.f, 0.f), d;
    bool at_origin = true;  // o is the camera-space origin: its render-space image is `origin` itself, nothing is added to it
    if (model == VSPG_CAMERA_SPHERICAL_EQUALAREA || model == VSPG_CAMERA_SPHERICAL_EQUIRECT) {
        float u = pfx / (float)S.xres, v = pfy / (float)S.yres;
        V3 dir;
        if (model == VSPG_CAMERA_SPHERICAL_EQUIRECT) {
            const float theta = kPi * v, phi = (2 * kPi) * u;
            float sinTheta, cosTheta, sinPhi, cosPhi;
            sincosf_(theta, &sinTheta, &cosTheta);
            sincosf_(phi, &sinPhi, &cosPhi);
            dir = mk(clampf(sinTheta, -1, 1) * cosPhi, clampf(sinTheta, -1, 1) * sinPhi, clampf(cosTheta, -1, 1));  // vecmath.h:1666-1672
        } else {
            wrap_equal_area_square(&u, &v);
            dir = env_square_to_sphere(u, v);
        }
        d = mk(dir.x, dir.z, dir.y);
    } else {
        const float cx = S.cam.sx * pfx + S.cam.ox, cy = S.cam.sy * pfy + S.cam.oy;
        if (model == VSPG_CAMERA_ORTHOGRAPHIC) {
            o = mk(cx, cy, 0.f);
            d = mk(0.f, 0.f, 1.f);
            at_origin = false;
        } else {
            d = normalize(mk(cx, cy, 1.f));
        }
        if (S.cam_lens_radius > 0) {
            camera_thin_lens(S.cam_lens_radius, S.cam_focal_distance, uLensX, uLensY, &o, &d);
            at_origin = false;
        }
    }
    const Frame f{ld3(S.cam.right), ld3(S.cam.up), ld3(S.cam.fwd)};
    const V3 origin = ld3(S.cam.origin);
    *ro = at_origin ? origin : origin + f.from_local(o);
    *rd = f.from_local(d);
}
