// vspg_imagelight.h -- ProjectionLight and GoniometricLight for the RGB build (src/pbrt/lights.h:342-455; lights.cpp:319-441, 564-624):
// lights at a position whose intensity per direction is a texel of an image.  Two entry points, used by sample_light (vspg_path.h)
// and pinned through vspg_light_sample_batch against tests/imagelight_model.py:
//   projection_sample_li   ProjectionLight::SampleLi (lights.cpp:362-373) with ProjectionLight::I (:385-402)
//   goniometric_sample_li  GoniometricLight::SampleLi (lights.cpp:587-596) with GoniometricLight::I (lights.h:440-443)
// (one body, image_light_sample_li, which reads the slot's type: the two differ in the texel gather and the `!Li` test alone)
// Both are delta lights like the point and the spot light (vspg_pointlight.h): pdf 1, PDF_Li 0, the exact point, no normal; the caller
// sets delta_light.  SampleLe / PDF_Le and the PiecewiseConstant2D they alone read are not here: Li never calls them.
//
// The records (DPointLight + DImageLight, vspg_device.h) are built on the host: position, I and mInv as for a point light; the image,
// the screen window, screenFromLight's rows and hither by image_light_build (vspg_scene_build.hip).  wl = ApplyInverse(-wi) is NOT
// normalised, unlike the spot's: the projection divides by its w, and a goniometric light's transform is held orthonormal at create.
//
// Loads: the light is the lane's pick, so the record's fields and the texel are vector loads; a projection texel is one 16-byte load
// (float4, clamped at zero at upload: max(0, x) there and here give the same bits), a goniometric texel one 4-byte load.  The texel
// index is clamped into the image whatever the direction (a NaN direction fails every comparison in front of it).
#pragma once
#include "vspg_device.h"
#include "vspg_envlight.h"  // env_sphere_to_square: EqualAreaSphereToSquare

// renderFromLight.ApplyInverse(-wi) (transform.h:401-406: the linear part of mInv)
VDEV V3 image_light_wl(const DPointLight &P, V3 wi) {
    const V3 w = -wi;
    const float *mi = P.mi;
    return V3{mi[0] * w.x + mi[1] * w.y + mi[2] * w.z, mi[4] * w.x + mi[5] * w.y + mi[6] * w.z, mi[8] * w.x + mi[9] * w.y + mi[10] * w.z};
}
// Image::LookupNearestChannel's index (util/image.h:352-356) under WrapMode::Clamp (:136-138): truncate uv * resolution, then clamp
VDEV int image_light_texel(float uv, int res) {
    const int i = (int)(uv * (float)res);
    return i < 0 ? 0 : (i > res - 1 ? res - 1 : i);
}

// ProjectionLight::I (lights.cpp:385-402) without the light's own I: ClampZero(rgb) of the texel the direction wl looks through, 0 where
// there is none
VDEV Spec projection_texel(const DImageLight &G, V3 wl) {
    if (wl.z < G.hither) return sp(0.f);  // "Discard directions behind projection light"
    // ps = screenFromLight(Point3f(wl)): Transform::operator()(Point3f) (transform.h:310-319), the sums as written and the `wp == 1` test
    const float *s = G.sfl;
    float xp = s[0] * wl.x + s[1] * wl.y + s[2] * wl.z + s[3];
    float yp = s[4] * wl.x + s[5] * wl.y + s[6] * wl.z + s[7];
    const float wp = s[8] * wl.x + s[9] * wl.y + s[10] * wl.z + s[11];
    if (wp != 1) {
        xp = xp / wp;
        yp = yp / wp;
    }
    // Inside(ps, screenBounds): inclusive on both sides (vecmath.h:1454-1456)
    if (!(xp >= G.sb[0] && xp <= G.sb[2] && yp >= G.sb[1] && yp <= G.sb[3])) return sp(0.f);
    // screenBounds.Offset (vecmath.h:1233-1240)
    float ox = xp - G.sb[0], oy = yp - G.sb[1];
    if (G.sb[2] > G.sb[0]) ox = ox / (G.sb[2] - G.sb[0]);
    if (G.sb[3] > G.sb[1]) oy = oy / (G.sb[3] - G.sb[1]);
    const int ix = image_light_texel(ox, G.xres), iy = image_light_texel(oy, G.yres);
    const float4 t = static_cast<const float4 *>(G.texels)[(size_t)iy * (size_t)G.xres + (size_t)ix];
    return Spec{t.x, t.y, t.z};
}
// GoniometricLight::I (lights.h:440-443) without the light's own I: the texel, as it is (no ClampZero in the text)
VDEV Spec goniometric_texel(const DImageLight &G, V3 wl) {
    float u, v;
    env_sphere_to_square(wl, &u, &v);
    const int ix = image_light_texel(u, G.xres), iy = image_light_texel(v, G.yres);
    return sp(static_cast<const float *>(G.texels)[(size_t)iy * (size_t)G.xres + (size_t)ix]);
}
// The two gathers behind one name.  Inlined like the rest of sample_light: behind a call of its own (tried: three floats in and out in
// registers) the full-scene pipeline kernels of scenes WITHOUT such a light ran 0.75 % slower than the parent's, inlined they do not
// (DESIGN.md 4.12).
VDEV Spec image_light_texel_rgb(const DPointLight &P, const DImageLight &G, V3 wi) {
    const V3 wl = image_light_wl(P, wi);
    return P.type == VSPG_LIGHT_PROJECTION ? projection_texel(G, wl) : goniometric_texel(G, wl);
}

// ProjectionLight::SampleLi (`if (!Li) return {}`) and GoniometricLight::SampleLi (a sample is always returned)
VDEV bool image_light_sample_li(const DPointLight &P, const DImageLight &G, V3 ctxp, LightLi *ls) {
    const V3 p = ld3(P.pos);
    const V3 d = p - ctxp;
    const V3 wi = normalize(d);
    // scale * s.Sample(lambda) [* texel] / DistanceSquared(p, ctx.p())
    const Spec Li = wdiv(lds(P.I) * image_light_texel_rgb(P, G, wi), len2(d));
    if (P.type == VSPG_LIGHT_PROJECTION && !nonzero(Li)) return false;
    ls->wi = wi;
    ls->L = Li;
    ls->pdf = 1;
    ls->pLight = p3i_exact(p);  // Interaction(p, &mediumInterface): the exact point, no normal
    ls->nLight = mk(0, 0, 0);
    return true;
}
VDEV bool projection_sample_li(const DPointLight &P, const DImageLight &G, V3 ctxp, LightLi *ls) { return image_light_sample_li(P, G, ctxp, ls); }
VDEV bool goniometric_sample_li(const DPointLight &P, const DImageLight &G, V3 ctxp, LightLi *ls) { return image_light_sample_li(P, G, ctxp, ls); }
