// vspg_pointlight.h -- PointLight and SpotLight for the RGB build (src/pbrt/lights.h:203-263, 811-873; lights.cpp:196-248, 1425-1555):
// lights at a position inside the scene.  Two entry points, used by sample_light (vspg_path.h) and pinned through
// vspg_light_sample_batch against tests/pointlight_model.py:
//   point_sample_li  PointLight::SampleLi  (lights.h:243-250)
//   spot_sample_li   SpotLight::SampleLi   (lights.h:852-864), with SpotLight::I (lights.cpp:1447-1450)
// Both are delta lights: pdf 1, PDF_Li 0 (a ray never hits them), and the caller sets delta_light so that the estimate is divided by
// r_l alone (IsDeltaLight, guidedvolpathvspgintegrator.cpp:1248-1249), as for the distant light.
//
// The records (DPointLight, vspg_device.h) are built on the host with the renderer: the position is renderFromLight(Point3f(0, 0, 0))
// evaluated there by Transform::operator()(Point3f)'s arithmetic, its `w == 1` test included (transform.h:310-319) -- for an affine
// matrix the translation column --, I is the reference's scale * I multiplied out, and the two cosines are the constructor's
// (lights.cpp:1438-1439).  They sit behind the light sampler in DScene: only the full-scene kernels read them.
//
// A context point EQUAL to the light's position is not guarded, as in the reference: p - ctx.p is the zero vector, Normalize divides
// 0 by 0 and wi is NaN, Li is I / 0.  No test goes there.
//
// Loads: the light is the lane's pick, so a record's fields are vector loads (11 floats for a point light, 23 for a spot).
#pragma once
#include "vspg_device.h"

// SmoothStep (util/math.h:268-274)
VDEV float smooth_step(float x, float a, float b) {
    if (a == b) return x < a ? 0.f : 1.f;
    const float t = clampf((x - a) / (b - a), 0.f, 1.f);
    return t * t * (3 - 2 * t);
}

VDEV bool point_sample_li(const DPointLight &P, V3 ctxp, LightLi *ls) {
    const V3 p = ld3(P.pos);
    const V3 d = p - ctxp;
    ls->wi = normalize(d);
    ls->L = wdiv(lds(P.I), len2(d));  // scale * I->Sample(lambda) / DistanceSquared(p, ctx.p())
    ls->pdf = 1;
    ls->pLight = p3i_exact(p);        // Interaction(p, &mediumInterface): the exact point, no normal
    ls->nLight = mk(0, 0, 0);
    return true;
}

VDEV bool spot_sample_li(const DPointLight &P, V3 ctxp, LightLi *ls) {
    const V3 p = ld3(P.pos);
    const V3 d = p - ctxp;
    const V3 wi = normalize(d);
    // wLight = Normalize(renderFromLight.ApplyInverse(-wi)) (transform.h:401-406: the linear part of mInv)
    const V3 w = -wi;
    const float *mi = P.mi;
    const V3 wLight = normalize(V3{mi[0] * w.x + mi[1] * w.y + mi[2] * w.z, mi[4] * w.x + mi[5] * w.y + mi[6] * w.z, mi[8] * w.x + mi[9] * w.y + mi[10] * w.z});
    // I(wLight) = SmoothStep(CosTheta(wLight), cosFalloffEnd, cosFalloffStart) * scale * Iemit
    const Spec Iw = lds(P.I) * smooth_step(wLight.z, P.cosFalloffEnd, P.cosFalloffStart);
    const Spec Li = wdiv(Iw, len2(d));
    if (!nonzero(Li)) return false;  // `if (!Li) return {}`
    ls->wi = wi;
    ls->L = Li;
    ls->pdf = 1;
    ls->pLight = p3i_exact(p);
    ls->nLight = mk(0, 0, 0);
    return true;
}
