// vspg_spherelight.h -- DiffuseAreaLight on a full Shape "sphere" for the RGB build (src/pbrt/shapes.h:293-393, shapes.cpp:33-58;
// src/pbrt/lights.cpp:796-864, lights.h:492-511).  Three entry points, used by sample_light and li_surface_pre (vspg_path.h) and
// pinned through vspg_light_sample_batch / vspg_light_pdf_batch against tests/spherelight_model.py:
//   sphere_sample_li  DiffuseAreaLight::SampleLi (lights.cpp:796-820) over Sphere::Sample(ctx, u) (shapes.h:293-361), whose inside
//                     branch is Sphere::Sample(u) (shapes.cpp:38-58)
//   sphere_pdf_li     DiffuseAreaLight::PDF_Li (lights.cpp:822-826) = Sphere::PDF(ctx, wi) (shapes.h:364-393)
//   sphere_light_L    DiffuseAreaLight::L (lights.h:492-511) without image and alpha
// No image, no alpha texture, no SampleLe.  The (u, v) of a sample (SafeACos, atan2: shapes.h:347-353, shapes.cpp:50-54) is NOT
// computed: only textures read it and the build has none.
//
// Two records describe the light (vspg_device.h): the sphere's own DSphere (matrices, radius) and the DSphereLight beside it (Le,
// two_sided, the shape's reverseOrientation, 1 / Area(), the centre renderFromObject(Point3f(0, 0, 0)) formed on the host by
// Transform::operator()(Point3f)'s arithmetic, `w == 1` test included).  Area() = phiMax * radius * (zMax - zMin) is OBJECT space:
// under a matrix with scale the cone branch and the area alike ignore the scale, as in the reference ("Scaling detected ...",
// lights.cpp:790-794, is a warning there).
//
// Loads: the light is the lane's pick, so both records are read with vector loads; the branches (inside / cone, Taylor) diverge per
// lane by nature.  sinf / cosf are vspg_libm.h's host-exact ones; their arguments are u * 2 pi, inside the reduction's range.
#pragma once
#include "vspg_device.h"

VDEV Spec sphere_light_L(const DSphereLight &E, V3 n, V3 w) {  // lights.h:495-496: Dot(Normal3f, Vector3f)
    if (!E.two_sided && dot_vn(w, n) < 0) return sp(0.f);
    return lds(E.Le);
}

// ctx.OffsetRayOrigin(pCenter) is inside or on the sphere: Sample and PDF take the area branch (shapes.h:295-297, :365-367)
VDEV bool sphere_ctx_inside(const DSphere &S, const DSphereLight &E, const LsCtx &ctx) {
    const V3 pCenter = ld3(E.center);
    const V3 pOrigin = offset_ray_origin(ctx.pi, ctx.n, pCenter - ctx.pi.mid());  // OffsetRayOrigin(pt) = OffsetRayOrigin(pt - p()) (shapes.h:82-84)
    return len2(pOrigin - pCenter) <= sqr(S.radius);
}

VDEV bool sphere_sample_li(const DSphere &S, const DSphereLight &E, const LsCtx &ctx, float u0, float u1, LightLi *ls) {
    constexpr float g5 = (5 * kMachineEps) / (1 - 5 * kMachineEps);
    const V3 pCenter = ld3(E.center), ctxp = ctx.pi.mid();
    P3i pi;
    V3 n;
    float pdf;
    if (sphere_ctx_inside(S, E, ctx)) {
        // Sphere::Sample(u) (shapes.cpp:38-58); SampleUniformSphere (util/sampling.h:391-396)
        const float z = 1 - 2 * u0;
        const float r = safe_sqrt(1 - sqr(z));
        const float phi = 2 * kPi * u1;
        float sinPhi, cosPhi;
        sincosf_(phi, &sinPhi, &cosPhi);
        V3 pObj = V3{0.f + S.radius * (r * cosPhi), 0.f + S.radius * (r * sinPhi), 0.f + S.radius * z};
        const float sc = S.radius / len(pObj);  // pObj *= radius / Distance(pObj, Point3f(0, 0, 0))
        pObj = V3{pObj.x * sc, pObj.y * sc, pObj.z * sc};
        n = sphere_normal_to_render(S, pObj);   // Normalize((*renderFromObject)(Normal3f(pObj)))
        if (E.reverse) n = -n;
        pi = sphere_point_to_render(S, pObj);   // (*renderFromObject)(Point3fi(pObj, gamma(5) * Abs(pObj)))
        // Sphere::Sample(ctx, u), shapes.h:299-313
        V3 wi = pi.mid() - ctxp;
        if (len2(wi) == 0) return false;
        wi = normalize(wi);
        pdf = E.inv_area / (__builtin_fabsf(dot_vn(-wi, n)) / len2(ctxp - pi.mid()));  // AbsDot(Normal3f, Vector3f)
        if (isinf_(pdf)) return false;
    } else {
        // the cone the sphere subtends (shapes.h:316-360)
        const float sinThetaMax = S.radius / len(ctxp - pCenter);
        const float sin2ThetaMax = sqr(sinThetaMax);
        const float cosThetaMax = safe_sqrt(1 - sin2ThetaMax);
        float oneMinusCosThetaMax = 1 - cosThetaMax;
        float cosTheta = (cosThetaMax - 1) * u0 + 1;
        float sin2Theta = 1 - sqr(cosTheta);
        if (sin2ThetaMax < 0.00068523f) {  // sin^2(1.5 deg): the Taylor series for small angles
            sin2Theta = sin2ThetaMax * u0;
            cosTheta = __builtin_sqrtf(1 - sin2Theta);
            oneMinusCosThetaMax = sin2ThetaMax / 2;
        }
        const float cosAlpha = sin2Theta / sinThetaMax + cosTheta * safe_sqrt(1 - sin2Theta / sqr(sinThetaMax));
        const float sinAlpha = safe_sqrt(1 - sqr(cosAlpha));
        const float phi = u1 * 2 * kPi;
        float sinPhi, cosPhi;
        sincosf_(phi, &sinPhi, &cosPhi);
        // SphericalDirection (vecmath.h:1666-1672), Frame::FromZ (vecmath.h:1867-1871)
        const V3 w = V3{clampf(sinAlpha, -1, 1) * cosPhi, clampf(sinAlpha, -1, 1) * sinPhi, clampf(cosAlpha, -1, 1)};
        Frame f;
        f.z = normalize(pCenter - ctxp);
        coordinate_system(f.z, &f.x, &f.y);
        n = f.from_local(-w);
        const V3 p = V3{pCenter.x + S.radius * n.x, pCenter.y + S.radius * n.y, pCenter.z + S.radius * n.z};
        if (E.reverse) n = -n;
        pi = p3i_from_err(p, V3{g5 * __builtin_fabsf(p.x), g5 * __builtin_fabsf(p.y), g5 * __builtin_fabsf(p.z)});
        pdf = 1 / (2 * kPi * oneMinusCosThetaMax);
    }
    // DiffuseAreaLight::SampleLi (lights.cpp:803-819)
    const V3 d = pi.mid() - ctxp;
    if (pdf == 0 || len2(d) == 0) return false;
    const V3 wi = normalize(d);
    const Spec Le = sphere_light_L(E, n, -wi);
    if (!nonzero(Le)) return false;
    ls->L = Le;
    ls->wi = wi;
    ls->pdf = pdf;
    ls->pLight = pi;
    ls->nLight = n;
    return true;
}

VDEV float sphere_pdf_li(const DSphere &S, const DSphereLight &E, const LsCtx &ctx, V3 wi) {
    const V3 pCenter = ld3(E.center), ctxp = ctx.pi.mid();
    if (sphere_ctx_inside(S, E, ctx)) {
        // ray = ctx.SpawnRay(wi); Intersect(ray) with tMax = Infinity (shapes.h:370-373)
        const V3 o = offset_ray_origin(ctx.pi, ctx.n, wi);
        float t;
        V3 pObj;
        if (!sphere_intersect(S, o, wi, kInf, &t, &pObj)) return 0;
        const SphereSurf ss = sphere_interaction<false>(S, pObj);
        float pdf = E.inv_area / (__builtin_fabsf(dot_vn(-wi, ss.n)) / len2(ctxp - ss.pi.mid()));
        if (isinf_(pdf)) pdf = 0;
        return pdf;
    }
    const float sin2ThetaMax = S.radius * S.radius / len2(ctxp - pCenter);
    const float cosThetaMax = safe_sqrt(1 - sin2ThetaMax);
    float oneMinusCosThetaMax = 1 - cosThetaMax;
    if (sin2ThetaMax < 0.00068523f) oneMinusCosThetaMax = sin2ThetaMax / 2;
    return 1 / (2 * kPi * oneMinusCosThetaMax);
}
