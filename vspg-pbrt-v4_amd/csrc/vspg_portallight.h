// vspg_portallight.h -- PortalImageInfiniteLight for the RGB build (src/pbrt/lights.h:699-808, lights.cpp:1181-1345): an environment map
// seen through a rectangular opening.  An infinite light of type VSPG_LIGHT_IMAGE_INFINITE whose DScene::portal[k].res > 0 is one
// (vspg_renderer_set_portal_environment_image builds the record; vspg_renderer_set_environment_image clears it).  Four entry points,
// used by sample_light<FULL> and the escaped-ray loop of li_surface_pre (vspg_path.h) and pinned through vspg_portallight_batch
// against tests/portallight_model.py:
//   portal_image_bounds  ImageBounds  (lights.h:785-791)                    -- vspg_portalmap.h
//   portal_Le            Le           (lights.cpp:1287-1294): depends on the ray's ORIGIN
//   portal_pdf_li        PDF_Li       (lights.cpp:1331-1345): depends on the context's point
//   portal_sample_li     SampleLi     (lights.cpp:1305-1329)
// The arithmetic, the bounded bisection and what is defined for NaN inputs: vspg_portalmap.h (host and device).
#pragma once
// (vspg_portalmap.h opens its own namespace block: vspg_path.h includes it in front of its own)

VDEV bool is_portal(const DScene &S, int k) { return S.portal[k].res > 0; }

VDEV Spec portal_Le(const DScene &S, int k, V3 ro, V3 rd, float *uv = nullptr) {
    float rgb[3];
    if (!portal_radiance(S.portal[k], ro, rd, rgb, uv)) return sp(0.f);
    return Spec{rgb[0], rgb[1], rgb[2]} * lds(S.inf_L[k]);
}
VDEV float portal_pdf_li(const DScene &S, int k, V3 ctxp, V3 w) { return portal_pdf(S.portal[k], ctxp, w); }
VDEV bool portal_sample_li(const DScene &S, int k, V3 ctxp, float u0, float u1, LightLi *ls, PortalSample *dbg = nullptr) {
    PortalSample ps = {};
    const bool ok = portal_sample(S.portal[k], ctxp, u0, u1, &ps);
    if (dbg) *dbg = ps;
    if (!ok) return false;
    ls->L = Spec{ps.rgb[0], ps.rgb[1], ps.rgb[2]} * lds(S.inf_L[k]);
    ls->wi = ps.wi;
    ls->pdf = ps.pdf;
    ls->pLight = p3i_exact(ctxp + ps.wi * (2 * S.scene_radius));
    ls->nLight = mk(0, 0, 0);
    return true;
}

// (The entry points are inlined wherever they are used.  The out-of-line form was built and measured and was worse in registers
//  and scratch -- DESIGN.md 4.13 holds the figures.)
