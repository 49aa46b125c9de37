// vspg_probe_kernels.h -- the kernels behind the parity-probe entry points (k_ray_batch, k_tmaj_batch, k_primitives, k_libm_*,
// k_blackbody, the envlight and light-sample batches) and the density-storage builders (k_brick_flags, k_brick_fill,
// k_majorant_build and what follows it).
//
// Text of vspg_capi.hip, included there once at the place where it stood: it is part of that translation unit, uses the constants
// defined above it (kBlock) and is not meant for any other unit.
#pragma once

namespace {

// vspg_ray_batch (include/vspg.h): Integrator::Intersect, then Interaction::SpawnRay / SpawnRayTo from the hit and Intersect /
// IntersectP of the spawned ray -- the full-scene intersection code of the path kernels (rectangles, BVH triangles, spheres)
__global__ __launch_bounds__(kBlock) void k_ray_batch(const DScene *__restrict__ Sp, int n, const VspgRayQuery *__restrict__ q, VspgRayResult *__restrict__ out) {
    const DScene &S = *Sp;
    stage_scene_lds(S);
    __syncthreads();
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    VspgRayResult o;
    o.hit = 0; o.prim = 0; o.t = 0.f; o.hit2 = 0; o.any2 = 0; o.t2 = 0.f;
    for (int k = 0; k < 3; ++k) o.p[k] = o.n[k] = o.o2[k] = o.d2[k] = 0.f;
    const VspgRayQuery Q = q[i];
    const Isect si = scene_intersect<true>(S, ld3(Q.o), ld3(Q.d), Q.tMax);
    if (si.hit) {
        const P3i pi = surf_pi<true>(S, si.quad, si.p);
        const V3 pm = pi.mid();
        o.hit = 1;
        o.prim = is_sphere(si.quad) ? 2000000 + sphere_of(si.quad) : (is_tri(si.quad) ? 1000000 + S.tris[tri_of(si.quad)].id : si.quad);
        o.t = si.t;
        o.p[0] = pm.x; o.p[1] = pm.y; o.p[2] = pm.z;
        o.n[0] = si.n.x; o.n[1] = si.n.y; o.n[2] = si.n.z;
        if (Q.mode != 0) {
            const V3 w = ld3(Q.w);
            const V3 d2 = Q.mode == 1 ? w : w - pm;
            const V3 o2 = offset_ray_origin(pi, si.n, d2);
            o.o2[0] = o2.x; o.o2[1] = o2.y; o.o2[2] = o2.z;
            o.d2[0] = d2.x; o.d2[1] = d2.y; o.d2[2] = d2.z;
            const Isect s2 = scene_intersect<true>(S, o2, d2, Q.tMax2);
            o.hit2 = s2.hit ? 1 : 0;
            o.t2 = s2.hit ? s2.t : 0.f;
            o.any2 = scene_intersect_any<true>(S, o2, d2, Q.tMax2) ? 1 : 0;
        }
    }
    out[i] = o;
}

template <class Medium>
__global__ __launch_bounds__(kBlock) void k_tmaj_batch(const DScene *__restrict__ Sp, int variant, int n,
                                                       const VspgTmajQuery *__restrict__ q, VspgTmajResult *__restrict__ out) {
    const DScene &S = *Sp;
    int i = blockIdx.x * kBlock + threadIdx.x;
    stage_scene_lds(S);
    __syncthreads();
    if (i >= n) return;
    const Medium medium = MediumMaker<Medium>::make(S, S.majorant);
    VspgTmajQuery Q = q[i];
    VspgTmajResult R;
    memset(&R, 0, sizeof R);
    R.last_t = -1.f;
    R.majorant_scale = 1.f;
    Rng rng;
    rng.set_sequence(hash_float(Q.rng_a), hash_float(Q.rng_b));
    const int ch = Q.channel;
    V3 ro = ld3(Q.o), rd = ld3(Q.d), rdn = normalize(rd);
    bool guide = Q.vsp >= 0.f;
    float vsp = guide ? fmax_(fmin_(Q.vsp, 0.999f), 0.001f) : Q.vsp;
    int ncb = 0;
    float sum = 0, last_t = -1.f;
    V3 lastp = mk(0, 0, 0);
    auto rec = [&](V3 p, const MediumProps &mp, Spec sigma_maj, Spec, bool) {
        ncb++;
        lastp = p;
        last_t = dot(p - ro, rdn);
        Spec sigma_t = mp.sigma_t;
        sum += ch_of(sigma_t, ch) / ch_of(sigma_maj, ch);
        if (Q.stop_after > 0 && ncb >= Q.stop_after) return false;
        return true;
    };
    Spec T = sp(1.f), rf = sp(1.f);
    if (variant == VSPG_TMAJ_PLAIN) {
        T = sample_T_maj(medium, ro, rd, Q.tMax, Q.u, rng, ch, rec);
    } else if (variant == VSPG_TMAJ_OPTICAL_DEPTH) {
        T = sample_T_maj_ods(medium, ro, rd, Q.tMax, Q.u, rng, ch, guide, vsp, S.prm.vspmisratio,
                             S.prm.vspsamplingmethod == VSPG_VSP_NDS, &rf, rec);
    } else {
        float vrc = vsp, ms = 1.f;
        T = sample_T_maj_resampling(medium, ro, rd, Q.tMax, Q.u, rng, ch, guide, vsp, &vrc, &ms, rec);
        R.vrc = vrc;
        R.majorant_scale = ms;
    }
    R.T_maj[0] = T.r; R.T_maj[1] = T.g; R.T_maj[2] = T.b;
    R.r_u_factor[0] = rf.r; R.r_u_factor[1] = rf.g; R.r_u_factor[2] = rf.b;
    R.last_t = last_t;
    R.last_p[0] = lastp.x; R.last_p[1] = lastp.y; R.last_p[2] = lastp.z;
    R.n_callbacks = ncb;
    R.sum_sigt_over_maj = sum;
    out[i] = R;
}

__global__ __launch_bounds__(kBlock) void k_primitives(int n, const float *__restrict__ f, const float *__restrict__ g,
                                                       uint64_t *__restrict__ hash, uint32_t *__restrict__ rng_u32,
                                                       float *__restrict__ fexp) {
    int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    hash[i] = hash_float(f[i]);
    Rng r;
    r.set_sequence(hash_float(f[i]), hash_float(g[i]));
    rng_u32[i] = r.u32();
    fexp[i] = fast_exp(f[i]);
}

__global__ __launch_bounds__(kBlock) void k_guiding_query(const DScene *__restrict__ Sp, int is_volume, float g, int n,
                                                          const float *__restrict__ p, const float *__restrict__ a,
                                                          const float *__restrict__ wi, const float *__restrict__ u,
                                                          int32_t *__restrict__ ok, float *__restrict__ pdf,
                                                          float *__restrict__ inc, float *__restrict__ vsp,
                                                          float *__restrict__ ws, float *__restrict__ pdfs) {
    const DScene &S = *Sp;
    int i = blockIdx.x * kBlock + threadIdx.x;
    vspg_libm::stage_logf_tab_lds();
    __syncthreads();
    if (i >= n) return;
    float *glds = guide_lds();
    V3 pp = ld3(p + 3 * i), aa = ld3(a + 3 * i), w = ld3(wi + 3 * i);
    GDist d = is_volume ? gdist_init_volume(S.field, pp, aa, g, glds, kBlock) : gdist_init_surface(S.field, pp, aa, glds, kBlock);
    ok[i] = d.ok ? 1 : 0;
    pdf[i] = inc[i] = pdfs[i] = 0;
    vsp[i] = -1;
    ws[3 * i] = ws[3 * i + 1] = ws[3 * i + 2] = 0;
    if (!d.ok) return;
    pdf[i] = gdist_pdf(d, w);
    inc[i] = gdist_incoming_pdf(S.field, d, w);
    vsp[i] = gdist_vsp(S.field, d.field, d.region, d, w);
    V3 s;
    pdfs[i] = gdist_sample(d, u[2 * i], u[2 * i + 1], &s);
    ws[3 * i] = s.x; ws[3 * i + 1] = s.y; ws[3 * i + 2] = s.z;
}

__global__ __launch_bounds__(kBlock) void k_libm(int n, const float *__restrict__ x, float *__restrict__ lo,
                                                 float *__restrict__ so, float *__restrict__ co) {
    int i = blockIdx.x * kBlock + threadIdx.x;
    vspg_libm::stage_logf_tab_lds();
    __syncthreads();
    if (i >= n) return;
    lo[i] = logf_(x[i]);
    so[i] = sinf_(x[i]);
    co[i] = cosf_(x[i]);
}
__global__ __launch_bounds__(kBlock) void k_libm_powf(int n, const float *__restrict__ x, const float *__restrict__ y, float *__restrict__ out) {
    int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = vspg_libm::powf_host_exact(x[i], y[i]);
}
__global__ __launch_bounds__(kBlock) void k_blackbody(int n, const float *__restrict__ u, const float *__restrict__ T, float *__restrict__ out) {
    int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const Spec s = blackbody_sample(T[i], u[i]);
    for (int k = 0; k < 3; ++k) out[6 * i + k] = sample_visible_wavelength(u[i], k);
    out[6 * i + 3] = s.r; out[6 * i + 4] = s.g; out[6 * i + 5] = s.b;
}
// vspg_envlight_batch (include/vspg.h): Le, PDF_Li and SampleLi of image infinite light k as the path kernels evaluate them
__global__ __launch_bounds__(kBlock) void k_envlight(const DScene *__restrict__ Sp, int k, int n, const float *__restrict__ dirs,
                                                     const float *__restrict__ u, float *__restrict__ out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const DScene &S = *Sp;
    float *o = out + (size_t)VSPG_ENVLIGHT_OUT * i;
    const V3 d = ld3(dirs + 3 * (size_t)i);
    float uv[2];
    const Spec Le = env_Le(S, k, d, uv);
    o[0] = Le.r; o[1] = Le.g; o[2] = Le.b;
    o[3] = uv[0]; o[4] = uv[1];
    o[5] = env_pdf_li(S, k, d);
    LightLi ls{};
    const bool ok = env_sample_li(S, k, mk(0, 0, 0), u[2 * (size_t)i], u[2 * (size_t)i + 1], &ls, uv);
    o[6] = ok ? 1.f : 0.f;
    o[7] = ok ? uv[0] : 0.f; o[8] = ok ? uv[1] : 0.f;
    o[9] = ok ? ls.wi.x : 0.f; o[10] = ok ? ls.wi.y : 0.f; o[11] = ok ? ls.wi.z : 0.f;
    o[12] = ok ? ls.pdf : 0.f;
    o[13] = ok ? ls.L.r : 0.f; o[14] = ok ? ls.L.g : 0.f; o[15] = ok ? ls.L.b : 0.f;
}
// vspg_portallight_batch (include/vspg.h): ImageBounds, Le, PDF_Li and SampleLi of portal light k as the path kernels evaluate them
__global__ __launch_bounds__(kBlock) void k_portallight(const DScene *__restrict__ Sp, int k, int n, const float *__restrict__ ctx_p,
                                                        const float *__restrict__ dirs, const float *__restrict__ u, float *__restrict__ out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const DScene &S = *Sp;
    float *o = out + (size_t)VSPG_PORTALLIGHT_OUT * i;
    for (int j = 0; j < VSPG_PORTALLIGHT_OUT; ++j) o[j] = 0.f;
    const V3 p = ld3(ctx_p + 3 * (size_t)i), d = ld3(dirs + 3 * (size_t)i);
    float b[4];
    if (portal_image_bounds(S.portal[k], p, b)) {
        o[0] = 1.f;
        for (int j = 0; j < 4; ++j) o[1 + j] = b[j];
    }
    float uv[2] = {0.f, 0.f}, rgb[3];
    const bool inside = portal_radiance(S.portal[k], p, d, rgb, uv);
    const Spec Le = portal_Le(S, k, p, d);
    o[5] = inside ? 1.f : 0.f;
    o[6] = uv[0]; o[7] = uv[1];
    o[8] = Le.r; o[9] = Le.g; o[10] = Le.b;
    o[11] = portal_pdf_li(S, k, p, d);
    LightLi ls{};
    PortalSample ps;
    const bool ok = portal_sample_li(S, k, p, u[2 * (size_t)i], u[2 * (size_t)i + 1], &ls, &ps);
    o[12] = ok ? 1.f : 0.f;
    if (ok) {
        o[13] = ps.u; o[14] = ps.v; o[15] = ps.mapPDF; o[16] = ps.duv_dw;
        o[17] = ls.wi.x; o[18] = ls.wi.y; o[19] = ls.wi.z;
        o[20] = ls.pdf;
        o[21] = ls.L.r; o[22] = ls.L.g; o[23] = ls.L.b;
        const V3 pl = ls.pLight.mid();
        o[27] = pl.x; o[28] = pl.y; o[29] = pl.z;
    }
    o[24] = (float)ps.trips_x; o[25] = (float)ps.trips_y; o[26] = (float)ps.why;
}
// vspg_light_sample_batch (include/vspg.h): lightSampler.Sample, lightSampler.PMF and light.SampleLi as the path kernels call them
__global__ __launch_bounds__(kBlock) void k_light_sample_batch(const DScene *__restrict__ Sp, int n, const float *__restrict__ ctx_p,
                                                               const float *__restrict__ ctx_n, const float *__restrict__ u, float *__restrict__ out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const DScene &S = *Sp;
    stage_scene_lds(S);  // sample_light reads a rectangle light's record from the LDS copy
    __syncthreads();
    if (i >= n) return;
    float *o = out + (size_t)VSPG_LIGHT_SAMPLE_OUT * i;
    for (int k = 0; k < VSPG_LIGHT_SAMPLE_OUT; ++k) o[k] = 0.f;
    const V3 p = ld3(ctx_p + 3 * (size_t)i), nn = ld3(ctx_n + 3 * (size_t)i);
    int lightIndex = 0;
    float pmf = 0.f;
    if (!light_sampler_sample(S, p, nn, u[3 * (size_t)i], &lightIndex, &pmf)) {
        o[0] = -1.f;
        return;
    }
    o[0] = (float)lightIndex;
    o[1] = pmf;
    o[2] = light_sampler_pmf(S, p, nn, lightIndex);
    LightLi ls{};
    bool delta_light = false;
    if (!sample_light(S, lightIndex, p, LsCtx{p3i_exact(p), nn}, u[3 * (size_t)i + 1], u[3 * (size_t)i + 2], &ls, &delta_light)) return;
    o[3] = 1.f;
    o[4] = ls.wi.x; o[5] = ls.wi.y; o[6] = ls.wi.z;
    o[7] = ls.L.r; o[8] = ls.L.g; o[9] = ls.L.b;
    o[10] = ls.pdf;
    const V3 pl = ls.pLight.mid();
    o[11] = pl.x; o[12] = pl.y; o[13] = pl.z;
    o[14] = delta_light ? 1.f : 0.f;
}
// vspg_texture_eval_batch (include/vspg.h): the reflectance of a vertex on primitive prim[i] (device numbering: a rectangle's index, or
// -2 - the triangle's position in S.tris) with the three floats hit[3i..], through tex_of_prim / texture_eval as vertex_setup<FULL> calls them
__global__ __launch_bounds__(kBlock) void k_texture_eval(const DScene *__restrict__ Sp, int n, const int32_t *__restrict__ prim,
                                                         const float *__restrict__ hit, float *__restrict__ out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const DScene &S = *Sp;
    stage_scene_lds(S);  // tex_uv_quad reads the rectangle's record from the LDS copy
    __syncthreads();
    if (i >= n) return;
    float *o = out + (size_t)VSPG_TEXTURE_EVAL_OUT * i;
    const int pr = prim[i];
    const V3 h = ld3(hit + 3 * (size_t)i);
    const int k = S.n_textured != 0 ? tex_of_prim(S, pr) : 0;
    if (k != 0) {
        const TexEval e = texture_eval(S, k, pr, h);
        o[0] = e.uv.u; o[1] = e.uv.v; o[2] = e.s; o[3] = e.t;
        o[4] = e.R.r; o[5] = e.R.g; o[6] = e.R.b;
        o[7] = e.has_lobes ? 1.f : 0.f;
    } else {  // an untextured surface: its (u, v) and the constant reflectance of bsdf_make / bsdf_make_tri
        TexUv uv;
        Bsdf b;
        if (is_tri(pr)) {
            alignas(8) const float def[6] = {0.f, 0.f, 1.f, 0.f, 1.f, 1.f};  // the default uv (0,0) (1,0) (1,1)
            uv = tex_uv_tri(def, h);
            b = bsdf_make_tri(S.tris[tri_of(pr)]);
        } else {
            uv = tex_uv_quad(quad_at(pr), h);
            b = bsdf_make<false>(quad_at(pr));
        }
        o[0] = uv.u; o[1] = uv.v; o[2] = 0.f; o[3] = 0.f;
        o[4] = b.R.r; o[5] = b.R.g; o[6] = b.R.b;
        o[7] = b.has_lobes ? 1.f : 0.f;
    }
}
// vspg_camera_ray_batch (include/vspg.h): the render-space camera ray of sample sample_index[i] of pixel pixel_xy[2i..] -- the raster
// point as start_path_common forms it (BoxFilter radius .5) and camera_generate_ray (vspg_camera.h) itself.  u: the filter's and the
// lens's variates per element, or null: the renderer's sampler in start_path_common's order (wavelength, filter 2, time, lens 2).
__global__ __launch_bounds__(kBlock) void k_camera_ray(const DScene *__restrict__ Sp, int n, const int32_t *__restrict__ pixel_xy,
                                                       const int32_t *__restrict__ sample_index, const float *__restrict__ u,
                                                       float *__restrict__ out_o, float *__restrict__ out_d) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const DScene &S = *Sp;
    const int px = pixel_xy[2 * (size_t)i], py = pixel_xy[2 * (size_t)i + 1];
    float f0, f1, l0, l1;
    if (u) {
        f0 = u[4 * (size_t)i], f1 = u[4 * (size_t)i + 1], l0 = u[4 * (size_t)i + 2], l1 = u[4 * (size_t)i + 3];
    } else {
        Sampler sampler;
        sampler.start_pixel_sample(px, py, S.seed, sample_index[i]);
        (void)sampler.get1d();  // wavelength
        f0 = sampler.get1d(), f1 = sampler.get1d();
        (void)sampler.get1d();  // time
        l0 = sampler.get1d(), l1 = sampler.get1d();
    }
    const float fpx = (1 - f0) * -0.5f + f0 * 0.5f, fpy = (1 - f1) * -0.5f + f1 * 0.5f;
    const float pfx = ((float)px + fpx) + 0.5f, pfy = ((float)py + fpy) + 0.5f;
    V3 ro, rd;
    camera_generate_ray(S, pfx, pfy, l0, l1, &ro, &rd);
    float *o = out_o + 3 * (size_t)i, *d = out_d + 3 * (size_t)i;
    o[0] = ro.x; o[1] = ro.y; o[2] = ro.z;
    d[0] = rd.x; d[1] = rd.y; d[2] = rd.z;
}
// vspg_light_pdf_batch (include/vspg.h): for one light with a shape (a rectangle or a sphere of the light list) what li_surface_pre
// computes when a ray from the context along wi is weighed against it -- light_sampler_pmf, light_pdf_li / sphere_pdf_li, and the
// shape's own intersection from ctx.SpawnRay(wi) with light_L / sphere_light_L at the hit.  ctx_perr == nullptr: exact points.
__global__ __launch_bounds__(kBlock) void k_light_pdf_batch(const DScene *__restrict__ Sp, int lightIndex, int n, const float *__restrict__ ctx_p,
                                                            const float *__restrict__ ctx_perr, const float *__restrict__ ctx_n,
                                                            const float *__restrict__ wi_in, float *__restrict__ out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const DScene &S = *Sp;
    stage_scene_lds(S);
    __syncthreads();
    if (i >= n) return;
    float *o = out + (size_t)VSPG_LIGHT_PDF_OUT * i;
    for (int k = 0; k < VSPG_LIGHT_PDF_OUT; ++k) o[k] = 0.f;
    const V3 p = ld3(ctx_p + 3 * (size_t)i), wi = ld3(wi_in + 3 * (size_t)i);
    LsCtx ctx;
    ctx.pi = ctx_perr ? p3i_from_err(p, ld3(ctx_perr + 3 * (size_t)i)) : p3i_exact(p);
    ctx.n = ld3(ctx_n + 3 * (size_t)i);
    o[1] = light_sampler_pmf(S, ctx.pi.mid(), ctx.n, lightIndex);
    const V3 ro = offset_ray_origin(ctx.pi, ctx.n, wi);  // ctx.SpawnRay(wi)
    float t = 0.f;
    V3 ph;
    Spec L = sp(0.f);
    bool hit;
    if (lightIndex < S.n_lights) {
        const DQuad &q = light_quad_at(lightIndex);
        o[0] = light_pdf_li(q, ctx, wi);
        hit = quad_intersect(q, ro, wi, kInf, &t, &ph);
        if (hit) L = light_L(q, ld3(q.n), -wi);
    } else {  // (the host admits nothing else) an emissive sphere
        const int si = S.light_spheres[lightIndex - S.n_lights - S.n_inf - S.n_point];
        const DSphere &sph = S.spheres[si];
        const DSphereLight &E = S.sphere_light[si];
        o[0] = sphere_pdf_li(sph, E, ctx, wi);
        hit = sphere_intersect(sph, ro, wi, kInf, &t, &ph);
        if (hit) L = sphere_light_L(E, sphere_interaction<false>(sph, ph).n, -wi);
    }
    if (!hit) return;
    o[2] = 1.f;
    o[3] = L.r; o[4] = L.g; o[5] = L.b;
    o[6] = t;
}
__global__ __launch_bounds__(kBlock) void k_libm_log1m(int n, const float *__restrict__ x, float *__restrict__ out) {
    int i = blockIdx.x * kBlock + threadIdx.x;
    vspg_libm::stage_log_tab_lds();
    __syncthreads();
    if (i >= n) return;
    out[i] = neg_log1m_d(x[i]);
}

// ---- octet bricks (DScene::brick_index / octets) built on the device from the uploaded raw samples -------------------
// brick (bx, by, bz) covers the octets of base voxels [8b - 1, 8b + 6]^3, i.e. raw voxels [8b - 1, 8b + 7]^3
__device__ __forceinline__ float raw_at(const float *d, int nx, int ny, int nz, int x, int y, int z) {
    if (x < 0 || y < 0 || z < 0 || x >= nx || y >= ny || z >= nz) return 0.f;
    return d[((size_t)z * ny + y) * nx + x];
}
__global__ __launch_bounds__(kBlock) void k_brick_flags(const float *__restrict__ d, int nx, int ny, int nz, int bnx, int bny,
                                                        int32_t *__restrict__ flags) {
    const int b = blockIdx.x;
    const int bx = b % bnx, by = (b / bnx) % bny, bz = b / (bnx * bny);
    __shared__ int s_any;
    if (threadIdx.x == 0) s_any = 0;
    __syncthreads();
    bool any = false;
    for (int i = threadIdx.x; i < 9 * 9 * 9; i += kBlock) {
        const int x = 8 * bx - 1 + i % 9, y = 8 * by - 1 + (i / 9) % 9, z = 8 * bz - 1 + i / 81;
        any = any || raw_at(d, nx, ny, nz, x, y, z) != 0.f;
    }
    if (any) s_any = 1;
    __syncthreads();
    if (threadIdx.x == 0) flags[b] = s_any;
}
__global__ __launch_bounds__(512) void k_brick_fill(const float *__restrict__ d, int nx, int ny, int nz, int bnx, int bny,
                                                    const int32_t *__restrict__ active /* brick number of slot */, float4 *__restrict__ octets) {
    const int b = active[blockIdx.x];
    const int bx = b % bnx, by = (b / bnx) % bny, bz = b / (bnx * bny);
    const int l = threadIdx.x, lx = l & 7, ly = (l >> 3) & 7, lz = l >> 6;
    const int ix = 8 * bx + lx - 1, iy = 8 * by + ly - 1, iz = 8 * bz + lz - 1;  // base voxel of this octet
    float4 lo, hi;
    lo.x = raw_at(d, nx, ny, nz, ix, iy, iz);         lo.y = raw_at(d, nx, ny, nz, ix + 1, iy, iz);
    lo.z = raw_at(d, nx, ny, nz, ix, iy + 1, iz);     lo.w = raw_at(d, nx, ny, nz, ix + 1, iy + 1, iz);
    hi.x = raw_at(d, nx, ny, nz, ix, iy, iz + 1);     hi.y = raw_at(d, nx, ny, nz, ix + 1, iy, iz + 1);
    hi.z = raw_at(d, nx, ny, nz, ix, iy + 1, iz + 1); hi.w = raw_at(d, nx, ny, nz, ix + 1, iy + 1, iz + 1);
    float4 *q = octets + ((size_t)blockIdx.x * 512u + (size_t)l) * 2u;
    q[0] = lo;
    q[1] = hi;
}

// ---- majorant grid of a grid medium built on the device (vspg_renderer_update_grid) ------------------------------------
// One workgroup per majorant cell: the cell's majorant is the maximum over its voxel box [lo, hi]^3.  The box separates per axis, and
// the per-axis tables (ranges[axis * R + c] = {lo, hi} in array coordinates, clipped to the grid; hi < lo: empty) come from the host
// (majorant_axis_ranges: the arithmetic create's builders use -- recomputed here, the NANOVDB lerp and the double division would have to
// match the host's rounding).  A box holds a handful of voxels (a small grid under 64^3 cells) or several hundred thousand (1024^3
// under 16^3 cells: 66^3): the threads stride over the flattened box, x fastest, so a wavefront reads runs of whole rows; then a
// wavefront reduction through lane shuffles and one through LDS.  The maximum of finite floats does not depend on the order.
// NVDB: the start value is 0 and the cell gets (max + density_offset) * majorant_scale; GRID: the start value is the voxel at lo.
constexpr int kMajBlock = 256;
template <bool NVDB>
__global__ __launch_bounds__(kMajBlock) void k_majorant_build(const float *__restrict__ d, int nx, int ny, int R,
                                                             const int2 *__restrict__ ranges, float density_offset, float majorant_scale,
                                                             float *__restrict__ maj) {
    const int c = blockIdx.x;
    const int2 rx = ranges[c % R], ry = ranges[R + (c / R) % R], rz = ranges[2 * R + c / (R * R)];
    const int bx = rx.y - rx.x + 1, by = ry.y - ry.x + 1, bz = rz.y - rz.x + 1;
    // (a box lies inside the grid, and a grid holds at most 2^31 voxels: unsigned arithmetic holds the count and the strided index)
    const unsigned n = (bx > 0 && by > 0 && bz > 0) ? (unsigned)bx * (unsigned)by * (unsigned)bz : 0u;
    float mx = 0.f;
    if (!NVDB && n > 0) mx = d[((size_t)rz.x * ny + ry.x) * nx + rx.x];
    for (unsigned i = threadIdx.x; i < n; i += kMajBlock) {
        const unsigned row = i / (unsigned)bx, zz = row / (unsigned)by;
        const int x = rx.x + (int)(i - row * (unsigned)bx), y = ry.x + (int)(row - zz * (unsigned)by), z = rz.x + (int)zz;
        const float v = d[((size_t)z * ny + y) * nx + x];
        mx = mx < v ? v : mx;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float v = __shfl_down(mx, o, 64);
        mx = mx < v ? v : mx;
    }
    __shared__ float s_max[kMajBlock / 64];
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kMajBlock / 64; ++w) mx = mx < s_max[w] ? s_max[w] : mx;
        maj[c] = NVDB ? (mx + density_offset) * majorant_scale : mx;
    }
}

// ImageSpaceGuidingBuffer::Update stand-in: 5x5 box filter over the sufficient statistics,
// then the contribution / variance criterion (own design, unpinned).
constexpr int kIsgRadius = 2;
// One workgroup = one 16 x 16 pixel tile: the five statistics of the tile and its two-pixel halo are staged in LDS with one
// coalesced pass, and the 25 taps of a pixel read LDS (round 5; as 50 global loads per pixel the kernel took 113 us per 1080p
// update against ~15 us of HBM time).  The sum keeps its order -- rows outer, columns inner, taps outside the image skipped --
// so the buffer keeps its bits.
constexpr int kIsgTile = 16;
static_assert(kIsgTile * kIsgTile == kBlock, "one thread per pixel of the tile");
__global__ __launch_bounds__(kBlock) void k_isg_update(int W, int H, int criterion, const float *__restrict__ stats,
                                                       float *__restrict__ vsp /* null: leave the VSP buffer alone */,
                                                       float *__restrict__ contrib /* null: no contribution estimate */) {
    constexpr int TW = kIsgTile + 2 * kIsgRadius;
    __shared__ float s_t[5][TW * TW];
    const int tx0 = (int)blockIdx.x * kIsgTile - kIsgRadius, ty0 = (int)blockIdx.y * kIsgTile - kIsgRadius;
    for (int j = threadIdx.x; j < TW * TW; j += kBlock) {
        const int xx = tx0 + j % TW, yy = ty0 + j / TW;
        float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f);
        float s4 = 0.f;
        if (xx >= 0 && xx < W && yy >= 0 && yy < H) {
            const float *st = stats + ((size_t)yy * W + xx) * VSPG_ISG_STATS;
            s0 = *reinterpret_cast<const float4 *>(st);
            s4 = st[4];
        }
        s_t[0][j] = s0.x; s_t[1][j] = s0.y; s_t[2][j] = s0.z; s_t[3][j] = s0.w; s_t[4][j] = s4;
    }
    __syncthreads();
    const int lx = threadIdx.x % kIsgTile, ly = threadIdx.x / kIsgTile;
    const int x = (int)blockIdx.x * kIsgTile + lx, y = (int)blockIdx.y * kIsgTile + ly;
    if (x >= W || y >= H) return;
    const int i = y * W + x;
    float a[5] = {0, 0, 0, 0, 0};
    for (int dy = -kIsgRadius; dy <= kIsgRadius; ++dy)
        for (int dx = -kIsgRadius; dx <= kIsgRadius; ++dx) {
            int xx = x + dx, yy = y + dy;
            if (xx < 0 || xx >= W || yy < 0 || yy >= H) continue;
            const int j = (ly + kIsgRadius + dy) * TW + (lx + kIsgRadius + dx);
            a[0] += s_t[0][j]; a[1] += s_t[1][j]; a[2] += s_t[2][j]; a[3] += s_t[3][j]; a[4] += s_t[4][j];
        }
    float r = -1.f;
    if (a[0] > 0) {
        float v, s;
        if (criterion == VSPG_VSP_VARIANCE) {
            v = __builtin_sqrtf(a[3] / a[0]);
            s = __builtin_sqrtf(a[4] / a[0]);
        } else {
            v = a[1] / a[0];
            s = a[2] / a[0];
        }
        if (v + s > 0) r = v / (v + s);
    }
    if (vsp) vsp[i] = r;
    // contribution estimate for guided RR (own stand-in): filtered mean of the samples' average radiance, 0 = none
    if (contrib) contrib[i] = a[0] > 0 ? (a[1] + a[2]) / a[0] : 0.f;
}

}  // namespace
