// portallight_build_check -- the portal light's host builder (portal_refusal, portal_build_tables: csrc/vspg_scene_build.hip) and the
// host build of its sampling code (csrc/vspg_portalmap.h, the text the kernels compile) in a stand-alone program, for the sanitizers:
// tests/test_portallight_model.py compiles it with the two host-only units under ASan / UBSan, feeds it case files written from
// tests/portallight_model.py and compares what it writes with the model bit for bit.
//
//   portallight_build_check CASE OUT [CASE OUT ...]
// CASE (little endian): int32 res, n; float m34[12], portal[12], L[3], scene_radius; float image[res*res*3]; float ctx[3n], dirs[3n], u[2n]
// OUT: int32 refused (1: nothing else follows); float record[20]; image[res*res*3]; func[res*res]; table[res*res]; phi[3]; out[32n]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vspg_scene_build.h"
#include "vspg_portalmap.h"

using namespace vspg_host;

static bool read_all(FILE *f, void *p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

static int run_case(const char *in, const char *outp) {
    FILE *f = fopen(in, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", in); return 2; }
    int32_t hdr[2];
    float m34[12], portal[12], L[3], radius;
    if (!read_all(f, hdr, sizeof hdr) || !read_all(f, m34, sizeof m34) || !read_all(f, portal, sizeof portal) || !read_all(f, L, sizeof L) ||
        !read_all(f, &radius, 4)) { fprintf(stderr, "%s: short header\n", in); fclose(f); return 2; }
    const int res = hdr[0], n = hdr[1];
    if (res < 1 || res > 4096 || n < 0 || n > (1 << 20)) { fprintf(stderr, "%s: bad sizes\n", in); fclose(f); return 2; }
    std::vector<float> image((size_t)res * res * 3), ctx((size_t)n * 3), dirs((size_t)n * 3), u((size_t)n * 2);
    if (!read_all(f, image.data(), image.size() * 4) || !read_all(f, ctx.data(), ctx.size() * 4) || !read_all(f, dirs.data(), dirs.size() * 4) ||
        !read_all(f, u.data(), u.size() * 4)) { fprintf(stderr, "%s: short body\n", in); fclose(f); return 2; }
    fclose(f);
    FILE *o = fopen(outp, "wb");
    if (!o) { fprintf(stderr, "cannot write %s\n", outp); return 2; }
    float m[9], mi[9];
    int32_t refused = !env_matrices(m34, m, mi) || portal_refusal(portal) != 0;
    fwrite(&refused, 4, 1, o);
    if (refused) { fclose(o); return 0; }
    PortalTables T;
    portal_build_tables(image.data(), res, mi, portal, &T);
    DPortalLight P = T.rec;
    P.image = T.env.buf.data() + T.o_image;
    P.func = T.env.buf.data() + T.o_func;
    P.sat = T.env.buf.data() + T.o_sat;
    float rec[20] = {0};
    for (int c = 0; c < 3; ++c) {
        rec[c] = P.p0[c]; rec[3 + c] = P.p2[c]; rec[6 + c] = P.fx[c]; rec[9 + c] = P.fy[c]; rec[12 + c] = P.fz[c]; rec[16 + c] = P.sum_phi[c];
    }
    rec[15] = P.area;
    fwrite(rec, 4, 20, o);
    const size_t npx = (size_t)res * res;
    fwrite(P.image, 4, npx * 3, o);
    fwrite(P.func, 4, npx, o);
    fwrite(P.sat, 4, npx, o);
    float phi[3];  // PortalImageInfiniteLight::Phi as lsb::build forms it
    for (int c = 0; c < 3; ++c) phi[c] = L[c] * P.area * P.sum_phi[c] / (float)(res * res);
    fwrite(phi, 4, 3, o);
    std::vector<float> out((size_t)n * VSPG_PORTALLIGHT_OUT, 0.f);
    for (int i = 0; i < n; ++i) {  // what k_portallight (csrc/vspg_probe_kernels.h) writes
        float *e = out.data() + (size_t)i * VSPG_PORTALLIGHT_OUT;
        const V3 p = ld3(&ctx[3 * (size_t)i]), d = ld3(&dirs[3 * (size_t)i]);
        float b[4];
        if (portal_image_bounds(P, p, b)) {
            e[0] = 1.f;
            for (int j = 0; j < 4; ++j) e[1 + j] = b[j];
        }
        float uv[2] = {0.f, 0.f}, rgb[3] = {0.f, 0.f, 0.f};
        const bool inside = portal_radiance(P, p, d, rgb, uv);
        e[5] = inside ? 1.f : 0.f;
        e[6] = uv[0]; e[7] = uv[1];
        for (int c = 0; c < 3; ++c) e[8 + c] = inside ? rgb[c] * L[c] : 0.f;
        e[11] = portal_pdf(P, p, d);
        PortalSample ps = {};
        const bool ok = portal_sample(P, p, u[2 * (size_t)i], u[2 * (size_t)i + 1], &ps);
        e[12] = ok ? 1.f : 0.f;
        if (ok) {
            e[13] = ps.u; e[14] = ps.v; e[15] = ps.mapPDF; e[16] = ps.duv_dw;
            e[17] = ps.wi.x; e[18] = ps.wi.y; e[19] = ps.wi.z;
            e[20] = ps.pdf;
            for (int c = 0; c < 3; ++c) e[21 + c] = ps.rgb[c] * L[c];
            const V3 pl = p + ps.wi * (2 * radius);
            e[27] = pl.x; e[28] = pl.y; e[29] = pl.z;
        }
        e[24] = (float)ps.trips_x; e[25] = (float)ps.trips_y; e[26] = (float)ps.why;
    }
    fwrite(out.data(), 4, out.size(), o);
    fclose(o);
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 3 || (argc - 1) % 2) { fprintf(stderr, "usage: %s CASE OUT [CASE OUT ...]\n", argv[0]); return 2; }
    for (int i = 1; i + 1 < argc; i += 2)
        if (const int rc = run_case(argv[i], argv[i + 1])) return rc;
    printf("%d cases\n", (argc - 1) / 2);
    return 0;
}
