// vspg_pbrt -- render a pbrt-v4 scene file (the subset of vspg_scenefile.h) with the MI355X-native GuidedVolPathVSPG path.
//   vspg_pbrt scene.pbrt [--spp N] [--outfile image.exr|image.pfm] [--seed S] [--device D] [--wave-log waves.jsonl] [--parse-only]
//             [--cropwindow x0,x1,y0,y1] [--pixelbounds x0,x1,y0,y1]   (cmd/pbrt.cpp:132-153; they override the file's Film parameters)
//             [--mse-reference-image ref.exr|ref.pfm --mse-reference-out file]  (cmd/pbrt.cpp:60-61, :244-248: after every wave the MSE
//              of the film against the image is appended to the file as "spp, mse", cpu/integrators.cpp:243-257; reduced on the device.
//              vspg_pbrt_sharded does not cover it.)
//             [--write-partial-images]   (cmd/pbrt.cpp:81, integrators.cpp:258-261: the image file is rewritten after every wave)
// The counterpart of `pbrt scene.pbrt` for this integrator (cmd/pbrt.cpp -> RenderCPU, cpu/render.cpp:56-57); the image is written
// by its extension (RGBFilm::WriteImage, film.cpp:531-569): OpenEXR -- resolved on the device, HALF unless the Film says
// "bool savefp16" false -- or PFM.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "vspg_scenefile.h"

int main(int argc, char **argv) {
    std::string scene, out;
    int spp = -1, seed = -1, device = 0;
    std::string waveLogPath;
    bool parseOnly = false, writePartial = false;
    vspg::FilmOverrides film;
    std::string cropArg, boundsArg;
    std::string mseImagePath, mseOutPath;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto next = [&]() -> const char * { if (i + 1 >= argc) { std::fprintf(stderr, "%s needs a value\n", a.c_str()); std::exit(2); } return argv[++i]; };
        if (a == "--spp") spp = std::atoi(next());
        else if (a == "--outfile") out = next();
        else if (a == "--seed") seed = std::atoi(next());
        else if (a == "--device") device = std::atoi(next());
        else if (a == "--wave-log") waveLogPath = next();
        else if (a == "--parse-only") parseOnly = true;
        else if (a == "--cropwindow") cropArg = next();
        else if (a == "--pixelbounds") boundsArg = next();
        else if (a == "--mse-reference-image") mseImagePath = next();
        else if (a == "--mse-reference-out") mseOutPath = next();
        else if (a == "--write-partial-images") writePartial = true;
        else if (!a.empty() && a[0] == '-') { std::fprintf(stderr, "unknown option %s\n", a.c_str()); return 2; }
        else scene = a;
    }
    if (scene.empty()) { std::fprintf(stderr, "usage: vspg_pbrt scene.pbrt [--spp N] [--outfile image.exr|image.pfm] [--seed S] [--device D] [--wave-log waves.jsonl] [--parse-only] [--cropwindow x0,x1,y0,y1] [--pixelbounds x0,x1,y0,y1] [--mse-reference-image ref.exr|ref.pfm --mse-reference-out file] [--write-partial-images]\n"); return 2; }
    try {
        vspg::CheckMseReferenceOptions(mseImagePath, mseOutPath);
        if (!cropArg.empty()) vspg::ParseCropWindowArg(cropArg, &film);
        if (!boundsArg.empty()) vspg::ParsePixelBoundsArg(boundsArg, &film);
        auto sd = vspg::ParseSceneFile(scene);
        vspg::ResolvePixelBounds(*sd, film);
        if (spp > 0) sd->pixelSamples = spp;
        if (seed >= 0) sd->seed = seed;
        if (!out.empty()) sd->filmFilename = out;
        for (const auto &w : sd->warnings) std::fprintf(stderr, "Warning: %s\n", w.c_str());
        std::printf("scene: %d rectangles, %d triangles, %d infinite lights, medium type %d%s, film %dx%d @ %d spp, integrator \"%s\"",
                    sd->scene.n_quads, sd->scene.n_triangles, sd->scene.n_infinite_lights, sd->scene.medium.type,
                    sd->scene.medium.has_transform ? " (placed)" : "", sd->xres, sd->yres, sd->pixelSamples, sd->integratorName.c_str());
        {   // medium boundaries: spheres, interface-material surfaces, medium transitions, the camera's side
            int n_interface = 0, n_transition = 0;
            auto transition = [](int b) { b &= VSPG_IFACE_INSIDE | VSPG_IFACE_OUTSIDE; return b == VSPG_IFACE_INSIDE || b == VSPG_IFACE_OUTSIDE; };
            for (int i = 0; i < sd->scene.n_quads; ++i) { n_interface += sd->scene.quads[i].material == VSPG_MATERIAL_INTERFACE; n_transition += transition(sd->scene.quads[i].medium_interface); }
            for (int i = 0; i < sd->scene.n_spheres; ++i) { n_interface += sd->scene.spheres[i].material == VSPG_MATERIAL_INTERFACE; n_transition += transition(sd->scene.spheres[i].medium_interface); }
            for (size_t i = 0; i < sd->triFlags.size(); ++i) { n_interface += (sd->triFlags[i] & VSPG_TRI_INTERFACE) != 0; n_transition += transition(sd->triFlags[i] >> VSPG_TRI_IFACE_SHIFT); }
            if (sd->scene.n_spheres || n_interface || n_transition || sd->scene.camera_outside_medium)
                std::printf("; %d spheres, %d interface-material surfaces, %d medium transitions, camera %s the medium", sd->scene.n_spheres, n_interface, n_transition,
                            sd->scene.camera_outside_medium ? "outside" : "in");
        }
        if (sd->scene.medium.type == VSPG_MEDIUM_RGBGRID)
            std::printf("; RGB grid %d x %d x %d:%s%s%s, scale %g, Lescale %g", sd->scene.medium.nx, sd->scene.medium.ny, sd->scene.medium.nz, sd->scene.rgb_sigma_a ? " sigma_a" : "",
                        sd->scene.rgb_sigma_s ? " sigma_s" : "", sd->scene.rgb_Le ? " Le" : "", sd->scene.rgb_sigma_scale, sd->scene.rgb_le_scale);
        if (sd->scene.medium.temperature) std::printf("; temperature grid (blackbody emission under \"vspsamplingmethod\" \"nds\")");
        std::printf("\n");
        std::printf("pixel bounds: [ (%d, %d) - (%d, %d) ]\n", sd->boundsX0, sd->boundsY0, sd->boundsX1, sd->boundsY1);
        {   // the camera: the model (VSPG_CAMERA_*), its lens and the raster map (%.9g round-trips a float)
            const VspgCamera &c = sd->scene.camera;
            std::printf("camera: model %d lens_radius %.9g focal_distance %.9g raster (%.9g, %.9g, %.9g, %.9g)\n", sd->cameraModel.model, sd->cameraModel.lens_radius,
                        sd->cameraModel.focal_distance, c.sx, c.ox, c.sy, c.oy);
        }
        std::vector<float> mseImage;
        if (!mseImagePath.empty()) {
            mseImage = vspg::LoadMseReferenceImage(mseImagePath, sd->xres, sd->yres, sd->boundsX0, sd->boundsY0, sd->boundsX1, sd->boundsY1);
            std::printf("MSE reference image: %s\n", mseImagePath.c_str());
        }
        for (int i = 0; i < sd->scene.n_point_lights; ++i) {  // one line per point light: position (renderFromLight's translation) and I, %.9g round-trips a float
            const VspgPointLight &pl = sd->scene.point_lights[i];
            std::printf("point light %d: type %d at (%.9g, %.9g, %.9g) I (%.9g, %.9g, %.9g)", i, pl.type, pl.render_from_light[3], pl.render_from_light[7],
                        pl.render_from_light[11], pl.I[0], pl.I[1], pl.I[2]);
            if (pl.type == VSPG_LIGHT_PROJECTION || pl.type == VSPG_LIGHT_GONIOMETRIC) {  // ... and of a projection / goniometric light its image
                int xres = 1, yres = 1;
                for (const auto &l : sd->lightImages)
                    if (l.slot == i) { xres = l.xres; yres = l.yres; }
                std::printf(" %s image %d x %d", pl.type == VSPG_LIGHT_PROJECTION ? "projection" : "goniometric", xres, yres);
                if (pl.type == VSPG_LIGHT_PROJECTION) std::printf(" fov %.9g", pl.cone_angle_deg);
            }
            std::printf("\n");
        }
        {   // ... the image textures and the surfaces that carry one
            const VspgSceneTextures &tx = sd->textures;
            for (int k = 0; k < tx.n_textures; ++k) {
                const VspgTexture &t = tx.textures[k];
                std::printf("texture %d: %d x %d x %d wrap %d filter %d invert %d scale %.9g mapping (%.9g, %.9g, %.9g, %.9g)\n", k, t.xres, t.yres, t.channels,
                            t.wrap, t.filter, t.invert, t.scale, t.su, t.sv, t.du, t.dv);
            }
            for (int i = 0; i < sd->scene.n_quads; ++i)
                if (tx.quad_texture[i]) std::printf("rectangle %d: texture %d\n", i, tx.quad_texture[i] - 1);
            for (int i = 0; tx.tri_texture && i < sd->scene.n_triangles; ++i)
                if (tx.tri_texture[i])
                    std::printf("triangle %d: texture %d uv (%.9g, %.9g) (%.9g, %.9g) (%.9g, %.9g)\n", i, tx.tri_texture[i] - 1, tx.tri_uv[6 * i], tx.tri_uv[6 * i + 1],
                                tx.tri_uv[6 * i + 2], tx.tri_uv[6 * i + 3], tx.tri_uv[6 * i + 4], tx.tri_uv[6 * i + 5]);
        }
        if (parseOnly) return 0;
        auto integrator = vspg::CreateIntegrator(*sd, device);
        std::printf("%s\n", integrator->ToString().c_str());
        auto *vi = static_cast<vspg::GuidedVolPathVSPGIntegrator *>(integrator.get());
        std::FILE *wl = nullptr;
        if (!waveLogPath.empty()) {
            wl = std::fopen(waveLogPath.c_str(), "w");
            if (!wl) throw vspg::Error("cannot open " + waveLogPath);
            vi->SetWaveLog(wl);
        }
        std::FILE *mseOut = nullptr;
        if (!mseImagePath.empty()) {
            mseOut = std::fopen(mseOutPath.c_str(), "w");  // (integrators.cpp:155-157)
            if (!mseOut) throw vspg::Error(mseOutPath + ": cannot open for writing");
            vi->SetMseReference(mseImage, mseOut);
        }
        vi->SetOutput(sd->filmFilename, sd->saveFP16, writePartial);
        integrator->Render();
        if (wl) { vi->SetWaveLog(nullptr); std::fclose(wl); }
        if (mseOut) std::fclose(mseOut);
        vi->WriteImage();
        VspgCounters c = vi->Counters();
        std::printf("paths %llu segments %llu -> %s\n", (unsigned long long)c.paths, (unsigned long long)c.segments, sd->filmFilename.c_str());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
