// example_render.cpp -- the scene-file lines of SURVEY.md App. F expressed through the host adapter:
//   Integrator "guidedvolpathvspg" "integer maxdepth" 5 "bool vspguiding" true "bool surfaceguiding" false ...
//   MakeNamedMedium "fog" "string type" "homogeneous" "rgb sigma_a" [.05 .05 .05] "rgb sigma_s" [.45 .45 .45] "float g" 0
// usage: example_render [xres yres spp out.pfm [train|load cachefile | trstore|trload tr.pfm | sequence frame1.pfm | rgbsequence frame1.pfm]]
//   train: the reference's default guiding options (cfg 5: the field trains in-loop) + "bool storeGuidingCache" true
//   load:  the same options + "bool loadGuidingCache" true (no training, guidedvolpathvspgintegrator.cpp:117-122)
//   trstore / trload: the NDS+ workflow on a thin 12^3 "uniformgrid" medium -- pass 1 "vspsamplingmethod" resampling +
//          "bool storeTrBuffer" true, pass 2 "vspsamplingmethod" nds + "bool collisionProbabilityBias" true + "bool loadTrBuffer" true
//   sequence: two frames of a volume sequence on the 12^3 "uniformgrid" medium through ONE integrator -- frame 0 to out.pfm, then
//          SetMediumDensity + ClearFilm + Render, frame 1 to frame1.pfm; a density of the wrong size is refused ("refused: ...")
//   rgbsequence: the same for a coloured 10 x 9 x 8 "rgbgrid" medium (sigma_a and sigma_s grids) -- frame 0 to out.pfm, then
//          SetMediumRgbGrids + ClearFilm + Render, frame 1 to frame1.pfm; grids of the wrong size and an Le grid the scene never had are
//          refused
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "vspg_host.h"

// the "rgbsequence" frames: R G B per voxel, x fastest; every value a small integer over a power of two (exact in float)
static const int kRgbN[3] = {10, 9, 8};
static vspg::RgbGridStorage rgb_frame(int frame) {
    static const int A[2][5] = {{7, 13, 29, 3, 17}, {3, 5, 11, 2, 11}}, S[2][5] = {{5, 11, 3, 7, 13}, {13, 7, 5, 3, 17}};
    vspg::RgbGridStorage g;
    for (int k = 0; k < kRgbN[2]; ++k)
        for (int j = 0; j < kRgbN[1]; ++j)
            for (int i = 0; i < kRgbN[0]; ++i)
                for (int c = 0; c < 3; ++c) {
                    g.sigma_a.push_back((float)((i * A[frame][0] + j * A[frame][1] + k * A[frame][2] + c * A[frame][3]) % A[frame][4]) / 64.f);
                    g.sigma_s.push_back((float)((i * S[frame][0] + j * S[frame][1] + k * S[frame][2] + c * S[frame][3]) % S[frame][4]) / 4.f);
                }
    return g;
}

int main(int argc, char **argv) {
    int xres = argc > 1 ? std::atoi(argv[1]) : 256, yres = argc > 2 ? std::atoi(argv[2]) : 256;
    int spp = argc > 3 ? std::atoi(argv[3]) : 16;
    const char *out = argc > 4 ? argv[4] : "fogbox.pfm";
    try {
        VspgScene scene;
        if (vspg_scene_fog_box(&scene, xres, yres) != 0) throw vspg::Error(vspg_last_error());
        scene.medium = vspg::CreateMedium("homogeneous", vspg::ParameterDictionary()
                                                             .RGB("sigma_a", .05f, .05f, .05f)
                                                             .RGB("sigma_s", .45f, .45f, .45f)
                                                             .Float("g", 0.f));
        vspg::ParameterDictionary ip;
        const std::string mode = argc > 6 ? argv[5] : "";
        std::vector<float> densityStorage;
        vspg::RgbGridStorage rgbStorage;
        if (mode == "rgbsequence") {
            const vspg::RgbGridStorage f0 = rgb_frame(0);
            scene.medium = vspg::CreateMedium("rgbgrid", vspg::ParameterDictionary()
                                                             .Int("nx", kRgbN[0]).Int("ny", kRgbN[1]).Int("nz", kRgbN[2])
                                                             .RGBArray("sigma_a", f0.sigma_a).RGBArray("sigma_s", f0.sigma_s)
                                                             .Point3("p0", -0.8f, -0.8f, -0.5f).Point3("p1", 0.8f, 0.7f, 0.9f)
                                                             .Float("g", 0.3f).Float("scale", 1.5f),
                                             nullptr, nullptr, nullptr, &rgbStorage);
            rgbStorage.Attach(&scene);
            ip.Int("maxdepth", 5).Bool("vspguiding", true).Bool("surfaceguiding", false).Bool("volumeguiding", false)
                .Bool("vspsecondaryguiding", false);
        } else if (mode == "trstore" || mode == "trload" || mode == "sequence") {
            const int n = 12;
            std::vector<float> d((size_t)n * n * n);
            for (int k = 0; k < n; ++k)
                for (int j = 0; j < n; ++j)
                    for (int i = 0; i < n; ++i) d[((size_t)k * n + j) * n + i] = (float)((i * 7 + j * 13 + k * 29) % 17) / 16.f;
            scene.medium = vspg::CreateMedium("uniformgrid", vspg::ParameterDictionary()
                                                                 .Int("nx", n).Int("ny", n).Int("nz", n)
                                                                 .FloatArray("density", d)
                                                                 .Point3("p0", -0.8f, -0.8f, -0.5f).Point3("p1", 0.8f, 0.7f, 0.9f)
                                                                 .RGB("sigma_a", .02f, .03f, .04f).RGB("sigma_s", .5f, .45f, .4f)
                                                                 .Float("g", 0.3f),
                                             &densityStorage);
            ip.Int("maxdepth", 5).Bool("vspguiding", true).Bool("surfaceguiding", false).Bool("volumeguiding", false)
                .Bool("vspsecondaryguiding", false);
            if (mode != "sequence") ip.String("trBufferFileName", argv[6]);  // ("sequence": the App.-F options, as the default mode)
            if (mode == "trstore") ip.String("vspsamplingmethod", "resampling").Bool("storeTrBuffer", true);
            if (mode == "trload") ip.String("vspsamplingmethod", "nds").Bool("collisionProbabilityBias", true).Bool("loadTrBuffer", true);
        } else if (mode == "train" || mode == "load") {
            ip.Int("maxdepth", 5).Bool("vspguiding", true);  // surface / volume / secondary-VSP guiding default to true
            ip.Bool(mode == "train" ? "storeGuidingCache" : "loadGuidingCache", true).String("guidingCacheFileName", argv[6]);
        } else {
            ip.Int("maxdepth", 5).Bool("vspguiding", true).Bool("surfaceguiding", false).Bool("volumeguiding", false)
                .Bool("vspsecondaryguiding", false);
        }
        auto integrator = vspg::Integrator::Create("guidedvolpathvspg", ip, scene, xres, yres, spp);
        std::printf("%s\n", integrator->ToString().c_str());
        integrator->Render();
        auto *vi = static_cast<vspg::GuidedVolPathVSPGIntegrator *>(integrator.get());
        vspg::Film film = vi->GetFilm();
        film.WritePFM(out);
        if (mode == "sequence") {  // the next frame: same grid, other values; the film starts over, everything else persists
            const int n = 12;
            std::vector<float> d((size_t)n * n * n);
            for (int k = 0; k < n; ++k)
                for (int j = 0; j < n; ++j)
                    for (int i = 0; i < n; ++i) d[((size_t)k * n + j) * n + i] = (float)((i * 5 + j * 11 + k * 3) % 13) / 12.f;
            vi->SetMediumDensity(d);
            vi->ClearFilm();
            vi->Render();
            vi->GetFilm().WritePFM(argv[6]);
            d.pop_back();
            try {
                vi->SetMediumDensity(d);
                std::printf("a density of %zu values was accepted\n", d.size());
            } catch (const vspg::Error &e) {
                std::printf("refused: %s\n", e.what());
            }
            try {
                vi->SetMediumTemperature(std::vector<float>((size_t)n * n * n, 1500.f));
                std::printf("a temperature grid was accepted\n");
            } catch (const vspg::Error &e) {
                std::printf("refused: %s\n", e.what());
            }
        }
        if (mode == "rgbsequence") {  // the next frame of a coloured sequence: both sigma grids replaced, the film starts over
            vspg::RgbGridStorage f1 = rgb_frame(1);
            vi->SetMediumRgbGrids(f1);
            vi->ClearFilm();
            vi->Render();
            vi->GetFilm().WritePFM(argv[6]);
            vspg::RgbGridStorage bad;
            bad.sigma_s = f1.sigma_s;
            bad.sigma_s.pop_back();
            try {
                vi->SetMediumRgbGrids(bad);
                std::printf("a sigma_s grid of %zu values was accepted\n", bad.sigma_s.size());
            } catch (const vspg::Error &e) {
                std::printf("refused: %s\n", e.what());
            }
            bad.sigma_s.clear();
            bad.Le = f1.sigma_a;
            try {
                vi->SetMediumRgbGrids(bad);
                std::printf("an Le grid was accepted\n");
            } catch (const vspg::Error &e) {
                std::printf("refused: %s\n", e.what());
            }
        }
        VspgTrainStats ts = vi->TrainingStats();
        std::printf("guiding: training %d iterations %d regions %d/%d\n", ts.training, ts.iteration, ts.n_regions[0], ts.n_regions[1]);
        VspgCounters c = vi->Counters();
        float rgb[3];
        film.GetPixelRGB(xres / 2, yres / 2, rgb);
        std::printf("paths %llu segments %llu centre pixel %g %g %g -> %s\n", (unsigned long long)c.paths,
                    (unsigned long long)c.segments, rgb[0], rgb[1], rgb[2], out);
    } catch (const vspg::Error &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
