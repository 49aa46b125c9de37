// vspg_imgtool.cpp -- looks at and converts the image files host/vspg_image.h reads and writes (PFM, OpenEXR); no device, no HIP library.
// A small counterpart of the reference's `imgtool info` / `imgtool convert` (cmd/imgtool.cpp) for this build's two formats.
//   vspg_imgtool info FILE
//   vspg_imgtool convert IN OUT [--fp32|--fp16] [--compression none|zips|zip]
// `convert` keeps the pixel type of IN unless told otherwise (a PFM file is float32), the data and display windows and the
// samplesPerPixel / renderTimeSeconds / MSE attributes; PFM output carries the pixels only.
#include <cstdio>
#include <string>

#include "vspg_image.h"

static void usage() {
    std::fprintf(stderr, "usage: vspg_imgtool info FILE\n       vspg_imgtool convert IN OUT [--fp32|--fp16] [--compression none|zips|zip]\n");
}

int main(int argc, char **argv) {
    if (argc < 3) { usage(); return 2; }
    const std::string cmd = argv[1];
    try {
        if (cmd == "info" && argc == 3) {
            const vspg::Image img = vspg::ReadImage(argv[2]);
            std::printf("{\"xres\": %d, \"yres\": %d, \"type\": \"%s\", \"channels\": [", img.xres, img.yres, img.half ? "half" : "float");
            for (size_t i = 0; i < img.channels.size(); ++i) std::printf("%s\"%s\"", i ? ", " : "", img.channels[i].c_str());
            const int fx = img.fullX > 0 ? img.fullX : img.xres, fy = img.fullY > 0 ? img.fullY : img.yres;
            std::printf("], \"dataWindow\": [%d, %d, %d, %d], \"displayWindow\": [0, 0, %d, %d]", img.dataX0, img.dataY0, img.dataX0 + img.xres - 1,
                        img.dataY0 + img.yres - 1, fx - 1, fy - 1);
            if (img.fileCompression >= 0) std::printf(", \"compression\": %d, \"lineOrder\": %d", img.fileCompression, img.fileLineOrder);
            if (img.samplesPerPixel) std::printf(", \"samplesPerPixel\": %d", *img.samplesPerPixel);
            if (img.renderTimeSeconds) std::printf(", \"renderTimeSeconds\": %.9g", *img.renderTimeSeconds);
            if (img.MSE) std::printf(", \"MSE\": %.9g", *img.MSE);
            std::printf("}\n");
            return 0;
        }
        if (cmd == "convert" && argc >= 4) {
            vspg::ExrCompression comp = vspg::ExrCompression::Zip;
            int type = -1;  // 0 float, 1 half, -1 as the input
            for (int i = 4; i < argc; ++i) {
                const std::string a = argv[i];
                if (a == "--fp32") type = 0;
                else if (a == "--fp16") type = 1;
                else if (a == "--compression" && i + 1 < argc) {
                    const std::string v = argv[++i];
                    if (v == "none") comp = vspg::ExrCompression::None;
                    else if (v == "zips") comp = vspg::ExrCompression::Zips;
                    else if (v == "zip") comp = vspg::ExrCompression::Zip;
                    else { std::fprintf(stderr, "unknown compression %s (none, zips, zip)\n", v.c_str()); return 2; }
                } else { std::fprintf(stderr, "unknown option %s\n", a.c_str()); return 2; }
            }
            vspg::Image img = vspg::ReadImage(argv[2]);
            if (type >= 0) img.half = type == 1;
            vspg::WriteImage(img, argv[3], comp);
            return 0;
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    usage();
    return 2;
}
