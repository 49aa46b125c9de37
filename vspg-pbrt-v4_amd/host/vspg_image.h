// vspg_image.h -- the host's Image layer: pbrt's Image::Read / Image::Write by file extension (src/pbrt/util/image.cpp:1006-1054),
// for the two formats this build covers: PFM (:1756-1800, :1650-1754) and OpenEXR (:1056-1247).  Plain C++17 + zlib, no device.
//
// The OpenEXR library itself is not part of this build; the codec below covers the part of the container the reference reads and
// writes for this integrator (all little endian):
//   magic 76 2f 31 01, version 2 (long names accepted; tiled, deep and multi-part files refused), single-part scan-line files;
//   channels all HALF or all FLOAT with xSampling = ySampling = 1 (ReadEXR's own restriction, image.cpp:1143-1158), sorted by name;
//   compression NONE, ZIPS (1 scan line per chunk) and ZIP (16 per chunk; Imf::Header's default, so what the reference writes);
//   line order INCREASING_Y written, either read; dataWindow = the pixel bounds, displayWindow = the full resolution (:1179-1196);
//   the eight required attributes plus samplesPerPixel (int), renderTimeSeconds (float), MSE (float) when set (:1204-1225).
// NOT written: worldToCamera, worldToNDC (the camera matrices) and chromaticities.  NOT covered: RLE, PIZ, PXR24, B44, B44A, DWAA, DWAB,
// tiled, multi-part and deep files, UINT or mixed channel types, sub-sampled channels: reading one is an Error that names the file and
// what was met.  Unknown attributes are skipped by their size.  A truncated file, or an offset table or chunk size that points outside
// the file, is an Error too: every read is checked against the file's length (inside an attribute's value: against the attribute's
// size), and the pixel allocation against what the file's bytes could hold.
#pragma once
#include <cstdint>
#include <optional>
#include <string>
#include <vector>

#include "vspg_host.h"

namespace vspg {

enum class ExrCompression { None = 0, Zips = 2, Zip = 3 };

struct Image {
    int xres = 0, yres = 0;               // the size of the pixel data (the data window)
    bool half = false;                    // the file's pixel type: HALF (true) or FLOAT; `data` is float either way (widened exactly)
    std::vector<std::string> channels;    // PFM: "R","G","B" or "Y"; EXR: the file's names, in the file's (sorted) order
    std::vector<float> data;              // xres * yres * channels.size(), interleaved, rows top first
    // metadata (ImageMetadata, util/image.h:95-112)
    int dataX0 = 0, dataY0 = 0;           // pixelBounds.pMin: where the data sits in the full image
    int fullX = 0, fullY = 0;             // fullResolution; 0 = the data is the full image
    std::optional<int> samplesPerPixel;
    std::optional<float> renderTimeSeconds, MSE;
    // what an EXR file was stored with (-1: not an EXR file); ignored when writing
    int fileCompression = -1, fileLineOrder = -1;

    int NChannels() const { return (int)channels.size(); }
    int ChannelIndex(const std::string &name) const;  // -1 if absent
    // the named channels, interleaved in the order asked for; a missing one is an Error "<what> has no channel "<name>""
    std::vector<float> Gather(const std::vector<std::string> &names, const std::string &what) const;
};

Image ReadImage(const std::string &filename);  // by extension: .pfm (1 or 3 channels), .exr
// by extension: .pfm (1 or 3 channels, float32 whatever `half` says), .exr (HALF or FLOAT by `half`)
void WriteImage(const Image &image, const std::string &filename, ExrCompression compression = ExrCompression::Zip);

// An EXR file from pixel values that already are its scan-line payload: per row the samples of each channel in NAME order, one
// channel after the other (for "B","G","R": VSPG_RESOLVE_SCANLINE_BGR of vspg_film_resolve), 2 bytes per sample if `half`, else 4.
// `meta` gives xres, yres, channels (any order; they are sorted) and the metadata; its `data` is not looked at.
void WriteExrScanlines(const Image &meta, bool half, const void *scanlines, const std::string &filename,
                       ExrCompression compression = ExrCompression::Zip);

// Half(float) / operator float of util/float.h:417-463: round to nearest even, subnormal halves, >= 65520 to +-inf,
// any NaN to 0x7e00 | sign; the widening is exact.
uint16_t FloatToHalfBits(float v);
float HalfBitsToFloat(uint16_t h);

bool HasExtension(const std::string &filename, const char *ext /* ".exr" */);  // case-insensitive

}  // namespace vspg
