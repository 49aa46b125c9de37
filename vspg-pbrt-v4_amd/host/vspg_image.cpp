// vspg_image.cpp -- PFM and OpenEXR (the subset of vspg_image.h) reading and writing
#include "vspg_image.h"

#include <zlib.h>

#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstring>
#include <new>
#include <numeric>

namespace vspg {

bool HasExtension(const std::string &fn, const char *ext) {
    const size_t n = std::strlen(ext);
    if (fn.size() < n) return false;
    for (size_t i = 0; i < n; ++i)
        if (std::tolower((unsigned char)fn[fn.size() - n + i]) != std::tolower((unsigned char)ext[i])) return false;
    return true;
}

std::vector<float> Image::Gather(const std::vector<std::string> &names, const std::string &what) const {
    std::vector<size_t> idx;
    for (const std::string &n : names) {
        const int at = ChannelIndex(n);
        if (at < 0) throw Error(what + " has no channel \"" + n + "\"");
        idx.push_back((size_t)at);
    }
    const size_t npix = (size_t)xres * (size_t)yres, nc = channels.size(), k = idx.size();
    std::vector<float> out(npix * k);
    for (size_t i = 0; i < npix; ++i)
        for (size_t c = 0; c < k; ++c) out[i * k + c] = data[i * nc + idx[c]];
    return out;
}
int Image::ChannelIndex(const std::string &name) const {
    for (size_t i = 0; i < channels.size(); ++i)
        if (channels[i] == name) return (int)i;
    return -1;
}

// ---- half ----
uint16_t FloatToHalfBits(float v) {
    uint32_t x;
    std::memcpy(&x, &v, 4);
    const uint16_t sign = (uint16_t)((x >> 16) & 0x8000u);
    const uint32_t a = x & 0x7fffffffu;
    if (a > 0x7f800000u) return sign | 0x7e00u;   // any NaN
    if (a >= 0x477ff000u) return sign | 0x7c00u;  // >= 65520 (halfway between 65504 and 2^16; the tie goes to the even 2^16): inf
    const int e = (int)(a >> 23);
    uint32_t m = a & 0x7fffffu, h, rem, halfway;
    if (e >= 113) {  // a normal half: 2^-14 and up
        h = ((uint32_t)(e - 112) << 10) | (m >> 13);
        rem = m & 0x1fffu;
        halfway = 0x1000u;
    } else {  // a subnormal half or zero: multiples of 2^-24
        if (e < 101) return sign;  // below 2^-26: nearer to 0 than to 2^-24
        m |= 0x800000u;
        const int shift = 126 - e;  // 14 .. 25
        h = m >> shift;
        rem = m & ((1u << shift) - 1u);
        halfway = 1u << (shift - 1);
    }
    if (rem > halfway || (rem == halfway && (h & 1u))) ++h;  // (a carry into the exponent is the right result)
    return sign | (uint16_t)h;
}
float HalfBitsToFloat(uint16_t hb) {
    const uint32_t sign = (uint32_t)(hb & 0x8000u) << 16;
    const uint32_t e = (hb >> 10) & 0x1fu;
    uint32_t m = hb & 0x3ffu, x;
    if (e == 0x1f) x = sign | 0x7f800000u | (m << 13);  // inf / NaN (payload kept)
    else if (e != 0) x = sign | ((e + 112) << 23) | (m << 13);
    else if (m == 0) x = sign;
    else {  // subnormal: normalise
        int k = 0;
        while (!(m & 0x400u)) { m <<= 1; ++k; }
        x = sign | ((uint32_t)(113 - k) << 23) | ((m & 0x3ffu) << 13);
    }
    float f;
    std::memcpy(&f, &x, 4);
    return f;
}

// ---- files ----
static std::vector<uint8_t> read_file(const std::string &filename) {
    std::FILE *f = std::fopen(filename.c_str(), "rb");
    if (!f) throw Error(filename + ": cannot open");
    std::vector<uint8_t> buf;
    uint8_t chunk[65536];
    size_t n;
    while ((n = std::fread(chunk, 1, sizeof chunk, f)) > 0) buf.insert(buf.end(), chunk, chunk + n);
    const bool bad = std::ferror(f) != 0;
    std::fclose(f);
    if (bad) throw Error(filename + ": read failed");
    return buf;
}
// (through a temporary file beside it and a rename: a viewer that polls a file rewritten after every wave never sees it cut short)
static void write_file(const std::string &filename, const std::vector<uint8_t> &bytes) {
    const std::string tmp = filename + ".tmp";
    std::FILE *f = std::fopen(tmp.c_str(), "wb");
    if (!f) throw Error(filename + ": cannot open for writing");
    bool ok = std::fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
    ok = std::fclose(f) == 0 && ok;
    if (ok) ok = std::rename(tmp.c_str(), filename.c_str()) == 0;
    if (!ok) {
        std::remove(tmp.c_str());
        throw Error(filename + ": write failed");
    }
}

// ---- PFM (util/image.cpp:1650-1800): "PF" | "Pf", width height, scale (< 0: little endian), float32 scan lines bottom to top ----
static Image read_pfm(const std::string &filename) {
    const std::vector<uint8_t> buf = read_file(filename);
    size_t pos = 0;
    auto token = [&]() {
        while (pos < buf.size() && std::isspace(buf[pos])) ++pos;
        std::string t;
        while (pos < buf.size() && !std::isspace(buf[pos]) && t.size() < 64) t.push_back((char)buf[pos++]);
        return t;
    };
    const std::string magic = token(), ws = token(), hs = token(), ss = token();
    Image img;
    if (magic == "PF") img.channels = {"R", "G", "B"};
    else if (magic == "Pf") img.channels = {"Y"};
    else throw Error(filename + ": not a PFM image (it begins with neither \"PF\" nor \"Pf\")");
    char *end = nullptr;
    const long w = std::strtol(ws.c_str(), &end, 10);
    const bool wok = !ws.empty() && *end == 0;
    const long h = std::strtol(hs.c_str(), &end, 10);
    const bool hok = !hs.empty() && *end == 0;
    const float scale = std::strtof(ss.c_str(), &end);
    if (!wok || !hok || ss.empty() || *end != 0 || w <= 0 || h <= 0 || w > 32768 || h > 32768 || scale == 0 || pos >= buf.size())
        throw Error(filename + ": malformed PFM header");
    ++pos;  // the single whitespace byte after the header
    const size_t nc = img.channels.size(), row = (size_t)w * nc;
    if (buf.size() - pos < row * (size_t)h * 4) throw Error(filename + ": truncated PFM image: " + std::to_string(buf.size() - pos) + " bytes of pixels, " +
                                                              std::to_string(row * (size_t)h * 4) + " expected");
    img.xres = (int)w; img.yres = (int)h;
    img.data.resize(row * (size_t)h);
    for (long y = 0; y < h; ++y) std::memcpy(&img.data[(size_t)(h - 1 - y) * row], &buf[pos + (size_t)y * row * 4], row * 4);
    if (scale > 0)  // big-endian file
        for (float &v : img.data) {
            unsigned char *b = reinterpret_cast<unsigned char *>(&v);
            std::swap(b[0], b[3]);
            std::swap(b[1], b[2]);
        }
    const float mag = scale < 0 ? -scale : scale;
    if (mag != 1.f)
        for (float &v : img.data) v *= mag;
    return img;
}
static void write_pfm(const Image &img, const std::string &filename) {
    const size_t nc = img.channels.size();
    if (nc != 1 && nc != 3) throw Error(filename + ": a PFM image has 1 or 3 channels, this one has " + std::to_string(nc));
    char head[64];
    const int hn = std::snprintf(head, sizeof head, "%s\n%d %d\n-1.000000\n", nc == 3 ? "PF" : "Pf", img.xres, img.yres);
    // a PFM pixel is R, G, B (WritePFM asks the image for those channels, image.cpp:1760): by name, or by the name's last part
    // ("Transmittance.R"), whatever order the image keeps them in
    size_t order[3] = {0, 1, 2};
    if (nc == 3)
        for (int c = 0; c < 3; ++c) {
            int at = -1;
            for (size_t k = 0; k < 3; ++k) {
                const std::string &n = img.channels[k];
                const size_t dot = n.find_last_of('.');
                if ((dot == std::string::npos ? n : n.substr(dot + 1)) == std::string(1, "RGB"[c])) at = (int)k;
            }
            if (at < 0) throw Error(filename + ": a 3-channel PFM image holds R, G, B; the image's channels are \"" + img.channels[0] + "\", \"" +
                                    img.channels[1] + "\", \"" + img.channels[2] + "\"");
            order[c] = (size_t)at;
        }
    const size_t row = (size_t)img.xres * nc;
    if (img.data.size() != row * (size_t)img.yres) throw Error(filename + ": the image holds " + std::to_string(img.data.size()) + " values, its size asks for " + std::to_string(row * (size_t)img.yres));
    std::vector<uint8_t> out((size_t)hn + row * (size_t)img.yres * 4);
    std::memcpy(out.data(), head, (size_t)hn);
    for (int y = 0; y < img.yres; ++y) {  // bottom scan line first
        uint8_t *dst = &out[(size_t)hn + (size_t)y * row * 4];
        const float *src = &img.data[(size_t)(img.yres - 1 - y) * row];
        for (size_t x = 0; x < (size_t)img.xres; ++x)
            for (size_t c = 0; c < nc; ++c) std::memcpy(dst + (x * nc + c) * 4, &src[x * nc + order[c]], 4);
    }
    write_file(filename, out);
}

// ---- OpenEXR ----
namespace {
constexpr uint8_t kExrMagic[4] = {0x76, 0x2f, 0x31, 0x01};
const char *compression_name(int c) {
    static const char *names[] = {"NONE", "RLE", "ZIPS", "ZIP", "PIZ", "PXR24", "B44", "B44A", "DWAA", "DWAB"};
    return c >= 0 && c < 10 ? names[c] : "unknown";
}
int lines_per_chunk(int compression) { return compression == (int)ExrCompression::Zip ? 16 : 1; }

// every read of the file goes through here: nothing is touched at or past `end` -- the file's length, or the end of the attribute
// value a cursor was made for -- wherever `pos` stands
struct Cursor {
    const std::vector<uint8_t> &buf;
    const std::string &filename;
    size_t pos = 0;
    size_t end = 0;  // <= buf.size()
    Cursor(const std::vector<uint8_t> &b, const std::string &fn, size_t at = 0) : buf(b), filename(fn), pos(at), end(b.size()) {}
    Cursor(const std::vector<uint8_t> &b, const std::string &fn, size_t at, size_t limit) : buf(b), filename(fn), pos(at), end(std::min(limit, b.size())) {}
    [[noreturn]] void truncated(const char *what) const {
        if (end < buf.size()) throw Error(filename + ": the " + what + " runs past its attribute's size");
        throw Error(filename + ": truncated EXR file: it ends (at " + std::to_string(buf.size()) + " bytes) inside " + what);
    }
    void need(size_t n, const char *what) const {
        if (pos > end || n > end - pos) truncated(what);
    }
    void skip(size_t n, const char *what) {
        need(n, what);
        pos += n;
    }
    int32_t i32(const char *what) {
        need(4, what);
        int32_t v;
        std::memcpy(&v, &buf[pos], 4);
        pos += 4;
        return v;
    }
    uint64_t u64(const char *what) {
        need(8, what);
        uint64_t v;
        std::memcpy(&v, &buf[pos], 8);
        pos += 8;
        return v;
    }
    uint8_t u8(const char *what) {
        need(1, what);
        return buf[pos++];
    }
    float f32(const char *what) {
        need(4, what);
        float v;
        std::memcpy(&v, &buf[pos], 4);
        pos += 4;
        return v;
    }
    std::string str(const char *what) {  // NUL-terminated, at most 255 characters
        std::string s;
        for (;;) {
            const uint8_t c = u8(what);
            if (c == 0) return s;
            if (s.size() >= 255) throw Error(filename + ": a name in the EXR " + what + " is longer than 255 characters");
            s.push_back((char)c);
        }
    }
};

struct Writer {
    std::vector<uint8_t> out;
    void bytes(const void *p, size_t n) { out.insert(out.end(), (const uint8_t *)p, (const uint8_t *)p + n); }
    void i32(int32_t v) { bytes(&v, 4); }
    void f32(float v) { bytes(&v, 4); }
    void u8(uint8_t v) { out.push_back(v); }
    void str(const std::string &s) { bytes(s.c_str(), s.size() + 1); }
    void attr(const char *name, const char *type, int32_t size) { str(name); str(type); i32(size); }
};

// the ZIP / ZIPS block transform: even bytes then odd bytes, then differences offset by 128
void zip_forward(const uint8_t *raw, size_t n, std::vector<uint8_t> &d) {
    d.resize(n);
    const size_t half = (n + 1) / 2;
    for (size_t i = 0; i < n; ++i) d[(i & 1) ? half + i / 2 : i / 2] = raw[i];
    uint8_t prev = n ? d[0] : 0;
    for (size_t i = 1; i < n; ++i) {
        const uint8_t cur = d[i];
        d[i] = (uint8_t)(cur - prev + 128);
        prev = cur;
    }
}
void zip_inverse(std::vector<uint8_t> &d, uint8_t *raw) {
    const size_t n = d.size(), half = (n + 1) / 2;
    for (size_t i = 1; i < n; ++i) d[i] = (uint8_t)(d[i - 1] + d[i] - 128);
    for (size_t i = 0; i < n; ++i) raw[i] = d[(i & 1) ? half + i / 2 : i / 2];
}
}  // namespace

static Image read_exr(const std::string &filename) {
    const std::vector<uint8_t> buf = read_file(filename);
    Cursor c(buf, filename);
    c.need(4, "the magic number");
    if (std::memcmp(buf.data(), kExrMagic, 4) != 0) throw Error(filename + ": not an OpenEXR file (wrong magic number)");
    c.pos = 4;
    const int32_t version = c.i32("the version field");
    if ((version & 0xff) != 2) throw Error(filename + ": EXR file format version " + std::to_string(version & 0xff) + ", only version 2 is read");
    if (version & 0x200) throw Error(filename + ": tiled EXR files are not supported (scan-line files only)");
    if (version & 0x800) throw Error(filename + ": deep EXR files are not supported");
    if (version & 0x1000) throw Error(filename + ": multi-part EXR files are not supported");
    if (version & ~0x4ff) throw Error(filename + ": unknown EXR version flags " + std::to_string(version & ~0x4ff));

    Image img;
    std::vector<int> types;
    int compression = -1, lineOrder = -1;
    int dw[4], disp[4];
    bool haveDw = false, haveDisp = false, haveChannels = false;
    for (;;) {
        const std::string name = c.str("header");
        if (name.empty()) break;
        const std::string type = c.str("header");
        const int32_t size = c.i32("header");
        if (size < 0) throw Error(filename + ": attribute \"" + name + "\" has the negative size " + std::to_string(size));
        c.need((size_t)size, "the header");
        const size_t endPos = c.pos + (size_t)size;
        auto expect = [&](const char *t, int32_t n) {
            if (type != t || (n >= 0 && size != n))
                throw Error(filename + ": attribute \"" + name + "\" is a " + type + " of " + std::to_string(size) + " bytes, expected " + t);
        };
        if (name == "channels") {
            expect("chlist", -1);
            Cursor cc(buf, filename, c.pos, endPos);  // (bounded by the attribute's own size, not by the file's)
            for (;;) {
                const std::string ch = cc.str("channel list");
                if (ch.empty()) break;
                const int32_t t = cc.i32("channel list");
                cc.skip(4, "channel list");  // pLinear, reserved
                const int32_t xs = cc.i32("channel list"), ys = cc.i32("channel list");
                if (t == 0) throw Error(filename + ": channel \"" + ch + "\" is UINT; only HALF and FLOAT channels are supported");
                if (t != 1 && t != 2) throw Error(filename + ": channel \"" + ch + "\" has the unknown pixel type " + std::to_string(t));
                if (xs != 1 || ys != 1) throw Error(filename + ": channel \"" + ch + "\" is sub-sampled (" + std::to_string(xs) + " x " + std::to_string(ys) + "); only 1 x 1 is supported");
                img.channels.push_back(ch);
                types.push_back(t);
            }
            haveChannels = true;
        } else if (name == "compression") {
            expect("compression", 1);
            compression = buf[c.pos];
        } else if (name == "lineOrder") {
            expect("lineOrder", 1);
            lineOrder = buf[c.pos];
        } else if (name == "dataWindow" || name == "displayWindow") {
            expect("box2i", 16);
            std::memcpy(name == "dataWindow" ? dw : disp, &buf[c.pos], 16);
            (name == "dataWindow" ? haveDw : haveDisp) = true;
        } else if (name == "samplesPerPixel" && type == "int" && size == 4) {
            int32_t v;
            std::memcpy(&v, &buf[c.pos], 4);
            img.samplesPerPixel = v;
        } else if ((name == "renderTimeSeconds" || name == "MSE") && type == "float" && size == 4) {
            float v;
            std::memcpy(&v, &buf[c.pos], 4);
            (name == "MSE" ? img.MSE : img.renderTimeSeconds) = v;
        }  // (anything else is skipped by its size)
        c.pos = endPos;
    }
    if (!haveChannels || !haveDw || !haveDisp || compression < 0 || lineOrder < 0)
        throw Error(filename + ": the EXR header lacks a required attribute (channels, compression, dataWindow, displayWindow, lineOrder)");
    if (compression != 0 && compression != 2 && compression != 3)
        throw Error(filename + ": " + compression_name(compression) + " compression (" + std::to_string(compression) + ") is not supported; NONE, ZIPS and ZIP are");
    if (lineOrder != 0 && lineOrder != 1) throw Error(filename + ": line order " + std::to_string(lineOrder) + " is not supported (INCREASING_Y and DECREASING_Y are)");
    if (img.channels.empty()) throw Error(filename + ": the EXR file has no channels");
    if (img.channels.size() > 64) throw Error(filename + ": " + std::to_string(img.channels.size()) + " channels; at most 64 are read");
    for (int t : types)
        if (t != types[0]) throw Error(filename + ": mixed channel types (HALF and FLOAT); all channels must have one type");
    img.half = types[0] == 1;
    const int64_t w = (int64_t)dw[2] - dw[0] + 1, h = (int64_t)dw[3] - dw[1] + 1;
    if (w <= 0 || h <= 0 || w > 32768 || h > 32768)
        throw Error(filename + ": data window (" + std::to_string(dw[0]) + "," + std::to_string(dw[1]) + ")-(" + std::to_string(dw[2]) + "," + std::to_string(dw[3]) + ") is empty or larger than 32768");
    const int64_t fw = (int64_t)disp[2] - disp[0] + 1, fh = (int64_t)disp[3] - disp[1] + 1;
    img.xres = (int)w; img.yres = (int)h;
    img.dataX0 = dw[0] - disp[0]; img.dataY0 = dw[1] - disp[1];
    img.fullX = fw > 0 && fw <= 0x7fffffff ? (int)fw : 0;
    img.fullY = fh > 0 && fh <= 0x7fffffff ? (int)fh : 0;
    img.fileCompression = compression; img.fileLineOrder = lineOrder;

    const size_t nc = img.channels.size(), bps = img.half ? 2 : 4;
    const size_t rowBytes = (size_t)w * nc * bps;
    const int L = lines_per_chunk(compression);
    const size_t nChunks = (size_t)((h + L - 1) / L);
    if (nChunks * 8 > buf.size() - c.pos) c.truncated("the chunk offset table");
    std::vector<uint64_t> offsets(nChunks);
    for (uint64_t &o : offsets) o = c.u64("the chunk offset table");
    // The pixel allocation is bounded by what the file could hold, not by its claims: exactly for NONE, and for ZIP / ZIPS by
    // deflate's ceiling of 1032 bytes out per byte in (zlib's technical notes), before any chunk is looked at.
    {
        const uint64_t rest = buf.size() - c.pos, rawTotal = (uint64_t)rowBytes * (uint64_t)h;
        const uint64_t most = compression == 0 ? rest : rest * 1032u;
        if (rawTotal > most)
            throw Error(filename + ": the data window asks for " + std::to_string(rawTotal) + " bytes of pixels, the " + std::to_string(rest) +
                        " bytes of chunks in the file can hold at most " + std::to_string(most));
    }
    img.data.resize((size_t)w * (size_t)h * nc);
    std::vector<uint8_t> seen(nChunks, 0), raw, d;
    for (size_t k = 0; k < nChunks; ++k) {
        const uint64_t off = offsets[k];
        if (off > buf.size() || buf.size() - off < 8)
            throw Error(filename + ": chunk " + std::to_string(k) + " is at offset " + std::to_string(off) + ", outside the file of " + std::to_string(buf.size()) + " bytes");
        Cursor cc(buf, filename, (size_t)off);
        const int32_t y = cc.i32("a chunk header"), dataSize = cc.i32("a chunk header");
        const int64_t rel = (int64_t)y - dw[1];
        if (rel < 0 || rel >= h || rel % L != 0) throw Error(filename + ": chunk " + std::to_string(k) + " starts at scan line " + std::to_string(y) + ", which begins no block of the data window");
        const size_t block = (size_t)(rel / L);
        if (seen[block]) throw Error(filename + ": two chunks hold scan line " + std::to_string(y));
        seen[block] = 1;
        const size_t lines = (size_t)std::min<int64_t>(L, h - rel), rawSize = lines * rowBytes;
        if (dataSize < 0 || (size_t)dataSize > buf.size() - cc.pos)
            throw Error(filename + ": chunk " + std::to_string(k) + " claims " + std::to_string(dataSize) + " bytes at offset " + std::to_string(cc.pos) + ", past the end of the file of " + std::to_string(buf.size()) + " bytes");
        const uint8_t *src = &buf[cc.pos];
        if ((size_t)dataSize != rawSize) {
            if (compression == 0 || (size_t)dataSize > rawSize)
                throw Error(filename + ": chunk " + std::to_string(k) + " holds " + std::to_string(dataSize) + " bytes, its scan lines take " + std::to_string(rawSize));
            d.resize(rawSize);
            uLongf got = (uLongf)rawSize;
            const int zr = uncompress(d.data(), &got, src, (uLong)dataSize);
            if (zr != Z_OK || got != rawSize)
                throw Error(filename + ": chunk " + std::to_string(k) + " does not inflate to its " + std::to_string(rawSize) + " bytes (zlib " + std::to_string(zr) + ", " + std::to_string(got) + " bytes)");
            raw.resize(rawSize);
            zip_inverse(d, raw.data());
            src = raw.data();
        }
        for (size_t l = 0; l < lines; ++l) {
            float *dst = &img.data[((size_t)rel + l) * (size_t)w * nc];
            for (size_t ch = 0; ch < nc; ++ch) {
                const uint8_t *plane = src + l * rowBytes + ch * (size_t)w * bps;
                for (size_t x = 0; x < (size_t)w; ++x) {
                    if (img.half) {
                        uint16_t hb;
                        std::memcpy(&hb, plane + x * 2, 2);
                        dst[x * nc + ch] = HalfBitsToFloat(hb);
                    } else {
                        std::memcpy(&dst[x * nc + ch], plane + x * 4, 4);
                    }
                }
            }
        }
    }
    return img;
}

void WriteExrScanlines(const Image &meta, bool half, const void *scanlines, const std::string &filename, ExrCompression compression) {
    const int w = meta.xres, h = meta.yres;
    if (w <= 0 || h <= 0 || meta.channels.empty()) throw Error(filename + ": an empty image cannot be written");
    std::vector<std::string> names = meta.channels;
    std::sort(names.begin(), names.end());
    const int fullX = meta.fullX > 0 ? meta.fullX : w, fullY = meta.fullY > 0 ? meta.fullY : h;
    Writer wr;
    wr.bytes(kExrMagic, 4);
    wr.i32(2);
    // (attributes in name order, as a header kept in a map writes them)
    if (meta.MSE) { wr.attr("MSE", "float", 4); wr.f32(*meta.MSE); }
    int32_t chSize = 1;
    for (const std::string &n : names) chSize += (int32_t)n.size() + 1 + 16;
    wr.attr("channels", "chlist", chSize);
    for (const std::string &n : names) {
        wr.str(n);
        wr.i32(half ? 1 : 2);
        wr.i32(0);  // pLinear and three reserved bytes
        wr.i32(1);
        wr.i32(1);
    }
    wr.u8(0);
    wr.attr("compression", "compression", 1);
    wr.u8((uint8_t)compression);
    wr.attr("dataWindow", "box2i", 16);
    wr.i32(meta.dataX0); wr.i32(meta.dataY0); wr.i32(meta.dataX0 + w - 1); wr.i32(meta.dataY0 + h - 1);
    wr.attr("displayWindow", "box2i", 16);
    wr.i32(0); wr.i32(0); wr.i32(fullX - 1); wr.i32(fullY - 1);
    wr.attr("lineOrder", "lineOrder", 1);
    wr.u8(0);
    wr.attr("pixelAspectRatio", "float", 4);
    wr.f32(1.f);
    if (meta.renderTimeSeconds) { wr.attr("renderTimeSeconds", "float", 4); wr.f32(*meta.renderTimeSeconds); }
    if (meta.samplesPerPixel) { wr.attr("samplesPerPixel", "int", 4); wr.i32(*meta.samplesPerPixel); }
    wr.attr("screenWindowCenter", "v2f", 8);
    wr.f32(0.f); wr.f32(0.f);
    wr.attr("screenWindowWidth", "float", 4);
    wr.f32(1.f);
    wr.u8(0);

    const size_t rowBytes = (size_t)w * names.size() * (half ? 2 : 4);
    const int L = lines_per_chunk((int)compression);
    const size_t nChunks = ((size_t)h + L - 1) / L;
    const size_t tablePos = wr.out.size();
    wr.out.resize(tablePos + nChunks * 8);
    std::vector<uint8_t> d, z;
    const uint8_t *src = static_cast<const uint8_t *>(scanlines);
    for (size_t k = 0; k < nChunks; ++k) {
        const uint64_t off = wr.out.size();
        std::memcpy(&wr.out[tablePos + k * 8], &off, 8);
        const size_t first = k * L, lines = std::min<size_t>(L, (size_t)h - first), rawSize = lines * rowBytes;
        const uint8_t *raw = src + first * rowBytes;
        wr.i32(meta.dataY0 + (int32_t)first);
        if (compression != ExrCompression::None) {
            zip_forward(raw, rawSize, d);
            uLongf zn = compressBound((uLong)rawSize);
            z.resize(zn);
            if (compress2(z.data(), &zn, d.data(), (uLong)rawSize, Z_DEFAULT_COMPRESSION) != Z_OK) throw Error(filename + ": zlib failed to compress a block");
            if (zn < rawSize) {
                wr.i32((int32_t)zn);
                wr.bytes(z.data(), zn);
                continue;
            }
        }
        wr.i32((int32_t)rawSize);  // (NONE, or a block that does not shrink: stored as it is)
        wr.bytes(raw, rawSize);
    }
    write_file(filename, wr.out);
}

static void write_exr(const Image &img, const std::string &filename, ExrCompression compression) {
    const size_t nc = img.channels.size(), w = (size_t)img.xres, h = (size_t)img.yres;
    if (img.data.size() != w * h * nc) throw Error(filename + ": the image holds " + std::to_string(img.data.size()) + " values, its size asks for " + std::to_string(w * h * nc));
    std::vector<size_t> order(nc);  // the channels in name order
    std::iota(order.begin(), order.end(), (size_t)0);
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return img.channels[a] < img.channels[b]; });
    const size_t bps = img.half ? 2 : 4;
    std::vector<uint8_t> lines(w * h * nc * bps);
    for (size_t y = 0; y < h; ++y)
        for (size_t k = 0; k < nc; ++k) {
            uint8_t *plane = &lines[(y * nc + k) * w * bps];
            const float *srcp = &img.data[y * w * nc + order[k]];
            for (size_t x = 0; x < w; ++x) {
                if (img.half) {
                    const uint16_t hb = FloatToHalfBits(srcp[x * nc]);
                    std::memcpy(plane + x * 2, &hb, 2);
                } else {
                    std::memcpy(plane + x * 4, &srcp[x * nc], 4);
                }
            }
        }
    WriteExrScanlines(img, img.half, lines.data(), filename, compression);
}

Image ReadImage(const std::string &filename) {
    try {
        if (HasExtension(filename, ".pfm")) return read_pfm(filename);
        if (HasExtension(filename, ".exr")) return read_exr(filename);
    } catch (const std::bad_alloc &) {
        throw Error(filename + ": not enough memory for the image the file describes");
    }
    throw Error(filename + ": no reader for this file's extension (.pfm and .exr are read)");
}
void WriteImage(const Image &image, const std::string &filename, ExrCompression compression) {
    if (HasExtension(filename, ".pfm")) return write_pfm(image, filename);
    if (HasExtension(filename, ".exr")) return write_exr(image, filename, compression);
    throw Error(filename + ": no writer for this file's extension (.pfm and .exr are written)");
}

}  // namespace vspg
