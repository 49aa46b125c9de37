#include "vspg_host.h"
#include "vspg_image.h"
#include "vspg_nanovdb.h"

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <chrono>
#include <cstring>
#include <fstream>

namespace vspg {

// ---------------------------------------------------------------------------------------
ParameterDictionary &ParameterDictionary::Int(const std::string &n, int v) { Value x; x.type = 'i'; x.i = v; values[n] = x; return *this; }
ParameterDictionary &ParameterDictionary::Float(const std::string &n, float v) { Value x; x.type = 'f'; x.f[0] = v; values[n] = x; return *this; }
ParameterDictionary &ParameterDictionary::Bool(const std::string &n, bool v) { Value x; x.type = 'b'; x.i = v; values[n] = x; return *this; }
ParameterDictionary &ParameterDictionary::String(const std::string &n, const std::string &v) { Value x; x.type = 's'; x.s = v; values[n] = x; return *this; }
ParameterDictionary &ParameterDictionary::RGB(const std::string &n, float r, float g, float b) { Value x; x.type = 'c'; x.f[0] = r; x.f[1] = g; x.f[2] = b; values[n] = x; return *this; }

ParameterDictionary &ParameterDictionary::Point3(const std::string &n, float x, float y, float z) { Value v; v.type = 'p'; v.f[0] = x; v.f[1] = y; v.f[2] = z; values[n] = v; return *this; }
ParameterDictionary &ParameterDictionary::IntArray(const std::string &n, std::vector<int> a) { Value v; v.type = 'I'; v.iarr = std::move(a); values[n] = v; return *this; }
ParameterDictionary &ParameterDictionary::Point3Array(const std::string &n, std::vector<float> a) { Value v; v.type = 'P'; v.arr = std::move(a); values[n] = v; return *this; }
ParameterDictionary &ParameterDictionary::RGBArray(const std::string &n, std::vector<float> a) { Value v; v.type = 'C'; v.arr = std::move(a); values[n] = v; return *this; }
ParameterDictionary &ParameterDictionary::FloatArray(const std::string &n, std::vector<float> a) { Value v; v.type = 'a'; v.arr = std::move(a); values[n] = v; return *this; }

ParameterDictionary ParameterDictionary::Parse(const std::string &text) {
    ParameterDictionary d;
    size_t i = 0;
    const size_t n = text.size();
    auto skip = [&] {
        while (i < n) {
            if (std::isspace((unsigned char)text[i])) ++i;
            else if (text[i] == '#') { while (i < n && text[i] != '\n') ++i; }
            else break;
        }
    };
    auto quoted = [&]() -> std::string {
        if (i >= n || text[i] != '"') throw Error("parameter list: expected a quoted string at offset " + std::to_string(i));
        size_t j = text.find('"', i + 1);
        if (j == std::string::npos) throw Error("parameter list: unterminated string");
        std::string r = text.substr(i + 1, j - i - 1);
        i = j + 1;
        return r;
    };
    for (skip(); i < n; skip()) {
        const std::string decl = quoted();
        const size_t sp = decl.find_first_of(" \t");
        if (sp == std::string::npos) throw Error("parameter list: \"" + decl + "\" is not \"type name\"");
        const std::string type = decl.substr(0, sp), name = decl.substr(decl.find_first_not_of(" \t", sp));
        skip();
        const bool bracket = i < n && text[i] == '[';
        if (bracket) ++i;
        std::vector<std::string> toks;
        while (true) {
            skip();
            if (i >= n) { if (bracket) throw Error("parameter list: missing ]"); break; }
            if (text[i] == ']') { if (!bracket) throw Error("parameter list: stray ]"); ++i; break; }
            if (text[i] == '"') {
                if (!bracket && !toks.empty()) break;  // next declaration
                toks.push_back(quoted());
            } else {
                size_t j = i;
                while (j < n && !std::isspace((unsigned char)text[j]) && text[j] != ']' && text[j] != '"') ++j;
                toks.push_back(text.substr(i, j - i));
                i = j;
            }
            if (!bracket) break;
        }
        if (toks.empty()) throw Error("parameter \"" + name + "\" has no value");
        auto num = [&](const std::string &t) -> float {
            char *end = nullptr;
            float v = std::strtof(t.c_str(), &end);
            if (end == t.c_str() || *end) throw Error("parameter \"" + name + "\": \"" + t + "\" is not a number");
            return v;
        };
        if (type == "integer") {
            if (toks.size() == 1) d.Int(name, (int)std::strtol(toks[0].c_str(), nullptr, 10));
            else { std::vector<int> a; for (auto &t : toks) a.push_back((int)std::strtol(t.c_str(), nullptr, 10)); d.IntArray(name, std::move(a)); }
        } else if (type == "float") {
            if (toks.size() == 1) d.Float(name, num(toks[0]));
            else { std::vector<float> a; for (auto &t : toks) a.push_back(num(t)); d.FloatArray(name, std::move(a)); }
        } else if (type == "bool") {
            if (toks[0] != "true" && toks[0] != "false") throw Error("parameter \"" + name + "\": bool must be true or false");
            d.Bool(name, toks[0] == "true");
        } else if (type == "string") {
            d.String(name, toks[0]);
        } else if (type == "texture") {  // a named texture bound to a parameter: kept as a string under "texture <name>"
            d.String("texture " + name, toks[0]);
        } else if (type == "point3" && toks.size() > 3) {
            if (toks.size() % 3) throw Error("parameter \"" + name + "\": point3 values come in threes");
            std::vector<float> a; for (auto &t : toks) a.push_back(num(t));
            d.Point3Array(name, std::move(a));
        } else if (type == "rgb" && toks.size() > 3) {
            if (toks.size() % 3) throw Error("parameter \"" + name + "\": rgb values come in threes");
            std::vector<float> a; for (auto &t : toks) a.push_back(num(t));
            d.RGBArray(name, std::move(a));
        } else if (type == "rgb" || type == "point3") {
            if (toks.size() != 3) throw Error("parameter \"" + name + "\": " + type + " needs three values");
            if (type == "rgb") d.RGB(name, num(toks[0]), num(toks[1]), num(toks[2]));
            else d.Point3(name, num(toks[0]), num(toks[1]), num(toks[2]));
        } else if (type == "point2" || type == "vector3" || type == "normal3" || type == "normal" || type == "vector2") {
            std::vector<float> a; for (auto &t : toks) a.push_back(num(t));
            d.FloatArray(name, std::move(a));
        } else
            throw Error("parameter \"" + name + "\": type \"" + type + "\" is outside this build's scope");
    }
    return d;
}

const ParameterDictionary::Value *ParameterDictionary::find(const std::string &n, char type) const {
    auto it = values.find(n);
    if (it == values.end()) return nullptr;
    if (it->second.type != type)
        throw Error("parameter \"" + n + "\" has the wrong type");
    it->second.lookedUp = true;
    return &it->second;
}
int ParameterDictionary::GetOneInt(const std::string &n, int def) const { auto v = find(n, 'i'); return v ? v->i : def; }
float ParameterDictionary::GetOneFloat(const std::string &n, float def) const { auto v = find(n, 'f'); return v ? v->f[0] : def; }
bool ParameterDictionary::GetOneBool(const std::string &n, bool def) const { auto v = find(n, 'b'); return v ? v->i != 0 : def; }
std::string ParameterDictionary::GetOneString(const std::string &n, const std::string &def) const { auto v = find(n, 's'); return v ? v->s : def; }
bool ParameterDictionary::GetOneRGB(const std::string &n, float rgb[3]) const {
    auto v = find(n, 'c');
    if (!v) return false;
    rgb[0] = v->f[0]; rgb[1] = v->f[1]; rgb[2] = v->f[2];
    return true;
}
bool ParameterDictionary::GetOnePoint3(const std::string &n, float p[3]) const {
    auto v = find(n, 'p');
    if (!v) return false;
    p[0] = v->f[0]; p[1] = v->f[1]; p[2] = v->f[2];
    return true;
}
std::vector<float> ParameterDictionary::GetFloatArray(const std::string &n) const {
    auto it = values.find(n);
    if (it == values.end()) return {};
    if (it->second.type == 'f') { it->second.lookedUp = true; return {it->second.f[0]}; }
    auto v = find(n, 'a');
    return v->arr;
}
std::vector<int> ParameterDictionary::GetIntArray(const std::string &n) const {
    auto it = values.find(n);
    if (it == values.end()) return {};
    if (it->second.type == 'i') { it->second.lookedUp = true; return {it->second.i}; }
    auto v = find(n, 'I');
    return v->iarr;
}
std::vector<float> ParameterDictionary::GetPoint3Array(const std::string &n) const {
    auto it = values.find(n);
    if (it == values.end()) return {};
    if (it->second.type == 'p') { it->second.lookedUp = true; return {it->second.f[0], it->second.f[1], it->second.f[2]}; }
    auto v = find(n, 'P');
    return v->arr;
}
std::vector<float> ParameterDictionary::GetRGBArray(const std::string &n) const {
    auto it = values.find(n);
    if (it == values.end()) return {};
    if (it->second.type == 'c') { it->second.lookedUp = true; return {it->second.f[0], it->second.f[1], it->second.f[2]}; }
    auto v = find(n, 'C');
    return v->arr;
}
void ParameterDictionary::ReportUnused() const {
    for (const auto &kv : values)
        if (!kv.second.lookedUp) throw Error("\"" + kv.first + "\": unused parameter.");
}

// ---------------------------------------------------------------------------------------
static VspgMedium CreateGridMedium(const ParameterDictionary &p, std::vector<float> *densityStorage, std::vector<float> *leScaleStorage,
                                   std::vector<float> *temperatureStorage) {
    // GridMedium::Create (media.cpp:272-361)
    VspgMedium m;
    std::memset(&m, 0, sizeof m);
    std::vector<float> density = p.GetFloatArray("density");
    std::vector<float> temperature = p.GetFloatArray("temperature");
    if (density.empty()) throw Error("No \"density\" value provided for grid medium.");
    if (!temperature.empty() && temperature.size() != density.size())
        throw Error("Different number of samples (" + std::to_string(density.size()) + " vs " + std::to_string(temperature.size()) +
                    ") provided for \"density\" and \"temperature\".");
    const int nx = p.GetOneInt("nx", 1), ny = p.GetOneInt("ny", 1), nz = p.GetOneInt("nz", 1);
    if ((long long)density.size() != (long long)nx * ny * nz)
        throw Error("Grid medium has " + std::to_string(density.size()) + " density values; expected nx*ny*nz = " +
                    std::to_string((long long)nx * ny * nz));
    // emission (media.cpp:306-328): in RGB rendering mode SpectrumToPhotometric() is 1 (util/spectrum.cpp:48-49), so LeNorm = 1
    float le[3] = {0.f, 0.f, 0.f};
    const bool hasLe = p.GetOneRGB("Le", le);
    std::vector<float> leScale = p.GetFloatArray("Lescale");
    if (hasLe && !temperature.empty()) throw Error("Both \"Le\" and \"temperature\" values were provided.");
    // isEmissive = temperatureGrid ? true : Le_spec.MaxValue() > 0 (media.cpp:261); Le.MaxValue() == 0 -> ConstantSpectrum(0)
    const bool emissive = !temperature.empty() || (hasLe && (le[0] > 0 || le[1] > 0 || le[2] > 0));
    if (!temperature.empty() && !temperatureStorage)
        throw Error("CreateMedium(\"uniformgrid\") with \"temperature\" needs a temperatureStorage vector to own the grid");
    const float temperatureOffset = p.GetOneFloat("temperatureoffset", p.GetOneFloat("temperaturecutoff", 0.f));
    const float temperatureScale = p.GetOneFloat("temperaturescale", 1.f);
    if (!leScale.empty() && (long long)leScale.size() != (long long)nx * ny * nz)
        throw Error("Expected " + std::to_string(nx) + " x " + std::to_string(ny) + " " + std::to_string(nz) + " = " +
                    std::to_string((long long)nx * ny * nz) + " values for \"Lescale\" but were given " + std::to_string(leScale.size()) + ".");
    if (emissive && !leScale.empty() && !leScaleStorage)
        throw Error("CreateMedium(\"uniformgrid\") with \"Lescale\" needs a leScaleStorage vector to own the grid");
    float p0[3] = {0.f, 0.f, 0.f}, p1[3] = {1.f, 1.f, 1.f};
    p.GetOnePoint3("p0", p0);
    p.GetOnePoint3("p1", p1);
    const float g = p.GetOneFloat("g", 0.f);
    if (!p.GetOneString("preset", "").empty()) throw Error("medium \"preset\" tables are outside this build's scope");
    float sa[3] = {1.f, 1.f, 1.f}, ss[3] = {1.f, 1.f, 1.f};
    p.GetOneRGB("sigma_a", sa);
    p.GetOneRGB("sigma_s", ss);
    const float sigmaScale = p.GetOneFloat("scale", 1.f);
    p.ReportUnused();
    if (!densityStorage) throw Error("CreateMedium(\"uniformgrid\") needs a densityStorage vector to own the grid");
    *densityStorage = std::move(density);
    m.type = VSPG_MEDIUM_GRID;
    for (int i = 0; i < 3; ++i) {
        m.sigma_a[i] = sa[i] * sigmaScale;
        m.sigma_s[i] = ss[i] * sigmaScale;
        m.bounds_min[i] = p0[i];
        m.bounds_max[i] = p1[i];
    }
    m.g = g;
    m.nx = nx; m.ny = ny; m.nz = nz;
    m.density = densityStorage->data();
    if (emissive) {
        for (int i = 0; i < 3; ++i) m.Le[i] = le[i];
        if (!leScale.empty()) {  // LeScale[i] *= LeNorm (= 1)
            *leScaleStorage = std::move(leScale);
            m.le_scale = leScaleStorage->data();
            m.le_nx = nx; m.le_ny = ny; m.le_nz = nz;
        }  // else: the library builds the reference's 1x1x1 grid {LeNorm}
    }
    if (!temperature.empty()) {  // media.h:333-341: Le = LeScale.Lookup(p) * BlackbodySpectrum((T(p) - offset) * scale).Sample(lambda)
        *temperatureStorage = std::move(temperature);
        m.temperature = temperatureStorage->data();
        m.temperature_offset = temperatureOffset;
        m.temperature_scale = temperatureScale;
    }
    return m;
}

static VspgMedium CreateNanoVdbMedium(const ParameterDictionary &p, std::vector<float> *densityStorage, std::vector<float> *temperatureStorage) {
    // NanoVDBMedium::Create (media.cpp:683-734); the grid file through vspg_nanovdb.h (layout as understood there: unpinned)
    VspgMedium m;
    std::memset(&m, 0, sizeof m);
    const std::string filename = p.GetOneString("filename", "");
    if (filename.empty()) throw Error("Must supply \"filename\" to \"nanovdb\" medium.");
    const std::string gridname = p.GetOneString("gridname", "density");
    const std::string temperaturename = p.GetOneString("temperaturename", "temperature");
    NanoVdbFloatGrid dg, tg;
    if (!ReadNanoVdbFloatGrid(filename, gridname, &dg)) throw Error(filename + ": didn't find \"" + gridname + "\" grid.");
    const bool haveT = ReadNanoVdbFloatGrid(filename, temperaturename, &tg);
    const float LeScale = p.GetOneFloat("Lescale", 1.f);
    const float temperatureOffset = p.GetOneFloat("temperatureoffset", p.GetOneFloat("temperaturecutoff", 0.f));
    const float temperatureScale = p.GetOneFloat("temperaturescale", 1.f);
    const float densityOffset = p.GetOneFloat("densityoffset", 0.f);
    const float majorantScale = p.GetOneFloat("majorantscale", 1.f);
    const float g = p.GetOneFloat("g", 0.f);
    float sa[3] = {1.f, 1.f, 1.f}, ss[3] = {1.f, 1.f, 1.f};
    p.GetOneRGB("sigma_a", sa);
    p.GetOneRGB("sigma_s", ss);
    const float sigmaScale = p.GetOneFloat("scale", 1.f);
    p.ReportUnused();
    if (!densityStorage) throw Error("CreateMedium(\"nanovdb\") needs a densityStorage vector to own the grid");
    // indexToWorld must be a scale and a translation: worldToIndexF(p) = (p - grid_origin) / voxel_size is what the device evaluates
    // (a rotated grid goes in through the medium's own transform: MakeNamedMedium under the CTM)
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            if (i != j && std::fabs(dg.mat[3 * i + j]) > 1e-12 * (std::fabs(dg.mat[0]) + std::fabs(dg.mat[4]) + std::fabs(dg.mat[8])))
                throw Error(filename + ": grid \"" + gridname + "\" has a rotated / sheared index-to-world map; only scale + translation is read");
    m.type = VSPG_MEDIUM_NANOVDB;
    for (int i = 0; i < 3; ++i) {
        m.sigma_a[i] = sa[i] * sigmaScale;
        m.sigma_s[i] = ss[i] * sigmaScale;
        m.bounds_min[i] = (float)dg.worldMin[i];
        m.bounds_max[i] = (float)dg.worldMax[i];
        m.index_min[i] = dg.indexMin[i];
        m.voxel_size[i] = (float)dg.mat[4 * i];
        m.grid_origin[i] = (float)dg.vec[i];
    }
    m.g = g;
    m.nx = dg.dim[0]; m.ny = dg.dim[1]; m.nz = dg.dim[2];
    m.density_offset = densityOffset;
    m.majorant_scale = majorantScale;
    *densityStorage = std::move(dg.dense);
    m.density = densityStorage->data();
    if (haveT) {  // NanoVDBMedium's temperature grid (media.h:724-735): blackbody emission under "vspsamplingmethod" "nds" (include/vspg.h)
        bool same = true;
        for (int i = 0; i < 3; ++i) same = same && tg.indexMin[i] == dg.indexMin[i] && tg.dim[i] == m.nx * (i == 0) + m.ny * (i == 1) + m.nz * (i == 2);
        for (int i = 0; i < 9; ++i) same = same && tg.mat[i] == dg.mat[i];
        for (int i = 0; i < 3; ++i) same = same && tg.vec[i] == dg.vec[i];
        if (!same) throw Error(filename + ": the \"" + temperaturename + "\" grid's index bounding box or index-to-world map differs from the density grid's (outside this build's scope)");
        if (!temperatureStorage) throw Error("CreateMedium(\"nanovdb\") with a temperature grid needs a second storage vector to own it");
        *temperatureStorage = std::move(tg.dense);
        m.temperature = temperatureStorage->data();
        m.nvdb_le_scale = LeScale;
        m.temperature_offset = temperatureOffset;
        m.temperature_scale = temperatureScale;
    }
    return m;
}

void RgbGridStorage::Attach(VspgScene *scene) const {
    scene->rgb_sigma_a = sigma_a.empty() ? nullptr : sigma_a.data();
    scene->rgb_sigma_s = sigma_s.empty() ? nullptr : sigma_s.data();
    scene->rgb_Le = Le.empty() ? nullptr : Le.data();
    scene->rgb_sigma_scale = scale;
    scene->rgb_le_scale = Lescale;
}

static VspgMedium CreateRgbGridMedium(const ParameterDictionary &p, RgbGridStorage *rgb) {
    // RGBGridMedium::Create (media.cpp:411-484); sizes are counted in RGB triples, as GetRGBArray's vectors are
    VspgMedium m;
    std::memset(&m, 0, sizeof m);
    std::vector<float> sigma_a = p.GetRGBArray("sigma_a"), sigma_s = p.GetRGBArray("sigma_s"), Le = p.GetRGBArray("Le");
    if (sigma_a.empty() && sigma_s.empty()) throw Error("RGB grid requires \"sigma_a\" and/or \"sigma_s\" parameter values.");
    size_t nDensity;
    if (!sigma_a.empty()) {
        nDensity = sigma_a.size() / 3;
        if (!sigma_s.empty() && nDensity != sigma_s.size() / 3)
            throw Error("Different number of samples (" + std::to_string(nDensity) + " vs " + std::to_string(sigma_s.size() / 3) +
                        ") provided for \"sigma_a\" and \"sigma_s\".");
    } else
        nDensity = sigma_s.size() / 3;
    if (!Le.empty() && sigma_a.empty()) throw Error("RGB grid requires \"sigma_a\" if \"Le\" value provided.");
    if (!Le.empty() && nDensity != Le.size() / 3)
        throw Error("Expected " + std::to_string(nDensity) + " values for \"Le\" parameter but were given " + std::to_string(Le.size() / 3) + ".");
    const int nx = p.GetOneInt("nx", 1), ny = p.GetOneInt("ny", 1), nz = p.GetOneInt("nz", 1);
    if ((long long)nDensity != (long long)nx * ny * nz)
        throw Error("RGB grid medium has " + std::to_string(nDensity) + " density values; expected nx*ny*nz = " + std::to_string((long long)nx * ny * nz));
    float p0[3] = {0.f, 0.f, 0.f}, p1[3] = {1.f, 1.f, 1.f};
    p.GetOnePoint3("p0", p0);
    p.GetOnePoint3("p1", p1);
    const float LeScale = p.GetOneFloat("Lescale", 1.f);
    const float g = p.GetOneFloat("g", 0.f);
    const float sigmaScale = p.GetOneFloat("scale", 1.f);
    p.ReportUnused();
    if (!rgb) throw Error("CreateMedium(\"rgbgrid\") needs an RgbGridStorage to own the grids");
    rgb->sigma_a = std::move(sigma_a);
    rgb->sigma_s = std::move(sigma_s);
    rgb->Le = std::move(Le);
    rgb->scale = sigmaScale;
    rgb->Lescale = LeScale;
    m.type = VSPG_MEDIUM_RGBGRID;
    for (int i = 0; i < 3; ++i) {
        m.bounds_min[i] = p0[i];
        m.bounds_max[i] = p1[i];
    }
    m.g = g;
    m.nx = nx; m.ny = ny; m.nz = nz;
    return m;
}

VspgMedium CreateMedium(const std::string &name, const ParameterDictionary &p, std::vector<float> *densityStorage,
                        std::vector<float> *leScaleStorage, std::vector<float> *temperatureStorage, RgbGridStorage *rgbStorage) {
    VspgMedium m;
    std::memset(&m, 0, sizeof m);
    if (name == "rgbgrid") return CreateRgbGridMedium(p, rgbStorage);
    if (name == "uniformgrid") return CreateGridMedium(p, densityStorage, leScaleStorage, temperatureStorage);
    if (name == "nanovdb") return CreateNanoVdbMedium(p, densityStorage, temperatureStorage ? temperatureStorage : leScaleStorage);
    if (name != "homogeneous")
        throw Error("medium \"" + name + "\": only \"homogeneous\", \"uniformgrid\", \"rgbgrid\" and \"nanovdb\" are inside this build's scope");
    // HomogeneousMedium::Create (media.cpp:167-206)
    if (!p.GetOneString("preset", "").empty()) throw Error("medium \"preset\" tables are outside this build's scope");
    float sa[3] = {1.f, 1.f, 1.f}, ss[3] = {1.f, 1.f, 1.f}, le[3] = {0, 0, 0};  // defaults: ConstantSpectrum(1)
    p.GetOneRGB("sigma_a", sa);
    p.GetOneRGB("sigma_s", ss);
    bool hasLe = p.GetOneRGB("Le", le);
    float LeScale = p.GetOneFloat("Lescale", 1.f);
    float sigmaScale = p.GetOneFloat("scale", 1.f);
    float g = p.GetOneFloat("g", 0.0f);
    p.ReportUnused();
    m.type = VSPG_MEDIUM_HOMOGENEOUS;
    for (int i = 0; i < 3; ++i) {
        m.sigma_a[i] = sa[i] * sigmaScale;   // RGBUnboundedSpectrum::Scale (media.h:237-239)
        m.sigma_s[i] = ss[i] * sigmaScale;
        m.Le[i] = hasLe ? le[i] * LeScale : 0.f;
    }
    m.g = g;
    return m;
}

// ---------------------------------------------------------------------------------------
VspgIntegratorParams ParseIntegratorParams(const ParameterDictionary &parameters, GuidingCacheSettings *cache, TrBufferSettings *tr,
                                           IsgBufferSettings *isg) {
    // GuidedVolPathVSPGIntegrator::Create (guidedvolpathvspgintegrator.cpp:1260-1322)
    VspgIntegratorParams p;
    vspg_integrator_params_default(&p);
    p.maxdepth = parameters.GetOneInt("maxdepth", 5);
    p.minrrdepth = parameters.GetOneInt("minrrdepth", 1);
    p.usenee = parameters.GetOneBool("usenee", true);
    p.surfaceguiding = parameters.GetOneBool("surfaceguiding", true);
    p.volumeguiding = parameters.GetOneBool("volumeguiding", true);
    p.surfaceguidingtype = parameters.GetOneString("surfaceguidingtype", "ris") == "mis" ? VSPG_GUIDE_MIS : VSPG_GUIDE_RIS;
    p.volumeguidingtype = parameters.GetOneString("volumeguidingtype", "mis") == "mis" ? VSPG_GUIDE_MIS : VSPG_GUIDE_RIS;
    GuidingCacheSettings cs;
    cs.store = parameters.GetOneBool("storeGuidingCache", false);
    cs.load = parameters.GetOneBool("loadGuidingCache", false);
    cs.fileName = parameters.GetOneString("guidingCacheFileName", "");
    if (cache) *cache = cs;
    p.vspguiding = parameters.GetOneBool("vspguiding", true);
    p.vspprimaryguiding = parameters.GetOneBool("vspprimaryguiding", true);
    p.vspsecondaryguiding = parameters.GetOneBool("vspsecondaryguiding", true);
    p.vspmisratio = parameters.GetOneFloat("vspmisratio", 0.5f);
    std::string crit = parameters.GetOneString("vspcriterion", "variance");
    if (crit == "Contribution" || crit == "contribution") p.vspcriterion = VSPG_VSP_CONTRIBUTION;
    else if (crit == "Variance" || crit == "variance") p.vspcriterion = VSPG_VSP_VARIANCE;
    std::string meth = parameters.GetOneString("vspsamplingmethod", "resampling");
    if (meth == "Resampling" || meth == "resampling") p.vspsamplingmethod = VSPG_VSP_RESAMPLING;
    else if (meth == "NDS" || meth == "nds") p.vspsamplingmethod = VSPG_VSP_NDS;
    p.collisionProbabilityBias = parameters.GetOneBool("collisionProbabilityBias", false);
    IsgBufferSettings is;
    is.store = parameters.GetOneBool("storeISGBuffer", false);
    is.load = parameters.GetOneBool("loadISGBuffer", false);
    is.fileName = parameters.GetOneString("isgBufferFileName", "");
    if (isg) *isg = is;
    TrBufferSettings ts;
    ts.store = parameters.GetOneBool("storeTrBuffer", false);
    ts.load = parameters.GetOneBool("loadTrBuffer", false);
    ts.fileName = parameters.GetOneString("trBufferFileName", "");
    if (tr) *tr = ts;
    p.storeTrBuffer = ts.store;
    p.rrguiding = parameters.GetOneBool("rrguiding", false);
    p.surfacerrguiding = parameters.GetOneBool("surfacerrguiding", true);
    p.volumerrguiding = parameters.GetOneBool("volumerrguiding", true);
    std::string ls = parameters.GetOneString("lightsampler", "bvh");
    if (ls == "uniform") p.lightsampler = VSPG_LIGHTSAMPLER_UNIFORM;
    else if (ls == "power") p.lightsampler = VSPG_LIGHTSAMPLER_POWER;
    else if (ls == "bvh") p.lightsampler = VSPG_LIGHTSAMPLER_BVH;
    else throw Error("Light sample distribution type \"" + ls + "\" unknown.");
    p.regularize = parameters.GetOneBool("regularize", false);
    if ((is.store || is.load) && is.fileName.empty()) throw Error("storeISGBuffer / loadISGBuffer need \"isgBufferFileName\"");
    if ((ts.store || ts.load) && ts.fileName.empty()) throw Error("storeTrBuffer / loadTrBuffer need \"trBufferFileName\"");
    if ((cs.store || cs.load) && cs.fileName.empty()) throw Error("storeGuidingCache / loadGuidingCache need \"guidingCacheFileName\"");
    return p;
}

std::unique_ptr<Integrator> Integrator::Create(const std::string &name, const ParameterDictionary &parameters,
                                               const VspgScene &scene, int xres, int yres, int pixelSamples, int seed,
                                               int device, const VspgSceneTextures *textures) {
    std::unique_ptr<Integrator> integrator;
    if (name == "guidedvolpathvspg")
        integrator = GuidedVolPathVSPGIntegrator::Create(parameters, scene, xres, yres, pixelSamples, seed, device, textures);
    else if (name == "guidedvolpath") {
        // the reference's "guidedvolpath" has no VSP guiding and rejects "vspguiding" as unused;
        // BASELINE.json nevertheless names `guidedvolpath` + vspguiding: accept that spelling as
        // an alias of the VSPG integrator, and only that spelling
        if (!parameters.GetOneBool("vspguiding", false))
            throw Error("integrator \"guidedvolpath\" without \"vspguiding\" true is outside this build's scope "
                        "(directional guiding only); use \"guidedvolpathvspg\"");
        integrator = GuidedVolPathVSPGIntegrator::Create(parameters, scene, xres, yres, pixelSamples, seed, device, textures);
    } else
        throw Error(name + ": integrator type unknown.");  // integrators.cpp:3760
    parameters.ReportUnused();  // integrators.cpp:3766
    return integrator;
}

std::unique_ptr<GuidedVolPathVSPGIntegrator> GuidedVolPathVSPGIntegrator::Create(const ParameterDictionary &parameters,
                                                                                 const VspgScene &scene, int xres, int yres,
                                                                                 int pixelSamples, int seed, int device,
                                                                                 const VspgSceneTextures *textures) {
    GuidingCacheSettings cache;
    TrBufferSettings tr;
    IsgBufferSettings isg;
    VspgIntegratorParams p = ParseIntegratorParams(parameters, &cache, &tr, &isg);
    return std::make_unique<GuidedVolPathVSPGIntegrator>(p, scene, xres, yres, pixelSamples, seed, device, cache, tr, isg, textures);
}

GuidedVolPathVSPGIntegrator::GuidedVolPathVSPGIntegrator(const VspgIntegratorParams &p, const VspgScene &scene, int xres,
                                                         int yres, int pixelSamples, int seed, int device,
                                                         const GuidingCacheSettings &cache, const TrBufferSettings &tr,
                                                         const IsgBufferSettings &isg, const VspgSceneTextures *textures)
    : params(p), spp(pixelSamples), cacheSettings(cache), trSettings(tr), isgSettings(isg) {
    std::memset(&cfg, 0, sizeof cfg);
    cfg.xres = xres; cfg.yres = yres; cfg.spp = pixelSamples; cfg.seed = seed;
    cfg.shard_index = 0; cfg.shard_count = 1; cfg.device = device;
    bounds[2] = xres; bounds[3] = yres;
    int rc = vspg_renderer_create_textured(&scene, textures, &params, &cfg, &renderer);
    if (rc != 0) throw Error(std::string("GuidedVolPathVSPGIntegrator: ") + vspg_last_error());
    if (cacheSettings.load) {  // :116-125: FileExists() ? load (guideTraining = false) : warn and train a fresh field
        std::FILE *probe = std::fopen(cacheSettings.fileName.c_str(), "rb");
        if (!probe) {
            std::fprintf(stderr, "Warning: guiding cache file does not exists: guidingCacheFileName = %s\n", cacheSettings.fileName.c_str());
        } else {
            std::fclose(probe);
            std::string msg;
            try {
                GuidingCache gc = GuidingCache::Read(cacheSettings.fileName);
                VspgField f[2];
                for (int i = 0; i < 2; ++i)
                    f[i] = VspgField{(int32_t)gc.nodes[i].size(), (int32_t)gc.regions[i].size(), gc.nodes[i].data(), gc.regions[i].data()};
                if (vspg_renderer_set_guiding_field(renderer, &f[0], &f[1], nullptr) != 0) msg = vspg_last_error();
            } catch (const std::exception &e) {  // corrupt / truncated file: the renderer exists already, release it
                msg = e.what();
            }
            if (!msg.empty()) {
                vspg_renderer_destroy(renderer);
                renderer = nullptr;
                throw Error("GuidedVolPathVSPGIntegrator: loading \"" + cacheSettings.fileName + "\": " + msg);
            }
        }
    }
    if (isgSettings.load) {  // :151-159: a missing file is a warning, the buffer is then estimated in-loop as usual
        std::FILE *probe = std::fopen(isgSettings.fileName.c_str(), "rb");
        if (!probe) {
            std::fprintf(stderr, "Warning: ImageSpaceGuidingBuffer file does not exists: isgBufferFileName = %s\n", isgSettings.fileName.c_str());
        } else {
            std::fclose(probe);
            std::string msg;
            try {
                VspBuffer vb = VspBuffer::Load(isgSettings.fileName);
                if (vb.xres != xres || vb.yres != yres) msg = "resolution differs from the film's";
                else if (vspg_vsp_buffer_load(renderer, vb.vsp.data(), nullptr) != 0) msg = vspg_last_error();
            } catch (const Error &e) {
                msg = e.what();
            }
            if (!msg.empty()) {
                vspg_renderer_destroy(renderer);
                throw Error("GuidedVolPathVSPGIntegrator: loading \"" + isgSettings.fileName + "\": " + msg);
            }
        }
    }
    if (trSettings.load) {  // :180-188: a missing file is a warning, the render goes on without NDS+
        std::FILE *probe = std::fopen(trSettings.fileName.c_str(), "rb");
        if (!probe) {
            std::fprintf(stderr, "Warning: Tr buffer file does not exists: trBufferFileName = %s\n", trSettings.fileName.c_str());
        } else {
            std::fclose(probe);
            std::string msg;
            try {
                // (format by extension, as pbrt's Image::Read: the reference's EXR with its channel names, or this adapter's PFM)
                TrBuffer tb = HasExtension(trSettings.fileName, ".exr") ? TrBuffer::FromImage(ReadImage(trSettings.fileName), trSettings.fileName)
                                                                          : TrBuffer::Load(trSettings.fileName);
                if (tb.xres != xres || tb.yres != yres) msg = "resolution differs from the film's";
                else if (vspg_renderer_set_tr_buffer(renderer, tb.rgb.data(), nullptr) != 0) msg = vspg_last_error();
            } catch (const Error &e) {
                msg = e.what();
            }
            if (!msg.empty()) {
                vspg_renderer_destroy(renderer);
                throw Error("GuidedVolPathVSPGIntegrator: loading \"" + trSettings.fileName + "\": " + msg);
            }
        }
    }
}
GuidedVolPathVSPGIntegrator::~GuidedVolPathVSPGIntegrator() {
    if (isgSettings.store) {  // :214-216
        try {
            GetVspBuffer().Store(isgSettings.fileName);
        } catch (const Error &e) {
            std::fprintf(stderr, "GuidedVolPathVSPGIntegrator: storing the image-space guiding buffer failed: %s\n", e.what());
        }
    }
    if (trSettings.store) {  // :219-221
        try {
            if (HasExtension(trSettings.fileName, ".exr")) vspg::WriteImage(GetTrBuffer().ToImage(), trSettings.fileName);  // (trbuffer.h:52-71)
            else GetTrBuffer().Store(trSettings.fileName);
        } catch (const Error &e) {
            std::fprintf(stderr, "GuidedVolPathVSPGIntegrator: storing the transmittance buffer failed: %s\n", e.what());
        }
    }
    if (cacheSettings.store) {  // :210-213
        try {
            GetGuidingCache().Write(cacheSettings.fileName);
        } catch (const Error &e) {
            std::fprintf(stderr, "GuidedVolPathVSPGIntegrator: storing the guiding cache failed: %s\n", e.what());
        }
    }
    vspg_renderer_destroy(renderer);
}
VspgTrainStats GuidedVolPathVSPGIntegrator::TrainingStats() {
    VspgTrainStats st;
    if (vspg_renderer_training_stats(renderer, &st, nullptr) != 0) throw Error(vspg_last_error());
    return st;
}
VspBuffer GuidedVolPathVSPGIntegrator::GetVspBuffer() {
    VspBuffer vb;
    vb.xres = cfg.xres; vb.yres = cfg.yres;
    vb.vsp.resize((size_t)cfg.xres * cfg.yres);
    int ready = 0;
    if (vspg_vsp_buffer_read(renderer, vb.vsp.data(), &ready, nullptr) != 0) throw Error(vspg_last_error());
    vb.ready = ready != 0;
    if (!vb.ready) std::fill(vb.vsp.begin(), vb.vsp.end(), -1.f);  // no estimate yet
    return vb;
}
TrBuffer GuidedVolPathVSPGIntegrator::GetTrBuffer() {
    TrBuffer tb;
    tb.xres = cfg.xres; tb.yres = cfg.yres;
    tb.rgb.resize((size_t)cfg.xres * cfg.yres * 3);
    if (vspg_renderer_get_tr_buffer(renderer, tb.rgb.data(), nullptr, nullptr) != 0) throw Error(vspg_last_error());
    return tb;
}
static bool has_pfm_extension(const std::string &fn) {
    if (fn.size() < 4) return false;
    std::string e = fn.substr(fn.size() - 4);
    for (char &c : e) c = (char)std::tolower((unsigned char)c);
    return e == ".pfm";
}
// The PFM raster itself is the Image layer's (vspg_image.cpp); these four keep their PFM-only contract and their types.
void VspBuffer::Store(const std::string &filename) const {
    if (!has_pfm_extension(filename)) throw Error(filename + ": only the .pfm format is supported for the image-space guiding buffer");
    Image img;
    img.xres = xres; img.yres = yres;
    img.channels = {"Y"};
    img.data = vsp;
    vspg::WriteImage(img, filename);
}
VspBuffer VspBuffer::Load(const std::string &filename) {
    if (!has_pfm_extension(filename)) throw Error(filename + ": only the .pfm format is supported for the image-space guiding buffer");
    Image img = ReadImage(filename);
    if (img.NChannels() != 1) throw Error(filename + ": not a single-channel PFM image");
    VspBuffer vb;
    vb.xres = img.xres; vb.yres = img.yres;
    vb.vsp = std::move(img.data);
    vb.ready = true;
    return vb;
}
void TrBuffer::Store(const std::string &filename) const {
    if (!has_pfm_extension(filename)) throw Error(filename + ": only the .pfm format of pbrt's Image class is supported here (ToImage + WriteImage write OpenEXR)");
    Image img;
    img.xres = xres; img.yres = yres;
    img.channels = {"R", "G", "B"};
    img.data = rgb;
    vspg::WriteImage(img, filename);
}
TrBuffer TrBuffer::Load(const std::string &filename) {
    if (!has_pfm_extension(filename)) throw Error(filename + ": only the .pfm format of pbrt's Image class is supported here (ReadImage + FromImage read OpenEXR)");
    Image img = ReadImage(filename);
    if (img.NChannels() != 3) throw Error(filename + ": not a 3-channel PFM image");
    TrBuffer tb;
    tb.xres = img.xres; tb.yres = img.yres;
    tb.rgb = std::move(img.data);  // (a "PF" file's channels are R, G, B in that order)
    return tb;
}
Image TrBuffer::ToImage() const {
    Image img;
    img.xres = xres; img.yres = yres;
    img.half = false;
    img.channels = {"Transmittance.R", "Transmittance.G", "Transmittance.B"};
    img.data = rgb;
    return img;
}
TrBuffer TrBuffer::FromImage(const Image &image, const std::string &name) {
    TrBuffer tb;
    tb.xres = image.xres; tb.yres = image.yres;
    tb.rgb = image.Gather({"Transmittance.R", "Transmittance.G", "Transmittance.B"}, name + ": the image");
    return tb;
}
GuidingCache GuidedVolPathVSPGIntegrator::GetGuidingCache() {
    GuidingCache gc;
    for (int f = 0; f < 2; ++f) {
        int32_t nn = 0, nr = 0;
        if (vspg_renderer_get_guiding_field(renderer, f, nullptr, nullptr, &nn, &nr, nullptr) != 0) throw Error(vspg_last_error());
        gc.nodes[f].resize((size_t)nn);
        gc.regions[f].resize((size_t)nr);
        if (vspg_renderer_get_guiding_field(renderer, f, gc.nodes[f].data(), gc.regions[f].data(), &nn, &nr, nullptr) != 0)
            throw Error(vspg_last_error());
    }
    return gc;
}

void GuidingCache::Write(const std::string &filename) const {
    std::ofstream f(filename, std::ios::binary);
    if (!f) throw Error("cannot open \"" + filename + "\" for writing");
    const char magic[8] = {'V', 'S', 'P', 'G', 'F', 'L', 'D', '1'};
    const uint32_t head[2] = {VSPG_FIELD_LOBES, 0u};
    f.write(magic, 8);
    f.write(reinterpret_cast<const char *>(head), sizeof head);
    for (int i = 0; i < 2; ++i) {
        const uint32_t n[2] = {(uint32_t)nodes[i].size(), (uint32_t)regions[i].size()};
        f.write(reinterpret_cast<const char *>(n), sizeof n);
    }
    for (int i = 0; i < 2; ++i) {
        f.write(reinterpret_cast<const char *>(nodes[i].data()), (std::streamsize)(nodes[i].size() * sizeof(VspgKdNode)));
        f.write(reinterpret_cast<const char *>(regions[i].data()), (std::streamsize)(regions[i].size() * sizeof(VspgFieldRegion)));
    }
    if (!f) throw Error("short write to \"" + filename + "\"");
}
GuidingCache GuidingCache::Read(const std::string &filename) {
    std::ifstream f(filename, std::ios::binary);
    if (!f) throw Error("cannot open guiding cache \"" + filename + "\"");
    char magic[8];
    uint32_t head[2], n[2][2];
    f.read(magic, 8);
    f.read(reinterpret_cast<char *>(head), sizeof head);
    f.read(reinterpret_cast<char *>(n), sizeof n);
    if (!f || std::memcmp(magic, "VSPGFLD1", 8) != 0) throw Error("\"" + filename + "\" is not a VSPGFLD1 guiding cache");
    if (head[0] != VSPG_FIELD_LOBES) throw Error("guiding cache was written with a different lobe count");
    GuidingCache gc;
    for (int i = 0; i < 2; ++i) {
        if (n[i][0] > (1u << 24) || n[i][1] > (1u << 24)) throw Error("guiding cache header is corrupt");
        gc.nodes[i].resize(n[i][0]);
        gc.regions[i].resize(n[i][1]);
    }
    for (int i = 0; i < 2; ++i) {
        f.read(reinterpret_cast<char *>(gc.nodes[i].data()), (std::streamsize)(gc.nodes[i].size() * sizeof(VspgKdNode)));
        f.read(reinterpret_cast<char *>(gc.regions[i].data()), (std::streamsize)(gc.regions[i].size() * sizeof(VspgFieldRegion)));
    }
    if (!f) throw Error("guiding cache \"" + filename + "\" is truncated");
    return gc;
}

std::vector<float> LoadMseReferenceImage(const std::string &filename, int xres, int yres, int x0, int y0, int x1, int y1) {
    TrBuffer img;
    {   // Image::Read by extension; the channels R, G, B by name (integrators.cpp:131-135)
        const Image file = ReadImage(filename);
        img.xres = file.xres; img.yres = file.yres;
        img.rgb = file.Gather({"R", "G", "B"}, filename + ": the MSE reference image");
    }
    const int bw = x1 - x0, bh = y1 - y0;
    if (img.xres == xres && img.yres == yres) return img.rgb;
    if (img.xres != bw || img.yres != bh)
        throw Error(filename + ": the MSE reference image is " + std::to_string(img.xres) + " x " + std::to_string(img.yres) + ", it must have the size of the frame (" +
                    std::to_string(xres) + " x " + std::to_string(yres) + ") or of the pixel bounds (" + std::to_string(bw) + " x " + std::to_string(bh) + ")");
    std::vector<float> frame((size_t)xres * yres * 3, 0.f);
    for (int y = 0; y < bh; ++y)
        std::memcpy(&frame[((size_t)(y0 + y) * xres + x0) * 3], &img.rgb[(size_t)y * bw * 3], (size_t)bw * 3 * sizeof(float));
    return frame;
}
void CheckMseReferenceOptions(const std::string &image, const std::string &out) {
    if (!image.empty() && out.empty()) throw Error("Must provide MSE reference output filename via --mse-reference-out");
    if (!out.empty() && image.empty()) throw Error("Must provide MSE reference image via --mse-reference-image");
}
float FilmErrorAverage(const VspgFilmError &rec, const double sums[3]) {
    const float n = float(rec.x1 - rec.x0) * float(rec.y1 - rec.y0);
    float sum = 0;
    for (int c = 0; c < 3; ++c) {
        const float mean = float(sums[c] / n);  // (double / Float, stored as Float: image.cpp:605)
        sum += mean;
    }
    return sum / 3;
}
void GuidedVolPathVSPGIntegrator::SetMseReference(const std::vector<float> &frameImage, std::FILE *out) {
    if (frameImage.size() != (size_t)cfg.xres * cfg.yres * 3) throw Error("the MSE reference image does not have the size of the frame");
    if (vspg_renderer_set_reference_image(renderer, frameImage.data(), nullptr) != 0) throw Error(vspg_last_error());
    mseOut = out;
}
void GuidedVolPathVSPGIntegrator::SetEnvironmentImage(int light, const std::vector<float> &rgb, int res, const float *renderFromLight) {
    if (res < 1 || rgb.size() != (size_t)res * res * 3) throw Error("the environment image does not hold res * res * 3 values");
    if (vspg_renderer_set_environment_image(renderer, light, rgb.data(), res, renderFromLight, nullptr) != 0) throw Error(vspg_last_error());
}
void GuidedVolPathVSPGIntegrator::SetLightImage(int slot, const std::vector<float> &pixels, int xres, int yres, int channels) {
    if (xres < 1 || yres < 1 || channels < 1 || pixels.size() != (size_t)xres * yres * channels) throw Error("the light image does not hold xres * yres * channels values");
    if (vspg_renderer_set_light_image(renderer, slot, pixels.data(), xres, yres, channels, nullptr) != 0) throw Error(vspg_last_error());
}
void GuidedVolPathVSPGIntegrator::SetCamera(const VspgCamera &camera, const VspgCameraModel &model) {
    if (vspg_renderer_set_camera(renderer, &camera, &model, nullptr) != 0) throw Error(vspg_last_error());
}
void GuidedVolPathVSPGIntegrator::SetMediumDensity(const std::vector<float> &values) {
    if (vspg_renderer_update_grid(renderer, VSPG_GRID_DENSITY, values.data(), values.size(), VSPG_MEM_HOST, nullptr) != 0) throw Error(vspg_last_error());
}
void GuidedVolPathVSPGIntegrator::SetMediumTemperature(const std::vector<float> &values) {
    if (vspg_renderer_update_grid(renderer, VSPG_GRID_TEMPERATURE, values.data(), values.size(), VSPG_MEM_HOST, nullptr) != 0) throw Error(vspg_last_error());
}
void GuidedVolPathVSPGIntegrator::SetMediumRgbGrids(const RgbGridStorage &grids) {
    const std::vector<float> *g[3] = {&grids.sigma_a, &grids.sigma_s, &grids.Le};
    size_t n = 0;
    for (const std::vector<float> *v : g)
        if (!v->empty()) {
            if (n != 0 && v->size() != n) throw Error("SetMediumRgbGrids: the given grids differ in size");
            n = v->size();
        }
    auto ptr = [](const std::vector<float> &v) { return v.empty() ? nullptr : v.data(); };
    if (vspg_renderer_update_rgb_grids(renderer, ptr(grids.sigma_a), ptr(grids.sigma_s), ptr(grids.Le), n, VSPG_MEM_HOST, nullptr) != 0)
        throw Error(vspg_last_error());
}
void GuidedVolPathVSPGIntegrator::ClearFilm() {
    if (vspg_film_clear(renderer, nullptr) != 0) throw Error(vspg_last_error());
    sppDone = 0;
}

void GuidedVolPathVSPGIntegrator::Render() {
    // ImageTileIntegrator::Render (integrators.cpp:123-239): waves of 1 spp, PostProcessWave each
    int waveStart = 0, waveEnd = 1, nextWaveSize = 1;
    const auto renderStart = std::chrono::steady_clock::now();
    auto elapsed = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - renderStart).count(); };
    VspgCounters before;
    std::memset(&before, 0, sizeof before);
    // the film's error against the reference image, one record per wave (:243-257), kept on the device until the log is drained
    std::vector<VspgFilmError> errors;
    size_t logged = 0;
    auto drainErrors = [&]() {
        if (logged == 0) return;
        const size_t at = errors.size();
        errors.resize(at + logged);
        size_t n = 0;
        if (vspg_film_error_read(renderer, errors.data() + at, logged, &n, nullptr) != 0) throw Error(vspg_last_error());
        errors.resize(at + n);
        logged = 0;
    };
    while (waveStart < spp) {
        const auto t0 = std::chrono::steady_clock::now();
        const std::string kernel = waveLog ? vspg_renderer_kernel_name(renderer) : "";
        if (vspg_render_window(renderer, bounds[0], bounds[1], bounds[2], bounds[3], waveStart, waveEnd, nullptr) != 0) throw Error(vspg_last_error());
        PostProcessWave();
        if (mseOut) {  // (tag: the samples per pixel so far, the reference's waveStart at :254)
            if (vspg_film_error_enqueue(renderer, bounds[0], bounds[1], bounds[2], bounds[3], waveEnd, nullptr) != 0) throw Error(vspg_last_error());
            if (++logged == VSPG_FILM_ERROR_LOG_RECORDS) drainErrors();
        }
        if (waveLog) {  // one JSON line per wave: the counter read synchronises the stream, so `ms` is the wave's wall time
            VspgCounters c;
            if (vspg_get_counters(renderer, &c, nullptr) != 0) throw Error(vspg_last_error());
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            std::fprintf(waveLog, "{\"wave\": %d, \"ms\": %.4f, \"paths\": %llu, \"segments\": %llu, \"density_queries\": %llu, \"kernel\": \"%s\"", waveStart, ms,
                         (unsigned long long)(c.paths - before.paths), (unsigned long long)(c.segments - before.segments),
                         (unsigned long long)(c.density_queries - before.density_queries), kernel.c_str());
            if (mseOut) {  // (the stream is synchronised already: the wave's record is there)
                drainErrors();
                const VspgFilmError &e = errors.back(), &e0 = errors.front();
                std::fprintf(waveLog, ", \"mse\": %.9g, \"mrse\": %.9g, \"device_ms\": %.6f", FilmErrorAverage(e, e.sum_se), FilmErrorAverage(e, e.sum_rse),
                             e.tick_khz ? double(e.device_ticks - e0.device_ticks) / double(e.tick_khz) : 0.);
            }
            std::fprintf(waveLog, "}\n");
            std::fflush(waveLog);
            before = c;
        }
        sppDone = waveEnd;
        if (outPartial && !outFile.empty()) {  // --write-partial-images (:258-261): the image so far, with its metadata (:245-255)
            renderSeconds = elapsed();
            if (mseOut) {
                drainErrors();
                haveMse = true;
                lastMse = FilmErrorAverage(errors.back(), errors.back().sum_se);
            }
            WriteImage();
        }
        waveStart = waveEnd;
        waveEnd = std::min(spp, waveEnd + nextWaveSize);
    }
    if (mseOut) {
        drainErrors();
        if (!errors.empty()) {
            haveMse = true;
            lastMse = FilmErrorAverage(errors.back(), errors.back().sum_se);
        }
        for (const VspgFilmError &e : errors) std::fprintf(mseOut, "%d, %.9g\n", e.tag, FilmErrorAverage(e, e.sum_se));  // :254
        std::fflush(mseOut);
    }
    renderSeconds = elapsed();
}
void GuidedVolPathVSPGIntegrator::SetOutput(const std::string &filename, bool fp16, bool writePartial) {
    outFile = filename;
    outFp16 = fp16;
    outPartial = writePartial;
}
void GuidedVolPathVSPGIntegrator::WriteImage() {
    if (outFile.empty()) throw Error("GuidedVolPathVSPGIntegrator::WriteImage: no output file (SetOutput)");
    if (!HasExtension(outFile, ".exr")) {
        GetFilm().WritePFM(outFile);
        return;
    }
    Image meta;
    meta.xres = bounds[2] - bounds[0]; meta.yres = bounds[3] - bounds[1];
    meta.channels = {"B", "G", "R"};
    meta.dataX0 = bounds[0]; meta.dataY0 = bounds[1];
    meta.fullX = cfg.xres; meta.fullY = cfg.yres;
    meta.samplesPerPixel = sppDone;
    meta.renderTimeSeconds = (float)renderSeconds;
    if (haveMse) meta.MSE = lastMse;
    // the device hands over the scan-line payload itself: 6 (or 12) bytes per pixel, nothing rearranged on the host
    std::vector<unsigned char> lines((size_t)meta.xres * meta.yres * 3 * (outFp16 ? 2 : 4));
    uint64_t nClamped = 0;
    if (vspg_film_resolve(renderer, bounds[0], bounds[1], bounds[2], bounds[3], outFp16 ? VSPG_RESOLVE_F16 : VSPG_RESOLVE_F32, VSPG_RESOLVE_SCANLINE_BGR,
                          lines.data(), lines.size(), &nClamped, nullptr) != 0)
        throw Error(vspg_last_error());
    if (nClamped > 0) std::fprintf(stderr, "Warning: %d pixel values clamped to maximum fp16 value.\n", (int)nClamped);  // (film.cpp:558-559)
    WriteExrScanlines(meta, outFp16, lines.data(), outFile);
}
void GuidedVolPathVSPGIntegrator::PostProcessWave() {
    if (vspg_post_process_wave(renderer, nullptr) != 0) throw Error(vspg_last_error());
}
std::string GuidedVolPathVSPGIntegrator::ToString() const {
    char buf[256];
    std::snprintf(buf, sizeof buf, "[ GuidedVolPathVSPGIntegrator maxDepth: %d lightSampler: %s regularize: %s ]", params.maxdepth,
                  params.lightsampler == VSPG_LIGHTSAMPLER_BVH ? "bvh" : (params.lightsampler == VSPG_LIGHTSAMPLER_POWER ? "power" : "uniform"),
                  params.regularize ? "true" : "false");
    return buf;
}
void GuidedVolPathVSPGIntegrator::SetPixelBounds(int x0, int y0, int x1, int y1) {
    if (x0 < 0 || y0 < 0 || x1 <= x0 || y1 <= y0 || x1 > cfg.xres || y1 > cfg.yres) throw Error("pixel bounds are empty or not inside the film");
    bounds[0] = x0; bounds[1] = y0; bounds[2] = x1; bounds[3] = y1;
}
Film GuidedVolPathVSPGIntegrator::GetFilm() {
    std::vector<float> whole((size_t)cfg.xres * cfg.yres * 4);
    if (vspg_film_read(renderer, whole.data(), nullptr) != 0) throw Error(vspg_last_error());
    return CropFilm(whole, cfg.xres, bounds[0], bounds[1], bounds[2], bounds[3]);
}
Film CropFilm(const std::vector<float> &rgbw, int xres, int x0, int y0, int x1, int y1) {
    Film f;
    f.xres = x1 - x0; f.yres = y1 - y0; f.x0 = x0; f.y0 = y0;
    f.rgbw.resize((size_t)f.xres * f.yres * 4);
    for (int y = y0; y < y1; ++y)
        std::memcpy(&f.rgbw[(size_t)(y - y0) * f.xres * 4], &rgbw[((size_t)y * xres + x0) * 4], (size_t)f.xres * 4 * sizeof(float));
    return f;
}
VspgCounters GuidedVolPathVSPGIntegrator::Counters() {
    VspgCounters c;
    if (vspg_get_counters(renderer, &c, nullptr) != 0) throw Error(vspg_last_error());
    return c;
}

void Film::GetPixelRGB(int x, int y, float rgb[3]) const {
    const float *p = &rgbw[((size_t)y * xres + x) * 4];
    float w = p[3];
    for (int c = 0; c < 3; ++c) rgb[c] = w != 0 ? p[c] / w : p[c];
}
void Film::WritePFM(const std::string &filename) const {
    std::ofstream f(filename, std::ios::binary);
    f << "PF\n" << xres << " " << yres << "\n-1.0\n";
    for (int y = yres - 1; y >= 0; --y)
        for (int x = 0; x < xres; ++x) {
            float rgb[3];
            GetPixelRGB(x, y, rgb);
            f.write(reinterpret_cast<const char *>(rgb), sizeof rgb);
        }
}

}  // namespace vspg
