// vspg_scenefile.cpp -- see vspg_scenefile.h
#include "vspg_scenefile.h"
#include "vspg_image.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <type_traits>

namespace vspg {
namespace {

// ---- 4x4 float matrices, composed like pbrt's Transform (util/transform.h; SquareMatrix Mul in util/math.h: FMA accumulation) ----
struct M4 {
    float m[4][4];
};
M4 identity() {
    M4 r;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) r.m[i][j] = i == j ? 1.f : 0.f;
    return r;
}
M4 mul(const M4 &a, const M4 &b) {
    M4 r;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            float s = 0.f;
            for (int k = 0; k < 4; ++k) s = std::fmaf(a.m[i][k], b.m[k][j], s);
            r.m[i][j] = s;
        }
    return r;
}
M4 translate(float x, float y, float z) {
    M4 r = identity();
    r.m[0][3] = x; r.m[1][3] = y; r.m[2][3] = z;
    return r;
}
M4 scale(float x, float y, float z) {
    M4 r = identity();
    r.m[0][0] = x; r.m[1][1] = y; r.m[2][2] = z;
    return r;
}
M4 rotate(float thetaDeg, float ax, float ay, float az) {  // transform.h:220-247
    const float l = std::sqrt(ax * ax + ay * ay + az * az);
    if (!(l > 0)) throw Error("Rotate: zero-length axis");
    const float x = ax / l, y = ay / l, z = az / l;
    const float rad = (3.14159265358979323846f / 180) * thetaDeg;
    const float s = std::sin(rad), c = std::cos(rad);
    M4 r = identity();
    r.m[0][0] = x * x + (1 - x * x) * c; r.m[0][1] = x * y * (1 - c) - z * s; r.m[0][2] = x * z * (1 - c) + y * s;
    r.m[1][0] = x * y * (1 - c) + z * s; r.m[1][1] = y * y + (1 - y * y) * c; r.m[1][2] = y * z * (1 - c) - x * s;
    r.m[2][0] = x * z * (1 - c) - y * s; r.m[2][1] = y * z * (1 - c) + x * s; r.m[2][2] = z * z + (1 - z * z) * c;
    return r;
}
bool is_identity(const M4 &a) {
    const M4 i = identity();
    return std::memcmp(&a, &i, sizeof a) == 0;
}
void xf_point(const M4 &a, const float p[3], float out[3]) {  // Transform::operator()(Point3) (transform.h:310-319), affine
    for (int i = 0; i < 3; ++i) out[i] = a.m[i][0] * p[0] + a.m[i][1] * p[1] + a.m[i][2] * p[2] + a.m[i][3];
}
void xf_vector(const M4 &a, const float v[3], float out[3]) {
    for (int i = 0; i < 3; ++i) out[i] = a.m[i][0] * v[0] + a.m[i][1] * v[1] + a.m[i][2] * v[2];
}

// ---- tokens ----------------------------------------------------------------------------------------------------
struct Token {
    enum Kind { Word, String, Number, Open, Close } kind;
    std::string text;
    int line;
};
std::vector<Token> tokenize(const std::string &s) {
    std::vector<Token> out;
    int line = 1;
    for (size_t i = 0; i < s.size();) {
        const char c = s[i];
        if (c == '\n') { ++line; ++i; }
        else if (std::isspace((unsigned char)c)) ++i;
        else if (c == '#') { while (i < s.size() && s[i] != '\n') ++i; }
        else if (c == '[') { out.push_back({Token::Open, "[", line}); ++i; }
        else if (c == ']') { out.push_back({Token::Close, "]", line}); ++i; }
        else if (c == '"') {
            const size_t j = s.find('"', i + 1);
            if (j == std::string::npos) throw Error("line " + std::to_string(line) + ": unterminated string");
            out.push_back({Token::String, s.substr(i + 1, j - i - 1), line});
            i = j + 1;
        } else {
            size_t j = i;
            while (j < s.size() && !std::isspace((unsigned char)s[j]) && s[j] != '[' && s[j] != ']' && s[j] != '"' && s[j] != '#') ++j;
            const std::string t = s.substr(i, j - i);
            const bool num = std::isdigit((unsigned char)t[0]) || t[0] == '-' || t[0] == '+' || t[0] == '.';
            out.push_back({num ? Token::Number : Token::Word, t, line});
            i = j;
        }
    }
    return out;
}

struct GraphicsState {
    M4 ctm = identity();
    float Kd[3] = {0.5f, 0.5f, 0.5f};  // DiffuseMaterial default reflectance 0.5
    bool areaLight = false;
    float Le[3] = {0, 0, 0};
    bool twoSided = false;
    bool reverseOrientation = false;
    int texture = 0;                  // Material "diffuse" "texture reflectance" "name": 0 = none, k = texture k - 1 replaces Kd
    bool interfaceMaterial = false;   // Material "interface" (also "none", ""): no BSDF, the surface only separates media (scene.cpp:1340)
    std::string insideMedium, outsideMedium;
};
struct MediumNames { std::string inside, outside; };   // a shape's MediumInterface, resolved once the scene's medium is known
struct NamedMedium {
    std::string type;
    ParameterDictionary params;
    M4 ctm;
};

class Parser {
  public:
    explicit Parser(const std::string &text, const std::string &baseDir = "") : tok(tokenize(text)), baseDir(baseDir) {}
    std::unique_ptr<SceneDescription> run() {
        sd = std::make_unique<SceneDescription>();
        std::memset(&sd->scene, 0, sizeof sd->scene);
        while (pos < tok.size()) directive();
        finish();
        return std::move(sd);
    }

  private:
    std::vector<Token> tok;
    std::string baseDir;   // directory of the scene file: Include and relative file names resolve against it
    int includeDepth = 0;
    size_t pos = 0;
    std::unique_ptr<SceneDescription> sd;
    GraphicsState gs;
    std::vector<GraphicsState> stack;
    std::map<std::string, NamedMedium> media;
    std::map<std::string, ParameterDictionary> materials;
    bool haveCamera = false, haveLookAt = false, world = false;
    float eye[3] = {0, 0, 0}, look[3] = {0, 0, -1}, up[3] = {0, 1, 0}, fov = 90.f;
    float frameAspect = 0.f;             // Camera "frameaspectratio" (0 = the film's)
    std::vector<float> screenWindow;     // Camera "screenwindow": empty or four values
    std::string cameraMedium;
    std::vector<VspgQuad> quads;
    std::vector<VspgSphere> spheres;
    std::vector<MediumNames> quadMedia, sphereMedia, triMedia;   // per rectangle / sphere / triangle
    std::map<std::string, int> textures;   // Texture "name": its binding value (index + 1)
    std::vector<int> quadTexture;          // per rectangle

    [[noreturn]] void fail(const std::string &msg) const {
        const int line = pos < tok.size() ? tok[pos].line : (tok.empty() ? 0 : tok.back().line);
        throw Error("scene file line " + std::to_string(line) + ": " + msg);
    }
    float number() {
        if (pos >= tok.size() || tok[pos].kind != Token::Number) fail("expected a number");
        return std::strtof(tok[pos++].text.c_str(), nullptr);
    }
    void numbers(float *out, int n) {
        const bool br = pos < tok.size() && tok[pos].kind == Token::Open;
        if (br) ++pos;
        for (int i = 0; i < n; ++i) out[i] = number();
        if (br) { if (pos >= tok.size() || tok[pos].kind != Token::Close) fail("expected ]"); ++pos; }
    }
    std::string str() {
        if (pos >= tok.size() || tok[pos].kind != Token::String) fail("expected a quoted string");
        return tok[pos++].text;
    }
    // the parameter list that follows: everything up to the next directive word (bare true / false belong to the list),
    // re-assembled for ParameterDictionary::Parse
    ParameterDictionary params_with_bare_bools() {
        std::string text;
        while (pos < tok.size()) {
            if (tok[pos].kind == Token::Word && tok[pos].text == "Include" && pos + 1 < tok.size() && tok[pos + 1].kind == Token::String) {
                // beyond pbrt (whose Include is a directive only): an Include INSIDE a parameter list splices the file's parameters in,
                // so that the block `nanovdb2pbrt` prints can stay in its own file: MakeNamedMedium "c" "string type" "uniformgrid" Include "grid.pbrt"
                ++pos;
                splice_include();
                continue;
            }
            if (!(tok[pos].kind != Token::Word || tok[pos].text == "true" || tok[pos].text == "false")) break;
            const Token &t = tok[pos++];
            if (t.kind == Token::String) text += "\"" + t.text + "\" ";
            else text += t.text + " ";
        }
        return ParameterDictionary::Parse(text);
    }
    // pbrt's Include (parser.cpp): the named file's tokens take the directive's place.  Relative names resolve against the
    // including scene file's directory.
    void splice_include() {
        std::string name = str();
        if (!name.empty() && name[0] != '/' && !baseDir.empty()) name = baseDir + "/" + name;
        if (++includeDepth > 16) fail("Include nested deeper than 16 files");
        std::ifstream f(name);
        if (!f) fail("Include \"" + name + "\": cannot open");
        std::stringstream ss;
        ss << f.rdbuf();
        const std::vector<Token> inc = tokenize(ss.str());
        tok.insert(tok.begin() + (std::ptrdiff_t)pos, inc.begin(), inc.end());
    }
    void concat(const M4 &t) { gs.ctm = mul(gs.ctm, t); }

    void directive() {
        if (tok[pos].kind != Token::Word) fail("expected a directive, found \"" + tok[pos].text + "\"");
        const std::string d = tok[pos++].text;
        if (d == "LookAt") {
            float v[9];
            numbers(v, 9);
            if (world || !is_identity(gs.ctm)) fail("LookAt is supported as the camera's only transform");
            std::memcpy(eye, v, 12); std::memcpy(look, v + 3, 12); std::memcpy(up, v + 6, 12);
            haveLookAt = true;
        } else if (d == "Camera") {
            const std::string type = str();
            ParameterDictionary p = params_with_bare_bools();
            // PerspectiveCamera / OrthographicCamera / SphericalCamera::Create (cameras.cpp:366-407, :459-509, :638-692)
            if (type == "realistic") fail("Camera \"realistic\" (RealisticCamera) is outside this build's scope");
            if (type != "perspective" && type != "orthographic" && type != "spherical")
                fail("Camera \"" + type + "\": only \"perspective\", \"orthographic\" and \"spherical\" are inside this build's scope");
            if (type == "perspective") fov = p.GetOneFloat("fov", 90.f);
            const float lensradius = p.GetOneFloat("lensradius", 0.f);
            const float focaldistance = p.GetOneFloat("focaldistance", type == "spherical" ? 1e30f : 1e6f);
            frameAspect = p.GetOneFloat("frameaspectratio", 0.f);   // (0: the film's, known at the end of the file)
            screenWindow = p.GetFloatArray("screenwindow");
            if (!screenWindow.empty() && screenWindow.size() != 4) fail("\"screenwindow\" should have four values");
            VspgCameraModel &cm = sd->cameraModel;
            cm.model = VSPG_CAMERA_PERSPECTIVE, cm.lens_radius = 0.f, cm.focal_distance = 0.f;
            if (type == "spherical") {  // (the lens parameters and the window are read and not used, as the reference does)
                const std::string mapping = p.GetOneString("mapping", "equalarea");
                if (mapping == "equalarea") cm.model = VSPG_CAMERA_SPHERICAL_EQUALAREA;
                else if (mapping == "equirectangular") cm.model = VSPG_CAMERA_SPHERICAL_EQUIRECT;
                else fail("Camera \"spherical\": unknown mapping \"" + mapping + "\" (\"equalarea\" or \"equirectangular\")");
            } else {
                cm.model = type == "orthographic" ? VSPG_CAMERA_ORTHOGRAPHIC : VSPG_CAMERA_PERSPECTIVE;
                if (!(lensradius >= 0) || !std::isfinite(lensradius)) fail("Camera: \"lensradius\" must be finite and not negative");
                if (lensradius > 0) {
                    if (!(focaldistance > 0) || !std::isfinite(focaldistance)) fail("Camera: \"focaldistance\" must be finite and positive under a lens");
                    cm.lens_radius = lensradius, cm.focal_distance = focaldistance;
                }
            }
            p.ReportUnused();
            haveCamera = true;
            cameraMedium = gs.outsideMedium;  // the camera takes the current OUTSIDE medium (scene.cpp:153-155, 664-665)
        } else if (d == "Sampler") {
            const std::string sname = str();  // every sampler is run as "independent": the path's parity is defined on it (samplers.h:442-476)
            if (sname != "independent") sd->warnings.push_back("Sampler \"" + sname + "\" runs as \"independent\"");
            ParameterDictionary p = params_with_bare_bools();
            sd->pixelSamples = p.GetOneInt("pixelsamples", 16);
            sd->seed = p.GetOneInt("seed", 0);
            p.ReportUnused();
        } else if (d == "PixelFilter") {
            const std::string type = str();
            ParameterDictionary p = params_with_bare_bools();
            if (type != "box") fail("PixelFilter \"" + type + "\": the film accumulates with pbrt's box filter of radius 0.5 only");
            if (p.GetOneFloat("radius", 0.5f) != 0.5f || p.GetOneFloat("xradius", 0.5f) != 0.5f || p.GetOneFloat("yradius", 0.5f) != 0.5f)
                fail("box filter radius must be 0.5");
            p.ReportUnused();
        } else if (d == "Film") {
            const std::string type = str();
            ParameterDictionary p = params_with_bare_bools();
            if (type != "rgb") fail("Film \"" + type + "\": only \"rgb\" is inside this build's scope");
            sd->xres = p.GetOneInt("xresolution", 1280);
            sd->yres = p.GetOneInt("yresolution", 720);
            sd->filmFilename = p.GetOneString("filename", "pbrt.pfm");
            sd->saveFP16 = p.GetOneBool("savefp16", true);
            sd->cropWindow = p.GetFloatArray("cropwindow");
            sd->pixelBoundsParam = p.GetIntArray("pixelbounds");   // (resolved once the command line is known: ResolvePixelBounds)
            p.ReportUnused();
        } else if (d == "Integrator") {
            sd->integratorName = str();
            sd->integratorParams = params_with_bare_bools();
        } else if (d == "Option" && pos < tok.size() && tok[pos].kind == Token::String && tok[pos].text == "bool disabletexturefiltering") {
            // Options->disableTextureFiltering (options.h): every texture lookup reads level 0 -- the only evaluation this build has
            ++pos;
            const bool br = pos < tok.size() && tok[pos].kind == Token::Open;
            if (br) ++pos;
            if (pos >= tok.size() || tok[pos].kind != Token::Word || (tok[pos].text != "true" && tok[pos].text != "false")) fail("Option \"bool disabletexturefiltering\": expected true or false");
            sd->disableTextureFiltering = tok[pos++].text == "true";
            if (br) { if (pos >= tok.size() || tok[pos].kind != Token::Close) fail("expected ]"); ++pos; }
        } else if (d == "Option" || d == "ColorSpace") {
            std::string what = d;
            while (pos < tok.size() && tok[pos].kind != Token::Word) what += " " + tok[pos++].text;
            sd->warnings.push_back("ignored: " + what);
        } else if (d == "Texture") {
            const std::string name = str(), type = str(), cls = str();
            ParameterDictionary p = params_with_bare_bools();
            texture(name, type, cls, p);
        } else if (d == "WorldBegin") {
            if (!haveCamera) fail("WorldBegin before Camera");
            world = true;
            gs.ctm = identity();
        } else if (d == "AttributeBegin" || d == "TransformBegin") {
            stack.push_back(gs);
        } else if (d == "AttributeEnd" || d == "TransformEnd") {
            if (stack.empty()) fail(d + " without a matching Begin");
            gs = stack.back();
            stack.pop_back();
        } else if (d == "Identity") {
            gs.ctm = identity();
        } else if (d == "Translate") {
            float v[3]; numbers(v, 3); concat(translate(v[0], v[1], v[2]));
        } else if (d == "Scale") {
            float v[3]; numbers(v, 3); concat(scale(v[0], v[1], v[2]));
        } else if (d == "Rotate") {
            float v[4]; numbers(v, 4); concat(rotate(v[0], v[1], v[2], v[3]));
        } else if (d == "Transform" || d == "ConcatTransform") {
            float v[16]; numbers(v, 16);
            M4 t;
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < 4; ++j) t.m[i][j] = v[4 * j + i];  // the file lists the matrix column by column (parser.cpp: Transpose)
            if (t.m[3][0] != 0 || t.m[3][1] != 0 || t.m[3][2] != 0 || t.m[3][3] != 1) fail("projective transforms are outside this build's scope");
            if (d == "Transform") gs.ctm = t; else concat(t);
        } else if (d == "ReverseOrientation") {
            gs.reverseOrientation = !gs.reverseOrientation;
        } else if (d == "Material") {
            const std::string type = str();
            ParameterDictionary p = params_with_bare_bools();
            set_material(type, p);
        } else if (d == "MakeNamedMaterial") {
            const std::string name = str();
            materials[name] = params_with_bare_bools();
        } else if (d == "NamedMaterial") {
            const std::string name = str();
            auto it = materials.find(name);
            if (it == materials.end()) fail("NamedMaterial \"" + name + "\" is not defined");
            ParameterDictionary p = it->second;
            set_material(p.GetOneString("type", "diffuse"), p);
        } else if (d == "AreaLightSource") {
            const std::string type = str();
            ParameterDictionary p = params_with_bare_bools();
            if (type != "diffuse") fail("AreaLightSource \"" + type + "\": only \"diffuse\"");
            float L[3] = {1, 1, 1};
            p.GetOneRGB("L", L);
            const float sc = p.GetOneFloat("scale", 1.f);
            gs.twoSided = p.GetOneBool("twosided", false);
            p.ReportUnused();
            for (int k = 0; k < 3; ++k) gs.Le[k] = L[k] * sc;
            gs.areaLight = true;
        } else if (d == "LightSource") {
            const std::string type = str();
            ParameterDictionary p = params_with_bare_bools();
            light_source(type, p);
        } else if (d == "MakeNamedMedium") {
            const std::string name = str();
            NamedMedium m;
            m.params = params_with_bare_bools();
            m.type = m.params.GetOneString("type", "");
            m.ctm = gs.ctm;
            media[name] = m;
        } else if (d == "MediumInterface") {
            gs.insideMedium = str();
            gs.outsideMedium = pos < tok.size() && tok[pos].kind == Token::String ? str() : gs.insideMedium;
        } else if (d == "Shape") {
            const std::string type = str();
            ParameterDictionary p = params_with_bare_bools();
            shape(type, p);
        } else if (d == "Include") {
            splice_include();
        } else {
            fail("directive \"" + d + "\" is outside this build's scope");
        }
    }
    void set_material(const std::string &type, ParameterDictionary &p) {
        if (type == "interface" || type == "none" || type.empty()) {  // a null Material (scene.cpp:1340, materials.cpp:736): medium boundaries
            (void)p.GetOneString("type", "");
            p.ReportUnused();
            gs.interfaceMaterial = true;
            return;
        }
        if (type != "diffuse") fail("Material \"" + type + "\": only \"diffuse\" and \"interface\" are inside this build's scope");
        gs.interfaceMaterial = false;
        gs.texture = 0;
        float kd[3] = {0.5f, 0.5f, 0.5f};
        if (p.Has("texture reflectance")) {  // a named spectrum texture (Texture "name" "spectrum" "imagemap") replaces the constant
            const std::string tname = p.GetOneString("texture reflectance", "");
            auto it = textures.find(tname);
            if (it == textures.end()) fail("Material \"diffuse\": texture \"" + tname + "\" is not defined (a \"spectrum\" \"imagemap\" Texture)");
            if (p.Has("reflectance")) fail("Material \"diffuse\": \"reflectance\" is given twice (a value and a texture)");
            gs.texture = it->second;
        } else if (!p.GetOneRGB("reflectance", kd) && p.Has("reflectance")) { const float f = p.GetOneFloat("reflectance", 0.5f); kd[0] = kd[1] = kd[2] = f; }
        (void)p.GetOneString("type", "");
        p.ReportUnused();
        std::memcpy(gs.Kd, kd, sizeof kd);
    }
    // LightSource "point" (PointLight::Create, lights.cpp:224-248): I, scale, power, from under the current CTM.  Under
    // PBRT_RGB_RENDERING SpectrumToPhotometric is 1 (util/spectrum.cpp:48-49), so the record's I is I * scale with `power` folded into
    // the scale as Create does.  The transform is the library's (vspg_point_light_at): ctm * Translate(from).
    void point_light(ParameterDictionary &p) {
        if (sd->scene.n_point_lights >= VSPG_MAX_POINT_LIGHTS) fail("too many point lights");
        VspgPointLight &pl = sd->scene.point_lights[sd->scene.n_point_lights];
        std::memset(&pl, 0, sizeof pl);
        pl.type = VSPG_LIGHT_POINT;
        float I[3] = {1, 1, 1}, from[3] = {0, 0, 0};
        p.GetOneRGB("I", I);
        float sc = p.GetOneFloat("scale", 1.f);
        const float phi_v = p.GetOneFloat("power", -1.f);
        if (phi_v > 0) {
            const float k_e = 4 * 3.14159265358979323846f;
            sc *= phi_v / k_e;
        }
        p.GetOnePoint3("from", from);
        p.ReportUnused();
        for (int k = 0; k < 3; ++k) pl.I[k] = I[k] * sc;
        float ctm[16];
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) ctm[4 * i + j] = gs.ctm.m[i][j];
        if (vspg_point_light_at(&pl, from, ctm) != 0) fail(std::string("LightSource \"point\": ") + vspg_last_error());
        sd->scene.n_point_lights++;
    }
    void ctm16(float ctm[16]) const {
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) ctm[4 * i + j] = gs.ctm.m[i][j];
    }
    // The image of a projection / goniometric light, by the host Image layer (.pfm, .exr); the checks of lights.cpp:502-510 / :669-678
    Image light_image(const std::string &what, std::string fn) {
        if (fn[0] != '/' && !baseDir.empty()) fn = baseDir + "/" + fn;  // ResolveFilename
        Image img = ReadImage(fn);
        for (float v : img.data) {
            if (std::isinf(v)) fail(fn + ": image has infinite pixel values and so is not suitable as a light.");
            if (v != v) fail(fn + ": image has not-a-number pixel values and so is not suitable as a light.");
        }
        if (img.xres > VSPG_LIGHT_IMAGE_MAX_RES || img.yres > VSPG_LIGHT_IMAGE_MAX_RES)
            fail(fn + ": " + what + " images above " + std::to_string(VSPG_LIGHT_IMAGE_MAX_RES) + " texels a side are outside this build's scope");
        return img;
    }
    // LightSource "projection" (ProjectionLight::Create, lights.cpp:490-560): scale, fov, filename under the current CTM, flipped in y by the
    // library (vspg_projection_light_at).  The record's I is the scale as an RGB multiplier of the texels (SpectrumToPhotometric is 1
    // under PBRT_RGB_RENDERING).  "power" is refused: its normalisation weighs the texels with the colour space's LuminanceVector, which
    // the reference computes at run time and nothing here can pin.
    void projection_light(ParameterDictionary &p) {
        if (sd->scene.n_point_lights >= VSPG_MAX_POINT_LIGHTS) fail("too many point lights");
        const int slot = sd->scene.n_point_lights;
        VspgPointLight &pl = sd->scene.point_lights[slot];
        std::memset(&pl, 0, sizeof pl);
        pl.type = VSPG_LIGHT_PROJECTION;
        const float sc = p.GetOneFloat("scale", 1.f);
        if (p.Has("power")) fail("LightSource \"projection\": \"power\" is outside this build's scope (its normalisation needs the colour space's luminance vector; give \"scale\")");
        const float fov = p.GetOneFloat("fov", 90.f);
        const std::string fn = p.GetOneString("filename", "");
        p.ReportUnused();
        if (fn.empty()) fail("Must provide \"filename\" to \"projection\" light source");  // lights.cpp:498-499
        if (!(fov > 0 && fov < 180)) fail("LightSource \"projection\": \"fov\" must lie in (0, 180)");
        const Image img = light_image("projection", fn);
        for (const char *c : {"R", "G", "B"})
            if (img.ChannelIndex(c) < 0) fail("Image provided to \"projection\" light must have R, G, and B channels.");  // :514-517
        SceneDescription::LightImage li;
        li.slot = slot; li.xres = img.xres; li.yres = img.yres; li.channels = 3;
        li.pixels = img.Gather({"R", "G", "B"}, fn);
        sd->lightImages.push_back(std::move(li));
        for (int k = 0; k < 3; ++k) pl.I[k] = sc;
        float ctm[16];
        ctm16(ctm);
        if (vspg_projection_light_at(&pl, ctm) != 0) fail(std::string("LightSource \"projection\": ") + vspg_last_error());
        pl.cone_angle_deg = fov;  // a projection slot's field of view (include/vspg.h)
        sd->scene.n_point_lights++;
    }
    // LightSource "goniometric" (GoniometricLight::Create, lights.cpp:652-734): I, scale, power, filename under the current CTM with y and z
    // swapped by the library (vspg_goniometric_light_at).  An RGB image is averaged to Y, a Y image is taken as it is (:687-709); without a
    // file name the reference warns and goes on with an empty image, here with the 1 x 1 image of ones the renderer is created with.
    void goniometric_light(ParameterDictionary &p) {
        if (sd->scene.n_point_lights >= VSPG_MAX_POINT_LIGHTS) fail("too many point lights");
        const int slot = sd->scene.n_point_lights;
        VspgPointLight &pl = sd->scene.point_lights[slot];
        std::memset(&pl, 0, sizeof pl);
        pl.type = VSPG_LIGHT_GONIOMETRIC;
        float I[3] = {1, 1, 1};
        p.GetOneRGB("I", I);
        float sc = p.GetOneFloat("scale", 1.f);
        const float phi_v = p.GetOneFloat("power", -1.f);
        const std::string fn = p.GetOneString("filename", "");
        p.ReportUnused();
        SceneDescription::LightImage li;
        li.slot = slot; li.xres = li.yres = 1; li.channels = 1;
        li.pixels.assign(1, 1.f);
        if (fn.empty()) {
            sd->warnings.push_back("No \"filename\" parameter provided for goniometric light: a 1 x 1 image of ones (a point light)");
        } else {
            const Image img = light_image("goniometric", fn);
            if (img.xres != img.yres)  // lights.cpp:680-685
                fail(fn + ": image resolution (" + std::to_string(img.xres) + ", " + std::to_string(img.yres) +
                     ") is non-square. It's unlikely this is an equal-area environment map.");
            const bool rgb = img.ChannelIndex("R") >= 0 && img.ChannelIndex("G") >= 0 && img.ChannelIndex("B") >= 0, y = img.ChannelIndex("Y") >= 0;
            if (rgb && y) fail(fn + ": has both \"R\", \"G\", and \"B\" or \"Y\" channels.");
            if (!rgb && !y) fail(fn + ": has neither \"R\", \"G\", and \"B\" or \"Y\" channels.");
            li.xres = li.yres = img.xres;
            if (y) {
                li.pixels = img.Gather({"Y"}, fn);
            } else {
                const std::vector<float> c = img.Gather({"R", "G", "B"}, fn);
                li.pixels.resize(c.size() / 3);
                for (size_t i = 0; i < li.pixels.size(); ++i) {  // ImageChannelValues::Average (util/image.h:205-210)
                    float sum = 0;
                    for (int k = 0; k < 3; ++k) sum += c[3 * i + k];
                    li.pixels[i] = sum / 3;
                }
            }
            sd->lightImages.push_back(li);
        }
        if (phi_v > 0) {  // lights.cpp:714-722
            float sumY = 0;
            for (float v : li.pixels) sumY += v;
            const float k_e = 4 * 3.14159265358979323846f * sumY / (float)(li.xres * li.yres);
            sc *= phi_v / k_e;
        }
        for (int k = 0; k < 3; ++k) pl.I[k] = I[k] * sc;
        float ctm[16];
        ctm16(ctm);
        if (vspg_goniometric_light_at(&pl, ctm) != 0) fail(std::string("LightSource \"goniometric\": ") + vspg_last_error());
        sd->scene.n_point_lights++;
    }
    void light_source(const std::string &type, ParameterDictionary &p) {
        if (type == "point") { point_light(p); return; }
        if (type == "projection") { projection_light(p); return; }
        if (type == "goniometric") { goniometric_light(p); return; }
        // (The library, its binding and vspg_spot_light_look_at carry everything a "spot" needs; the reader does not accept it yet.)
        if (type == "spot")
            fail("LightSource \"spot\": not read from scene files yet -- build the scene through the C-ABI (VspgScene.point_lights, vspg_spot_light_look_at)");
        if (sd->scene.n_infinite_lights >= VSPG_MAX_INFINITE_LIGHTS) fail("too many infinite lights");
        VspgInfiniteLight &il = sd->scene.infinite_lights[sd->scene.n_infinite_lights];
        float L[3] = {1, 1, 1};
        p.GetOneRGB("L", L);
        const float sc = p.GetOneFloat("scale", 1.f);
        if (type == "infinite") {
            // Light::Create, "infinite" (lights.cpp:1618-1750).  `scale /= SpectrumToPhotometric(illuminant)` is the same step in the
            // uniform and in the image branch (:1629, :1652, :1717), and under PBRT_RGB_RENDERING SpectrumToPhotometric is `return 1.f`
            // (util/spectrum.cpp:48-49): the uniform branch below takes L * scale as it stands, and so does the image branch.
            std::string fn = p.GetOneString("filename", "");
            if (!p.GetPoint3Array("portal").empty()) fail("LightSource \"infinite\": \"portal\" (PortalImageInfiniteLight) is outside this build's scope");
            if (p.Has("illuminance")) fail("LightSource \"infinite\": \"illuminance\" is outside this build's scope (give \"scale\")");
            il.w_light[0] = 0; il.w_light[1] = 1; il.w_light[2] = 0;
            if (fn.empty()) {
                il.type = VSPG_LIGHT_UNIFORM_INFINITE;
            } else {
                if (p.Has("L")) fail("Can't specify both emission \"L\" and \"filename\" with ImageInfiniteLight");  // lights.cpp:1647
                if (fn[0] != '/' && !baseDir.empty()) fn = baseDir + "/" + fn;  // ResolveFilename
                const Image img = ReadImage(fn);
                for (const char *c : {"R", "G", "B"})
                    if (img.ChannelIndex(c) < 0) fail(fn + ": image provided to \"infinite\" light must have R, G, and B channels.");  // :1710-1714
                if (img.xres != img.yres)  // lights.cpp:1096-1099
                    fail(fn + ": image resolution (" + std::to_string(img.xres) + ", " + std::to_string(img.yres) +
                         ") is non-square. It's unlikely this is an equal area environment map.");
                if (img.xres > VSPG_ENV_MAX_RES) fail(fn + ": environment maps above " + std::to_string(VSPG_ENV_MAX_RES) + " texels a side are outside this build's scope");
                SceneDescription::EnvImage e;
                e.light = sd->scene.n_infinite_lights;
                e.res = img.xres;
                e.rgb = img.Gather({"R", "G", "B"}, fn);
                for (float v : e.rgb) {  // lights.cpp:1694-1703
                    if (std::isinf(v)) fail(fn + ": image has infinite pixel values and so is not suitable as a light.");
                    if (v != v) fail(fn + ": image has not-a-number pixel values and so is not suitable as a light.");
                }
                for (int i = 0; i < 3; ++i)
                    for (int j = 0; j < 4; ++j) e.renderFromLight[4 * i + j] = gs.ctm.m[i][j];
                sd->envImages.push_back(std::move(e));
                il.type = VSPG_LIGHT_IMAGE_INFINITE;
                L[0] = L[1] = L[2] = 1.f;  // the multiplier is `scale` alone
            }
        } else if (type == "distant") {
            float from[3] = {0, 0, 0}, to[3] = {0, 0, 1};
            p.GetOnePoint3("from", from);
            p.GetOnePoint3("to", to);
            // DistantLight::Create (lights.cpp): the light shines along (to - from); SampleLi's wi points back towards `from`
            const float w[3] = {from[0] - to[0], from[1] - to[1], from[2] - to[2]};
            float wr[3];
            xf_vector(gs.ctm, w, wr);
            const float l = std::sqrt(wr[0] * wr[0] + wr[1] * wr[1] + wr[2] * wr[2]);
            if (!(l > 0)) fail("distant light: from == to");
            for (int k = 0; k < 3; ++k) il.w_light[k] = wr[k] / l;
            il.type = VSPG_LIGHT_DISTANT;
        } else {
            fail("LightSource \"" + type + "\": only \"infinite\", \"distant\", \"point\", \"projection\" and \"goniometric\" are inside this build's scope");
        }
        p.ReportUnused();
        for (int k = 0; k < 3; ++k) il.L[k] = L[k] * sc;
        sd->scene.n_infinite_lights++;
    }
    // Texture "name" "spectrum" "imagemap" (SpectrumImageTexture::Create, textures.cpp; TextureMapping2D::Create "uv"; include/vspg.h
    // VspgTexture): the image by the host Image layer, everything else as the reference names and defaults it
    void texture(const std::string &name, const std::string &type, const std::string &cls, ParameterDictionary &p) {
        if (type == "float") fail("Texture \"" + name + "\": \"float\" textures are outside this build's scope (\"spectrum\" \"imagemap\" on a diffuse reflectance only)");
        if (type != "spectrum") fail("Texture \"" + name + "\": texture type \"" + type + "\" is outside this build's scope (\"spectrum\" only)");
        if (cls != "imagemap") fail("directive \"Texture\" with class \"" + cls + "\" is outside this build's scope (Texture \"" + name + "\": \"imagemap\" only)");
        if (sd->textures.n_textures >= VSPG_MAX_TEXTURES) fail("more than " + std::to_string(VSPG_MAX_TEXTURES) + " textures");
        const std::string mapping = p.GetOneString("mapping", "uv");
        if (mapping != "uv") fail("Texture \"" + name + "\": mapping \"" + mapping + "\" is outside this build's scope (\"uv\" only)");
        std::string fn = p.GetOneString("filename", "");
        const std::string filter = p.GetOneString("filter", "bilinear"), wrap = p.GetOneString("wrap", "repeat");
        VspgTexture t;
        std::memset(&t, 0, sizeof t);
        t.scale = p.GetOneFloat("scale", 1.f);
        t.invert = p.GetOneBool("invert", false) ? 1 : 0;
        t.su = p.GetOneFloat("uscale", 1.f); t.sv = p.GetOneFloat("vscale", 1.f);
        t.du = p.GetOneFloat("udelta", 0.f); t.dv = p.GetOneFloat("vdelta", 0.f);
        (void)p.GetOneFloat("maxanisotropy", 8.f);   // read and ignored: level 0 has no ellipse
        (void)p.GetOneString("encoding", "sRGB");    // read and ignored: float images carry linear values
        p.ReportUnused();
        if (filter == "point") t.filter = VSPG_TEXFILTER_POINT;
        else if (filter == "bilinear" || filter == "trilinear" || filter == "ewa" || filter == "EWA") t.filter = VSPG_TEXFILTER_BILINEAR;  // all Bilerp(0, st) at level 0
        else fail("Texture \"" + name + "\": filter \"" + filter + "\" unknown");
        if (wrap == "repeat") t.wrap = VSPG_TEXWRAP_REPEAT;
        else if (wrap == "clamp") t.wrap = VSPG_TEXWRAP_CLAMP;
        else if (wrap == "black") t.wrap = VSPG_TEXWRAP_BLACK;
        else fail("Texture \"" + name + "\": wrap mode \"" + wrap + "\" is outside this build's scope (\"repeat\", \"clamp\", \"black\")");
        if (fn.empty()) fail("Texture \"" + name + "\": \"imagemap\" needs a \"filename\"");
        const size_t dot = fn.find_last_of('.');
        const std::string ext = dot == std::string::npos ? "" : fn.substr(dot);
        if (ext != ".pfm" && ext != ".exr") fail("Texture \"" + name + "\": " + fn + ": 8-bit images and colour encodings are outside this build's scope (.pfm / .exr float images only)");
        if (fn[0] != '/' && !baseDir.empty()) fn = baseDir + "/" + fn;  // ResolveFilename
        const Image img = ReadImage(fn);
        const bool rgb = img.ChannelIndex("R") >= 0 && img.ChannelIndex("G") >= 0 && img.ChannelIndex("B") >= 0;
        if (!rgb && img.ChannelIndex("Y") < 0) fail(fn + ": a texture image needs R, G and B channels, or Y");
        t.xres = img.xres; t.yres = img.yres; t.channels = rgb ? 3 : 1;
        sd->texturePixels.push_back(rgb ? img.Gather({"R", "G", "B"}, fn) : img.Gather({"Y"}, fn));
        sd->textures.textures[sd->textures.n_textures++] = t;   // (finish() points `pixels` at the stored image)
        textures[name] = sd->textures.n_textures;
    }
    void add_triangle(const float *a, const float *b, const float *c, const float *uva = nullptr, const float *uvb = nullptr, const float *uvc = nullptr) {
        if (gs.areaLight) fail("emissive triangles are outside this build's scope (emission lives on rectangles: use a planar \"bilinearmesh\" patch)");
        const float *v[3] = {a, b, c};
        for (int i = 0; i < 3; ++i)
            for (int k = 0; k < 3; ++k) sd->triP.push_back(v[i][k]);
        for (int k = 0; k < 3; ++k) sd->triKd.push_back(gs.Kd[k]);
        // the geometric normal Normalize(Cross(p0 - p2, p1 - p2)) flips with reverseOrientation ^ transformSwapsHandedness
        // (shapes.h:934-936) -- the vertices above are already in render space, as the reference's TriangleMesh keeps them
        sd->triFlags.push_back((gs.interfaceMaterial ? VSPG_TRI_INTERFACE : 0) | (gs.reverseOrientation != swaps_handedness(gs.ctm) ? VSPG_TRI_FLIP_NORMAL : 0));
        triMedia.push_back(MediumNames{gs.insideMedium, gs.outsideMedium});
        sd->triTexture.push_back(gs.texture);
        static const float def[3][2] = {{0, 0}, {1, 0}, {1, 1}};   // Triangle::InteractionFromIntersection's default uv
        const float *uv[3] = {uva ? uva : def[0], uvb ? uvb : def[1], uvc ? uvc : def[2]};
        for (int i = 0; i < 3; ++i)
            for (int k = 0; k < 2; ++k) sd->triUv.push_back(uv[i][k]);
    }
    static bool swaps_handedness(const M4 &m) {  // Transform::SwapsHandedness (util/transform.cpp): det of the upper 3x3 < 0
        const float det = m.m[0][0] * (m.m[1][1] * m.m[2][2] - m.m[1][2] * m.m[2][1]) - m.m[0][1] * (m.m[1][0] * m.m[2][2] - m.m[1][2] * m.m[2][0]) +
                          m.m[0][2] * (m.m[1][0] * m.m[2][1] - m.m[1][1] * m.m[2][0]);
        return det < 0;
    }
    void shape(const std::string &type, ParameterDictionary &p) {
        if (!world) fail("Shape before WorldBegin");
        // MediumInterface (round 4): the shape keeps its inside / outside medium NAMES; finish() turns them into "the scene's medium"
        // or "no medium" once it is known which medium the scene holds (this build holds one: a second one is refused there).
        if (gs.interfaceMaterial && gs.areaLight) fail("an area light on a shape with the \"interface\" material is outside this build's scope");
        if (type == "sphere") {
            const float radius = p.GetOneFloat("radius", 1.f);
            const float zmin = p.GetOneFloat("zmin", -radius), zmax = p.GetOneFloat("zmax", radius), phimax = p.GetOneFloat("phimax", 360.f);
            p.ReportUnused();
            if (!(radius > 0)) fail("sphere: radius must be positive");
            if (zmin > -radius || zmax < radius || phimax < 360.f) fail("partial spheres (zmin / zmax / phimax) are outside this build's scope");
            // (The library and its binding carry sphere area lights; the reader does not accept them yet.)
            if (gs.areaLight)
                fail("emissive spheres are not read from scene files yet -- build the scene through the C-ABI (VspgScene.sphere_Le / sphere_two_sided; "
                     "add_sphere_light in the Python binding)");
            if (gs.texture)
                fail("Shape \"sphere\" with a textured material (\"texture reflectance\"): textures on spheres are outside this build's scope");
            if (spheres.size() >= VSPG_MAX_SPHERES) fail("more than " + std::to_string(VSPG_MAX_SPHERES) + " spheres");
            VspgSphere sp;
            std::memset(&sp, 0, sizeof sp);
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < 4; ++j) sp.render_from_object[4 * i + j] = gs.ctm.m[i][j];
            if (vspg_transform_inverse(sp.render_from_object, sp.object_from_render) != 0) fail(std::string("sphere: ") + vspg_last_error());
            sp.radius = radius;
            for (int k = 0; k < 3; ++k) sp.Kd[k] = gs.Kd[k];
            sp.reverse_orientation = gs.reverseOrientation;   // (the handedness of the CTM is the library's to find: Sphere's constructor, shapes.h:122)
            sp.material = gs.interfaceMaterial ? VSPG_MATERIAL_INTERFACE : VSPG_MATERIAL_DIFFUSE;
            spheres.push_back(sp);
            sphereMedia.push_back(MediumNames{gs.insideMedium, gs.outsideMedium});
            return;
        }
        std::vector<float> P = p.GetPoint3Array("P");
        if (p.Has("N") || p.Has("S")) fail("shading normals / tangents (\"N\", \"S\") on meshes are outside this build's scope");
        const std::vector<float> uv = p.GetFloatArray("uv");   // "point2 uv": one pair per vertex
        std::vector<float> W(P.size());
        for (size_t i = 0; i + 2 < P.size(); i += 3) xf_point(gs.ctm, &P[i], &W[i]);
        if (type == "bilinearmesh") {
            std::vector<int> idx = p.GetIntArray("indices");
            p.ReportUnused();
            if (idx.empty()) idx = {0, 1, 2, 3};
            if (P.size() % 3) fail("bilinearmesh: \"P\" must hold whole points (a multiple of three floats)");
            if (idx.size() != 4 || W.size() < 12) fail("bilinearmesh: one patch of four points is supported");
            static const float patchUv[4][2] = {{0, 0}, {1, 0}, {0, 1}, {1, 1}};   // BilinearPatch's default parametrisation
            if (!uv.empty()) {
                bool def = uv.size() == 2 * (W.size() / 3);
                for (int k = 0; def && k < 4; ++k)
                    def = idx[k] >= 0 && 2 * (size_t)idx[k] + 1 < uv.size() && uv[2 * idx[k]] == patchUv[k][0] && uv[2 * idx[k] + 1] == patchUv[k][1];
                if (!def) fail("bilinearmesh: only the default \"uv\" (0,0) (1,0) (0,1) (1,1) is inside this build's scope");
            }
            const int nv = (int)(W.size() / 3);
            for (int k = 0; k < 4; ++k)
                if (idx[k] < 0 || idx[k] >= nv) fail("bilinearmesh: vertex index out of range");
            const float *p00 = &W[3 * idx[0]], *p10 = &W[3 * idx[1]], *p01 = &W[3 * idx[2]], *p11 = &W[3 * idx[3]];
            float e1[3], e2[3];
            bool parallelogram = true;
            for (int k = 0; k < 3; ++k) {
                e1[k] = p10[k] - p00[k];
                e2[k] = p01[k] - p00[k];
                parallelogram = parallelogram && std::fabs((p10[k] + e2[k]) - p11[k]) <= 1e-6f * (1 + std::fabs(p11[k]));
            }
            if (parallelogram) {
                if (quads.size() >= VSPG_MAX_QUADS) fail("more than " + std::to_string(VSPG_MAX_QUADS) + " rectangles");
                VspgQuad q;
                std::memset(&q, 0, sizeof q);
                for (int k = 0; k < 3; ++k) { q.p00[k] = p00[k]; q.e1[k] = e1[k]; q.e2[k] = e2[k]; q.Kd[k] = gs.Kd[k]; q.Le[k] = gs.areaLight ? gs.Le[k] : 0.f; }
                q.two_sided = gs.twoSided;
                // BilinearPatch flips n when reverseOrientation ^ transformSwapsHandedness (shapes.h:1163-1164, shapes.cpp:1267-1270):
                // a mirroring CTM turns the patch's parametrisation over
                q.reverse_orientation = gs.reverseOrientation != swaps_handedness(gs.ctm);
                q.material = gs.interfaceMaterial ? VSPG_MATERIAL_INTERFACE : VSPG_MATERIAL_DIFFUSE;
                quads.push_back(q);
                quadTexture.push_back(gs.texture);
                quadMedia.push_back(MediumNames{gs.insideMedium, gs.outsideMedium});
            } else {
                add_triangle(p00, p10, p11, patchUv[0], patchUv[1], patchUv[3]);
                add_triangle(p00, p11, p01, patchUv[0], patchUv[3], patchUv[2]);
            }
        } else if (type == "trianglemesh") {
            // (a triangle's orientation -- reverseOrientation ^ transformSwapsHandedness, shapes.h:934-936 -- travels as a flag: only a
            // medium transition can tell the two sides of a diffuse triangle apart)
            std::vector<int> idx = p.GetIntArray("indices");
            p.ReportUnused();
            if (P.size() % 3) fail("trianglemesh: \"P\" must hold whole points (a multiple of three floats)");
            const int nv = (int)(W.size() / 3);
            if (idx.empty()) { if (nv != 3) fail("trianglemesh without indices must have exactly three points"); idx = {0, 1, 2}; }
            if (idx.size() % 3) fail("trianglemesh: indices come in threes");
            if (!uv.empty() && uv.size() != 2 * (size_t)nv) fail("trianglemesh: \"uv\" must hold one pair per vertex");
            for (size_t i = 0; i < idx.size(); i += 3) {
                for (int k = 0; k < 3; ++k) if (idx[i + k] < 0 || idx[i + k] >= nv) fail("trianglemesh: vertex index out of range");
                if (uv.empty()) add_triangle(&W[3 * idx[i]], &W[3 * idx[i + 1]], &W[3 * idx[i + 2]]);
                else add_triangle(&W[3 * idx[i]], &W[3 * idx[i + 1]], &W[3 * idx[i + 2]], &uv[2 * idx[i]], &uv[2 * idx[i + 1]], &uv[2 * idx[i + 2]]);
            }
        } else {
            fail("Shape \"" + type + "\": only \"bilinearmesh\", \"trianglemesh\" and \"sphere\" are inside this build's scope");
        }
    }
    void finish() {
        if (!haveCamera) throw Error("scene file: no Camera");
        if (!stack.empty()) throw Error("scene file: unbalanced AttributeBegin");
        VspgScene &s = sd->scene;
        s.n_quads = (int)quads.size();
        for (int i = 0; i < s.n_quads; ++i) s.quads[i] = quads[i];
        if (!haveLookAt) { eye[0] = eye[1] = eye[2] = 0; look[0] = 0; look[1] = 0; look[2] = 1; up[0] = 0; up[1] = 1; up[2] = 0; }
        if (vspg_camera_look_at_window(&s.camera, sd->cameraModel.model, eye, look, up, fov, screenWindow.empty() ? nullptr : screenWindow.data(), frameAspect,
                                       sd->xres, sd->yres) != 0)
            throw Error(std::string("Camera: ") + vspg_last_error());
        s.n_spheres = (int)spheres.size();
        for (int i = 0; i < s.n_spheres; ++i) s.spheres[i] = spheres[i];
        // The scene's medium: the library holds ONE (include/vspg.h).  Every name a camera or a shape refers to must be that one
        // (or "", no medium); a second medium is refused by name.
        std::string theMedium = cameraMedium;
        auto see = [&](const std::string &name) {
            if (name.empty()) return;
            if (theMedium.empty()) theMedium = name;
            else if (name != theMedium)
                throw Error("scene file: media \"" + theMedium + "\" and \"" + name + "\" are both in use -- this build renders ONE medium per scene (with or without boundaries)");
        };
        for (const auto *v : {&quadMedia, &sphereMedia, &triMedia})
            for (const MediumNames &m : *v) { see(m.inside); see(m.outside); }
        auto bits = [&](const MediumNames &m) {
            return (!theMedium.empty() && m.inside == theMedium ? VSPG_IFACE_INSIDE : 0) | (!theMedium.empty() && m.outside == theMedium ? VSPG_IFACE_OUTSIDE : 0);
        };
        for (int i = 0; i < s.n_quads; ++i) s.quads[i].medium_interface = bits(quadMedia[i]);
        for (int i = 0; i < s.n_spheres; ++i) s.spheres[i].medium_interface = bits(sphereMedia[i]);
        for (size_t i = 0; i < triMedia.size(); ++i) sd->triFlags[i] |= bits(triMedia[i]) << VSPG_TRI_IFACE_SHIFT;
        s.camera_outside_medium = !theMedium.empty() && cameraMedium != theMedium;   // CameraBase::medium = the outside medium at the Camera directive
        s.medium.type = VSPG_MEDIUM_NONE;
        if (!theMedium.empty()) {
            const std::string cameraMedium = theMedium;   // (the block below creates the scene's medium, whoever named it)
            auto it = media.find(cameraMedium);
            if (it == media.end()) throw Error("medium \"" + cameraMedium + "\" is not defined");
            ParameterDictionary p = it->second.params;
            (void)p.GetOneString("type", "");
            if (it->second.type == "nanovdb") {  // ResolveFilename (media.cpp:686): relative to the scene file's directory
                const std::string fn = p.GetOneString("filename", "");
                if (!fn.empty() && fn[0] != '/' && !baseDir.empty()) p.String("filename", baseDir + "/" + fn);
            }
            s.medium = CreateMedium(it->second.type, p, &sd->density, &sd->leScale, &sd->temperature, &sd->rgb);
            if (s.medium.type == VSPG_MEDIUM_RGBGRID) sd->rgb.Attach(&s);
            if (!is_identity(it->second.ctm)) {
                if (s.medium.type == VSPG_MEDIUM_HOMOGENEOUS) { /* a homogeneous medium has no frame */ }
                else {
                    s.medium.has_transform = 1;
                    for (int i = 0; i < 4; ++i)
                        for (int j = 0; j < 4; ++j) s.medium.render_from_medium[4 * i + j] = it->second.ctm.m[i][j];
                    if (vspg_transform_inverse(s.medium.render_from_medium, s.medium.medium_from_render) != 0)
                        throw Error(std::string("MakeNamedMedium \"") + cameraMedium + "\": " + vspg_last_error());
                }
            }
        }
        if (!sd->triP.empty()) {
            s.n_triangles = (int)(sd->triP.size() / 9);
            s.tri_p = sd->triP.data();
            s.tri_kd = sd->triKd.data();
            s.tri_flags = sd->triFlags.data();
        }
        // image textures: the record beside the scene (vspg_renderer_create_textured)
        VspgSceneTextures &tx = sd->textures;
        for (int k = 0; k < tx.n_textures; ++k) tx.textures[k].pixels = sd->texturePixels[k].data();
        for (int i = 0; i < s.n_quads; ++i) tx.quad_texture[i] = quadTexture[i];
        bool triTextured = false;
        for (int v : sd->triTexture) triTextured = triTextured || v != 0;
        if (triTextured) { tx.tri_texture = sd->triTexture.data(); tx.tri_uv = sd->triUv.data(); }
        if (tx.n_textures > 0 && !sd->disableTextureFiltering)
            sd->warnings.push_back("textures are evaluated at level 0 (point or bilinear), as under Option \"bool disabletexturefiltering\" true");
    }
};

}  // namespace

std::unique_ptr<SceneDescription> ParseSceneString(const std::string &text) { return Parser(text).run(); }
std::unique_ptr<SceneDescription> ParseSceneFile(const std::string &filename) {
    std::ifstream f(filename);
    if (!f) throw Error(filename + ": cannot open");
    std::stringstream ss;
    ss << f.rdbuf();
    const size_t slash = filename.find_last_of('/');
    return Parser(ss.str(), slash == std::string::npos ? std::string(".") : filename.substr(0, slash)).run();
}
std::unique_ptr<Integrator> CreateIntegrator(const SceneDescription &sd, int device) {
    // the bounds a host resolved with its command line, else the file's own (a throw-away copy takes the warnings)
    int b[4] = {sd.boundsX0, sd.boundsY0, sd.boundsX1, sd.boundsY1};
    if (!sd.boundsResolved) {
        SceneDescription own;
        own.xres = sd.xres; own.yres = sd.yres; own.cropWindow = sd.cropWindow; own.pixelBoundsParam = sd.pixelBoundsParam;
        ResolvePixelBounds(own);
        b[0] = own.boundsX0; b[1] = own.boundsY0; b[2] = own.boundsX1; b[3] = own.boundsY1;
    }
    auto integrator = Integrator::Create(sd.integratorName, sd.integratorParams, sd.scene, sd.xres, sd.yres, sd.pixelSamples, sd.seed, device,
                                         sd.textures.n_textures > 0 ? &sd.textures : nullptr);
    integrator->SetPixelBounds(b[0], b[1], b[2], b[3]);
    // a thin lens, an orthographic or a spherical camera is set on the live renderer (a pinhole perspective is what it was created with)
    if (sd.cameraModel.model != VSPG_CAMERA_PERSPECTIVE || sd.cameraModel.lens_radius > 0) integrator->SetCamera(sd.scene.camera, sd.cameraModel);
    for (const SceneDescription::EnvImage &e : sd.envImages) integrator->SetEnvironmentImage(e.light, e.rgb, e.res, e.renderFromLight);
    for (const SceneDescription::LightImage &l : sd.lightImages) integrator->SetLightImage(l.slot, l.pixels, l.xres, l.yres, l.channels);
    return integrator;
}

template <class T>
static std::vector<T> split_numbers(const std::string &arg, const char *option) {
    std::vector<T> v;
    size_t pos = 0;
    while (pos <= arg.size()) {
        const size_t comma = std::min(arg.find(',', pos), arg.size());
        const std::string item = arg.substr(pos, comma - pos);
        char *end = nullptr;
        if (std::is_integral<T>::value) {  // (an integer option takes integers: "1.5" is refused, not truncated)
            const long n = std::strtol(item.c_str(), &end, 10);
            if (item.empty() || *end != 0) throw Error(std::string(option) + ": \"" + item + "\" is not an integer");
            v.push_back((T)n);
        } else {
            const double d = std::strtod(item.c_str(), &end);
            if (item.empty() || *end != 0) throw Error(std::string(option) + ": \"" + item + "\" is not a number");
            v.push_back((T)d);
        }
        pos = comma + 1;
    }
    return v;
}
void ParseCropWindowArg(const std::string &arg, FilmOverrides *o) {
    const std::vector<float> c = split_numbers<float>(arg, "--cropwindow");
    if (c.size() != 4) throw Error("Didn't find four values after --cropwindow");  // cmd/pbrt.cpp:134
    o->haveCropWindow = true;
    for (int i = 0; i < 4; ++i) o->cropWindow[i] = c[i];
}
void ParsePixelBoundsArg(const std::string &arg, FilmOverrides *o) {
    const std::vector<int> p = split_numbers<int>(arg, "--pixelbounds");
    if (p.size() != 4) throw Error("Didn't find four integer values after --pixelbounds");  // cmd/pbrt.cpp:150
    o->havePixelBounds = true;
    for (int i = 0; i < 4; ++i) o->pixelBounds[i] = p[i];
}

void ResolvePixelBounds(SceneDescription &sd, const FilmOverrides &o) {
    const int W = sd.xres, H = sd.yres;
    int x0 = 0, y0 = 0, x1 = W, y1 = H;  // film.cpp:97: the whole frame
    // a Bounds2 built from two corners orders them per axis, and Intersect may leave it empty (film.cpp:100-103, 113-117)
    const auto pixel_bounds = [&](const int pb[4]) {
        const int bx0 = std::min(pb[0], pb[1]), bx1 = std::max(pb[0], pb[1]), by0 = std::min(pb[2], pb[3]), by1 = std::max(pb[2], pb[3]);
        x0 = std::max(bx0, 0); x1 = std::min(bx1, W); y0 = std::max(by0, 0); y1 = std::min(by1, H);
        if (x0 != bx0 || x1 != bx1 || y0 != by0 || y1 != by1) sd.warnings.push_back("Supplied pixel bounds extend beyond image resolution. Clamping.");
    };
    // film.cpp:134-137, 157-166: ceil(resolution * crop) in float, corner by corner
    const auto crop_bounds = [&](float cx0, float cx1, float cy0, float cy1) {
        x0 = (int)std::ceil((float)W * cx0); y0 = (int)std::ceil((float)H * cy0);
        x1 = (int)std::ceil((float)W * cx1); y1 = (int)std::ceil((float)H * cy1);
    };
    const auto clamp01 = [](float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); };
    const bool filePb = !sd.pixelBoundsParam.empty(), fileCrop = !sd.cropWindow.empty();
    if (o.havePixelBounds) {  // film.cpp:99-108
        pixel_bounds(o.pixelBounds);
        if (filePb) sd.warnings.push_back("Pixel bounds supplied on command line will override pixel bounds specified with Film.");
    } else if (filePb) {      // film.cpp:109-120
        if (sd.pixelBoundsParam.size() != 4) throw Error(std::to_string(sd.pixelBoundsParam.size()) + " values supplied for \"pixelbounds\". Expected 4.");
        pixel_bounds(sd.pixelBoundsParam.data());
    }
    if (o.haveCropWindow) {   // film.cpp:123-144
        const float *c = o.cropWindow;
        const float cx0 = std::min(c[0], c[1]), cx1 = std::max(c[0], c[1]), cy0 = std::min(c[2], c[3]), cy1 = std::max(c[2], c[3]);
        if (cx0 < 0.f || cx1 > 1.f || cy0 < 0.f || cy1 > 1.f)
            sd.warnings.push_back("Film crop window is not in [0,1] range; did you mean to use \"pixelbounds\"? Clamping to valid range.");
        crop_bounds(clamp01(cx0), clamp01(cx1), clamp01(cy0), clamp01(cy1));
        if (fileCrop) sd.warnings.push_back("Crop window supplied on command line will override crop window specified with Film.");
        if (o.havePixelBounds || filePb) sd.warnings.push_back("Both pixel bounds and crop window were specified. Using the crop window.");
    } else if (fileCrop) {    // film.cpp:145-168
        if (o.havePixelBounds) {
            sd.warnings.push_back("Ignoring \"cropwindow\" since pixel bounds were specified on the command line.");
        } else if (sd.cropWindow.size() == 4) {
            if (filePb) sd.warnings.push_back("Both pixel bounds and crop window were specified. Using the crop window.");
            const std::vector<float> &c = sd.cropWindow;
            crop_bounds(clamp01(std::min(c[0], c[1])), clamp01(std::max(c[0], c[1])), clamp01(std::min(c[2], c[3])), clamp01(std::max(c[2], c[3])));
        } else {
            throw Error(std::to_string(sd.cropWindow.size()) + " values supplied for \"cropwindow\". Expected 4.");
        }
    }
    if (x1 <= x0 || y1 <= y0)  // film.cpp:170-171
        throw Error("Degenerate pixel bounds provided to film: [ (" + std::to_string(x0) + ", " + std::to_string(y0) + ") - (" + std::to_string(x1) + ", " +
                    std::to_string(y1) + ") ].");
    sd.boundsX0 = x0; sd.boundsY0 = y0; sd.boundsX1 = x1; sd.boundsY1 = y1;
    sd.boundsResolved = true;
}

}  // namespace vspg
