// vspg_host.h -- C++ host adapter: the reference's Integrator / Medium plugin surface for the
// GuidedVolPathVSPG path, implemented on top of the C-ABI (include/vspg.h).
//
// Mirrors (names, argument meaning, defaults, error behaviour):
//   ParameterDictionary::GetOne*/ReportUnused     src/pbrt/paramdict.h, paramdict.cpp:642-664
//   Integrator::Create(name, params, ...)          src/pbrt/cpu/integrators.cpp:3711-3768
//   GuidedVolPathVSPGIntegrator::Create / Render / PostProcessWave / ToString
//                                                  src/pbrt/cpu/guidedvolpathvspgintegrator.cpp:1260-1322, 230-260
//   ImageTileIntegrator::Render wave loop          src/pbrt/cpu/integrators.cpp:75-269 (1-spp waves :239)
//   HomogeneousMedium::Create / Medium::Create     src/pbrt/media.cpp:167-206, 816-841
// The reference aborts the process on fatal errors (ErrorExit); this adapter throws
// vspg::Error with the same trigger conditions so an embedding application can decide.
#pragma once
#include <map>
#include <cstdio>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/vspg.h"

namespace vspg {

struct Error : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// A small typed parameter dictionary: the subset of pbrt's ParameterDictionary the path reads.
class ParameterDictionary {
  public:
    ParameterDictionary &Int(const std::string &n, int v);
    ParameterDictionary &Float(const std::string &n, float v);
    ParameterDictionary &Bool(const std::string &n, bool v);
    ParameterDictionary &String(const std::string &n, const std::string &v);
    ParameterDictionary &RGB(const std::string &n, float r, float g, float b);
    ParameterDictionary &Point3(const std::string &n, float x, float y, float z);
    ParameterDictionary &FloatArray(const std::string &n, std::vector<float> v);
    ParameterDictionary &IntArray(const std::string &n, std::vector<int> v);
    ParameterDictionary &Point3Array(const std::string &n, std::vector<float> xyz);
    ParameterDictionary &RGBArray(const std::string &n, std::vector<float> rgb);   // r g b r g b ... ("rgb name" [ several triples ])
    // The reference's scene-file parameter-list syntax ("type name" value | [ values ]), e.g. the block
    // cmd/nanovdb2pbrt.cpp:97-126 prints for a grid:
    //   "integer nx" 64 "integer ny" 64 "integer nz" 32 "point3 p0" [ -1 -1 0 ] "point3 p1" [ 1 1 1 ] "float density" [ ... ]
    // Types: integer (several -> IntArray), float (one value -> Float, several -> FloatArray), bool, string, rgb,
    // point3 (several points -> Point3Array; several rgb triples -> RGBArray); point2 / vector3 / normal3 arrays are kept as float arrays under their name.
    static ParameterDictionary Parse(const std::string &text);

    int GetOneInt(const std::string &n, int def) const;
    float GetOneFloat(const std::string &n, float def) const;
    bool GetOneBool(const std::string &n, bool def) const;
    std::string GetOneString(const std::string &n, const std::string &def) const;
    // returns false if absent
    bool GetOneRGB(const std::string &n, float rgb[3]) const;
    bool GetOnePoint3(const std::string &n, float p[3]) const;
    std::vector<float> GetFloatArray(const std::string &n) const;  // a single "float" value is a 1-element array
    std::vector<int> GetIntArray(const std::string &n) const;      // a single "integer" value is a 1-element array
    std::vector<float> GetPoint3Array(const std::string &n) const; // x y z x y z ...; a single "point3" is one point
    std::vector<float> GetRGBArray(const std::string &n) const;    // r g b r g b ...; a single "rgb" is one triple (paramdict.h GetRGBArray)
    bool Has(const std::string &n) const { return values.count(n) != 0; }
    // paramdict.cpp:642-664: any parameter that was never looked up is a fatal error
    void ReportUnused() const;

  private:
    struct Value {
        char type;  // i f b s c p a(rray) I(nt array) P(oint array) C(olour array)
        int i = 0;
        std::vector<int> iarr;
        float f[3] = {0, 0, 0};
        std::string s;
        std::vector<float> arr;
        mutable bool lookedUp = false;
    };
    const Value *find(const std::string &n, char type) const;
    std::map<std::string, Value> values;
};

// Medium::Create (media.cpp:816-841): "homogeneous" (HomogeneousMedium::Create :167-206) and "uniformgrid"
// (GridMedium::Create :272-361; the density array is copied into *densityStorage, which must outlive the
// renderer creation -- VspgMedium.density points into it; likewise the "Lescale" and "temperature" grids); "nanovdb"
// (NanoVDBMedium::Create :683-734; its temperature grid goes to temperatureStorage, or to leScaleStorage when that is all the caller
// passed); "rgbgrid" (RGBGridMedium::Create :411-484: its grids live in the tail of VspgScene, not in VspgMedium -- they are copied into
// *rgbStorage, which must outlive the renderer creation and whose Attach() points a scene record at them); other names -> Error:
// outside scope
struct RgbGridStorage {
    std::vector<float> sigma_a, sigma_s, Le;   // 3 * nx * ny * nz floats each, R G B per voxel, x fastest; empty = absent
    float scale = 1.f, Lescale = 1.f;          // "scale" (sigmaScale), "Lescale"
    void Attach(VspgScene *scene) const;       // fills rgb_sigma_a / rgb_sigma_s / rgb_Le / rgb_sigma_scale / rgb_le_scale
};
VspgMedium CreateMedium(const std::string &name, const ParameterDictionary &parameters,
                        std::vector<float> *densityStorage = nullptr, std::vector<float> *leScaleStorage = nullptr,
                        std::vector<float> *temperatureStorage = nullptr, RgbGridStorage *rgbStorage = nullptr);

struct Image;  // vspg_image.h: pbrt's Image by file extension (PFM, OpenEXR)

struct Film {
    int xres = 0, yres = 0;   // the size of the film's pixelBounds: the window that was rendered (the whole frame by default)
    int x0 = 0, y0 = 0;       // ... and its origin in the frame; pixel (x, y) below is relative to it
    std::vector<float> rgbw;  // xres*yres*4: sum w*r, sum w*g, sum w*b, sum w
    // RGBFilm::GetPixelRGB (film.h:269-287) without the output colour transform
    void GetPixelRGB(int x, int y, float rgb[3]) const;
    void WritePFM(const std::string &filename) const;
};

// the pixels [x0, x1) x [y0, y1) of a whole-frame film (xres pixels per row)
Film CropFilm(const std::vector<float> &rgbw, int xres, int x0, int y0, int x1, int y1);

// Guiding-cache file (openpgl::cpp::Field::Store / Field(device, file), guidedvolpathvspgintegrator.cpp:
// 117-128, 210-213).  Format "VSPGFLD1", little endian:
//   char magic[8] = "VSPGFLD1"; uint32 lobes (= VSPG_FIELD_LOBES); uint32 reserved;
//   for field in {surface, volume}: uint32 n_nodes, n_regions;
//   for field in {surface, volume}: VspgKdNode nodes[n_nodes]; VspgFieldRegion regions[n_regions];
// (structs exactly as declared in include/vspg.h).
struct GuidingCache {
    std::vector<VspgKdNode> nodes[2];
    std::vector<VspgFieldRegion> regions[2];
    void Write(const std::string &filename) const;
    static GuidingCache Read(const std::string &filename);
};
struct GuidingCacheSettings {  // "storeGuidingCache" / "loadGuidingCache" / "guidingCacheFileName"
    bool store = false, load = false;
    std::string fileName;
};

// TrBuffer (src/pbrt/cpu/trbuffer.h:17-104): the per-pixel transmittance estimates of the primary rays, kept between
// runs for NDS+.  The reference stores it through pbrt's Image class (format by file extension, normally OpenEXR).
// Store / Load read and write the PFM raster of that class only (util/image.cpp:1756-1800 WritePFM: "PF", width height,
// scale -1 = little endian, RGB float32, scanlines bottom to top) and refuse other extensions.  PFM carries no channel
// names; the reference's EXR layout -- FLOAT channels "Transmittance.R/G/B" (trbuffer.h:52-71) -- goes through ToImage /
// FromImage and vspg_image.h's WriteImage / ReadImage, which is what the integrator does for a "trBufferFileName" ending in .exr.
struct TrBuffer {
    int xres = 0, yres = 0;
    std::vector<float> rgb;  // row-major, top row first, 3 floats per pixel
    void Store(const std::string &filename) const;
    static TrBuffer Load(const std::string &filename);
    Image ToImage() const;                                              // FLOAT, channels Transmittance.R / .G / .B
    static TrBuffer FromImage(const Image &image, const std::string &name);  // by those names; `name` is for the Error
};
// The image-space VSP buffer between runs ("storeISGBuffer" / "loadISGBuffer" / "isgBufferFileName",
// guidedvolpathvspgintegrator.cpp:151-159, 214-216).  OpenPGL's own file format is not part of the reference tree; this
// adapter keeps the one plane the path reads -- the per-pixel volume-scatter-probability estimate -- as a single-channel
// PFM ("Pf", same raster conventions as TrBuffer; a value outside [0,1] = no estimate for the pixel).
struct VspBuffer {
    int xres = 0, yres = 0;
    bool ready = false;
    std::vector<float> vsp;  // row-major, top row first
    void Store(const std::string &filename) const;
    static VspBuffer Load(const std::string &filename);
};
struct IsgBufferSettings {
    bool store = false, load = false;
    std::string fileName;
};
struct TrBufferSettings {  // "storeTrBuffer" / "loadTrBuffer" / "trBufferFileName"
    bool store = false, load = false;
    std::string fileName;
};

// --mse-reference-image (cmd/pbrt.cpp:60-61, ImageTileIntegrator::Render, cpu/integrators.cpp:129-158): the image the film is
// compared with after every wave.  Read with ReadImage (vspg_image.h: PFM or OpenEXR; channels R, G, B by name, half files widened
// exactly).  It has the size of
// the frame -- then the pixel bounds select the part compared (:136-153) -- or exactly the size of the pixel bounds; anything else
// is an Error that names both sizes.  Returned as a frame-sized image (W*H*3, top row first), what vspg_renderer_set_reference_image
// takes; outside the pixel bounds nothing is ever compared.
std::vector<float> LoadMseReferenceImage(const std::string &filename, int xres, int yres, int x0, int y0, int x1, int y1);
// cmd/pbrt.cpp:244-248: each of --mse-reference-image / --mse-reference-out needs the other (throws Error with the reference's words)
void CheckMseReferenceOptions(const std::string &image, const std::string &out);
// The reference's last step on a record's sums (util/image.cpp:603-606 and ImageChannelValues::Average, util/image.h:205-210):
// per channel Float(sum / (Float(width) * Float(height))), then the three averaged in Float.
float FilmErrorAverage(const VspgFilmError &rec, const double sums[3]);

class Integrator {
  public:
    virtual ~Integrator() = default;
    virtual void Render() = 0;
    virtual std::string ToString() const = 0;
    // the film's pixelBounds [x0, x1) x [y0, y1), inside the frame and not empty (film.cpp:97-172; the scene-file reader resolves
    // "cropwindow" / "pixelbounds"): Render() covers these pixels only (integrators.cpp:183).  Default: the whole frame.
    virtual void SetPixelBounds(int x0, int y0, int x1, int y1) = 0;
    // The image of image infinite light `light` (an index into the scene's infinite lights): res * res * 3 floats, top row first, and
    // the rows of renderFromLight (12 floats) or nullptr for the identity (vspg_renderer_set_environment_image).  Throws on refusal.
    virtual void SetEnvironmentImage(int light, const std::vector<float> &rgb, int res, const float *renderFromLight) = 0;
    // The image of the projection / goniometric light in point-light slot `slot`: xres * yres * channels floats, top row first, 3 channels
    // (R, G, B) or 1 (Y) (vspg_renderer_set_light_image).  Throws on refusal.
    virtual void SetLightImage(int slot, const std::vector<float> &pixels, int xres, int yres, int channels) = 0;
    // The camera of the live renderer: a thin lens, an orthographic or a spherical model (vspg_renderer_set_camera).  Throws on refusal.
    virtual void SetCamera(const VspgCamera &camera, const VspgCameraModel &model) = 0;
    // Integrator::Create: "guidedvolpathvspg"; "guidedvolpath" is accepted as an alias ONLY when
    // the dictionary carries "vspguiding" (the option BASELINE.json names), see SURVEY.md 0.1
    static std::unique_ptr<Integrator> Create(const std::string &name, const ParameterDictionary &parameters,
                                              const VspgScene &scene, int xres, int yres, int pixelSamples,
                                              int seed = 0, int device = 0, const VspgSceneTextures *textures = nullptr);
};

class GuidedVolPathVSPGIntegrator : public Integrator {
  public:
    static std::unique_ptr<GuidedVolPathVSPGIntegrator> Create(const ParameterDictionary &parameters,
                                                               const VspgScene &scene, int xres, int yres,
                                                               int pixelSamples, int seed, int device,
                                                               const VspgSceneTextures *textures = nullptr);
    GuidedVolPathVSPGIntegrator(const VspgIntegratorParams &p, const VspgScene &scene, int xres, int yres,
                                int pixelSamples, int seed, int device, const GuidingCacheSettings &cache = {},
                                const TrBufferSettings &tr = {}, const IsgBufferSettings &isg = {},
                                const VspgSceneTextures *textures = nullptr);  // image textures beside the scene (vspg_renderer_create_textured)
    ~GuidedVolPathVSPGIntegrator() override;
    void Render() override;       // wave loop: 1 spp per wave, PostProcessWave after each
    void PostProcessWave();       // guidedvolpathvspgintegrator.cpp:230-260
    std::string ToString() const override;
    Film GetFilm();               // the pixels of the pixel bounds (RGBFilm::WriteImage, film.cpp:541-557)
    void SetPixelBounds(int x0, int y0, int x1, int y1) override;
    void SetEnvironmentImage(int light, const std::vector<float> &rgb, int res, const float *renderFromLight) override;
    void SetLightImage(int slot, const std::vector<float> &pixels, int xres, int yres, int channels) override;
    void SetCamera(const VspgCamera &camera, const VspgCameraModel &model) override;
    VspgCounters Counters();
    VspgTrainStats TrainingStats();      // guideTraining / guiding_field->GetIteration()
    GuidingCache GetGuidingCache();      // the field as it stands (trained in-loop or loaded)
    TrBuffer GetTrBuffer();              // the transmittance buffer as it stands (recorded or loaded)
    VspBuffer GetVspBuffer();            // the image-space VSP estimate as it stands
    const VspgIntegratorParams &Params() const { return params; }
    // one JSON line per wave while rendering: {wave, ms, paths, segments, density_queries, kernel} (not owned; NULL = off)
    // With an MSE reference image the lines gain "mse", "mrse" and "device_ms" (device clock since the run's first record).
    void SetWaveLog(std::FILE *f) { waveLog = f; }
    // Options->mseReferenceImage / mseReferenceOutput (integrators.cpp:129-158, :243-262): `frameImage` as LoadMseReferenceImage
    // returns it; Render() then records the film's error over the pixel bounds after every wave ON THE DEVICE (vspg_film_error_enqueue:
    // no film read-back, no host synchronisation per wave) and writes one line "spp, mse.Average()" per wave ("%d, %.9g\n", :254) to
    // `out` (not owned) when it ends.  Recording completes the film after every wave, so the carry of in-flight paths between
    // one-sample waves is given up.  Not covered: vspg_pbrt_sharded.
    void SetMseReference(const std::vector<float> &frameImage, std::FILE *out);
    // The next frame of a volume sequence: replace the grid medium's density / temperature values in place (vspg_renderer_update_grid,
    // host source; nx*ny*nz values in the layout the scene was created with).  Majorants and bricks are rebuilt on the device; the BVH,
    // the light sampler, the guiding fields, the VSP buffer, the TrBuffer and the film stay -- ClearFilm() starts the new frame's film.
    // Throw on refusal: a medium that is no grid, a wrong size, a temperature grid the scene never had.
    void SetMediumDensity(const std::vector<float> &values);
    void SetMediumTemperature(const std::vector<float> &values);
    // The same for an "rgbgrid" medium (vspg_renderer_update_rgb_grids, host source): the sigma_a / sigma_s / Le values of `grids`
    // replace the renderer's, 3*nx*ny*nz floats each; an EMPTY vector keeps that grid (scale and Lescale stay create's and are not
    // read).  Octets and majorants are rebuilt on the device.  Throws on refusal: another medium, nothing given, a wrong size, a grid
    // the scene never had, a value that is negative or not finite.
    void SetMediumRgbGrids(const RgbGridStorage &grids);
    void ClearFilm();             // vspg_film_clear: the film to zero (statistics, VSP buffer and fields stay); Render() starts at wave 0 again
    // The film's file (RGBFilm::WriteImage, film.cpp:531-569), format by extension:
    //   .exr  the pixel bounds resolved ON THE DEVICE (vspg_film_resolve, scan-line layout) and written as they arrive: HALF channels
    //         B, G, R by default, FLOAT with fp16 = false (the Film's "savefp16"); dataWindow = the pixel bounds, displayWindow = the
    //         frame; samplesPerPixel, renderTimeSeconds and -- with an MSE reference -- MSE (the last wave's average) attributes; the
    //         reference's warning "%d pixel values clamped to maximum fp16 value." when the clamp touched any;
    //   any other name (.pfm)  GetFilm().WritePFM(), byte for byte as ever.
    // writePartial (--write-partial-images, cmd/pbrt.cpp:81, integrators.cpp:258-261): Render() rewrites the file after every wave with
    // samplesPerPixel = the waves so far; that completes the film each wave, so the carry of in-flight paths is given up.
    // Out of scope: vspg_pbrt_sharded (stays PFM), the Film's "maxcomponentvalue", the camera matrices in the metadata (worldToCamera,
    // worldToNDC), PIZ and the other compressions, tiled EXR.
    void SetOutput(const std::string &filename, bool fp16 = true, bool writePartial = false);
    void WriteImage();            // the film as it stands to the file SetOutput named

  private:
    std::FILE *waveLog = nullptr;
    std::FILE *mseOut = nullptr;
    VspgIntegratorParams params;
    VspgRenderConfig cfg;
    VspgRenderer *renderer = nullptr;
    int bounds[4] = {0, 0, 0, 0};  // x0, y0, x1, y1
    int spp;
    std::string outFile;
    bool outFp16 = true, outPartial = false;
    int sppDone = 0;              // waves rendered so far (metadata.samplesPerPixel)
    double renderSeconds = 0;     // (metadata.renderTimeSeconds)
    bool haveMse = false;
    float lastMse = 0;            // (metadata.MSE)
    GuidingCacheSettings cacheSettings;
    TrBufferSettings trSettings;
    IsgBufferSettings isgSettings;
};

// parameter parsing only (no device): used by Create and by the CPU self test
VspgIntegratorParams ParseIntegratorParams(const ParameterDictionary &parameters, GuidingCacheSettings *cache = nullptr,
                                           TrBufferSettings *tr = nullptr, IsgBufferSettings *isg = nullptr);

}  // namespace vspg
