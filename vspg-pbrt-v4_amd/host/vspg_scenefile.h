// vspg_scenefile.h -- a reader for the subset of the pbrt-v4 scene-file format the GuidedVolPathVSPG path needs
// (SURVEY 8f row 4): the directives of App. F plus what configs 3-5 add -- placed grid media, triangle meshes, sky and sun.
//
// What it stands in for: the parser -> BasicSceneBuilder -> BasicScene::CreateIntegrator chain
// (src/pbrt/parser.cpp, scene.cpp:883-887, cpu/render.cpp:56-57) up to Integrator::Create(name, parameters, ...)
// (cpu/integrators.cpp:3739-3744), Medium::Create (media.cpp:816-841) and Light::Create for "infinite" / "distant"
// (lights.cpp).  Everything is routed through the adapter's ParameterDictionary, so parameter names, defaults and the
// unused-parameter error are the reference's.
//
// Directives: LookAt, Camera "perspective" (fov, lensradius, focaldistance, screenwindow, frameaspectratio) / "orthographic" (the same
// without fov) / "spherical" (mapping "equalarea" | "equirectangular"; its lens parameters and window are read and ignored, as in the
// reference; "realistic" is refused by name), Sampler (pixelsamples, seed), PixelFilter "box", Film "rgb"
// (xresolution, yresolution, filename, savefp16, cropwindow, pixelbounds), Integrator, Option (ignored but "disabletexturefiltering"), ColorSpace (ignored), WorldBegin, AttributeBegin/End,
// Identity, Translate, Scale, Rotate, Transform, ConcatTransform, ReverseOrientation, Material "diffuse" (reflectance: rgb, float, or
// "texture reflectance" "name") / "interface", Texture "name" "spectrum" "imagemap" (filename: .pfm / .exr with R, G, B or Y; filter, wrap,
// scale, invert, mapping "uv", uscale, vscale, udelta, vdelta; maxanisotropy and encoding are read and ignored; other classes, other
// mappings and "float" textures are refused by name; a textured material on Shape "sphere" is refused by name; "uv" on trianglemesh,
// the default uv only on bilinearmesh; a scene with textures that does not set Option "bool disabletexturefiltering" true gets a warning),
// MakeNamedMaterial / NamedMaterial ("diffuse", "interface"), AreaLightSource "diffuse" (L, scale, twosided), LightSource "infinite"
// (L, scale; or "filename": an equal-area octahedral environment map, .exr / .pfm, square, with R, G, B -- the CTM in effect is the
// light's transform; no "portal", no "illuminance") / "distant" (L, scale, from, to) / "point" (I, scale, power, from under the CTM: a
// VspgPointLight filled by vspg_point_light_at; LightSource "spot" is still REFUSED by name here -- the library, its binding and
// vspg_spot_light_look_at carry everything it needs, the reader's few lines are a follow-up) / "projection" (scale, fov, filename: a slide
// with R, G, B, .exr / .pfm; "power" is refused by name) / "goniometric" (I, scale, power, filename: a square equal-area map, Y or R, G, B
// averaged; no filename = a warning and a point light), both placed by the CTM with the reference's flip / swap, MakeNamedMedium ("homogeneous", "uniformgrid", "rgbgrid", "nanovdb"), MediumInterface,
// Include (as a directive, and -- beyond pbrt -- inside a parameter list, for the block the reference's nanovdb2pbrt prints),
// Shape "bilinearmesh" (one patch: a parallelogram becomes a rectangle, anything else two triangles) / "trianglemesh"
// (P, indices) / "sphere" (radius; full spheres).  Anything else is an Error naming the directive: nothing is silently dropped.
//
// Conventions of this build: render space == world space (pbrt's --render-coord-sys world); ONE medium per scene,
// with the reference's boundaries (round 4): every shape carries its MediumInterface and its material -- an "interface" material
// makes it a pure medium boundary (guidedvolpathvspgintegrator.cpp:399-404) -- and the camera starts in the "outside" medium of the
// MediumInterface in effect at the Camera directive (scene.cpp:153-155); a second medium in the same scene is refused by name;
// emission on rectangles only; the film is written as OpenEXR or PFM by its file name's extension (host/vspg_image.h; "maxcomponentvalue"
// is not read).
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "vspg_host.h"

namespace vspg {

struct SceneDescription {
    VspgScene scene;                     // pointers inside refer to the vectors below: keep the description alive while creating
    // Camera "perspective" (lensradius, focaldistance) / "orthographic" / "spherical" (mapping): the model beside scene.camera.  A host
    // hands both to vspg_renderer_set_camera after create when this is not the pinhole perspective (CreateIntegrator does).
    VspgCameraModel cameraModel = {VSPG_CAMERA_PERSPECTIVE, 0.f, 0.f};
    std::vector<float> density, leScale, temperature, triP, triKd;
    std::vector<int32_t> triFlags;       // VSPG_TRI_* per triangle (material, MediumInterface, orientation)
    RgbGridStorage rgb;                  // MakeNamedMedium "string type" "rgbgrid": the grids scene.rgb_* point at
    // LightSource "infinite" "string filename": the image of infinite light `light` (R, G, B interleaved, top row first) and the
    // rows of its renderFromLight (the CTM at the directive).  CreateIntegrator hands them to the renderer it creates
    // (Integrator::SetEnvironmentImage -> vspg_renderer_set_environment_image); a host that creates the renderer itself does the same.
    struct EnvImage {
        int light = 0, res = 0;
        std::vector<float> rgb;
        float renderFromLight[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    };
    std::vector<EnvImage> envImages;
    // LightSource "projection" / "goniometric" "string filename": the image of point-light slot `slot` (R, G, B interleaved or Y alone, top
    // row first), handed to the renderer the same way (Integrator::SetLightImage -> vspg_renderer_set_light_image)
    struct LightImage {
        int slot = 0, xres = 0, yres = 0, channels = 0;
        std::vector<float> pixels;
    };
    std::vector<LightImage> lightImages;
    // Texture "name" "spectrum" "imagemap" and the surfaces that `Material "diffuse" "texture reflectance" "name"` binds them to: the
    // record vspg_renderer_create_textured takes beside the scene (CreateIntegrator hands it over); its pointers refer to the vectors here
    VspgSceneTextures textures = {};
    std::vector<std::vector<float>> texturePixels;   // per texture, xres * yres * channels floats, top row first
    std::vector<int32_t> triTexture;                 // per triangle: 0 = none, k = texture k - 1
    std::vector<float> triUv;                        // per triangle: uv0, uv1, uv2 (the mesh's "uv" or the default)
    bool disableTextureFiltering = false;            // Option "bool disabletexturefiltering": what the library evaluates either way
    std::string integratorName = "volpath";
    ParameterDictionary integratorParams;
    int xres = 1280, yres = 720;         // Film defaults (film.cpp)
    int pixelSamples = 16;               // Sampler default
    int seed = 0;
    std::string filmFilename = "pbrt.pfm";
    bool saveFP16 = true;                // Film "savefp16" (film.cpp:531-569): an .exr film is HALF, or FLOAT when false
    // Film "cropwindow" / "pixelbounds" as the file gives them (x0 x1 y0 y1; empty = not given), and the film's pixelBounds
    // [x0, x1) x [y0, y1) resolved from them by ResolvePixelBounds: all the render loop covers and the written image holds
    std::vector<float> cropWindow;
    std::vector<int> pixelBoundsParam;
    int boundsX0 = 0, boundsY0 = 0, boundsX1 = 1280, boundsY1 = 720;
    bool boundsResolved = false;         // ResolvePixelBounds has run (the parser only stores the two arrays)
    std::vector<std::string> warnings;   // directives that were accepted and ignored (Option, ColorSpace)
};

// --cropwindow x0,x1,y0,y1 / --pixelbounds x0,x1,y0,y1 (cmd/pbrt.cpp:132-153): they take precedence over the file's
struct FilmOverrides {
    bool haveCropWindow = false, havePixelBounds = false;
    float cropWindow[4] = {0, 1, 0, 1};   // x0 x1 y0 y1, fractions of the frame
    int pixelBounds[4] = {0, 0, 0, 0};    // x0 x1 y0 y1, pixels
};
// "x0,x1,y0,y1" -> four numbers; throws Error when there are not exactly four
void ParseCropWindowArg(const std::string &arg, FilmOverrides *o);
void ParsePixelBoundsArg(const std::string &arg, FilmOverrides *o);
// The film's pixelBounds by the rules of RGBFilm's base (film.cpp:97-172): the command line over the file, a crop window over
// pixel bounds; the file's crop window is min/max-ordered and clamped to [0,1], bounds are ceil(resolution * crop) in float;
// pixel bounds are clamped to the frame with a warning; a wrong value count and empty bounds are errors (vspg::Error).
// Called ONCE, when the command line is known: with overrides the file's own values are not even examined where the reference
// does not examine them (a malformed "cropwindow" under --cropwindow is no error, film.cpp:123).  CreateIntegrator resolves the
// file's own values itself when no host has.
void ResolvePixelBounds(SceneDescription &sd, const FilmOverrides &overrides = FilmOverrides());

// Parse scene text (the contents of a .pbrt file).  Throws vspg::Error on anything outside the subset above.
std::unique_ptr<SceneDescription> ParseSceneString(const std::string &text);
std::unique_ptr<SceneDescription> ParseSceneFile(const std::string &filename);
// Integrator::Create for the parsed scene (BasicScene::CreateIntegrator, scene.cpp:883-887)
std::unique_ptr<Integrator> CreateIntegrator(const SceneDescription &sd, int device = 0);

}  // namespace vspg
