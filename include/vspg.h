/*
 * vspg.h -- C-ABI of the MI355X-native GuidedVolPathVSPG hot path.
 *
 * The reference (kehanxuuu/vspg-pbrt-v4) has no FFI: the path sits behind C++ plugin
 * classes chosen by string in static Create() functions.  This header is
 * the boundary a maintainer would bind instead; every entry point names the reference
 * interface it replaces (paths relative to the reference root, file:line).
 *
 * Conventions
 *   - plain C, plain pointers and sizes; no C++/torch types.
 *   - every function returns 0 on success, a negative VSPG_E* code on failure;
 *     vspg_last_error() returns a human-readable message for the calling thread.
 *     (The reference aborts the process via ErrorExit/LOG_FATAL,
 *     src/pbrt/cpu/integrators.cpp:3760-3766; a library must not, so fatal conditions
 *     become error codes with the same trigger conditions.)
 *   - the library owns all device memory behind the opaque handle; host buffers are owned
 *     by the caller.  `stream` arguments are hipStream_t passed as void* (NULL = default).
 *   - one renderer per GPU; one host thread drives it (this replaces the
 *     ParallelFor2D thread-pool fan-out of src/pbrt/cpu/integrators.cpp:183-207).
 *   - there is NO CPU fallback: without a usable HIP device every compute entry point
 *     fails with VSPG_ENODEVICE.
 */
#ifndef VSPG_H
#define VSPG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSPG_ABI_VERSION 7

/* ---- error codes ------------------------------------------------------------------- */
#define VSPG_OK 0
#define VSPG_EINVAL (-1)     /* bad argument / unsupported parameter combination          */
#define VSPG_ENODEVICE (-2)  /* no HIP device / kernels not loadable                      */
#define VSPG_EHIP (-3)       /* a HIP runtime call failed (message has the hipError name) */
#define VSPG_ESCOPE (-4)     /* valid in the reference, outside this library's hot path   */

/* ---- scene description (synthetic analytic scene) ---------------- */
#define VSPG_MAX_QUADS 16

/* A rectangle p00 + u*e1 + v*e2, u,v in [0,1], e1 perpendicular to e2.  Stands in for a
 * pbrt "bilinearmesh" rectangle with a "diffuse" material and, when Le != 0, a "diffuse"
 * area light (src/pbrt/shapes.cpp:1128-1143, src/pbrt/bxdfs.h:31-80,
 * src/pbrt/lights.cpp:796-820). */
/* Medium boundaries (round 4).  A surface carries what pbrt's GeometricPrimitive hands the hit (src/pbrt/cpu/primitive.cpp:77): a material -- "diffuse", or NONE for `Material "interface"` (materials.cpp:736, scene.cpp:1340: a null
 * Material; GetBSDF returns no BSDF and Li skips the hit, guidedvolpathvspgintegrator.cpp:399-404) -- and a MediumInterface
 * {inside, outside} (base/medium.h:113-128; `MediumInterface "name_in" "name_out"`).  The library holds ONE medium
 * (VspgScene.medium), so each side is "the medium" or "no medium": medium_interface is a pair of bits.  Only a TRANSITION
 * (inside != outside, MediumInterface::IsMediumTransition) changes anything: Interaction::GetMedium(w) then returns the
 * outside medium for Dot(w, n) > 0, the inside one otherwise (interaction.h:117-121), n being the surface's geometric
 * normal after reverse_orientation; a surface that is not a transition leaves a ray in the medium it arrived in
 * (SurfaceInteraction::SetIntersectionProperties, interaction.h:218-229). */
enum { VSPG_MATERIAL_DIFFUSE = 0, VSPG_MATERIAL_INTERFACE = 1 };
#define VSPG_IFACE_INSIDE 1   /* the scene's medium lies on the inside (behind the normal):  MediumInterface "m" ""  */
#define VSPG_IFACE_OUTSIDE 2  /* ... on the outside (the side the normal points to):         MediumInterface ""  "m" */
/* (0 and VSPG_IFACE_INSIDE | VSPG_IFACE_OUTSIDE: not a transition) */

typedef struct VspgQuad {
    float p00[3];
    float e1[3];
    float e2[3];
    float Kd[3];                  /* diffuse reflectance R (RGB) */
    float Le[3];                  /* emitted radiance (RGB); all zero = not a light */
    int32_t two_sided;            /* DiffuseAreaLight "twosided" */
    int32_t reverse_orientation;  /* flips the geometric normal normalize(e1 x e2) */
    int32_t material;             /* VSPG_MATERIAL_* */
    int32_t medium_interface;     /* VSPG_IFACE_* bits */
} VspgQuad;

/* Shape "sphere" (src/pbrt/shapes.h:107-330): the full sphere of `radius` around the object-space origin (partial spheres
 * -- zmin / zmax / phimax -- are refused), placed by renderFromObject.  Both matrices of pbrt's Transform, row-major, as
 * for VspgMedium (vspg_transform_inverse fills the inverse).  Intersection = Sphere::BasicIntersect with its interval
 * arithmetic (shapes.h:147-229), interaction = InteractionFromIntersection + Transform::operator()(SurfaceInteraction)
 * (shapes.h:237-284, transform.cpp:229-261).  Diffuse or interface.  A diffuse sphere becomes a DiffuseAreaLight through the tail of
 * VspgScene (sphere_Le / sphere_two_sided, below): this record keeps its size, which sits inside VspgScene in front of fields whose
 * offsets callers rely on.
 * Matrices get no check beyond "affine": under a matrix with scale the light does what the reference does -- the cone branch of
 * Sphere::Sample / PDF and Area() work with the object-space radius and ignore the scale (shapes.h:316-360). */
#define VSPG_MAX_SPHERES 8
typedef struct VspgSphere {
    float render_from_object[16];
    float object_from_render[16];
    float radius;
    float Kd[3];
    int32_t reverse_orientation;
    int32_t material;
    int32_t medium_interface;
} VspgSphere;

/* Pinhole camera: raster point (x,y) -> camera-space point (sx*x+ox, sy*y+oy, 1),
 * normalised, then rotated into render space by the orthonormal frame (right, up, fwd).
 * Replaces PerspectiveCamera::GenerateRayDifferential (src/pbrt/cameras.cpp:435-447)
 * for lensRadius == 0.  Fill with vspg_camera_look_at().  A renderer is created with this pinhole; a thin lens, an
 * orthographic or a spherical camera is set on the live renderer (vspg_renderer_set_camera, below), which reads the same record. */
typedef struct VspgCamera {
    float origin[3];
    float right[3], up[3], fwd[3];
    float sx, ox, sy, oy;
} VspgCamera;

enum { VSPG_MEDIUM_NONE = 0, VSPG_MEDIUM_HOMOGENEOUS = 1, VSPG_MEDIUM_GRID = 2, VSPG_MEDIUM_NANOVDB = 3 };
/* RGBGridMedium ("rgbgrid", src/pbrt/media.h:391-467, media.cpp:369-484): per-voxel RGB sigma_a / sigma_s / Le grids.  Of this record it
 * reads type, g, nx / ny / nz, the bounds and the transform; its grids and scales travel in the tail of VspgScene (rgb_*, below), and
 * sigma_a / sigma_s / Le / density here are ignored. */
#define VSPG_MEDIUM_RGBGRID 4

/* The scene's one medium.  Without medium boundaries (no transition surface, camera_outside_medium == 0) it fills the
 * scene -- ray.medium for every ray, rounds 1-3 -- otherwise a ray is in it or in no medium at all, as the camera and
 * the MediumInterfaces it crossed say.
 * HOMOGENEOUS mirrors HomogeneousMedium (src/pbrt/media.h:221-283; parameters
 * src/pbrt/media.cpp:167-206): sigma_a/sigma_s are RGB, already multiplied by "scale";
 * Le already multiplied by "Lescale".
 * GRID mirrors GridMedium ("uniformgrid", src/pbrt/media.h:284-390,
 * src/pbrt/media.cpp:209-361): density grid nx*ny*nz, x fastest, over `bounds` in medium
 * space == render space (identity renderFromMedium); sigma_a/sigma_s are the RGB spectra
 * already multiplied by "scale"; majorant grid is 16^3 (media.cpp:252). */
typedef struct VspgMedium {
    int32_t type;
    float sigma_a[3];
    float sigma_s[3];
    float g;
    float Le[3];
    /* grid only */
    int32_t nx, ny, nz;
    float bounds_min[3], bounds_max[3];
    const float *density; /* HOST pointer, nx*ny*nz floats; copied at create time */
    /* VSPG_MEDIUM_NANOVDB only -- NanoVDBMedium (src/pbrt/media.h:657-753, media.cpp:549-675) over a DENSE copy
     * of the density grid (what cmd/nanovdb2pbrt.cpp:97-126 dumps): voxel (i,j,k) of the array is index
     * (index_min + (i,j,k)); values outside the index bounding box are the background 0.
     * worldToIndexF(p) = (p - grid_origin) / voxel_size; `bounds` is the grid's world bounding box;
     * majorants live on a 64^3 grid (media.cpp:574); "densityoffset" / "majorantscale" as in the RGB-mode ctor. */
    int32_t index_min[3];
    float voxel_size[3];
    float grid_origin[3];
    float density_offset;
    float majorant_scale;
    /* VSPG_MEDIUM_GRID only -- emission of GridMedium (src/pbrt/media.h:326-342, media.cpp:316-328): Le at a point =
     * LeScale.Lookup(p) * Le when that scale is positive.  `Le` above is Le_spec sampled (RGB); le_scale is the
     * "Lescale" grid ALREADY multiplied by the reference's photometric normalisation 1 / SpectrumToPhotometric(Le)
     * (HOST pointer, le_nx*le_ny*le_nz floats, x fastest, copied at create time).  NULL with a non-zero Le = the
     * reference's default 1x1x1 grid holding 1 (trilinear against the zero background: a tent over the bounds).
     * Temperature grids (blackbody emission) are outside this build's scope. */
    const float *le_scale;
    int32_t le_nx, le_ny, le_nz;
    /* grid media -- renderFromMedium (src/pbrt/media.h:322, :354, :693, :708; the Transform the scene file's CTM gave
     * the medium): has_transform = 0 means identity.  Both matrices of pbrt's Transform are passed, row-major
     * (m and mInv, util/transform.h:186-187): a pbrt host hands over its own inverse, so that
     * Transform::ApplyInverse(Ray, &tMax) / ApplyInverse(Point3f) (transform.h:387-429, transform.cpp:263-303) see the same
     * floats.  vspg_transform_inverse() fills medium_from_render for callers that only have m.  Affine matrices only
     * (last row 0 0 0 1). */
    int32_t has_transform;
    float render_from_medium[16];
    float medium_from_render[16];
    /* Temperature grid of an emissive GridMedium (media.h:333-341; "temperature", media.cpp:276-302) or NanoVDBMedium (media.h:724-735;
     * config 5 "explosion"): as many samples as `density`, same layout -- for NanoVDB the same index bounding box and index-to-world
     * map (the .nvdb reader checks).  Where the scaled temperature T' = (T(p) - temperature_offset) * temperature_scale exceeds 100,
     *   Le(p) = scale * BlackbodySpectrum(T').Sample(lambda),  scale = nvdb_le_scale (NanoVDB) / the le_scale grid's value (GridMedium)
     * at the path's three sampled wavelengths, which the RGB build stores as R, G, B.  The path adds volume
     * emission in the DELTA-TRACKING callback only (guidedvolpathvspgintegrator.cpp:895-906): under "vspsamplingmethod" "nds";
     * a heterogeneous medium under the default "resampling" never evaluates it and the grid has no effect on
     * the result.  A GridMedium with both Le and temperature is VSPG_EINVAL (media.cpp:307-308).  HOST pointer; NULL = none. */
    const float *temperature;
    float nvdb_le_scale, temperature_offset, temperature_scale;
} VspgMedium;

/* Triangle geometry (src/pbrt/shapes.h:828-1030, shapes.cpp:168-262, cpu/aggregates.cpp:529-640):
 * a soup of diffuse, non-emissive, two-sided triangles next to the rectangles; the library builds a BVH over them
 * (own builder) and traverses it on the device.  tri_p: 9 floats per triangle (p0, p1, p2), tri_kd: 3 per triangle.
 * HOST pointers, copied at create time. */
/* Infinite lights (src/pbrt/lights.h:  UniformInfiniteLight :554-601, DistantLight :207-250; escaped-ray MIS
 * guidedvolpathvspgintegrator.cpp:353-374): L = scale * Lemit already multiplied out (RGB).  Distant: w_light = the
 * normalised direction TOWARDS the light in render space.
 * Image (ImageInfiniteLight, lights.h:607-697, lights.cpp:1072-1142): L = the RGB multiplier of the image's texels (the
 * reference's `scale`, multiplied out); w_light is ignored.  The image itself is not part of the scene record: a renderer created
 * with such a slot holds a 1 x 1 image of (1, 1, 1) under the identity transform (the uniform sky of colour L; lights.cpp:1683 "happily,
 * this all just works") until vspg_renderer_set_environment_image replaces it. */
enum { VSPG_LIGHT_UNIFORM_INFINITE = 0, VSPG_LIGHT_DISTANT = 1, VSPG_LIGHT_IMAGE_INFINITE = 2 };
#define VSPG_MAX_INFINITE_LIGHTS 4
typedef struct VspgInfiniteLight {
    int32_t type;
    float L[3];
    float w_light[3];
} VspgInfiniteLight;

/* Point and spot lights (PointLight, src/pbrt/lights.h:203-263, lights.cpp:196-248; SpotLight, lights.h:811-873,
 * lights.cpp:1425-1555): lights AT a position inside the scene, delta lights like the distant light (SampleLi has pdf 1, PDF_Li is 0,
 * the estimate is weighted as IsDeltaLight prescribes, guidedvolpathvspgintegrator.cpp:1248-1249).
 *   I                  the reference's `scale * I` multiplied out (RGB), the convention of VspgInfiniteLight.L
 *   render_from_light  the light's Transform, row-major and affine (last row 0 0 0 1), BOTH matrices as for VspgSphere / VspgMedium
 *   light_from_render  so that ApplyInverse sees the caller's floats.  The light sits at render_from_light(0, 0, 0); a spot light
 *                      shines along render_from_light(0, 0, 1).  vspg_point_light_at / vspg_spot_light_look_at fill both.
 *   cone_angle_deg     spot lights (for a projection light: its field of view, below): "coneangle" (the whole cone's half angle) and "conedeltaangle" (the width of the smooth falloff
 *   cone_delta_deg     band inside it).  The library forms cosFalloffEnd = cosf(Radians(cone_angle_deg)) and cosFalloffStart =
 *                      cosf(Radians(cone_angle_deg - cone_delta_deg)) on the host, as the constructor does (lights.cpp:1438-1439).
 * A context point that coincides with the light's position divides by zero, as in the reference, which has no guard. */
enum { VSPG_LIGHT_POINT = 3, VSPG_LIGHT_SPOT = 4 };
/* Projection and goniometric lights (ProjectionLight, src/pbrt/lights.h:342-392, lights.cpp:319-441, :490-560; GoniometricLight,
 * lights.h:395-455, lights.cpp:564-624, :652-734): delta lights at a position like the two above, whose intensity per direction comes
 * from an image.  They travel in the same VspgPointLight slots; type, I and both matrices keep their meaning.
 *   projection   a slide projector: the light looks along render_from_light(0, 0, 1) through Perspective(fov, 1e-3, 1e30); the slide (R, G, B
 *                per texel, clamped at zero) fills the screen window [-aspect, aspect] x [-1, 1] (aspect > 1) or [-1, 1] x [-1/aspect, 1/aspect].
 *                The field of view ("fov": the full angle of the beam across the slide's shorter axis, in degrees) is cone_angle_deg of
 *                the slot -- a projection light has no other use for the field, and the scene record keeps its size --: valid values lie
 *                in (0, 180), anything else (NaN included) is VSPG_EINVAL; cone_delta_deg is not read.  vspg_projection_light_at builds ctm * Scale(1, -1, 1).
 *   goniometric  a bulb whose intensity is I times one texel (Y) of a square equal-area map (EqualAreaSphereToSquare of the direction in
 *                light space, nearest texel, clamped at the edge).  vspg_goniometric_light_at builds ctm * swapYZ.  The linear part of
 *                light_from_render must be orthonormal -- the mapping is defined for unit vectors and the reference hands it
 *                ApplyInverse(-wi) unnormalised --: every entry of R R^T - 1 (R = the 3 x 3 of light_from_render, in double) must lie
 *                within 1e-4, a hundred times what float products of rotations leave and far below any real scale; beyond it VSPG_ESCOPE.
 * The image is not part of the scene record: a renderer created with such a slot holds a 1 x 1 image of ones (a uniform square beam; a
 * point light) until vspg_renderer_set_light_image replaces it.  SampleLe / PDF_Le and the PiecewiseConstant2D they alone read are out
 * of scope: Li never calls them. */
enum { VSPG_LIGHT_PROJECTION = 5, VSPG_LIGHT_GONIOMETRIC = 6 };
#define VSPG_LIGHT_IMAGE_MAX_RES 4096
#define VSPG_MAX_POINT_LIGHTS 8
typedef struct VspgPointLight {
    int32_t type;                 /* VSPG_LIGHT_POINT | VSPG_LIGHT_SPOT | VSPG_LIGHT_PROJECTION | VSPG_LIGHT_GONIOMETRIC */
    float I[3];
    float render_from_light[16];
    float light_from_render[16];
    float cone_angle_deg;
    float cone_delta_deg;
} VspgPointLight;

/* tri_flags (optional, one int32 per triangle, HOST pointer; NULL = all 0): bit 0 = VSPG_MATERIAL_INTERFACE, bits 1-2 =
 * the VSPG_IFACE_* bits, bit 3 = flip the geometric normal (the mesh's reverseOrientation ^ transformSwapsHandedness,
 * shapes.h:934-936 -- only a medium transition can tell the two sides of a diffuse triangle apart). */
#define VSPG_TRI_INTERFACE 1
#define VSPG_TRI_IFACE_SHIFT 1
#define VSPG_TRI_FLIP_NORMAL 8

/* Image textures on diffuse reflectance: SpectrumImageTexture ("imagemap", src/pbrt/textures.h:250-290, textures.cpp:359-387) under
 * UVMapping (textures.h:86-106), bound to a DiffuseMaterial's "reflectance" (materials.h:369-380) on rectangles and triangles, evaluated
 * as the reference does under `Option "bool disabletexturefiltering" true`: every ray differential is zero (interaction.cpp:43-47), so
 * MIPMap::Filter (util/mipmap.cpp:229-298) takes level 0 for every filter -- "bilinear", "trilinear" and "ewa" all become Bilerp(0, st)
 * (VSPG_TEXFILTER_BILINEAR), "point" becomes Texel(0, round(st * res - 0.5)).  With (u, v) the hit's surface parameters:
 *   st = (su * u + du, sv * v + dv);  st[1] = 1 - st[1]
 *   bilinear: x = st[0] * xres - 0.5f, xi = floor(x), dx = x - xi, likewise y; the texels (xi, yi) (xi+1, yi) (xi, yi+1) (xi+1, yi+1) through
 *             RemapPixelCoords (util/image.h:93-146: repeat = Mod, non-negative; clamp; black = the texel counts as 0), summed as
 *             ((1-dx)(1-dy) v0 + dx (1-dy) v1 + (1-dx) dy v2 + dx dy v3) per channel, in that order, no contraction (util/image.h:279-292)
 *   point:    texel (round(x), round(y)), std::round (halves away from zero), through the same wrap
 *   rgb = scale * filtered;  rgb = ClampZero(invert ? 1 - rgb : rgb);  R = Clamp(rgb, 0, 1) (the albedo spectrum type)
 * A one-channel image broadcasts to grey.  A hit whose R is all zero has no BSDF lobes (DiffuseBxDF::Flags): the path ends there
 * without next-event estimation, as at a Kd = 0 surface.
 * (u, v) of a hit: a rectangle p00 + u e1 + v e2 has u = Dot(p - p00, e1) / |e1|^2, v = Dot(p - p00, e2) / |e2|^2 (pbrt's default
 * patch uv (0,0) (1,0) (0,1) (1,1)); a triangle has uv = b0 uv0 + b1 uv1 + b2 uv2 (shapes.h, `uvHit`) with the mesh's "uv" or the
 * default (0,0) (1,0) (1,1).
 * Out of scope: filtered lookups (ray differentials, levels above 0, EWA), images whose resolution is no power of two
 * (Image::GeneratePyramid resamples those before level 0 exists), 8-bit images and colour encodings, spheres, float textures, alpha,
 * bump or displacement, textures on Le or on anything but diffuse reflectance, procedural textures. */
#define VSPG_MAX_TEXTURES 8
#define VSPG_TEXTURE_MAX_RES 4096
enum { VSPG_TEXWRAP_REPEAT = 0, VSPG_TEXWRAP_CLAMP = 1, VSPG_TEXWRAP_BLACK = 2 };
enum { VSPG_TEXFILTER_POINT = 0, VSPG_TEXFILTER_BILINEAR = 1 };
typedef struct VspgTexture {
    const float *pixels;      /* HOST pointer, xres * yres * channels floats, top row first; copied at create time */
    int32_t xres, yres;       /* 1 .. VSPG_TEXTURE_MAX_RES, powers of two */
    int32_t channels;         /* 1 (grey) or 3 (R, G, B) */
    int32_t wrap;             /* VSPG_TEXWRAP_* */
    int32_t filter;           /* VSPG_TEXFILTER_* */
    int32_t invert;           /* 0 or 1 */
    float scale;              /* "scale" */
    float su, sv, du, dv;     /* UVMapping "uscale", "vscale", "udelta", "vdelta" */
} VspgTexture;

typedef struct VspgScene {
    int32_t n_quads;
    VspgQuad quads[VSPG_MAX_QUADS];
    VspgCamera camera;
    VspgMedium medium;
    int32_t n_triangles;
    const float *tri_p;
    const float *tri_kd;
    int32_t n_infinite_lights;
    VspgInfiniteLight infinite_lights[VSPG_MAX_INFINITE_LIGHTS];
    /* round 4: medium boundaries */
    const int32_t *tri_flags;
    int32_t n_spheres;
    VspgSphere spheres[VSPG_MAX_SPHERES];
    /* the camera's medium (CameraBase::medium = the current OUTSIDE medium at the Camera directive, scene.cpp:153-155):
     * 0 = the scene's medium (as ever), 1 = none -- the camera looks at the volume from outside */
    int32_t camera_outside_medium;
    /* Point and spot lights.  THE RECORD GREW by this tail (VSPG_ABI_VERSION stays 7: nothing in front of it moved): callers are
     * recompiled against this header, and a caller that fills the record field by field zeroes it first (memset), which leaves
     * n_point_lights = 0.
     * The scene's LIGHT LIST, which every light sampler indexes, is: the emissive rectangles in rectangle order, then the infinite
     * lights, then the point lights (then the emissive spheres, below) -- every index of a scene without point lights keeps its
     * meaning. */
    int32_t n_point_lights;
    VspgPointLight point_lights[VSPG_MAX_POINT_LIGHTS];
    /* Sphere area lights (DiffuseAreaLight on Shape "sphere": lights.cpp:796-864, shapes.h:293-393).  THE RECORD GREW by this second
     * tail in the same way (VSPG_ABI_VERSION stays 7); a zeroed record holds no sphere light.  Both arrays are indexed by sphere:
     *   sphere_Le[i]         the radiance sphere i emits: the reference's `scale * L` multiplied out (RGB), the convention of VspgQuad.Le;
     *                        all zero = not a light.  A component that is negative, NaN or infinite is VSPG_EINVAL.
     *   sphere_two_sided[i]  DiffuseAreaLight "twosided": 0 = the side the normal points to emits (the outside, or the inside under
     *                        reverse_orientation), 1 = both.  Any other value is VSPG_EINVAL.
     * An emissive sphere whose material is VSPG_MATERIAL_INTERFACE is VSPG_ESCOPE: the reference allows it, the library does not, so
     * that a shadow ray's end point never lies on a surface its chain of segments walks through.
     * No image, no alpha, no SampleLe.
     * The LIGHT LIST gains a fourth range: emissive rectangles, infinite lights, point lights, then the EMISSIVE SPHERES in sphere
     * order -- every index of a scene without them keeps its meaning. */
    float sphere_Le[VSPG_MAX_SPHERES][3];
    int32_t sphere_two_sided[VSPG_MAX_SPHERES];
    /* RGB grid medium (medium.type == VSPG_MEDIUM_RGBGRID; RGBGridMedium, media.h:391-467, media.cpp:369-484 in the RGB rendering build:
     * RGBUnboundedSpectrum / RGBIlluminantSpectrum hold an RGB, Sample() returns it, MaxValue() is its largest component).  THE RECORD
     * GREW by this third tail in the same way (VSPG_ABI_VERSION stays 7); a zeroed record holds no RGB grid.
     *   rgb_sigma_a, rgb_sigma_s, rgb_Le   HOST pointers, 3 * nx * ny * nz floats each (medium.nx / ny / nz), voxel-major with x fastest,
     *                                      R, G, B per voxel; copied at create time.  NULL = absent: an absent sigma grid counts as the
     *                                      constant 1 in SamplePoint and in the majorant (media.h:424-429, media.cpp:404-406).
     *   rgb_sigma_scale                    "scale" (sigmaScale): multiplies both looked-up coefficients and the majorant
     *   rgb_le_scale                       "Lescale": Le(p) = rgb_le_scale * Lookup(Le grid, p) when there is an Le grid and the scale is > 0
     * Lookup is SampledGrid::Lookup(p, convert) (util/containers.h:784-801): trilinear per channel, Lerp(t, a, b) = (1 - t) a + t b over
     * x, then y, then z, voxels outside the grid = 0.  The 16^3 majorant grid holds ONE scalar per cell for all three channels:
     * rgb_sigma_scale * (MaxValue(sigma_a box) + MaxValue(sigma_s box)), the maximum over voxels and channels taken per grid, then summed.
     * VSPG_EINVAL at create: both sigma grids NULL; rgb_Le without rgb_sigma_a (media.cpp:386-387, :433-434); a value in any grid that is
     * negative, NaN or infinite; nx, ny or nz < 1; a scale that is NaN or infinite; medium.temperature set.
     * In-place update: vspg_renderer_update_rgb_grids (below); read-back of the device image: vspg_rgb_octets_read.
     * Limits: dense storage only; vspg_renderer_update_grid and vspg_brick_info / _read return VSPG_EINVAL and
     * vspg_renderer_set_arithmetic to a tolerance mode VSPG_ESCOPE, each with the renderer unchanged; VSPG_KERNEL=wg falls through to
     * the per-lane kernel; one medium per scene, as ever. */
    const float *rgb_sigma_a;
    const float *rgb_sigma_s;
    const float *rgb_Le;
    float rgb_sigma_scale;
    float rgb_le_scale;
} VspgScene;

/* The scene's image textures (VspgTexture, above) and which surface carries which: a record BESIDE VspgScene, handed to
 * vspg_renderer_create_textured.  VspgScene keeps its size and every offset (VSPG_ABI_VERSION stays 7): a caller that knows no textures
 * calls vspg_renderer_create as ever.  A zeroed record holds no texture.
 *   textures[k]        texture k, k < n_textures
 *   quad_texture[i]    rectangle i of the scene: 0 = none (its Kd), k = texture k - 1 replaces Kd
 *   tri_texture        one int32 per triangle of the scene with the same convention, HOST pointer, NULL = none
 *   tri_uv             6 floats per triangle (uv0, uv1, uv2), HOST pointer, NULL = the default (0,0) (1,0) (1,1)
 * VSPG_EINVAL at create: n_textures outside 0 .. VSPG_MAX_TEXTURES; a surface's index outside 0 .. n_textures; a texture on a
 * surface whose material is VSPG_MATERIAL_INTERFACE; a NULL image; xres or yres outside 1 .. VSPG_TEXTURE_MAX_RES; channels other
 * than 1 or 3; an unknown wrap or filter, an invert other than 0 or 1; a texel, parameter or uv that is NaN or infinite.
 * VSPG_ESCOPE: a resolution that is not a power of two.  Spheres have no field: textures on them are out of scope.
 * A scene with a textured surface runs the full-scene kernels (vspg_renderer_kernel_name); the kernels of untextured scenes are
 * the ones they were. */
typedef struct VspgSceneTextures {
    int32_t n_textures;
    VspgTexture textures[VSPG_MAX_TEXTURES];
    int32_t quad_texture[VSPG_MAX_QUADS];
    const int32_t *tri_texture;
    const float *tri_uv;
} VspgSceneTextures;

/* ---- integrator parameters: same names and defaults as
 * GuidedVolPathVSPGIntegrator::Create (src/pbrt/cpu/guidedvolpathvspgintegrator.cpp:
 * 1260-1322).  Use vspg_integrator_params_default() then override. ------------------ */
enum { VSPG_GUIDE_MIS = 0, VSPG_GUIDE_RIS = 1 };              /* guiding.h:52-55 */
enum { VSPG_VSP_CONTRIBUTION = 0, VSPG_VSP_VARIANCE = 1 };    /* "vspcriterion" */
enum { VSPG_VSP_RESAMPLING = 0, VSPG_VSP_NDS = 1 };           /* "vspsamplingmethod" */
enum { VSPG_LIGHTSAMPLER_UNIFORM = 0, VSPG_LIGHTSAMPLER_POWER = 1, VSPG_LIGHTSAMPLER_BVH = 2 };

typedef struct VspgIntegratorParams {
    int32_t maxdepth;                  /* 5 */
    int32_t minrrdepth;                /* 1 */
    int32_t usenee;                    /* true */
    int32_t surfaceguiding;            /* true  (directional guiding of BSDF sampling) */
    int32_t volumeguiding;             /* true  (directional guiding of phase sampling) */
    int32_t surfaceguidingtype;        /* "ris" */
    int32_t volumeguidingtype;         /* "mis" */
    int32_t vspguiding;                /* true */
    int32_t vspprimaryguiding;         /* true */
    int32_t vspsecondaryguiding;       /* true */
    float vspmisratio;                 /* 0.5 */
    int32_t vspcriterion;              /* "variance" */
    int32_t vspsamplingmethod;         /* "resampling" */
    int32_t collisionProbabilityBias;  /* false (NDS+: needs a transmittance buffer, vspg_renderer_set_tr_buffer) */
    int32_t rrguiding;                 /* false: guided Russian roulette (needs the image-space contribution estimate) */
    int32_t lightsampler;              /* "bvh" */
    int32_t regularize;                /* false (no-op for diffuse BxDFs) */
    int32_t guide_num_training_waves;  /* 128, hidden constant integrators.h:502 */
    int32_t storeTrBuffer;             /* false: record the primary rays' transmittance (TrBuffer) for read-back */
    int32_t surfacerrguiding;          /* true  (with rrguiding: guided survival probability at surface vertices, else 1) */
    int32_t volumerrguiding;           /* true  (same for volume vertices) */
} VspgIntegratorParams;

/* Film "rgb" + Sampler "independent" + PixelFilter "box" (SURVEY.md App. F). */
typedef struct VspgRenderConfig {
    int32_t xres, yres;   /* Film xresolution / yresolution */
    int32_t spp;          /* Sampler "pixelsamples" (only used for bookkeeping) */
    int32_t seed;         /* --seed / sampler "seed" (src/pbrt/samplers.h:457-460) */
    /* multi-GPU sharding of sample indices: this renderer handles wave w iff
     * w % shard_count == shard_index.  1-GPU: index 0, count 1. */
    int32_t shard_index, shard_count;
    int32_t device;       /* HIP device ordinal */
} VspgRenderConfig;

typedef struct VspgCounters {
    uint64_t paths;             /* camera samples run to termination */
    uint64_t segments;          /* iterations of the Li() path loop (roofline unit, 8d) */
    uint64_t volume_scatters;   /* real scattering events ("Volume interactions") */
    uint64_t surface_hits;      /* "Surface interactions" */
    uint64_t density_queries;   /* tentative collisions ("Integrator/Density query") */
    uint64_t shadow_rays;
    uint64_t shadow_density_queries; /* tentative collisions of the NEE shadow rays' ratio tracking in a HETEROGENEOUS medium (8 voxels + a
                                        majorant each, like density_queries; the reference's densityQueryCount does not count them) */
} VspgCounters;

/* ---- guiding field (spatial-directional cache) -------------------------------------------
 * Stands in for an openpgl::cpp::Field after Field::Update / Field(file)
 * (guidedvolpathvspgintegrator.cpp:111-128, 234-246).  OpenPGL is not part of the reference tree,
 * so the layout and the mixture math are this build's own design: a kd-tree over
 * positions whose leaves hold a parallax-aware von-Mises-Fisher mixture of the incident radiance
 * plus a per-lobe volume-scatter-probability estimate.  The renderer trains the field in-loop (Field::Update,
 * SURVEY 8a row a18; see "guiding-cache training" below) or takes a trained one (vspg_renderer_set_guiding_field). */
#define VSPG_FIELD_LOBES 8
typedef struct VspgKdNode {
    float split;      /* inner node: split plane position along `axis` */
    uint32_t packed;  /* bits 0-1: axis 0..2, 3 = leaf; bits 2-31: left child index (right = left+1),
                         or the region index for a leaf */
} VspgKdNode;
typedef struct VspgFieldRegion {
    float pivot[3];                    /* reference point of the lobes' parallax distances */
    int32_t n_lobes;                   /* 0 = region not trained: Init() fails there */
    float weight[VSPG_FIELD_LOBES];    /* mixture weights, sum 1 */
    float kappa[VSPG_FIELD_LOBES];     /* vMF concentrations */
    float mu[3][VSPG_FIELD_LOBES];     /* vMF mean directions (unit), SoA */
    float distance[VSPG_FIELD_LOBES];  /* distance of the lobe's source from the pivot; +inf = none */
    float vsp[VSPG_FIELD_LOBES];       /* volume scatter probability along the lobe, in [0,1] */
} VspgFieldRegion;
typedef struct VspgField {
    int32_t n_nodes, n_regions;
    const VspgKdNode *nodes;           /* HOST pointers; node 0 is the root */
    const VspgFieldRegion *regions;
} VspgField;

/* ---- guiding-cache training -------------------------------------------
 * With surfaceguiding / volumeguiding / vspsecondaryguiding set and no field uploaded, the renderer
 * trains the field itself, like the reference (guideTraining, guidedvolpathvspgintegrator.cpp:109,
 * 230-248): every path records its vertices (guiding.h:682-832), turns them into radiance samples when
 * it ends (PathSegmentStorage::PropagateSamples, :627) and vspg_post_process_wave refits the field
 * (Field::Update, :239) while fewer than guide_num_training_waves updates have run. */
typedef struct VspgTrainSample {
    float p[3];       /* vertex position */
    float dir[3];     /* sampled direction at the vertex (direction the radiance arrives from) */
    float weight;     /* incident radiance estimate / pdf */
    float pdf;        /* pdf the direction was sampled with */
    float distance;   /* distance to the next vertex along dir */
    uint32_t flags;   /* VSPG_SAMPLE_* */
} VspgTrainSample;
#define VSPG_SAMPLE_VOLUME 1u       /* vertex lies in the medium -> volume field */
#define VSPG_SAMPLE_NEXT_VOLUME 2u  /* the next event along dir was a volume scatter (VSP statistics) */
typedef struct VspgTrainStats {
    int32_t training;      /* 1 while the field is still being trained */
    int32_t iteration;     /* Field::GetIteration(): number of updates done */
    uint64_t n_samples;    /* radiance samples recorded since the last update */
    uint64_t n_zero;       /* zero-valued samples dropped since the last update */
    int32_t n_nodes[2], n_regions[2];  /* [0] surface field, [1] volume field */
    uint64_t n_dropped;    /* samples beyond the sample buffer's capacity (xres*yres*(maxdepth+1), at most 2^26) since the
                            * last update: a training vspg_render_wave() over SEVERAL sample indices runs them as 1-spp
                            * launches into one buffer that the single following vspg_post_process_wave() consumes --
                            * call render_wave / post_process_wave per sample index (the reference's waves) to lose none */
} VspgTrainStats;

typedef struct VspgRenderer VspgRenderer; /* opaque */

/* ---- helpers (host only, no device needed) ----------------------------------------- */
int vspg_abi_version(void);
const char *vspg_last_error(void);
void vspg_integrator_params_default(VspgIntegratorParams *p);
/* pbrt "LookAt" + Camera "perspective" "float fov" (fov spans the shorter image axis,
 * src/pbrt/cameras.cpp:474-489), world == render space. */
int vspg_camera_look_at(VspgCamera *cam, const float eye[3], const float look[3],
                        const float up[3], float fov_degrees, int xres, int yres);
/* inv = m^-1 for an affine row-major 4x4 (computed in double, rounded once); returns VSPG_EINVAL for a singular matrix. */
int vspg_transform_inverse(const float m[16], float inv[16]);
/* The transform of a spot light given like the scene file's "from" / "to" under the current transformation matrix `ctm` (row-major,
 * affine; NULL = identity), SpotLight::Create (lights.cpp:1531-1536):
 *   renderFromLight = ctm * Translate(from) * Inverse(Frame::FromZ(Normalize(to - from)))
 * Fills l->render_from_light and l->light_from_render (the product of the inverses in the opposite order) and nothing else.  The
 * frame is CoordinateSystem's (util/vecmath.h:1007-1013) in float; matrix products accumulate by fused multiply-add in float, as
 * SquareMatrix's do; the inverse of the frame and of `ctm` are vspg_transform_inverse's.  VSPG_EINVAL: a null argument, from == to,
 * a non-finite argument, a `ctm` that is not affine or is singular. */
int vspg_spot_light_look_at(VspgPointLight *l, const float from[3], const float to[3], const float ctm[16] /* or NULL */);
/* The same for a point light at `from` (PointLight::Create, lights.cpp:240-242): renderFromLight = ctm * Translate(from). */
int vspg_point_light_at(VspgPointLight *l, const float from[3], const float ctm[16] /* or NULL */);
/* The same for a projection light (ProjectionLight::Create, lights.cpp:555-556): renderFromLight = ctm * Scale(1, -1, 1), and for a
 * goniometric light (GoniometricLight::Create, lights.cpp:724-726): renderFromLight = ctm * swapYZ.  Both lights sit at the origin of
 * `ctm` (NULL = identity: the flip / the swap as it stands).  VSPG_EINVAL as above. */
int vspg_projection_light_at(VspgPointLight *l, const float ctm[16] /* or NULL */);
int vspg_goniometric_light_at(VspgPointLight *l, const float ctm[16] /* or NULL */);
/* Fills `scene` with the App.-F fog box: box [-1,1]^3, Kd .73 walls, 0.5x0.5 ceiling
 * light Le (17,12,4) at y=.999, homogeneous fog sigma_a .05 sigma_s .45 g 0, camera at
 * (0,0,-.95) looking +z, fov 60. */
int vspg_scene_fog_box(VspgScene *scene, int xres, int yres);

/* ---- renderer life cycle ----------------------------------------------------------- */
/* Replaces Integrator::Create("guidedvolpathvspg", ...) + the integrator constructor
 * (src/pbrt/cpu/integrators.cpp:3739-3744, guidedvolpathvspgintegrator.cpp:61-198):
 * validates parameters, uploads scene and medium, allocates film, image-space VSP buffer
 * and path-state queues on `cfg->device`. */
int vspg_renderer_create(const VspgScene *scene, const VspgIntegratorParams *params,
                         const VspgRenderConfig *cfg, VspgRenderer **out);
/* The same with image textures on the diffuse reflectance of rectangles and triangles (VspgSceneTextures, above); textures == NULL or
 * a zeroed record: exactly vspg_renderer_create. */
int vspg_renderer_create_textured(const VspgScene *scene, const VspgSceneTextures *textures, const VspgIntegratorParams *params,
                                  const VspgRenderConfig *cfg, VspgRenderer **out);
/* Replaces ~GuidedVolPathVSPGIntegrator (guidedvolpathvspgintegrator.cpp:200-228). */
int vspg_renderer_destroy(VspgRenderer *r);

/* Uploads trained guiding fields: surface_field feeds SurfaceSamplingDistribution::Init
 * (guiding.h:90), volume_field feeds VolumeSamplingDistribution::Init (guiding.h:388); either may be
 * NULL (= untrained, Init() returns false as OpenPGL does before the first Field::Update).  Until
 * this is called a renderer created with surfaceguiding / volumeguiding / vspsecondaryguiding
 * refuses to render (VSPG_ESCOPE): the reference would train the field itself. */
int vspg_renderer_set_guiding_field(VspgRenderer *r, const VspgField *surface_field,
                                    const VspgField *volume_field, void *stream);

/* Replaces one wave of ImageTileIntegrator::Render -- the ParallelFor2D over all pixels
 * for sample indices [wave_start, wave_end) (src/pbrt/cpu/integrators.cpp:183-207),
 * i.e. EvaluatePixelSample -> Li -> SampleDistance -> film.AddSample for every pixel.
 * Asynchronous on `stream` -- with one exception: a scene with MEDIUM BOUNDARIES over a grid / NanoVDB medium (the wavefront
 * pipeline's boundary flavour) runs path-loop iterations until its path list is empty, and the emptiness test is a host read:
 * the call then synchronises `stream` once per iteration past the ones every pass needs and once at the end of every sample
 * pass (a host that overlaps work on other streams should issue that work first).  A pass whose list does not run dry
 * within the iteration cap returns VSPG_ESCOPE after the samples of the paths that did finish have entered the film. */
int vspg_render_wave(VspgRenderer *r, int wave_start, int wave_end, void *stream);

/* The same over a pixel window: the film's Bounds2i pixelBounds (the "cropwindow" / "pixelbounds" of src/pbrt/film.cpp:97-172), which
 * is all the render loop covers (`film.PixelBounds()`, src/pbrt/cpu/integrators.cpp:111,183).  [x0, x1) x [y0, y1) in absolute film
 * pixels; the library is strict -- 0 <= x0 < x1 <= xres and the same in y, else VSPG_EINVAL (clamping to the frame and the
 * degenerate-bounds error are the host adapter's job, as they are Film's).  The launch runs EvaluatePixelSample -> Li -> film.AddSample
 * for the window's pixels and this shard's sample indices of [wave_start, wave_end), and touches nothing that belongs to a pixel
 * outside the window: film, image-space statistics, TrBuffer, training records and counters.  Every per-pixel buffer keeps its
 * xres * yres size and absolute indexing (a renderer may be given several windows in its lifetime), and vspg_post_process_wave /
 * _step stay whole-image.  Pixel samples are independent, so disjoint windows that tile the frame give the film, statistics and
 * counters of one full-frame launch bit for bit.  Streams, parked one-sample results, shards, the boundary pipeline's host
 * synchronisation and the VSPG_ESCOPE cases are vspg_render_wave's; the kernel is the one vspg_renderer_kernel_name reports, in
 * every arithmetic mode.  vspg_render_wave(r, a, b, s) == vspg_render_window(r, 0, 0, xres, yres, a, b, s). */
int vspg_render_window(VspgRenderer *r, int x0, int y0, int x1, int y1, int wave_start, int wave_end, void *stream);

/* Replaces GuidedVolPathVSPGIntegrator::PostProcessWave
 * (guidedvolpathvspgintegrator.cpp:230-260): waveCounter++, image-space VSP buffer update
 * when waveCounter == 2^bufferWave.  Asynchronous on `stream`. */
int vspg_post_process_wave(VspgRenderer *r, void *stream);

/* The same after a STEP that covered n_waves sample indices -- a sharded render: every rank runs its own
 * sample index of the step, then all ranks post-process with n_waves = the number of ranks.  waveCounter += n_waves;
 * the image-space buffer update runs on the step that takes waveCounter to or past 2^bufferWave (n_waves = 1: exactly
 * the reference's schedule, :251).  isg_stats_sum: DEVICE pointer to W*H*VSPG_ISG_STATS floats holding the SUM over
 * all ranks of the per-rank statistics (vspg_isg_stats_device_ptr, all-reduced by the caller -- only needed when
 * vspg_isg_update_due() says the update falls on this step), or NULL to use the renderer's own.  The renderer's own
 * statistics are never overwritten, so nothing is counted twice.  N ranks stepping this way compute what ONE renderer
 * computes that renders [w, w + N) per step and post-processes with n_waves = N (up to float summation order of the
 * statistics).  vspg_post_process_wave(r, s) == vspg_post_process_step(r, 1, NULL, s). */
int vspg_isg_update_due(VspgRenderer *r, int n_waves);
int vspg_post_process_step(VspgRenderer *r, int n_waves, const float *isg_stats_sum, void *stream);

/* Sharded guiding-field training ("all-reduce guiding samples / statistics per wave").  Field::Update (:239) fits
 * the field from sufficient statistics accumulated over the step's radiance samples.  With an exchange hook installed, the
 * update sums those statistics over the ranks at its accumulation points -- the sample count and weight, then (both fields
 * in one buffer) the position statistics before the split, after it, and the EM step's: five in-place sum all-reduces of at
 * most 2.3 MB per training step -- and continues from the sums, so EVERY rank fits the SAME field from ALL ranks' samples: N ranks stepping
 * this way train what one renderer trains that renders [w, w + N) per step (up to float summation order; the ranks' fields
 * are bit-identical to each other when the all-reduce hands every rank the same bits, as RCCL's and gloo's do).
 * `fn` sums n_floats floats at dev_ptr in place over the ranks, enqueued on `stream`; it returns 0 or an error code that
 * vspg_post_process_step passes on.  Every rank must install a hook (or none): the hook is called the same number of times
 * on every rank -- the decision to update is taken on the summed sample count.  NULL removes it. */
typedef int (*VspgExchangeFn)(float *dev_ptr, size_t n_floats, void *stream, void *user);
int vspg_renderer_set_exchange(VspgRenderer *r, VspgExchangeFn fn, void *user);

/* Name of the kernel instantiation vspg_render_wave launches for this renderer as it stands (bench / profile
 * bookkeeping; static storage). */
const char *vspg_renderer_kernel_name(VspgRenderer *r);

/* The arithmetic the path kernels compute in (ABI 7; csrc/vspg_arith.h).  The reference has no such switch: its float arithmetic is
 * what its compiler makes of src/pbrt/util/sampling.h:222-225, media_sampleTMaj.h:379-404 ... -- IEEE division, glibc's libm.
 *   VSPG_ARITH_EXACT         (default) that arithmetic bit for bit: the mode every parity test and the benchmark's `value` run in;
 *   VSPG_ARITH_FAST_WEIGHTS  quotients that only scale a path's contribution through v_rcp_f32; every path keeps the oracle's
 *                            trajectory, radiance agrees to float rounding (relMSE vs the exact film ~1e-13);
 *   VSPG_ARITH_FAST          every division / square root at 2.5 ulp, the hardware's log / sin / cos: the same estimator, but not the
 *                            oracle's paths (the reference seeds a shadow ray's RNG from the bits of its origin and direction,
 *                            guidedvolpathvspgintegrator.cpp:1193) -- equal in distribution, validated statistically.
 * Returns VSPG_ESCOPE (and names the kernel) for configurations without tolerance-mode instantiations: they cover unguided renders of
 * rectangle scenes over a homogeneous medium and unguided "resampling" renders over a "uniformgrid" medium. */
#define VSPG_ARITH_EXACT 0
#define VSPG_ARITH_FAST_WEIGHTS 1
#define VSPG_ARITH_FAST 2
int vspg_renderer_set_arithmetic(VspgRenderer *r, int mode);
int vspg_renderer_get_arithmetic(VspgRenderer *r);

/* Film access.  The film is W*H float4 {sum w*r, sum w*g, sum w*b, sum w} in HBM
 * (the accumulate contract of RGBFilm::AddSample, src/pbrt/film.h:251-267, in float).
 * vspg_film_device_ptr exposes it for the frame-end RCCL all-reduce.
 * A one-sample vspg_render_wave may leave its samples parked beside the film until the next launch starts (it adds them as each
 * pixel's new path begins, in the same order as ever); every call that reads or writes the film or the image-space statistics
 * adds them first, on the stream it is given (ordered behind the launch that parked them by an event when the streams differ).
 * The two *_device_ptr getters have no stream: they add the parked samples on the stream of the launch that parked them and
 * wait for that stream, so what the pointer shows is complete AT THE TIME OF THE CALL.  The pointer VALUE is fixed for the
 * renderer's lifetime, the CONTENTS are not: a host that keeps the pointer across waves (to all-reduce the film or the
 * statistics plane itself) must call vspg_flush(r, stream) -- asynchronous, no host wait -- after the last vspg_render_wave and
 * before it reads through the pointer on `stream` (or on work ordered behind it); a no-op when nothing is parked.
 * The same contract covers PATHS: a one-sample wave of the barrier-free workgroup kernel may also leave the paths that were in flight
 * when its tiles ran out suspended beside the film; the next such wave resumes them, and until then the film, the statistics and
 * the counters lack them as well as the parked samples.  vspg_flush and every accessor named above -- and vspg_get_counters,
 * vspg_reset_counters, vspg_renderer_set_arithmetic, vspg_renderer_set_camera, the buffer setters, the due update of vspg_post_process_step -- finish them
 * first (one short launch on the call's stream); vspg_renderer_destroy drops them.  VSPG_WG3_CARRY=0 in the environment (read
 * per wave) makes every wave finish its own paths.
 * vspg_film_error_enqueue and vspg_film_resolve (below) read the film and belong to this list: each finishes parked samples and
 * suspended paths first, on its stream, so its record or image is of the COMPLETE film -- a host that records or writes an image after
 * every wave therefore gives up the carry of in-flight paths between waves (every wave is followed by the short drain launch). */
int vspg_flush(VspgRenderer *r, void *stream);
int vspg_film_device_ptr(VspgRenderer *r, float **dev_ptr, size_t *n_floats);
int vspg_film_read(VspgRenderer *r, float *host_rgbw /* W*H*4 */, void *stream);
int vspg_film_clear(VspgRenderer *r, void *stream);

/* Film error against a reference image, reduced on the device: what ImageTileIntegrator::Render computes after every wave when
 * --mse-reference-image is given (src/pbrt/cpu/integrators.cpp:129-158, :243-262) -- Image::MSE (src/pbrt/util/image.cpp:575-607) and
 * its relative form Image::MRSE (:609-639) of the film against the reference image -- without reading the film back.
 * Over the window [x0,x1) x [y0,y1) and per channel c, with v_c = RGBFilm::GetPixelRGB (film.h:269-287: w != 0 ? rgbSum_c / w :
 * rgbSum_c, one float division):
 *   se  = Sqr(double(v_c) - double(ref_c))                              (image.cpp:594)
 *   rse = Sqr(double(v_c) - double(ref_c)) / Sqr(ref_c + 0.01)          (image.cpp:626; the sum and the square in double)
 * a term that IsInf is skipped, a NaN term is not (:595-597, :627-629).  A record carries the six SUMS in double and the window's
 * pixel count: sums of disjoint windows add, means do not.  The reference's last step is the caller's:
 *   mse_c = Float(sum_se[c] / (Float(x1 - x0) * Float(y1 - y0))) (image.cpp:603-606), Average() = (mse_0 + mse_1 + mse_2) / 3 in Float
 *   (image.h:205-210).
 * The order in which a sum is associated is a fixed function of the window alone (csrc/vspg_film_error.h): the same film and window
 * give the same bits on every call.  device_ticks is the device's constant-rate clock at the moment the record was completed, so
 * error-over-time curves need no host synchronisation per wave; tick_khz is its rate. */
typedef struct VspgFilmError {
    int32_t  x0, y0, x1, y1;   /* the window */
    int32_t  tag;              /* caller's label, e.g. samples per pixel so far */
    uint32_t tick_khz;         /* rate of device_ticks (hipDeviceAttributeWallClockRate), filled in at read */
    uint64_t n_pixels;         /* (x1-x0)*(y1-y0): the divisor of Image::MSE */
    uint64_t device_ticks;     /* device clock when the record was completed */
    double   sum_se[3];        /* image.cpp:575-607 before the division */
    double   sum_rse[3];       /* image.cpp:609-639 before the division */
} VspgFilmError;
#define VSPG_FILM_ERROR_LOG_RECORDS 4096
/* The reference image: full frame, absolute indexing, like every per-pixel buffer (a renderer may be given several windows).  The
 * first call allocates the device copy (a float4 per pixel), the per-row partial sums and the log of VSPG_FILM_ERROR_LOG_RECORDS
 * records; a renderer that never calls it allocates and launches nothing.  NULL removes the image (records already in the log stay).
 * Synchronises `stream`. */
int vspg_renderer_set_reference_image(VspgRenderer *r, const float *host_rgb /* W*H*3, row-major, top row first; NULL removes */, void *stream);
/* Appends one record of the film as it stands to the device-side log.  Asynchronous on `stream`; window rules are
 * vspg_render_window's.  VSPG_EINVAL without a reference image and on a full log (nothing is dropped silently).  It reads the film
 * only.  Enqueues of one renderer on different streams are ordered behind each other by an event. */
int vspg_film_error_enqueue(VspgRenderer *r, int x0, int y0, int x1, int y1, int tag, void *stream);
/* Synchronises `stream`, copies the records in enqueue order and empties the log.  max_records smaller than the log's content:
 * VSPG_EINVAL, log untouched. */
int vspg_film_error_read(VspgRenderer *r, VspgFilmError *out, size_t max_records, size_t *n_out, void *stream);

/* The film resolved to pixel values on the device: what RGBFilm::GetImage hands RGBFilm::WriteImage (src/pbrt/film.cpp:531-569), over
 * the window [x0,x1) x [y0,y1) (vspg_render_window's rules: strict, VSPG_EINVAL otherwise).  Per pixel and channel
 *   v_c = w != 0 ? sum_c / w : sum_c      (RGBFilm::GetPixelRGB, film.h:269-287: one float division, no colour transform).
 * VSPG_RESOLVE_F32 stores v_c unchanged; *n_clamped is 0.  VSPG_RESOLVE_F16 stores Half(v_c) (util/float.h:417-463: round to nearest
 * even, subnormal halves, >= 65520 to +-inf, any NaN to 0x7e00 | sign) after the clamp of film.cpp:544-556: with m = r; if (m < g) m = g;
 * if (m < b) m = b; -- std::max({r,g,b}), NaN behaviour included -- iff m > 65504 every channel > 65504 becomes 65504 and the pixel
 * counts once in *n_clamped ("%d pixel values clamped to maximum fp16 value.").  Negative overflow is not clamped: -inf.
 * out_bytes must be (x1-x0)*(y1-y0)*3*(2|4), else VSPG_EINVAL with nothing written.  It belongs to the calls that finish parked
 * samples and suspended paths first (above), on `stream`, and synchronises `stream` like vspg_film_read.  The first call allocates a
 * staging buffer of xres*yres*12 bytes and a 4-byte counter, freed at destroy; a renderer that never calls it allocates and launches
 * nothing.  6 (or 12) bytes per pixel cross to the host instead of vspg_film_read's 16, and in the scan-line layout they are an
 * OpenEXR scan-line block's payload as they stand (channels sorted by name: B, G, R). */
#define VSPG_RESOLVE_F32 0
#define VSPG_RESOLVE_F16 1
#define VSPG_RESOLVE_RGB 0           /* interleaved R,G,B per pixel, rows top first: pbrt's Image memory layout */
#define VSPG_RESOLVE_SCANLINE_BGR 1  /* per row: the row's B values, then its G values, then its R values: an EXR scan line of channels B,G,R */
int vspg_film_resolve(VspgRenderer *r, int x0, int y0, int x1, int y1, int format, int layout,
                      void *host_out, size_t out_bytes, uint64_t *n_clamped /* or NULL */, void *stream);

/* Image-space VSP buffer (stands in for openpgl ImageSpaceGuidingBuffer,
 * guidedvolpathvspgintegrator.cpp:161-178, 1098-1112). */
int vspg_vsp_buffer_device_ptr(VspgRenderer *r, float **dev_ptr, size_t *n_floats);
int vspg_vsp_buffer_read(VspgRenderer *r, float *host_vsp /* W*H */, int *is_ready,
                         void *stream);
/* ImageSpaceGuidingBuffer(fileName) (guidedvolpathvspgintegrator.cpp:151-159): the buffer is used as handed over
 * (ready from the first wave on) and never updated again (calculateImageSpaceGuidingBuffer = false, :251-256).
 * Values outside [0,1] mean "no estimate for this pixel" (:1101-1112). */
int vspg_vsp_buffer_load(VspgRenderer *r, const float *host_vsp /* W*H */, void *stream);
/* per-pixel sufficient statistics (W*H*VSPG_ISG_STATS floats) for multi-GPU all-reduce */
#define VSPG_ISG_STATS 8
int vspg_isg_stats_device_ptr(VspgRenderer *r, float **dev_ptr, size_t *n_floats);

/* Transmittance buffer (TrBuffer, src/pbrt/cpu/trbuffer.h:17-104): per-pixel running mean of the primary
 * ray's ratio-tracking transmittance estimate, recorded by the resampling routine
 * (guidedvolpathvspgintegrator.cpp:727-728) while params.storeTrBuffer is set (or NDS+ is requested and no
 * buffer was handed over).  get = what TrBuffer::Store writes (RGB per pixel, row-major; host_spp, optional:
 * the per-pixel sample counts, for merging the buffers of sample-sharded ranks).  set = TrBuffer(fileName):
 * the renderer stops recording and NDS+ (vspsamplingmethod "nds" + collisionProbabilityBias) biases the
 * primary ray's real/null-collision probability with it (:929-938). */
int vspg_renderer_get_tr_buffer(VspgRenderer *r, float *host_rgb /* W*H*3 */, int32_t *host_spp /* W*H or NULL */,
                                void *stream);
int vspg_renderer_set_tr_buffer(VspgRenderer *r, const float *host_rgb /* W*H*3 */, void *stream);

int vspg_get_counters(VspgRenderer *r, VspgCounters *out, void *stream);
int vspg_reset_counters(VspgRenderer *r, void *stream);

/* ---- parity / debug entry points ---------------------------------------------------- */
/* Runs EvaluatePixelSample for n explicit (pixel, sampleIndex) pairs with the renderer's
 * current VSP buffer and returns the camera-weighted radiance L (RGB) per path plus the
 * number of path-loop segments -- the analogue of --debugstart x,y,n
 * (src/pbrt/cpu/integrators.cpp:77-95).  Host arrays. */
int vspg_trace_paths(VspgRenderer *r, int n, const int32_t *pixel_xy /* 2n */,
                     const int32_t *sample_index /* n */, float *out_L /* 3n */,
                     int32_t *out_segments /* n or NULL */, void *stream);

/* Batch drivers of the free-flight layer on device, for bit-level checks against the
 * oracle and the reference known answers.  All arrays are HOST
 * arrays of length n (or 3n where noted). */
typedef struct VspgTmajQuery {
    float o[3], d[3];  /* ray (d need not be normalised) */
    float tMax;
    float u;           /* traversal sample */
    float rng_a, rng_b;/* RNG(Hash(rng_a), Hash(rng_b)), integrator.cpp:323-325 */
    float vsp;         /* <0: guideScatterDecision=false */
    int32_t channel;   /* hero channel lambda.ChannelIdx() */
    int32_t stop_after;/* callback returns false at this (1-based) callback; 0 = never */
} VspgTmajQuery;

typedef struct VspgTmajResult {
    float T_maj[3];       /* returned majorant transmittance */
    float r_u_factor[3];  /* OpticalDepthSpace only (else 1) */
    float last_t;         /* distance along the NORMALISED ray of the last callback, -1 if none */
    float last_p[3];      /* its position */
    int32_t n_callbacks;
    float sum_sigt_over_maj; /* sum over callbacks of (sigma_t/sigma_maj)[channel] */
    float vrc;            /* Resampling: volumeRatioZeroCandidateCompensation */
    float majorant_scale; /* Resampling */
} VspgTmajResult;

enum { VSPG_TMAJ_PLAIN = 0, VSPG_TMAJ_OPTICAL_DEPTH = 1, VSPG_TMAJ_RESAMPLING = 2 };

/* Ray queries against the renderer's geometry (ABI 7): the batch driver behind the replays of the reference's own shape tests
 * (src/pbrt/shapes_test.cpp: Triangle Watertight / Reintersect / BadCases, FullSphere Reintersect) -- what Integrator::Intersect
 * (cpu/integrators.cpp:341-349) returns for `ray`, then, from that hit, the ray Interaction::SpawnRay(w) (`mode` 1,
 * interaction.h:99-101) or Interaction::SpawnRayTo(point w) (`mode` 2, interaction.h:104-108, ray.h:93-98) intersected again with
 * tMax2: closest hit (Intersect) and any hit (IntersectP). */
typedef struct {
    float o[3], d[3], tMax;
    int32_t mode;          /* 0: the first intersection only; 1: SpawnRay(w); 2: SpawnRayTo(w) */
    float w[3], tMax2;
} VspgRayQuery;
typedef struct {
    int32_t hit;           /* the first ray hit something */
    int32_t prim;          /* rectangle index | 1000000 + triangle index in the caller's soup | 2000000 + sphere index */
    float t, p[3], n[3];   /* tHit, the interaction point (midpoint of pi), the surface normal */
    float o2[3], d2[3];    /* the spawned ray */
    int32_t hit2, any2;    /* Intersect / IntersectP of the spawned ray */
    float t2;
} VspgRayResult;
int vspg_ray_batch(VspgRenderer *r, int n, const VspgRayQuery *q, VspgRayResult *out, void *stream);
/* Replaces SampleT_maj / SampleT_maj_OpticalDepthSpace / SampleT_maj_Resampling
 * (src/pbrt/media_sampleTMaj.h:49-117, 269-491, 136-248) on the renderer's medium with a
 * recording callback. */
int vspg_sample_tmaj_batch(VspgRenderer *r, int variant, int n, const VspgTmajQuery *q,
                           VspgTmajResult *out, void *stream);

/* Read-back of a grid / NanoVDB-semantics medium's device storage (test + diagnostics): the "octet bricks" the kernels read.
 * The grid is cut into bnx x bny x bnz bricks of 8 x 8 x 8 octets (bn = (n + 8) / 8 per axis; brick number = (bz * bny + by) * bnx +
 * bx; brick b holds the octets of base voxels 8b - 1 .. 8b + 6 per axis, i.e. raw voxels 8b - 1 .. 8b + 7, zero outside the grid).
 * An octet is the eight raw values {(x,y,z), (x+1,y,z), (x,y+1,z), (x+1,y+1,z), then the same four at z+1} of its base voxel;
 * a brick stores its 512 octets x fastest.  `indexed` = 1: only bricks that hold a non-zero value are stored, in increasing
 * brick number, behind an index (slot, or -1 = all zero); 0: every brick is stored and a brick's slot is its number.
 * VSPG_EINVAL for a renderer whose medium is not a grid. */
typedef struct VspgBrickInfo {
    int32_t bnx, bny, bnz;
    int32_t indexed;
    uint64_t n_stored;      /* stored bricks (dense: bnx * bny * bnz) */
    uint64_t index_bytes;   /* device bytes held by the index (0 when dense) */
    uint64_t octet_bytes;   /* device bytes held by the octets (one placeholder brick when n_stored == 0) */
} VspgBrickInfo;
int vspg_brick_info(VspgRenderer *r, VspgBrickInfo *out);
/* index: bnx * bny * bnz slots (dense: the identity, the slot the kernels compute); octets: n_stored * 512 * 8 floats.  HOST
 * arrays, either may be NULL. */
int vspg_brick_read(VspgRenderer *r, int32_t *index, float *octets, void *stream);

/* In-place update of a grid / NanoVDB-semantics medium's values (a volume sequence's next frame, or a tensor another program has
 * just written on the device): replaces the `nx * ny * nz` samples (x fastest, the layout the renderer was created with) of the
 * density grid (VSPG_GRID_DENSITY) or of the temperature grid (VSPG_GRID_TEMPERATURE: a plain copy, accepted only on a renderer
 * created WITH a temperature grid -- the kernel instantiation depends on whether there is one).  Bounds, transform, index_min,
 * voxel_size, grid_origin, density_offset, majorant_scale and the sigma spectra stay.  Afterwards every launch and batch entry point
 * behaves as if the renderer had been created with the new values: the majorant grid is rebuilt on the device (one workgroup per
 * cell takes the maximum over the cell's voxel box; the per-axis box tables are the host's, those vspg_renderer_create uses) and so
 * are the octet bricks, in the layout -- dense or indexed -- create chose (VSPG_DENSE_BRICKS is not read again; an indexed renderer
 * stores the bricks the NEW values occupy).
 *   memory = VSPG_MEM_HOST:   `values` is a host array.
 *   memory = VSPG_MEM_DEVICE: `values` is a pointer on the renderer's device, readable on `stream` at the time of the call (a torch
 *                             tensor's data_ptr(), say).  It never crosses to the host and is not copied on the device either: the
 *                             builders read it in place.
 * The call first finishes parked samples and suspended paths on `stream` (they end under the medium they started in), rebuilds,
 * and synchronises `stream` before it returns, as vspg_renderer_create does: `values` may be reused at once.
 * It touches nothing else: not the film (beyond resolving those parked samples), the image-space statistics, the VSP buffer and its
 * ready flag, the TrBuffer, the guiding fields and the training state, the counters, the reference image or the error log.  A caller
 * starting a new frame calls vspg_film_clear itself.
 * NaN voxels are the caller's contract to avoid: the majorant of a box that holds one is unspecified (as create's is, where it
 * depends on the order of a host loop).  For finite values the majorants equal create's (the sign of an all-zero box's zero apart).
 * VSPG_EINVAL, with the renderer exactly as it was: a null argument, an unknown `which` or `memory`, n_floats != nx*ny*nz, a medium
 * that is neither GRID nor NANOVDB, TEMPERATURE on a renderer created without a temperature grid. */
#define VSPG_GRID_DENSITY     0
#define VSPG_GRID_TEMPERATURE 1
#define VSPG_MEM_HOST   0
#define VSPG_MEM_DEVICE 1
int vspg_renderer_update_grid(VspgRenderer *r, int which, const float *values, size_t n_floats, int memory, void *stream);
/* The same for an RGB grid medium (VSPG_MEDIUM_RGBGRID): replaces the values of its sigma_a, sigma_s and / or Le grid in place.  ONE
 * call takes the three grids, because the majorant grid depends on both sigma grids and is rebuilt once; a NULL pointer means "keep
 * this grid".  Every given grid holds n_floats = 3 * nx * ny * nz floats (R, G, B per voxel, x fastest, as at create); `memory`
 * (VSPG_MEM_HOST / VSPG_MEM_DEVICE) holds for all given pointers: a device source is read where it lies, a host source is staged.
 * Dimensions, bounds, transform, rgb_sigma_scale and rgb_le_scale stay create's.  Afterwards the renderer computes, bit for bit, what a
 * renderer created with the new values computes (the sign of a majorant that is a zero apart): the octet image of each given sigma grid
 * is rebuilt on the device (one workgroup per 8^3 brick, every byte of the image written), the majorant grid by one workgroup per cell --
 * over the new values of a grid that is given and over the stored octets of one that is kept --, and the Le grid is a plain copy.
 * Order and what persists are vspg_renderer_update_grid's: every refusal, then parked samples and suspended paths are finished on
 * `stream` (under the old values), the rebuild, and `stream` is synchronised before the call returns; film, statistics, VSP buffer,
 * TrBuffer, guiding fields, training state, counters, reference image and error log stay.
 * VSPG_EINVAL, with majorants, octets, Le, film, counters and parked samples exactly as they were: a null renderer; a medium that is
 * not RGBGRID; all three pointers NULL; n_floats != 3*nx*ny*nz; an unknown `memory`; a grid the renderer was created without (an absent
 * grid has no storage: the kernels branch the constant in); a value in a given grid that is negative, NaN or infinite (-0.0 passes, as
 * at create) -- checked on the host for a host source and by one read pass on the device for a device source, before anything of the
 * renderer is written; the message names the grid. */
int vspg_renderer_update_rgb_grids(VspgRenderer *r, const float *sigma_a, const float *sigma_s, const float *Le,
                                   size_t n_floats /* 3*nx*ny*nz, per given grid */, int memory, void *stream);
/* Read-back of the device image of one sigma grid of an RGB grid medium (test + diagnostics): which = 0 sigma_a, 1 sigma_s.  host_out:
 * n_floats == bnx * bny * bnz * 512 * 32 floats (HOST array), bn = (n + 8) / 8 bricks per axis, brick number = (bz * bny + by) * bnx + bx;
 * a brick holds 8 x 8 x 8 octets (x fastest) of base voxels 8b - 1 .. 8b + 6, an octet the eight corners (x fastest, then y, then z) of its
 * base voxel as R, G, B, 0 each; zero outside the grid and in the octets behind base voxel n - 1.  VSPG_EINVAL for another medium, a
 * grid the renderer was created without, another `which` or a wrong size.  Synchronises `stream`. */
int vspg_rgb_octets_read(VspgRenderer *r, int which /* 0 sigma_a, 1 sigma_s */, float *host_out, size_t n_floats, void *stream);
/* Read-back of the majorant grid the kernels read (test + diagnostics), x fastest: res^3 floats with res = 16 for a GRID or RGBGRID medium,
 * 64 for NANOVDB semantics.  host_out: n_floats == res^3 floats (HOST array); res (may be NULL) receives the resolution.
 * VSPG_EINVAL for other media or a wrong n_floats (res is still reported for a grid medium, so a caller can size its array).
 * Synchronises `stream`. */
int vspg_majorant_read(VspgRenderer *r, float *host_out, size_t n_floats, int32_t *res, void *stream);
/* Batch driver of a grid medium's point query (parity tests), as the path kernels evaluate it: per element i, for the render-space
 * point p[3i..], out[10i..] = {sigma_a (3), sigma_s (3), Le (3)} of SamplePoint(p) -- Le as MediumProperties holds it, 0 for a
 * blackbody medium, whose emission needs the path's wavelengths -- then the value of the majorant-grid cell that holds p (the cell the
 * DDA starts in: floor(Offset(p) * res) per axis; 0 where p lies outside the bounds).  HOST arrays.  Serves GRID, NANOVDB and RGBGRID;
 * VSPG_EINVAL for other media. */
#define VSPG_MEDIUM_POINT_OUT 10
int vspg_medium_point_batch(VspgRenderer *r, int n, const float *p /*3n*/, float *out /*10n*/, void *stream);

/* Primitive batch (bit-exact layer): for each i computes on device
 *   hash[i]   = Hash(f[i])                      (src/pbrt/util/hash.h:100)
 *   rng_u32[i]= RNG(Hash(f[i]),Hash(g[i])).Uniform<uint32_t>()  (util/rng.h:82-88,119-125)
 *   fastexp[i]= FastExp(f[i])                   (util/math.h:450-474)
 */
int vspg_primitives_batch(VspgRenderer *r, int n, const float *f, const float *g,
                          uint64_t *hash, uint32_t *rng_u32, float *fastexp, void *stream);

/* Batch driver of the guiding-cache query (parity tests): for each i initialises the distribution
 * at p[i] (surface: cosine product with n[i]; volume: HG product with wo = n[i], asymmetry g) and
 * returns PDF(wi[i]), IncomingRadiancePDF(wi[i]), VolumeScatterProbability(wi[i]) and one sample
 * SamplePDF(u[i]) -> (ws[i], pdf_s[i]).  out_ok[i] = Init() result.  HOST arrays. */
int vspg_guiding_query_batch(VspgRenderer *r, int is_volume, float g, int n, const float *p /*3n*/,
                             const float *n_or_wo /*3n*/, const float *wi /*3n*/, const float *u /*2n*/,
                             int32_t *out_ok, float *out_pdf, float *out_incoming_pdf, float *out_vsp,
                             float *out_ws /*3n*/, float *out_pdf_s, void *stream);

/* Device float libm batch: logf(x), sinf(x), cosf(x) as the kernels evaluate them; they must
 * equal the host libm the CPU reference run uses (std::log/std::sin/std::cos of float,
 * src/pbrt/util/sampling.h:222-225, 325-341, src/pbrt/util/vecmath.h:1666-1672). */
/* Training state / radiance samples recorded since the last update (test + diagnostics; order is
 * unspecified) / the field as it stands (Field::Store counterpart: pass NULL arrays to get the sizes). */
int vspg_renderer_training_stats(VspgRenderer *r, VspgTrainStats *out, void *stream);
int vspg_train_samples_read(VspgRenderer *r, VspgTrainSample *out, size_t max_samples, size_t *n_out,
                            void *stream);
int vspg_renderer_get_guiding_field(VspgRenderer *r, int volume_field, VspgKdNode *nodes,
                                    VspgFieldRegion *regions, int32_t *n_nodes, int32_t *n_regions,
                                    void *stream);

int vspg_libm_batch(VspgRenderer *r, int n, const float *x, float *logf_out, float *sinf_out,
                    float *cosf_out, void *stream);
/* out[i] = (float)(-log(1.0 - (double)x[i])) as the kernels evaluate it: the DOUBLE-precision
 * std::log of the optical-depth-space distance sampling (src/pbrt/media_sampleTMaj.h:379-404). */
int vspg_libm_log1m_batch(VspgRenderer *r, int n, const float *x, float *out, void *stream);
/* out[i] = powf(x[i], y[i]) as the kernels evaluate it (the std::pow of the NDS+ bias,
 * src/pbrt/cpu/guidedvolpathvspgintegrator.cpp:937): bit-identical to glibc 2.35's powf. */
int vspg_libm_powf_batch(VspgRenderer *r, int n, const float *x, const float *y, float *out, void *stream);
/* out6[6 i ..] = {lambda_0..2, Le_0..2}: the wavelengths of SampledWavelengths::SampleVisible(u[i]) (util/spectrum.h:369-386; the
 * host's atanhf, bit for bit) and BlackbodySpectrum(T[i]).Sample(lambda) (:568-588) as the kernels evaluate a temperature grid's
 * emission (media.h:333-341, :724-735). */
int vspg_blackbody_batch(VspgRenderer *r, int n, const float *u, const float *T, float *out6, void *stream);

/* The image of an image infinite light (slot `infinite_light_index` of the scene's infinite lights, which must be of type
 * VSPG_LIGHT_IMAGE_INFINITE): an equal-area octahedral map of the whole sphere (util/math.cpp:292-361), res x res texels.
 *   host_rgb          res*res*3 floats (HOST array), top row first, R G B per texel, as pbrt's Image holds them
 *   res               1 .. VSPG_ENV_MAX_RES (4096)
 *   render_from_light rows 0..2 of the light's transform, 3 x 4 row-major (the translation column is read by nothing: the light
 *                     transforms directions only); NULL = identity
 * The host builds, in the reference's order of operations, the texel table, d = the average of R, G, B per texel
 * (Image::GetSamplingDistribution, util/image.h:450-469), the COMPENSATED function max(d - average(d), 0) (all ones where that
 * leaves nothing; lights.cpp:1104-1110) and its PiecewiseConstant2D (util/sampling.h:625-649, 737-754), uploads them and swaps them
 * in behind `stream`.  Only the compensated distribution exists on the device: every call site of the integrator samples and
 * evaluates lights with allowIncompletePDF = true (guidedvolpathvspgintegrator.cpp:365, 1166), so the plain distribution of
 * lights.cpp:1100-1102 is never read.  The "power" light sampler's table is rebuilt with the light's Phi (lights.cpp:1125-1142).
 * Like vspg_renderer_update_grid the call finishes parked samples and suspended paths on `stream` first, synchronises `stream`
 * before it returns, and touches nothing else: film, VSP buffer, guiding fields and training state, counters and the error log
 * persist.
 * VSPG_EINVAL, with the renderer exactly as it was: a null renderer or image, an index that is no infinite light or one of another
 * type, res < 1 or res > VSPG_ENV_MAX_RES, a texel that is NaN or infinite (lights.cpp:1694-1703), a singular or non-finite matrix. */
#define VSPG_ENV_MAX_RES 4096
int vspg_renderer_set_environment_image(VspgRenderer *r, int infinite_light_index, const float *host_rgb, int res,
                                        const float *render_from_light /*12 or NULL*/, void *stream);
/* Gives a projection or goniometric light (point-light slot `point_light_index`) its image, modelled on the call above.
 *   host_pixels   xres*yres*channels floats (HOST array), top row first
 *   channels      3 (R, G, B) for a projection slot, 1 (Y) for a goniometric slot
 *   xres, yres    1 .. VSPG_LIGHT_IMAGE_MAX_RES (4096); a goniometric image must be square (lights.cpp:680-685)
 * The host builds the device image (a projection slide as one float4 per texel, already clamped at zero, pad 0; a goniometric map as
 * one float per texel, as given), the slide's screen window and A, the light's Phi (ProjectionLight::Phi lights.cpp:404-424 per
 * channel of I; GoniometricLight::Phi :603-610) for the "power" alias table and its LightBounds (:426-441, :612-624; the power uses
 * the largest component of I) for the "bvh" tree, uploads the image into one allocation of its own and swaps it in behind `stream`;
 * the old image is released after the swap.  It finishes parked samples and suspended paths on `stream` first, synchronises `stream`
 * before it returns, and keeps everything vspg_renderer_set_environment_image keeps.
 * VSPG_EINVAL, with the renderer exactly as it was and before any allocation: a null argument, an index that is no point-light slot
 * or a slot of another type, a wrong `channels` for the slot's type, a resolution out of range or a non-square goniometric image, a
 * pixel that is NaN or infinite (lights.cpp:502-510, :669-678). */
int vspg_renderer_set_light_image(VspgRenderer *r, int point_light_index, const float *host_pixels, int xres, int yres,
                                  int channels, void *stream);
/* Batch driver of the image infinite light (parity tests), as the path kernels evaluate it.  dirs: 3n floats, u: 2n floats, out:
 * VSPG_ENVLIGHT_OUT floats per element (HOST arrays):
 *   [0..2] Le(dirs[i])   [3..4] the (u, v) that Le looked up   [5] PDF_Li(dirs[i])
 *   SampleLi(ctx.p = 0, u[i]):  [6] 1 = a sample, 0 = none (everything after it is 0 then)   [7..8] its (u, v)   [9..11] wi
 *   [12] pdf   [13..15] L
 * VSPG_EINVAL for a slot that vspg_renderer_set_portal_environment_image turned into a portal light (vspg_portallight_batch serves it). */
#define VSPG_ENVLIGHT_OUT 16
int vspg_envlight_batch(VspgRenderer *r, int infinite_light_index, int n, const float *dirs /*3n*/, const float *u /*2n*/,
                        float *out /*16n*/, void *stream);

/* Turns an image infinite light (slot `infinite_light_index`, type VSPG_LIGHT_IMAGE_INFINITE) into a PortalImageInfiniteLight
 * (src/pbrt/lights.h:699-808, lights.cpp:1181-1345): the same equal-area map, seen through a rectangular opening.  NEE samples only the
 * part of the map the context point sees through the portal, and an escaped ray receives radiance only where its direction, seen
 * from its ORIGIN, passes through the portal.  Arguments as vspg_renderer_set_environment_image, plus
 *   portal   12 floats: the four vertices of the opening in render space, in order round the rectangle
 * The host builds, in the reference's order of operations: portalFrame = Frame::FromXY(p03, p01); the rectified res x res image
 * (RenderFromImage at texel centres, the inverse rotation, EqualAreaSphereToSquare, Image::BilerpChannel under the octahedral wrap);
 * d = average(R, G, B) * duv_dw(centre); the summed-area table in double, stored as float (SummedAreaTable::LookupInt returns Float);
 * Area() and Phi's sums.  This is sequential host work (see DESIGN.md 4.13 for its cost at 1024^2 and 4096^2).  tan and atan2 are the
 * library's own functions (csrc/vspg_trig.h), so parity with a reference build is "the same texel except within their error bound of
 * a texel edge" -- the reference's own result depends on its platform's libm.
 * The call keeps what vspg_renderer_set_environment_image keeps: it finishes parked samples and suspended paths on `stream`,
 * synchronises, rebuilds the light sampler's tables with the portal light's Phi (lights.cpp:1262-1285); film, VSP buffer, guiding
 * fields, counters and the error log persist.  The light stays LightType::Infinite with no Bounds(): under "bvh" it sits among the
 * infinite lights as the image light does.  A later vspg_renderer_set_environment_image on the slot turns it back into a plain
 * image light, after which the renderer computes what one that never had a portal computes.
 * VSPG_EINVAL, with the renderer exactly as it was and before any allocation: every refusal of vspg_renderer_set_environment_image; a
 * null `portal` or a vertex that is NaN or infinite; an edge of zero length; a quadrilateral that fails the constructor's tests
 * (lights.cpp:1222-1228: opposite edges parallel, sides perpendicular, thresholds .001 compared in double).  The reference only prints
 * "Infinite light portal isn't a planar quadrilateral" there and renders on with a broken frame; the library refuses.
 * Scene files still refuse a "portal" parameter by name: the light is reached through this call (and the Python binding) only. */
int vspg_renderer_set_portal_environment_image(VspgRenderer *r, int infinite_light_index, const float *host_rgb, int res,
                                               const float *render_from_light /*12 or NULL*/,
                                               const float *portal /*12: four points, render space*/, void *stream);
/* Batch driver of the portal light (parity tests), as the path kernels evaluate it; the slot must hold a portal light.  ctx_p: 3n
 * floats (the context point / ray origin), dirs: 3n floats, u: 2n floats, out: VSPG_PORTALLIGHT_OUT floats per element (HOST arrays):
 *   ImageBounds(ctx_p):  [0] 1 = bounds, 0 = none   [1..4] pMin.x, pMin.y, pMax.x, pMax.y
 *   Le(ray(ctx_p, dirs)):  [5] 1 = the direction lies inside the bounds   [6..7] the direction's (u, v) where it has one   [8..10] Le
 *   [11] PDF_Li(ctx_p, dirs)
 *   SampleLi(ctx_p, u):  [12] 1 = a sample, 0 = none ([13..23] and [27..29] are 0 then)   [13..14] its (u, v)   [15] mapPDF
 *   [16] duv_dw   [17..19] wi   [20] pdf   [21..23] L   [27..29] pLight
 *   [24] [25] the trip counts of the x and y bisections   [26] why no sample: 0 a sample, 1 no bounds, 2 zero window integral,
 *   3 zero conditional integral, 4 a non-finite interpolation parameter, 5 duv_dw == 0   [30] [31] 0 */
#define VSPG_PORTALLIGHT_OUT 32
int vspg_portallight_batch(VspgRenderer *r, int infinite_light_index, int n, const float *ctx_p /*3n*/, const float *dirs /*3n*/,
                           const float *u /*2n*/, float *out /*32n*/, void *stream);
/* Reads a portal light's tables back as the renderer holds them (each pointer may be NULL): *res_out, the rectified image
 * (res*res*3), func (res*res), the float summed-area table (res*res), and record20 = {portal[0], portal[2], frame x, y, z (3 each),
 * Area(), Phi's three sums, the scene's radius (the sceneRadius of pLight = ctx.p + 2 * sceneRadius * wi)}. */
int vspg_portallight_read(VspgRenderer *r, int infinite_light_index, int *res_out, float *image, float *func, float *table,
                          float *record20 /*20*/, void *stream);

/* Batch driver of light sampling (parity tests): per element the renderer's light sampler picks a light for the context and that
 * light is sampled -- the light_sampler_sample, light_sampler_pmf and sample_light the path kernels call, under the sampler the
 * renderer was created with ("uniform", "power", "bvh") and for every light kind the scene holds.  HOST arrays.
 *   ctx_p  3n floats: the context point            ctx_n  3n floats: its normal, zeros = a medium vertex
 *   u      3n floats: the pick's variate, then the two of SampleLi
 *   out    VSPG_LIGHT_SAMPLE_OUT floats per element:
 *   [0] the picked index into the light list, -1 = none (everything after it is 0 then)   [1] the pmf Sample returned
 *   [2] PMF(ctx, that light)   [3] 1 = SampleLi gave a sample, 0 = none (everything after it is 0 then)
 *   [4..6] wi   [7..9] L   [10] pdf   [11..13] pLight   [14] 1 = a delta light   [15] 0 */
#define VSPG_LIGHT_SAMPLE_OUT 16
int vspg_light_sample_batch(VspgRenderer *r, int n, const float *ctx_p /*3n*/, const float *ctx_n /*3n*/, const float *u /*3n*/,
                            float *out /*16n*/, void *stream);

/* Batch driver of a light's PDF (parity tests): per element what the path kernels compute when a ray that leaves the context along
 * wi is to be weighed against light `light_index` of the light list -- the light_sampler_pmf, the PDF_Li (light_pdf_li for a
 * rectangle, sphere_pdf_li for a sphere), the intersection and the L the kernels call.  HOST arrays.
 *   ctx_p     3n floats: the context point      ctx_perr  3n floats: its error bounds (Point3fi(p, pError)), NULL = exact points
 *   ctx_n     3n floats: its normal, zeros = a medium vertex      wi  3n floats: the ray's direction (as given, not normalised here)
 *   out       VSPG_LIGHT_PDF_OUT floats per element:
 *   [0] PDF_Li(ctx, wi)   [1] lightSampler.PMF(ctx, light)   [2] 1 = the ray ctx.SpawnRay(wi) hits the light's shape, 0 = not
 *   (everything after it is 0 then)   [3..5] L at the hit towards -wi   [6] the hit's distance along wi   [7] 0
 * VSPG_EINVAL: light_index outside the light list, or an infinite or delta light (they have no shape to hit). */
#define VSPG_LIGHT_PDF_OUT 8
int vspg_light_pdf_batch(VspgRenderer *r, int light_index, int n, const float *ctx_p /*3n*/, const float *ctx_perr /*3n or NULL*/,
                         const float *ctx_n /*3n*/, const float *wi /*3n*/, float *out /*8n*/, void *stream);

/* Replaces the image of texture `texture_index` (0 .. n_textures - 1 of the scene the renderer was created with) on a live renderer,
 * modelled on vspg_renderer_set_light_image.  host_pixels: xres * yres * channels floats (HOST array), top row first; the resolution and
 * the channel count may differ from the old image's; wrap, filter, invert, scale and the mapping stay.  The host builds the device image
 * (one float4 per texel: R, G, B -- or the grey value three times -- and a pad of 0), uploads it into an allocation of its own and swaps
 * it in behind `stream`; the old image is released after the swap.  It finishes parked samples and suspended paths on `stream` first,
 * synchronises `stream` before it returns, and keeps what vspg_renderer_set_environment_image keeps: film, VSP buffer, guiding fields
 * and training state, counters and the error log persist.  Afterwards the renderer computes what one created with that image
 * computes, bit for bit.
 * VSPG_EINVAL, with the renderer exactly as it was and before any allocation: a null argument, an index that names no texture, a
 * resolution outside 1 .. VSPG_TEXTURE_MAX_RES, channels other than 1 or 3, a texel that is NaN or infinite.  VSPG_ESCOPE, likewise: a
 * resolution that is not a power of two. */
int vspg_renderer_set_texture_image(VspgRenderer *r, int texture_index, const float *host_pixels, int xres, int yres, int channels,
                                    void *stream);
/* Batch driver of the texture lookup (parity tests): per element the reflectance a path vertex on primitive prim[i] with the three
 * floats hit[3i..] gets -- tex_uv_quad / tex_uv_tri and texture_lookup (csrc/vspg_texture.h), the functions the path kernels call.
 * HOST arrays.
 *   prim   n int32: a rectangle's index (>= 0), or -2 - j for triangle j of the caller's soup
 *   hit    3n floats: what a vertex carries -- the point on a rectangle, the barycentrics (b0, b1, b2) of a triangle hit
 *   out    VSPG_TEXTURE_EVAL_OUT floats per element:
 *   [0..1] (u, v)   [2..3] (s, t) after the flip   [4..6] R   [7] has_lobes (1 or 0)
 *   An untextured primitive reports its (u, v), (s, t) = 0, its clamped Kd and whether that has a non-zero component.
 * VSPG_EINVAL: a null argument, a prim that names no rectangle or triangle of the scene (a sphere, a degenerate triangle the build
 * dropped). */
#define VSPG_TEXTURE_EVAL_OUT 8
int vspg_texture_eval_batch(VspgRenderer *r, int n, const int32_t *prim /*n*/, const float *hit /*3n*/, float *out /*8n*/, void *stream);

/* ---- Camera models: thin-lens perspective, orthographic, spherical (csrc/vspg_camera.h) -----------------------------------------
 * GenerateRay of PerspectiveCamera, OrthographicCamera and SphericalCamera (src/pbrt/cameras.cpp:410-433, :290-312, :616-636).
 * VspgScene keeps its size and VSPG_ABI_VERSION stays 7: a renderer is created with the pinhole perspective its VspgCamera describes,
 * and the model is set on the live renderer.  A VspgCamera serves every model: the frame and origin place the camera; sx, ox, sy, oy
 * map a raster point to the screen window (perspective: at camera depth 1; orthographic: in camera-space units on the plane z = 0;
 * spherical: not read).  Out of scope: RealisticCamera, motion blur (the time sample is drawn and unused), ray differentials, We /
 * SampleWi / PDF_We, projective transforms, a second camera per renderer. */
enum { VSPG_CAMERA_PERSPECTIVE = 0, VSPG_CAMERA_ORTHOGRAPHIC = 1,
       VSPG_CAMERA_SPHERICAL_EQUALAREA = 2, VSPG_CAMERA_SPHERICAL_EQUIRECT = 3 };
typedef struct VspgCameraModel { int32_t model; float lens_radius; float focal_distance; } VspgCameraModel;  /* zeroed = today's pinhole */
/* Replaces the camera of a live renderer; model NULL = the pinhole perspective.  It belongs to the calls that finish parked samples
 * and suspended paths first (vspg_flush's list above) -- they end under the camera they started with --, then synchronises `stream`
 * and copies the camera into the scene record.  It CLEARS NOTHING: the film, the image-space statistics, the VSP buffer, TrBuffer,
 * guiding fields, counters and the error log keep their contents, which were gathered under the old camera; vspg_film_clear and its
 * peers are the caller's business.  A model other than the pinhole perspective is served by the full-scene kernels
 * (vspg_renderer_kernel_name tells); perspective with lens_radius == 0 is exactly the pinhole: the same kernel, the same film bits as
 * without the call.  A spherical model ignores both lens fields, as the reference does.
 * VSPG_EINVAL, with the renderer exactly as it was: a null renderer or camera; an unknown model; a non-finite frame, origin or
 * affine term; lens_radius negative or non-finite; focal_distance not finite and positive while lens_radius > 0 (perspective and
 * orthographic). */
int vspg_renderer_set_camera(VspgRenderer *r, const VspgCamera *cam, const VspgCameraModel *model /* NULL = pinhole perspective */, void *stream);
/* vspg_camera_look_at with the model's screen window (cameras.cpp:375-404, :474-503).  Host only.  The default window is
 * [-a, a] x [-1, 1] for a = frame_aspect > 1, else [-1, 1] x [-1/a, 1/a]; frame_aspect 0 = xres / yres ("frameaspectratio");
 * screen_window {xmin, xmax, ymin, ymax} overrides it ("screenwindow").  Perspective scales the window by tan(fov / 2); orthographic
 * takes it as it is (fov_degrees is not read); spherical fills the frame and origin only (sx = ox = sy = oy = 0).  Raster y points
 * down.  With a NULL window, frame_aspect 0 and the perspective model the result equals vspg_camera_look_at's bit for bit.
 * VSPG_EINVAL: vspg_camera_look_at's refusals, an unknown model, a frame_aspect that is negative or not finite, a window with a
 * non-finite value. */
int vspg_camera_look_at_window(VspgCamera *cam, int model, const float eye[3], const float look[3], const float up[3],
                               float fov_degrees, const float screen_window[4] /* or NULL */, float frame_aspect /* 0 = xres/yres */, int xres, int yres);
/* Batch driver of the camera ray (parity tests): the render-space ray start_path gives sample sample_index[i] of pixel
 * pixel_xy[2i..] under the renderer's camera -- camera_generate_ray (csrc/vspg_camera.h), the function the full-scene kernels call.
 * u: per element the filter's and the lens's two variates (4n floats), or NULL: the renderer's own sampler draws them in its order
 * (wavelength, filter 2, time, lens 2).  out_o, out_d: 3n floats each.  HOST arrays.
 * VSPG_EINVAL: a null argument, a pixel outside the frame, a negative sample index. */
int vspg_camera_ray_batch(VspgRenderer *r, int n, const int32_t *pixel_xy, const int32_t *sample_index,
                          const float *u /* 4n: filter u0 u1, lens u0 u1; NULL = the renderer's sampler */, float *out_o, float *out_d, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VSPG_H */
