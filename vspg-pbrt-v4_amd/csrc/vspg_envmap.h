// vspg_envmap.h -- the pieces of the image infinite light (vspg_envlight.h) that the host builders evaluate too, host and device:
// the rotation, EqualAreaSphereToSquare and the octahedral pixel remap.  The portal light's rectified image is resampled from the
// equal-area image through them on the host (portal_build_tables, vspg_scene_build.hip).
#pragma once
#include "vspg_device.h"

VSPG_NS_BEGIN

// __host__ twins of the vector helpers of vspg_device.h that the shared (VHD) code below and in vspg_portalmap.h calls: the originals
// stay __device__ functions, spelled as they are, and overload resolution picks by the side being compiled.  The same expressions in
// the same order; the host units are built with the kernels' flags (-ffp-contract=off), so the same floats.
#define VHOST __host__ inline
VHOST V3 ld3(const float *p) { return V3{p[0], p[1], p[2]}; }
VHOST V3 operator+(V3 a, V3 b) { return V3{a.x + b.x, a.y + b.y, a.z + b.z}; }
VHOST V3 operator-(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
VHOST V3 operator*(V3 a, float s) { return V3{a.x * s, a.y * s, a.z * s}; }
VHOST V3 operator*(float s, V3 a) { return V3{a.x * s, a.y * s, a.z * s}; }
VHOST float sqr(float x) { return x * x; }
VHOST float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
VHOST float len2(V3 a) { return sqr(a.x) + sqr(a.y) + sqr(a.z); }
VHOST float len(V3 a) { return __builtin_sqrtf(len2(a)); }
VHOST V3 normalize(V3 a) {
    float l = len(a);
    return V3{a.x / l, a.y / l, a.z / l};
}
VHOST float diff_of_products(float a, float b, float c, float d) {
    float cd = c * d;
    float dop = __builtin_fmaf(a, b, -cd);
    float err = __builtin_fmaf(-c, d, cd);
    return dop + err;
}
VHOST V3 cross(V3 v, V3 w) {
    return V3{diff_of_products(v.y, w.z, v.z, w.y), diff_of_products(v.z, w.x, v.x, w.z), diff_of_products(v.x, w.y, v.y, w.x)};
}
VHOST float fmax_(float a, float b) { return a < b ? b : a; }
VHOST float fmin_(float a, float b) { return b < a ? b : a; }
VHOST float safe_sqrt(float x) { return __builtin_sqrtf(fmax_(0.f, x)); }
VHOST float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }
#undef VHOST

// Transform::operator()(Vector3f) / ApplyInverse(Vector3f) (util/transform.h:206-211, 412-420): rows of m / mInv, no translation
VHD V3 env_xform(const float *m, V3 v) {
    return V3{m[0] * v.x + m[1] * v.y + m[2] * v.z, m[3] * v.x + m[4] * v.y + m[5] * v.z, m[6] * v.x + m[7] * v.y + m[8] * v.z};
}

// EqualAreaSphereToSquare (util/math.cpp:317-361)
VHD void env_sphere_to_square(V3 d, float *pu, float *pv) {
    const float x = __builtin_fabsf(d.x), y = __builtin_fabsf(d.y), z = __builtin_fabsf(d.z);
    const float r = safe_sqrt(1 - z);
    const float a = fmax_(x, y);
    float b = fmin_(x, y);
    b = a == 0 ? 0 : b / a;
    // EvaluatePolynomial(b, t1..t7) (util/math.h:330-337): Horner by FMA, innermost coefficient first
    const float t1 = 0.406758566246788489601959989e-5f, t2 = 0.636226545274016134946890922156f, t3 = 0.61572017898280213493197203466e-2f,
                t4 = -0.247333733281268944196501420480f, t5 = 0.881770664775316294736387951347e-1f, t6 = 0.419038818029165735901852432784e-1f,
                t7 = -0.251390972343483509333252996350e-1f;
    float phi = __builtin_fmaf(b, t7, t6);
    phi = __builtin_fmaf(b, phi, t5);
    phi = __builtin_fmaf(b, phi, t4);
    phi = __builtin_fmaf(b, phi, t3);
    phi = __builtin_fmaf(b, phi, t2);
    phi = __builtin_fmaf(b, phi, t1);
    if (x < y) phi = 1 - phi;
    float v = phi * r;
    float u = r - v;
    if (d.z < 0) {  // southern hemisphere -> mirror u, v
        const float t = u;
        u = v;
        v = t;
        u = 1 - u;
        v = 1 - v;
    }
    u = __builtin_copysignf(u, d.x);
    v = __builtin_copysignf(v, d.y);
    *pu = 0.5f * (u + 1);
    *pv = 0.5f * (v + 1);
}

// RemapPixelCoords under WrapMode::OctahedralSphere (util/image.h:100-125) for a square image; shared with the portal light's host
// builder, whose bilinear resampling reads the equal-area image through it (vspg_scene_build.hip)
VHD void env_remap_octahedral(int *ppx, int *ppy, int res) {
    int px = *ppx, py = *ppy;
    if (px < 0) {
        px = -px;
        py = res - 1 - py;
    } else if (px >= res) {
        px = 2 * res - 1 - px;
        py = res - 1 - py;
    }
    if (py < 0) {
        px = res - 1 - px;
        py = -py;
    } else if (py >= res) {
        px = res - 1 - px;
        py = 2 * res - 1 - py;
    }
    if (res == 1) px = py = 0;  // "things don't go as expected for 1x1 images"
    *ppx = px;
    *ppy = py;
}

VSPG_NS_END
