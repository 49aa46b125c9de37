// vspg_rgbgrid.h -- RGBGridMedium ("rgbgrid", src/pbrt/media.h:391-467, media.cpp:369-484) in the RGB rendering build: sigma_a, sigma_s
// and Le are grids of RGB, RGBUnboundedSpectrum / RGBIlluminantSpectrum::Sample(lambda) returns the RGB and MaxValue() its largest
// component (util/spectrum.h:661-803).  Included by the units that instantiate kernels over it (vspg_wf_rgbgrid.hip, vspg_capi.hip).
//
// Device storage ("RGB octets"): per sigma grid and per base voxel (ix, iy, iz) in [-1, n - 1]^3 the eight RGB corner values of the
// trilinear filter, each padded to a float4, in the corner order of GridMediumT::Octet -- 8 x 16 = 128 bytes, 128-byte aligned: ONE
// cache line per grid per query, two per sample_point (a random query costs a 128-byte line of HBM traffic whatever it
// asks of the line).  Voxels outside the grid are stored as 0 (the bounds test of SampledGrid::Lookup(Point3i) baked in).  The octets
// of a grid are laid out in the 8 x 8 x 8 bricks of the scalar grids (DScene::octets), every brick stored (dense).  128 bytes per base
// voxel and grid: 32 / 3 times the caller's 12-byte RGB voxel.  An absent grid is not stored: the pointer is null and the constant 1
// is branched in wave-uniformly.  The Le grid is read by the delta-tracking callback only ("nds") and stays the caller's raw array.
#pragma once
#include "vspg_device.h"

VSPG_NS_BEGIN

// the slot of base voxel (ix, iy, iz)'s octet, in octets (of 8 float4): host builder and kernels share it
__host__ __device__ __forceinline__ size_t rgb_octet_slot(int ox, int oy, int oz, int bnx, int bny) {  // o = i + 1 in [0, n]
    const size_t brick = ((size_t)(oz >> 3) * (size_t)bny + (size_t)(oy >> 3)) * (size_t)bnx + (size_t)(ox >> 3);
    return brick * 512u + (size_t)((ox & 7) + 8 * ((oy & 7) + 8 * (oz & 7)));
}

// BND, MAJLDS: GridMediumT's.  The ray transform, the bounds test and the DDA set-up are GridMediumT's own code (`base`), run with
// sigma_t = 1: the majorant grid holds sigmaScale * (max sigma_a + max sigma_s) itself, one scalar for the three channels.
template <int BND = -1, bool MAJLDS = false>
struct RgbGridMediumT {
    using Base = GridMediumT<false, false, BND, false, MAJLDS>;
    using Iter = typename Base::Iter;
    static constexpr bool kMajLds = MAJLDS;
    static constexpr int kBnd = BND;
    static constexpr bool kEmit = false;  // (blackbody emission: an RGB grid medium has no temperature grid; its Le grid needs no wavelengths)
    static constexpr int kRes = kMajRes;
    static constexpr int kAdvanceRounds = Base::kAdvanceRounds;
    static constexpr int kGrey = 0;
    static constexpr bool kSimpleScene = false;
    static constexpr bool kSingleSegment = false;
    static constexpr bool kAlwaysRealCollision = false;
    static constexpr bool kNullZero = false;
    Base base;  // sigma_a = 1, sigma_s = 0 (sigma_t = 1 + 0), the grid's size, bounds, transform and majorants; no density storage
    float g;
    const float4 *oct_a, *oct_s;  // null = absent (wave-uniform)
    const float *Le;              // raw RGB voxels, null = not emissive
    float sigma_scale, le_scale;

    struct Lattice {  // SampledGrid::Lookup(Point3f, convert) (containers.h:784-790): voxel coordinates and offsets
        int ix, iy, iz;
        float dx, dy, dz;
    };
    VDEV Lattice lattice(V3 p) const {
        const float sx = p.x * base.nx - .5f, sy = p.y * base.ny - .5f, sz = p.z * base.nz - .5f;
        const float fx = __builtin_floorf(sx), fy = __builtin_floorf(sy), fz = __builtin_floorf(sz);
        Lattice l;
        l.ix = (int)fx; l.iy = (int)fy; l.iz = (int)fz;
        l.dx = sx - (float)l.ix; l.dy = sy - (float)l.iy; l.dz = sz - (float)l.iz;
        return l;
    }
    // Lerp(d.z, Lerp(d.y, d00, d10), Lerp(d.y, d01, d11)) of one channel (containers.h:792-800), Lerp(t, a, b) = (1 - t) a + t b
    static VDEV float tri(const Lattice &l, float v000, float v100, float v010, float v110, float v001, float v101, float v011, float v111) {
        const float d00 = (1 - l.dx) * v000 + l.dx * v100;
        const float d10 = (1 - l.dx) * v010 + l.dx * v110;
        const float d01 = (1 - l.dx) * v001 + l.dx * v101;
        const float d11 = (1 - l.dx) * v011 + l.dx * v111;
        const float a = (1 - l.dy) * d00 + l.dy * d10, b = (1 - l.dy) * d01 + l.dy * d11;
        return (1 - l.dz) * a + l.dz * b;
    }
    // one sigma grid at the lattice position: its octet is one aligned 128-byte line, fetched as eight 16-byte loads through a
    // global-address-space pointer (GridMediumT::octet); a base voxel outside [-1, n - 1]^3 has all-zero corners and no fetch
    VDEV Spec lookup_octet(const float4 *oct, const Lattice &l) const {
        const int ox = l.ix + 1, oy = l.iy + 1, oz = l.iz + 1;
        if (!((unsigned)ox <= (unsigned)base.nx && (unsigned)oy <= (unsigned)base.ny && (unsigned)oz <= (unsigned)base.nz)) return sp(0.f);
        typedef float v4f_ __attribute__((ext_vector_type(4)));
        const v4f_ VSPG_GLOBAL_AS *q = (const v4f_ VSPG_GLOBAL_AS *)(oct + rgb_octet_slot(ox, oy, oz, base.bnx, base.bny) * 8u);
        const v4f_ c0 = q[0], c1 = q[1], c2 = q[2], c3 = q[3], c4 = q[4], c5 = q[5], c6 = q[6], c7 = q[7];
        return Spec{tri(l, c0.x, c1.x, c2.x, c3.x, c4.x, c5.x, c6.x, c7.x), tri(l, c0.y, c1.y, c2.y, c3.y, c4.y, c5.y, c6.y, c7.y),
                    tri(l, c0.z, c1.z, c2.z, c3.z, c4.z, c5.z, c6.z, c7.z)};
    }
    // the Le grid: raw voxels, SampledGrid::Lookup(Point3i, convert) (containers.h:821-827) per corner
    VDEV Spec lookup_raw(const float *data, const Lattice &l) const {
        const int nx = base.nx, ny = base.ny, nz = base.nz;
        auto at = [&](int x, int y, int z) {
            if (x < 0 || y < 0 || z < 0 || x >= nx || y >= ny || z >= nz) return sp(0.f);
            const float VSPG_GLOBAL_AS *v = (const float VSPG_GLOBAL_AS *)(data + (((size_t)z * ny + y) * nx + x) * 3u);
            return Spec{v[0], v[1], v[2]};
        };
        const Spec v000 = at(l.ix, l.iy, l.iz), v100 = at(l.ix + 1, l.iy, l.iz), v010 = at(l.ix, l.iy + 1, l.iz), v110 = at(l.ix + 1, l.iy + 1, l.iz);
        const Spec v001 = at(l.ix, l.iy, l.iz + 1), v101 = at(l.ix + 1, l.iy, l.iz + 1), v011 = at(l.ix, l.iy + 1, l.iz + 1), v111 = at(l.ix + 1, l.iy + 1, l.iz + 1);
        return Spec{tri(l, v000.r, v100.r, v010.r, v110.r, v001.r, v101.r, v011.r, v111.r), tri(l, v000.g, v100.g, v010.g, v110.g, v001.g, v101.g, v011.g, v111.g),
                    tri(l, v000.b, v100.b, v010.b, v110.b, v001.b, v101.b, v011.b, v111.b)};
    }

    VDEV V3 to_medium(V3 p) const { return base.to_medium(p); }
    VDEV V3 offset(V3 p) const { return base.offset(p); }
    VDEV Iter empty_iter() const { return base.empty_iter(); }
    VDEV Iter sample_ray(V3 o, V3 d, float raytMax) const { return base.sample_ray(o, d, raytMax); }  // media.h:444-455
    VDEV MediumProps sample_point(V3 p) const {  // media.h:417-441
        p = base.to_medium(p);
        const Lattice l = lattice(base.offset(p));
        // one grid interpolated before the other is fetched into: the 24 corner floats of a grid are dead once its Spec is formed
        Spec sa = sp(1.f), ss = sp(1.f);
        if (oct_a) sa = lookup_octet(oct_a, l);
        sa = sa * sigma_scale;
        if (oct_s) ss = lookup_octet(oct_s, l);
        ss = ss * sigma_scale;
        Spec le = sp(0.f);
        if (Le && le_scale > 0) le = lookup_raw(Le, l) * le_scale;  // IsEmissive (media.h:411): wave-uniform
        return MediumProps{sa, ss, le, g, ss + sa, 0.f, 0.f};
    }
    VDEV Spec sigma_n(const MediumProps &mp, Spec sigma_maj) const { return clamp_zero(sigma_maj - mp.sigma_a - mp.sigma_s); }
    VDEV bool is_homogeneous() const { return false; }
};
using RgbGridMedium = RgbGridMediumT<>;

template <int BND, bool MAJLDS> struct MediumMaker<RgbGridMediumT<BND, MAJLDS>> {
    static VDEV RgbGridMediumT<BND, MAJLDS> make(const DScene &S, const float *majorant) {
        using M = RgbGridMediumT<BND, MAJLDS>;
        typename M::Base b{sp(1.f), sp(0.f), S.g, S.nx, S.ny, S.nz, ld3(S.bounds_min), ld3(S.bounds_max), nullptr, nullptr, S.bnx, S.bny,
                           majorant ? majorant : S.majorant, 0, 0, 0, V3{0.f, 0.f, 0.f}, V3{0.f, 0.f, 0.f}, 0.f, nullptr, 0, 0, 0, sp(0.f),
                           S.has_xform ? S.minv : nullptr, nullptr, 0.f, 0.f, 0.f};
        return M{b, S.g, S.rgb_oct_a, S.rgb_oct_s, S.rgb_Le, S.rgb_sigma_scale, S.rgb_le_scale};
    }
};

VSPG_NS_END  // namespace vspg
