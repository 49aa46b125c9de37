// vspg_trig.h -- the project's own tanf and atan2f for the portal light's gnomonic-angle map (vspg_portallight.h).
//
// Why own functions: the reference calls std::tan and std::atan2 of its platform's libm there, so its own texel choice within a few
// ulp of a texel edge depends on the platform.  The device library's versions cannot be restated on the host and vspg_libm.h holds no
// host-exact text of glibc's, so one definition serves the host builder, the kernels and the NumPy mirror (tests/portallight_model.py)
// operation for operation: plain float operations and explicit fmaf, no contraction (-ffp-contract=off).  DESIGN.md 4.13 derives
// the error bounds and records the sweep that measured them (tests/portallight_shim.cpp).
//
//   portal_tanf(a)       sin(a) / cos(a) of sincosf_host_exact's pair: two correctly-scaled floats (each within 1 ulp) and one
//                        division.  cos of a float is never 0 (no float is an odd multiple of pi / 2), so the quotient is finite for
//                        every |a| < 120 -- also at a = +-(float)(pi / 2), where the true tangent is ~ -+2.3e7.
//   portal_atan2f(y, x)  atan(y / x) for x > 0 (the only case ImageFromRender meets: w.z > 0).  Cephes' atanf scheme: |t| > tan(3 pi / 8)
//                        -> pi / 2 - atan(1 / |t|); |t| > tan(pi / 8) -> pi / 4 + atan((|t| - 1) / (|t| + 1)); then the odd polynomial
//                        z + z^3 P(z^2) on |z| <= tan(pi / 8).  t = +-inf (x underflowed) gives +-pi / 2; a NaN passes through.
#pragma once
#include "vspg_libm.h"

namespace vspg_libm {

VSPG_HD float portal_tanf(float a) {
    float s, c;
    sincosf_host_exact(a, &s, &c);
    return s / c;
}

VSPG_HD float portal_atanf(float t) {
    const float a = __builtin_fabsf(t);
    float y0, z;
    if (a > 2.414213562373095f) {  // tan(3 pi / 8)
        y0 = 1.57079632679489661923f;
        z = -1.f / a;
    } else if (a > 0.4142135623730950f) {  // tan(pi / 8)
        y0 = 0.78539816339744830961f;
        z = (a - 1.f) / (a + 1.f);
    } else {
        y0 = 0.f;
        z = a;
    }
    const float w = z * z;
    float p = __builtin_fmaf(w, 8.05374449538e-2f, -1.38776856032e-1f);
    p = __builtin_fmaf(w, p, 1.99777106478e-1f);
    p = __builtin_fmaf(w, p, -3.33329491539e-1f);
    const float r = y0 + __builtin_fmaf(p * w, z, z);
    return __builtin_copysignf(r, t);
}
VSPG_HD float portal_atan2f(float y, float x) { return portal_atanf(y / x); }

}  // namespace vspg_libm
