// Test shim: the project's own tanf / atan2f (csrc/vspg_trig.h, the header the kernels and the host builder use) for the CPU sweep of
// tests/test_portallight_model.py against float64.
#include <math.h>
#include <stdint.h>

#include "../vspg-pbrt-v4_amd/csrc/vspg_trig.h"

extern "C" {
void portal_tanf(int n, const float *x, float *y) { for (int i = 0; i < n; ++i) y[i] = vspg_libm::portal_tanf(x[i]); }
void portal_atanf(int n, const float *x, float *y) { for (int i = 0; i < n; ++i) y[i] = vspg_libm::portal_atanf(x[i]); }
void portal_atan2f(int n, const float *y, const float *x, float *o) { for (int i = 0; i < n; ++i) o[i] = vspg_libm::portal_atan2f(y[i], x[i]); }
}
