// vspg_wg3_exact.hip -- the exact-arithmetic instantiations of k_render_wave_wg3 for rectangle scenes without guiding (the headline
// workload and its three siblings), in a translation unit of their own so that csrc/Makefile can give them flags of their own.
//
// -mllvm -amdgpu-atomic-optimizer-strategy=None (Makefile): the kernel's scheduler issues its queue and counter atomics from lane 0
// only (`if (lane == 0) atomicAdd(...)`, vspg_wg3.h).  The atomic optimizer does not know that and wraps each one in a wave
// reduction (mbcnt of exec, compare, exec swap, popcount, readlane), which one lane never needs; the atomics it could merge -- many
// lanes, one address -- do not occur in this kernel.  Off here: 88 fewer vector and 175 fewer scalar instructions in the
// headline instantiation, same atomics, same values.
#include <hip/hip_runtime.h>

#include "vspg_wg3.h"

VSPG_NS_BEGIN
int wg3_launch_exact(const Wg3Launch &L) { return wg3_launch_unguided(L); }
VSPG_NS_END  // namespace vspg

#ifdef VSPG_W3_TIMELINE
// diagnostic build only: the last launch's per-wavefront records (vspg_wg3.h), read and cleared
extern "C" int vspg_w3_timeline_read(unsigned long long *out, int blocks) {
    using namespace vspg;
    if (blocks < 0 || blocks > (int)W3T_MAX_BLOCKS) return -1;
    const size_t bytes = (size_t)blocks * 8 * 32 * sizeof(unsigned long long);
    if (hipDeviceSynchronize() != hipSuccess) return -2;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_w3_timeline), bytes) != hipSuccess) return -3;
    void *p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_w3_timeline)) != hipSuccess || hipMemset(p, 0, sizeof(g_w3_timeline)) != hipSuccess) return -4;
    return 0;
}
#endif
