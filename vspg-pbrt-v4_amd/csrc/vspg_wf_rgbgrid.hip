// vspg_wf_rgbgrid.hip -- the kernels over RGBGridMedium ("rgbgrid", vspg_rgbgrid.h) that are not text of vspg_capi.hip: the wavefront
// pipeline's instantiations (vspg_wf_launch.h) and the path replay (vspg_trace.h), in a unit of their own so that `make -j` compiles
// them beside the others.
#include "vspg_wf_launch.h"
#include "vspg_rgbgrid.h"
#include "vspg_trace.h"
VSPG_NS_BEGIN
// {unguided, guided, guided + training} x {no boundaries, boundaries}; under "nds" the same media run k_wf_segment_vertex (the Le grid's
// branch is wave-uniform and part of every instantiation, as GridMediumT's LeScale grid is).  No grey layout: the medium is chromatic
// by construction.  The majorant grid is 16^3 and read from the block's LDS copy, as GridMedium's.
int wf_dispatch_rgbgrid(const WfLaunch &L, bool guided, bool train) {
#define VSPG_WF_RGB_CASE(BNDV)                                                       \
    do {                                                                             \
        using M = RgbGridMediumT<BNDV, VSPG_WF_MAJ_LDS != 0>;                        \
        using WM = RgbGridMediumT<-1, VSPG_WF_MAJ_LDS != 0>;                         \
        if (guided && train) return wf_run_pass<M, true, true, WM>(L);               \
        if (guided) return wf_run_pass<M, true, false, WM>(L);                       \
        return wf_run_pass<M, false, false, WM>(L);                                  \
    } while (0)
    if (L.bnd) VSPG_WF_RGB_CASE(1);
    VSPG_WF_RGB_CASE(0);
#undef VSPG_WF_RGB_CASE
}

int trace_launch_rgbgrid(const TraceLaunch &T, bool guided) {
    const dim3 grid((unsigned)((T.n + kTraceBlock - 1) / kTraceBlock)), block(kTraceBlock);
    if (guided) hipLaunchKernelGGL((k_trace_paths<RgbGridMedium, true>), grid, block, 0, T.stream, T.dscene, T.vsp, T.vsp_ready, T.n, T.pixel_xy, T.sample_index, T.out_L, T.out_seg);
    else hipLaunchKernelGGL((k_trace_paths<RgbGridMedium, false>), grid, block, 0, T.stream, T.dscene, T.vsp, T.vsp_ready, T.n, T.pixel_xy, T.sample_index, T.out_L, T.out_seg);
    return (int)hipGetLastError();
}
VSPG_NS_END  // namespace vspg
