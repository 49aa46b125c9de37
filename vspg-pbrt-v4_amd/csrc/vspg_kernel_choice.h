// vspg_kernel_choice.h -- which path kernel serves a renderer: one pure function of a dozen scene facts and four environment variables
// (choose_kernel) and the name of what it chose (kernel_name).  Plain C++17, no HIP and no renderer: vspg_capi.hip fills the facts in
// (choice_facts) and launches what the record says; tests/kernel_choice_table.cpp walks the table on a CPU.
#pragma once
#include <cstdlib>
#include <string>

#include "../../include/vspg.h"

namespace vspg_choice {

struct ChoiceFacts {  // what the decision reads of a renderer
    int medium_type = VSPG_MEDIUM_NONE;
    int n_tris = 0, n_inf = 0, n_spheres = 0;
    int n_point = 0;  // point and spot lights
    int n_textured = 0;  // surfaces whose reflectance is an image texture (vspg_texture.h)
    bool has_boundaries = false;
    int lightsampler = VSPG_LIGHTSAMPLER_UNIFORM;
    bool medium_grey = false, surfaces_grey = false, null_zero = false;  // bitwise grey sigma_a / sigma_s / Le; grey Kd; sigma_n == 0
    bool guided = false, rrguiding = false, training = false;            // guided: wants_guiding(prm)
    bool tr_calc = false, has_temperature = false;
    bool resampling = true;  // vspsamplingmethod == VSPG_VSP_RESAMPLING (else NDS / NDS+)
    bool camera_general = false;  // the camera is not the pinhole perspective: another model, or lens_radius > 0 (vspg_camera.h)
};
struct ChoiceEnv {  // ... and of the process environment
    std::string kernel;           // VSPG_KERNEL=wg|lane|wf picks a path kernel where several serve a configuration (tests, A/B runs); empty == unset
    char wg_sched = 0;            // VSPG_WG_SCHED's first character: '1' = k_render_wave_wg, '2' = k_render_wave_wg2 (tests compare the three schedulers)
    bool wg_sched_set = false;    // ... and whether it is set at all, to an empty value included
    bool no_grey_guided = false;  // VSPG_NO_GREY_GUIDED is set
    char wf_merged = 0;           // VSPG_WF_MERGED's first character where that is '0' or '1', else 0
};
inline ChoiceEnv read_choice_env() {  // (at every entry-point call, never cached: tests flip these between calls)
    ChoiceEnv e;
    if (const char *v = std::getenv("VSPG_KERNEL")) e.kernel = v;
    if (const char *v = std::getenv("VSPG_WG_SCHED")) e.wg_sched_set = true, e.wg_sched = v[0];
    e.no_grey_guided = std::getenv("VSPG_NO_GREY_GUIDED") != nullptr;
    if (const char *v = std::getenv("VSPG_WF_MERGED")) e.wf_merged = v[0] == '0' || v[0] == '1' ? v[0] : 0;
    return e;
}

// Lane: k_render_wave, the per-lane persistent kernel.  Wg / Wg2 / Wg3: the workgroup kernel's schedulers k_render_wave_wg (film flush
// between the phases, three barriers), k_render_wave_wg2 (tiles from a global head, samples parked and resolved by the next launch,
// two barriers) and k_render_wave_wg3 (vspg_wg3.h: ring queues in LDS, every wavefront its own scheduler).  WfWalk / WfSegmentVertex:
// the multi-kernel wavefront pipeline (vspg_wavefront.h) of the resampling routine / of NDS and NDS+.
enum class Family { Lane, Wg, Wg2, Wg3, WfWalk, WfSegmentVertex };
// The medium type a kernel is instantiated with.  Homogeneous: HomogeneousMedium, the full-scene code paths; HomogeneousSimple =
// HomogeneousMediumT<0,false>: rectangle scenes with area lights only; HomogeneousGrey = <1,false>: sigma_a, sigma_s, Le bitwise grey, the
// broadcast-spectrum instantiation; HomogeneousGreyScene = <2,false>: ... and every Kd bitwise grey, beta is grey by construction too;
// HomogeneousGreySceneNullZero = <2,true>: ... and the null-collision coefficient is exactly 0.  NanoDenseGrey: the pipeline only.
// RgbGrid: RgbGridMediumT (vspg_rgbgrid.h), the pipeline and the per-lane kernel; it has no grey layout, no workgroup kernel and no
// tolerance-mode instantiation.
enum class MediumInst { Homogeneous, HomogeneousSimple, HomogeneousGrey, HomogeneousGreyScene, HomogeneousGreySceneNullZero, Grid, GridGrey, NanoDense, NanoDenseGrey, RgbGrid };

struct KernelChoice {
    Family family = Family::Lane;
    MediumInst medium = MediumInst::Homogeneous;
    bool guided = false, train = false;  // the kernel's GUIDED / TRAIN parameters
    bool wg_guided = false;              // the workgroup kernel's guided launch shape (vspg_guided_wg.h)
    bool wg_full = false;                // ... its full-scene instantiation
    bool wf_merged = false;              // the pipeline runs both walks of an iteration as one kernel (k_wf_walk)
    // vspg_fast.hip holds this kernel in the tolerance modes too (vspg_arith.h): the unguided rectangle-scene k_render_wave_wg3 and the
    // unguided resampling pipeline over GridMedium
    bool arith_covered = false;
};

// The only place that decides.
inline KernelChoice choose_kernel(const ChoiceFacts &f, const ChoiceEnv &env) {
    const bool hom = f.medium_type == VSPG_MEDIUM_HOMOGENEOUS, grid = f.medium_type == VSPG_MEDIUM_GRID, nvdb = f.medium_type == VSPG_MEDIUM_NANOVDB;
    const bool rgbgrid = f.medium_type == VSPG_MEDIUM_RGBGRID;
    const bool k_unset = env.kernel.empty(), k_wg = env.kernel == "wg", k_wf = env.kernel == "wf";
    // a scene of rectangles and area lights only, one medium filling it: what the workgroup kernel's specialised instantiations are built for
    // (HomogeneousMediumT::kSimpleScene).  Triangle hits carry a per-hit error bound the LDS pool record has no room for; medium boundaries,
    // interface materials and spheres are served by the full-scene code paths; so are power / BVH picks of a multi-light scene, and
    // point and spot lights (sample_light<FULL> alone dispatches on them), and textured surfaces (vertex_setup<FULL> alone looks a texel up),
    // and every camera but the pinhole perspective (start_path_common<true> alone generates their rays).
    const bool simple = f.n_tris == 0 && f.n_inf == 0 && f.n_point == 0 && f.lightsampler == VSPG_LIGHTSAMPLER_UNIFORM && !f.has_boundaries && f.n_spheres == 0 &&
                        f.n_textured == 0 && !f.camera_general;
    // guided renders over a homogeneous medium: the grey / zero-null-coefficient / rectangle-scene instantiation (the segment half of the
    // loop sheds the same per-channel work as the headline kernel's instantiation)
    const bool guided_grey_simple = hom && f.medium_grey && f.surfaces_grey && f.null_zero && simple && !env.no_grey_guided;
    const bool cross_check = !k_unset || env.wg_sched_set;  // (the cross-check kernels exist in exact arithmetic only)
    KernelChoice c;
    c.guided = f.guided;
    c.train = f.guided && f.training;  // a18: while the field trains, the guided kernels record path segments and emit radiance samples

    // "wf" = the wavefront pipeline: heterogeneous media.  Default for those; VSPG_KERNEL=lane|wg selects the single-kernel schedulers
    // instead (kept as cross-checks).  Guided builds too, training passes included (segment recording in the dense kernels), guided
    // Russian roulette (round 3: the vertex kernel reads the pixel's contribution estimate) and, in its own shape, NDS / NDS+.
    if ((grid || nvdb || rgbgrid) && (k_unset || k_wf)) {
        c.family = f.resampling ? Family::WfWalk : Family::WfSegmentVertex;
        const bool grey = !f.guided && f.medium_grey;
        c.medium = rgbgrid ? MediumInst::RgbGrid : nvdb ? (grey ? MediumInst::NanoDenseGrey : MediumInst::NanoDense) : (grey ? MediumInst::GridGrey : MediumInst::Grid);
        // both walks of an iteration as ONE kernel where the job lists are short or a third kernel sits in the chain (boundary scenes,
        // guided pipelines); side by side on two streams for dense unguided clouds (k_wf_walk, vspg_wavefront.h: measured both ways).
        // VSPG_WF_MERGED=0|1 overrides.
        c.wf_merged = env.wf_merged ? env.wf_merged == '1' : f.has_boundaries || f.guided;
        c.arith_covered = !cross_check && !f.guided && !f.tr_calc && grid && f.resampling && !f.has_temperature;
        return c;
    }
    // round 3: the workgroup kernel's guided vertex (vspg_guided_wg.h, four waves per SIMD) is the DEFAULT for a trained or loaded field
    // over a homogeneous medium in a rectangle scene; VSPG_KERNEL=lane selects the per-lane kernel (tests compare the two).  Guided Russian
    // roulette (per-pixel state), triangles / infinite lights and non-uniform light samplers stay per-lane.  It was opt-in before: measured on
    // MI355X (1080p fog box, reference-default options) the per-lane kernel ran a guided wave in 2.33 ms, the three-barrier
    // workgroup kernel in 2.58 ms (384-path pool, kd nodes in L2) / 2.93 ms (320-path pool + the upper kd levels in LDS): it issued 18 %
    // fewer vector instructions at 68 % instead of 54 % lane utilisation, but the guided vertex code needs ~240 registers either way (2 waves
    // per SIMD) and at that occupancy the phase barriers cost more than the compaction saves.
    // It stays on k_render_wave_wg2: k_render_wave_wg3 lives on the pool's slack over the workgroup's lanes (HISTORY round 5), which the
    // larger records do not leave -- the guided / training instantiations hold 544 / 448 paths for 512 lanes (reference-default trained wave
    // 1.45 ms against 1.42).
    if ((k_unset || k_wg) && f.guided && !f.rrguiding && hom && simple) {
        c.family = Family::Wg2;
        c.wg_guided = true;
        c.medium = guided_grey_simple ? MediumInst::HomogeneousGreySceneNullZero : MediumInst::HomogeneousSimple;
        return c;
    }
    // Round 4: everything else over a homogeneous medium, unguided -- triangles (BVH), spheres, infinite lights, power / BVH light samplers,
    // medium boundaries -- runs the workgroup kernel's FULL-scene instantiation (k_render_wave_wg2<HomogeneousMedium>; a 512-path pool: no
    // slack for k_render_wave_wg3 either) instead of the per-lane kernel; VSPG_KERNEL=lane keeps the per-lane kernel (tests compare the two).
    if ((k_unset || k_wg) && hom && !f.guided && !simple) {
        c.family = Family::Wg2;
        c.wg_full = true;
        c.medium = MediumInst::Homogeneous;
        return c;
    }
    // scheduler: "wg" = workgroup-level wavefront kernel, "lane" = per-lane persistent kernel.  Default: wg for homogeneous media (dense,
    // equally long phases); lane for grid media, whose tracking walks have very different lengths per path -- a phase lasts as long as its
    // longest walk, while the per-lane kernel refills a lane the moment its path ends (measured on the 256^3 cloud stand-in: 30.5 vs 38.6 ms
    // per wave).  VSPG_KERNEL=wg|lane overrides (unguided builds only).  Not for a grid with a TrBuffer (its running mean needs a pixel's
    // samples in order: the per-lane kernel owns a pixel per launch) or with a temperature grid (blackbody emission needs the path's
    // wavelength sample, which k_render_wave_wg's pool record does not carry).
    if (simple && !f.guided && !nvdb && !rgbgrid && (k_wg || (k_unset && !grid)) && !(grid && (f.has_temperature || f.tr_calc))) {
        // Which scheduler: k_render_wave_wg2 serves every homogeneous configuration since round 3 -- with the shared
        // tile head it beat k_render_wave_wg on the unguided workload too (0.776 against 0.808 ms); VSPG_WG_SCHED=1 selects k_render_wave_wg
        // for the unguided instantiations, grid media (under VSPG_KERNEL=wg only) stay on it.  Round 5: the barrier-free k_render_wave_wg3
        // serves whatever k_render_wave_wg2 served and leaves it the pool's slack (above); VSPG_WG_SCHED=2 keeps k_render_wave_wg2.
        c.family = grid || env.wg_sched == '1' ? Family::Wg : env.wg_sched == '2' ? Family::Wg2 : Family::Wg3;
        c.medium = grid                ? MediumInst::Grid
                   : !f.medium_grey    ? MediumInst::HomogeneousSimple
                   : !f.surfaces_grey  ? MediumInst::HomogeneousGrey
                   : !f.null_zero      ? MediumInst::HomogeneousGreyScene
                                       : MediumInst::HomogeneousGreySceneNullZero;
        c.arith_covered = !cross_check && !f.tr_calc;
        return c;
    }
    // the per-lane kernel: everything else -- an RGB grid medium under VSPG_KERNEL=wg included (no workgroup kernel is built for it: the
    // branch above leaves it out)
    c.medium = rgbgrid                          ? MediumInst::RgbGrid
               : nvdb                           ? MediumInst::NanoDense
               : grid                           ? (!f.guided && f.medium_grey ? MediumInst::GridGrey : MediumInst::Grid)
               : f.guided && guided_grey_simple ? MediumInst::HomogeneousGreySceneNullZero
                                                : MediumInst::Homogeneous;
    return c;
}

// The kernel's name in exact arithmetic, composed from the choice: family, medium, then ",guided" and ",train".
inline std::string kernel_name(const KernelChoice &c) {
    // the pipeline is named by its walk kernel: k_wf_dist_walk (beside k_wf_shadow_walk), or k_wf_walk where one kernel runs both
    static const char *const family[] = {"k_render_wave", "k_render_wave_wg", "k_render_wave_wg2", "k_render_wave_wg3", "k_wf_dist_walk", "k_wf_segment_vertex"};
    static const char *const medium[] = {"HomogeneousMedium", "HomogeneousMediumT<0,false>", "HomogeneousMediumT<1,false>", "HomogeneousMediumT<2,false>",
                                         "HomogeneousMediumT<2,true>", "GridMedium", "GridMediumGrey", "NanoDenseMedium", "NanoDenseMediumGrey", "RgbGridMedium"};
    // (the guided workgroup kernel over a non-grey scene has always been reported under the full-scene medium's name)
    const MediumInst m = c.medium == MediumInst::HomogeneousSimple && c.guided ? MediumInst::Homogeneous : c.medium;
    return std::string(c.family == Family::WfWalk && c.wf_merged ? "k_wf_walk" : family[(int)c.family]) + "<" + medium[(int)m] + (c.guided ? ",guided" : "") +
           (c.train ? ",train" : "") + ">";
}

}  // namespace vspg_choice
