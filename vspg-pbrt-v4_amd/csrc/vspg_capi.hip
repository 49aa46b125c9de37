// vspg_capi.hip -- the renderer behind the C-ABI of include/vspg.h: its kernels (gfx950), its buffers, every launch and the entry
// points that take a renderer.  Three kernel families are text of this translation unit kept in headers (vspg_train_kernels.h,
// vspg_wg_sched.h, vspg_probe_kernels.h); scene preprocessing and the entry points that need no renderer are host code in units of
// their own (vspg_scene_build.hip, vspg_scene_api.hip).
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared (see csrc/Makefile).
// No CPU fallback lives here: every compute entry point needs a HIP device.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>
#include <algorithm>

#include "vspg_path.h"
#include "vspg_wg_kernel.h"
#include "vspg_guided_wg.h"
#include "vspg_wg3.h"
#include "vspg_trace.h"
#include "vspg_wavefront.h"
#include "vspg_wf_launch.h"
#include "vspg_film_error.h"
#include "vspg_film_resolve.h"
#include "vspg_kernel_choice.h"
#include "vspg_error.h"
#include "vspg_scene_build.h"
#ifdef VSPG_SINGLE_TU  // diagnostic builds that read device-side globals of the pipeline kernels (VSPG_WF_STATS, VSPG_PROFILE, VSPG_WF_DEBUG)
#include "vspg_wf_grid.hip"
#include "vspg_wf_nvdb.hip"
#include "vspg_wf_rgbgrid.hip"
#include "vspg_wg3_exact.hip"
#endif

using namespace vspg;
using namespace vspg_choice;
using namespace vspg_host;

// =======================================================================================
// kernels
// =======================================================================================
namespace {

constexpr int kBlock = 256;
static_assert(kBlock == kGuideBlock, "the guiding scratch in LDS is sized for kBlock threads");
#ifndef VSPG_WAVES_PER_SIMD
#define VSPG_WAVES_PER_SIMD 2
#endif
constexpr int kWavesPerSimd = VSPG_WAVES_PER_SIMD;  // register budget of k_render_wave: 512 / kWavesPerSimd VGPRs
constexpr int kBlocksPerCU = kWavesPerSimd;         // persistent 256-thread blocks per CU == resident blocks
constexpr int kChunk = 64;        // dynamic work items a wavefront claims per atomic (one 8x8 pixel tile)
constexpr int kNumCounters = 7;  // paths, segments, volume_scatters, surface_hits, density_queries, shadow_rays, shadow_density_queries

template <class PC>
__device__ __forceinline__ void flush_counters(const PC &pc, uint32_t paths, unsigned long long *g) {
    __shared__ unsigned int s[kNumCounters];
    if (threadIdx.x < kNumCounters) s[threadIdx.x] = 0;
    __syncthreads();
    atomicAdd(&s[0], paths);
    atomicAdd(&s[1], pc.segments);
    atomicAdd(&s[2], pc.volume_scatters);
    atomicAdd(&s[3], pc.surface_hits);
    atomicAdd(&s[4], pc.density_queries);
    atomicAdd(&s[5], pc.shadow_rays);
    atomicAdd(&s[6], pc.shadow_queries);
    __syncthreads();
    if (threadIdx.x < kNumCounters) atomicAdd(&g[threadIdx.x], (unsigned long long)s[threadIdx.x]);
}

// (reset_sibling_head -- the pair of global work heads used by alternate launches -- lives in vspg_wg3.h)
// Persistent wavefront kernel with path regeneration.
//   work item  = one pixel (all its samples [wave_start, wave_end) run in order by the lane that
//                claims it, so film / ISG statistics are read-modify-written by exactly one lane
//                per launch: no atomics, deterministic summation order);
//   claiming   = lanes whose path has ended are compacted with a wave ballot + prefix count and
//                served by ONE atomicAdd per wavefront on the global work head (stochastic path
//                termination -- Russian roulette, absorption at maxdepth -- leaves holes in the
//                wave; regeneration refills them instead of idling until the longest path ends);
//   path state = registers for the whole life of a path (no HBM round trip per segment);
//   items are tile-ordered (8x8 pixels per 64 items) so a fresh wavefront starts on one coherent
//   tile of primary rays.
template <class Medium, bool GUIDED, bool TRAIN = false>
__global__ __launch_bounds__(kBlock, kWavesPerSimd) void k_render_wave(const DScene *__restrict__ Sp, float4 *__restrict__ film,
                                                        float *__restrict__ isg_stats, const float *__restrict__ vsp_buf,
                                                        int vsp_ready, int wave_start, int wave_end,
                                                        int first_sample, int single_sample, PcgJump jump,
                                                        unsigned static_per_wave, unsigned dyn_base,
                                                        unsigned int *__restrict__ work_head,
                                                        unsigned long long *__restrict__ counters, TrainArgs train,
                                                        PixelWindow win) {
    // win: the pixels the launch covers (vspg_render_window; the whole frame for vspg_render_wave) -- items count over the 8x8 tiles
    // of the frame's grid that touch it, pixels outside it are masked like tile padding
    // first_sample: first sample index of this shard in [wave_start, wave_end); single_sample: the
    // launch covers exactly one sample per pixel (the reference's 1-spp waves) and `jump` is the
    // PCG skip-ahead for first_sample*65536
    const DScene &S = *Sp;
    const int W = S.xres;
    const int tilesX = win_tiles_x(win), tilesY = win_tiles_y(win);
    const unsigned total_items = (unsigned)(tilesX * tilesY) * 64u;
    const int lane = threadIdx.x & 63;
    reset_sibling_head(work_head);
    // heterogeneous media: the 16^3 majorant grid (16 KB) is staged into LDS once per workgroup with
    // coalesced 16-B loads; every DDA step then reads LDS instead of HBM/L2.  (Guided builds leave it in
    // global memory -- it stays in the vector L1: their 72 KB of guiding scratch plus the grid would allow
    // one block per CU only.)
    const float *maj_ptr = nullptr;
    if constexpr (!GUIDED && (std::is_same<Medium, GridMedium>::value || std::is_same<Medium, GridMediumGrey>::value)) {
        __shared__ float s_maj[kMajRes * kMajRes * kMajRes];
        const float4 *src = reinterpret_cast<const float4 *>(S.majorant);
        float4 *dst = reinterpret_cast<float4 *>(s_maj);
        for (int i = threadIdx.x; i < kMajRes * kMajRes * kMajRes / 4; i += kBlock) dst[i] = src[i];
        __syncthreads();
        maj_ptr = s_maj;
    }
    stage_scene_lds(S);
    __syncthreads();
    const Medium medium = MediumMaker<Medium>::make(S, maj_ptr);
    // guided builds: the per-lane guiding scratch (vspg_guiding.h: 9 floats x 8 lobes) lives in LDS,
    // element e of lane t at s_gmix[e * kBlock + t] (conflict-free)
    float *glds = nullptr;
    if constexpr (GUIDED) glds = guide_lds();
    typename std::conditional<TRAIN, PathCountersT<PathRecorder>, PathCounters>::type pc;
    pc.segments = pc.volume_scatters = pc.surface_hits = pc.density_queries = pc.shadow_rays = pc.shadow_queries = 0;
    if constexpr (TRAIN) {
        pc.rec.base = train.segbuf;  // re-pointed at the lane's work item when a path starts
        pc.rec.stride = (int)train.n_items;
        pc.rec.max_seg = train_rec_capacity(S.prm.maxdepth);
        pc.rec.reset();
    }
    uint32_t paths = 0;

    bool has = false;        // this lane carries a live path
    bool exhausted = false;  // wave-uniform: the global work head ran past the last item
    // wave-local slice [local_next, local_end) of the item space.  Every wavefront starts with a
    // STATIC slice (static_per_wave items, ~3/4 of its fair share, no atomics at all); the remaining
    // items [dyn_base, total) are handed out dynamically in chunks of kChunk through one returning
    // atomic per chunk, which evens out the tail.  (One atomic per refill on a single hot counter
    // saturates at ~10^2 dequeues/us on this chip and capped the kernel at the atomic rate.)
    const unsigned wave_id = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    unsigned local_next = wave_id * static_per_wave, local_end = local_next + static_per_wave;
    int px = 0, py = 0, s = 0, ch = 0;
    Sampler sampler;
    PathState st;
    IsgSample isg;

    // Training launches (one sample per pixel): every path writes its segment records into its OWN column of a
    // buffer sized for the whole wave (1.3 GB at 1080p -- this part has 288 GB) and leaves; PropagateSamples runs
    // afterwards as its own kernel over all paths at full occupancy (k_propagate).  Propagating inside this kernel
    // meant a lock-step loop over the longest recorded path, ~100 dependent loads, for the few lanes that had just
    // finished (8.0 ms per training wave), or parking finished lanes until enough had gathered (4.4 ms).
    unsigned my_item = 0;
    while (true) {
        // ---- regeneration: ballot the empty lanes, prefix-count them, hand out items -----------
        unsigned long long need = __ballot(!has);
        if (need != 0ull && !(exhausted && local_next >= local_end)) {
            if (local_next >= local_end && !exhausted) {
                unsigned base = 0;
                if (lane == 0) base = atomicAdd(work_head, (unsigned)kChunk);
                base = __builtin_amdgcn_readfirstlane(base) + dyn_base;
                local_next = base;
                local_end = base + (unsigned)kChunk < total_items ? base + (unsigned)kChunk : total_items;
                if (base + (unsigned)kChunk >= total_items) exhausted = true;
                if (base >= total_items) local_next = local_end = 0;
            }
            const unsigned rank = (unsigned)__popcll(need & ((1ull << lane) - 1ull));
            const unsigned avail = local_end - local_next;  // lanes beyond `avail` wait for the next chunk
            if (!has && rank < avail) {
                VSPG_PROF(PS_START);
                const unsigned item = local_next + rank;
                const unsigned tile = item >> 6, l = item & 63u;
                px = (win_tile_x0(win) + (int)(tile % (unsigned)tilesX)) * 8 + (int)(l & 7u);
                py = (win_tile_y0(win) + (int)(tile / (unsigned)tilesX)) * 8 + (int)(l >> 3);
                s = first_sample;
                if (win_has(win, px, py) && s < wave_end) {
                    if (single_sample)
                        start_path<!Medium::kSimpleScene>(S, vsp_buf, vsp_ready, px, py, jump, sampler, st, &ch, isg);
                    else
                        start_path<!Medium::kSimpleScene>(S, vsp_buf, vsp_ready, px, py, s, sampler, st, &ch, isg);
                    has = true;
                    if constexpr (GUIDED) load_contribution_estimate(S, px, py, st);
                    if constexpr (TRAIN) {
                        my_item = item;
                        pc.rec.base = train.segbuf + item;
                        pc.rec.reset();
                    }
                }
            }
            const unsigned cnt = (unsigned)__popcll(need);
            local_next += cnt < avail ? cnt : avail;
        }
        if (__ballot(has) == 0ull) {
            if (exhausted && local_next >= local_end) break;
            continue;
        }
        // ---- one path segment for every live lane ----------------------------------------------
        bool finished = false;
        if (has) {
            const bool alive = li_segment<Medium, GUIDED>(S, medium, vsp_buf, vsp_ready, px, py, st, ch, sampler, isg, pc, glds, kBlock);
            if (!alive) {
                VSPG_PROF(PS_FINISH);
                const Spec L = finish_radiance(st.L);
                const size_t idx = (size_t)py * W + px;
                film_add_sample(film + idx, L);
                isg_add_sample_atomic(isg_stats + idx * VSPG_ISG_STATS, L, isg);
                paths++;
                finished = true;
                if constexpr (TRAIN) train.seg_count[my_item] = pc.rec.n;  // PropagateSamples (:627) follows in k_propagate
            }
        }
        if (finished) {
            s += S.shard_count > 1 ? S.shard_count : 1;
            if (!TRAIN && s < wave_end) {
                start_path<!Medium::kSimpleScene>(S, vsp_buf, vsp_ready, px, py, s, sampler, st, &ch, isg);  // next sample of the same pixel
                if constexpr (GUIDED) load_contribution_estimate(S, px, py, st);
            } else {
                has = false;
            }
        }
    }
    flush_counters(pc, paths, counters);
}

}  // namespace

// (three kernel families of this unit are kept in headers, each included where its text stood: the order of definitions is theirs)
#include "vspg_train_kernels.h"  // the guiding-field update: k_propagate, k_field_aux, k_train_*
#include "vspg_wg_sched.h"       // k_render_wave_wg, k_render_wave_wg2

namespace {

// film += the launch's sample buffer; ISG statistics likewise (the same read-modify-write forms the in-kernel flush used)
// (over the window of the launch that parked them: the planes hold nothing of that launch outside it)
__global__ __launch_bounds__(kBlock) void k_film_resolve(int W, PixelWindow win, const float4 *__restrict__ wave_samples, float4 *__restrict__ film,
                                                         float *__restrict__ isg_stats) {
    const size_t j = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const size_t ww = (size_t)(win.x1 - win.x0);
    if (j >= ww * (size_t)(win.y1 - win.y0)) return;
    const size_t i = ((size_t)win.y0 + j / ww) * (size_t)W + (size_t)win.x0 + j % ww;
    const float4 parked = wave_samples[i];
    if (carry_sentinel(parked.w)) return;  // (a path still in flight, vspg_wg3.h CARRY: none is left behind the drain that runs before this kernel)
    resolve_sample(parked, film + i, isg_stats + i * VSPG_ISG_STATS);
}

// (k_trace_paths: vspg_trace.h)
}  // namespace

#include "vspg_probe_kernels.h"  // the parity probes' kernels; the brick and majorant builders
#include "vspg_rgb_update_kernels.h"  // the RGB grid medium's storage rebuilt on the device (vspg_renderer_update_rgb_grids)

// =======================================================================================
// host side
// =======================================================================================

struct VspgRenderer {
    VspgScene scene;
    VspgIntegratorParams prm;
    VspgRenderConfig cfg;
    int arith = VSPG_ARITH_EXACT;   // vspg_renderer_set_arithmetic (vspg_arith.h): which instantiations the path kernels are launched from
    std::string kernel_name_buf;
    DScene hscene;
    DScene *dscene = nullptr;
    float4 *film = nullptr;
    float *isg_stats = nullptr;
    float *contrib = nullptr;     // guided RR: contribution estimate, W*H
    float *tr_rgb = nullptr;      // TrBuffer: W*H*3 running mean, W*H sample counts
    int32_t *tr_spp = nullptr;
    float *vsp = nullptr;
    unsigned long long *counters = nullptr;
    unsigned int *work_head = nullptr;   // two counters, used by alternate launches (reset_sibling_head)
    unsigned int *work_head8_raw = nullptr, *work_head8 = nullptr;  // k_render_wave_wg3's: two sets of kWg3Heads cursors, 2 KB-aligned
    unsigned int head8_parity = 0;
    unsigned int head_parity = 0;
    VspgKdNode *fnodes[2] = {nullptr, nullptr};        // guiding fields (device copies)
    VspgFieldRegion *fregions[2] = {nullptr, nullptr};
    float *faux[2] = {nullptr, nullptr};               // DField::aux
    float4 *flobes[2] = {nullptr, nullptr};            // DField::lobes
    bool field_set = false;
    bool medium_grey = false;   // homogeneous medium with bitwise-grey sigma_a, sigma_s, Le
    bool surfaces_grey = false; // every rectangle's (clamped) Kd bitwise grey
    bool null_zero = false;     // homogeneous medium whose ClampZero((sigma_t - sigma_a) - sigma_s) is exactly 0 per channel
    // a18: on-device training of the guiding field
    bool training = false;
    int field_iteration = 0;
    float *segbuf = nullptr;                  // segment records of a training wave, one column per work item
    int *seg_count = nullptr;                 // records per work item
    size_t segbuf_items = 0;
    VspgTrainSample *samples = nullptr;
    unsigned long long sample_capacity = 0;
    unsigned long long *train_counters = nullptr;  // [0] samples, [1] zero-valued, [2..3] spare
    RegionStats *rstats[2] = {nullptr, nullptr};
    float *train_acc = nullptr;               // kTrainCapRegions x kStatFloats accumulators of one pass
    float *train_sumw = nullptr;        // [0] sum of sample weights, [1] sample count (as a float, for the cross-rank sum)
    VspgExchangeFn exchange = nullptr;  // sharded training: sums a device buffer over the ranks (vspg_renderer_set_exchange)
    void *exchange_user = nullptr;
    int *train_reg = nullptr;                 // region of every sample of the batch (field being updated)
    unsigned int *train_order = nullptr;      // sample indices sorted by region
    unsigned int *train_hist = nullptr, *train_cursor = nullptr, *train_nsorted = nullptr;
    int *train_nsplit = nullptr;              // [0] regions the split pass of the running update created (both fields), [1] a region without lobes exists
    float *density = nullptr;   // GridMedium density samples (raw; released once the octet bricks are built)
    int32_t *brick_index = nullptr;
    float4 *octets = nullptr;
    size_t n_bricks = 0;
    float *le_scale = nullptr;  // emissive GridMedium: LeScale grid
    float *temperature = nullptr;  // temperature grid (raw samples)
    float *majorant = nullptr;  // 16^3 majorant grid
    float4 *rgb_oct[2] = {nullptr, nullptr};  // RGB grid medium: the octets of the sigma_a / sigma_s grid (vspg_rgbgrid.h), null = absent
    float *rgb_Le = nullptr;                  // ... its Le grid, raw
    float *env_buf[VSPG_MAX_INFINITE_LIGHTS] = {nullptr, nullptr, nullptr, nullptr};  // image infinite lights: one allocation per light (DEnvLight's arrays)
    void *light_img_buf[VSPG_MAX_POINT_LIGHTS] = {};  // projection / goniometric lights: one allocation per slot (DImageLight::texels)
    float4 *tex_buf[VSPG_MAX_TEXTURES] = {};  // image textures: one allocation per texture (DTexture::texels)
    float *tri_uv = nullptr;                  // ... the textured triangles' uv side array (DScene::tri_uv)
    int n_textured = 0;                       // surfaces that carry a texture (ChoiceFacts::n_textured)
    int n_texture_slots = 0;                  // VspgSceneTextures::n_textures of the scene the renderer was created with
    std::vector<int32_t> tri_pos;             // triangle of the caller's soup -> position in `tris`, -1 = dropped (vspg_texture_eval_batch)
    DTri *tris = nullptr;          // triangle soup in BVH leaf order + the BVH (depth-first, skip links)
    DBvh4Node *bvh = nullptr;
    // wavefront pipeline (vspg_wavefront.h): path SoA, lists and per-iteration control blocks, allocated at first use
    float *wf_pool = nullptr;
    // k_render_wave_wg2: one {L, ISG code} per pixel of a one-sample launch.  The samples of launch w enter the film at the start of
    // launch w + 1 (inside the kernel, as each pixel's new path begins) or, when anything else wants the film or the statistics
    // first, through k_film_resolve (flush_parked_samples): two buffers, `ws_parked` says the other one holds unresolved samples.
    float4 *wave_samples[2] = {nullptr, nullptr};
    int ws_cur = 0;
    bool ws_parked = false;
    PixelWindow ws_win = {0, 0, 0, 0};  // the window of the launch that parked them (vspg_render_window)
    hipStream_t ws_stream = nullptr;  // the stream of the launch that parked them
    hipEvent_t ws_event = nullptr;    // recorded behind that launch: whoever touches the parked samples on another stream waits on it
    // k_render_wave_wg3_carry (vspg_wg3.h, CARRY): the paths a one-sample launch left in flight, one image per workgroup.  The next launch
    // of the same shape resumes them; anything else drains them first (drain_carried_paths, through flush_parked_samples).  Two
    // buffers like the sample planes: a launch resumes from the one its predecessor suspended into and suspends into the other.
    unsigned int *carry_img[2] = {nullptr, nullptr};
    int carry_cur = 0;
    bool carry_pending = false;
    Wg3Launch carry_shape = {};       // the launch that wrote the pending image: instantiation, grid, window
    int carry_arith = 0;              // ... and its arithmetic mode
    unsigned long long carry_resumes = 0;  // launches that resumed from an image (vspg_debug_carry_resumes)
    unsigned long long carry_kept = 0;     // ... that suspended nothing because an update was due behind them (vspg_debug_carry_kept)
    bool step_post_processed = false;      // vspg_post_process_step ran since the last path launch: the caller post-processes its steps
    unsigned int *wf_lists = nullptr;   // 4 x n_items: active (even / odd iterations), walk, shadow
    hipStream_t wf_stream2 = nullptr;   // the shadow walks' stream (wf_render_pass)
    hipEvent_t wf_ev_vertex = nullptr, wf_ev_shadow = nullptr;
    WfIter *wf_iters = nullptr;
    size_t wf_items = 0;
    int num_cus = 0;
    int vsp_ready = 0;
    bool vsp_loaded = false;  // ImageSpaceGuidingBuffer(fileName): no further updates
    int wave_counter = 0, buffer_wave = 0;
    size_t npix = 0;
    // film error against a reference image (vspg_film_error.h): allocated by the first vspg_renderer_set_reference_image
    float4 *fe_ref = nullptr;            // the reference image, a padded float4 per pixel, full frame
    bool fe_ref_set = false;
    double *fe_partials = nullptr;       // six sums per row of the window being reduced (yres rows)
    VspgFilmError *fe_log = nullptr;     // VSPG_FILM_ERROR_LOG_RECORDS records
    size_t fe_count = 0;                 // records enqueued since the last read (the host's count: enqueue order is host order)
    hipStream_t fe_stream = nullptr;     // the stream of the last enqueue ...
    hipEvent_t fe_event = nullptr;       // ... and an event behind it: the partial sums are shared, an enqueue on another stream waits
    bool fe_inflight = false;
    // the resolved film (vspg_film_resolve.h): allocated by the first vspg_film_resolve
    void *rs_stage = nullptr;            // the window's pixel values on their way to the host: at most npix * 12 bytes
    unsigned int *rs_clamped = nullptr;  // pixels the fp16 clamp touched in the last resolve
};

// Upload one light's tables into a fresh allocation and point the HOST scene record's slot at it.  The caller copies the record to
// the device and frees *old_buf once no launch can read it.
static int env_install(VspgRenderer *r, int k, const EnvTables &T, const float *m, const float *mi, hipStream_t s, float **old_buf) {
    float *buf = nullptr;
    HIPCHK(hipMalloc(&buf, T.buf.size() * sizeof(float)));
    hipError_t e = hipMemcpyAsync(buf, T.buf.data(), T.buf.size() * sizeof(float), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // (the host vector is pageable and the caller's to drop)
    if (e != hipSuccess) {
        (void)hipFree(buf);
        return fail(VSPG_EHIP, std::string("uploading the environment image: ") + hipGetErrorName(e));
    }
    DEnvLight &E = r->hscene.env[k];
    E.res = T.res;
    E.integral = T.integral;
    for (int j = 0; j < 9; ++j) { E.m[j] = m[j]; E.mi[j] = mi[j]; }
    for (int c = 0; c < 3; ++c) E.sum_L[c] = T.sum_L[c];
    E.texels = buf;
    E.func = buf + T.o_func;
    E.cdf = buf + T.o_cdf;
    E.mfunc = buf + T.o_mfunc;
    E.mcdf = buf + T.o_mcdf;
    *old_buf = r->env_buf[k];
    r->env_buf[k] = buf;
    return 0;
}

// The same for a projection / goniometric light's image (point-light slot k)
static int image_light_install(VspgRenderer *r, int k, const ImageLightTables &T, hipStream_t s, void **old_buf) {
    void *buf = nullptr;
    HIPCHK(hipMalloc(&buf, T.buf.size() * sizeof(float)));
    hipError_t e = hipMemcpyAsync(buf, T.buf.data(), T.buf.size() * sizeof(float), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        (void)hipFree(buf);
        return fail(VSPG_EHIP, std::string("uploading the light image: ") + hipGetErrorName(e));
    }
    image_light_apply(T, &r->hscene.image_light[k]);
    r->hscene.image_light[k].texels = buf;
    *old_buf = r->light_img_buf[k];
    r->light_img_buf[k] = buf;
    return 0;
}

// The same for a texture's image (texture k): `img` is texture_image_build's, one float4 per texel
static int texture_install(VspgRenderer *r, int k, const std::vector<float> &img, int xres, int yres, hipStream_t s, float4 **old_buf) {
    float4 *buf = nullptr;
    HIPCHK(hipMalloc(&buf, img.size() * sizeof(float)));
    hipError_t e = hipMemcpyAsync(buf, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        (void)hipFree(buf);
        return fail(VSPG_EHIP, std::string("uploading the texture image: ") + hipGetErrorName(e));
    }
    DTexture &T = r->hscene.tex[k];
    T.texels = buf;
    T.xres = xres;
    T.yres = yres;
    *old_buf = r->tex_buf[k];
    r->tex_buf[k] = buf;
    return 0;
}

// One pass of the wavefront pipeline: sample index `sample` of every pixel.  The pipeline's kernels are instantiated in their own
// translation units (vspg_wf_grid.hip / vspg_wf_nvdb.hip: wf_dispatch_*, vspg_wf_launch.h), which `make -j` builds beside this one;
// here the pass is prepared -- buffers, grids, streams -- and handed over as a plain WfLaunch.
static int wf_render_pass(VspgRenderer *r, const KernelChoice &c, const PixelWindow &win, int sample, hipStream_t s) {
    const bool nvdb = r->scene.medium.type == VSPG_MEDIUM_NANOVDB, guided = c.guided, train = c.train, grey = r->medium_grey;
    const int tilesX = win_tiles_x(win), tilesY = win_tiles_y(win);  // the pass's slots: the pixels of the window's tiles
    const size_t items = (size_t)tilesX * tilesY * 64;
    // Path-loop iterations of a pass.  Without medium boundaries every iteration ends at a vertex and raises the depth: maxdepth + 1
    // of them.  With boundaries an iteration may instead cross an interface (Li's `continue` at :399-404, depth unchanged): the loop
    // runs until the list is empty -- a convex bounding shape costs at most two crossings per vertex -- under a generous cap.
    const bool bnd = r->hscene.has_boundaries != 0;
    const int base_iters = r->prm.maxdepth + 1;
    const int max_iters = bnd ? 4 * (r->prm.maxdepth + 2) + 16 : base_iters;
    const int n_iters = max_iters + 1;
    if (!r->wf_pool || r->wf_items < items) {  // (grown, never shrunk: a renderer may be given several windows)
        if (r->wf_pool) (void)hipFree(r->wf_pool);
        if (r->wf_lists) (void)hipFree(r->wf_lists);
        if (r->wf_iters) (void)hipFree(r->wf_iters);
        r->wf_pool = nullptr; r->wf_lists = nullptr; r->wf_iters = nullptr;
        HIPCHK(hipMalloc(&r->wf_pool, (size_t)kWfPoolFloats * items * sizeof(float)));
        HIPCHK(hipMalloc(&r->wf_lists, 4 * items * sizeof(unsigned int)));
        HIPCHK(hipMalloc(&r->wf_iters, (size_t)n_iters * sizeof(WfIter)));
        r->wf_items = items;
    }
    HIPCHK(hipMemsetAsync(r->wf_iters, 0, (size_t)n_iters * sizeof(WfIter), s));
    WfLaunch L;
    WfArgs &a = L.a;
    a.scene = r->dscene;
    a.P = WfPool{r->wf_pool, items};
    a.film = r->film;
    a.isg_stats = r->isg_stats;
    a.vsp_buf = r->vsp;
    a.vsp_ready = r->vsp_ready;
    a.sample = sample;
    a.jump = pcg_jump((unsigned long long)sample * 65536ull);
    a.n_items = (unsigned)items;
    a.tilesX = (unsigned)tilesX;
    a.pix_org = (unsigned)(win.x0 & ~7) | ((unsigned)(win.y0 & ~7) << 16);
    a.win = win;
    a.list_active = r->wf_lists;
    a.list_active2 = r->wf_lists + items;
    a.list_walk = r->wf_lists + 2 * items;
    a.list_shadow = r->wf_lists + 3 * items;
    a.iters = r->wf_iters;
    a.counters = r->counters;
    a.train = TrainArgs{nullptr, nullptr, nullptr, nullptr, 0, 0};
    a.rec_cap = train_rec_capacity(r->prm.maxdepth);
    {   // (VSPG_WF_COMPACT=0: the full layout for a grey medium too -- same results, for A/B runs)
        const char *e = getenv("VSPG_WF_COMPACT");
        a.compact_results = grey && !(e && e[0] == '0') ? 1 : 0;
    }
    if (train) {  // a18: the pass records path segments; PropagateSamples (k_propagate) follows it
        a.train = TrainArgs{r->segbuf, r->seg_count, r->samples, r->train_counters, r->sample_capacity, (unsigned)items};
        HIPCHK(hipMemsetAsync(r->seg_count, 0, items * sizeof(int), s));
    }
    {   // tuning knobs (defaults measured on the 256^3 cloud stand-in)
        const char *e1 = getenv("VSPG_WF_ROUNDS"), *e2 = getenv("VSPG_WF_REFILL");
        a.walk_rounds = e1 ? atoi(e1) : (nvdb ? GridMediumT<true>::kAdvanceRounds : GridMediumT<false>::kAdvanceRounds);
        a.walk_refill = e2 ? atoi(e2) : kWfRefill;
        if (a.walk_rounds < 1) a.walk_rounds = 1;
        if (a.walk_refill < 1) a.walk_refill = 1;
        if (a.walk_refill > 64) a.walk_refill = 64;

    }
    // persistent grids: the dense kernels stride over their list, the walk kernels pull jobs
    const unsigned max_blocks = (unsigned)((items + kWfBlock - 1) / kWfBlock);
    // (the two walk kernels of neighbouring iterations run side by side: VSPG_WF_WALK_BLOCKS / VSPG_WF_SHADOW_BLOCKS = resident
    // workgroups per CU of each, within their launch bounds)
    static const int walk_blocks = [] { const char *e = getenv("VSPG_WF_WALK_BLOCKS"); const int v = e ? atoi(e) : 0; return v >= 1 && v <= kWfWalkWavesPerSimd ? v : kWfWalkWavesPerSimd; }();
    static const int shadow_blocks = [] { const char *e = getenv("VSPG_WF_SHADOW_BLOCKS"); const int v = e ? atoi(e) : 0; return v >= 1 && v <= kWfShadowWavesPerSimd ? v : kWfShadowWavesPerSimd; }();
    L.dense = (unsigned)r->num_cus * 8u;
    L.walk = (unsigned)r->num_cus * (unsigned)walk_blocks;
    L.swalk = (unsigned)r->num_cus * (unsigned)shadow_blocks;
    const int merged_blocks = [] { const char *e = getenv("VSPG_WF_MERGED_BLOCKS"); const int v = e ? atoi(e) : 0; return v >= 1 && v <= kWfMergedWavesPerSimd ? v : kWfMergedWavesPerSimd; }();  // (read per pass)
    L.mwalk = (unsigned)r->num_cus * (unsigned)merged_blocks;
    if (L.dense > max_blocks) L.dense = max_blocks;
    if (L.walk > max_blocks) L.walk = max_blocks;
    if (L.swalk > max_blocks) L.swalk = max_blocks;
    if (L.mwalk > max_blocks) L.mwalk = max_blocks;
    // The shadow walk of iteration i runs beside the distance walk of iteration i + 1, on the renderer's second stream; the
    // vertex kernel of iteration i + 1 waits for both (it adds the shadow walk's result first thing).  VSPG_WF_SERIAL=1 keeps
    // everything on the caller's stream (same results; for A/B runs and debugging).
    L.serial = [] { const char *e = getenv("VSPG_WF_SERIAL"); return e && *e && *e != '0'; }();  // (read per pass: a test flips it)
    if (!L.serial && !r->wf_stream2) {
        HIPCHK(hipStreamCreateWithFlags(&r->wf_stream2, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&r->wf_ev_vertex, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&r->wf_ev_shadow, hipEventDisableTiming));
    }
    // both walks of an iteration as ONE kernel where the job lists are short or a third kernel sits in the chain (boundary scenes,
    // guided pipelines); side by side on two streams for dense unguided clouds (k_wf_walk, vspg_wavefront.h: measured both ways).
    // VSPG_WF_MERGED=0|1 overrides (choose_kernel; decided per call: tests and A/Bs flip it).
    L.merged = c.wf_merged;
    // job cursors of the merged walk kernel's stream: boundary scenes' short lists are dealt out to kWfSegs of them (wf_claim_refill;
    // VSPG_WF_SEGS=1|8 overrides, read per pass)
    L.segs = bnd ? kWfSegs : 1;
    if (const char *e = getenv("VSPG_WF_SEGS")) L.segs = atoi(e) > 1 ? kWfSegs : 1;
    L.s = s;
    L.s2 = L.serial ? s : r->wf_stream2;
    L.ev_vertex = r->wf_ev_vertex;
    L.ev_shadow = r->wf_ev_shadow;
    L.bnd = bnd;
    L.nds = r->prm.vspsamplingmethod != VSPG_VSP_RESAMPLING;
    L.emit = r->hscene.temperature != nullptr;
    L.maxdepth = r->prm.maxdepth;
    L.base_iters = base_iters;
    L.max_iters = max_iters;
    // (tolerance modes: vspg_renderer_set_arithmetic accepted the renderer only if vspg_fast.hip holds its instantiation)
    const int rc = r->arith == VSPG_ARITH_FAST_WEIGHTS ? vspg_arith1_wf_grid(&L, grey ? 1 : 0)
                   : r->arith == VSPG_ARITH_FAST     ? vspg_arith2_wf_grid(&L, grey ? 1 : 0)
                   : c.medium == MediumInst::RgbGrid ? wf_dispatch_rgbgrid(L, guided, train)
                   : nvdb                            ? wf_dispatch_nvdb(L, guided, train, grey)
                                                     : wf_dispatch_grid(L, guided, train, grey);
    if (rc == WF_E_NOT_DRAINED)
        return fail(VSPG_ESCOPE, "paths still alive after the pipeline's iteration cap: more medium-boundary crossings per vertex than a pass provides for");
    if (rc != 0) return fail(VSPG_EHIP, std::string("the wavefront pipeline: ") + hipGetErrorName((hipError_t)rc));
    if (train) {
        hipLaunchKernelGGL(k_propagate, dim3((unsigned)((items + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a.train, a.rec_cap);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

// Profiling markers (trace ranges): with VSPG_ROCTX=1 in the environment every vspg_render_wave / vspg_post_process_step
// call is a roctx range (rocprofv3 --marker-trace shows waves and post-processing on the timeline).  libroctx64 is looked up at
// run time, so the library carries no link dependency on it and costs nothing when the variable is unset.
namespace {
struct RoctxApi {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
    RoctxApi() {
        const char *e = getenv("VSPG_ROCTX");
        if (!e || !*e || *e == '0') return;
        // rocprofv3 listens to the rocprofiler-sdk's roctx; roctracer's libroctx64 (same entry points) serves older tools
        void *h = nullptr;
        for (const char *name : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"})
            if ((h = dlopen(name, RTLD_NOW | RTLD_GLOBAL))) break;
        if (!h) return;
        push = reinterpret_cast<int (*)(const char *)>(dlsym(h, "roctxRangePushA"));
        pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
        if (!push || !pop) push = nullptr, pop = nullptr;
    }
};
const RoctxApi g_roctx;
struct RoctxRange {
    explicit RoctxRange(const char *name) { if (g_roctx.push) g_roctx.push(name); }
    ~RoctxRange() { if (g_roctx.pop) g_roctx.pop(); }
};
// vspg_medium_point_batch (include/vspg.h): SamplePoint as the path kernels call it, and the majorant cell that holds the point
template <class Medium>
__global__ __launch_bounds__(kBlock) void k_medium_point_batch(const DScene *__restrict__ Sp, int n, const float *__restrict__ p, float *__restrict__ out) {
    const DScene &S = *Sp;
    stage_scene_lds(S);
    __syncthreads();
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const Medium medium = MediumMaker<Medium>::make(S, S.majorant);
    const V3 pr = ld3(p + 3 * (size_t)i);
    const MediumProps mp = medium.sample_point(pr);
    const V3 o = medium.offset(medium.to_medium(pr));
    constexpr int R = Medium::kRes;
    float maj = 0.f;
    if (o.x >= 0.f && o.x <= 1.f && o.y >= 0.f && o.y <= 1.f && o.z >= 0.f && o.z <= 1.f) {  // Inside(p, bounds); the cell as the DDA's set-up clamps it
        auto cell = [](float v) { return (int)(v < 0 ? 0.f : (v > (float)(R - 1) ? (float)(R - 1) : v)); };
        maj = S.majorant[cell(o.x * R) + R * (cell(o.y * R) + R * cell(o.z * R))];
    }
    float *q = out + (size_t)i * VSPG_MEDIUM_POINT_OUT;
    q[0] = mp.sigma_a.r; q[1] = mp.sigma_a.g; q[2] = mp.sigma_a.b;
    q[3] = mp.sigma_s.r; q[4] = mp.sigma_s.g; q[5] = mp.sigma_s.b;
    q[6] = mp.Le.r; q[7] = mp.Le.g; q[8] = mp.Le.b;
    q[9] = maj;
}
// A kernel instantiation as a value: what vspg_render_window's launch lambdas are handed.  Only the tuples named there are built -- each
// further one costs minutes of compile time.
template <class M, bool G = false, bool T = false, int NP = 0, int BLK = 0, int WV = 0>
struct KernelInst {
    using Medium = M;
    static constexpr bool guided = G, train = T;
    static constexpr int pool = NP, block = BLK, waves = WV;
};
template <class M, int NP> using WgHomogInst = KernelInst<M, false, false, NP, kWgBlockHomog, kWgWavesHomog>;
template <class M, int NP, bool T = false> using WgGuidedInst = KernelInst<M, true, T, NP, kWgBlockGuided, kWgWavesGuided>;
}  // namespace

extern "C" {

int vspg_renderer_create(const VspgScene *scene, const VspgIntegratorParams *params, const VspgRenderConfig *cfg,
                         VspgRenderer **out) {
    return vspg_renderer_create_textured(scene, nullptr, params, cfg, out);
}
int vspg_renderer_create_textured(const VspgScene *scene, const VspgSceneTextures *textures, const VspgIntegratorParams *params,
                                  const VspgRenderConfig *cfg, VspgRenderer **out) {
    if (!out) return fail(VSPG_EINVAL, "null out pointer");
    *out = nullptr;
    int rc = validate(scene, params, cfg);
    if (rc) return rc;
    static const VspgSceneTextures no_textures = {};
    const VspgSceneTextures &tx = textures ? *textures : no_textures;
    if ((rc = validate_textures(*scene, tx))) return rc;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        return fail(VSPG_ENODEVICE, std::string("no HIP device available (") + hipGetErrorName(e) + "); this library has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(VSPG_EINVAL, "device ordinal out of range");
    HIPCHK(hipSetDevice(cfg->device));
    VspgRenderer *r = new VspgRenderer();
    r->scene = *scene;
    r->prm = *params;
    if (r->prm.rrguiding) r->prm.minrrdepth = 1;  // guidedvolpathvspgintegrator.cpp:195-197
    r->cfg = *cfg;
    if (r->cfg.shard_count < 1) { r->cfg.shard_count = 1; r->cfg.shard_index = 0; }
    build_dscene(r->scene, r->prm, r->cfg, &r->hscene);
    apply_scene_textures(r->scene, tx, &r->hscene);
    r->n_texture_slots = tx.n_textures;
    {
        auto same = [](const float *v) { return std::memcmp(&v[0], &v[1], 4) == 0 && std::memcmp(&v[1], &v[2], 4) == 0; };
        const VspgMedium &m = r->scene.medium;
        r->medium_grey = m.type != VSPG_MEDIUM_NONE && m.type != VSPG_MEDIUM_RGBGRID && same(m.sigma_a) && same(m.sigma_s) && same(m.Le) && !m.temperature && !getenv("VSPG_NO_GREY");
        r->surfaces_grey = !getenv("VSPG_NO_GREY_KD");
        r->null_zero = m.type == VSPG_MEDIUM_HOMOGENEOUS && !getenv("VSPG_NO_NULLZERO");
        for (int k = 0; k < 3; ++k) r->null_zero = r->null_zero && !(r->hscene.sigma_n_raw[k] > 0) && r->hscene.sigma_n_raw[k] == r->hscene.sigma_n_raw[k];
        for (int i = 0; i < r->hscene.n_quads; ++i) r->surfaces_grey = r->surfaces_grey && same(r->hscene.quads[i].Kd);
    }
    r->npix = (size_t)cfg->xres * cfg->yres;
#define CK(expr)                                                                                                  \
    do {                                                                                                          \
        hipError_t e2 = (expr);                                                                                   \
        if (e2 != hipSuccess) {                                                                                   \
            vspg_renderer_destroy(r);                                                                             \
            return fail(VSPG_EHIP, std::string(#expr) + ": " + hipGetErrorName(e2));                              \
        }                                                                                                         \
    } while (0)
    if (scene->medium.type == VSPG_MEDIUM_GRID || scene->medium.type == VSPG_MEDIUM_NANOVDB) {
        const size_t n = (size_t)scene->medium.nx * scene->medium.ny * scene->medium.nz;
        std::vector<float> maj = scene->medium.type == VSPG_MEDIUM_GRID ? build_majorant_grid(scene->medium)
                                                                        : build_majorant_grid_nvdb(scene->medium);
        CK(hipMalloc(&r->density, n * sizeof(float)));
        CK(hipMemcpy(r->density, scene->medium.density, n * sizeof(float), hipMemcpyHostToDevice));
        CK(hipMalloc(&r->majorant, maj.size() * sizeof(float)));
        CK(hipMemcpy(r->majorant, maj.data(), maj.size() * sizeof(float), hipMemcpyHostToDevice));
        r->hscene.density = nullptr;
        r->hscene.majorant = r->majorant;
        {   // octet bricks (see DScene): flags on the device, slot numbering on the host, fill on the device
            const int nx = scene->medium.nx, ny = scene->medium.ny, nz = scene->medium.nz;
            const int bnx = (nx + 1 + 7) / 8, bny = (ny + 1 + 7) / 8, bnz = (nz + 1 + 7) / 8;
            const size_t nb = (size_t)bnx * bny * bnz;
            int32_t *dflags = nullptr, *dactive = nullptr;
            CK(hipMalloc(&dflags, nb * sizeof(int32_t)));
            hipLaunchKernelGGL(k_brick_flags, dim3((unsigned)nb), dim3(kBlock), 0, 0, r->density, nx, ny, nz, bnx, bny, dflags);
            std::vector<int32_t> flags(nb), index(nb), active;
            hipError_t ef = hipGetLastError();  // a launch that failed would leave the flags uninitialised
            if (ef == hipSuccess) ef = hipMemcpy(flags.data(), dflags, nb * sizeof(int32_t), hipMemcpyDeviceToHost);
            (void)hipFree(dflags);
            CK(ef);
            // Dense bricks: when storing EVERY brick fits the budget (16 KB per 8^3 voxels: 0.5 GB for 256^3, 4.3 GB for 512^3 of this
            // part's 288 GB) the index is dropped and a brick's slot is its position in the grid -- a density query is then one
            // memory round trip, not two dependent ones (measured: 11.4 -> 10.9 ms per 1080p cloud wave).  Sparse assets beyond the
            // budget keep the index (empty bricks cost no storage and no fetch).  VSPG_DENSE_BRICKS=0|1 forces either.
            const char *dense_env = getenv("VSPG_DENSE_BRICKS");
            const size_t dense_budget = (size_t)8 << 30;
            const bool dense = dense_env ? dense_env[0] == '1' : nb * 512 * 2 * sizeof(float4) <= dense_budget;
            for (size_t b = 0; b < nb; ++b) {
                const bool keep = dense || flags[b];
                index[b] = keep ? (int32_t)active.size() : -1;
                if (keep) active.push_back((int32_t)b);
            }
            r->n_bricks = active.size();
            if (!dense) {
                CK(hipMalloc(&r->brick_index, nb * sizeof(int32_t)));
                CK(hipMemcpy(r->brick_index, index.data(), nb * sizeof(int32_t), hipMemcpyHostToDevice));
            }
            CK(hipMalloc(&r->octets, (r->n_bricks ? r->n_bricks : 1) * 512 * 2 * sizeof(float4)));
            if (r->n_bricks) {
                CK(hipMalloc(&dactive, r->n_bricks * sizeof(int32_t)));
                hipError_t ea = hipMemcpy(dactive, active.data(), r->n_bricks * sizeof(int32_t), hipMemcpyHostToDevice);
                if (ea == hipSuccess) {
                    hipLaunchKernelGGL(k_brick_fill, dim3((unsigned)r->n_bricks), dim3(512), 0, 0, r->density, nx, ny, nz, bnx, bny, dactive, r->octets);
                    ea = hipGetLastError();
                    if (ea == hipSuccess) ea = hipDeviceSynchronize();
                }
                (void)hipFree(dactive);
                CK(ea);
            }
            (void)hipFree(r->density);  // the kernels read the bricks only
            r->density = nullptr;
            r->hscene.brick_index = r->brick_index;
            r->hscene.octets = r->octets;
            r->hscene.bnx = bnx; r->hscene.bny = bny; r->hscene.bnz = bnz;
        }
        r->scene.medium.density = nullptr;  // the host array belongs to the caller
        const VspgMedium &m = scene->medium;
        if (m.temperature) {  // as many samples as the density grid (media.cpp:283-288; the .nvdb reader checks the bounding boxes)
            CK(hipMalloc(&r->temperature, n * sizeof(float)));
            CK(hipMemcpy(r->temperature, m.temperature, n * sizeof(float), hipMemcpyHostToDevice));
            r->hscene.temperature = r->temperature;
            r->hscene.temperature_offset = m.temperature_offset;
            r->hscene.temperature_scale = m.temperature_scale;
            r->hscene.nvdb_le_scale = m.nvdb_le_scale;
        }
        // isEmissive = temperatureGrid ? true : Le_spec.MaxValue() > 0 (media.cpp:261)
        if (m.type == VSPG_MEDIUM_GRID && (m.temperature || m.Le[0] != 0 || m.Le[1] != 0 || m.Le[2] != 0)) {
            const float one = 1.f;  // "Lescale" absent: SampledGrid({1}, 1, 1, 1) (media.cpp:319-320)
            const float *src = m.le_scale ? m.le_scale : &one;
            const int lx = m.le_scale ? m.le_nx : 1, ly = m.le_scale ? m.le_ny : 1, lz = m.le_scale ? m.le_nz : 1;
            const size_t ln = (size_t)lx * ly * lz;
            CK(hipMalloc(&r->le_scale, ln * sizeof(float)));
            CK(hipMemcpy(r->le_scale, src, ln * sizeof(float), hipMemcpyHostToDevice));
            r->hscene.le_scale = r->le_scale;
            r->hscene.le_nx = lx; r->hscene.le_ny = ly; r->hscene.le_nz = lz;
        }
        r->scene.medium.le_scale = nullptr;
        r->scene.medium.temperature = nullptr;  // (the host array belongs to the caller)
    }
    if (scene->medium.type == VSPG_MEDIUM_RGBGRID) {  // majorants and the storage image are the host's (vspg_scene_build.hip); dense, no index
        const VspgMedium &m = scene->medium;
        const std::vector<float> maj = build_majorant_grid_rgb(*scene);
        CK(hipMalloc(&r->majorant, maj.size() * sizeof(float)));
        CK(hipMemcpy(r->majorant, maj.data(), maj.size() * sizeof(float), hipMemcpyHostToDevice));
        r->hscene.majorant = r->majorant;
        int bnx, bny, bnz;
        rgb_brick_counts(m, &bnx, &bny, &bnz);
        r->hscene.bnx = bnx; r->hscene.bny = bny; r->hscene.bnz = bnz;
        const float *src[2] = {scene->rgb_sigma_a, scene->rgb_sigma_s};
        for (int k = 0; k < 2; ++k)
            if (src[k]) {
                const std::vector<float> img = build_rgb_octets(src[k], m);
                CK(hipMalloc(&r->rgb_oct[k], img.size() * sizeof(float)));
                CK(hipMemcpy(r->rgb_oct[k], img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice));
            }
        r->hscene.rgb_oct_a = r->rgb_oct[0];
        r->hscene.rgb_oct_s = r->rgb_oct[1];
        if (scene->rgb_Le) {
            const size_t n3 = (size_t)m.nx * m.ny * m.nz * 3;
            CK(hipMalloc(&r->rgb_Le, n3 * sizeof(float)));
            CK(hipMemcpy(r->rgb_Le, scene->rgb_Le, n3 * sizeof(float), hipMemcpyHostToDevice));
            r->hscene.rgb_Le = r->rgb_Le;
        }
        r->scene.rgb_sigma_a = r->scene.rgb_sigma_s = r->scene.rgb_Le = nullptr;  // (the host arrays belong to the caller)
    }
    if (scene->n_triangles > 0) {
        std::vector<DTri> sorted;
        std::vector<DBvh4Node> nodes4;
        if (const int brc = build_triangle_bvh(*scene, &sorted, &nodes4, tx.tri_texture)) { vspg_renderer_destroy(r); return brc; }
        if (!sorted.empty()) {
            CK(hipMalloc(&r->tris, sorted.size() * sizeof(DTri)));
            CK(hipMemcpy(r->tris, sorted.data(), sorted.size() * sizeof(DTri), hipMemcpyHostToDevice));
            CK(hipMalloc(&r->bvh, nodes4.size() * sizeof(DBvh4Node)));
            CK(hipMemcpy(r->bvh, nodes4.data(), nodes4.size() * sizeof(DBvh4Node), hipMemcpyHostToDevice));
            r->hscene.n_tris = (int32_t)sorted.size();
            r->hscene.n_bvh_nodes = (int32_t)nodes4.size();
            r->hscene.tris = r->tris;
            r->hscene.bvh = r->bvh;
            r->tri_pos.assign((size_t)scene->n_triangles, -1);
            for (size_t i = 0; i < sorted.size(); ++i) r->tri_pos[(size_t)sorted[i].id] = (int32_t)i;
            const std::vector<float> uv = build_tri_uv(tx.tri_uv, sorted);  // (empty: no triangle is textured)
            if (!uv.empty()) {
                CK(hipMalloc(&r->tri_uv, uv.size() * sizeof(float)));
                CK(hipMemcpy(r->tri_uv, uv.data(), uv.size() * sizeof(float), hipMemcpyHostToDevice));
                r->hscene.tri_uv = r->tri_uv;
            }
        }
        r->n_textured = count_textured(*scene, tx, sorted);
        r->scene.tri_p = nullptr;  // the host arrays belong to the caller
        r->scene.tri_kd = nullptr;
        r->scene.tri_flags = nullptr;
    } else
        r->n_textured = count_textured(*scene, tx, std::vector<DTri>());
    r->hscene.n_textured = r->n_textured;
    for (int k = 0; k < tx.n_textures; ++k) {  // image textures (vspg_texture.h): one float4 per texel, built on the host
        const VspgTexture &t = tx.textures[k];
        float4 *old = nullptr;
        if (const int trc = texture_install(r, k, texture_image_build(t.pixels, t.xres, t.yres, t.channels), t.xres, t.yres, nullptr, &old)) {
            vspg_renderer_destroy(r);
            return trc;
        }
    }
    for (int k = 0; k < r->hscene.n_inf; ++k)
        if (r->hscene.inf_type[k] == VSPG_LIGHT_IMAGE_INFINITE) {  // the 1 x 1 white image (include/vspg.h): the light is valid from creation on
            const float white[3] = {1.f, 1.f, 1.f};
            EnvTables T;
            env_build_tables(white, 1, &T);
            float m[9], mi[9], *old = nullptr;
            env_matrices(nullptr, m, mi);
            if (const int erc = env_install(r, k, T, m, mi, nullptr, &old)) { vspg_renderer_destroy(r); return erc; }
        }
    for (int k = 0; k < r->hscene.n_point; ++k)
        if (r->hscene.point[k].type == VSPG_LIGHT_PROJECTION || r->hscene.point[k].type == VSPG_LIGHT_GONIOMETRIC) {  // the 1 x 1 image of ones
            const float ones[3] = {1.f, 1.f, 1.f};
            ImageLightTables T;
            image_light_build(r->hscene.point[k].type, ones, 1, 1, scene->point_lights[k].cone_angle_deg, &T);
            void *old = nullptr;
            if (const int irc = image_light_install(r, k, T, nullptr, &old)) { vspg_renderer_destroy(r); return irc; }
        }
    CK(hipMalloc(&r->dscene, sizeof(DScene)));
    CK(hipMemcpy(r->dscene, &r->hscene, sizeof(DScene), hipMemcpyHostToDevice));
    CK(hipMalloc(&r->film, r->npix * sizeof(float4)));
    CK(hipMemset(r->film, 0, r->npix * sizeof(float4)));
    CK(hipMalloc(&r->isg_stats, r->npix * VSPG_ISG_STATS * sizeof(float)));
    CK(hipMemset(r->isg_stats, 0, r->npix * VSPG_ISG_STATS * sizeof(float)));
    CK(hipMalloc(&r->vsp, r->npix * sizeof(float)));
    CK(hipMemset(r->vsp, 0, r->npix * sizeof(float)));
    CK(hipMalloc(&r->counters, kNumCounters * sizeof(unsigned long long)));
    CK(hipMemset(r->counters, 0, kNumCounters * sizeof(unsigned long long)));
    CK(hipMalloc(&r->work_head, 2 * sizeof(unsigned int)));
    CK(hipMemset(r->work_head, 0, 2 * sizeof(unsigned int)));
    CK(hipMalloc(&r->work_head8_raw, 4 * (size_t)kWg3HeadSetBytes));
    CK(hipMemset(r->work_head8_raw, 0, 4 * (size_t)kWg3HeadSetBytes));
    r->work_head8 = reinterpret_cast<unsigned int *>((reinterpret_cast<uintptr_t>(r->work_head8_raw) + 2 * (uintptr_t)kWg3HeadSetBytes - 1) &
                                                     ~(2 * (uintptr_t)kWg3HeadSetBytes - 1));  // (the sibling set is at address ^ kWg3HeadSetBytes)
    {
        hipDeviceProp_t prop;
        CK(hipGetDeviceProperties(&prop, cfg->device));
        r->num_cus = prop.multiProcessorCount;
    }
    if (r->prm.rrguiding) {
        CK(hipMalloc(&r->contrib, r->npix * sizeof(float)));
        CK(hipMemset(r->contrib, 0, r->npix * sizeof(float)));
        r->hscene.contrib = r->contrib;
        CK(hipMemcpy(r->dscene, &r->hscene, sizeof(DScene), hipMemcpyHostToDevice));
    }
    // calculateTrBuffer (guidedvolpathvspgintegrator.cpp:190-193); trBufferLoad is vspg_renderer_set_tr_buffer
    if (r->prm.storeTrBuffer || (r->prm.vspguiding && r->prm.vspprimaryguiding && r->prm.vspsamplingmethod == VSPG_VSP_NDS &&
                                 r->prm.collisionProbabilityBias)) {
        CK(hipMalloc(&r->tr_rgb, r->npix * 3 * sizeof(float)));
        CK(hipMemset(r->tr_rgb, 0, r->npix * 3 * sizeof(float)));
        CK(hipMalloc(&r->tr_spp, r->npix * sizeof(int32_t)));
        CK(hipMemset(r->tr_spp, 0, r->npix * sizeof(int32_t)));
        r->hscene.tr_rgb = r->tr_rgb;
        r->hscene.tr_spp = r->tr_spp;
        r->hscene.tr_calc = 1;
        CK(hipMemcpy(r->dscene, &r->hscene, sizeof(DScene), hipMemcpyHostToDevice));
    }
    // guideTraining (guidedvolpathvspgintegrator.cpp:109).  The reference also trains when only the guided-RR
    // flags are set (they default to true); this build trains iff the field will be queried.
    if (wants_guiding(r->prm)) {
        r->training = wants_training(r->prm);
        r->field_set = true;
        for (int f = 0; f < 2; ++f) {
            CK(hipMalloc(&r->fnodes[f], sizeof(VspgKdNode) * kTrainCapNodes));
            CK(hipMemset(r->fnodes[f], 0, sizeof(VspgKdNode) * kTrainCapNodes));
            CK(hipMalloc(&r->fregions[f], sizeof(VspgFieldRegion) * kTrainCapRegions));
            CK(hipMemset(r->fregions[f], 0, sizeof(VspgFieldRegion) * kTrainCapRegions));
            CK(hipMalloc(&r->rstats[f], sizeof(RegionStats) * kTrainCapRegions));
            CK(hipMemset(r->rstats[f], 0, sizeof(RegionStats) * kTrainCapRegions));
            const VspgKdNode root = {0.f, 3u};  // one leaf -> region 0, untrained (n_lobes 0)
            CK(hipMemcpy(r->fnodes[f], &root, sizeof root, hipMemcpyHostToDevice));
            CK(hipMalloc(&r->faux[f], sizeof(float) * 2 * GK * kTrainCapRegions));
            CK(hipMemset(r->faux[f], 0, sizeof(float) * 2 * GK * kTrainCapRegions));
            CK(hipMalloc(&r->flobes[f], sizeof(float4) * kRegionLobeQuads * kTrainCapRegions));
            CK(hipMemset(r->flobes[f], 0, sizeof(float4) * kRegionLobeQuads * kTrainCapRegions));
            r->hscene.field[f] = DField{1, 1, r->fnodes[f], r->fregions[f], r->faux[f], r->flobes[f]};
        }
        CK(hipMemcpy(r->dscene, &r->hscene, sizeof(DScene), hipMemcpyHostToDevice));
    }
    // segment records, radiance samples and the update's scratch exist only for a renderer that trains (an
    // rrguiding-only renderer queries nothing and records nothing)
    if (r->training) {
        r->segbuf_items = (size_t)((cfg->xres + 7) / 8) * (size_t)((cfg->yres + 7) / 8) * 64;  // the work items of a 1-spp wave
        CK(hipMalloc(&r->segbuf, r->segbuf_items * (size_t)train_rec_capacity(r->prm.maxdepth) * SG_FLOATS * sizeof(float)));
        CK(hipMalloc(&r->seg_count, r->segbuf_items * sizeof(int)));
        r->sample_capacity = (unsigned long long)r->npix * (unsigned long long)(r->prm.maxdepth + 1);
        if (r->sample_capacity > (1ull << 26)) r->sample_capacity = 1ull << 26;
        CK(hipMalloc(&r->samples, r->sample_capacity * sizeof(VspgTrainSample)));
        CK(hipMalloc(&r->train_counters, 4 * sizeof(unsigned long long)));
        CK(hipMemset(r->train_counters, 0, 4 * sizeof(unsigned long long)));
        CK(hipMalloc(&r->train_acc, (size_t)kTrainKeys * kStatFloats * sizeof(float)));
        CK(hipMalloc(&r->train_sumw, 2 * sizeof(float)));
        CK(hipMalloc(&r->train_reg, r->sample_capacity * sizeof(int)));
        CK(hipMalloc(&r->train_order, r->sample_capacity * sizeof(unsigned int)));
        CK(hipMalloc(&r->train_hist, (size_t)kTrainKeys * sizeof(unsigned int)));
        CK(hipMalloc(&r->train_cursor, (size_t)kTrainKeys * sizeof(unsigned int)));
        CK(hipMalloc(&r->train_nsplit, 2 * sizeof(int)));
        CK(hipMalloc(&r->train_nsorted, sizeof(unsigned int)));
    }
#undef CK
    *out = r;
    return 0;
}

int vspg_renderer_destroy(VspgRenderer *r) {
    if (!r) return 0;
    (void)hipSetDevice(r->cfg.device);
    if (r->dscene) (void)hipFree(r->dscene);
    if (r->film) (void)hipFree(r->film);
    if (r->isg_stats) (void)hipFree(r->isg_stats);
    if (r->contrib) (void)hipFree(r->contrib);
    if (r->tr_rgb) (void)hipFree(r->tr_rgb);
    if (r->tr_spp) (void)hipFree(r->tr_spp);
    if (r->vsp) (void)hipFree(r->vsp);
    if (r->counters) (void)hipFree(r->counters);
    if (r->work_head) (void)hipFree(r->work_head);
    if (r->work_head8_raw) (void)hipFree(r->work_head8_raw);
    for (int f = 0; f < 2; ++f) {
        if (r->fnodes[f]) (void)hipFree(r->fnodes[f]);
        if (r->fregions[f]) (void)hipFree(r->fregions[f]);
        if (r->faux[f]) (void)hipFree(r->faux[f]);
        if (r->flobes[f]) (void)hipFree(r->flobes[f]);
    }
    for (int f = 0; f < 2; ++f)
        if (r->rstats[f]) (void)hipFree(r->rstats[f]);
    if (r->segbuf) (void)hipFree(r->segbuf);
    if (r->seg_count) (void)hipFree(r->seg_count);
    if (r->samples) (void)hipFree(r->samples);
    if (r->train_counters) (void)hipFree(r->train_counters);
    if (r->train_acc) (void)hipFree(r->train_acc);
    if (r->train_sumw) (void)hipFree(r->train_sumw);
    if (r->train_reg) (void)hipFree(r->train_reg);
    if (r->train_order) (void)hipFree(r->train_order);
    if (r->train_hist) (void)hipFree(r->train_hist);
    if (r->train_cursor) (void)hipFree(r->train_cursor);
    if (r->train_nsorted) (void)hipFree(r->train_nsorted);
    if (r->train_nsplit) (void)hipFree(r->train_nsplit);
    for (int k = 0; k < VSPG_MAX_TEXTURES; ++k) if (r->tex_buf[k]) (void)hipFree(r->tex_buf[k]);
    if (r->tri_uv) (void)hipFree(r->tri_uv);
    if (r->tris) (void)hipFree(r->tris);
    if (r->bvh) (void)hipFree(r->bvh);
    for (int k = 0; k < 2; ++k) if (r->wave_samples[k]) (void)hipFree(r->wave_samples[k]);
    if (r->ws_event) (void)hipEventDestroy(r->ws_event);
    for (int k = 0; k < 2; ++k) if (r->carry_img[k]) (void)hipFree(r->carry_img[k]);  // (paths still in flight end with their renderer)
    if (r->wf_pool) (void)hipFree(r->wf_pool);
    if (r->wf_lists) (void)hipFree(r->wf_lists);
    if (r->wf_iters) (void)hipFree(r->wf_iters);
    if (r->wf_ev_vertex) (void)hipEventDestroy(r->wf_ev_vertex);
    if (r->wf_ev_shadow) (void)hipEventDestroy(r->wf_ev_shadow);
    if (r->wf_stream2) (void)hipStreamDestroy(r->wf_stream2);
    if (r->density) (void)hipFree(r->density);
    if (r->brick_index) (void)hipFree(r->brick_index);
    if (r->octets) (void)hipFree(r->octets);
    if (r->le_scale) (void)hipFree(r->le_scale);
    if (r->temperature) (void)hipFree(r->temperature);
    if (r->majorant) (void)hipFree(r->majorant);
    for (int k = 0; k < 2; ++k) if (r->rgb_oct[k]) (void)hipFree(r->rgb_oct[k]);
    if (r->rgb_Le) (void)hipFree(r->rgb_Le);
    for (int k = 0; k < VSPG_MAX_INFINITE_LIGHTS; ++k) if (r->env_buf[k]) (void)hipFree(r->env_buf[k]);
    for (int k = 0; k < VSPG_MAX_POINT_LIGHTS; ++k) if (r->light_img_buf[k]) (void)hipFree(r->light_img_buf[k]);
    if (r->fe_ref) (void)hipFree(r->fe_ref);
    if (r->fe_partials) (void)hipFree(r->fe_partials);
    if (r->fe_log) (void)hipFree(r->fe_log);
    if (r->fe_event) (void)hipEventDestroy(r->fe_event);
    if (r->rs_stage) (void)hipFree(r->rs_stage);
    if (r->rs_clamped) (void)hipFree(r->rs_clamped);
    delete r;
    return 0;
}

// Which path kernel serves a renderer: choose_kernel (vspg_kernel_choice.h) decides from these facts and the process environment, afresh at
// every entry point; what a renderer reports and what it launches come from that one record.  Nothing else reads the renderer for it.
static ChoiceFacts choice_facts(const VspgRenderer *r) {
    ChoiceFacts f;
    f.medium_type = r->scene.medium.type;
    f.n_tris = r->hscene.n_tris, f.n_inf = r->hscene.n_inf, f.n_spheres = r->hscene.n_spheres;
    f.n_point = r->hscene.n_point;
    f.n_textured = r->n_textured;
    f.has_boundaries = r->hscene.has_boundaries != 0;
    f.lightsampler = r->hscene.lsamp.mode;
    f.medium_grey = r->medium_grey, f.surfaces_grey = r->surfaces_grey && r->n_textured == 0, f.null_zero = r->null_zero;
    f.guided = wants_guiding(r->prm), f.rrguiding = r->prm.rrguiding != 0, f.training = r->training;
    f.tr_calc = r->hscene.tr_calc != 0, f.has_temperature = r->hscene.temperature != nullptr;
    f.resampling = r->prm.vspsamplingmethod == VSPG_VSP_RESAMPLING;
    f.camera_general = camera_model_general(VspgCameraModel{r->hscene.cam_model, r->hscene.cam_lens_radius, r->hscene.cam_focal_distance});
    return f;
}
// The samples a one-sample wg2 launch parked are resolved by the next such launch; anything else that reads or writes the film or
// the image-space statistics calls this first (VSPG_WG2_DEFER=0: every launch resolves its own samples at once).
static bool wg2_defer_enabled() {  // (read per launch: a test flips it)
    const char *e = getenv("VSPG_WG2_DEFER");
    return !(e && e[0] == '0');
}
// (the parking launch ran on ws_stream; work on any other stream that reads its samples is ordered behind it by ws_event)
static int order_after_parking(VspgRenderer *r, hipStream_t s) {
    if (r->ws_parked && r->ws_event && s != r->ws_stream) HIPCHK(hipStreamWaitEvent(s, r->ws_event, 0));
    return 0;
}
// One-sample launches of k_render_wave_wg3 carry their in-flight paths into the next launch (VSPG_WG3_CARRY=0: every launch drains
// its own, today's kernel; so does VSPG_WG2_DEFER=0 -- nothing is carried where nothing is parked).
static bool wg3_carry_enabled() {  // (read per launch: a test flips it)
    const char *e = getenv("VSPG_WG3_CARRY");
    return !(e && e[0] == '0') && wg2_defer_enabled();
}
static int wg3_launch_any(int arith, const Wg3Launch &L) {
    return arith == VSPG_ARITH_FAST_WEIGHTS ? vspg_arith1_wg3(&L) : arith == VSPG_ARITH_FAST ? vspg_arith2_wg3(&L) : wg3_launch_exact(L);
}
// The drain: the pending image's paths run to their ends in a launch of the shape that suspended them -- no tiles, nothing suspended.
// Each parks its sample over its pixel's sentinel: behind it the renderer is where a self-contained launch would have left it.
static int drain_carried_paths(VspgRenderer *r, hipStream_t s) {
    if (!r->carry_pending) return 0;
    if (const int rc = order_after_parking(r, s)) return rc;
    Wg3Launch L = r->carry_shape;
    L.vsp_ready = r->vsp_ready;
    L.first_sample = -1;  // (no path of this launch: every resumed one is an old one)
    L.work_head = r->work_head8 + (r->head8_parity & 1u) * (unsigned)(kWg3HeadSetBytes / 4);  // (claims nothing; the next launch's set stays zero)
    L.ws_prev = nullptr;
    L.ws_out = r->wave_samples[r->ws_cur ^ 1];
    L.stream = s;
    L.carry = 1;
    L.resume = r->carry_img[r->carry_cur ^ 1];
    L.suspend = nullptr;
    const int lrc = wg3_launch_any(r->carry_arith, L);
    if (lrc != 0) return fail(VSPG_EHIP, std::string("k_render_wave_wg3_carry (drain): ") + hipGetErrorName((hipError_t)lrc));
    r->carry_pending = false;
    // (the parked plane is complete behind THIS launch now: whoever touches it on another stream waits on it)
    r->ws_stream = s;
    if (r->ws_event) HIPCHK(hipEventRecord(r->ws_event, s));
    return 0;
}
static int flush_parked_samples(VspgRenderer *r, hipStream_t s) {
    if (const int rc = drain_carried_paths(r, s)) return rc;
    if (!r->ws_parked) return 0;
    if (const int rc = order_after_parking(r, s)) return rc;
    const size_t n_win = (size_t)(r->ws_win.x1 - r->ws_win.x0) * (size_t)(r->ws_win.y1 - r->ws_win.y0);
    hipLaunchKernelGGL(k_film_resolve, dim3((unsigned)((n_win + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, r->cfg.xres, r->ws_win,
                       r->wave_samples[r->ws_cur ^ 1], r->film, r->isg_stats);
    HIPCHK(hipGetLastError());
    r->ws_parked = false;
    return 0;
}
const char *vspg_renderer_kernel_name(VspgRenderer *r) {
    if (!r) return "";
    // (the tolerance modes: the inline namespace of vspg_fast.hip's symbols)
    r->kernel_name_buf = std::string(r->arith == VSPG_ARITH_EXACT ? "" : r->arith == VSPG_ARITH_FAST_WEIGHTS ? "fastw::" : "fast::") +
                         kernel_name(choose_kernel(choice_facts(r), read_choice_env()));
    return r->kernel_name_buf.c_str();
}
// Which instantiations a renderer's path kernels are launched from (vspg_arith.h).  The tolerance modes exist for the unguided
// rectangle-scene workgroup kernel and the unguided resampling pipeline over GridMedium; anything else is refused by name.
int vspg_renderer_set_arithmetic(VspgRenderer *r, int mode) {
    if (!r) return fail(VSPG_EINVAL, "null renderer");
    if (mode != VSPG_ARITH_EXACT && mode != VSPG_ARITH_FAST_WEIGHTS && mode != VSPG_ARITH_FAST) return fail(VSPG_EINVAL, "unknown arithmetic mode");
    const KernelChoice c = choose_kernel(choice_facts(r), read_choice_env());
    if (mode != VSPG_ARITH_EXACT && !c.arith_covered)
        return fail(VSPG_ESCOPE, "the tolerance-mode instantiations cover unguided renders of rectangle scenes over a homogeneous medium and unguided "
                                 "\"resampling\" renders over a uniformgrid medium (this renderer runs " + kernel_name(c) + ")");
    if (mode != r->arith && r->carry_pending) {  // (paths in flight end in the arithmetic they started in)
        HIPCHK(hipSetDevice(r->cfg.device));
        if (const int rc = drain_carried_paths(r, r->ws_stream)) return rc;
    }
    r->arith = mode;
    return 0;
}
int vspg_renderer_get_arithmetic(VspgRenderer *r) { return r ? r->arith : VSPG_EINVAL; }

int vspg_render_wave(VspgRenderer *r, int wave_start, int wave_end, void *stream) {
    const RoctxRange range("vspg_render_wave");  // (around the window call's own range: traces keep the name they filter on)
    if (!r) return fail(VSPG_EINVAL, "null renderer");
    return vspg_render_window(r, 0, 0, r->cfg.xres, r->cfg.yres, wave_start, wave_end, stream);
}

// The window's tiles are those of the frame's 8x8 grid that touch it (PixelWindow, vspg_device.h): everything a launch sizes -- blocks,
// static shares, tile cursors, the pipeline's lists, the training columns -- follows `items`, the pixels of those tiles.
int vspg_render_window(VspgRenderer *r, int x0, int y0, int x1, int y1, int wave_start, int wave_end, void *stream) {
    const RoctxRange range("vspg_render_window");
    if (!r) return fail(VSPG_EINVAL, "null renderer");
    if (x0 < 0 || y0 < 0 || x1 <= x0 || y1 <= y0 || x1 > r->cfg.xres || y1 > r->cfg.yres)
        return fail(VSPG_EINVAL, "pixel window [" + std::to_string(x0) + "," + std::to_string(x1) + ") x [" + std::to_string(y0) + "," + std::to_string(y1) +
                                     ") is empty or not inside the " + std::to_string(r->cfg.xres) + " x " + std::to_string(r->cfg.yres) + " film");
    if (wave_end < wave_start || wave_start < 0) return fail(VSPG_EINVAL, "bad wave range");
    if (wave_end == wave_start) return 0;
    const KernelChoice c = choose_kernel(choice_facts(r), read_choice_env());  // what this call launches, decided once
    HIPCHK(hipSetDevice(r->cfg.device));
    const PixelWindow win = {x0, y0, x1, y1};
    const bool whole = x0 == 0 && y0 == 0 && x1 == r->cfg.xres && y1 == r->cfg.yres;
    const int tilesX = win_tiles_x(win), tilesY = win_tiles_y(win);
    const long long items = (long long)tilesX * tilesY * 64;
    // persistent grid: exactly the resident wavefronts (never more blocks than tiles of work)
    long long blocks = (long long)r->num_cus * kBlocksPerCU;
    const long long max_blocks = (items + kBlock - 1) / kBlock;
    if (blocks > max_blocks) blocks = max_blocks;
    const long long n_waves = blocks * (kBlock / 64);
    // static slice per wavefront: 3/4 of the fair share, whole tiles
    // (VSPG_LANE_STATIC: the static share in 64ths, default 48 = 3/4)
    static const int lane_static64 = [] { const char *e = getenv("VSPG_LANE_STATIC"); const int v = e ? atoi(e) : 48; return v < 0 ? 0 : (v > 64 ? 64 : v); }();
    const unsigned static_per_wave = (unsigned)((items * lane_static64 / 64 / n_waves) / 64 * 64);
    const unsigned dyn_base = (unsigned)(static_per_wave * n_waves);
    // first sample index of this shard in the range, and how many it has
    const int sc = r->cfg.shard_count, si = r->cfg.shard_index;
    int first = wave_start;
    if (sc > 1) first += ((si - wave_start % sc) % sc + sc) % sc;
    if (first >= wave_end) return 0;  // nothing for this shard in the range
    const int n_samples = (wave_end - 1 - first) / sc + 1;
    const PcgJump jump = pcg_jump((unsigned long long)first * 65536ull);
    const int single = n_samples == 1 ? 1 : 0;
    const bool wf = c.family == Family::WfWalk || c.family == Family::WfSegmentVertex;
    const bool parks = c.family == Family::Wg2 || c.family == Family::Wg3;  // (a launch of these parks its samples, below)
    if (c.guided && !r->field_set) return fail(VSPG_ESCOPE, "guiding enabled but the renderer holds no guiding field");
    // a one-sample launch of k_render_wave_wg2 resolves the samples its predecessor parked; every other launch adds to the film
    // itself, so the parked samples go in first
    // (a launch resolves parked samples pixel by pixel as it starts them: those of ANOTHER window go in through k_film_resolve first)
    const bool defer = parks && single && wg2_defer_enabled();
    const bool same_win = r->ws_win.x0 == x0 && r->ws_win.y0 == y0 && r->ws_win.x1 == x1 && r->ws_win.y1 == y1;
    if (!defer || !same_win) { const int rc = flush_parked_samples(r, (hipStream_t)stream); if (rc) return rc; }
    // ... and a k_render_wave_wg3 launch of that kind also takes over the paths its predecessor left in flight (below); any other drains them
    // (not where the paths themselves keep a per-pixel running mean, the TrBuffer's: two samples of a pixel would be in flight at once)
    const bool carry = defer && c.family == Family::Wg3 && !r->hscene.tr_calc && wg3_carry_enabled();
    if (r->carry_pending && !carry) { const int rc = drain_carried_paths(r, (hipStream_t)stream); if (rc) return rc; }
    if (wf) {  // one pass per sample index of this shard, in order
#ifdef VSPG_WF_DEBUG
        auto checksum = [&](const void *dptr, size_t bytes) -> unsigned long long {
            if (!dptr || !bytes) return 0ull;
            std::vector<unsigned char> h(bytes);
            (void)hipDeviceSynchronize();
            (void)hipMemcpy(h.data(), dptr, bytes, hipMemcpyDeviceToHost);
            unsigned long long x = 1469598103934665603ull;
            for (size_t i = 0; i < bytes; ++i) { x ^= h[i]; x *= 1099511628211ull; }
            return x;
        };
        const size_t nb = (size_t)r->hscene.bnx * r->hscene.bny * r->hscene.bnz;
        const void *bufs[6] = {r->tris, r->bvh, r->brick_index, r->octets, r->dscene, r->majorant};
        const size_t sizes[6] = {(size_t)r->hscene.n_tris * sizeof(DTri), (size_t)r->hscene.n_bvh_nodes * sizeof(DBvh4Node), nb * 4, r->n_bricks * 512 * 32,
                                 sizeof(DScene), (size_t)16 * 16 * 16 * 4};
        unsigned long long before[6];
        for (int k = 0; k < 6; ++k) before[k] = checksum(bufs[k], sizes[k]);
#endif
        for (int w = first; w < wave_end; w += sc > 1 ? sc : 1) {
            const int rc = wf_render_pass(r, c, win, w, (hipStream_t)stream);
            if (rc) return rc;
        }
#ifdef VSPG_WF_DEBUG
        {
            const char *names[6] = {"tris", "bvh", "brick_index", "octets", "dscene", "majorant"};
            for (int k = 0; k < 6; ++k)
                if (checksum(bufs[k], sizes[k]) != before[k]) fprintf(stderr, "VSPG_WF_DEBUG: the pipeline changed %s (%zu bytes at %p)\n", names[k], sizes[k], bufs[k]);
            fprintf(stderr, "VSPG_WF_DEBUG: pool %p..%p lists %p film %p isg %p tris %p bvh %p\n", (void *)r->wf_pool,
                    (void *)((char *)r->wf_pool + (size_t)kWfPoolFloats * r->wf_items * 4), (void *)r->wf_lists, (void *)r->film, (void *)r->isg_stats, (void *)r->tris, (void *)r->bvh);
        }
#endif
        return 0;
    }
    // a18: while the field trains, the guided kernels record path segments and emit radiance samples
    const bool train = c.train;
    TrainArgs targs = {nullptr, nullptr, nullptr, nullptr, 0, 0};
    if (train) {
        if (n_samples > 1) {  // a training launch covers one sample per pixel (the record buffer is sized for that): split
            for (int w = first; w < wave_end; w += sc > 1 ? sc : 1) {
                const int rc = vspg_render_window(r, x0, y0, x1, y1, w, w + 1, stream);
                if (rc) return rc;
            }
            return 0;
        }
        targs = TrainArgs{r->segbuf, r->seg_count, r->samples, r->train_counters, r->sample_capacity, (unsigned)items};
        HIPCHK(hipMemsetAsync(r->seg_count, 0, (size_t)items * sizeof(int), (hipStream_t)stream));
    }
    // exactly one path-kernel launch follows: it uses the counter the previous launch zeroed and zeroes the other one
    unsigned int *const work_head = r->work_head + (r->head_parity & 1u);
    r->head_parity ^= 1u;
    // the workgroup kernels' grid (k_render_wave_wg / _wg2 / _wg3)
    const unsigned tiles_magic = tilesX > 1 ? (unsigned)((0x100000000ull + (unsigned)tilesX - 1) / (unsigned)tilesX) : 0u;
    const bool wgrid = c.medium == MediumInst::Grid;
    const int wwaves = c.wg_guided ? kWgWavesGuided : wgrid ? kWgWavesGrid : kWgWavesHomog, wblock = c.wg_guided ? kWgBlockGuided : wgrid ? kWgBlockGrid : kWgBlockHomog;
    long long wblocks = (long long)r->num_cus * (wwaves * 4 / (wblock / 64));
    const long long wmax = (items + kWgChunk - 1) / kWgChunk;
    if (wblocks > wmax) wblocks = wmax;
    // Two schedulers park their samples (k_render_wave_wg2: tiles from a global head, two barriers; k_render_wave_wg3: barrier-free):
    // a launch writes its samples to ws_out and resolves those its predecessor left in ws_prev
    float4 *ws_out = nullptr;
    const float4 *ws_prev = nullptr;
    const int wg3_grey = r->medium_grey ? (r->surfaces_grey ? 2 : 1) : 0, wg3_null_zero = r->medium_grey && r->surfaces_grey && r->null_zero ? 1 : 0;
    if (parks) {
        for (int k = 0; k < 2; ++k)
            if (!r->wave_samples[k]) HIPCHK(hipMalloc(&r->wave_samples[k], r->npix * sizeof(float4)));
        const long long n_tiles = (long long)tilesX * tilesY;
        if (wblocks > n_tiles) wblocks = n_tiles;
        // CARRY (vspg_wg3.h): the pending image is resumed by a launch of the shape that wrote it, whose sample index differs from
        // the suspended paths' (that is how the kernel tells them apart); otherwise it is drained first
        if (r->carry_pending) {
            const Wg3Launch &P = r->carry_shape;
            const bool same_shape = carry && P.grey == wg3_grey && P.null_zero == wg3_null_zero && P.blocks == (unsigned)wblocks && P.windowed == (whole ? 0 : 1) &&
                                    r->carry_arith == r->arith && P.first_sample != first && P.dscene == r->dscene;
            if (!same_shape) { const int rc = drain_carried_paths(r, (hipStream_t)stream); if (rc) return rc; }
        }
        ws_out = r->wave_samples[r->ws_cur];
        ws_prev = defer && r->ws_parked ? r->wave_samples[r->ws_cur ^ 1] : nullptr;
        if (ws_prev) { const int rc = order_after_parking(r, (hipStream_t)stream); if (rc) return rc; }
    }
    using NullZero = HomogeneousMediumGreySceneNullZero;
    const auto not_built = [&] { return fail(VSPG_ESCOPE, "internal: no instantiation " + kernel_name(c) + " is built"); };
    switch (c.family) {
    case Family::Lane: {
        const auto launch = [&](auto inst) {
            using I = decltype(inst);
            hipLaunchKernelGGL((k_render_wave<typename I::Medium, I::guided, I::train>), dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, r->dscene,
                               r->film, r->isg_stats, r->vsp, r->vsp_ready, wave_start, wave_end, first, single, jump, static_per_wave, dyn_base, work_head,
                               r->counters, targs, win);
        };
        // (a medium's unguided, guided and guided + training builds)
        const auto launch_guided_or_not = [&](auto inst) {
            using M = typename decltype(inst)::Medium;
            if (c.train) launch(KernelInst<M, true, true>{});
            else if (c.guided) launch(KernelInst<M, true>{});
            else launch(KernelInst<M>{});
        };
        switch (c.medium) {
        case MediumInst::NanoDense: launch_guided_or_not(KernelInst<NanoDenseMedium>{}); break;
        case MediumInst::Grid: launch_guided_or_not(KernelInst<GridMedium>{}); break;
        case MediumInst::GridGrey: launch(KernelInst<GridMediumGrey>{}); break;
        case MediumInst::RgbGrid: launch_guided_or_not(KernelInst<RgbGridMedium>{}); break;
        case MediumInst::Homogeneous: launch_guided_or_not(KernelInst<HomogeneousMedium>{}); break;
        case MediumInst::HomogeneousGreySceneNullZero:  // (guided renders only)
            if (c.train) launch(KernelInst<NullZero, true, true>{});
            else launch(KernelInst<NullZero, true>{});
            break;
        default: return not_built();
        }
        break;
    }
    case Family::Wg: {  // (film flush between the phases, three barriers: grid media under VSPG_KERNEL=wg, and VSPG_WG_SCHED=1)
        const auto launch = [&](auto inst) {
            using I = decltype(inst);
            hipLaunchKernelGGL((k_render_wave_wg<typename I::Medium, false, I::pool, I::block, I::waves>), dim3((unsigned)wblocks), dim3(I::block), 0,
                               (hipStream_t)stream, r->dscene, r->film, r->isg_stats, r->vsp, r->vsp_ready, wave_end, first, single, jump, tiles_magic, work_head,
                               r->counters, win);
        };
        switch (c.medium) {
        case MediumInst::Grid: launch(KernelInst<GridMedium, false, false, kWgPoolGrid, kWgBlockGrid, kWgWavesGrid>{}); break;
        case MediumInst::HomogeneousGreySceneNullZero: launch(WgHomogInst<NullZero, kWgPoolHomogT<2>>{}); break;
        case MediumInst::HomogeneousGreyScene: launch(WgHomogInst<HomogeneousMediumGreyScene, kWgPoolHomogT<2>>{}); break;
        case MediumInst::HomogeneousGrey: launch(WgHomogInst<HomogeneousMediumGrey, kWgPoolHomogT<1>>{}); break;
        case MediumInst::HomogeneousSimple: launch(WgHomogInst<HomogeneousMediumSimple, kWgPoolHomogT<0>>{}); break;
        default: return not_built();
        }
        break;
    }
    case Family::Wg2: {
        // the share of the frame handed out from the global head, in 64ths (VSPG_WG2_TAIL; the rest is dealt to the workgroups
        // up front, interleaved).  Measured on the reference-default guided workload / the unguided one (ms per 1080p wave):
        // 0: 1.59 / 0.887, 8: 1.50 / 0.829, 16: 1.46 / 0.800, 32: 1.47 / 0.790, 64 (all of it): 1.454 / 0.775.
        const int tail64 = [] { const char *e = getenv("VSPG_WG2_TAIL"); const int v = e ? atoi(e) : 64; return v < 0 ? 0 : (v > 64 ? 64 : v); }();  // (per launch: a test varies it)
        const unsigned static_tiles = (unsigned)(((long long)tilesX * tilesY * (64 - tail64) / 64) / wblocks * wblocks);
        const auto launch = [&](auto inst) {
            using I = decltype(inst);
            hipLaunchKernelGGL((k_render_wave_wg2<typename I::Medium, I::guided, I::pool, I::block, I::waves, I::train>), dim3((unsigned)wblocks), dim3(I::block), 0,
                               (hipStream_t)stream, r->dscene, r->film, r->isg_stats, r->vsp, r->vsp_ready, wave_end, first, single, jump, tiles_magic, static_tiles,
                               work_head, ws_prev, ws_out, r->counters, targs, win);
        };
        switch (c.medium) {
        case MediumInst::HomogeneousGreySceneNullZero:
            if (c.train) launch(WgGuidedInst<NullZero, kWg2PoolTrainT<2>, true>{});
            else if (c.guided) launch(WgGuidedInst<NullZero, kWg2PoolGuidedT<2>>{});
            else launch(WgHomogInst<NullZero, kWg2PoolHomogT<2>>{});
            break;
        case MediumInst::HomogeneousSimple:
            if (c.train) launch(WgGuidedInst<HomogeneousMediumSimple, kWg2PoolTrainT<0>, true>{});
            else if (c.guided) launch(WgGuidedInst<HomogeneousMediumSimple, kWg2PoolGuidedT<0>>{});
            else launch(WgHomogInst<HomogeneousMediumSimple, kWg2PoolHomogT<0>>{});
            break;
        case MediumInst::HomogeneousGreyScene: launch(WgHomogInst<HomogeneousMediumGreyScene, kWg2PoolHomogT<2>>{}); break;
        case MediumInst::HomogeneousGrey: launch(WgHomogInst<HomogeneousMediumGrey, kWg2PoolHomogT<1>>{}); break;
        case MediumInst::Homogeneous: launch(WgHomogInst<HomogeneousMedium, kWg2PoolFull>{}); break;  // (the full-scene instantiation)
        default: return not_built();
        }
        break;
    }
    case Family::Wg3: {  // the unguided rectangle-scene instantiations (the headline workload): also built in the tolerance modes
        static_assert(kWgBlockHomog == VSPG_WG_BLOCK && kWgWavesHomog == VSPG_WG_WAVES, "wg3_launch_unguided's launch shape");
        // (its tile cursors: a pair of sets of its own, alternating like the counter pair of the other kernels -- which this launch leaves alone)
        unsigned int *const head8 = r->work_head8 + (r->head8_parity & 1u) * (unsigned)(kWg3HeadSetBytes / 4);
        r->head8_parity ^= 1u;
        r->head_parity ^= 1u;  // (undo the toggle above: no launch used that pair)
        Wg3Launch L3{r->dscene, r->film, r->isg_stats, r->vsp, r->vsp_ready, wave_end, first, single, jump, tiles_magic, head8, ws_prev, ws_out,
                     r->counters, (unsigned)wblocks, (hipStream_t)stream, wg3_grey, wg3_null_zero, whole ? 0 : 1, win, 0, nullptr, nullptr};
        bool update_follows = false;
        if (carry) {
            // (an image per workgroup of the largest grid a launch of this renderer can have, at the largest instantiation's size)
            const size_t img_bytes = (size_t)r->num_cus * (size_t)(kWgWavesHomog * 4 / (kWgBlockHomog / 64)) * (size_t)kWg3ImageStrideMax * sizeof(unsigned int);
            for (int k = 0; k < 2; ++k)
                if (!r->carry_img[k]) HIPCHK(hipMalloc(&r->carry_img[k], img_bytes));
            static_assert(kWg3ImageStrideMax % 4 == 0, "images are copied in 16-byte pieces");
            if ((reinterpret_cast<uintptr_t>(r->carry_img[0]) | reinterpret_cast<uintptr_t>(r->carry_img[1])) & 15u)
                return fail(VSPG_EHIP, "k_render_wave_wg3_carry: image buffers are not 16-byte aligned");
            L3.carry = 1;
            L3.resume = r->carry_pending ? r->carry_img[r->carry_cur ^ 1] : nullptr;
            // A step that ends in an update of the VSP buffer flushes the parked samples, and with them the carried paths: the launch of
            // such a step suspends nothing (it resumes, takes its tiles and runs every path to its end), which saves the images, the
            // drain launch and the empty chip between the two.  The step is the caller's: one wave, or shard_count of them under
            // sample-index sharding (sharding.py).  Predicted only for a caller that post-processed its previous step: one that never does
            // (wave counter 0, an update "due" for ever) keeps carrying.  Only a hint: a wrong guess either way leaves a state the drain
            // path handles as ever.
            // (VSPG_WG3_PREDICT=0: every carried launch suspends and the flush drains, for A/B runs and tests; read per launch)
            const char *const pe = getenv("VSPG_WG3_PREDICT");
            update_follows = !(pe && pe[0] == '0') && r->step_post_processed && vspg_isg_update_due(r, sc > 1 ? sc : 1) != 0;
            L3.suspend = update_follows ? nullptr : r->carry_img[r->carry_cur];
        }
        const int lrc = wg3_launch_any(r->arith, L3);  // (wg3_launch_unguided picks the grey / null-zero instantiation, vspg_wg3.h)
        if (lrc != 0) return fail(VSPG_EHIP, std::string("k_render_wave_wg3: ") + hipGetErrorName((hipError_t)lrc));
        if (carry) {
            if (r->carry_pending) r->carry_resumes++;
            r->carry_pending = !update_follows;  // (nothing suspended: the parked plane is complete behind this launch)
            if (update_follows) r->carry_kept++;
            if (r->carry_pending) {
                r->carry_cur ^= 1;
                r->carry_shape = L3;
                r->carry_arith = r->arith;
            }
        }
        break;
    }
    default: return not_built();
    }
    HIPCHK(hipGetLastError());
    r->step_post_processed = false;
    if (parks && single) {  // this launch's samples are parked in ws_out (its predecessor's, if any were, have just been resolved)
        r->ws_cur ^= 1;
        r->ws_parked = true;
        r->ws_win = win;
        r->ws_stream = (hipStream_t)stream;
        if (!r->ws_event) HIPCHK(hipEventCreateWithFlags(&r->ws_event, hipEventDisableTiming));
        HIPCHK(hipEventRecord(r->ws_event, (hipStream_t)stream));
        if (!defer) { const int rc = flush_parked_samples(r, (hipStream_t)stream); if (rc) return rc; }
    }
    if (train) {
        hipLaunchKernelGGL(k_propagate, dim3((unsigned)((items + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream, targs,
                           train_rec_capacity(r->prm.maxdepth));
        HIPCHK(hipGetLastError());
    }
    return 0;
}

// Field::Update (:239) on device; one host read of the sample count per training wave decides whether the
// update runs (more than 128 valid samples, :238) and sizes the grids.
static int train_update(VspgRenderer *r, hipStream_t s) {
    unsigned long long cnt[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(cnt, r->train_counters, sizeof cnt, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const unsigned long long n = cnt[0] < r->sample_capacity ? cnt[0] : r->sample_capacity;
    // sharded training: `xchg` sums a device buffer over the ranks (no-op without a hook); the decision to update is taken
    // on the SUMMED sample count, so every rank takes it alike and the hook runs the same number of times everywhere
    const auto xchg = [&](float *p, size_t nf) -> int {
        if (!r->exchange) return 0;
        const int rc = r->exchange(p, nf, (void *)s, r->exchange_user);
        return rc ? fail(rc, "the exchange hook of the sharded guiding-field update failed") : 0;
    };
    double n_all = (double)n;
    {
        float nf = (float)n;  // train_sumw[1]: the sample count the E-step divides the weight sum by
        HIPCHK(hipMemcpyAsync(r->train_sumw + 1, &nf, sizeof nf, hipMemcpyHostToDevice, s));
        if (r->exchange) {
            if (int rc = xchg(r->train_sumw + 1, 1)) return rc;
            HIPCHK(hipMemcpyAsync(&nf, r->train_sumw + 1, sizeof nf, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            n_all = (double)nf;
        }
    }
    if (n_all > (double)kTrainMinUpdateSamples) {
        const size_t acc_floats = (size_t)kTrainKeys * kStatFloats, acc_bytes = acc_floats * sizeof(float);
        unsigned grid = (unsigned)((n + kBlock - 1) / kBlock);
        if (grid < 1u) grid = 1u;  // (a rank whose own samples ran dry still takes part in the sums)
        if (grid > (unsigned)r->num_cus * 16u) grid = (unsigned)r->num_cus * 16u;
        const unsigned rgrid = (kTrainKeys + kBlock - 1) / kBlock;
        // counting sort: few, long chunks -- every workgroup flushes one atomic per bin its chunk touched
        unsigned sgrid = (unsigned)((n + kSortBlock - 1) / kSortBlock);
        if (sgrid < 1u) sgrid = 1u;
        if (sgrid > (unsigned)r->num_cus) sgrid = (unsigned)r->num_cus;
        // accumulation passes: every wavefront flushes its running sums at least once, so no more wavefronts than fill the chip
        const unsigned agrid = grid < (unsigned)r->num_cus * 4u ? grid : (unsigned)r->num_cus * 4u;
        const TrainFields tf{{r->rstats[0], r->rstats[1]}, {r->fregions[0], r->fregions[1]}, {r->fnodes[0], r->fnodes[1]}};
        const size_t hist_bytes = (size_t)kTrainKeys * sizeof(unsigned int);
        // key_of, order, n_sorted for both fields as the trees stand now; the second sort (redo) only if a tree changed
        auto sort_by_key = [&](float *sumw, const int *redo) -> int {
            HIPCHK(hipMemsetAsync(r->train_hist, 0, hist_bytes, s));
            hipLaunchKernelGGL(k_train_lookup, dim3(sgrid), dim3(kSortBlock), 0, s, r->dscene, r->samples, n, r->train_reg, r->train_hist, sumw, redo);
            hipLaunchKernelGGL(k_train_scan, dim3(1), dim3(kBlock), 0, s, r->train_hist, r->train_cursor, r->train_nsorted, redo);
            hipLaunchKernelGGL(k_train_scatter, dim3(sgrid), dim3(kSortBlock), 0, s, r->train_reg, n, r->train_cursor, r->train_order, redo);
            return 0;
        };
        HIPCHK(hipMemsetAsync(r->train_sumw, 0, sizeof(float), s));
        HIPCHK(hipMemsetAsync(r->train_nsplit, 0, 2 * sizeof(int), s));
        hipLaunchKernelGGL(k_train_decay, dim3(rgrid * 4), dim3(kBlock), 0, s, r->dscene, tf);
        if (int rc = sort_by_key(r->train_sumw, nullptr)) return rc;
        if (int rc = xchg(r->train_sumw, 1)) return rc;
        HIPCHK(hipMemsetAsync(r->train_acc, 0, acc_bytes, s));
        hipLaunchKernelGGL((k_train_pos<true>), dim3(agrid), dim3(kBlock), 0, s, r->samples, r->train_reg, r->train_order, r->train_nsorted,
                           r->train_acc, (const int *)nullptr);
        if (int rc = xchg(r->train_acc, acc_floats)) return rc;
        hipLaunchKernelGGL(k_train_split, dim3(2), dim3(kSplitBlock), 0, s, r->dscene, tf, r->train_acc, r->train_nsplit);
        if (int rc = sort_by_key(nullptr, r->train_nsplit)) return rc;  // the split changed the leaves
        HIPCHK(hipMemsetAsync(r->train_acc, 0, acc_bytes, s));
        hipLaunchKernelGGL((k_train_pos<false>), dim3(agrid), dim3(kBlock), 0, s, r->samples, r->train_reg, r->train_order, r->train_nsorted,
                           r->train_acc, (const int *)(r->train_nsplit + 1));
        if (int rc = xchg(r->train_acc, acc_floats)) return rc;
        hipLaunchKernelGGL(k_train_init_regions, dim3(rgrid), dim3(kBlock), 0, s, r->dscene, tf, r->train_acc);
        HIPCHK(hipMemsetAsync(r->train_acc, 0, acc_bytes, s));
        hipLaunchKernelGGL(k_train_estep, dim3(agrid), dim3(kBlock), 0, s, r->dscene, r->samples, r->train_reg, r->train_order, r->train_nsorted,
                           r->train_sumw, r->train_acc);
        if (int rc = xchg(r->train_acc, acc_floats)) return rc;
        hipLaunchKernelGGL(k_train_mstep, dim3(rgrid), dim3(kBlock), 0, s, r->dscene, tf, r->train_acc);
        for (int f = 0; f < 2; ++f)
            hipLaunchKernelGGL(k_field_aux, dim3((kTrainCapRegions + kBlock - 1) / kBlock * 2), dim3(kBlock), 0, s, r->dscene, f, r->fregions[f],
                               r->faux[f], r->flobes[f]);
        HIPCHK(hipGetLastError());
        r->field_iteration++;
        if (r->field_iteration >= r->prm.guide_num_training_waves) r->training = false;
    }
    return 0;
}

// The image-space buffer update falls on the step that takes the wave counter to (or past) 2^bufferWave; with one
// wave per step this is the reference's `waveCounter == pow(2, bufferWave)` (:251).
static bool isg_update_due(const VspgRenderer *r, int n_waves) {
    return (double)(r->wave_counter + n_waves) >= std::pow(2.0, (double)r->buffer_wave);
}
int vspg_isg_update_due(VspgRenderer *r, int n_waves) {
    if (!r || n_waves < 1) return 0;
    const bool do_vsp = r->prm.vspguiding && r->prm.vspprimaryguiding && !r->vsp_loaded;
    return (do_vsp || r->prm.rrguiding) && isg_update_due(r, n_waves) ? 1 : 0;
}

int vspg_post_process_step(VspgRenderer *r, int n_waves, const float *isg_stats_sum, void *stream) {
    // PostProcessWave (guidedvolpathvspgintegrator.cpp:230-260) after a step that covered n_waves sample indices
    const RoctxRange range("vspg_post_process_step");
    if (!r) return fail(VSPG_EINVAL, "null renderer");
    if (n_waves < 1) return fail(VSPG_EINVAL, "n_waves must be >= 1");
    const bool due = isg_update_due(r, n_waves);
    r->wave_counter += n_waves;
    r->step_post_processed = true;
    if (r->train_counters) {
        HIPCHK(hipSetDevice(r->cfg.device));
        if (r->training) {
            int rc = train_update(r, (hipStream_t)stream);
            if (rc) return rc;
        }
        HIPCHK(hipMemsetAsync(r->train_counters, 0, 4 * sizeof(unsigned long long), (hipStream_t)stream));  // Clear() (:248)
    }
    if (due) {
        const bool do_vsp = r->prm.vspguiding && r->prm.vspprimaryguiding && !r->vsp_loaded;  // calculateImageSpaceGuidingBuffer (:251)
        const bool do_contrib = r->prm.rrguiding != 0;  // cfg.EnableContributionEstimate(guideRR) (:164-168)
        if (do_vsp || do_contrib) {
            HIPCHK(hipSetDevice(r->cfg.device));
            { const int rc = flush_parked_samples(r, (hipStream_t)stream); if (rc) return rc; }  // the statistics of every wave so far
            hipLaunchKernelGGL(k_isg_update, dim3((unsigned)((r->cfg.xres + kIsgTile - 1) / kIsgTile), (unsigned)((r->cfg.yres + kIsgTile - 1) / kIsgTile)),
                               dim3(kBlock), 0, (hipStream_t)stream, r->cfg.xres, r->cfg.yres,
                               r->prm.vspcriterion, isg_stats_sum ? isg_stats_sum : r->isg_stats, do_vsp ? r->vsp : nullptr,
                               do_contrib ? r->contrib : nullptr);
            HIPCHK(hipGetLastError());
            if (do_vsp) r->vsp_ready = 1;
            if (do_contrib && !r->hscene.contrib_ready) {
                r->hscene.contrib_ready = 1;
                HIPCHK(hipMemcpyAsync(reinterpret_cast<char *>(r->dscene) + offsetof(DScene, contrib_ready), &r->hscene.contrib_ready,
                                      sizeof(int32_t), hipMemcpyHostToDevice, (hipStream_t)stream));
            }
        }
        while (std::pow(2.0, (double)r->buffer_wave) <= (double)r->wave_counter) r->buffer_wave++;
    }
    return 0;
}
int vspg_post_process_wave(VspgRenderer *r, void *stream) { return vspg_post_process_step(r, 1, nullptr, stream); }
int vspg_renderer_set_exchange(VspgRenderer *r, VspgExchangeFn fn, void *user) {
    if (!r) return fail(VSPG_EINVAL, "null renderer");
    r->exchange = fn;
    r->exchange_user = user;
    return 0;
}

int vspg_flush(VspgRenderer *r, void *stream) {
    if (!r) return fail(VSPG_EINVAL, "null renderer");
    if (!r->ws_parked) return 0;
    HIPCHK(hipSetDevice(r->cfg.device));
    return flush_parked_samples(r, (hipStream_t)stream);
}
// how many launches of this renderer resumed paths their predecessor left in flight (tests: the carry path was taken)
long long vspg_debug_carry_resumes(VspgRenderer *r) { return r ? (long long)r->carry_resumes : -1; }
// ... and how many suspended nothing because the step's update of the VSP buffer was predicted (tests: the prediction was taken)
long long vspg_debug_carry_kept(VspgRenderer *r) { return r ? (long long)r->carry_kept : -1; }
int vspg_film_device_ptr(VspgRenderer *r, float **dev_ptr, size_t *n_floats) {
    if (!r || !dev_ptr || !n_floats) return fail(VSPG_EINVAL, "null argument");
    if (r->ws_parked) {  // the caller reads the film on a stream of its own: the parked samples go in, and are in, before it gets the pointer
        HIPCHK(hipSetDevice(r->cfg.device));
        const hipStream_t s = r->ws_stream;
        if (const int rc = flush_parked_samples(r, s)) return rc;
        HIPCHK(hipStreamSynchronize(s));
    }
    *dev_ptr = reinterpret_cast<float *>(r->film);
    *n_floats = r->npix * 4;
    return 0;
}
int vspg_film_read(VspgRenderer *r, float *host, void *stream) {
    if (!r || !host) return fail(VSPG_EINVAL, "null argument");
    HIPCHK(hipSetDevice(r->cfg.device));
    if (const int rc = flush_parked_samples(r, (hipStream_t)stream)) return rc;
    HIPCHK(hipMemcpyAsync(host, r->film, r->npix * sizeof(float4), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}
int vspg_film_clear(VspgRenderer *r, void *stream) {
    if (!r) return fail(VSPG_EINVAL, "null renderer");
    HIPCHK(hipSetDevice(r->cfg.device));
    if (const int rc = flush_parked_samples(r, (hipStream_t)stream)) return rc;  // (their statistics stay; the film is cleared after)
    HIPCHK(hipMemsetAsync(r->film, 0, r->npix * sizeof(float4), (hipStream_t)stream));
    return 0;
}
// ---- the film resolved to pixel values (include/vspg.h, vspg_film_resolve.h) ----
int vspg_film_resolve(VspgRenderer *r, int x0, int y0, int x1, int y1, int format, int layout, void *host_out, size_t out_bytes,
                      uint64_t *n_clamped, void *stream) {
    if (!r || !host_out) return fail(VSPG_EINVAL, "null argument");
    if (x0 < 0 || y0 < 0 || x1 <= x0 || y1 <= y0 || x1 > r->cfg.xres || y1 > r->cfg.yres)
        return fail(VSPG_EINVAL, "pixel window [" + std::to_string(x0) + "," + std::to_string(x1) + ") x [" + std::to_string(y0) + "," + std::to_string(y1) +
                                     ") is empty or not inside the " + std::to_string(r->cfg.xres) + " x " + std::to_string(r->cfg.yres) + " film");
    if (format != VSPG_RESOLVE_F32 && format != VSPG_RESOLVE_F16) return fail(VSPG_EINVAL, "vspg_film_resolve: format " + std::to_string(format) + " is neither VSPG_RESOLVE_F32 nor VSPG_RESOLVE_F16");
    if (layout != VSPG_RESOLVE_RGB && layout != VSPG_RESOLVE_SCANLINE_BGR) return fail(VSPG_EINVAL, "vspg_film_resolve: layout " + std::to_string(layout) + " is neither VSPG_RESOLVE_RGB nor VSPG_RESOLVE_SCANLINE_BGR");
    const size_t want = (size_t)(x1 - x0) * (size_t)(y1 - y0) * 3 * (format == VSPG_RESOLVE_F16 ? 2 : 4);
    if (out_bytes != want)
        return fail(VSPG_EINVAL, "vspg_film_resolve: the window's pixels take " + std::to_string(want) + " bytes, out_bytes is " + std::to_string(out_bytes));
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    if (!r->rs_stage) HIPCHK(hipMalloc(&r->rs_stage, r->npix * 3 * sizeof(float)));
    if (!r->rs_clamped) HIPCHK(hipMalloc(&r->rs_clamped, sizeof(unsigned int)));
    if (const int rc = flush_parked_samples(r, s)) return rc;  // (the values are of the complete film)
    const PixelWindow win = {x0, y0, x1, y1};
    unsigned int clamped = 0;
    if (format == VSPG_RESOLVE_F16) {
        hipLaunchKernelGGL(k_film_pixels_zero, dim3(1), dim3(1), 0, s, r->rs_clamped);
        HIPCHK(hipGetLastError());
        film_resolve_launch<unsigned short>(r->cfg.xres, win, layout, r->film, r->rs_stage, r->rs_clamped, s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&clamped, r->rs_clamped, sizeof(clamped), hipMemcpyDeviceToHost, s));
    } else {
        film_resolve_launch<float>(r->cfg.xres, win, layout, r->film, r->rs_stage, r->rs_clamped, s);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(host_out, r->rs_stage, want, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (n_clamped) *n_clamped = clamped;
    return 0;
}
// ---- film error against a reference image (include/vspg.h, vspg_film_error.h) ----
// (work of an earlier enqueue that still reads the reference image or writes the partial sums: the host waits for it)
static int film_error_wait(VspgRenderer *r) {
    if (r->fe_inflight) HIPCHK(hipEventSynchronize(r->fe_event));
    r->fe_inflight = false;
    return 0;
}
int vspg_renderer_set_reference_image(VspgRenderer *r, const float *host_rgb, void *stream) {
    if (!r) return fail(VSPG_EINVAL, "null renderer");
    HIPCHK(hipSetDevice(r->cfg.device));
    if (const int rc = film_error_wait(r)) return rc;
    if (!host_rgb) {
        r->fe_ref_set = false;
        return 0;
    }
    hipStream_t s = (hipStream_t)stream;
    if (!r->fe_ref) HIPCHK(hipMalloc(&r->fe_ref, r->npix * sizeof(float4)));
    if (!r->fe_partials) HIPCHK(hipMalloc(&r->fe_partials, (size_t)r->cfg.yres * 6 * sizeof(double)));
    if (!r->fe_log) HIPCHK(hipMalloc(&r->fe_log, (size_t)VSPG_FILM_ERROR_LOG_RECORDS * sizeof(VspgFilmError)));
    if (!r->fe_event) HIPCHK(hipEventCreateWithFlags(&r->fe_event, hipEventDisableTiming));
    std::vector<float4> padded(r->npix);
    for (size_t i = 0; i < r->npix; ++i) padded[i] = make_float4(host_rgb[3 * i], host_rgb[3 * i + 1], host_rgb[3 * i + 2], 0.f);
    HIPCHK(hipMemcpyAsync(r->fe_ref, padded.data(), r->npix * sizeof(float4), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    r->fe_ref_set = true;
    return 0;
}
int vspg_film_error_enqueue(VspgRenderer *r, int x0, int y0, int x1, int y1, int tag, void *stream) {
    if (!r) return fail(VSPG_EINVAL, "null renderer");
    if (x0 < 0 || y0 < 0 || x1 <= x0 || y1 <= y0 || x1 > r->cfg.xres || y1 > r->cfg.yres)
        return fail(VSPG_EINVAL, "pixel window [" + std::to_string(x0) + "," + std::to_string(x1) + ") x [" + std::to_string(y0) + "," + std::to_string(y1) +
                                     ") is empty or not inside the " + std::to_string(r->cfg.xres) + " x " + std::to_string(r->cfg.yres) + " film");
    if (!r->fe_ref_set) return fail(VSPG_EINVAL, "vspg_film_error_enqueue: no reference image (vspg_renderer_set_reference_image)");
    if (r->fe_count >= (size_t)VSPG_FILM_ERROR_LOG_RECORDS)
        return fail(VSPG_EINVAL, "vspg_film_error_enqueue: the log holds " + std::to_string(VSPG_FILM_ERROR_LOG_RECORDS) +
                                     " records and is full (vspg_film_error_read empties it)");
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = flush_parked_samples(r, s)) return rc;  // (the record is of the complete film)
    if (r->fe_inflight && s != r->fe_stream) HIPCHK(hipStreamWaitEvent(s, r->fe_event, 0));
    const PixelWindow win = {x0, y0, x1, y1};
    hipLaunchKernelGGL(k_film_error_rows, dim3((unsigned)(y1 - y0)), dim3(kFilmErrorBlock), 0, s, r->cfg.xres, win, r->film, r->fe_ref, r->fe_partials);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_film_error_finish, dim3(1), dim3(kFilmErrorBlock), 0, s, win, tag, r->fe_partials, r->fe_log + r->fe_count);
    HIPCHK(hipGetLastError());
    ++r->fe_count;
    HIPCHK(hipEventRecord(r->fe_event, s));
    r->fe_stream = s;
    r->fe_inflight = true;
    return 0;
}
int vspg_film_error_read(VspgRenderer *r, VspgFilmError *out, size_t max_records, size_t *n_out, void *stream) {
    if (!r || !out) return fail(VSPG_EINVAL, "null argument");
    if (max_records < r->fe_count)
        return fail(VSPG_EINVAL, "vspg_film_error_read: the log holds " + std::to_string(r->fe_count) + " records, room for " + std::to_string(max_records));
    if (n_out) *n_out = 0;
    if (r->fe_count == 0) return 0;
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipStreamSynchronize(s));
    if (const int rc = film_error_wait(r)) return rc;  // (enqueues that went to another stream)
    HIPCHK(hipMemcpyAsync(out, r->fe_log, r->fe_count * sizeof(VspgFilmError), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    int khz = 0;
    HIPCHK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, r->cfg.device));
    for (size_t i = 0; i < r->fe_count; ++i) out[i].tick_khz = (uint32_t)khz;
    if (n_out) *n_out = r->fe_count;
    r->fe_count = 0;
    return 0;
}
int vspg_vsp_buffer_device_ptr(VspgRenderer *r, float **dev_ptr, size_t *n_floats) {
    if (!r || !dev_ptr || !n_floats) return fail(VSPG_EINVAL, "null argument");
    *dev_ptr = r->vsp;
    *n_floats = r->npix;
    return 0;
}
int vspg_vsp_buffer_read(VspgRenderer *r, float *host, int *is_ready, void *stream) {
    if (!r || !host) return fail(VSPG_EINVAL, "null argument");
    HIPCHK(hipSetDevice(r->cfg.device));
    HIPCHK(hipMemcpyAsync(host, r->vsp, r->npix * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    if (is_ready) *is_ready = r->vsp_ready;
    return 0;
}
// TrBuffer (cpu/trbuffer.h): read-back = what Store() writes, set = TrBuffer(fileName) / Load()
int vspg_renderer_get_tr_buffer(VspgRenderer *r, float *host_rgb, int32_t *host_spp, void *stream) {
    if (!r || !host_rgb) return fail(VSPG_EINVAL, "null argument");
    if (!r->tr_rgb) return fail(VSPG_EINVAL, "the renderer keeps no transmittance buffer (storeTrBuffer / NDS+ not requested)");
    HIPCHK(hipSetDevice(r->cfg.device));
    HIPCHK(hipMemcpyAsync(host_rgb, r->tr_rgb, r->npix * 3 * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream));
    if (host_spp) {
        if (r->tr_spp) HIPCHK(hipMemcpyAsync(host_spp, r->tr_spp, r->npix * sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
        else memset(host_spp, 0, r->npix * sizeof(int32_t));
    }
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}
int vspg_renderer_set_tr_buffer(VspgRenderer *r, const float *host_rgb, void *stream) {
    if (!r || !host_rgb) return fail(VSPG_EINVAL, "null argument");
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = flush_parked_samples(r, s)) return rc;  // (paths in flight end under the scene they started in)
    if (!r->tr_rgb) HIPCHK(hipMalloc(&r->tr_rgb, r->npix * 3 * sizeof(float)));
    HIPCHK(hipMemcpyAsync(r->tr_rgb, host_rgb, r->npix * 3 * sizeof(float), hipMemcpyHostToDevice, s));
    // trBufferLoad = true, calculateTrBuffer = false (:182-184).  Only these members are rewritten: the field
    // counters of the device-side scene belong to the training kernels.
    r->hscene.tr_rgb = r->tr_rgb;
    r->hscene.tr_calc = 0;
    r->hscene.tr_load = 1;
    HIPCHK(hipMemcpyAsync(reinterpret_cast<char *>(r->dscene) + offsetof(DScene, tr_rgb), &r->hscene.tr_rgb,
                          sizeof(DScene) - offsetof(DScene, tr_rgb), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}
int vspg_vsp_buffer_load(VspgRenderer *r, const float *host, void *stream) {
    if (!r || !host) return fail(VSPG_EINVAL, "null argument");
    HIPCHK(hipSetDevice(r->cfg.device));
    if (const int rc = flush_parked_samples(r, (hipStream_t)stream)) return rc;  // (paths in flight end under the buffer they started with)
    HIPCHK(hipMemcpyAsync(r->vsp, host, r->npix * sizeof(float), hipMemcpyHostToDevice, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    r->vsp_ready = 1;
    r->vsp_loaded = true;
    return 0;
}
int vspg_isg_stats_device_ptr(VspgRenderer *r, float **dev_ptr, size_t *n_floats) {
    if (!r || !dev_ptr || !n_floats) return fail(VSPG_EINVAL, "null argument");
    if (r->ws_parked) {
        HIPCHK(hipSetDevice(r->cfg.device));
        const hipStream_t s = r->ws_stream;
        if (const int rc = flush_parked_samples(r, s)) return rc;
        HIPCHK(hipStreamSynchronize(s));
    }
    *dev_ptr = r->isg_stats;
    *n_floats = r->npix * VSPG_ISG_STATS;
    return 0;
}
int vspg_get_counters(VspgRenderer *r, VspgCounters *out, void *stream) {
    if (!r || !out) return fail(VSPG_EINVAL, "null argument");
    HIPCHK(hipSetDevice(r->cfg.device));
    if (const int rc = drain_carried_paths(r, (hipStream_t)stream)) return rc;  // (the counters of paths in flight: they end first)
    unsigned long long h[kNumCounters];
    HIPCHK(hipMemcpyAsync(h, r->counters, sizeof h, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    out->paths = h[0]; out->segments = h[1]; out->volume_scatters = h[2];
    out->surface_hits = h[3]; out->density_queries = h[4]; out->shadow_rays = h[5];
    out->shadow_density_queries = h[6];
    return 0;
}
int vspg_reset_counters(VspgRenderer *r, void *stream) {
    if (!r) return fail(VSPG_EINVAL, "null renderer");
    HIPCHK(hipSetDevice(r->cfg.device));
    if (const int rc = drain_carried_paths(r, (hipStream_t)stream)) return rc;  // (... and are counted before the reset)
    HIPCHK(hipMemsetAsync(r->counters, 0, kNumCounters * sizeof(unsigned long long), (hipStream_t)stream));
    return 0;
}

// scoped device scratch for the batch entry points
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

int vspg_trace_paths(VspgRenderer *r, int n, const int32_t *pixel_xy, const int32_t *sample_index, float *out_L,
                     int32_t *out_segments, void *stream) {
    if (!r || n < 0 || (n > 0 && (!pixel_xy || !sample_index || !out_L))) return fail(VSPG_EINVAL, "bad arguments");
    if (n == 0) return 0;
    for (int i = 0; i < n; ++i)
        if (pixel_xy[2 * i] < 0 || pixel_xy[2 * i] >= r->cfg.xres || pixel_xy[2 * i + 1] < 0 || pixel_xy[2 * i + 1] >= r->cfg.yres)
            return fail(VSPG_EINVAL, "pixel outside the film");
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    DevBuf dp, ds, dl, dg;
    HIPCHK(hipMalloc(&dp.p, (size_t)n * 2 * sizeof(int32_t)));
    HIPCHK(hipMalloc(&ds.p, (size_t)n * sizeof(int32_t)));
    HIPCHK(hipMalloc(&dl.p, (size_t)n * 3 * sizeof(float)));
    HIPCHK(hipMalloc(&dg.p, (size_t)n * sizeof(int32_t)));
    HIPCHK(hipMemcpyAsync(dp.p, pixel_xy, (size_t)n * 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ds.p, sample_index, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    const bool grid = r->scene.medium.type == VSPG_MEDIUM_GRID;
    const bool guided = wants_guiding(r->prm);
    if (guided && !r->field_set) return fail(VSPG_ESCOPE, "guiding enabled but no guiding field uploaded");
#define VSPG_LAUNCH_TRACE(M, G)                                                                                       \
    hipLaunchKernelGGL((k_trace_paths<M, G>), dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, r->dscene, r->vsp, \
                       r->vsp_ready | VSP_NO_FEED, n, (const int32_t *)dp.p, (const int32_t *)ds.p, (float *)dl.p, (int32_t *)dg.p)
    const bool nvdb = r->scene.medium.type == VSPG_MEDIUM_NANOVDB;
    if (r->arith != VSPG_ARITH_EXACT) {  // the replay in the renderer's arithmetic (set_arithmetic accepted unguided homogeneous / uniformgrid only)
        const TraceLaunch T{r->dscene, r->vsp, r->vsp_ready | VSP_NO_FEED, n, (const int32_t *)dp.p, (const int32_t *)ds.p, (float *)dl.p, (int32_t *)dg.p, s, grid ? 1 : 0};
        const int trc = r->arith == VSPG_ARITH_FAST_WEIGHTS ? vspg_arith1_trace(&T) : vspg_arith2_trace(&T);
        if (trc != 0) return fail(VSPG_EHIP, std::string("k_trace_paths: ") + hipGetErrorName((hipError_t)trc));
    } else if (r->scene.medium.type == VSPG_MEDIUM_RGBGRID) {  // (the kernel lives in vspg_wf_rgbgrid.hip)
        const TraceLaunch T{r->dscene, r->vsp, r->vsp_ready | VSP_NO_FEED, n, (const int32_t *)dp.p, (const int32_t *)ds.p, (float *)dl.p, (int32_t *)dg.p, s, 0};
        const int trc = trace_launch_rgbgrid(T, guided);
        if (trc != 0) return fail(VSPG_EHIP, std::string("k_trace_paths: ") + hipGetErrorName((hipError_t)trc));
    } else
    if (nvdb && guided) VSPG_LAUNCH_TRACE(NanoDenseMedium, true);
    else if (nvdb) VSPG_LAUNCH_TRACE(NanoDenseMedium, false);
    else if (grid && guided) VSPG_LAUNCH_TRACE(GridMedium, true);
    else if (grid) VSPG_LAUNCH_TRACE(GridMedium, false);
    else if (guided) VSPG_LAUNCH_TRACE(HomogeneousMedium, true);
    else VSPG_LAUNCH_TRACE(HomogeneousMedium, false);
#undef VSPG_LAUNCH_TRACE
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_L, dl.p, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost, s));
    if (out_segments) HIPCHK(hipMemcpyAsync(out_segments, dg.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int vspg_ray_batch(VspgRenderer *r, int n, const VspgRayQuery *q, VspgRayResult *out, void *stream) {
    if (!r || n < 0 || (n > 0 && (!q || !out))) return fail(VSPG_EINVAL, "bad arguments");
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    DevBuf dq, dout;
    HIPCHK(hipMalloc(&dq.p, (size_t)n * sizeof(VspgRayQuery)));
    HIPCHK(hipMalloc(&dout.p, (size_t)n * sizeof(VspgRayResult)));
    HIPCHK(hipMemcpyAsync(dq.p, q, (size_t)n * sizeof(VspgRayQuery), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_ray_batch, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, r->dscene, n, (const VspgRayQuery *)dq.p, (VspgRayResult *)dout.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dout.p, (size_t)n * sizeof(VspgRayResult), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int vspg_sample_tmaj_batch(VspgRenderer *r, int variant, int n, const VspgTmajQuery *q, VspgTmajResult *out, void *stream) {
    if (!r || n < 0 || (n > 0 && (!q || !out))) return fail(VSPG_EINVAL, "bad arguments");
    if (variant < VSPG_TMAJ_PLAIN || variant > VSPG_TMAJ_RESAMPLING) return fail(VSPG_EINVAL, "unknown variant");
    if (n == 0) return 0;
    for (int i = 0; i < n; ++i)
        if (q[i].channel < 0 || q[i].channel > 2) return fail(VSPG_EINVAL, "channel must be 0..2");
    if (r->scene.medium.type == VSPG_MEDIUM_NONE) return fail(VSPG_EINVAL, "renderer has no medium");
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    DevBuf dq, dr;
    HIPCHK(hipMalloc(&dq.p, (size_t)n * sizeof(VspgTmajQuery)));
    HIPCHK(hipMalloc(&dr.p, (size_t)n * sizeof(VspgTmajResult)));
    HIPCHK(hipMemcpyAsync(dq.p, q, (size_t)n * sizeof(VspgTmajQuery), hipMemcpyHostToDevice, s));
    if (r->scene.medium.type == VSPG_MEDIUM_NANOVDB)
        hipLaunchKernelGGL(k_tmaj_batch<NanoDenseMedium>, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, r->dscene, variant, n,
                           (const VspgTmajQuery *)dq.p, (VspgTmajResult *)dr.p);
    else if (r->scene.medium.type == VSPG_MEDIUM_GRID)
        hipLaunchKernelGGL(k_tmaj_batch<GridMedium>, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, r->dscene, variant, n,
                           (const VspgTmajQuery *)dq.p, (VspgTmajResult *)dr.p);
    else if (r->scene.medium.type == VSPG_MEDIUM_RGBGRID)
        hipLaunchKernelGGL(k_tmaj_batch<RgbGridMedium>, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, r->dscene, variant, n,
                           (const VspgTmajQuery *)dq.p, (VspgTmajResult *)dr.p);
    else
        hipLaunchKernelGGL(k_tmaj_batch<HomogeneousMedium>, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, r->dscene, variant, n,
                           (const VspgTmajQuery *)dq.p, (VspgTmajResult *)dr.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dr.p, (size_t)n * sizeof(VspgTmajResult), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int vspg_primitives_batch(VspgRenderer *r, int n, const float *f, const float *g, uint64_t *hash, uint32_t *rng_u32,
                          float *fastexp, void *stream) {
    if (!r || n < 0 || (n > 0 && (!f || !g || !hash || !rng_u32 || !fastexp))) return fail(VSPG_EINVAL, "bad arguments");
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    DevBuf df, dg, dh, du, de;
    HIPCHK(hipMalloc(&df.p, (size_t)n * 4));
    HIPCHK(hipMalloc(&dg.p, (size_t)n * 4));
    HIPCHK(hipMalloc(&dh.p, (size_t)n * 8));
    HIPCHK(hipMalloc(&du.p, (size_t)n * 4));
    HIPCHK(hipMalloc(&de.p, (size_t)n * 4));
    HIPCHK(hipMemcpyAsync(df.p, f, (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dg.p, g, (size_t)n * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_primitives, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, n, (const float *)df.p, (const float *)dg.p,
                       (uint64_t *)dh.p, (uint32_t *)du.p, (float *)de.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hash, dh.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(rng_u32, du.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(fastexp, de.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

static bool has_bricks(const VspgRenderer *r) {
    return r->scene.medium.type == VSPG_MEDIUM_GRID || r->scene.medium.type == VSPG_MEDIUM_NANOVDB;
}

int vspg_brick_info(VspgRenderer *r, VspgBrickInfo *out) {
    if (!r || !out) return fail(VSPG_EINVAL, "null argument");
    if (!has_bricks(r)) return fail(VSPG_EINVAL, "renderer has no grid medium");
    const size_t nb = (size_t)r->hscene.bnx * r->hscene.bny * r->hscene.bnz;
    out->bnx = r->hscene.bnx; out->bny = r->hscene.bny; out->bnz = r->hscene.bnz;
    out->indexed = r->brick_index ? 1 : 0;
    out->n_stored = r->n_bricks;
    out->index_bytes = r->brick_index ? nb * sizeof(int32_t) : 0;
    out->octet_bytes = (r->n_bricks ? r->n_bricks : 1) * 512 * 2 * sizeof(float4);
    return 0;
}

int vspg_brick_read(VspgRenderer *r, int32_t *index, float *octets, void *stream) {
    if (!r) return fail(VSPG_EINVAL, "null renderer");
    if (!has_bricks(r)) return fail(VSPG_EINVAL, "renderer has no grid medium");
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    const size_t nb = (size_t)r->hscene.bnx * r->hscene.bny * r->hscene.bnz;
    if (index) {
        if (r->brick_index) HIPCHK(hipMemcpyAsync(index, r->brick_index, nb * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        else for (size_t b = 0; b < nb; ++b) index[b] = (int32_t)b;   // dense: GridMediumT::octet uses the cell number as the slot
    }
    if (octets && r->n_bricks) HIPCHK(hipMemcpyAsync(octets, r->octets, r->n_bricks * 512 * 2 * sizeof(float4), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int vspg_medium_point_batch(VspgRenderer *r, int n, const float *p, float *out, void *stream) {
    if (!r || n < 0 || (n > 0 && (!p || !out))) return fail(VSPG_EINVAL, "bad arguments");
    const int type = r->scene.medium.type;
    if (type != VSPG_MEDIUM_GRID && type != VSPG_MEDIUM_NANOVDB && type != VSPG_MEDIUM_RGBGRID) return fail(VSPG_EINVAL, "renderer has no grid medium");
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    DevBuf dp, dout;
    HIPCHK(hipMalloc(&dp.p, (size_t)n * 3 * sizeof(float)));
    HIPCHK(hipMalloc(&dout.p, (size_t)n * VSPG_MEDIUM_POINT_OUT * sizeof(float)));
    HIPCHK(hipMemcpyAsync(dp.p, p, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, s));
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
    if (type == VSPG_MEDIUM_RGBGRID) hipLaunchKernelGGL(k_medium_point_batch<RgbGridMedium>, grid, block, 0, s, r->dscene, n, (const float *)dp.p, (float *)dout.p);
    else if (type == VSPG_MEDIUM_NANOVDB) hipLaunchKernelGGL(k_medium_point_batch<NanoDenseMedium>, grid, block, 0, s, r->dscene, n, (const float *)dp.p, (float *)dout.p);
    else hipLaunchKernelGGL(k_medium_point_batch<GridMedium>, grid, block, 0, s, r->dscene, n, (const float *)dp.p, (float *)dout.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dout.p, (size_t)n * VSPG_MEDIUM_POINT_OUT * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int vspg_majorant_read(VspgRenderer *r, float *host_out, size_t n_floats, int32_t *res, void *stream) {
    if (!r || !host_out) return fail(VSPG_EINVAL, "null argument");
    if (!has_bricks(r) && r->scene.medium.type != VSPG_MEDIUM_RGBGRID) return fail(VSPG_EINVAL, "renderer has no grid medium");
    const int R = majorant_res(r->scene.medium);
    if (res) *res = R;
    if (n_floats != (size_t)R * R * R) return fail(VSPG_EINVAL, "n_floats is not the majorant grid's resolution cubed");
    HIPCHK(hipSetDevice(r->cfg.device));
    HIPCHK(hipMemcpyAsync(host_out, r->majorant, n_floats * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

// The density update's device work, behind the refusals and the flush: majorants into r->majorant (in place), then the bricks as create
// builds them -- flags on the device, slot numbering on the host, fill on the device -- from `d`, the new samples ON THE DEVICE.
// Temporaries are the caller's to free (`tmp`), whatever the outcome.
static int rebuild_density_storage(VspgRenderer *r, const float *d, hipStream_t s, std::vector<void *> &tmp) {
    const VspgMedium &m = r->scene.medium;
    const int nx = m.nx, ny = m.ny, nz = m.nz;
    const bool nvdb = m.type == VSPG_MEDIUM_NANOVDB;
    auto dev_alloc = [&](void **p, size_t bytes) {
        const hipError_t e = hipMalloc(p, bytes);
        if (e == hipSuccess) tmp.push_back(*p);
        return e;
    };
    {   // majorants: the three per-axis box tables are the host's (majorant_axis_ranges), the maxima the device's
        const int R = majorant_res(m);
        const std::vector<int2> ranges = majorant_axis_ranges(m);
        const int n[3] = {nx, ny, nz};
        for (int k = 0; k < 3; ++k)
            for (int c = 0; c < R; ++c) {  // (what the kernel indexes with: inside the grid, or empty)
                const int2 q = ranges[(size_t)k * R + c];
                if (q.y >= q.x && (q.x < 0 || q.y > n[k] - 1)) return fail(VSPG_EINVAL, "majorant cell footprint outside the density grid");
            }
        int2 *dranges = nullptr;
        HIPCHK(dev_alloc((void **)&dranges, ranges.size() * sizeof(int2)));
        HIPCHK(hipMemcpyAsync(dranges, ranges.data(), ranges.size() * sizeof(int2), hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));  // (`ranges` is pageable and leaves scope)
        if (nvdb) hipLaunchKernelGGL(k_majorant_build<true>, dim3((unsigned)(R * R * R)), dim3(kMajBlock), 0, s, d, nx, ny, R, dranges,
                                     m.density_offset, m.majorant_scale, r->majorant);
        else hipLaunchKernelGGL(k_majorant_build<false>, dim3((unsigned)(R * R * R)), dim3(kMajBlock), 0, s, d, nx, ny, R, dranges, 0.f, 1.f,
                                r->majorant);
        HIPCHK(hipGetLastError());
    }
    const int bnx = r->hscene.bnx, bny = r->hscene.bny, bnz = r->hscene.bnz;
    const size_t nb = (size_t)bnx * bny * bnz;
    const bool dense = r->brick_index == nullptr;  // the layout create chose
    std::vector<int32_t> index(nb), active;
    if (dense) {
        for (size_t b = 0; b < nb; ++b) active.push_back((int32_t)b);
    } else {
        int32_t *dflags = nullptr;
        HIPCHK(dev_alloc((void **)&dflags, nb * sizeof(int32_t)));
        hipLaunchKernelGGL(k_brick_flags, dim3((unsigned)nb), dim3(kBlock), 0, s, d, nx, ny, nz, bnx, bny, dflags);
        HIPCHK(hipGetLastError());
        std::vector<int32_t> flags(nb);
        HIPCHK(hipMemcpyAsync(flags.data(), dflags, nb * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (size_t b = 0; b < nb; ++b) {
            index[b] = flags[b] ? (int32_t)active.size() : -1;
            if (flags[b]) active.push_back((int32_t)b);
        }
        // the set of stored bricks follows the new values: another count is another allocation (one placeholder brick when none)
        if (active.size() != r->n_bricks) {
            float4 *fresh = nullptr;
            HIPCHK(hipMalloc(&fresh, (active.empty() ? 1 : active.size()) * 512 * 2 * sizeof(float4)));
            (void)hipFree(r->octets);  // (the stream is idle: the caller synchronised it behind the flush, and again above)
            r->octets = fresh;
            r->hscene.octets = fresh;
            HIPCHK(hipMemcpyAsync(reinterpret_cast<char *>(r->dscene) + offsetof(DScene, octets), &r->hscene.octets, sizeof r->hscene.octets,
                                  hipMemcpyHostToDevice, s));
        }
        r->n_bricks = active.size();
        HIPCHK(hipMemcpyAsync(r->brick_index, index.data(), nb * sizeof(int32_t), hipMemcpyHostToDevice, s));
    }
    if (!active.empty()) {
        int32_t *dactive = nullptr;
        HIPCHK(dev_alloc((void **)&dactive, active.size() * sizeof(int32_t)));
        HIPCHK(hipMemcpyAsync(dactive, active.data(), active.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_brick_fill, dim3((unsigned)active.size()), dim3(512), 0, s, d, nx, ny, nz, bnx, bny, dactive, r->octets);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(s));  // as create: the storage is complete, and the host vectors above may go
    return 0;
}

int vspg_renderer_update_grid(VspgRenderer *r, int which, const float *values, size_t n_floats, int memory, void *stream) {
    // every refusal comes before anything of the renderer changes -- parked samples included
    if (!r || !values) return fail(VSPG_EINVAL, "null argument");
    if (which != VSPG_GRID_DENSITY && which != VSPG_GRID_TEMPERATURE) return fail(VSPG_EINVAL, "unknown grid (VSPG_GRID_DENSITY / VSPG_GRID_TEMPERATURE)");
    if (memory != VSPG_MEM_HOST && memory != VSPG_MEM_DEVICE) return fail(VSPG_EINVAL, "unknown memory kind (VSPG_MEM_HOST / VSPG_MEM_DEVICE)");
    if (!has_bricks(r)) return fail(VSPG_EINVAL, "renderer has no grid medium");
    const size_t n = (size_t)r->scene.medium.nx * r->scene.medium.ny * r->scene.medium.nz;
    if (n_floats != n) return fail(VSPG_EINVAL, "n_floats is not nx * ny * nz of the grid the renderer was created with");
    if (which == VSPG_GRID_TEMPERATURE && !r->temperature)
        return fail(VSPG_EINVAL, "the renderer was created without a temperature grid (its kernels do not read one)");
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = flush_parked_samples(r, s)) return rc;  // (paths in flight end under the medium they started in)
    HIPCHK(hipStreamSynchronize(s));  // no launch may still read the old grid
    if (which == VSPG_GRID_TEMPERATURE) {
        HIPCHK(hipMemcpyAsync(r->temperature, values, n * sizeof(float), memory == VSPG_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
        return 0;
    }
    // a host source is staged on the device for the builders, as create stages it; a device source is read where it lies
    std::vector<void *> tmp;
    int rc = 0;
    const float *d = values;
    if (memory == VSPG_MEM_HOST) {
        float *staged = nullptr;
        hipError_t e = hipMalloc(&staged, n * sizeof(float));
        if (e == hipSuccess) {
            tmp.push_back(staged);
            e = hipMemcpyAsync(staged, values, n * sizeof(float), hipMemcpyHostToDevice, s);
        }
        if (e != hipSuccess) rc = fail(VSPG_EHIP, std::string("staging the density grid: ") + hipGetErrorName(e));
        d = staged;
    }
    if (!rc) rc = rebuild_density_storage(r, d, s, tmp);
    if (rc) (void)hipStreamSynchronize(s);
    for (void *p : tmp) (void)hipFree(p);
    return rc;
}

// The RGB grid medium's update (vspg_rgbgrid.h; kernels: vspg_rgb_update_kernels.h).  One call for the three grids: the majorant grid
// depends on both sigma grids and is rebuilt once.  A sigma grid that stays lends the majorant kernel its octets (corner 0 of octet
// (x + 1, y + 1, z + 1) is voxel (x, y, z)); create's host builders are not used here -- they are what this path is compared with.
int vspg_renderer_update_rgb_grids(VspgRenderer *r, const float *sigma_a, const float *sigma_s, const float *Le, size_t n_floats, int memory,
                                   void *stream) {
    // every refusal comes before anything of the renderer changes -- parked samples included
    if (!r) return fail(VSPG_EINVAL, "null renderer");
    if (r->scene.medium.type != VSPG_MEDIUM_RGBGRID) return fail(VSPG_EINVAL, "renderer has no RGB grid medium");
    if (!sigma_a && !sigma_s && !Le) return fail(VSPG_EINVAL, "no grid given (sigma_a, sigma_s and Le are all NULL)");
    const VspgMedium &m = r->scene.medium;
    const int nx = m.nx, ny = m.ny, nz = m.nz;
    const size_t n3 = (size_t)nx * ny * nz * 3;
    if (n_floats != n3) return fail(VSPG_EINVAL, "n_floats is not 3 * nx * ny * nz of the grids the renderer was created with");
    if (memory != VSPG_MEM_HOST && memory != VSPG_MEM_DEVICE) return fail(VSPG_EINVAL, "unknown memory kind (VSPG_MEM_HOST / VSPG_MEM_DEVICE)");
    const float *given[3] = {sigma_a, sigma_s, Le};
    const void *have[3] = {r->rgb_oct[0], r->rgb_oct[1], r->rgb_Le};
    for (int k = 0; k < 3; ++k)
        if (given[k] && !have[k])
            return fail(VSPG_EINVAL, std::string("the renderer was created without a \"") + (k == 0 ? "sigma_a" : k == 1 ? "sigma_s" : "Le") +
                                         "\" grid (its kernels branch the constant in and hold no storage for one)");
    const int R = majorant_res(m);
    const std::vector<int2> ranges = majorant_axis_ranges(m);
    {
        const int n[3] = {nx, ny, nz};
        for (int k = 0; k < 3; ++k)
            for (int c = 0; c < R; ++c) {  // (what the majorant kernel indexes with: inside the grid, or empty)
                const int2 q = ranges[(size_t)k * R + c];
                if (q.y >= q.x && (q.x < 0 || q.y > n[k] - 1)) return fail(VSPG_EINVAL, "majorant cell footprint outside the RGB grid");
            }
    }
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    if (memory == VSPG_MEM_HOST) {
        for (int k = 0; k < 3; ++k)
            if (given[k])
                if (const int rc = check_rgb_grid_values(given[k], n3, k)) return rc;
    } else {  // one read pass per given grid; the flags come back before anything of the renderer is written
        DevBuf dflags;
        int flags[3] = {0, 0, 0};
        HIPCHK(hipMalloc(&dflags.p, sizeof flags));
        HIPCHK(hipMemsetAsync(dflags.p, 0, sizeof flags, s));
        const unsigned blocks = (unsigned)std::min<size_t>((n3 + kBlock - 1) / kBlock, 4096);
        for (int k = 0; k < 3; ++k)
            if (given[k]) hipLaunchKernelGGL(k_rgb_validate, dim3(blocks), dim3(kBlock), 0, s, given[k], n3, (int *)dflags.p + k);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(flags, dflags.p, sizeof flags, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (int k = 0; k < 3; ++k)
            if (flags[k]) return rgb_grid_value_refusal(k);
    }
    if (const int rc = flush_parked_samples(r, s)) return rc;  // (paths in flight end under the medium they started in)
    HIPCHK(hipStreamSynchronize(s));  // no launch may still read the old grids
    // a host source of a sigma grid is staged on the device for the builders; a device source is read where it lies
    DevBuf staged[2], dranges;
    const float *d[2] = {sigma_a, sigma_s};
    if (memory == VSPG_MEM_HOST)
        for (int k = 0; k < 2; ++k)
            if (d[k]) {
                HIPCHK(hipMalloc(&staged[k].p, n3 * sizeof(float)));
                HIPCHK(hipMemcpyAsync(staged[k].p, d[k], n3 * sizeof(float), hipMemcpyHostToDevice, s));
                d[k] = (const float *)staged[k].p;
            }
    const int bnx = r->hscene.bnx, bny = r->hscene.bny, bnz = r->hscene.bnz;
    if (d[0] || d[1]) {
        HIPCHK(hipMalloc(&dranges.p, ranges.size() * sizeof(int2)));
        HIPCHK(hipMemcpyAsync(dranges.p, ranges.data(), ranges.size() * sizeof(int2), hipMemcpyHostToDevice, s));
        RgbMajSource src[2];
        for (int k = 0; k < 2; ++k) src[k] = RgbMajSource{d[k], d[k] ? nullptr : r->rgb_oct[k]};  // new values | its own octets | absent
        hipLaunchKernelGGL(k_majorant_build_rgb, dim3((unsigned)(R * R * R)), dim3(kMajBlock), 0, s, src[0], src[1], nx, ny, nz, bnx, bny, R,
                           (const int2 *)dranges.p, r->scene.rgb_sigma_scale, r->majorant);
        HIPCHK(hipGetLastError());
        const size_t nb = (size_t)bnx * bny * bnz;
        for (int k = 0; k < 2; ++k)
            if (d[k]) {
                hipLaunchKernelGGL(k_rgb_octet_build, dim3((unsigned)nb), dim3(512), 0, s, d[k], nx, ny, nz, bnx, bny, r->rgb_oct[k]);
                HIPCHK(hipGetLastError());
            }
    }
    if (Le) HIPCHK(hipMemcpyAsync(r->rgb_Le, Le, n3 * sizeof(float), memory == VSPG_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
    HIPCHK(hipStreamSynchronize(s));  // as create: the storage is complete, the sources and the temporaries may go
    return 0;
}

int vspg_rgb_octets_read(VspgRenderer *r, int which, float *host_out, size_t n_floats, void *stream) {
    if (!r || !host_out) return fail(VSPG_EINVAL, "null argument");
    if (r->scene.medium.type != VSPG_MEDIUM_RGBGRID) return fail(VSPG_EINVAL, "renderer has no RGB grid medium");
    if (which != 0 && which != 1) return fail(VSPG_EINVAL, "unknown grid (0 sigma_a, 1 sigma_s)");
    if (!r->rgb_oct[which]) return fail(VSPG_EINVAL, "the renderer was created without that grid");
    const size_t n = (size_t)r->hscene.bnx * r->hscene.bny * r->hscene.bnz * 512u * 32u;
    if (n_floats != n) return fail(VSPG_EINVAL, "n_floats is not bnx * bny * bnz * 512 * 32 (bn = (n + 8) / 8 per axis)");
    HIPCHK(hipSetDevice(r->cfg.device));
    HIPCHK(hipMemcpyAsync(host_out, r->rgb_oct[which], n * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

// A field that upload_field can take: absent / empty (the field is cleared), or arrays with children after their parent,
// leaves in range and 0..GK lobes per region.  Checked for BOTH fields before anything of the renderer changes.
static int validate_field(const VspgField *src) {
    if (!src || src->n_nodes <= 0 || src->n_regions <= 0) return 0;
    if (!src->nodes || !src->regions) return fail(VSPG_EINVAL, "guiding field without node / region arrays");
    for (int i = 0; i < src->n_nodes; ++i) {  // structural check: children after their parent, leaves in range
        uint32_t axis = src->nodes[i].packed & 3u, idx = src->nodes[i].packed >> 2;
        if (axis == 3u ? (int)idx >= src->n_regions : ((int)idx + 1 >= src->n_nodes || (int)idx <= i))
            return fail(VSPG_EINVAL, "malformed guiding-field kd-tree");
    }
    for (int i = 0; i < src->n_regions; ++i)
        if (src->regions[i].n_lobes < 0 || src->regions[i].n_lobes > VSPG_FIELD_LOBES)
            return fail(VSPG_EINVAL, "guiding-field region with an invalid lobe count");
    return 0;
}
// (src has passed validate_field)
static int upload_field(VspgRenderer *r, int f, const VspgField *src, hipStream_t s) {
    if (r->fnodes[f]) { (void)hipFree(r->fnodes[f]); r->fnodes[f] = nullptr; }
    if (r->fregions[f]) { (void)hipFree(r->fregions[f]); r->fregions[f] = nullptr; }
    if (r->faux[f]) { (void)hipFree(r->faux[f]); r->faux[f] = nullptr; }
    if (r->flobes[f]) { (void)hipFree(r->flobes[f]); r->flobes[f] = nullptr; }
    r->hscene.field[f] = DField{0, 0, nullptr, nullptr, nullptr, nullptr};
    if (!src || src->n_nodes <= 0 || src->n_regions <= 0) return 0;
    HIPCHK(hipMalloc(&r->fnodes[f], sizeof(VspgKdNode) * src->n_nodes));
    HIPCHK(hipMalloc(&r->fregions[f], sizeof(VspgFieldRegion) * src->n_regions));
    HIPCHK(hipMemcpyAsync(r->fnodes[f], src->nodes, sizeof(VspgKdNode) * src->n_nodes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(r->fregions[f], src->regions, sizeof(VspgFieldRegion) * src->n_regions, hipMemcpyHostToDevice, s));
    HIPCHK(hipMalloc(&r->faux[f], sizeof(float) * 2 * GK * src->n_regions));
    HIPCHK(hipMalloc(&r->flobes[f], sizeof(float4) * kRegionLobeQuads * src->n_regions));
    r->hscene.field[f] = DField{src->n_nodes, src->n_regions, r->fnodes[f], r->fregions[f], r->faux[f], r->flobes[f]};
    return 0;
}

int vspg_renderer_set_guiding_field(VspgRenderer *r, const VspgField *surface_field, const VspgField *volume_field,
                                    void *stream) {
    if (!r) return fail(VSPG_EINVAL, "null renderer");
    // a call refused by validation leaves the renderer exactly as it was: fields, training state, parked samples.  (A HIP
    // failure further down does not: training is off and the fields may be cleared by then -- but the device's scene record
    // is re-copied from the host's, so it never keeps a freed pointer.)
    if (const int vrc = validate_field(surface_field)) return vrc;
    if (const int vrc = validate_field(volume_field)) return vrc;
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    if (const int frc = flush_parked_samples(r, s)) return frc;  // (paths in flight end under the scene record they started with)
    HIPCHK(hipStreamSynchronize(s));  // no launch may still read the old field
    r->training = false;                // a loaded cache is not trained further (:117-122)
    int rc = upload_field(r, 0, surface_field, s);
    if (!rc) rc = upload_field(r, 1, volume_field, s);
    // the device's scene record follows the host's whatever happened above: it never keeps a pointer that was freed
    HIPCHK(hipMemcpyAsync(r->dscene, &r->hscene, sizeof(DScene), hipMemcpyHostToDevice, s));
    if (rc) {
        HIPCHK(hipStreamSynchronize(s));
        return rc;
    }
    for (int f = 0; f < 2; ++f)
        if (r->faux[f])
            hipLaunchKernelGGL(k_field_aux, dim3((r->hscene.field[f].n_regions * GK + kBlock - 1) / kBlock), dim3(kBlock), 0, s, r->dscene,
                               f, r->fregions[f], r->faux[f], r->flobes[f]);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    r->field_set = true;
    return 0;
}

int vspg_guiding_query_batch(VspgRenderer *r, int is_volume, float g, int n, const float *p, const float *n_or_wo,
                             const float *wi, const float *u, int32_t *out_ok, float *out_pdf, float *out_incoming_pdf,
                             float *out_vsp, float *out_ws, float *out_pdf_s, void *stream) {
    if (!r || n < 0 || (n > 0 && (!p || !n_or_wo || !wi || !u || !out_ok || !out_pdf || !out_incoming_pdf || !out_vsp || !out_ws || !out_pdf_s)))
        return fail(VSPG_EINVAL, "bad arguments");
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    DevBuf dp, da, dw, du, dok, dpdf, dinc, dvsp, dws, dps;
    const size_t n3 = (size_t)n * 3 * 4, n2 = (size_t)n * 2 * 4, n1 = (size_t)n * 4;
    HIPCHK(hipMalloc(&dp.p, n3)); HIPCHK(hipMalloc(&da.p, n3)); HIPCHK(hipMalloc(&dw.p, n3)); HIPCHK(hipMalloc(&du.p, n2));
    HIPCHK(hipMalloc(&dok.p, n1)); HIPCHK(hipMalloc(&dpdf.p, n1)); HIPCHK(hipMalloc(&dinc.p, n1)); HIPCHK(hipMalloc(&dvsp.p, n1));
    HIPCHK(hipMalloc(&dws.p, n3)); HIPCHK(hipMalloc(&dps.p, n1));
    HIPCHK(hipMemcpyAsync(dp.p, p, n3, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(da.p, n_or_wo, n3, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dw.p, wi, n3, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(du.p, u, n2, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_guiding_query, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, r->dscene, is_volume, g, n,
                       (const float *)dp.p, (const float *)da.p, (const float *)dw.p, (const float *)du.p, (int32_t *)dok.p,
                       (float *)dpdf.p, (float *)dinc.p, (float *)dvsp.p, (float *)dws.p, (float *)dps.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_ok, dok.p, n1, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_pdf, dpdf.p, n1, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_incoming_pdf, dinc.p, n1, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_vsp, dvsp.p, n1, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_ws, dws.p, n3, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_pdf_s, dps.p, n1, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int vspg_libm_batch(VspgRenderer *r, int n, const float *x, float *logf_out, float *sinf_out, float *cosf_out,
                    void *stream) {
    if (!r || n < 0 || (n > 0 && (!x || !logf_out || !sinf_out || !cosf_out))) return fail(VSPG_EINVAL, "bad arguments");
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    DevBuf dx, dl, ds, dc;
    HIPCHK(hipMalloc(&dx.p, (size_t)n * 4));
    HIPCHK(hipMalloc(&dl.p, (size_t)n * 4));
    HIPCHK(hipMalloc(&ds.p, (size_t)n * 4));
    HIPCHK(hipMalloc(&dc.p, (size_t)n * 4));
    HIPCHK(hipMemcpyAsync(dx.p, x, (size_t)n * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_libm, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, n, (const float *)dx.p, (float *)dl.p,
                       (float *)ds.p, (float *)dc.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(logf_out, dl.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(sinf_out, ds.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(cosf_out, dc.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int vspg_libm_powf_batch(VspgRenderer *r, int n, const float *x, const float *y, float *out, void *stream) {
    if (!r || !x || !y || !out || n <= 0) return fail(VSPG_EINVAL, "bad arguments");
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    DevBuf dx, dy, dout;
    HIPCHK(hipMalloc(&dx.p, (size_t)n * 4));
    HIPCHK(hipMalloc(&dy.p, (size_t)n * 4));
    HIPCHK(hipMalloc(&dout.p, (size_t)n * 4));
    HIPCHK(hipMemcpyAsync(dx.p, x, (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dy.p, y, (size_t)n * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_libm_powf, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, n, (const float *)dx.p, (const float *)dy.p,
                       (float *)dout.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dout.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int vspg_blackbody_batch(VspgRenderer *r, int n, const float *u, const float *T, float *out6, void *stream) {
    if (!r || !u || !T || !out6 || n < 0) return fail(VSPG_EINVAL, "null argument");
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    DevBuf du, dT, dout;
    HIPCHK(hipMalloc(&du.p, (size_t)n * 4));
    HIPCHK(hipMalloc(&dT.p, (size_t)n * 4));
    HIPCHK(hipMalloc(&dout.p, (size_t)n * 24));
    HIPCHK(hipMemcpyAsync(du.p, u, (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dT.p, T, (size_t)n * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_blackbody, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, n, (const float *)du.p, (const float *)dT.p, (float *)dout.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out6, dout.p, (size_t)n * 24, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int vspg_renderer_set_environment_image(VspgRenderer *r, int infinite_light_index, const float *host_rgb, int res,
                                        const float *render_from_light, void *stream) {
    // every refusal comes before anything of the renderer changes -- parked samples included
    if (!r || !host_rgb) return fail(VSPG_EINVAL, "null argument");
    const int k = infinite_light_index;
    if (k < 0 || k >= r->hscene.n_inf) return fail(VSPG_EINVAL, "infinite_light_index names no infinite light of the scene");
    if (r->hscene.inf_type[k] != VSPG_LIGHT_IMAGE_INFINITE) return fail(VSPG_EINVAL, "the infinite light is not of type VSPG_LIGHT_IMAGE_INFINITE");
    if (res < 1 || res > VSPG_ENV_MAX_RES) return fail(VSPG_EINVAL, "environment image resolution outside 1 .. VSPG_ENV_MAX_RES (4096)");
    const size_t n3 = (size_t)res * res * 3;
    for (size_t i = 0; i < n3; ++i) {
        if (host_rgb[i] != host_rgb[i]) return fail(VSPG_EINVAL, "environment image has not-a-number pixel values and so is not suitable as a light");
        if (std::isinf(host_rgb[i])) return fail(VSPG_EINVAL, "environment image has infinite pixel values and so is not suitable as a light");
    }
    float m[9], mi[9];
    if (!env_matrices(render_from_light, m, mi)) return fail(VSPG_EINVAL, "render_from_light is singular or not finite");
    EnvTables T;
    env_build_tables(host_rgb, res, &T);
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = flush_parked_samples(r, s)) return rc;  // (paths in flight end under the sky they started under)
    HIPCHK(hipStreamSynchronize(s));  // no launch may still read the old tables
    float *old = nullptr;
    if (const int rc = env_install(r, k, T, m, mi, s, &old)) return rc;
    r->hscene.portal[k] = DPortalLight{};  // a portal light becomes a plain image light again (its arrays lived in the old buffer)
    lsb::build(r->scene, r->prm, &r->hscene);  // the power sampler's alias table: the light's Phi changed
    // the light sampler and the environment slots are the tail of the record; the rest of the device's copy (the guiding fields a
    // training renderer updates in place) is not touched
    const size_t tail = offsetof(DScene, lsamp);
    HIPCHK(hipMemcpyAsync(reinterpret_cast<char *>(r->dscene) + tail, reinterpret_cast<const char *>(&r->hscene) + tail, sizeof(DScene) - tail,
                          hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    if (old) (void)hipFree(old);
    return 0;
}

int vspg_renderer_set_portal_environment_image(VspgRenderer *r, int infinite_light_index, const float *host_rgb, int res,
                                               const float *render_from_light, const float *portal, void *stream) {
    // every refusal comes before anything of the renderer changes and before any allocation
    if (!r || !host_rgb || !portal) return fail(VSPG_EINVAL, "null argument");
    const int k = infinite_light_index;
    if (k < 0 || k >= r->hscene.n_inf) return fail(VSPG_EINVAL, "infinite_light_index names no infinite light of the scene");
    if (r->hscene.inf_type[k] != VSPG_LIGHT_IMAGE_INFINITE) return fail(VSPG_EINVAL, "the infinite light is not of type VSPG_LIGHT_IMAGE_INFINITE");
    if (res < 1 || res > VSPG_ENV_MAX_RES) return fail(VSPG_EINVAL, "environment image resolution outside 1 .. VSPG_ENV_MAX_RES (4096)");
    const size_t n3 = (size_t)res * res * 3;
    for (size_t i = 0; i < n3; ++i) {
        if (host_rgb[i] != host_rgb[i]) return fail(VSPG_EINVAL, "environment image has not-a-number pixel values and so is not suitable as a light");
        if (std::isinf(host_rgb[i])) return fail(VSPG_EINVAL, "environment image has infinite pixel values and so is not suitable as a light");
    }
    float m[9], mi[9];
    if (!env_matrices(render_from_light, m, mi)) return fail(VSPG_EINVAL, "render_from_light is singular or not finite");
    if (const int rc = portal_refusal(portal)) return rc;
    PortalTables T;
    portal_build_tables(host_rgb, res, mi, portal, &T);
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = flush_parked_samples(r, s)) return rc;  // (paths in flight end under the sky they started under)
    HIPCHK(hipStreamSynchronize(s));  // no launch may still read the old tables
    float *old = nullptr;
    if (const int rc = env_install(r, k, T.env, m, mi, s, &old)) return rc;
    DPortalLight &P = r->hscene.portal[k];
    P = T.rec;
    P.image = r->env_buf[k] + T.o_image;
    P.func = r->env_buf[k] + T.o_func;
    P.sat = r->env_buf[k] + T.o_sat;
    lsb::build(r->scene, r->prm, &r->hscene);  // the power sampler's alias table: the light's Phi changed
    const size_t tail = offsetof(DScene, lsamp);  // (as in vspg_renderer_set_environment_image)
    HIPCHK(hipMemcpyAsync(reinterpret_cast<char *>(r->dscene) + tail, reinterpret_cast<const char *>(&r->hscene) + tail, sizeof(DScene) - tail,
                          hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    if (old) (void)hipFree(old);
    return 0;
}

int vspg_portallight_batch(VspgRenderer *r, int infinite_light_index, int n, const float *ctx_p, const float *dirs, const float *u, float *out,
                           void *stream) {
    if (!r || n < 0 || (n > 0 && (!ctx_p || !dirs || !u || !out))) return fail(VSPG_EINVAL, "null argument");
    const int k = infinite_light_index;
    if (k < 0 || k >= r->hscene.n_inf || r->hscene.inf_type[k] != VSPG_LIGHT_IMAGE_INFINITE || r->hscene.portal[k].res <= 0)
        return fail(VSPG_EINVAL, "infinite_light_index names no portal image infinite light of the scene");
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    DevBuf dp, dd, du, dout;
    HIPCHK(hipMalloc(&dp.p, (size_t)n * 12));
    HIPCHK(hipMalloc(&dd.p, (size_t)n * 12));
    HIPCHK(hipMalloc(&du.p, (size_t)n * 8));
    HIPCHK(hipMalloc(&dout.p, (size_t)n * VSPG_PORTALLIGHT_OUT * 4));
    HIPCHK(hipMemcpyAsync(dp.p, ctx_p, (size_t)n * 12, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dd.p, dirs, (size_t)n * 12, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(du.p, u, (size_t)n * 8, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_portallight, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, r->dscene, k, n, (const float *)dp.p, (const float *)dd.p,
                       (const float *)du.p, (float *)dout.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dout.p, (size_t)n * VSPG_PORTALLIGHT_OUT * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int vspg_portallight_read(VspgRenderer *r, int infinite_light_index, int *res_out, float *image, float *func, float *table, float *record20,
                          void *stream) {
    if (!r || !res_out) return fail(VSPG_EINVAL, "null argument");
    const int k = infinite_light_index;
    if (k < 0 || k >= r->hscene.n_inf || r->hscene.inf_type[k] != VSPG_LIGHT_IMAGE_INFINITE || r->hscene.portal[k].res <= 0)
        return fail(VSPG_EINVAL, "infinite_light_index names no portal image infinite light of the scene");
    const DPortalLight &P = r->hscene.portal[k];
    *res_out = P.res;
    if (record20) {
        for (int c = 0; c < 3; ++c) {
            record20[c] = P.p0[c]; record20[3 + c] = P.p2[c]; record20[6 + c] = P.fx[c]; record20[9 + c] = P.fy[c]; record20[12 + c] = P.fz[c];
            record20[16 + c] = P.sum_phi[c];
        }
        record20[15] = P.area;
        record20[19] = r->hscene.scene_radius;
    }
    if (!image && !func && !table) return 0;
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)P.res * P.res;
    if (image) HIPCHK(hipMemcpyAsync(image, P.image, n * 12, hipMemcpyDeviceToHost, s));
    if (func) HIPCHK(hipMemcpyAsync(func, P.func, n * 4, hipMemcpyDeviceToHost, s));
    if (table) HIPCHK(hipMemcpyAsync(table, P.sat, n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int vspg_renderer_set_light_image(VspgRenderer *r, int point_light_index, const float *host_pixels, int xres, int yres, int channels, void *stream) {
    // every refusal comes before anything of the renderer changes and before any allocation
    if (!r || !host_pixels) return fail(VSPG_EINVAL, "null argument");
    const int k = point_light_index;
    if (k < 0 || k >= r->hscene.n_point) return fail(VSPG_EINVAL, "point_light_index names no point-light slot of the scene");
    const int type = r->hscene.point[k].type;
    if (const int rc = image_light_refusal(type, host_pixels, xres, yres, channels)) return rc;
    ImageLightTables T;
    image_light_build(type, host_pixels, xres, yres, r->scene.point_lights[k].cone_angle_deg, &T);
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = flush_parked_samples(r, s)) return rc;  // (paths in flight end under the image they started under)
    HIPCHK(hipStreamSynchronize(s));  // no launch may still read the old image
    void *old = nullptr;
    if (const int rc = image_light_install(r, k, T, s, &old)) return rc;
    lsb::build(r->scene, r->prm, &r->hscene);  // the alias table and the BVH: the light's Phi and LightBounds changed
    // the light sampler and every light's slots are the tail of the record (as in vspg_renderer_set_environment_image)
    const size_t tail = offsetof(DScene, lsamp);
    HIPCHK(hipMemcpyAsync(reinterpret_cast<char *>(r->dscene) + tail, reinterpret_cast<const char *>(&r->hscene) + tail, sizeof(DScene) - tail,
                          hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    if (old) (void)hipFree(old);
    return 0;
}

int vspg_envlight_batch(VspgRenderer *r, int infinite_light_index, int n, const float *dirs, const float *u, float *out, void *stream) {
    if (!r || n < 0 || (n > 0 && (!dirs || !u || !out))) return fail(VSPG_EINVAL, "null argument");
    const int k = infinite_light_index;
    if (k < 0 || k >= r->hscene.n_inf || r->hscene.inf_type[k] != VSPG_LIGHT_IMAGE_INFINITE)
        return fail(VSPG_EINVAL, "infinite_light_index names no image infinite light of the scene");
    if (r->hscene.portal[k].res > 0)  // (the slot's DEnvLight then holds the 1 x 1 white image only: nothing the path kernels evaluate)
        return fail(VSPG_EINVAL, "the infinite light is a portal light: vspg_portallight_batch serves it");
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    DevBuf dd, du, dout;
    HIPCHK(hipMalloc(&dd.p, (size_t)n * 12));
    HIPCHK(hipMalloc(&du.p, (size_t)n * 8));
    HIPCHK(hipMalloc(&dout.p, (size_t)n * VSPG_ENVLIGHT_OUT * 4));
    HIPCHK(hipMemcpyAsync(dd.p, dirs, (size_t)n * 12, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(du.p, u, (size_t)n * 8, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_envlight, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, r->dscene, k, n, (const float *)dd.p, (const float *)du.p,
                       (float *)dout.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dout.p, (size_t)n * VSPG_ENVLIGHT_OUT * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int vspg_light_sample_batch(VspgRenderer *r, int n, const float *ctx_p, const float *ctx_n, const float *u, float *out, void *stream) {
    if (!r || n < 0 || (n > 0 && (!ctx_p || !ctx_n || !u || !out))) return fail(VSPG_EINVAL, "null argument");
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    DevBuf dp, dn, du, dout;
    HIPCHK(hipMalloc(&dp.p, (size_t)n * 12));
    HIPCHK(hipMalloc(&dn.p, (size_t)n * 12));
    HIPCHK(hipMalloc(&du.p, (size_t)n * 12));
    HIPCHK(hipMalloc(&dout.p, (size_t)n * VSPG_LIGHT_SAMPLE_OUT * 4));
    HIPCHK(hipMemcpyAsync(dp.p, ctx_p, (size_t)n * 12, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dn.p, ctx_n, (size_t)n * 12, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(du.p, u, (size_t)n * 12, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_light_sample_batch, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, r->dscene, n, (const float *)dp.p, (const float *)dn.p,
                       (const float *)du.p, (float *)dout.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dout.p, (size_t)n * VSPG_LIGHT_SAMPLE_OUT * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int vspg_light_pdf_batch(VspgRenderer *r, int light_index, int n, const float *ctx_p, const float *ctx_perr, const float *ctx_n, const float *wi,
                         float *out, void *stream) {
    if (!r || n < 0 || (n > 0 && (!ctx_p || !ctx_n || !wi || !out))) return fail(VSPG_EINVAL, "null argument");
    const DScene &H = r->hscene;
    if (light_index < 0 || light_index >= light_list_size(H)) return fail(VSPG_EINVAL, "light_index outside the scene's light list");
    if (light_index >= H.n_lights && light_index < H.n_lights + H.n_inf + H.n_point)
        return fail(VSPG_EINVAL, "vspg_light_pdf_batch serves lights with a shape (rectangles, spheres): an infinite or delta light has none");
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    DevBuf dp, de, dn, dw, dout;
    HIPCHK(hipMalloc(&dp.p, (size_t)n * 12));
    HIPCHK(hipMalloc(&dn.p, (size_t)n * 12));
    HIPCHK(hipMalloc(&dw.p, (size_t)n * 12));
    HIPCHK(hipMalloc(&dout.p, (size_t)n * VSPG_LIGHT_PDF_OUT * 4));
    HIPCHK(hipMemcpyAsync(dp.p, ctx_p, (size_t)n * 12, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dn.p, ctx_n, (size_t)n * 12, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dw.p, wi, (size_t)n * 12, hipMemcpyHostToDevice, s));
    if (ctx_perr) {
        HIPCHK(hipMalloc(&de.p, (size_t)n * 12));
        HIPCHK(hipMemcpyAsync(de.p, ctx_perr, (size_t)n * 12, hipMemcpyHostToDevice, s));
    }
    hipLaunchKernelGGL(k_light_pdf_batch, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, r->dscene, light_index, n, (const float *)dp.p,
                       (const float *)de.p, (const float *)dn.p, (const float *)dw.p, (float *)dout.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dout.p, (size_t)n * VSPG_LIGHT_PDF_OUT * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int vspg_renderer_set_texture_image(VspgRenderer *r, int texture_index, const float *host_pixels, int xres, int yres, int channels, void *stream) {
    // every refusal comes before anything of the renderer changes and before any allocation
    if (!r || !host_pixels) return fail(VSPG_EINVAL, "null argument");
    const int k = texture_index;
    if (k < 0 || k >= r->n_texture_slots) return fail(VSPG_EINVAL, "texture_index names no texture of the scene");
    if (const int rc = texture_image_refusal(host_pixels, xres, yres, channels)) return rc;
    const std::vector<float> img = texture_image_build(host_pixels, xres, yres, channels);
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = flush_parked_samples(r, s)) return rc;  // (paths in flight end under the image they started under)
    HIPCHK(hipStreamSynchronize(s));  // no launch may still read the old image
    float4 *old = nullptr;
    if (const int rc = texture_install(r, k, img, xres, yres, s, &old)) return rc;
    // the textures are the tail of the record (as in vspg_renderer_set_environment_image: the fields a training renderer updates in
    // place on the device lie in front of lsamp)
    const size_t tail = offsetof(DScene, lsamp);
    HIPCHK(hipMemcpyAsync(reinterpret_cast<char *>(r->dscene) + tail, reinterpret_cast<const char *>(&r->hscene) + tail, sizeof(DScene) - tail,
                          hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    if (old) (void)hipFree(old);
    return 0;
}

int vspg_texture_eval_batch(VspgRenderer *r, int n, const int32_t *prim, const float *hit, float *out, void *stream) {
    if (!r || n < 0 || (n > 0 && (!prim || !hit || !out))) return fail(VSPG_EINVAL, "null argument");
    if (n == 0) return 0;
    std::vector<int32_t> dev_prim((size_t)n);  // the caller's triangle j -> its position in the device's leaf order
    for (int i = 0; i < n; ++i) {
        const int p = prim[i];
        if (p >= 0) {
            if (p >= r->hscene.n_quads) return fail(VSPG_EINVAL, "prim names no rectangle of the scene");
            dev_prim[i] = p;
        } else {
            const long long j = -2ll - p;
            if (p == -1 || j >= (long long)r->tri_pos.size() || r->tri_pos[(size_t)j] < 0)
                return fail(VSPG_EINVAL, "prim names no triangle of the scene (or a degenerate one the build dropped)");
            dev_prim[i] = -2 - r->tri_pos[(size_t)j];
        }
    }
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    DevBuf dp, dh, dout;
    HIPCHK(hipMalloc(&dp.p, (size_t)n * 4));
    HIPCHK(hipMalloc(&dh.p, (size_t)n * 12));
    HIPCHK(hipMalloc(&dout.p, (size_t)n * VSPG_TEXTURE_EVAL_OUT * 4));
    HIPCHK(hipMemcpyAsync(dp.p, dev_prim.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dh.p, hit, (size_t)n * 12, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_texture_eval, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, r->dscene, n, (const int32_t *)dp.p, (const float *)dh.p,
                       (float *)dout.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dout.p, (size_t)n * VSPG_TEXTURE_EVAL_OUT * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));  // (dev_prim is pageable and dropped on return)
    return 0;
}

int vspg_renderer_set_camera(VspgRenderer *r, const VspgCamera *cam, const VspgCameraModel *model, void *stream) {
    // every refusal comes before anything of the renderer changes
    if (!r) return fail(VSPG_EINVAL, "null renderer");
    if (const int rc = camera_refusal(cam, model)) return rc;
    const VspgCameraModel rec = camera_model_record(model);
    if (r->arith != VSPG_ARITH_EXACT) {  // (the tolerance modes cover fewer kernels: the camera must not move the renderer out of them)
        ChoiceFacts f = choice_facts(r);
        f.camera_general = camera_model_general(rec);
        const KernelChoice c = choose_kernel(f, read_choice_env());
        if (!c.arith_covered)
            return fail(VSPG_ESCOPE, "the tolerance-mode instantiations do not cover " + kernel_name(c) + ", which this camera needs: set exact arithmetic first");
    }
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = flush_parked_samples(r, s)) return rc;  // (samples and paths in flight end under the camera they started with)
    HIPCHK(hipStreamSynchronize(s));  // no launch may still read the old camera
    r->scene.camera = *cam;
    r->hscene.cam = *cam;
    r->hscene.cam_model = rec.model;
    r->hscene.cam_lens_radius = rec.lens_radius;
    r->hscene.cam_focal_distance = rec.focal_distance;
    // two pieces of the record: `cam` in its first 4 KB and the model at its end (a training renderer updates fields between them in
    // place on the device: they are not the host copy's to overwrite)
    HIPCHK(hipMemcpyAsync(reinterpret_cast<char *>(r->dscene) + offsetof(DScene, cam), &r->hscene.cam, sizeof r->hscene.cam, hipMemcpyHostToDevice, s));
    const size_t tail = offsetof(DScene, cam_model);
    HIPCHK(hipMemcpyAsync(reinterpret_cast<char *>(r->dscene) + tail, reinterpret_cast<const char *>(&r->hscene) + tail, sizeof(DScene) - tail,
                          hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int vspg_camera_ray_batch(VspgRenderer *r, int n, const int32_t *pixel_xy, const int32_t *sample_index, const float *u, float *out_o, float *out_d,
                          void *stream) {
    if (!r || n < 0 || (n > 0 && (!pixel_xy || !sample_index || !out_o || !out_d))) return fail(VSPG_EINVAL, "null argument");
    if (n == 0) return 0;
    for (int i = 0; i < n; ++i) {
        const int x = pixel_xy[2 * (size_t)i], y = pixel_xy[2 * (size_t)i + 1];
        if (x < 0 || x >= r->cfg.xres || y < 0 || y >= r->cfg.yres) return fail(VSPG_EINVAL, "pixel outside the frame");
        if (sample_index[i] < 0) return fail(VSPG_EINVAL, "negative sample index");
    }
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    DevBuf dp, ds, du, doo, dd;
    HIPCHK(hipMalloc(&dp.p, (size_t)n * 8));
    HIPCHK(hipMalloc(&ds.p, (size_t)n * 4));
    if (u) HIPCHK(hipMalloc(&du.p, (size_t)n * 16));
    HIPCHK(hipMalloc(&doo.p, (size_t)n * 12));
    HIPCHK(hipMalloc(&dd.p, (size_t)n * 12));
    HIPCHK(hipMemcpyAsync(dp.p, pixel_xy, (size_t)n * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ds.p, sample_index, (size_t)n * 4, hipMemcpyHostToDevice, s));
    if (u) HIPCHK(hipMemcpyAsync(du.p, u, (size_t)n * 16, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_camera_ray, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, r->dscene, n, (const int32_t *)dp.p, (const int32_t *)ds.p,
                       (const float *)du.p, (float *)doo.p, (float *)dd.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_o, doo.p, (size_t)n * 12, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_d, dd.p, (size_t)n * 12, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int vspg_renderer_training_stats(VspgRenderer *r, VspgTrainStats *out, void *stream) {
    if (!r || !out) return fail(VSPG_EINVAL, "null argument");
    memset(out, 0, sizeof *out);
    out->training = r->training ? 1 : 0;
    out->iteration = r->field_iteration;
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    if (r->train_counters) {
        unsigned long long cnt[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(cnt, r->train_counters, sizeof cnt, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        out->n_samples = cnt[0];
        out->n_zero = cnt[1];
        out->n_dropped = cnt[0] > r->sample_capacity ? cnt[0] - r->sample_capacity : 0;
        DScene h;
        HIPCHK(hipMemcpyAsync(&h, r->dscene, sizeof h, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (int f = 0; f < 2; ++f) { out->n_nodes[f] = h.field[f].n_nodes; out->n_regions[f] = h.field[f].n_regions; }
    } else {
        for (int f = 0; f < 2; ++f) { out->n_nodes[f] = r->hscene.field[f].n_nodes; out->n_regions[f] = r->hscene.field[f].n_regions; }
    }
    return 0;
}
int vspg_train_samples_read(VspgRenderer *r, VspgTrainSample *out, size_t max_samples, size_t *n_out, void *stream) {
    if (!r || !n_out) return fail(VSPG_EINVAL, "null argument");
    *n_out = 0;
    if (!r->train_counters) return 0;
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    unsigned long long cnt = 0;
    HIPCHK(hipMemcpyAsync(&cnt, r->train_counters, sizeof cnt, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (cnt > r->sample_capacity) cnt = r->sample_capacity;
    *n_out = (size_t)cnt;
    const size_t n = cnt < max_samples ? (size_t)cnt : max_samples;
    if (out && n) {
        HIPCHK(hipMemcpyAsync(out, r->samples, n * sizeof(VspgTrainSample), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    return 0;
}
int vspg_renderer_get_guiding_field(VspgRenderer *r, int volume_field, VspgKdNode *nodes, VspgFieldRegion *regions,
                                    int32_t *n_nodes, int32_t *n_regions, void *stream) {
    if (!r || !n_nodes || !n_regions) return fail(VSPG_EINVAL, "null argument");
    const int f = volume_field ? 1 : 0;
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    DScene h;
    HIPCHK(hipMemcpyAsync(&h, r->dscene, sizeof h, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *n_nodes = h.field[f].n_nodes;
    *n_regions = h.field[f].n_regions;
    if (nodes && h.field[f].nodes && *n_nodes > 0)
        HIPCHK(hipMemcpyAsync(nodes, h.field[f].nodes, sizeof(VspgKdNode) * (size_t)*n_nodes, hipMemcpyDeviceToHost, s));
    if (regions && h.field[f].regions && *n_regions > 0)
        HIPCHK(hipMemcpyAsync(regions, h.field[f].regions, sizeof(VspgFieldRegion) * (size_t)*n_regions, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int vspg_libm_log1m_batch(VspgRenderer *r, int n, const float *x, float *out, void *stream) {
    if (!r || !x || !out || n < 0) return fail(VSPG_EINVAL, "bad argument");
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(r->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    DevBuf dx, dout;
    HIPCHK(hipMalloc(&dx.p, (size_t)n * 4));
    HIPCHK(hipMalloc(&dout.p, (size_t)n * 4));
    HIPCHK(hipMemcpyAsync(dx.p, x, (size_t)n * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_libm_log1m, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, n, (const float *)dx.p, (float *)dout.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dout.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

#ifdef VSPG_WF_DEBUG
int vspg_dbg_read(unsigned int *out8) {  // diagnostic build only
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_dbg_err), 8 * sizeof(unsigned int)));
    return 0;
}
#endif
#ifdef VSPG_WF_STATS
int vspg_wf_stats_read(unsigned long long *out16) {  // diagnostic build only: read and clear
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_wf_stats), 16 * sizeof(unsigned long long)));
    unsigned long long z[16] = {0};
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_wf_stats), z, sizeof z));
    return 0;
}
#endif
#ifdef VSPG_PROFILE
// diagnostic build only: dump and clear the per-section counters
int vspg_prof_read(unsigned long long *out /* PS_COUNT*3 */, int *n_sections) {
    unsigned long long h[PS_COUNT][3];
    HIPCHK(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_prof), sizeof h));
    memcpy(out, h, sizeof h);
    memset(h, 0, sizeof h);
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_prof), h, sizeof h));
    *n_sections = PS_COUNT;
    return 0;
}
#endif

}  // extern "C"
