// dpk_kernels.hip — MI355X (gfx950, CDNA4) DDIM sampler for DiffPose's GCNdiff denoiser.
//
// One persistent kernel runs the whole K-step reverse-diffusion loop of the reference
// (common/utils_diff.py:46-68) for a tile of P=4 poses per workgroup: every step's
// GCNdiff forward (models/gcndiff.py:101-113) and the DDIM update happen in LDS, so the
// only HBM traffic is the (N,17,5) input, the output and the weights (L2/MALL-resident).
//
// Tile geometry: 4 poses = 68 rows of 96 features; Linear/ChebConv
// GEMMs run on fp32 MFMA (v_mfma_f32_16x16x4_f32, exact fp32 fma chains) over 4 row tiles
// of 16 (each wave: 2 row tiles x half the columns), the 4 leftover rows on the VALU inside
// the same k-loop.  LayerNorm, 17-joint attention and the 17x17 graph products are VALU
// work between workgroup barriers.  Weights are repacked at load time into MFMA
// B-fragment order: one 1 KiB coalesced float4-per-lane load per (16 cols x 16 k) block.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "diffpose_kernels.h"

// Timing-only ablation builds (tools/ablate.py): bit set = phase skipped.  Outputs of such
// a build are wrong by construction; the shipped library is built with DPK_ABLATE=0.
#ifndef DPK_ABLATE
#define DPK_ABLATE 0
#endif
#define DPK_RUN(bit) ((DPK_ABLATE & (bit)) == 0)
// Phase tracing builds (tools/phase_trace.py): lane 0 of every wave stamps s_memtime before and
// after each workgroup barrier of one chosen DDIM step.
#ifndef DPK_TRACE
#define DPK_TRACE 0
#endif
// GEMM phase stamps: tools/gemm_probe.hip defines its own; trace builds stamp into the trace
// buffer (end of k-loop, end of epilogue); empty in the library
#if DPK_TRACE
namespace dpk {
__shared__ unsigned long long* tr_row[8];   // per-wave stamp row of the traced step (null: off)
__shared__ int tr_ix[8];
__device__ __forceinline__ void tr_stamp() {
    const int w = threadIdx.x >> 6;
    if (tr_row[w] && (threadIdx.x & 63) == 0 && tr_ix[w] < 256) tr_row[w][tr_ix[w]] = __builtin_amdgcn_s_memtime();
    if ((threadIdx.x & 63) == 0 && tr_row[w]) tr_ix[w] += 1;
}
}  // namespace dpk
#ifndef DPK_GEMM_HOOK
#define DPK_GEMM_HOOK(tag)                       \
    do {                                         \
        if ((tag) != 0) {                        \
            __builtin_amdgcn_sched_barrier(0);   \
            dpk::tr_stamp();                     \
            __builtin_amdgcn_sched_barrier(0);   \
        }                                        \
    } while (0)
#endif
#endif
#ifndef DPK_GEMM_HOOK
#define DPK_GEMM_HOOK(tag)
#endif


// Launch arguments of the sampler kernel, shared by both tile sizes (dpk_sampler.inc).
namespace dpk_shared {
struct SampleArgs {
    const float* arena;   // packed weights
    const float* coef;    // [K][6] = sqrt(1-at), sqrt(at), sqrt(an), c1, c2, t
    const float* tproj;   // [slots][NL][D] temb_proj(swish(temb)) per step (sample) / per pose (eps); zeros (pose)
    const float* x_in;    // [N][17][5]  (pose: [N][17][2] uv)
    float* x_out;         // [N][17][5]  final x (sample) or eps (eps mode); pose: [N][17][3] xyz or null
    float* xs;            // [K+1][N][17][5] or null
    float* x0s;           // [K][N][17][5]   or null
    float* uvxyz;         // pose: [H][N][17][5] cat(uv, root-processed xyz), repeated H times; or null
    int N;
    int K;
    int H;                // pose: test_times
    int root_mode;        // pose: 0 reference in-place quirk (root zeroed), 1 root-relative, 2 raw
    unsigned mask;        // 17-bit key mask
    const unsigned* pmask;  // per-pose 17-bit key masks [N] (dpk_set_pose_masks), or null: `mask` for all
    float eta;
    unsigned long long seed;
    int pose_off;         // first pose of this launch (a batch split over two launches, see launch_sampler)
    int num_layers;       // GraAttenLayer + _ResChebGC_diff pairs run (config num_layer, 1..NL)
    // Step-split last round (sample mode, launch_sampler): the last split_n tiles run their K steps
    // as two halves on two workgroups.  Blocks [0, split_n) run steps [0, split_k) of tiles
    // split_full + b and publish x_t through x_out and flags[b]; blocks [split_n, split_n + split_full)
    // run whole tiles; the last split_n blocks wait for their tile's flag and run [split_k, K).
    int split_n;
    int split_k;
    int split_full;
    unsigned* flags;      // [split_n] handoff words: 0 between launches, (token << 2) | state during one
    unsigned token;       // nonzero, per launch (30 bits)
    // (round 4; after the round-3 fields so their kernel-argument offsets, and the code built around
    // them, stay as they were)
    const float* noise;   // [K][N][17][5] caller noise for c1*z (the reference's per-step randn_like), or null
    int* split_stats;     // device counter: second halves that recomputed their first half's steps
    int split_dbg;        // dpk_debug_split: 0 normal; 1 first halves start late; 2 no idle wait
    // Hypothesis start (dpk_sample_start; after the round-4 fields for the same reason): with start_on the
    // launch runs the START instantiation of the kernel, whose load of x_in gives
    // x_T = x*start_sa + (e*scale)*start_sb (qsample_elem) and writes it to xs[0]
    int start_on;
    float start_sa;       // sqrtf(alpha_bar[t_start + 1])
    float start_sb;       // sqrtf(1 - alpha_bar[t_start + 1])
    const float* start_scale;   // [start_scale_rows][17][5], pose n reads row n % start_scale_rows; null: ones
    int start_scale_rows;
    // joints of the handle's model: 17, or 2..16 on padded tiles (the PAD kernels; every [..][17][5] above is then
    // [..][n_pts][5]).  In the padding ahead of the next pointer: no other field's offset moves
    int n_pts;
    const float* start_noise;   // [N][17][5] the caller's draws e, or null: normal_noise(seed, -1, element)
    // The denoising loss (dpk_diff_loss; eps mode, read under if constexpr (EPS_MODE) alone; at the end, so no
    // other field's offset moves).  With loss_t set the tile's load of x_in gives x_t = qsample_elem at pose n's own
    // row clamp(loss_t[n]) of loss_qtab (scale, draws and seed are the start's fields above) and writes it to
    // loss_xt; the epilogue stages (e*scale - eps)^2 and one lane per pose sums it into loss_out.  x_out may be null
    const float* loss_t;        // [N] per-pose timesteps, or null: plain dpk_eps
    const float* loss_qtab;     // [loss_nt][2] = sqrtf(abar[t + 1]), sqrtf(1 - abar[t + 1]) (Sched::qtab)
    int loss_nt;
    float* loss_out;            // [N] or null
    float* loss_xt;             // [N][17][5] or null
#if DPK_TRACE
    unsigned long long* trace;   // [blocks][NW][TRACE_SLOTS]
    int trace_step;
#endif
};

// The launch census (dpk_debug_sampler_kernels; host bookkeeping only).  One word names one compiled sample_kernel:
// the instance namespace's tile (DPK_TILE_ID: 0 dpk, 1 dpk8, 2 dpk2, 3 dpkw, 4 dpkw4, 5 dpkn, 6 dpkn4) in bits 0..3
// and the kernel's six template arguments: MODE in bits 4..5, SPARSE in bit 6, G16 in bits 7..8, ZM in bit 9, START
// in bit 10, PAD in bit 11.  Every hipLaunchKernelGGL site of launch_gemm_mode (dpk_genfused.inc) leaves the word of
// the instantiation it names in last_kernel, built from that site's own template arguments; launch_tiles moves it
// into the handle.
constexpr uint32_t kernel_id(int tile, int mode, bool sparse, int g16, int zm, bool start, bool pad) {
    return (uint32_t)tile | (uint32_t)mode << 4 | (uint32_t)sparse << 6 | (uint32_t)g16 << 7 | (uint32_t)zm << 9 |
           (uint32_t)start << 10 | (uint32_t)pad << 11;
}
constexpr uint32_t KERNEL_NONE = ~0u;
static thread_local uint32_t last_kernel = KERNEL_NONE;
}  // namespace dpk_shared

#include "dpk_stage.inc"
#include "dpk_genplan.inc"
#include "dpk_scratch.inc"
#include "dpk_counter.inc"

// All the host knows a compiled sampler instance by: its shape half (dpk_stage.inc) and how to launch it.  One
// per instance namespace, built where the table is (INSTANCES).
struct SamplerInst : InstShape {
    using Launch = void (*)(bool sparse, int gm, int blocks, size_t shmem, hipStream_t st,
                            const dpk_shared::SampleArgs& a, const float* W, const char* W16);
    void (*temb)(const float* temb, const float* t, int stride, int count, float* out, hipStream_t st);
    // appends the id (dpk_shared::kernel_id) of every sample_kernel compiled for this tile (dpk_genfused.inc)
    void (*kernels)(const SamplerInst& self, std::vector<uint32_t>& out);
    Launch launch[3];            // per kernel mode (M_SAMPLE, M_EPS, M_POSE); null: not compiled
    const SamplerInst* wave8;    // the same tile on 8 waves (M_SAMPLE only), or null
    const SamplerInst* tail2;    // the 2-pose tile of the same shape (launch_sampler's tail plans), or null
    // dpk_sample's timestep projections: true, the schedule's (Sched::tps, built per schedule and weight upload);
    // false, computed by every call into K * tp floats of pool scratch (then counted in floats, eps_scratch)
    bool sched_tps;
};

#define DPK_P 4
#define DPK_TILE_ID 0
namespace dpk {
#include "dpk_sampler.inc"
#include "dpk_genfused.inc"
}  // namespace dpk
#undef DPK_TILE_ID
// The same 4-pose tile on 8 waves, two per SIMD (dpk_layout.inc DPK_NW): each SIMD's GEMM column tiles split
// between its two waves, the per-pose phases split between the two waves of a pose as in the 2-pose tile.
// At most 256 registers per lane; dpk_set_tile_waves chooses between this instance and dpk per GEMM mode.
// (the sibling tiles of the shipped shape carry no padded kernels: DPK_PADDED 0, dpk_layout.inc)
#define DPK_NW 8
#undef DPK_PADDED
#define DPK_PADDED 0
#define DPK_TILE_ID 1
namespace dpk8 {
#include "dpk_sampler.inc"
#include "dpk_genfused.inc"
}  // namespace dpk8
#undef DPK_TILE_ID
#undef DPK_NW
#undef DPK_P
#define DPK_P 2
#define DPK_TILE_ID 2
namespace dpk2 {
#include "dpk_sampler.inc"
#include "dpk_genfused.inc"
}  // namespace dpk2
#undef DPK_TILE_ID
#undef DPK_PADDED
// The persistent sampler at a wider model (round 5): hid 128 / 8 heads (d_k 16), 2-pose tiles (4-pose
// tiles of 128-wide rows do not fit 160 KB of LDS), fp32 or f16x3 GEMMs; a handle of that shape runs it instead of the
// per-op launches of dpk_generic.inc
#undef DPK_P
#define DPK_P 2
#undef DPK_D
#undef DPK_NH
#define DPK_D 128
#define DPK_NH 8
#define DPK_TILE_ID 3
namespace dpkw {
#include "dpk_sampler.inc"
#include "dpk_genfused.inc"
}  // namespace dpkw
#undef DPK_TILE_ID
#undef DPK_NH
#undef DPK_D
#undef DPK_P
// ... at hid 128 / 4 heads (d_k 32), 2-pose tiles
#define DPK_P 2
#define DPK_D 128
#define DPK_NH 4
#define DPK_TILE_ID 4
namespace dpkw4 {
#include "dpk_sampler.inc"
#include "dpk_genfused.inc"
}  // namespace dpkw4
#undef DPK_TILE_ID
#undef DPK_NH
#undef DPK_D
#undef DPK_P
// ... and at hid 64 / 2 heads (d_k 32; the generic-shape tests' width) and hid 64 / 4 heads (d_k 16), 4-pose
// tiles (129 KB of LDS)
#define DPK_P 4
#define DPK_D 64
#define DPK_NH 2
#define DPK_TILE_ID 5
namespace dpkn {
#include "dpk_sampler.inc"
#include "dpk_genfused.inc"
}  // namespace dpkn
#undef DPK_TILE_ID
#undef DPK_NH
#define DPK_NH 4
#define DPK_TILE_ID 6
namespace dpkn4 {
#include "dpk_sampler.inc"
#include "dpk_genfused.inc"
}  // namespace dpkn4
#undef DPK_TILE_ID
#undef DPK_NH
#undef DPK_D
#undef DPK_P

namespace dpk {

// ---------------------------------------------------------------------------------------
// Elementwise DDIM update for externally computed eps; z from the caller's draws of this step
// (`noise`, n floats) or counter-based.  xt and xn may be one array (a caller's x = update(x), as dpkg::ddim runs
// the per-op loop): neither is __restrict__.
__global__ void __launch_bounds__(256) ddim_kernel(const float* xt, const float* __restrict__ et,
                                                   float* xn, float* __restrict__ x0o, long long n,
                                                   const float* __restrict__ cf, int step, float eta,
                                                   unsigned long long seed, const float* __restrict__ noise) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float z = noise ? noise[i] : (eta != 0.f ? normal_noise(seed, step, i) : 0.f);
    float x0, x1;
    ddim_elem(cf, xt[i], et[i], z, x0, x1);
    xn[i] = x1;
    if (x0o) x0o[i] = x0;
}

}  // namespace dpk

// =======================================================================================
// Host side: handle, weight repacking, schedule, launches (the C ABI of diffpose_kernels.h)
// =======================================================================================
using namespace dpk;

// One DDIM schedule on the device, immutable once built: the step scalars coef [K][6] and the
// per-step timestep projections tps [K][NL][D] = temb_proj_l(swish(temb(t_s))) (they depend only
// on the weights and the schedule; SURVEY a7: batch-invariant).  dpk_set_schedule builds a new one
// instead of rewriting the old, so a launch still in flight (or a captured graph) keeps reading
// the schedule it was launched with; the old one is freed once every stream that used it has
// passed its last launch (an event per stream), or never if a graph was captured with it.
struct Sched {
    uint64_t serial = 0;           // unique per schedule built (keys the generic path's loop graphs)
    float* buf = nullptr;          // device: coef, then tps (16-byte aligned), then qtab
    float* coef = nullptr;
    float* tps = nullptr;
    float* qtab = nullptr;         // device: the noising roots [nt][2] (sched_roots), behind tps
    int nt = 0;                    // timesteps of the alpha table: n_alpha - 1
    int K = 0;
    float eta = 0.f;
    std::vector<float> h_coef;
    std::vector<float> h_qtab;     // qtab on the host (start_spec reads it)
    uint64_t tps_gen = 0;          // weights generation tps was computed from (0: not yet)
    int pins = 0;                  // captured graphs that read it (CapRes): kept while any is alive
    std::vector<std::pair<hipStream_t, hipEvent_t>> uses;   // last launch on each stream
};

// What the launches captured in one stream capture (one hipGraph) read by address: the schedules
// they were captured with, scratch buffers (dpk_scratch.inc: one per capturing stream, the captured
// launches of one stream are sequential graph nodes and share it) and step-split flag slots (one
// per capturing stream likewise).  A HIP user object retained by the capture's graph drops the
// graph's reference when the graph and its executable instances are destroyed (host callback, no
// HIP calls); the handle's next uncaptured call then waits for the device once and recycles the
// resources.  Where the runtime cannot retain one, they are kept until dpk_destroy.
struct CapRes {
    unsigned long long id = 0;                 // capture sequence id (hipStreamGetCaptureInfo_v2)
    std::atomic<int> refs{1};                  // the handle's reference (+1 while a graph holds one)
    std::atomic<bool> released{false};
    bool tracked = false;                      // a graph retains our user object
    std::vector<Sched*> scheds;
    std::vector<ScratchBuf> bufs;              // scratch per capturing stream (taken from the pool's spare)
    std::vector<std::pair<hipStream_t, int>> slots;   // flag slot per capturing stream
};
static void cap_release_cb(void* p) {
    CapRes* c = static_cast<CapRes*>(p);
    c->released.store(true);
    if (c->refs.fetch_sub(1) == 1) delete c;
}

// The weights of a handle that runs a sampler instance, as that instance reads them
struct InstWeights {
    const SamplerInst* inst = nullptr;   // null: a per-op handle (dpk_handle::gen)
    Packed pk;                     // the arenas packed from the handle's staging (inst->pack), as uploaded
    float* arena = nullptr;        // device: packed weights + graph constants
    float* temb = nullptr;         // device: timestep-MLP weights
    char* arena16 = nullptr;       // device: split-fp16 GEMM weights (gemm mode 1; instances that have the mode)
    char* arenabf = nullptr;       // device: bf16 GEMM weights (gemm mode 2), same layout
};

struct GenModel;   // dpk_generic.inc: the per-op forward for model shapes no instance is compiled for
struct BwdModel;   // dpk_generic_bwd.inc: what dpk_diff_loss_grad keeps (built on its first call)
struct TrainState; // dpk_train.inc: the device-side optimiser's arrays, between dpk_train_begin and dpk_train_end
struct dpk_handle {
    int device = 0;
    GenModel* gen = nullptr;       // non-null: this handle's shape runs on the per-op path (then w.inst is null)
    int n_pts = J;                 // joints of the handle's model
    int kind = 0;                  // 0: GCNdiff (coords 5->5), 1: GCNpose (coords 2->3)
    int num_layers = NL;           // config num_layer (1..NL): layers the kernels run
    int n_cu = 256;                // compute units of the device (workgroups per round)
    int tail_plan = 2;             // dpk_set_tail_plan: 0 4-pose tiles, 1 2-pose tail round, 2 step split
    unsigned* flags = nullptr;     // device: FLAG_SLOTS x n_cu step-split handoff words (zero between launches),
                                   // then the split fallback counter
    std::vector<int> slot_free;    // flag slots no launch holds
    std::vector<std::pair<int, hipEvent_t>> slot_busy;   // uncaptured launches: slot until its event completes
    std::vector<hipEvent_t> slot_ev;   // idle events for slot_busy
    int split_dbg = 0;             // dpk_debug_split mode
    unsigned token = 0;            // per-launch handoff token (30 bits, never 0)
    std::vector<CapRes*> caps;     // resources of captured launches (per capture)
    std::string err;
    InstWeights w;                 // the sampler instance serving this handle and its weights
    float* tproj_zero = nullptr;   // device: [NL][D] zeros (GCNpose: no timestep projection)
    hipStream_t aux = nullptr;     // handle-internal stream for schedule construction
    uint64_t weights_gen = 0;      // bumped by every weight/graph upload
    Sched* sched = nullptr;        // current schedule
    std::vector<Sched*> retired;   // replaced schedules not yet known to be unused
    ScratchPool pool;              // timestep projections of dpk_eps (and dpk_sample, !sched_tps) or per-op scratch
    Stage stage;                   // host staging of the weights and the graph, whatever the shape
    uint64_t stage_serial = 0;     // bumped whenever the staging is uploaded anew (pack_upload)
    BwdModel* bwd = nullptr;       // dpk_diff_loss_grad's arenas (and, on a sampler instance, its per-op model)
    TrainState* train = nullptr;   // non-null: training (dpk_train_begin); the device holds the weights, the staging lags
    int gemm_mode = 0;             // 0: fp32 MFMA, 1: 3x fp16-split MFMA, 2: bf16 MFMA (dpk_set_gemm_mode)
    int tile_waves = 0;            // dpk_set_tile_waves: 4 or 8 waves on the 4-pose tiles of dpk_sample; 0 the mode's default
    bool have_graph = false, have_weights = false;
    unsigned mask = (1u << J) - 1u;
    const unsigned* pmask = nullptr;   // dpk_set_pose_masks: caller-owned device array
    int pmask_n = 0;
    bool profiling = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_used, ev_free;
    std::vector<uint32_t> kernels;   // the launch census: distinct sample_kernel ids since dpk_debug_sampler_kernels read them
#if DPK_TRACE
    unsigned long long* trace = nullptr;
    size_t trace_len = 0;
    int trace_step = -1;
#endif
};

static int fail(dpk_handle* h, int code, const std::string& msg) {
    if (h) h->err = msg;
    return code;
}

// Does the handle's model ride padded in its instance's tiles (fewer joints than the tile's 17)?
static bool padded(const dpk_handle* h) { return h->w.inst && h->n_pts != h->w.inst->J; }

// The gemm modes the handle's path runs, bit m for mode m: its sampler instance's (a padded handle: without bf16,
// whose kernels are built for 17 joints alone), or fp32 alone per op
static int gemm_modes(const dpk_handle* h) { return h->w.inst ? (padded(h) ? h->w.inst->modes & 3 : h->w.inst->modes) : 1; }

// `launch` (returns a DPK code) on `st`, between an event pair when the handle is profiling (dpk_profile;
// never under a capture)
template <class F>
static int profiled(dpk_handle* h, hipStream_t st, bool cap, const char* who, F launch) {
    if (!h->profiling || cap) return launch();
    if (h->ev_free.empty()) {
        hipEvent_t a, b;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess)
            return fail(h, DPK_E_HIP, std::string(who) + ": event record");
        h->ev_free.push_back({a, b});
    }
    const std::pair<hipEvent_t, hipEvent_t> ev = h->ev_free.back();
    h->ev_free.pop_back();
    if (hipEventRecord(ev.first, st) != hipSuccess) return fail(h, DPK_E_HIP, std::string(who) + ": event record");
    const int rc = launch();
    if (rc) return rc;
    if (hipEventRecord(ev.second, st) != hipSuccess) return fail(h, DPK_E_HIP, std::string(who) + ": event record");
    h->ev_used.push_back(ev);
    return DPK_OK;
}

#define HIPCHK(h, expr)                                                                        \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail((h), DPK_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));    \
    } while (0)

// Is `st` capturing a graph right now?  (Launches then become graph nodes: nothing may be
// allocated or freed, and the schedule they read must outlive the graph.)
static int capturing(dpk_handle* h, hipStream_t st, bool* cap) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    HIPCHK(h, hipStreamIsCapturing(st, &cs));
    *cap = cs != hipStreamCaptureStatusNone;
    return DPK_OK;
}

static void sched_free(Sched* s) {
    if (s->buf) (void)hipFree(s->buf);
    for (auto& u : s->uses) (void)hipEventDestroy(u.second);
    delete s;
}

// Free the retired schedules whose every recorded use has completed (never one a live graph reads).
static void sched_sweep(dpk_handle* h) {
    std::vector<Sched*> keep;
    for (Sched* s : h->retired) {
        bool done = s->pins == 0;
        for (auto& u : s->uses) done = done && hipEventQuery(u.second) == hipSuccess;
        if (done) sched_free(s);
        else keep.push_back(s);
    }
    h->retired.swap(keep);
}

// The CapRes of the capture `st` is recording into (created on its first captured launch).
static int cap_get(dpk_handle* h, hipStream_t st, CapRes** out) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    unsigned long long id = 0;
    hipGraph_t graph = nullptr;
    HIPCHK(h, hipStreamGetCaptureInfo_v2(st, &cs, &id, &graph, nullptr, nullptr));
    for (CapRes* c : h->caps)
        if (c->id == id) {
            *out = c;
            return DPK_OK;
        }
    CapRes* c = new CapRes();
    c->id = id;
    // hand the graph a user object that releases the resources with it (DPK_CAPTURE_RELEASE=0: keep them
    // until dpk_destroy instead)
    const char* env = getenv("DPK_CAPTURE_RELEASE");
    if (graph && !(env && atoi(env) == 0)) {
        c->refs.fetch_add(1);              // the graph's reference (dropped by cap_release_cb)
        hipUserObject_t obj = nullptr;
        if (hipUserObjectCreate(&obj, c, cap_release_cb, 1, hipUserObjectNoDestructorSync) != hipSuccess) {
            c->refs.fetch_sub(1);
            (void)hipGetLastError();
        } else if (hipGraphRetainUserObject(graph, obj, 1, hipGraphUserObjectMove) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipUserObjectRelease(obj, 1);   // runs the callback: drops the graph's reference
        } else {
            c->tracked = true;
        }
    }
    h->caps.push_back(c);
    *out = c;
    return DPK_OK;
}

static void slot_put(dpk_handle* h, int slot) { h->slot_free.push_back(slot); }

// Wait for the device in relaxed capture mode: a thread capturing in global mode (torch.cuda.graph's
// default) would otherwise see this potentially unsafe call invalidate its capture.  false (error
// cleared) if the runtime refuses the sync, e.g. while a stream of the device is capturing.
static bool drain_relaxed() {
    hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
    const bool exch = hipThreadExchangeStreamCaptureMode(&mode) == hipSuccess;
    const hipError_t se = hipDeviceSynchronize();
    if (exch) (void)hipThreadExchangeStreamCaptureMode(&mode);
    if (se != hipSuccess) (void)hipGetLastError();
    return se == hipSuccess;
}

// Uncaptured calls only: recycle the resources of captures whose graphs are gone.  No drain: the release
// callback runs when the graph's executable is destroyed, and on this runtime destroying an executable
// waits for its launches in flight (tools/probe_user_object_release.py: deleting a CUDAGraph 0.1 ms after
// its 175 ms replay was enqueued returned when the replay had finished, and `released` was never seen
// set while it ran), so nothing the capture reads is still in use.  A drain here, even in relaxed capture
// mode, invalidates another thread's global-mode capture on this runtime (round 4 without the relaxed
// mode, advisor r04; round 6 with it, ADVICE r05: test_sweep_while_another_thread_captures failed with
// hipErrorStreamCaptureInvalidated), so the recycling relies on that blocking destruction.
static void cap_sweep(dpk_handle* h) {
    bool any = false;
    for (CapRes* c : h->caps) any = any || (c->tracked && c->released.load());
    if (!any) return;
    std::vector<CapRes*> keep;
    for (CapRes* c : h->caps) {
        if (!(c->tracked && c->released.load())) {
            keep.push_back(c);
            continue;
        }
        for (Sched* s : c->scheds) --s->pins;
        scratch_release(h->pool, c->bufs);
        for (auto& s : c->slots) slot_put(h, s.second);
        if (c->refs.fetch_sub(1) == 1) delete c;
    }
    h->caps.swap(keep);
    sched_sweep(h);
}

// After enqueuing a launch that reads `s` on `st`: pin it to the capture if the launch was
// captured, else record its completion on that stream.
static int sched_note_use(dpk_handle* h, Sched* s, hipStream_t st, bool cap) {
    if (cap) {
        CapRes* c = nullptr;
        const int rc = cap_get(h, st, &c);
        if (rc) return rc;
        if (std::find(c->scheds.begin(), c->scheds.end(), s) == c->scheds.end()) {
            c->scheds.push_back(s);
            ++s->pins;
        }
        return DPK_OK;
    }
    hipEvent_t ev = nullptr;
    for (auto& u : s->uses)
        if (u.first == st) ev = u.second;
    if (!ev) {
        HIPCHK(h, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        s->uses.push_back({st, ev});
    }
    HIPCHK(h, hipEventRecord(ev, st));
    return DPK_OK;
}

// tps of `s` from the current weights, on the handle's own stream; returns once they are written
static int sched_compute_tps(dpk_handle* h, Sched* s) {
    h->w.inst->temb(h->w.temb, s->coef + 5, 6, s->K, s->tps, h->aux);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->aux));
    s->tps_gen = h->weights_gen;
    return DPK_OK;
}

// Does the handle's instance read dpk_sample's timestep projections from the schedule (SamplerInst::sched_tps)?
static bool sched_tps(const dpk_handle* h) { return h->w.inst && h->w.inst->sched_tps; }

// The arenas packed for the handle's instance (h->w.pk), to the device
static int upload(dpk_handle* h) {
    HIPCHK(h, hipSetDevice(h->device));
    // launches already enqueued on any stream may still read the arena: overwrite it only after
    // the device has drained (weights and graphs are loaded rarely; the launches stay async)
    HIPCHK(h, hipDeviceSynchronize());
    // every uncaptured launch has completed: the retired schedules only they used go now, so the
    // projections below are recomputed for the current schedule and the graph-pinned ones only
    sched_sweep(h);
    InstWeights& w = h->w;
    if (!w.arena) HIPCHK(h, hipMalloc(&w.arena, w.inst->arena_floats * 4));
    if (!w.temb) HIPCHK(h, hipMalloc(&w.temb, w.inst->temb_floats * 4));
    HIPCHK(h, hipMemcpy(w.arena, w.pk.arena.data(), w.inst->arena_floats * 4, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(w.temb, w.pk.temb.data(), w.inst->temb_floats * 4, hipMemcpyHostToDevice));
    if (w.inst->has_mode(1)) {
        if (!w.arena16) HIPCHK(h, hipMalloc(&w.arena16, w.inst->arena16_bytes));
        HIPCHK(h, hipMemcpy(w.arena16, w.pk.a16.data(), w.inst->arena16_bytes, hipMemcpyHostToDevice));
    }
    if (w.inst->has_mode(2)) {
        if (!w.arenabf) HIPCHK(h, hipMalloc(&w.arenabf, w.inst->arenabf_bytes));
        HIPCHK(h, hipMemcpy(w.arenabf, w.pk.abf.data(), w.inst->arenabf_bytes, hipMemcpyHostToDevice));
    }
    ++h->weights_gen;
    if (!h->have_weights || h->kind != 0 || !sched_tps(h)) return DPK_OK;
    // every live schedule (current, retired, pinned by a graph) follows the new weights
    if (h->sched) {
        const int rc = sched_compute_tps(h, h->sched);
        if (rc) return rc;
    }
    for (Sched* s : h->retired) {
        const int rc = sched_compute_tps(h, s);
        if (rc) return rc;
    }
    return DPK_OK;
}

// Flag slots of step-split launches (launch_sampler).  No two launches that may overlap share a slot:
// an uncaptured launch holds one until an event recorded behind it has completed (checked at the
// next launch), a captured one for the life of its graph (shared by the captured launches of one
// stream, which are sequential graph nodes; every launch leaves its words at 0).  -1 when all are
// held (the caller then runs the 2-pose tail plan).
constexpr int FLAG_SLOTS = 64;
static int split_slot(dpk_handle* h, hipStream_t st, bool cap) {
    if (!h->flags) return -1;
    if (cap) {
        CapRes* c = nullptr;
        if (cap_get(h, st, &c)) return -1;
        for (auto& s : c->slots)
            if (s.first == st) return s.second;
        if (h->slot_free.empty()) return -1;
        const int slot = h->slot_free.back();
        h->slot_free.pop_back();
        c->slots.push_back({st, slot});
        return slot;
    }
    std::vector<std::pair<int, hipEvent_t>> busy;
    for (auto& b : h->slot_busy) {
        if (hipEventQuery(b.second) == hipSuccess) {
            h->slot_free.push_back(b.first);
            h->slot_ev.push_back(b.second);
        } else {
            busy.push_back(b);
        }
    }
    (void)hipGetLastError();          // hipEventQuery's hipErrorNotReady
    h->slot_busy.swap(busy);
    if (h->slot_free.empty()) return -1;
    const int slot = h->slot_free.back();
    h->slot_free.pop_back();
    return slot;
}
// after an uncaptured launch that used `slot` on `st`
static int split_slot_hold(dpk_handle* h, int slot, hipStream_t st) {
    hipEvent_t ev = nullptr;
    if (!h->slot_ev.empty()) {
        ev = h->slot_ev.back();
        h->slot_ev.pop_back();
    } else if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
        h->slot_free.push_back(slot);    // the launch is enqueued; a later launch reusing the slot is
        HIPCHK(h, hipStreamSynchronize(st));   // safe once this one has finished
        return DPK_OK;
    }
    h->slot_busy.push_back({slot, ev});
    HIPCHK(h, hipEventRecord(ev, st));
    return DPK_OK;
}

// Waves on the 4-pose tiles of a dpk_sample launch: the handle's choice (dpk_set_tile_waves), else the GEMM
// mode's default (the paired measurements per mode).
// fp32 +1.2 %, bf16 (config 3) +1.5 % on 8 waves, every one of 5 interleaved pairs faster; f16x3 -6 %: both
// waves of a SIMD split the same activation rows into fp16 hi + lo (profiles/w8_ab_*.txt)
constexpr int TILE_WAVES_DEFAULT[3] = {8, 4, 8};   // fp32, f16x3, bf16
// A graph outside the compiled H36M pattern (the dense Chebyshev path) defaults to 4 waves in every mode: its
// 8-wave kernels do not fit 256 registers (442-532 spilled VGPRs, profiles/w8_resource_usage.txt; the 4-wave
// dense kernels already fill 512) and were not measured; they run on explicit request only.
static int tile_waves(const dpk_handle* h) {
    if (h->tile_waves) return h->tile_waves;
    return h->w.pk.sparse ? TILE_WAVES_DEFAULT[h->gemm_mode] : 4;
}

// One launch of kernel mode `mode` on the instance `tile` (the handle's, or a sibling tile of it) for the
// handle's graph pattern and GEMM mode.
static void launch_tiles(dpk_handle* h, const SamplerInst* tile, int mode, int blocks, size_t shmem, hipStream_t st,
                         const SampleArgs& a) {
    const char* a16 = h->gemm_mode == 2 ? h->w.arenabf : h->w.arena16;
    dpk_shared::last_kernel = dpk_shared::KERNEL_NONE;
    tile->launch[mode](h->w.pk.sparse, h->gemm_mode, blocks, shmem, st, a, h->w.arena, a16);
    // the census: what the launch site said it launched (or recorded into a capture), not what was asked for above
    const uint32_t id = dpk_shared::last_kernel;
    if (id != dpk_shared::KERNEL_NONE && std::find(h->kernels.begin(), h->kernels.end(), id) == h->kernels.end())
        h->kernels.push_back(id);
}

// The sampler over a.N poses.  One 4-pose workgroup per CU per round; a partial last round of r
// tiles would cost a whole round.  Plan 2 (sample mode, at least one full round before it,
// r <= n_cu / 2): each of those tiles runs steps [0, K/2) and [K/2, K) on two workgroups, one
// launch of full + 2r blocks ordered [first halves | full tiles | second halves].  The dispatcher
// starts blocks in order as CUs free up, so the first halves run beside the first full round and
// the second halves after the last one: the tail costs half a round, and a second half only ever
// waits for a block numbered below it (no deadlock for any CU count).  E.g. config 5's 2,560
// poses per GPU = 640 tiles: 2.5 round times instead of 3.  Every tile runs the same per-step
// arithmetic, so the outputs are bitwise those of plan 0.
// Plan 1 (and plan 2 where it does not apply): when the last round would leave at least half the
// CUs idle (at most 2 poses per CU remain) those poses run as 2-pose workgroups (dpk2, about 0.6
// of a 4-pose tile's time), one per CU, in a second launch after the full rounds.  Each
// workgroup's result depends only on its own poses.
// Both plans need the 2-pose sibling (plan 2 falls back on plan 1): an instance without one (the other
// widths) runs ceil(N / P) of its tiles in one launch, and so does a padded handle of any instance (the sibling
// tiles have no padded kernels).
static int launch_sampler(dpk_handle* h, int mode, hipStream_t st, SampleArgs a, bool cap) {
    const SamplerInst* in = h->w.inst;
    const int N = a.N, P = in->P;
    if (!in->tail2 || padded(h)) {
        launch_tiles(h, in, mode, (N + P - 1) / P, 0, st, a);
        HIPCHK(h, hipGetLastError());
        return DPK_OK;
    }
    // every 4-pose tile of a dpk_sample launch, step-split halves included, on one instance; dpk_eps and
    // dpk_pose stay on 4 waves
    const SamplerInst* tile = mode == M_SAMPLE && in->wave8 && tile_waves(h) == 8 ? in->wave8 : in;
    const int round4 = P * h->n_cu;
    if (mode == M_SAMPLE) {
        const int tiles = (N + P - 1) / P, q = tiles / h->n_cu, r = tiles % h->n_cu;
        if (h->tail_plan == 2 && a.K >= 2 && q >= 1 && r > 0 && 2 * r <= h->n_cu) {
            const int slot = split_slot(h, st, cap);
            if (slot >= 0) {
                a.pose_off = 0;
                a.split_n = r;
                a.split_k = a.K / 2;
                a.split_full = q * h->n_cu;
                a.flags = h->flags + (size_t)slot * h->n_cu;
                a.split_stats = reinterpret_cast<int*>(h->flags + (size_t)FLAG_SLOTS * h->n_cu);
                a.split_dbg = h->split_dbg;
                h->token = (h->token + 1) & 0x3fffffffu;
                if (h->token == 0) h->token = 1;
                a.token = h->token;
                launch_tiles(h, tile, mode, q * h->n_cu + 2 * r, 0, st, a);
                HIPCHK(h, hipGetLastError());
                return cap ? DPK_OK : split_slot_hold(h, slot, st);
            }
        }
    }
    int n4 = N;
    const int rem = N % round4;
    if (h->tail_plan >= 1 && rem != 0 && rem <= 2 * h->n_cu) n4 = N - rem;
    if (n4 > 0) {
        a.pose_off = 0;
        launch_tiles(h, tile, mode, (n4 + P - 1) / P, 0, st, a);
    }
    if (n4 < N) {
        // pad the 2-pose kernel's LDS past half a CU's so the dispatcher places one per CU
        const int P2 = in->tail2->P;
        const size_t half = 160 * 1024 / 2, lds2 = (size_t)in->tail2->lds_bytes;
        const size_t pad = lds2 > half ? 0 : half - lds2 + 256;
        a.pose_off = n4;
        launch_tiles(h, in->tail2, mode, (N - n4 + P2 - 1) / P2, pad, st, a);
    }
    HIPCHK(h, hipGetLastError());
    return DPK_OK;
}

// n floats of scratch for one call (dpk_scratch.inc): the stream's own buffer, the spare grown alongside, or
// under a capture that capture's.  A captured call that cannot be served returns DPK_E_STATE with `why` and,
// in `got`, the capacity that fell short; the caller words the refusal (poses in dpk_eps, floats on the
// generic path).
static int call_scratch(dpk_handle* h, hipStream_t st, bool cap, size_t n, const char* who, ScratchBuf& got,
                        ScratchStatus& why) {
    why = SCRATCH_OK;
    if (!cap) {
        got = ScratchBuf{st, scratch_get(h->pool, st, n), n};
        if (got.p) return DPK_OK;
        return fail(h, DPK_E_HIP, std::string(who) + ": scratch of " + std::to_string(n) + " floats: " +
                                      hipGetErrorString(hipGetLastError()));
    }
    CapRes* c = nullptr;
    const int rc = cap_get(h, st, &c);
    if (rc) return rc;
    why = scratch_get_captured(h->pool, c->bufs, st, n, got);
    return why == SCRATCH_OK ? DPK_OK : DPK_E_STATE;
}

// Launch arguments of one eps / sample / pose call over N poses, for whichever sampler instance `arena` was
// packed for: tproj per pose, per step of `sc`, or zeros.
static SampleArgs eps_args(const dpk_handle* h, const float* arena, const float* tproj, const float* x, float* out,
                           int N) {
    SampleArgs a{};
    a.arena = arena;
    a.tproj = tproj;
    a.x_in = x;
    a.x_out = out;
    a.N = N;
    a.K = 1;
    a.mask = h->mask;
    a.pmask = h->pmask;
    a.num_layers = h->num_layers;
    a.n_pts = h->n_pts;
    return a;
}
static SampleArgs sample_args(const dpk_handle* h, const float* arena, const float* tproj, const Sched* sc,
                              const float* x, float* out, float* xs, float* x0s, int N, uint64_t seed,
                              const float* noise) {
    SampleArgs a = eps_args(h, arena, tproj, x, out, N);
    a.coef = sc->coef;
    a.K = sc->K;
    a.eta = sc->eta;
    a.xs = xs;
    a.x0s = x0s;
    a.seed = seed;
    a.noise = noise;
    return a;
}
// The hypothesis start of one dpk_sample_start / dpk_q_sample call (start_spec): the two scalars of
// alpha_bar[t_start + 1], the scale rows and the caller's draws (null: counter-based)
struct StartSpec {
    float sa, sb;
    const float* scale;
    int rows;
    const float* noise;
};
static SampleArgs pose_args(const dpk_handle* h, const float* arena, const float* zeros, const float* x2d, float* xyz,
                            float* uvxyz, int N, int H, int root_mode) {
    SampleArgs a = eps_args(h, arena, zeros, x2d, xyz, N);
    a.uvxyz = uvxyz;
    a.H = H;
    a.root_mode = root_mode;
    return a;
}

#include "dpk_generic.inc"
#include "dpk_grad_layout.inc"
#include "dpk_generic_bwd.inc"
#include "dpk_train_layout.inc"
#include "dpk_train.inc"

// ---------------------------------------------------------------------------------------
// The compiled sampler instances: which shapes have a fused kernel, on which tile, with which kernel modes.
// First the launchers that exist, instantiated explicitly: these and no others (a mode not listed for an
// instance is a null pointer in its descriptor below; naming it there would compile kernels nobody runs).
// The kernels stand in the code object in this list's order, however the host code is arranged.
#define DPK_LAUNCHER(ns, MODE)                                                                                  \
    template void ns::launch_sample<MODE>(bool, int, int, size_t, hipStream_t, const SampleArgs&, const float*, \
                                          const char*);
DPK_LAUNCHER(dpkw, M_SAMPLE) DPK_LAUNCHER(dpkw4, M_SAMPLE) DPK_LAUNCHER(dpkn, M_SAMPLE) DPK_LAUNCHER(dpkn4, M_SAMPLE)
DPK_LAUNCHER(dpkw, M_EPS) DPK_LAUNCHER(dpkw4, M_EPS) DPK_LAUNCHER(dpkn, M_EPS) DPK_LAUNCHER(dpkn4, M_EPS)
DPK_LAUNCHER(dpk, M_EPS) DPK_LAUNCHER(dpk2, M_EPS)
DPK_LAUNCHER(dpk8, M_SAMPLE) DPK_LAUNCHER(dpk, M_SAMPLE) DPK_LAUNCHER(dpk2, M_SAMPLE)
DPK_LAUNCHER(dpk, M_POSE) DPK_LAUNCHER(dpk2, M_POSE)
#undef DPK_LAUNCHER

// The descriptors: {shape half, timestep MLP, kernel list, {M_SAMPLE, M_EPS, M_POSE}, 8-wave sibling, 2-pose sibling, sched_tps}
#define DPK_INST(ns, ...) \
    namespace ns { constexpr SamplerInst INST = {SHAPE, fused_temb, list_kernels, __VA_ARGS__}; }
// the shipped shape (hid 96 / 4 heads): its 8-wave and 2-pose tiles are reached through the 4-pose tile's entry
DPK_INST(dpk8, {launch_sample<M_SAMPLE>, nullptr, nullptr}, nullptr, nullptr, true)
DPK_INST(dpk2, {launch_sample<M_SAMPLE>, launch_sample<M_EPS>, launch_sample<M_POSE>}, nullptr, nullptr, true)
DPK_INST(dpk, {launch_sample<M_SAMPLE>, launch_sample<M_EPS>, launch_sample<M_POSE>}, &dpk8::INST, &dpk2::INST, true)
// hid 128 / 8 and 4 heads (2-pose tiles), hid 64 / 2 and 4 heads (4-pose tiles): GCNdiff, gemm modes 0 and 1
DPK_INST(dpkw, {launch_sample<M_SAMPLE>, launch_sample<M_EPS>, nullptr}, nullptr, nullptr, false)
DPK_INST(dpkw4, {launch_sample<M_SAMPLE>, launch_sample<M_EPS>, nullptr}, nullptr, nullptr, false)
DPK_INST(dpkn, {launch_sample<M_SAMPLE>, launch_sample<M_EPS>, nullptr}, nullptr, nullptr, false)
DPK_INST(dpkn4, {launch_sample<M_SAMPLE>, launch_sample<M_EPS>, nullptr}, nullptr, nullptr, false)
#undef DPK_INST

// dpk_create gives a handle the first entry that fits its config; a config none fits runs per op (GenModel)
// A GCNdiff model of fewer than 17 joints fits its width's entry as padded tiles (InstShape::fits) and gets it
// from DPK_PAD_MIN joints up: the smallest measured count from which upward the padded tile beat the per-op path by
// more than 1 % at hid 96 / 4 x 5 layers, hid 128 / 8 x 5 and hid 64 / 2 x 2 alike (B=1024, K=50, fp32, medians of 9
// alternating pairs; profiles/padded_joints_bench.txt).  A padded tile costs what 17 joints cost, the per-op path
// grows with the rows: hid 96 and hid 64 won from the smallest count measured (4: 0.77, 0.57 of the per-op time),
// the 2-pose tiles of hid 128 from 7 (0.93; 1.03 at 6, 1.26 at 4), so one constant for every width is 7
constexpr int DPK_PAD_MIN = 7;
constexpr const SamplerInst* INSTANCES[] = {&dpk::INST, &dpkw::INST, &dpkw4::INST, &dpkn::INST, &dpkn4::INST};
constexpr bool instances_consistent() {
    for (const SamplerInst* i : INSTANCES) {
        // what fits promises (shape half, checked on the CPU) is what is compiled, on the tail tile too
        for (const SamplerInst* t : {i, i->tail2 ? i->tail2 : i})
            if (!t->launch[M_SAMPLE] || !t->launch[M_EPS] || (t->launch[M_POSE] != nullptr) != i->pose) return false;
        if (i->wave8 && !i->wave8->launch[M_SAMPLE]) return false;
    }
    return true;
}
static_assert(instances_consistent(), "an instance's fits and its compiled kernel modes disagree");

// Scratch for dpk_eps's per-pose projections [N][NL][D] (dpk_diff_loss on an instance takes the same).  Where the
// schedule holds dpk_sample's they are all the pool serves: at least 64 poses, refusals in poses (but for the
// three-launch A/B form of dpk_diff_loss, DPK_LOSS_FUSED=0, which asks in floats).  Elsewhere it is counted in floats
// (gen_scratch).
static int eps_scratch(dpk_handle* h, hipStream_t st, bool cap, int N, float** out) {
    const size_t PP = h->w.inst->tp;
    if (!sched_tps(h)) return gen_scratch(h, st, cap, (size_t)N * PP, out, "dpk_eps");
    ScratchBuf buf;
    ScratchStatus why;
    const int rc = call_scratch(h, st, cap, (size_t)(cap ? N : std::max(N, 64)) * PP, "dpk_eps", buf, why);
    *out = buf.p;
    if (why == SCRATCH_NO_SPARE)
        return fail(h, rc, "dpk_eps: a captured call needs a projection buffer of " + std::to_string(N) +
                               " poses, and the spare holds " + std::to_string(buf.cap / PP) +
                               "; make an uncaptured dpk_eps call of >= N poses before the capture");
    if (why == SCRATCH_SHARED_TOO_SMALL)
        return fail(h, rc, "dpk_eps: the captured calls of one stream share the buffer of the capture's "
                           "first call (" + std::to_string(buf.cap / PP) + " poses); this one has " +
                               std::to_string(N) + "; warm up with the largest N before capturing");
    return rc;
}

// What dpk_eps, dpk_sample and dpk_pose do once their arguments and the handle's state have passed: the
// per-pose masks cover the N poses (models/GraFormer.py:107-108 broadcasts [N,1,17]), the handle's device is
// current, and an uncaptured call recycles what destroyed graphs have released.
static int enter_call(dpk_handle* h, int N, const char* who, hipStream_t st, bool* cap) {
    if (h->pmask && N > h->pmask_n)
        return fail(h, DPK_E_INVALID, std::string(who) + ": " + std::to_string(N) + " poses but dpk_set_pose_masks covers " +
                                          std::to_string(h->pmask_n));
    HIPCHK(h, hipSetDevice(h->device));
    const int rc = capturing(h, st, cap);
    if (rc) return rc;
    if (!*cap) cap_sweep(h);
    return DPK_OK;
}

extern "C" {

int dpk_version(void) { return 105; }

int dpk_kernel_geometry(int* ppw, int* tpw, int* lds) {
    if (ppw) *ppw = P;
    if (tpw) *tpw = NT;
    if (lds) *lds = SM_FLOATS * 4;
    return DPK_OK;
}

int dpk_create(const dpk_config* cfg, dpk_handle** out) {
    if (!cfg || !out) return DPK_E_INVALID;
    *out = nullptr;
    const bool pose_io = cfg->coords_in == CIN_POSE && cfg->coords_out == COUT_POSE;
    if (cfg->hid_dim < 2 || cfg->n_head < 1 || cfg->hid_dim % cfg->n_head != 0 || cfg->num_layers < 1 ||
        cfg->n_pts < 2 || cfg->n_pts > dpkg::GJ_MAX || cfg->coords_in < 1 || cfg->coords_out < 1)
        return DPK_E_UNSUPPORTED;
    // GCNpose: coords 2 -> 3; GCNdiff: x and eps share a shape (coords in == out)
    int kind;
    if (pose_io) kind = 1;
    else if (cfg->coords_in == cfg->coords_out) kind = 0;
    else return DPK_E_UNSUPPORTED;
    // GCNdiff's timestep embedding spreads hid_dim / 2 frequencies over log(10000) / (hid_dim / 2 - 1)
    // (models/gcndiff.py:15-33): hid_dim 2 and 3 divide by zero there (the reference raises ZeroDivisionError;
    // gen_temb would hand out NaN).  GCNpose never evaluates the embedding.
    if (kind == 0 && cfg->hid_dim < 4) return DPK_E_UNSUPPORTED;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device < 0 || cfg->device >= ndev) return DPK_E_HIP;
    dpk_handle* h = new dpk_handle();
    h->device = cfg->device;
    h->kind = kind;
    h->num_layers = cfg->num_layers;
    h->n_pts = cfg->n_pts;
    h->mask = cfg->n_pts >= 32 ? ~0u : (1u << cfg->n_pts) - 1u;   // every key attends (all-ones src_mask)
    stage_init(h->stage, cfg->hid_dim, cfg->n_head, cfg->n_pts, cfg->num_layers, cfg->coords_in, cfg->coords_out, kind);
    // a shape an instance is compiled for runs the persistent sampler; any other (hid_dim a multiple of n_head,
    // n_pts <= 32) the per-op path.  DPK_FORCE_GENERIC=1 sends every shape there, DPK_GEN_FUSED=0 the widths
    // other than the shipped one (A/B; tests compare the two paths)
    const char* fg = getenv("DPK_FORCE_GENERIC");
    const char* fe = getenv("DPK_GEN_FUSED");
    const bool no_inst = fg && atoi(fg) != 0, no_widths = fe && atoi(fe) == 0;
    // fewer joints than the tiles' 17 ride padded from DPK_PAD_MIN joints up (DPK_PAD_MIN_JOINTS=2: every count,
    // 17: none); below it the per-op path
    int pad_min = DPK_PAD_MIN;
    if (const char* pm = getenv("DPK_PAD_MIN_JOINTS")) pad_min = atoi(pm);
    const bool no_pad = cfg->n_pts != J && cfg->n_pts < pad_min;
    for (const SamplerInst* i : INSTANCES)
        if (!h->w.inst && !no_inst && !no_pad && !(no_widths && i != &dpk::INST) &&
            i->fits(cfg->hid_dim, cfg->n_head, cfg->n_pts, cfg->num_layers, cfg->coords_in, cfg->coords_out, kind))
            h->w.inst = i;
    if (!h->w.inst) {
        h->gen = gen_new(h->stage);
        h->pool.replaced = gen_scratch_replaced;   // its recorded loops are keyed by scratch address
        h->pool.ctx = h->gen;
    }
    if (hipSetDevice(h->device) != hipSuccess ||
        hipStreamCreateWithFlags(&h->aux, hipStreamNonBlocking) != hipSuccess ||
        hipDeviceGetAttribute(&h->n_cu, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess) {
        if (h->aux) (void)hipStreamDestroy(h->aux);
        gen_free(h->gen);
        delete h;
        return DPK_E_HIP;
    }
    h->n_cu = std::max(h->n_cu, 1);
    // DPK_TILE_WAVES=0/4/8: the initial tile instance (A/B timing)
    if (const char* tw = getenv("DPK_TILE_WAVES")) {
        const int v = atoi(tw);
        if (v == 0 || v == 4 || v == 8) h->tile_waves = v;
    }
    // DPK_TAIL_SPLIT=0/1/2: the initial tail plan (A/B timing); trace builds stamp per block id
    if (const char* ts = getenv("DPK_TAIL_SPLIT")) h->tail_plan = std::min(std::max(atoi(ts), 0), 2);
    if (DPK_TRACE) h->tail_plan = 0;
    // FLAG_SLOTS x n_cu handoff words + the fallback counter
    const size_t flag_bytes = ((size_t)FLAG_SLOTS * h->n_cu + 4) * 4;
    for (int s = FLAG_SLOTS - 1; s >= 0; --s) h->slot_free.push_back(s);
    if (hipMalloc(&h->flags, flag_bytes) != hipSuccess || hipMemset(h->flags, 0, flag_bytes) != hipSuccess) {
        if (h->flags) (void)hipFree(h->flags);
        (void)hipStreamDestroy(h->aux);
        gen_free(h->gen);
        delete h;
        return DPK_E_HIP;
    }
    *out = h;
    return DPK_OK;
}

void dpk_destroy(dpk_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    for (void* p : {(void*)h->w.arena, (void*)h->w.temb, (void*)h->w.arena16, (void*)h->w.arenabf})
        if (p) (void)hipFree(p);
    if (h->tproj_zero) (void)hipFree(h->tproj_zero);
    if (h->flags) (void)hipFree(h->flags);
    gen_free(h->gen);
    bwd_free(h->bwd);
    train_free(h->train);
    // hipFree waits for the device, so in-flight launches finish before their buffers go
    if (h->sched) sched_free(h->sched);
    for (Sched* s : h->retired) sched_free(s);
    scratch_free_all(h->pool);
    for (CapRes* c : h->caps) {
        scratch_free(c->bufs);
        // a graph still alive keeps the CapRes object (its callback touches only that)
        if (c->refs.fetch_sub(1) == 1) delete c;
    }
    for (auto& b : h->slot_busy) (void)hipEventDestroy(b.second);
    for (hipEvent_t e : h->slot_ev) (void)hipEventDestroy(e);
    if (h->aux) (void)hipStreamDestroy(h->aux);
    for (auto* v : {&h->ev_used, &h->ev_free})
        for (auto& e : *v) {
            (void)hipEventDestroy(e.first);
            (void)hipEventDestroy(e.second);
        }
    delete h;
}

const char* dpk_last_error(const dpk_handle* h) { return h ? h->err.c_str() : "null handle"; }

// Repack the handle's arenas from its staging and upload them (weights loaded; the graph's terms are zeros
// until dpk_set_graph).  Weights and graphs are loaded rarely, so everything is repacked every time.
static int pack_upload(dpk_handle* h) {
    ++h->stage_serial;
    if (h->gen) return gen_upload(h, h->gen);
    h->w.inst->pack(h->stage, h->w.pk, true);      // with the half-width arenas of the modes the instance has
    return upload(h);
}

int dpk_set_graph(dpk_handle* h, const float* adj) {
    if (!h || !adj) return fail(h, DPK_E_INVALID, "dpk_set_graph: null argument");
    if (h->train) return fail(h, DPK_E_STATE, "dpk_set_graph: not while training (the upload would overwrite the device's weights "
                                              "from a stale staging); dpk_train_end first");
    stage_set_graph(h->stage, adj);
    h->have_graph = true;
    return h->have_weights ? pack_upload(h) : DPK_OK;
}

int dpk_set_mask(dpk_handle* h, const uint8_t* m) {
    if (!h || !m) return fail(h, DPK_E_INVALID, "dpk_set_mask: null argument");
    unsigned bits = 0;
    for (int j = 0; j < h->n_pts; ++j)
        if (m[j]) bits |= 1u << j;
    h->mask = bits;
    return DPK_OK;
}

int dpk_set_pose_masks(dpk_handle* h, const uint32_t* bits_dev, int n) {
    if (!h) return DPK_E_INVALID;
    if (bits_dev && n <= 0) return fail(h, DPK_E_INVALID, "dpk_set_pose_masks: n must be positive");
    h->pmask = reinterpret_cast<const unsigned*>(bits_dev);
    h->pmask_n = bits_dev ? n : 0;
    return DPK_OK;
}

int dpk_load_weights(dpk_handle* h, const char* const* names, const float* const* ptrs, const int64_t* numels,
                     int n) {
    if (!h || !names || !ptrs || !numels || n <= 0) return fail(h, DPK_E_INVALID, "dpk_load_weights: bad args");
    for (int i = 0; i < n; ++i)
        if (!names[i] || !ptrs[i]) return fail(h, DPK_E_INVALID, "dpk_load_weights: null entry");
    if (h->train) return fail(h, DPK_E_STATE, "dpk_load_weights: not while training (dpk_train_set writes the parameters of a "
                                              "run); dpk_train_end first");
    std::string err;
    if (!stage_load(h->stage, names, ptrs, numels, n, err))
        return fail(h, DPK_E_WEIGHTS, "dpk_load_weights: " + err);
    h->have_weights = true;
    const int rc = pack_upload(h);
    if (rc || h->gen || h->kind == 0) return rc;
    // the pose backbone adds no timestep projection: a zero row per layer (E_CHEB1 adds +0)
    if (!h->tproj_zero) {
        HIPCHK(h, hipMalloc(&h->tproj_zero, h->w.inst->tp * 4));
        HIPCHK(h, hipMemset(h->tproj_zero, 0, h->w.inst->tp * 4));
    }
    return DPK_OK;
}

// The roots every noising reads, per timestep t of the alpha table: q[t] = (sqrtf(abar[t + 1]), sqrtf(1 - abar[t + 1])),
// fp32 like the reference's a.sqrt() and (1.0 - a).sqrt() (runners/diffpose_frame.py:222, :363).  The one place
// they are rounded: the hypothesis start at t_start (start_spec) and dpk_diff_loss's per-pose t read this table
static std::vector<float> sched_roots(const float* abar, int n_alpha) {
    std::vector<float> q((size_t)(n_alpha - 1) * 2);
    for (int t = 0; t + 1 < n_alpha; ++t) {
        const float a = abar[t + 1], one = 1.0f;
        volatile float sa = sqrtf(a);
        volatile float om = one - a;
        volatile float sb = sqrtf(om);
        q[2 * (size_t)t] = sa;
        q[2 * (size_t)t + 1] = sb;
    }
    return q;
}

int dpk_set_schedule(dpk_handle* h, const float* abar, int n_alpha, const int* seq, int K, float eta) {
    if (!h || !abar || !seq || K <= 0 || n_alpha < 2) return fail(h, DPK_E_INVALID, "dpk_set_schedule: bad args");
    if (h->kind != 0) return fail(h, DPK_E_STATE, "GCNpose handle (coords 2->3) has no diffusion schedule");
    std::vector<float> c((size_t)K * 6);
    // execution order: i over reversed(seq), j over reversed([-1] + seq[:-1]) (utils_diff.py:49-52)
    for (int s = 0; s < K; ++s) {
        const int t = seq[K - 1 - s];
        const int tn = (K - 2 - s) >= 0 ? seq[K - 2 - s] : -1;
        if (t + 1 < 0 || t + 1 >= n_alpha || tn + 1 < 0 || tn + 1 >= n_alpha)
            return fail(h, DPK_E_INVALID, "dpk_set_schedule: timestep outside alpha table (index t+1)");
        const float at = abar[t + 1], an = abar[tn + 1];
        const float one = 1.0f;
        volatile float s1a = sqrtf(one - at);
        volatile float sa = sqrtf(at);
        volatile float san = sqrtf(an);
        volatile float r = at / an;
        volatile float u = one - r;
        volatile float v = one - an;
        volatile float w = u * v;
        volatile float inner = w / (one - at);
        volatile float c1 = eta * sqrtf(inner);
        volatile float c1sq = c1 * c1;
        volatile float c2 = sqrtf((one - an) - c1sq);
        c[s * 6 + 0] = s1a;
        c[s * 6 + 1] = sa;
        c[s * 6 + 2] = san;
        c[s * 6 + 3] = c1;
        c[s * 6 + 4] = c2;
        c[s * 6 + 5] = (float)t;
    }
    HIPCHK(h, hipSetDevice(h->device));
    sched_sweep(h);
    const std::vector<float> q = sched_roots(abar, n_alpha);
    // an identical schedule keeps its device buffers (and every graph captured with them)
    if (h->sched && h->sched->K == K && h->sched->eta == eta && h->sched->h_coef == c && h->sched->h_qtab == q)
        return DPK_OK;
    Sched* s = new Sched();
    static uint64_t sched_serial = 0;
    s->serial = ++sched_serial;
    const size_t tps_off = ((size_t)K * 6 + 3) / 4 * 4;
    const size_t q_off = tps_off + (size_t)K * NL * D;
    hipError_t e = hipMalloc(&s->buf, (q_off + q.size()) * 4);
    if (e != hipSuccess) {
        delete s;
        return fail(h, DPK_E_HIP, std::string("dpk_set_schedule: hipMalloc: ") + hipGetErrorString(e) +
                                      " (a schedule cannot be built while a graph is being captured)");
    }
    s->coef = s->buf;
    s->tps = s->buf + tps_off;
    s->qtab = s->buf + q_off;
    s->nt = n_alpha - 1;
    s->h_qtab = q;
    s->K = K;
    s->eta = eta;
    s->h_coef = c;
    // a fresh buffer no launch has seen: the copy cannot race any stream
    e = hipMemcpyAsync(s->coef, c.data(), c.size() * 4, hipMemcpyHostToDevice, h->aux);
    if (e == hipSuccess) e = hipMemcpyAsync(s->qtab, s->h_qtab.data(), q.size() * 4, hipMemcpyHostToDevice, h->aux);
    if (e == hipSuccess) e = hipStreamSynchronize(h->aux);
    if (e != hipSuccess) {
        sched_free(s);
        return fail(h, DPK_E_HIP, std::string("dpk_set_schedule: coef upload: ") + hipGetErrorString(e));
    }
    if (h->have_weights && sched_tps(h)) {   // every other handle computes its projections per call
        const int rc = sched_compute_tps(h, s);
        if (rc) {
            sched_free(s);
            return rc;
        }
    }
    if (h->sched) h->retired.push_back(h->sched);
    h->sched = s;
    sched_sweep(h);
    return DPK_OK;
}


static int check_ready(dpk_handle* h, int kind = 0) {
    if (h->kind != kind)
        return fail(h, DPK_E_STATE, kind ? "GCNdiff handle: dpk_pose needs a GCNpose handle (coords 2->3)"
                                         : "GCNpose handle (coords 2->3): use dpk_pose");
    if (!h->have_graph) return fail(h, DPK_E_STATE, "graph (adjacency) not set");
    if (!h->have_weights) return fail(h, DPK_E_STATE, "weights not loaded");
    if (!(gemm_modes(h) >> h->gemm_mode & 1)) {
        static const char* const NAMES[3] = {"0 (fp32)", "1 (f16x3)", "2 (bf16)"};
        const Stage& s = h->stage;
        return fail(h, DPK_E_UNSUPPORTED,
                    std::string("gemm mode ") + NAMES[h->gemm_mode] + " is not available at hid " + std::to_string(s.D) +
                        " / " + std::to_string(s.H) + " heads / " + std::to_string(s.J) + " joints" +
                        (h->w.inst ? " (the persistent sampler of this shape has no kernels for it)"
                                   : " (per-op path: fp32 GEMMs only)") +
                        "; dpk_gemm_modes lists the modes of a handle");
    }
    if (h->gemm_mode == 1 && !h->w.pk.w16_ok)
        return fail(h, DPK_E_UNSUPPORTED, "gemm mode 1 (3x fp16): a GEMM weight has |w| >= 1015, outside the split-fp16 "
                                          "packing range; use gemm mode 0 (fp32)");
    return DPK_OK;
}

// dpk_eps on a sampler instance once its projection rows tp [N][NL][D] are there: the timestep MLP, then the tiles
static int eps_launch(dpk_handle* h, const float* x, const float* t, float* eps, int N, hipStream_t st, bool cap,
                      float* tp) {
    h->w.inst->temb(h->w.temb, t, 1, N, tp, st);
    HIPCHK(h, hipGetLastError());
    return profiled(h, st, cap, "dpk_eps", [&] {
        return launch_sampler(h, M_EPS, st, eps_args(h, h->w.arena, tp, x, eps, N), cap);
    });
}

int dpk_eps(dpk_handle* h, const float* x, const float* t, float* eps, int N, void* stream) {
    if (!h) return DPK_E_INVALID;
    if (N < 0 || (N > 0 && (!x || !t || !eps))) return fail(h, DPK_E_INVALID, "dpk_eps: bad args");
    int rc = check_ready(h);
    if (rc) return rc;
    if ((rc = train_fresh(h, "dpk_eps"))) return rc;
    if (N == 0) return DPK_OK;
    hipStream_t st = (hipStream_t)stream;
    bool cap = false;
    if ((rc = enter_call(h, N, "dpk_eps", st, &cap))) return rc;
    if (h->gen) return gen_eps(h, x, t, eps, N, st, cap);
    float* tp = nullptr;             // per-pose projections [N][NL][D]
    if ((rc = eps_scratch(h, st, cap, N, &tp))) return rc;
    return eps_launch(h, x, t, eps, N, st, cap, tp);
}

int dpk_sample(dpk_handle* h, const float* x, float* out, float* xs, float* x0s, int N, uint64_t seed,
               void* stream) {
    return dpk_sample_noise(h, x, out, xs, x0s, N, seed, nullptr, stream);
}

// What every noising call checks first: a schedule is bound (its table of roots), and the scale rows divide the batch
static int noising_check(dpk_handle* h, const char* who, int N, const float* scale, int scale_rows) {
    if (!h->sched) return fail(h, DPK_E_INVALID, std::string(who) + ": no schedule set (dpk_set_schedule)");
    if (scale && (scale_rows < 1 || N % scale_rows != 0))
        return fail(h, DPK_E_INVALID, std::string(who) + ": scale_rows " + std::to_string(scale_rows) + " must be at least 1 and divide N = " +
                                          std::to_string(N));
    return DPK_OK;
}

// The scalars of a hypothesis start at t_start: row t_start of the schedule's table of roots (sched_roots)
static int start_spec(dpk_handle* h, const char* who, int N, int t_start, const float* scale, int scale_rows,
                      const float* start_noise, StartSpec* s) {
    if (!h->sched) return noising_check(h, who, N, scale, scale_rows);
    if (t_start + 1 > h->sched->nt)
        return fail(h, DPK_E_INVALID, std::string(who) + ": t_start " + std::to_string(t_start) + " outside the alpha table (index t_start + 1 of " +
                                          std::to_string(h->sched->nt + 1) + " entries)");
    const int rc = noising_check(h, who, N, scale, scale_rows);
    if (rc) return rc;
    const float* q = h->sched->h_qtab.data() + 2 * (size_t)t_start;
    *s = StartSpec{q[0], q[1], scale, scale ? scale_rows : 1, start_noise};
    return DPK_OK;
}

int dpk_sample_noise(dpk_handle* h, const float* x, float* out, float* xs, float* x0s, int N, uint64_t seed,
                     const float* noise, void* stream) {
    return dpk_sample_start(h, x, out, xs, x0s, N, seed, noise, -1, nullptr, 0, nullptr, stream);
}

int dpk_sample_start(dpk_handle* h, const float* x, float* out, float* xs, float* x0s, int N, uint64_t seed,
                     const float* noise, int t_start, const float* scale, int scale_rows, const float* start_noise,
                     void* stream) {
    if (!h) return DPK_E_INVALID;
    if (N < 0 || (N > 0 && (!x || !out))) return fail(h, DPK_E_INVALID, "dpk_sample: bad args");
    int rc = check_ready(h);
    if (rc) return rc;
    if ((rc = train_fresh(h, "dpk_sample"))) return rc;
    const bool start_on = t_start >= 0;
    StartSpec start{};
    if (start_on && (rc = start_spec(h, "dpk_sample_start", N, t_start, scale, scale_rows, start_noise, &start))) return rc;
    Sched* sc = h->sched;
    if (!sc) return fail(h, DPK_E_STATE, "schedule not set");
    if (N == 0) return DPK_OK;
    if (sched_tps(h) && sc->tps_gen != h->weights_gen)
        return fail(h, DPK_E_STATE, "dpk_sample: schedule projections are stale");
    hipStream_t st = (hipStream_t)stream;
    bool cap = false;
    if ((rc = enter_call(h, N, "dpk_sample", st, &cap))) return rc;
    if (!cap) sched_sweep(h);
    if (h->gen) return gen_sample(h, sc, x, out, xs, x0s, N, seed, noise, start_on ? &start : nullptr, st, cap);
    float* tps = sc->tps;            // per-step projections [K][NL][D]: the schedule's, or this call's
    if (!sched_tps(h)) {
        if ((rc = gen_scratch(h, st, cap, (size_t)sc->K * h->w.inst->tp, &tps, "dpk_sample"))) return rc;
        h->w.inst->temb(h->w.temb, sc->coef + 5, 6, sc->K, tps, st);
    }
    // xs[0]: x, or with the start on x_T, which the kernel writes
    if (xs && !start_on) HIPCHK(h, hipMemcpyAsync(xs, x, (size_t)N * h->n_pts * CIN * 4, hipMemcpyDeviceToDevice, st));
    SampleArgs a = sample_args(h, h->w.arena, tps, sc, x, out, xs, x0s, N, seed, noise);
    if (start_on) {
        a.start_on = 1;
        a.start_sa = start.sa;
        a.start_sb = start.sb;
        a.start_scale = start.scale;
        a.start_scale_rows = start.rows;
        a.start_noise = start.noise;
    }
#if DPK_TRACE
    if (h->trace_step >= 0) {
        const size_t len = (size_t)((N + P - 1) / P) * tile_waves(h) * TRACE_SLOTS;
        if (h->trace_len < len) {
            if (h->trace) HIPCHK(h, hipFree(h->trace));
            HIPCHK(h, hipMalloc(&h->trace, len * 8));
            h->trace_len = len;
        }
        HIPCHK(h, hipMemsetAsync(h->trace, 0, len * 8, st));
    }
    a.trace = h->trace_step >= 0 ? h->trace : nullptr;
    a.trace_step = h->trace_step;
#endif
    rc = profiled(h, st, cap, "dpk_sample", [&] { return launch_sampler(h, M_SAMPLE, st, a, cap); });
    return rc ? rc : sched_note_use(h, sc, st, cap);
}

int dpk_q_sample(dpk_handle* h, const float* x, float* xT, int N, int t_start, const float* scale, int scale_rows,
                 const float* start_noise, uint64_t seed, void* stream) {
    if (!h) return DPK_E_INVALID;
    if (N < 0 || t_start < 0 || (N > 0 && (!x || !xT))) return fail(h, DPK_E_INVALID, "dpk_q_sample: bad args");
    StartSpec start{};
    int rc = start_spec(h, "dpk_q_sample", N, t_start, scale, scale_rows, start_noise, &start);
    if (rc) return rc;
    if (N == 0) return DPK_OK;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    bool cap = false;
    if ((rc = capturing(h, st, &cap))) return rc;
    if (!cap) cap_sweep(h);
    gen_qsample(st, x, xT, nullptr, N, h->gen ? h->gen->s.J * h->gen->s.cin : h->n_pts * CIN, start, seed);
    HIPCHK(h, hipGetLastError());
    return DPK_OK;
}

int dpk_diff_loss(dpk_handle* h, const float* x0, const float* t, const float* scale, int scale_rows,
                  const float* noise, uint64_t seed, float* loss, float* xt, float* eps, int N, void* stream) {
    if (!h) return DPK_E_INVALID;
    if (N < 0 || (N > 0 && (!x0 || !t))) return fail(h, DPK_E_INVALID, "dpk_diff_loss: bad args");
    if (!loss && !xt && !eps) return fail(h, DPK_E_INVALID, "dpk_diff_loss: loss_dev, xt_dev and eps_dev are all null");
    if (h->kind != 0)
        return fail(h, DPK_E_UNSUPPORTED, "dpk_diff_loss: GCNpose handle (coords 2->3) has no diffusion objective");
    int rc = noising_check(h, "dpk_diff_loss", N, scale, scale_rows);
    if (rc) return rc;
    const bool need_eps = loss || eps;          // x_t alone needs neither weights nor a graph, like dpk_q_sample
    if (need_eps && (rc = check_ready(h))) return rc;
    if (need_eps && (rc = train_fresh(h, "dpk_diff_loss"))) return rc;
    if (N == 0) return DPK_OK;
    Sched* sc = h->sched;
    hipStream_t st = (hipStream_t)stream;
    bool cap = false;
    if ((rc = enter_call(h, N, "dpk_diff_loss", st, &cap))) return rc;
    if (!cap) sched_sweep(h);
    // A sampler instance runs it in dpk_eps's own launch: the noising where the tile loads its poses, the sum in the
    // epilogue (sample_kernel, EPS_MODE).  DPK_LOSS_FUSED=0 keeps the three launches below on such a handle too (A/B)
    const char* lf = getenv("DPK_LOSS_FUSED");
    if (h->w.inst && need_eps && !(lf && atoi(lf) == 0)) {
        float* tp = nullptr;
        if ((rc = eps_scratch(h, st, cap, N, &tp))) return rc;
        h->w.inst->temb(h->w.temb, t, 1, N, tp, st);
        HIPCHK(h, hipGetLastError());
        SampleArgs a = eps_args(h, h->w.arena, tp, x0, eps, N);
        a.loss_t = t;
        a.loss_qtab = sc->qtab;
        a.loss_nt = sc->nt;
        a.loss_out = loss;
        a.loss_xt = xt;
        a.start_scale = scale;
        a.start_scale_rows = scale ? scale_rows : 1;
        a.start_noise = noise;
        a.seed = seed;
        rc = profiled(h, st, cap, "dpk_diff_loss", [&] { return launch_sampler(h, M_EPS, st, a, cap); });
        return rc ? rc : sched_note_use(h, sc, st, cap);
    }
    // one request of the call's scratch, counted in floats on every handle: what the eps evaluation takes (the
    // per-op forward's buffers, or an instance's projection rows), then x_t and eps where the caller keeps neither
    const int pe = h->gen ? h->gen->s.J * h->gen->s.cin : h->n_pts * CIN;
    const auto up64 = [](size_t v) { return (v + 63) / 64 * 64; };   // 256-byte boundaries between the parts
    const size_t n = (size_t)N * pe;
    const size_t eps_floats = up64(!need_eps ? 0 : h->gen ? gen_eps_floats(h->gen->s, N) : (size_t)N * h->w.inst->tp);
    const size_t extra = (xt ? 0 : up64(n)) + (need_eps && !eps ? n : 0);
    float* S = nullptr;
    if (eps_floats + extra && (rc = gen_scratch(h, st, cap, eps_floats + extra, &S, "dpk_diff_loss"))) return rc;
    float* own = S ? S + eps_floats : nullptr;
    if (!xt) xt = own, own += up64(n);
    if (need_eps && !eps) eps = own;
    const StartSpec spec{0.f, 0.f, scale, scale ? scale_rows : 1, noise};
    gen_qsample_t(st, x0, xt, N, pe, t, sc->qtab, sc->nt, spec, seed);
    HIPCHK(h, hipGetLastError());
    if (need_eps) {
        rc = h->gen ? gen_eps(h, xt, t, eps, N, st, cap, S) : eps_launch(h, xt, t, eps, N, st, cap, S);
        if (rc) return rc;
    }
    if (loss) {
        gen_diff_loss(st, eps, N, pe, spec, seed, loss);
        HIPCHK(h, hipGetLastError());
    }
    return sched_note_use(h, sc, st, cap);
}

// dpk_diff_loss_grad and dpk_diff_loss_grad_train behind their own argument checks (`who` names the entry point)
static int grad_call(dpk_handle* h, const std::string& who, const float* x0, const float* t, const float* scale,
                     int scale_rows, const float* noise, uint64_t seed, float weight, float* loss, float* grads, int N,
                     void* stream, const DropRun& dr) {
    if (h->kind != 0)
        return fail(h, DPK_E_UNSUPPORTED, who + ": GCNpose handle (coords 2->3) has no diffusion objective");
    if (h->gemm_mode != 0)
        return fail(h, DPK_E_UNSUPPORTED, who + ": the backward is fp32 (per-op kernels on the fp32 MFMA); "
                                                "set gemm mode 0 (fp32) for the call");
    int rc = noising_check(h, who.c_str(), N, scale, scale_rows);
    if (rc) return rc;
    if ((rc = check_ready(h))) return rc;
    if (N == 0) return DPK_OK;
    hipStream_t st = (hipStream_t)stream;
    bool cap = false;
    if ((rc = enter_call(h, N, who.c_str(), st, &cap))) return rc;
    if (cap)
        return fail(h, DPK_E_STATE, who + ": not callable while a graph is being captured (its scratch and "
                                          "its arenas are allocated by the call)");
    sched_sweep(h);
    if ((rc = bwd_prepare(h))) return rc;
    const StartSpec spec{0.f, 0.f, scale, scale ? scale_rows : 1, noise};
    if ((rc = bwd_run(h, x0, t, spec, seed, weight, loss, grads, N, st, dr))) return rc;
    return sched_note_use(h, h->sched, st, false);
}

int dpk_diff_loss_grad(dpk_handle* h, const float* x0, const float* t, const float* scale, int scale_rows,
                       const float* noise, uint64_t seed, float weight, float* loss, float* grads, int N, void* stream) {
    if (!h) return DPK_E_INVALID;
    if (N < 0 || (N > 0 && (!x0 || !t || !grads))) return fail(h, DPK_E_INVALID, "dpk_diff_loss_grad: bad args");
    return grad_call(h, "dpk_diff_loss_grad", x0, t, scale, scale_rows, noise, seed, weight, loss, grads, N, stream,
                     DropRun{});
}

// a dropout rate must lie in [0, 1): the text of the refusal, empty when it does
static std::string drop_rate_error(const char* name, float p) {
    if (p >= 0.f && p < 1.f) return "";
    return std::string("dropout rate ") + name + " = " + std::to_string(p) + " is not in [0, 1)";
}

int dpk_diff_loss_grad_train(dpk_handle* h, const float* x0, const float* t, const float* scale, int scale_rows,
                             const float* noise, uint64_t seed, float weight, const dpk_dropout* drop,
                             uint64_t drop_seed, int64_t pose0, float* loss, float* grads, int N, void* stream) {
    if (!h) return DPK_E_INVALID;
    const std::string who = "dpk_diff_loss_grad_train";
    if (N < 0 || (N > 0 && (!x0 || !t || !grads))) return fail(h, DPK_E_INVALID, who + ": bad args");
    if (!drop) return fail(h, DPK_E_INVALID, who + ": drop is NULL");
    const std::pair<const char*, float> rates[3] = {{"sublayer", drop->sublayer}, {"attn", drop->attn}, {"gconv", drop->gconv}};
    for (const auto& r : rates) {
        const std::string e = drop_rate_error(r.first, r.second);
        if (!e.empty()) return fail(h, DPK_E_INVALID, who + ": " + e);
    }
    if (pose0 < 0) return fail(h, DPK_E_INVALID, who + ": pose0 = " + std::to_string(pose0) + " is negative");
    DropRun dr;
    dr.sublayer = drop->sublayer, dr.attn = drop->attn, dr.gconv = drop->gconv;
    dr.seed = drop_seed, dr.pose0 = pose0;
    return grad_call(h, who, x0, t, scale, scale_rows, noise, seed, weight, loss, grads, N, stream, dr);
}

int dpk_dropout_mask(uint64_t drop_seed, int layer, int site, float p, int64_t first, int64_t n, uint8_t* keep,
                     void* stream) {
    if (layer < 0 || site < 0 || site >= dpkg::DROP_SITES || !(p >= 0.f && p < 1.f) || first < 0 || n < 0 ||
        (n > 0 && !keep))
        return DPK_E_INVALID;
    if (n == 0) return DPK_OK;
    DropRun dr;
    dr.sublayer = dr.attn = dr.gconv = p;
    dr.seed = drop_seed;
    const dpkg::DropSite d = dr.site(layer, site);
    const long long groups = ((first + n + 3) >> 2) - (first >> 2);
    hipLaunchKernelGGL(dpkg::drop_mask_bytes, dim3(gen_blocks(groups)), dim3(256), 0, (hipStream_t)stream, keep,
                       (long long)first, (long long)n, d);
    return hipGetLastError() == hipSuccess ? DPK_OK : DPK_E_HIP;
}

int dpk_train_draws(uint64_t e_seed, uint64_t t_seed, int T, int64_t batch, int64_t pose0, int n, int pose_floats,
                    float* e, float* t, void* stream) {
    if (T < 1 || T > (1 << 24) || batch < 1 || pose0 < 0 || n < 0 || n > batch - pose0 || pose_floats < 1 ||
        (n > 0 && !e && !t))
        return DPK_E_INVALID;
    if (n == 0) return DPK_OK;
    const long long ne = e ? (long long)n * pose_floats : 0, nt = t ? n : 0;
    // one work item per float; a grid-stride loop past 2^20 workgroups
    const long long blocks = std::min<long long>((ne + nt + 255) / 256, 1 << 20);
    hipLaunchKernelGGL(dpkg::train_draws, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, e, t, ne, nt,
                       (long long)pose0 * pose_floats, (long long)pose0, (long long)batch, T,
                       (unsigned long long)e_seed, (unsigned long long)t_seed);
    return hipGetLastError() == hipSuccess ? DPK_OK : DPK_E_HIP;
}

int dpk_param_count(const dpk_handle* h) {
    if (!h || h->kind != 0) return 0;
    return (int)grad_layout(h->stage).e.size();
}

int dpk_param_layout(const dpk_handle* h, int i, const char** name, int64_t* offset, int64_t* numel) {
    if (!h || h->kind != 0) return DPK_E_UNSUPPORTED;
    // names live as long as the process: one table per shape ever asked for
    static std::vector<std::pair<std::string, GradLayout>*> tables;
    const Stage& s = h->stage;
    const std::string key = std::to_string(s.D) + "/" + std::to_string(s.J) + "/" + std::to_string(s.L) + "/" +
                            std::to_string(s.cin) + "/" + std::to_string(s.cout);
    const GradLayout* g = nullptr;
    for (auto* tb : tables)
        if (tb->first == key) g = &tb->second;
    if (!g) {
        tables.push_back(new std::pair<std::string, GradLayout>(key, grad_layout(s)));
        g = &tables.back()->second;
    }
    if (i < 0 || i >= (int)g->e.size()) return DPK_E_INVALID;
    if (name) *name = g->e[i].name.c_str();
    if (offset) *offset = g->e[i].offset;
    if (numel) *numel = g->e[i].numel;
    return DPK_OK;
}

int dpk_train_begin(dpk_handle* h, const dpk_optim_config* cfg) {
    if (!h) return DPK_E_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    return train_begin(h, cfg);
}

int dpk_train_apply(dpk_handle* h, const float* grads, float lr, float* gnorm, void* stream) {
    if (!h) return DPK_E_INVALID;
    if (!h->train) return fail(h, DPK_E_STATE, "dpk_train_apply: training has not begun (dpk_train_begin)");
    if (!grads) return fail(h, DPK_E_INVALID, "dpk_train_apply: grads_dev is NULL");
    if (!(lr >= 0.f)) return fail(h, DPK_E_INVALID, "dpk_train_apply: lr = " + std::to_string(lr) + " is negative or NaN");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    bool cap = false;
    const int rc = capturing(h, st, &cap);
    if (rc) return rc;
    if (cap) return fail(h, DPK_E_STATE, "dpk_train_apply: not callable while a graph is being captured (the step count and "
                                         "Adam's bias corrections are the host's, by value)");
    return train_apply(h, grads, lr, gnorm, st);
}

int dpk_train_sync(dpk_handle* h) {
    if (!h) return DPK_E_INVALID;
    if (!h->train) return fail(h, DPK_E_STATE, "dpk_train_sync: training has not begun (dpk_train_begin)");
    return train_sync(h);
}

// `which` of dpk_train_get / dpk_train_set as the array, or null with the refusal's text in h
static float* train_array(dpk_handle* h, const char* who, int which) {
    static const char* const NAMES[5] = {"params", "exp_avg", "exp_avg_sq", "max_exp_avg_sq", "the EMA shadow"};
    if (!h->train) return fail(h, DPK_E_STATE, std::string(who) + ": training has not begun (dpk_train_begin)"), nullptr;
    if (which < 0 || which > 4)
        return fail(h, DPK_E_INVALID, std::string(who) + ": which = " + std::to_string(which) + " is not in 0..4"), nullptr;
    if (!h->train->arr[which])
        return fail(h, DPK_E_INVALID, std::string(who) + ": which = " + std::to_string(which) + " (" + NAMES[which] +
                                          ") is not kept: dpk_train_begin was called without " +
                                          (which == 3 ? "amsgrad" : "an ema_mu >= 0")), nullptr;
    return h->train->arr[which];
}

int dpk_train_get(dpk_handle* h, int which, float* out, int64_t* step, void* stream) {
    if (!h) return DPK_E_INVALID;
    float* a = train_array(h, "dpk_train_get", which);
    if (!a) return h->train ? DPK_E_INVALID : DPK_E_STATE;
    if (!out) return fail(h, DPK_E_INVALID, "dpk_train_get: out_dev is NULL");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(out, a, h->train->F * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (step) *step = h->train->step;
    return DPK_OK;
}

int dpk_train_set(dpk_handle* h, int which, const float* in, int64_t step, void* stream) {
    if (!h) return DPK_E_INVALID;
    float* a = train_array(h, "dpk_train_set", which);
    if (!a) return h->train ? DPK_E_INVALID : DPK_E_STATE;
    if (!in) return fail(h, DPK_E_INVALID, "dpk_train_set: in_dev is NULL");
    if (step < -1) return fail(h, DPK_E_INVALID, "dpk_train_set: step = " + std::to_string(step) + " (-1 leaves the count alone)");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    bool cap = false;
    const int rc = capturing(h, st, &cap);
    if (rc) return rc;
    if (cap) return fail(h, DPK_E_STATE, "dpk_train_set: not callable while a graph is being captured");
    HIPCHK(h, hipMemcpyAsync(a, in, h->train->F * 4, hipMemcpyDeviceToDevice, st));
    if (step >= 0) h->train->step = step;
    if (which == 0) {
        train_refresh_launch(h, st);
        HIPCHK(h, hipGetLastError());
        h->train->host_stale = true;
    }
    return DPK_OK;
}

int dpk_train_end(dpk_handle* h) {
    if (!h) return DPK_E_INVALID;
    if (!h->train) return fail(h, DPK_E_STATE, "dpk_train_end: training has not begun (dpk_train_begin)");
    const int rc = train_sync(h);
    if (rc) return rc;
    train_free(h->train);
    h->train = nullptr;
    return DPK_OK;
}

int dpk_pose(dpk_handle* h, const float* x2d, float* xyz, float* uvxyz, int N, int H, int root_mode,
             void* stream) {
    if (!h) return DPK_E_INVALID;
    if (N < 0 || H < 1 || root_mode < 0 || root_mode > 2 || (N > 0 && (!x2d || (!xyz && !uvxyz))))
        return fail(h, DPK_E_INVALID, "dpk_pose: bad args");
    int rc = check_ready(h, 1);
    if (rc) return rc;
    if (N == 0) return DPK_OK;
    hipStream_t st = (hipStream_t)stream;
    bool cap = false;
    if ((rc = enter_call(h, N, "dpk_pose", st, &cap))) return rc;
    if (h->gen) return gen_pose(h, x2d, xyz, uvxyz, N, H, root_mode, st, cap);
    return profiled(h, st, cap, "dpk_pose", [&] {
        return launch_sampler(h, M_POSE, st, pose_args(h, h->w.arena, h->tproj_zero, x2d, xyz, uvxyz, N, H, root_mode), cap);
    });
}

int dpk_set_gemm_mode(dpk_handle* h, int mode) {
    if (!h) return DPK_E_INVALID;
    if (mode < 0 || mode > 2)
        return fail(h, DPK_E_INVALID, "dpk_set_gemm_mode: mode must be 0 (fp32), 1 (3xfp16) or 2 (bf16)");
    // a padded handle names its joint count at the set (the other refusals of a mode come at the call, check_ready)
    if (mode == 2 && padded(h))
        return fail(h, DPK_E_UNSUPPORTED, "dpk_set_gemm_mode: gemm mode 2 (bf16) is built for 17 joints; this handle has " +
                                              std::to_string(h->n_pts) + " joints on padded tiles (fp32 and f16x3)");
    h->gemm_mode = mode;
    return DPK_OK;
}

int dpk_fused(const dpk_handle* h) { return h && h->w.inst ? 1 : 0; }

int dpk_gemm_modes(const dpk_handle* h) { return h ? gemm_modes(h) : 0; }

int dpk_set_tile_waves(dpk_handle* h, int waves) {
    if (!h) return DPK_E_INVALID;
    if (waves != 0 && waves != 4 && waves != 8)
        return fail(h, DPK_E_INVALID, "dpk_set_tile_waves: waves must be 0 (the GEMM mode's default), 4 or 8");
    if (waves == 8 && padded(h))
        return fail(h, DPK_E_UNSUPPORTED, "dpk_set_tile_waves: the 8-wave tile is compiled for 17 joints; this handle has " +
                                              std::to_string(h->n_pts) + " joints on padded 4-wave tiles");
    if (waves == 8 && !(h->w.inst && h->w.inst->wave8))
        return fail(h, DPK_E_UNSUPPORTED, "dpk_set_tile_waves: the 8-wave tile is compiled for hid 96 / 4 heads / 17 joints");
    h->tile_waves = waves;
    return DPK_OK;
}

int dpk_set_tail_plan(dpk_handle* h, int plan) {
    if (!h) return DPK_E_INVALID;
    if (plan < 0 || plan > 2) return fail(h, DPK_E_INVALID, "dpk_set_tail_plan: plan must be 0, 1 or 2");
    h->tail_plan = DPK_TRACE ? 0 : plan;
    return DPK_OK;
}

int dpk_profile(dpk_handle* h, int enable) {
    if (!h) return DPK_E_INVALID;
    h->profiling = enable != 0;
    return DPK_OK;
}

int dpk_profile_read(dpk_handle* h, float* ms, int cap, int* count) {
    if (!h || (cap > 0 && !ms)) return fail(h, DPK_E_INVALID, "dpk_profile_read: bad args");
    HIPCHK(h, hipSetDevice(h->device));
    int n = 0;
    for (auto& e : h->ev_used) {
        HIPCHK(h, hipEventSynchronize(e.second));
        float t = 0.f;
        HIPCHK(h, hipEventElapsedTime(&t, e.first, e.second));
        if (n < cap) ms[n] = t;
        ++n;
        h->ev_free.push_back(e);
    }
    h->ev_used.clear();
    if (count) *count = n;
    return DPK_OK;
}

int dpk_ddim_update(dpk_handle* h, const float* xt, const float* et, float* xn, float* x0, int64_t n, int step,
                    uint64_t seed, void* stream) {
    return dpk_ddim_update_noise(h, xt, et, xn, x0, n, step, seed, nullptr, stream);
}

int dpk_ddim_update_noise(dpk_handle* h, const float* xt, const float* et, float* xn, float* x0, int64_t n,
                          int step, uint64_t seed, const float* noise, void* stream) {
    if (!h) return DPK_E_INVALID;
    if (n < 0 || (n > 0 && (!xt || !et || !xn))) return fail(h, DPK_E_INVALID, "dpk_ddim_update: bad args");
    Sched* sc = h->sched;
    if (!sc) return fail(h, DPK_E_STATE, "schedule not set");
    if (step < 0 || step >= sc->K) return fail(h, DPK_E_INVALID, "dpk_ddim_update: step out of range");
    if (n == 0) return DPK_OK;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    bool cap = false;
    int rc = capturing(h, st, &cap);
    if (rc) return rc;
    if (!cap) cap_sweep(h);
    const long long nb = (n + 255) / 256;
    hipLaunchKernelGGL(ddim_kernel, dim3((unsigned)nb), dim3(256), 0, st, xt, et, xn, x0, (long long)n,
                       sc->coef + step * 6, step, sc->eta, (unsigned long long)seed, noise);
    HIPCHK(h, hipGetLastError());
    return sched_note_use(h, sc, st, cap);
}

int dpk_debug_split(dpk_handle* h, int mode, int* fallbacks) {
    if (!h) return DPK_E_INVALID;
    if (mode < 0 || mode > 2) return fail(h, DPK_E_INVALID, "dpk_debug_split: mode must be 0, 1 or 2");
    h->split_dbg = mode;
    if (fallbacks) {
        HIPCHK(h, hipSetDevice(h->device));
        HIPCHK(h, hipDeviceSynchronize());
        int* ctr = reinterpret_cast<int*>(h->flags + (size_t)FLAG_SLOTS * h->n_cu);
        HIPCHK(h, hipMemcpy(fallbacks, ctr, 4, hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemset(ctr, 0, 4));
    }
    return DPK_OK;
}

int dpk_debug_resources(dpk_handle* h, int* out, int n) {
    if (!h || (n > 0 && !out)) return DPK_E_INVALID;
    int released = 0, tracked = 0, retired = (int)h->retired.size();
    for (CapRes* c : h->caps) {
        tracked += c->tracked ? 1 : 0;
        released += (c->tracked && c->released.load()) ? 1 : 0;
    }
    // the pool's spare: in poses of dpk_eps projections on the shipped shape (sched_tps), else in KiB
    const size_t spare = h->pool.spare.cap;
    const int v[8] = {(int)h->caps.size(), tracked, released, (int)h->slot_free.size(), retired,
                      sched_tps(h) ? (int)(spare / h->w.inst->tp) : 0, gen_graph_count(h->gen),
                      sched_tps(h) ? 0 : (int)((spare * 4) >> 10)};
    for (int i = 0; i < n && i < 8; ++i) out[i] = v[i];
    return DPK_OK;
}

int dpk_debug_generic_forms(dpk_handle* h, unsigned* forms) {
    if (!h || !forms) return DPK_E_INVALID;
    *forms = gen_take_forms(h->gen);
    return DPK_OK;
}

int dpk_debug_grad_forms(dpk_handle* h, unsigned* gemm_forms, unsigned* bwd_forms) {
    if (!h || !gemm_forms || !bwd_forms) return DPK_E_INVALID;
    *gemm_forms = h->bwd ? h->bwd->fforms : 0;
    *bwd_forms = h->bwd ? h->bwd->bforms : 0;
    if (h->bwd) h->bwd->fforms = h->bwd->bforms = 0;
    return DPK_OK;
}

int dpk_debug_sampler_kernels(dpk_handle* h, uint32_t* ids, int cap, int* count) {
    if (!count || cap < 0 || (cap > 0 && !ids)) return fail(h, DPK_E_INVALID, "dpk_debug_sampler_kernels: bad args");
    std::vector<uint32_t> v;
    if (h) {
        v.swap(h->kernels);
    } else {
        for (const SamplerInst* i : INSTANCES)
            for (const SamplerInst* t : {i, i->wave8, i->tail2})
                if (t) t->kernels(*t, v);
    }
    for (int k = 0; k < cap && k < (int)v.size(); ++k) ids[k] = v[k];
    *count = (int)v.size();
    return DPK_OK;
}

#if DPK_TRACE
// trace builds only (not part of the C ABI): choose the traced step; copy the stamps out
int dpk_debug_trace(dpk_handle* h, int step, unsigned long long* out, long long cap) {
    if (!h) return DPK_E_INVALID;
    h->trace_step = step;
    if (!out || !h->trace) return DPK_OK;
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, hipMemcpy(out, h->trace, std::min((size_t)cap, h->trace_len) * 8, hipMemcpyDeviceToHost));
    return (int)std::min((size_t)cap, h->trace_len);
}
#endif

}  // extern "C"
