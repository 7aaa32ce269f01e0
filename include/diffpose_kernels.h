/*
 * diffpose_kernels.h — C ABI of the MI355X-native DiffPose DDIM sampler (libdpk.so).
 *
 * Drop-in boundary for the reference hot path (reference at nwicakson/diffpose-nw):
 *   - the denoiser callable  GCNdiff.forward(x, mask, t, cemd) -> eps      models/gcndiff.py:101-113
 *     (called once per step at common/utils_diff.py:58)
 *   - the DDIM reverse loop  generalized_steps(x, src_mask, seq, model, b, eta)
 *                                                                           common/utils_diff.py:46-68
 *   - its caller             Diffpose.test_hyber                           runners/diffpose_frame.py:345-370
 * The reference has no FFI of its own (pure PyTorch); these entry points are what a
 * ctypes binding of that seam needs.  INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - All tensor pointers are caller-owned DEVICE memory (fp32, row-major, contiguous)
 *     on the device the handle was created for; work is enqueued on `stream`
 *     (a hipStream_t, NULL = default stream) and is asynchronous.
 *   - Poses are (N, n_pts, 5) uvxyz: N poses x the handle's joints (17 on Human3.6M) x 5 channels.
 *   - Caller memory (tests/test_gpu_caller_memory.py holds every entry point to this, each array between guard
 *     words): a call reads and writes exactly the extents documented for each array, not one element before or
 *     past them, so an array may end at the last byte the caller owns.  float arrays (and the 32-bit mask
 *     and status words) need 4-byte alignment and nothing more; double and int64 arrays their natural 8 bytes.  Inputs are never written.  Every element of a
 *     non-NULL output is written; an optional output passed as NULL is not touched, and a call over N = 0 poses
 *     (elements, frames) returns DPK_OK and touches nothing.  An output may BE an input only where its description
 *     says "may be": the same pointer, the same extent.  Any other overlap between the arrays of one call is
 *     undefined.
 *   - Return value 0 = OK, negative = error (DPK_E_*); dpk_last_error() has the text.
 *   - A handle is bound to one device and is not thread-safe: one handle per rank/thread.
 *   - Stream order: launches (dpk_sample / dpk_eps / dpk_pose / dpk_ddim_update) may be in
 *     flight on several streams at once.  dpk_set_schedule never rewrites a schedule a launch
 *     may still read: it builds a new one, and the old one is freed only after every stream
 *     that used it has passed its last launch.  Uncaptured dpk_eps calls keep their per-pose
 *     timestep projections in a buffer per caller stream.  dpk_load_weights / dpk_set_graph
 *     wait for the device to drain before overwriting the weights (configuration calls).
 *   - Graph capture (hipStreamBeginCapture / torch.cuda.graph): dpk_sample (dpk_sample_noise,
 *     dpk_sample_start), dpk_eps, dpk_pose, dpk_ddim_update and dpk_q_sample may be captured.  A captured launch reads the schedule current at
 *     capture time for the graph's whole life (a later dpk_set_schedule builds a new one and
 *     leaves the captured one in place); weights reloaded later are seen by replays.  It also
 *     keeps the key mask it was captured with: the dpk_set_mask bits by value, and the
 *     dpk_set_pose_masks array by address (that array must stay allocated and unchanged while
 *     the graph may replay).  Nothing is allocated inside a captured call.  What the launches of
 *     one capture read by address (their schedules, one dpk_eps projection buffer and one
 *     step-split flag slot per capturing stream, shared by that stream's captured calls) belongs
 *     to the capture: a user object retained by the captured graph releases it when the graph and
 *     its executable instances are destroyed, and the handle's next uncaptured call recycles it
 *     (after one device-wide wait).  The first captured dpk_eps of a capture takes the handle's
 *     spare projection buffer, which every uncaptured dpk_eps of at least N poses sizes: make one
 *     with the capture's largest N before it (else DPK_E_STATE).  Replays of one executable graph
 *     must not overlap each other (HIP orders launches of the same graph exec), and neither may
 *     two executable instances of one captured graph (they share its projection buffer and flag
 *     slot): capture again for a second concurrent instance.
 */
#ifndef DIFFPOSE_KERNELS_H
#define DIFFPOSE_KERNELS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPK_OK              0
#define DPK_E_INVALID      -1   /* bad argument (null pointer, N<0, size mismatch)       */
#define DPK_E_UNSUPPORTED  -2   /* model dims / mode neither path supports               */
#define DPK_E_HIP          -3   /* HIP runtime error                                     */
#define DPK_E_STATE        -4   /* weights / graph / schedule not set yet                */
#define DPK_E_WEIGHTS      -5   /* unknown, missing or mis-sized state_dict entry        */

typedef struct dpk_handle dpk_handle;

/* Model hyper-parameters (configs/human36m_diffpose_uvxyz_*.yml model: section,
 * emd_dim = 4*hid_dim per models/gcndiff.py:68).  The persistent sampler is compiled for
 * hid_dim 96, n_head 4, n_pts 17 and coords_dim [5,5] (GCNdiff, the denoiser) or [2,3]
 * (GCNpose, the 2D->3D front-end; runners/diffpose_frame.py:138), with num_layers (the
 * config's num_layer, models/gcndiff.py:63-90) a run-time value in 1..5 (the reference's
 * configs all use 5); other shapes run the generic-shape path (dpk_create). */
typedef struct {
    int hid_dim;
    int num_layers;
    int n_head;
    int n_pts;
    int coords_in;
    int coords_out;
    int device;        /* HIP device ordinal */
} dpk_config;

/* Library version (major*10000 + minor*100 + patch). */
int dpk_version(void);

/* Create a handle on cfg->device.  Replaces GCNdiff(adj, config) construction
 * (models/gcndiff.py:55-99; runners/diffpose_frame.py:118-127).  The shape every reference config
 * uses (hid_dim 96, n_head 4, n_pts 17, num_layer 1..5, coords [5,5] or GCNpose's [2,3]) runs the
 * persistent sampler; any other shape with hid_dim a multiple of n_head (and, for GCNdiff, at least 4:
 * its timestep embedding divides by hid_dim / 2 - 1, models/gcndiff.py:15-33, where the reference raises
 * ZeroDivisionError for hid_dim 2 and 3; GCNpose has no embedding and takes hid_dim >= 2), 2 <= n_pts <= 32
 * and coords in == out (or [2,3]) runs the generic-shape path: the same model as per-op HIP kernels, or, for GCNdiff
 * at hid_dim 128 / n_head 8 or 4 and hid_dim 64 / n_head 2 or 4 on 17 joints (num_layer <= 5, coords [5,5]), the
 * persistent sampler compiled at that width (round 5).  GCNdiff on 2..16 joints at any of these five shapes runs
 * the same persistent sampler as padded tiles (an n-joint pose in a 17-row pose block, its graph terms
 * zero-embedded, the rows and attention keys past n dead), from DPK_PAD_MIN joints up (the environment variable
 * DPK_PAD_MIN_JOINTS overrides it: 2 every count, 17 none), in gemm modes 0 and 1, on 4-wave tiles (dpk_fused says
 * which path a handle got).  The four width instances run gemm modes 0 (fp32) and
 * 1 (f16x3), the per-op kernels mode 0 alone; a call in a mode the handle's path lacks fails with
 * DPK_E_UNSUPPORTED (dpk_gemm_modes says which it has).  Per-stream scratch grown on demand; under a caller's stream capture the
 * launches are recorded into the caller's graph from a capture-owned scratch (round 5; the first capture
 * of a size needs one uncaptured call of at least that size, else DPK_E_STATE).  Other shapes:
 * DPK_E_UNSUPPORTED. */
int dpk_create(const dpk_config* cfg, dpk_handle** out);

/* Dense n_pts x n_pts adjacency as passed to GCNdiff(adj, ...) (row-normalised,
 * models/GraFormer.py:32-44).  Derives the Chebyshev terms T0..T2 of its
 * normalised Laplacian once (models/ChebConv.py:90-130), instead of per call. */
int dpk_set_graph(dpk_handle* h, const float* adj_host);

/* Load a GCNdiff state_dict (keys as in models/gcndiff.py, with or without the
 * DataParallel "module." prefix; runners/diffpose_frame.py:130-132).  Copies the n
 * host arrays, repacks GEMM weights into MFMA fragment order and precomputes each
 * layer's GraphNet Laplacian (models/GraFormer.py:174-178).  All keys required. */
int dpk_load_weights(dpk_handle* h, const char* const* names, const float* const* host_ptrs,
                     const int64_t* numels, int n);

/* Attention key mask, n_pts bytes (nonzero = attend).  Default all ones, the
 * reference's src_mask (runners/diffpose_frame.py:39-40); zero entries take the
 * masked_fill(-1e9) path of models/GraFormer.py:107-108. */
int dpk_set_mask(dpk_handle* h, const uint8_t* mask_host);

/* Per-pose key masks: the reference's masked_fill broadcasts a [N,1,n_pts] mask
 * over heads and queries (models/GraFormer.py:107-108, mask.unsqueeze(1)).
 * bits_dev: n uint32 words in device memory, bit j of word i = key j of pose i
 * attends.  Owned by the caller and read by every later dpk_eps / dpk_sample /
 * dpk_pose launch (pose i of the launch uses word i; a launch of more than n
 * poses fails with DPK_E_INVALID) until replaced; NULL returns to the
 * dpk_set_mask mask for all poses.  The launches read the array asynchronously, on
 * their streams: free or rewrite it only after they have completed (and never while
 * a graph captured with it may replay). */
int dpk_set_pose_masks(dpk_handle* h, const uint32_t* bits_dev, int n);

/* DDIM schedule.  alpha_bar: fp32 table (1-cat([0],betas)).cumprod(0), n_alpha = T+1
 * entries (compute_alpha, common/utils_diff.py:40-43); seq: K timesteps in
 * ascending order as built by test_hyber (runners/diffpose_frame.py:310-317);
 * eta as in common/utils_diff.py:61-63.  Step scalars are evaluated in fp32 in
 * the reference's operation order.  Host-synchronous: builds a new device schedule
 * (step scalars + per-step timestep projections, on a handle-internal stream) unless
 * the schedule is unchanged; see "Stream order" above.  Not callable while a graph is
 * being captured. */
int dpk_set_schedule(dpk_handle* h, const float* alpha_bar, int n_alpha, const int* seq, int K, float eta);

/* One denoiser evaluation eps = GCNdiff(x, mask, t) for N poses with a
 * per-pose timestep t_dev[N] (float, as model(xt, mask, t.float(), 0)).  eps_dev [N,n_pts,5] may be x_dev. */
int dpk_eps(dpk_handle* h, const float* x_dev, const float* t_dev, float* eps_dev, int N, void* stream);

/* The whole K-step reverse loop of generalized_steps for N poses in ONE
 * persistent kernel (the per-step timestep projections come with the schedule).
 *   x_dev   [N,n_pts,5] input x (= xs[0])
 *   out_dev [N,n_pts,5] final sample xs[-1]; may be x_dev (x = sample(x)), the step-split last round and the
 *           hypothesis start of dpk_sample_start included: xs[0] still holds what the loop started from
 *   xs_dev  [K+1,N,n_pts,5] or NULL: full trajectory xs (xs[0] copied from x_dev; x_T under dpk_sample_start)
 *   x0s_dev [K,N,n_pts,5]   or NULL: x0_preds
 *   seed: noise stream for eta > 0 (counter-based, not torch.randn_like). */
int dpk_sample(dpk_handle* h, const float* x_dev, float* out_dev, float* xs_dev, float* x0s_dev,
               int N, uint64_t seed, void* stream);

/* dpk_sample with the caller's noise for eta > 0: noise_dev [K,N,n_pts,5] fp32 device, slice k the
 * draw z of the k-th executed step (t = seq[K-1-k]) in x' = sqrt(an)*x0 + c1*z + c2*et — what the
 * reference draws as torch.randn_like(x) once per step (common/utils_diff.py:65), so a caller that
 * draws the same K tensors reproduces the reference's eta > 0 trajectory.  NULL = counter-based
 * noise from `seed` (dpk_sample).  Read asynchronously on `stream`. */
int dpk_sample_noise(dpk_handle* h, const float* x_dev, float* out_dev, float* xs_dev, float* x0s_dev,
                     int N, uint64_t seed, const float* noise_dev, void* stream);

/* dpk_sample_noise from a noised hypothesis start: what test_hyber's commented-out line
 * (runners/diffpose_frame.py:355-363) computes in front of generalized_steps, inside the same launch:
 *   x_T = (x * sqrt(a)) + ((e * scale) * sqrt(1 - a)),  a = alpha_bar[t_start + 1]
 * from the table of the last dpk_set_schedule (the reference's (1-b).cumprod(0).index_select(0, t) at
 * t = t_start); sqrt(a) and sqrt(1 - a) are taken on the host in fp32 and every element is four fp32
 * roundings in that order (no FMA), so x_T is bitwise what torch computes for the same inputs.  The K steps
 * then run from x_T, and with xs_dev given xs[0] is x_T (written by the kernel; x_dev is not modified).
 *   t_start          < 0: no start; the call is dpk_sample_noise and the four arguments below are ignored
 *   scale_dev        [scale_rows,n_pts,5] fp32 device or NULL (all ones).  Pose n reads row n % scale_rows, so
 *                    the [F,17,5] noise_scale of dpk_gmm_sample serves N = H*F hypothesis-major poses (the
 *                    reference's noise_scale.repeat(test_times,1,1)); scale_rows must divide N
 *   start_noise_dev  [N,n_pts,5] fp32 device: the draws e (the reference's torch.randn_like(input_uvxyz), :359),
 *                    or NULL: counter-based draws from `seed` at step -1, a counter domain disjoint from
 *                    eta's per-step draws (steps 0..K-1).  A pose's draw depends on the seed and its global
 *                    element index alone, not on tiles, tail plans or N
 * DPK_E_INVALID (with dpk_last_error text) when t_start + 1 >= n_alpha (the reference's index_select raises),
 * when scale_rows < 1 or does not divide N, or when no schedule is set.  Capture-safe like dpk_sample: nothing
 * is allocated, the scalars are captured by value and the pointers are read at replay.  No fixture of the
 * reference pins this path (its :363 never executes); the yardstick is the oracle's loop started from the x_T
 * that line gives in torch. */
int dpk_sample_start(dpk_handle* h, const float* x_dev, float* out_dev, float* xs_dev, float* x0s_dev,
                     int N, uint64_t seed, const float* noise_dev,
                     int t_start, const float* scale_dev, int scale_rows, const float* start_noise_dev,
                     void* stream);

/* The start alone, x_T into xT_dev [N,n_pts,5] (may be x_dev), for generic model callables whose loop runs on the
 * host: the sibling of dpk_ddim_update.  Arguments, arithmetic, draws and refusals as in dpk_sample_start
 * (t_start >= 0); needs a schedule (its alpha table), no weights.  A pose has n_pts * coords_in floats on every handle. */
int dpk_q_sample(dpk_handle* h, const float* x_dev, float* xT_dev, int N, int t_start,
                 const float* scale_dev, int scale_rows, const float* start_noise_dev,
                 uint64_t seed, void* stream);

/* The forward of the training objective in eval mode (runners/diffpose_frame.py:211-226; dropout off): the
 * denoising loss of N poses, each noised at its own timestep.  For pose n with t = t_dev[n] and element r:
 *   target = e * scale                                    (the reference's e = e * targets_noise_scale)
 *   x_t    = (x0 * sa[t]) + (target * sb[t])              (the four roundings of dpk_q_sample)
 *   eps    = GCNdiff(x_t, mask, t)                         (bitwise dpk_eps of (x_t, t) on this handle)
 *   loss_dev[n] = sum over r ascending of (target - eps)^2, one fp32 accumulator, no FMA
 * with sa[t] = sqrtf(alpha_bar[t + 1]) and sb[t] = sqrtf(1 - alpha_bar[t + 1]) from the table built and uploaded
 * with the schedule, the one dpk_q_sample and dpk_sample_start read: at t_dev == t_start everywhere x_t is bitwise
 * dpk_q_sample's x_T.  The batch mean of loss_dev is the reference's loss_diff (:226).
 *   x0_dev    [N,n_pts,5] the clean poses
 *   t_dev     [N] float, integer-valued, 0 .. n_alpha - 2 (the array dpk_eps takes); the table index is clamped to
 *             that range (NaN reads row 0), so no value reads outside the table
 *   scale_dev [scale_rows,n_pts,5] or NULL (ones); pose n reads row n % scale_rows, which must divide N
 *   noise_dev [N,n_pts,5] the draws e, or NULL: counter-based from `seed` at step -1 (the start's key)
 *   loss_dev [N], xt_dev [N,n_pts,5], eps_dev [N,n_pts,5]: outputs, each optional, at least one non-NULL
 * GCNdiff handles of every kind, every gemm mode the handle has, the handle's key mask and per-pose masks as in
 * dpk_eps.  DPK_E_UNSUPPORTED on a GCNpose handle; DPK_E_INVALID with dpk_sample_start's wording when no schedule
 * is set or scale_rows does not divide N.  On a handle with a persistent sampler instance (dpk_fused) it is dpk_eps's
 * one launch: the noising where the eps-mode tile loads its poses, the sum in its epilogue (the squares staged in LDS,
 * one lane per pose), nothing but the projection rows in scratch; DPK_LOSS_FUSED=0 runs the three-launch form there
 * too (A/B).  Per op it is three launches (noising, the dpk_eps forward, the per-pose sums), with x_t and eps that the
 * caller does not ask for in the call's scratch; x_t alone is the noising kernel on every handle.  Capture-safe like
 * dpk_eps (make the same call once uncaptured first); a captured call keeps the schedule it was captured with. */
int dpk_diff_loss(dpk_handle* h, const float* x0_dev, const float* t_dev, const float* scale_dev, int scale_rows,
                  const float* noise_dev, uint64_t seed, float* loss_dev, float* xt_dev, float* eps_dev, int N,
                  void* stream);

/* The gradient of that objective with respect to every parameter of GCNdiff, in eval mode (dropout off) and fp32:
 * what the reference's loss_diff.backward() leaves in p.grad (runners/diffpose_frame.py:219-229) for
 *   L = sum over n of weight * loss_n
 * so weight = 1 / N gives the gradient of the reference's loss_diff (:226), and a rank that holds a shard of a batch
 * of B poses passes 1 / B, so that the shards' gradients add.
 *   x0_dev, t_dev, scale_dev, scale_rows, noise_dev, seed   exactly dpk_diff_loss's: the noising, the clamped table
 *             index, the counter-based draws at step -1; the handle's key mask and per-pose masks as in dpk_eps
 *   loss_dev  [N] or NULL: the per-pose loss of this call's own forward, the per-op fp32 forward (on a handle with a
 *             persistent sampler instance it is not promised bitwise equal to dpk_diff_loss, which runs the sampler's
 *             tiles; both stand inside the same bar against the float64 model)
 *   grads_dev one flat fp32 array, dL/dtheta of every parameter in the state_dict's order, under its names and in
 *             its torch layouts (nn.Linear [out,in], ChebConv [3,1,in,out], A_hat [n_pts,n_pts]; the fused QKV block
 *             of the arena split back into self_attn.linears.0/1/2).  dpk_param_count entries, entry i described by
 *             dpk_param_layout: its name (valid for the process's life), its offset in floats (a multiple of 4) and its
 *             numel.  The array's extent is the last entry's offset + numel floats; every float of it is written (zero
 *             where a gradient is zero, and in the padding between entries).
 * The gradient of A_hat goes back through the GraphNet Laplacian c_i^-1/2 A_ij c_j^-1/2, c = column sums + 1e-5
 * (models/GraFormer.py:174-178; both uses of a layer); the ChebConvs' adjacency is a constant; the timestep MLP is
 * differentiated down to temb.dense.0, per pose.  No gradient with respect to the input.
 * Every handle runs it on the per-op kernels (csrc/dpk_generic_bwd.inc): a training forward that keeps what the
 * backward reads in the call's scratch (DESIGN.md section 3.4 has the floats per pose), dA = dC W^T on the forward's GEMM
 * kernels against a transposed copy of the weights, dW = A^T dC and every other sum over rows or poses as a store pass
 * of partials over a fixed row partition plus an ordered sum pass (no float atomics): two calls with the same
 * arguments on the same handle give bitwise the same grads_dev.  A handle with a persistent sampler instance builds
 * its per-op model and the transposed weights on the first call (and again after new weights or a new graph), which
 * waits for the device; its sampling path is untouched (dpk_fused stays 1).
 * DPK_E_UNSUPPORTED on a GCNpose handle and when the handle's gemm mode is not 0 (the backward is fp32);
 * DPK_E_STATE when `stream` is capturing (the call allocates); otherwise dpk_diff_loss's refusals and the caller-memory
 * contract above (N = 0 touches nothing). */
int dpk_diff_loss_grad(dpk_handle* h, const float* x0_dev, const float* t_dev, const float* scale_dev, int scale_rows,
                       const float* noise_dev, uint64_t seed, float weight, float* loss_dev, float* grads_dev, int N,
                       void* stream);
/* The same gradient in train mode: dropout at the reference's five sites per layer l, with counter-based masks.
 *   site   id  module of the reference                      tensor the mask covers   rate
 *   attn   0   atten_layers.l.self_attn.dropout (p_attn)    [N, n_head, n_pts, n_pts] drop->attn (reference 0.1)
 *   sub0   1   atten_layers.l.sublayer.0.dropout            [N, n_pts, hid]           drop->sublayer (config.model.dropout)
 *   sub1   2   atten_layers.l.sublayer.1.dropout            [N, n_pts, hid]           drop->sublayer
 *   gc1    3   gconv_layers.l.gconv1.dropout (on the relu)  [N, n_pts, hid]           drop->gconv (reference 0.1)
 *   gc2    4   gconv_layers.l.gconv2.dropout                [N, n_pts, hid]           drop->gconv
 * The mask (this formula is the contract).  Element i is its flat index in the tensor above over the whole batch: for a
 * call whose first pose is global pose `pose0`, i = (pose0 + n) * per_pose + local, per_pose = n_pts * hid, or
 * n_head * n_pts * n_pts for attn.  Element i of (l, site) under drop_seed keeps its value iff (w >> 8) >= thr, with
 *   w    output word i & 3 of Philox4x32-10 at counter {(i >> 2) lo, (i >> 2) hi, l * 8 + site, 0xD809},
 *        key {drop_seed lo, drop_seed hi} (one call serves four consecutive elements),
 *   thr  (uint32) ceilf(p * 16777216.0f), taken once on the host (the product is exact, the decision an integer
 *        comparison).
 * A kept element becomes x * s, s = 1.0f / (1.0f - p) in fp32 taken on the host; a dropped one 0.0f.  Rate 0 keeps
 * everything and multiplies by nothing.  Counter word 3 (0xD809) is not the normal draws' (0x5EED): the masks are
 * disjoint from e and from eta's draws under an equal seed.  Forward and backward each recompute the decision from the
 * counter; no mask is stored, the call's scratch is dpk_diff_loss_grad's.
 *   drop, drop_seed  the rates and the masks' key
 *   pose0            the global index of the call's first pose: the shards of one batch, each with weight 1 / B, add up
 *                    to the unsharded gradient.  pose0 keys the masks only: it does not move the counter-based e of a
 *                    NULL noise_dev, which stays normal_noise(seed, -1, element of this call).
 *   loss_dev         the train-mode loss per pose
 * Everything else is dpk_diff_loss_grad's: the arguments, the layout of grads_dev, the caller-memory contract (N = 0
 * touches nothing), bitwise repeatability, its refusals.  With all three rates 0 the outputs are bitwise
 * dpk_diff_loss_grad's (the same launches).  DPK_E_INVALID, with the offending value in dpk_last_error, for a NULL
 * drop, a rate that is negative, NaN or >= 1, or pose0 < 0. */
typedef struct { float sublayer, attn, gconv; } dpk_dropout;
int dpk_diff_loss_grad_train(dpk_handle* h, const float* x0_dev, const float* t_dev, const float* scale_dev,
                             int scale_rows, const float* noise_dev, uint64_t seed, float weight,
                             const dpk_dropout* drop, uint64_t drop_seed, int64_t pose0, float* loss_dev,
                             float* grads_dev, int N, void* stream);
/* The mask itself, without a handle (to replay a step elsewhere): keep_dev[i - first] = 1 or 0 for elements
 * first .. first + n - 1 of (layer, site) under drop_seed at rate p; exactly n bytes written on `stream` of the
 * current device, n = 0 touches nothing.  DPK_E_INVALID for a negative layer, a site outside 0..4, a rate outside
 * [0, 1), negative first or n, or a NULL keep_dev with n > 0. */
int dpk_dropout_mask(uint64_t drop_seed, int layer, int site, float p, int64_t first, int64_t n, uint8_t* keep_dev,
                     void* stream);
/* The draws of one training step (runners/diffpose_frame.py:214-218) without a handle: e and the antithetic t of poses
 * pose0 .. pose0 + n - 1 of a global batch of `batch` poses, every value a function of its seed and its global index
 * alone, so a rank's rows are bitwise the rows of the whole batch's draw.  These formulas are the contract.
 *   e_dev [n,pose_floats] or NULL.  For global pose p = pose0 .. pose0 + n - 1 and element r of it,
 *             e_dev[(p - pose0) * pose_floats + r] = normal_noise(e_seed, step = -1, idx = p * pose_floats + r),
 *         the draw of the sampler and the loss calls: Philox4x32-10 at counter {idx lo, idx hi, 0xFFFFFFFF, 0x5EED}
 *         under the key {e_seed lo, e_seed hi}, u1 = ((c0 >> 8) + 1) / 2^24, u2 = (c1 >> 8) / 2^24,
 *         z = sqrtf(-2 logf(u1)) * cosf(6.283185307179586f * u2) in fp32.  idx is 64-bit, both counter words are live.
 *         At pose0 = 0 it is bitwise what dpk_diff_loss, dpk_diff_loss_grad(_train) and dpk_q_sample draw for a NULL
 *         noise_dev under seed = e_seed; a shard passes its rows as noise_dev.
 *   t_dev [n] or NULL: float, integer-valued, the array dpk_diff_loss_grad takes.  The reference's
 *         cat([r, T - r - 1])[:batch] of h = batch / 2 + 1 draws r: with q = p < h ? p : p - h (p - h < h always),
 *             w = splitmix64's output mixer on t_seed + 0x9E3779B97F4A7C15 * (q + 1) mod 2^64
 *                 (the 64-bit word behind dpk_gmm_sample's seeded uniforms at counter q),
 *             r = ((w >> 32) * T) >> 32,        t = p < h ? r : T - 1 - r,
 *         integer arithmetic only; T = the number of diffusion timesteps, t in 0 .. T - 1.
 * One elementwise launch on `stream` of the current device.  The caller-memory contract above: exactly n * pose_floats
 * and n floats written, pointers 4-byte aligned, a NULL output untouched, n = 0 returns DPK_OK and touches nothing;
 * capture-safe (nothing allocated, every scalar passed by value).  DPK_E_INVALID, before anything is touched, for T < 1 or
 * T > 2^24, batch < 1, pose0 < 0, n < 0, pose0 + n > batch, pose_floats < 1, or both outputs NULL with n > 0. */
int dpk_train_draws(uint64_t e_seed, uint64_t t_seed, int T, int64_t batch, int64_t pose0, int n, int pose_floats,
                    float* e_dev, float* t_dev, void* stream);
/* Parameters of a GCNdiff handle (0 for NULL or a GCNpose handle), and entry i of their layout in grads_dev. */
int dpk_param_count(const dpk_handle* h);
int dpk_param_layout(const dpk_handle* h, int i, const char** name, int64_t* offset, int64_t* numel);

/* The optimiser step on the device: clip_grad_norm_, Adam and the EMA of the reference's loop body
 * (runners/diffpose_frame.py:229-236) on parameters that stay on the device for a training run.  Every array below is
 * flat fp32 in grads_dev's layout (dpk_param_layout), F floats = the last entry's offset + numel.
 *   beta1, beta2, eps, amsgrad   torch.optim.Adam's (the reference: 0.9, 0.999, config.optim.eps, config.optim.amsgrad)
 *   grad_clip                    config.optim.grad_clip; <= 0: no clipping (the norm is still computed and reported)
 *   ema_mu                       config.model.ema_rate; < 0: no EMA shadow
 * beta1, beta2 and ema_mu are read as the decimals they were written as: the shortest decimal that rounds to the float
 * passed (0.999f is 0.999), in double.  1 - beta2 from the float itself would be off by 1.3e-5 of its value, and with it
 * every exp_avg_sq.
 *
 * dpk_train_begin (a configuration call: it waits for the device) needs a GCNdiff handle with weights and a graph.  It
 * allocates params (from the loaded weights, back in their torch layouts; A_hat as loaded), exp_avg and exp_avg_sq
 * (zero), max_exp_avg_sq (zero, with amsgrad) and the EMA shadow (a copy of params, with ema_mu >= 0), sets the step
 * count to 0, and builds what dpk_diff_loss_grad's first call builds (a persistent-sampler handle's per-op model, the
 * transposed weights).  DPK_E_UNSUPPORTED on a GCNpose handle; DPK_E_STATE without weights or a graph, or when already
 * begun; DPK_E_INVALID, the offending value in dpk_last_error, for a NULL cfg, a beta outside [0, 1), eps < 0 or NaN,
 * ema_mu > 1 or NaN.
 *
 * dpk_train_apply is one step: four launches on `stream`, no host wait, no allocation.  grads_dev (exactly F floats,
 * read only; what dpk_diff_loss_grad(_train) wrote, all-reduced by the caller where there are several ranks) and
 * gnorm_dev (one float, or NULL) follow the caller-memory contract above.  In order, every operation one fp32 rounding
 * unless it says fp64, nothing fused but the two fmaf of step 3 (this order is the contract):
 *   1. norm.  The squares of all F floats are summed in fp64 (each square exact) over a fixed partition: part b of 256
 *      holds elements [b c, (b + 1) c), c = ceil(F / 256); thread t of 256 adds its elements t, t + 256, ... of the part
 *      in ascending order; the 256 threads' sums, then the 256 parts' sums, are added in a binary tree (x[i] += x[i + w],
 *      w = 128, 64, .. 1).  gnorm = (float) sqrt(sum), the root in fp64.  No atomics: the same input gives the same bits.
 *   2. clip.  coef = fminf(grad_clip / (gnorm + 1e-6f), 1.0f), a NaN quotient staying NaN (torch's clamp); 1.0f with
 *      grad_clip <= 0.  It stays on the device.  g = grads_dev[i] * coef; a non-finite norm propagates as in
 *      clip_grad_norm_(error_if_nonfinite=False).
 *   3. Adam, weight_decay 0, at step k = count + 1.  The host takes, in double and each rounded once to fp32:
 *      omb1 = 1 - beta1, omb2 = 1 - beta2, step_size = lr / (1 - beta1^k), bc2_sqrt = sqrt(1 - beta2^k).  Per element:
 *        m = fmaf(g - m, omb1, m)                     (the difference rounded, then one rounding over product + sum)
 *        v = fmaf(omb2 * g, g, v * beta2)             (omb2 * g and v * beta2 rounded, then one rounding)
 *        vmax = v > vmax or v is NaN ? v : vmax;  used = vmax          (amsgrad; otherwise used = v)
 *        p = p - (step_size * m) / (sqrtf(used) / bc2_sqrt + eps)
 *      (torch's single-tensor path: lerp_, mul_ + addcmul_, maximum, addcdiv_, with the two fusions torch's CPU kernels
 *      make in lerp_ and addcmul_; division and square root correctly rounded).
 *   4. EMA (with a shadow): shadow = a * p + b * shadow, a = (float)(1.0 - mu), b = (float)mu, two products and a sum:
 *      EMAHelper.update's (1. - mu) * p + mu * shadow on fp32 tensors.
 *   5. refresh.  Everything the per-op forward and backward read is rewritten from params, on the device: the forward's
 *      weight arena and its gemm_sk copies, the transposed arena and its copies, the A_hat rows, and each layer's
 *      GraphNet Laplacian and its transpose, computed in the weight load's order (column sums ascending in fp32,
 *      1.0f / sqrtf(r + 1e-5f), (d_i a_ij) d_j).  The result is bitwise what dpk_load_weights of the same parameters
 *      builds (csrc/dpk_train_layout.inc, checked on the CPU).  The Chebyshev terms do not depend on the parameters.
 * The padding between entries carries zero gradients and stays zero (with eps = 0 it becomes 0 / 0).
 * On a per-op handle every later call on `stream` (dpk_eps, dpk_sample, dpk_diff_loss, the gradient calls, recorded
 * K-step loops) reads the new weights.  On a persistent-sampler handle the gradient calls do too (they run the per-op
 * model), but the sampler's own arenas and the host staging are not rewritten per step: dpk_sample*, dpk_eps and
 * dpk_diff_loss return DPK_E_STATE, naming dpk_train_sync, from an apply until dpk_train_sync has run.  Calls in flight
 * on other streams that read the weights are the caller's to order against the step.
 * DPK_E_STATE when training has not begun or `stream` is capturing; DPK_E_INVALID for a NULL grads_dev or a negative
 * or NaN lr.
 *
 * dpk_train_sync (a configuration call: it waits for the device) downloads params, refills the host staging and, on a
 * persistent-sampler handle, repacks and uploads the sampler's arenas (recomputing the schedules' timestep
 * projections).  The per-op arenas stay as the refresh left them.
 * dpk_train_end syncs and frees the trainer's arrays: the handle is an ordinary one with the trained weights.  While
 * training, dpk_load_weights and dpk_set_graph return DPK_E_STATE; dpk_destroy frees everything.
 *
 * dpk_train_get / dpk_train_set copy exactly F floats between device memory and one array on `stream`, for
 * checkpoints: which = 0 params, 1 exp_avg, 2 exp_avg_sq, 3 max_exp_avg_sq, 4 the EMA shadow (3 without amsgrad, 4
 * without a shadow, or a value outside 0..4: DPK_E_INVALID).  get: *step (may be NULL) receives the step count.  set:
 * step >= 0 sets the count, -1 leaves it; setting params runs the refresh (and a persistent-sampler handle needs a
 * sync again); DPK_E_STATE on a capturing stream. */
typedef struct {
    float beta1, beta2, eps;
    int   amsgrad;
    float grad_clip;
    float ema_mu;
} dpk_optim_config;
int dpk_train_begin(dpk_handle* h, const dpk_optim_config* cfg);
int dpk_train_apply(dpk_handle* h, const float* grads_dev, float lr, float* gnorm_dev, void* stream);
int dpk_train_sync(dpk_handle* h);
int dpk_train_get(dpk_handle* h, int which, float* out_dev, int64_t* step, void* stream);
int dpk_train_set(dpk_handle* h, int which, const float* in_dev, int64_t step, void* stream);
int dpk_train_end(dpk_handle* h);

/* One DDIM update for an externally computed eps (generic model callables):
 * the per-element body of common/utils_diff.py:59-65 for schedule step `step`
 * (0 = first executed step, t = seq[K-1]).  x0_dev may be NULL; xnext_dev may be xt_dev. */
int dpk_ddim_update(dpk_handle* h, const float* xt_dev, const float* eps_dev, float* xnext_dev,
                    float* x0_dev, int64_t n_elems, int step, uint64_t seed, void* stream);

/* dpk_ddim_update with this step's draw z (noise_dev [n_elems] fp32 device; NULL = counter-based). */
int dpk_ddim_update_noise(dpk_handle* h, const float* xt_dev, const float* eps_dev, float* xnext_dev,
                          float* x0_dev, int64_t n_elems, int step, uint64_t seed, const float* noise_dev,
                          void* stream);

/* GCNpose front-end (models/gcnpose.py:55-113) for a handle created with coords_in 2,
 * coords_out 3 (create_pose_model, runners/diffpose_frame.py:134-154), fused with the
 * sampler-input assembly of test_hyber (runners/diffpose_frame.py:337-342):
 *   x2d_dev   [N,17,2]  input_2d
 *   xyz_dev   [N,17,3]  model_pose(input_2d) as returned by the model, or NULL
 *   uvxyz_dev [H,N,17,5] cat(input_2d, root-processed xyz).repeat(H,1,1), or NULL
 *   root_mode 0: what the reference's in-place `xyz[:, :, :] -= xyz[:, :1, :]` yields on CPU
 *                torch (aliasing: only the root row is zeroed; pinned by golden g5)
 *             1: true root-relative (xyz - xyz[:, :1]);  2: no root subtraction
 * The key mask of dpk_set_mask applies (GCNpose.forward(x, mask)).  At least one of
 * xyz_dev / uvxyz_dev must be non-NULL. */
int dpk_pose(dpk_handle* h, const float* x2d_dev, float* xyz_dev, float* uvxyz_dev, int N, int H,
             int root_mode, void* stream);

/* Per-frame evaluation of the sampler output (test_hyber, runners/diffpose_frame.py:382-387),
 * handle-free, one thread per frame, fp64:
 *   out_uvxyz_dev [H,F,17,5] sampler output (hypothesis-major, as generalized_steps returns it)
 *   targets_dev   [F,17,3]   targets_3d
 *   root_mode     as in dpk_pose, applied to prediction and target
 *   p1_dev [F] (double)      MPJPE of each frame (metres; common/utils.py:103-127 per frame)
 *   p2_dev [F] (double)      P-MPJPE of each frame, after the best similarity transform
 *                            (common/loss.py:25-64 / common/utils.py:155-187)
 *   xyz_dev [F,17,3] or NULL the hypothesis-mean, root-processed xyz (output_xyz)
 * Returns DPK_OK, DPK_E_INVALID or DPK_E_HIP (no handle, so no dpk_last_error text). */
int dpk_pose_metrics(const float* out_uvxyz_dev, const float* targets_dev, int F, int H, int root_mode,
                     double* p1_dev, double* p2_dev, float* xyz_dev, void* stream);

/* dpk_pose_metrics for a skeleton of n_pts joints, 2 <= n_pts <= 32 (the range of dpk_create):
 *   out_uvxyz_dev [H,F,n_pts,5], targets_dev [F,n_pts,3], xyz_dev [F,n_pts,3] or NULL
 * Joint 0 is the root.  One kernel instance per joint count, each with the frame in registers (no
 * private memory); the arithmetic and its order are those of the 17-joint call, which is this call
 * with n_pts = 17.  An n_pts outside 2..32 returns DPK_E_INVALID before anything else is looked at;
 * the other refusals are dpk_pose_metrics's. */
int dpk_pose_metrics_n(const float* out_uvxyz_dev, const float* targets_dev, int F, int H, int n_pts,
                       int root_mode, double* p1_dev, double* p2_dev, float* xyz_dev, void* stream);

/* GMM 2D-keypoint sampling of the input pipeline: replaces
 * PoseGenerator_gmm.__getitem__ (common/generators.py:24-53) for a whole batch.
 *   gmm_dev      [n_src,17,kernel_n,5] fp32  per joint: [w, mu_u, mu_v, var_u, var_v] x kernel_n
 *   poses3d_dev  [n_src,17,3] fp32           3D poses (made root-relative here, generators.py:19)
 *   index_dev    [F] int64 or NULL           source frame of each output (taken modulo n_src, as
 *                                            generators.py:26-29); NULL = 0..F-1
 *   u_dev        [F,17] fp64 or NULL         the uniform draw np.random.choice consumes for each
 *                                            joint (RandomState.random_sample, in frame-then-joint
 *                                            order); NULL = counter-based uniforms from `seed`
 *   atol                                     numpy's tolerance on sum(w) = 1 (sqrt(eps) of the
 *                                            weights' dtype: 3.4526698e-4 for float32)
 *   uvxyz_dev, noise_scale_dev  [F,17,5] fp32 outputs (uvxyz = [mu_u, mu_v, xyz - xyz_root],
 *                                            noise_scale = [var_u, var_v, 1, 1, 1])
 *   status_dev   one int (device)            0, or an OR of 1 (a negative weight) and 2 (weights
 *                                            not summing to 1 within atol): numpy's ValueErrors
 * Component selection is numpy's RandomState.choice(kernel_n, 1, p) bit for bit given u.
 * Returns DPK_OK, DPK_E_INVALID (kernel_n outside 1..64, bad pointers) or DPK_E_HIP. */
int dpk_gmm_sample(const float* gmm_dev, const float* poses3d_dev, int n_src, int kernel_n,
                   const int64_t* index_dev, int F, const double* u_dev, uint64_t seed, double atol,
                   float* uvxyz_dev, float* noise_scale_dev, int* status_dev, void* stream);

/* The same for float64 arrays (numpy data kept in double): weights and poses are read as
 * double, the root-relative subtraction runs in double and the outputs are rounded to float32 —
 * the reference's order (generators.py:19 on the float64 array, .float() at :46-50). */
int dpk_gmm_sample_f64(const double* gmm_dev, const double* poses3d_dev, int n_src, int kernel_n,
                       const int64_t* index_dev, int F, const double* u_dev, uint64_t seed, double atol,
                       float* uvxyz_dev, float* noise_scale_dev, int* status_dev, void* stream);

/* dpk_gmm_sample / dpk_gmm_sample_f64 for a skeleton of n_pts joints, 2 <= n_pts <= 32:
 *   gmm_dev [n_src,n_pts,kernel_n,5], poses3d_dev [n_src,n_pts,3], u_dev [F,n_pts] or NULL,
 *   uvxyz_dev, noise_scale_dev [F,n_pts,5]
 * Joint 0 is the root.  The seeded uniform of (frame f, joint j) is keyed by f * n_pts + j.  The
 * 17-joint calls are these with n_pts = 17.  An n_pts outside 2..32 returns DPK_E_INVALID before
 * anything else is looked at; the other refusals are dpk_gmm_sample's. */
int dpk_gmm_sample_n(const float* gmm_dev, const float* poses3d_dev, int n_src, int n_pts, int kernel_n,
                     const int64_t* index_dev, int F, const double* u_dev, uint64_t seed, double atol,
                     float* uvxyz_dev, float* noise_scale_dev, int* status_dev, void* stream);
int dpk_gmm_sample_f64_n(const double* gmm_dev, const double* poses3d_dev, int n_src, int n_pts, int kernel_n,
                         const int64_t* index_dev, int F, const double* u_dev, uint64_t seed, double atol,
                         float* uvxyz_dev, float* noise_scale_dev, int* status_dev, void* stream);

/* GEMM arithmetic of the sampler's transformer/ResChebGC GEMMs (not part of the reference
 * interface; the reference computes everything in fp32 on its device):
 *   mode 0 (default): fp32 MFMA (v_mfma_f32_16x16x4_f32), fp32 accumulate;
 *   mode 1: 3-term fp16 split (a = a_hi + a_lo, w*64 = w_hi + w_lo; a_hi w_hi + a_hi w_lo +
 *           a_lo w_hi on v_mfma_f32_16x16x32_f16, fp32 accumulate), ~fp32-accurate products;
 *   mode 2: bf16 (a and w rounded to bf16, one v_mfma_f32_16x16x32_bf16 product, fp32
 *           accumulate; since round 5 also attention's score and P.V products, and the GraphNet
 *           products from bf16 activations against L_g as a bf16 hi + lo pair): a reduced-precision
 *           mode for the tolerance study of BASELINE config 3.
 * The input/output ChebConvs, LayerNorm, the softmax and the DDIM update stay fp32 in all modes, and
 * so do attention and the GraphNet products in modes 0 and 1.
 * Applies to later dpk_sample / dpk_eps / dpk_pose calls on this handle.  Any of 0..2 is accepted
 * here; which of them a handle runs depends on its shape (dpk_gemm_modes): all three at hid 96 / 4
 * heads, modes 0 and 1 at hid 128 / 8 or 4 heads and hid 64 / 2 or 4 heads on the persistent sampler,
 * mode 0 alone per op; modes 0 and 1 at all five of those shapes on fewer than 17 joints (padded tiles), where mode 2
 * is refused here, at the set, with the joint count in the message.  A call in a mode the handle lacks returns
 * DPK_E_UNSUPPORTED, its message naming the mode and the shape.  Range: mode 1 needs every GEMM weight |w| < 1015 at every width (else those
 * calls return DPK_E_UNSUPPORTED) and GEMM inputs (LayerNorm/attention/graph/Chebyshev outputs) below
 * 65504 in magnitude; an overflow there shows as non-finite outputs. */
int dpk_set_gemm_mode(dpk_handle* h, int mode);

/* The gemm modes calls on this handle run: bit m set when mode m does (0b111 at hid 96 / 4 heads,
 * 0b011 on the four other persistent-sampler shapes, 0b001 on a per-op handle; 0 for a null handle). */
int dpk_gemm_modes(const dpk_handle* h);

/* 1 when a persistent sampler instance serves the handle (17 joints, or fewer on padded tiles), 0 when its calls
 * run per op (NULL: 0).  A padded handle lists gemm modes 0b011 and refuses dpk_set_gemm_mode(h, 2) and
 * dpk_set_tile_waves(h, 8) with DPK_E_UNSUPPORTED, naming its joint count. */
int dpk_fused(const dpk_handle* h);

/* How dpk_sample balances a partial last round of tiles (4 poses per workgroup, one workgroup
 * per CU per round; not part of the reference interface, which has no tiles):
 *   plan 0: the last round in 4-pose tiles like the others;
 *   plan 1: when it holds at most 2 poses per CU, one round of 2-pose tiles (about 0.6 of a
 *           round);
 *   plan 2 (default): when at least one full round precedes it and it holds at most half a
 *           round of tiles, each of its tiles runs its K steps as two halves on two CUs (the
 *           first half's x_t handed over through `out` and a device flag), so the last round
 *           costs about half a round; otherwise plan 1.
 * Plans 0 and 2 give bitwise the same outputs (the same tiles, the same per-step arithmetic);
 * plan 1 agrees within fp32 rounding (other rows on the 4-row tail path).  The plan-2 handoff
 * assumes no dispatch order: a second half whose first half has not started after a few ms runs
 * the whole tile itself (correct output, only slower; dpk_debug_split counts these), and a first
 * half that then starts leaves without writing.  Plan 2 needs one of 64 flag slots per handle: an
 * uncaptured call holds one until its launch has completed, a capture one per capturing stream
 * for the graph's life; a call that finds none free runs plan 1.  dpk_eps and dpk_pose (one step)
 * use plan 1 for plan 2.  The environment variable DPK_TAIL_SPLIT sets a new handle's plan. */
int dpk_set_tail_plan(dpk_handle* h, int plan);

/* Waves of the workgroup that runs a 4-pose tile of dpk_sample: 4 (one per SIMD), 8 (two per SIMD:
 * each SIMD's GEMM column tiles split between its two waves, the per-pose phases between the two
 * waves of a pose), or 0 (default): what the measurements chose for the handle's GEMM mode.  All
 * 4-pose tiles of a launch, the halves of step-split tiles included, run on the same instance, so
 * plans 0 and 2 stay bitwise equal; the 2-pose tail round, dpk_eps and dpk_pose always run 4 waves.
 * Both instances compute bitwise the same outputs.  Handles of another model shape, or of fewer
 * than 17 joints on padded tiles (plain 4-wave tiles, no tail plans), accept 0 and 4.  With an
 * adjacency outside the compiled H36M pattern (the dense Chebyshev path) 0 means 4 in every mode: the dense
 * 8-wave kernels exceed their register budget and run only when 8 is asked for.
 * The environment variable DPK_TILE_WAVES sets a new handle's value. */
int dpk_set_tile_waves(dpk_handle* h, int waves);

/* Launch timing of the sampler kernel itself: with enable != 0, every dpk_sample /
 * dpk_eps brackets its sampler-kernel launch with a pair of HIP events on the
 * caller's stream.  dpk_profile_read waits for the recorded events and returns up to
 * `cap` elapsed times in ms (oldest first), then clears them. */
int dpk_profile(dpk_handle* h, int enable);
int dpk_profile_read(dpk_handle* h, float* ms_out, int cap, int* count);

/* Test hooks (not part of the reference interface).
 * dpk_debug_split: mode 0 normal; 1: step-split first halves start ~100 ms late and second halves
 * do not wait for an unstarted first half, so every split tile takes the recompute path; 2: second
 * halves do not wait for an unstarted first half.  With `fallbacks` non-NULL, waits for the device
 * and returns (then clears) the number of second halves that ran their tile's first-half steps.
 * dpk_debug_resources: out[0..7] = captures holding resources, captures whose graph holds our
 * user object, captures released (graph gone, not yet recycled), free flag slots, retired
 * schedules, spare dpk_eps capacity (poses); generic-shape handles also: K-step loops recorded as
 * hipGraphs (out[6]) and the spare capture scratch in KiB (out[7]).
 * dpk_debug_generic_forms: which kernel forms of the per-op path (csrc/dpk_generic.inc) the handle's calls
 * have launched since the last read, then cleared: *forms = an OR of one bit per form the host chooses
 * between per call, from the shape, the batch and pointer alignment (dpkg::GenForm; bit 0 gemm_narrow,
 * 1 gemm_sk<4>, 2 gemm_sk<2>, 3..8 gemm<128|64|32> with 16-byte / scalar loads, 9..11 attention staged
 * + vector / staged + scalar / unstaged, 12..13 graph staged / unstaged, 14..15 cheb_basis staged /
 * unstaged).  Host bookkeeping only: it waits for nothing, and a K-step loop recorded as a hipGraph sets
 * its bits when it is recorded, not when it is replayed.  0 on a handle that runs a persistent sampler.
 * dpk_debug_sampler_kernels: which compiled kernels of the persistent sampler the handle's calls have launched
 * since the last read, then cleared: up to `cap` distinct ids in ids[], their full number in *count (ids past
 * `cap` are dropped: 256 words hold any answer).  An id names one sample_kernel<MODE, SPARSE, G16, ZM, START,
 * PAD> of one tile: bits 0..3 the tile (0 dpk: hid 96 / 4 heads, 4 poses on 4 waves; 1 dpk8: on 8 waves; 2 dpk2:
 * 2 poses; 3 dpkw: hid 128 / 8; 4 dpkw4: hid 128 / 4; 5 dpkn: hid 64 / 2; 6 dpkn4: hid 64 / 4), bits 4..5 MODE
 * (0 sample, 1 eps, 2 pose), bit 6 SPARSE (the compiled H36M pattern), bits 7..8 G16 (the gemm mode), bit 9 ZM
 * (the caller's noise), bit 10 START (dpk_sample_start), bit 11 PAD (fewer than 17 joints).  The id is written
 * where the kernel is launched, from that launch's own template arguments.  Host bookkeeping only: it waits for
 * nothing, and a captured launch counts when it is recorded, not when its graph is replayed.  A per-op handle
 * returns 0 ids.  With h == NULL: every id compiled into the library (cap may be 0 to ask for *count alone). */
int dpk_debug_split(dpk_handle* h, int mode, int* fallbacks);
int dpk_debug_resources(dpk_handle* h, int* out, int n);
int dpk_debug_generic_forms(dpk_handle* h, unsigned* forms);
/* dpk_debug_grad_forms: the same for dpk_diff_loss_grad(_train), then cleared: *gemm_forms the dpk_debug_generic_forms bits of
 * its training forward and of its dX GEMMs, *bwd_forms the backward's own (bit 0 dw_partial with 16-byte loads, 1 with
 * scalar loads, 2 attention_bwd with the pose's rows staged in LDS, 3 ln_bwd, 4..5 graph on L_g^T staged / unstaged,
 * 6 cheb_t, 7 dlg_partial staged (+ dlg_chain), 8 the timestep MLP's backward, 9 attention_bwd unstaged, 10 dlg_partial
 * unstaged; of a train-mode call, each only where its site's rate is not 0: 11 attention with dropout on the
 * probabilities, forward and backward, 12 the sublayers' drop + residual add, 13 the dropout on a ChebConv's ReLU). */
int dpk_debug_grad_forms(dpk_handle* h, unsigned* gemm_forms, unsigned* bwd_forms);
int dpk_debug_sampler_kernels(dpk_handle* h, uint32_t* ids, int cap, int* count);

/* Poses per workgroup of the sampler kernel and its static LDS bytes (for docs/bench). */
int dpk_kernel_geometry(int* poses_per_workgroup, int* threads_per_workgroup, int* lds_bytes);

const char* dpk_last_error(const dpk_handle* h);
void dpk_destroy(dpk_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* DIFFPOSE_KERNELS_H */
