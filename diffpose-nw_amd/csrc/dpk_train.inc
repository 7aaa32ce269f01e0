// dpk_train.inc — the optimiser step on the device (dpk_train_*): the parameters, Adam's moments and the EMA shadow
// as flat fp32 arrays in dpk_param_layout's order, resident for a training run.  One step is four launches on the
// caller's stream: the gradient's norm in two (fp64 partial sums over a fixed partition, then an ordered final pass
// that also leaves the clip coefficient on the device), clip + Adam + EMA in one pass over the arrays, and one gather
// that rewrites every arena the per-op forward and backward read from the new parameters (dpk_train_layout.inc says
// where each float comes from).  Included after dpk_generic_bwd.inc.

namespace dpkg {

constexpr int NORM_PARTS = 256;      // the fixed partition of the norm: parts x 256 threads, whatever the device

// part b sums the squares of g[b * chunk .. (b + 1) * chunk) in fp64 (the square of an fp32 is exact there): thread t
// the elements t, t + 256, ... of the part in ascending order, then a tree over the 256 threads in a fixed order
__global__ __launch_bounds__(256) void train_norm_partial(const float* __restrict__ g, long long n, long long chunk,
                                                          double* __restrict__ partial) {
    __shared__ double red[256];
    const long long lo = (long long)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
    double acc = 0.0;
    for (long long i = lo + threadIdx.x; i < hi; i += 256) {
        const double v = (double)g[i];
        acc += v * v;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// The parts in the same tree, the root in fp64 rounded once to fp32, and the clip coefficient
// (torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max=1.0), fp32; a NaN stays a NaN as in torch's
// clamp).  scal[0] = the norm, scal[1] = the coefficient (1 with clip <= 0)
__global__ __launch_bounds__(NORM_PARTS) void train_norm_final(const double* __restrict__ partial, float clip,
                                                               float* __restrict__ scal, float* __restrict__ gnorm) {
    __shared__ double red[NORM_PARTS];
    red[threadIdx.x] = partial[threadIdx.x];
    __syncthreads();
    for (int w = NORM_PARTS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const float gn = (float)sqrt(red[0]);
    float coef = 1.0f;
    if (clip > 0.f) {
        const float c = clip / (gn + 1e-6f);
        coef = c != c ? c : fminf(c, 1.0f);
    }
    scal[0] = gn, scal[1] = coef;
    if (gnorm) *gnorm = gn;
}

struct AdamConsts {
    float omb1, beta2, omb2;         // 1 - beta1, beta2, 1 - beta2
    float step_size, bc2_sqrt, eps;  // lr / (1 - beta1^k), sqrt(1 - beta2^k)
    float ema_a, ema_b;              // 1 - mu, mu
};

// Clip, Adam and the EMA, four consecutive floats a thread; every operation below is one fp32 rounding, in this order,
// the two fmaf the only fused ones (the library is built with -ffp-contract=off; torch's CPU lerp_ and addcmul_ fuse
// the same two): the contract of include/diffpose_kernels.h.  g may sit at any
// 4-byte boundary (the caller's), the state arrays are the library's own
__global__ __launch_bounds__(256) void train_adam(const float* __restrict__ g, const float* __restrict__ scal, float* __restrict__ p,
                                                  float* __restrict__ m, float* __restrict__ v, float* __restrict__ vmax,
                                                  float* __restrict__ shadow, long long n4, AdamConsts c) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= n4) return;
    const float coef = scal[1];
    float4 P = reinterpret_cast<float4*>(p)[q], Mo = reinterpret_cast<float4*>(m)[q], V = reinterpret_cast<float4*>(v)[q];
    float4 X = vmax ? reinterpret_cast<float4*>(vmax)[q] : float4{0.f, 0.f, 0.f, 0.f};
    float4 S = shadow ? reinterpret_cast<float4*>(shadow)[q] : float4{0.f, 0.f, 0.f, 0.f};
    float* pp = &P.x;
    float* mm = &Mo.x;
    float* vv = &V.x;
    float* xx = &X.x;
    float* ss = &S.x;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float gi = g[4 * q + e] * coef;
        mm[e] = __fmaf_rn(gi - mm[e], c.omb1, mm[e]);                  // lerp_: one rounding over the product and sum
        vv[e] = __fmaf_rn(c.omb2 * gi, gi, vv[e] * c.beta2);           // mul_ then addcmul_: (value g) g + v, fused
        float used = vv[e];
        if (vmax) {
            if (vv[e] > xx[e] || vv[e] != vv[e]) xx[e] = vv[e];     // torch.maximum: a NaN goes through
            used = xx[e];
        }
        const float den = sqrtf(used) / c.bc2_sqrt + c.eps;
        pp[e] = pp[e] - (c.step_size * mm[e]) / den;
        const float a = c.ema_a * pp[e], b = c.ema_b * ss[e];
        ss[e] = a + b;
    }
    reinterpret_cast<float4*>(p)[q] = P, reinterpret_cast<float4*>(m)[q] = Mo, reinterpret_cast<float4*>(v)[q] = V;
    if (vmax) reinterpret_cast<float4*>(vmax)[q] = X;
    if (shadow) reinterpret_cast<float4*>(shadow)[q] = S;
}

// The refresh: float i of the four arenas laid end to end (end[a]: where arena a ends) from its source in the flat
// parameters, train_gather of dpk_train_layout.inc on the device.  ahat: each layer's A_hat offset in the flat array
struct RefreshDst {
    float* dst[4];
    unsigned end[4];
};
__global__ __launch_bounds__(256) void train_refresh(RefreshDst d, const int* __restrict__ idx, const int* __restrict__ ahat,
                                                     const float* __restrict__ p, int J) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= d.end[3]) return;
    const int c = idx[i];
    if (c == -1) return;             // TRAIN_KEEP
    float val;
    if (c >= 0) val = p[c];
    else {                           // TRAIN_LG: stage_load's GraphNet Laplacian, operation for operation
        const int e = -2 - c, JJ = J * J, r = e % JJ, ii = r / J, jj = r % J;
        const float* A = p + ahat[e / JJ];
        float ri = 0.f, rj = 0.f;
        for (int k = 0; k < J; ++k) ri += A[k * J + ii], rj += A[k * J + jj];
        const float di = 1.0f / sqrtf(ri + 1e-5f), dj = 1.0f / sqrtf(rj + 1e-5f);
        val = (di * A[ii * J + jj]) * dj;
    }
    const int a = i < d.end[0] ? 0 : i < d.end[1] ? 1 : i < d.end[2] ? 2 : 3;
    d.dst[a][i - (a ? d.end[a - 1] : 0u)] = val;
}

}  // namespace dpkg

// ---------------------------------------------------------------------------------------
// Host side

struct TrainState {
    dpk_optim_config cfg{};
    double beta1 = 0, beta2 = 0, mu = 0;     // cfg's as the decimals they were written as (train_decimal)
    size_t F = 0;
    float* state = nullptr;      // device, one allocation: params | exp_avg | exp_avg_sq | [max_exp_avg_sq] | [shadow]
    float* arr[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};     // by dpk_train_get's `which`
    double* partial = nullptr;   // device: NORM_PARTS partial sums, then scal (norm, coefficient)
    float* scal = nullptr;
    int* idx = nullptr;          // device: the four arenas' sources end to end, then the layers' A_hat offsets
    int* ahat = nullptr;
    dpkg::RefreshDst dst{};
    int64_t step = 0;
    bool host_stale = false;     // the host staging (and a sampler instance's arenas) are behind `params`
    std::vector<GradEntry> entries;
};

static void train_free(TrainState* t) {
    if (!t) return;
    for (void* p : {(void*)t->state, (void*)t->partial, (void*)t->idx})
        if (p) (void)hipFree(p);
    delete t;
}

static void train_refresh_launch(const dpk_handle* h, hipStream_t st) {
    const TrainState* t = h->train;
    hipLaunchKernelGGL(dpkg::train_refresh, dim3(gen_blocks(t->dst.end[3])), dim3(256), 0, st, t->dst, t->idx, t->ahat,
                       t->arr[0], h->stage.J);
}

static std::string train_cfg_error(const dpk_optim_config* c) {
    if (!c) return "cfg is NULL";
    if (!(c->beta1 >= 0.f && c->beta1 < 1.f)) return "beta1 = " + std::to_string(c->beta1) + " is not in [0, 1)";
    if (!(c->beta2 >= 0.f && c->beta2 < 1.f)) return "beta2 = " + std::to_string(c->beta2) + " is not in [0, 1)";
    if (!(c->eps >= 0.f)) return "eps = " + std::to_string(c->eps) + " is negative or NaN";
    if (!(c->ema_mu <= 1.f)) return "ema_mu = " + std::to_string(c->ema_mu) + " is above 1 or NaN";
    return "";
}

static int train_begin(dpk_handle* h, const dpk_optim_config* cfg) {
    if (h->kind != 0)
        return fail(h, DPK_E_UNSUPPORTED, "dpk_train_begin: GCNpose handle (coords 2->3) has no diffusion objective");
    const std::string bad = train_cfg_error(cfg);
    if (!bad.empty()) return fail(h, DPK_E_INVALID, "dpk_train_begin: " + bad);
    if (!h->have_graph) return fail(h, DPK_E_STATE, "dpk_train_begin: graph (adjacency) not set");
    if (!h->have_weights) return fail(h, DPK_E_STATE, "dpk_train_begin: weights not loaded");
    if (h->train) return fail(h, DPK_E_STATE, "dpk_train_begin: training has already begun on this handle (dpk_train_end)");
    int rc = bwd_prepare(h);         // the per-op model and the transposed arena; waits for the device
    if (rc) return rc;
    HIPCHK(h, hipDeviceSynchronize());
    const Stage& s = h->stage;
    const TrainLayout lay = train_layout(s);
    GenModel* g = h->gen ? h->gen : h->bwd->own;
    const GemmArena& fa = g->arena;
    const GemmArena& ba = h->bwd->dev;
    const size_t n[4] = {lay.fwd.size(), lay.fwdp.size(), lay.bwd.size(), lay.bwdp.size()};
    if (n[0] != s.floats || n[1] != fa.hp.size() || n[2] != h->bwd->arena.floats || n[3] != ba.hp.size() ||
        n[0] > fa.dev_floats || n[1] > fa.devp_floats || n[2] > ba.dev_floats || n[3] > ba.devp_floats ||
        n[0] + n[1] + n[2] + n[3] >= 0x7fffffffu)
        return fail(h, DPK_E_STATE, "dpk_train_begin: the refresh layout and the handle's arenas disagree");
    TrainState* t = new TrainState();
    t->cfg = *cfg;
    t->beta1 = train_decimal(cfg->beta1), t->beta2 = train_decimal(cfg->beta2), t->mu = train_decimal(cfg->ema_mu);
    t->F = lay.F;
    t->entries = h->bwd->lay.e;
    const bool ams = cfg->amsgrad != 0, ema = cfg->ema_mu >= 0.f;
    const size_t F = t->F, arrays = 3 + (ams ? 1 : 0) + (ema ? 1 : 0);
    // params from the staging: each float back where the refresh reads it from (stage_load's transposes undone), and
    // A_hat as loaded
    std::vector<float> hp(F, 0.f);
    for (size_t i = 0; i < lay.fwd.size(); ++i)
        if (lay.fwd[i] >= 0) hp[lay.fwd[i]] = s.h[i];
    for (int l = 0; l < s.L; ++l)
        std::copy(s.ahat.begin() + (size_t)l * s.J * s.J, s.ahat.begin() + (size_t)(l + 1) * s.J * s.J, hp.begin() + lay.ahat[l]);
    std::vector<int> hidx;
    for (const std::vector<int32_t>* v : {&lay.fwd, &lay.fwdp, &lay.bwd, &lay.bwdp}) hidx.insert(hidx.end(), v->begin(), v->end());
    const size_t n_idx = hidx.size();
    hidx.insert(hidx.end(), lay.ahat.begin(), lay.ahat.end());
    auto alloc = [&]() -> int {
        HIPCHK(h, hipMalloc(&t->state, arrays * F * 4));
        HIPCHK(h, hipMalloc(&t->partial, dpkg::NORM_PARTS * 8 + 16));
        HIPCHK(h, hipMalloc(&t->idx, hidx.size() * 4));
        HIPCHK(h, hipMemset(t->state, 0, arrays * F * 4));
        HIPCHK(h, hipMemset(t->partial, 0, dpkg::NORM_PARTS * 8 + 16));
        HIPCHK(h, hipMemcpy(t->state, hp.data(), F * 4, hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(t->idx, hidx.data(), hidx.size() * 4, hipMemcpyHostToDevice));
        return DPK_OK;
    };
    if ((rc = alloc())) {
        train_free(t);
        return rc;
    }
    t->scal = reinterpret_cast<float*>(t->partial + dpkg::NORM_PARTS);
    t->ahat = t->idx + n_idx;
    size_t k = 0;
    t->arr[0] = t->state + F * k++, t->arr[1] = t->state + F * k++, t->arr[2] = t->state + F * k++;
    if (ams) t->arr[3] = t->state + F * k++;
    if (ema) {
        t->arr[4] = t->state + F * k++;
        if (hipMemcpy(t->arr[4], t->arr[0], F * 4, hipMemcpyDeviceToDevice) != hipSuccess) {
            train_free(t);
            return fail(h, DPK_E_HIP, "dpk_train_begin: copying the parameters into the EMA shadow");
        }
    }
    float* const dsts[4] = {fa.dev, fa.devp, ba.dev, ba.devp};
    unsigned end = 0;
    for (int a = 0; a < 4; ++a) t->dst.dst[a] = dsts[a], t->dst.end[a] = end += (unsigned)n[a];
    h->train = t;
    return DPK_OK;
}

static int train_apply(dpk_handle* h, const float* grads, float lr, float* gnorm, hipStream_t st) {
    TrainState* t = h->train;
    const int64_t k = t->step + 1;
    const TrainStep ts = train_step_consts(t->beta1, t->beta2, lr, k);
    dpkg::AdamConsts c;
    c.omb1 = (float)(1.0 - t->beta1), c.beta2 = (float)t->beta2, c.omb2 = (float)(1.0 - t->beta2);
    c.step_size = ts.step_size, c.bc2_sqrt = ts.bc2_sqrt, c.eps = t->cfg.eps;
    c.ema_a = (float)(1.0 - t->mu), c.ema_b = (float)t->mu;
    const long long F = (long long)t->F, chunk = (F + dpkg::NORM_PARTS - 1) / dpkg::NORM_PARTS;
    hipLaunchKernelGGL(dpkg::train_norm_partial, dim3(dpkg::NORM_PARTS), dim3(256), 0, st, grads, F, chunk, t->partial);
    hipLaunchKernelGGL(dpkg::train_norm_final, dim3(1), dim3(dpkg::NORM_PARTS), 0, st, t->partial, t->cfg.grad_clip, t->scal, gnorm);
    hipLaunchKernelGGL(dpkg::train_adam, dim3(gen_blocks(F / 4)), dim3(256), 0, st, grads, t->scal, t->arr[0], t->arr[1],
                       t->arr[2], t->arr[3], t->arr[4], F / 4, c);
    train_refresh_launch(h, st);
    HIPCHK(h, hipGetLastError());
    t->step = k;
    t->host_stale = true;
    return DPK_OK;
}

// The host staging from `params` through stage_load; on a persistent-sampler handle then its instance's pack and
// upload (which recomputes the schedules' timestep projections).  The per-op arenas are at these weights already (the
// refresh wrote them, to stage_load's bits), so the staging's serial stays and nothing of theirs is rebuilt.
static int train_sync(dpk_handle* h) {
    TrainState* t = h->train;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());
    if (!t->host_stale) return DPK_OK;
    std::vector<float> hp(t->F);
    HIPCHK(h, hipMemcpy(hp.data(), t->arr[0], t->F * 4, hipMemcpyDeviceToHost));
    std::vector<const char*> names;
    std::vector<const float*> ptrs;
    std::vector<int64_t> numels;
    for (const GradEntry& e : t->entries)
        names.push_back(e.name.c_str()), ptrs.push_back(hp.data() + e.offset), numels.push_back(e.numel);
    std::string err;
    if (!stage_load(h->stage, names.data(), ptrs.data(), numels.data(), (int)names.size(), err))
        return fail(h, DPK_E_STATE, "dpk_train_sync: " + err);
    if (h->w.inst) {
        h->w.inst->pack(h->stage, h->w.pk, true);
        const int rc = upload(h);
        if (rc) return rc;
    }
    t->host_stale = false;
    return DPK_OK;
}

// a sampler-path call (dpk_sample*, dpk_eps, dpk_diff_loss) on a persistent-sampler handle whose instance arenas are
// behind the trained parameters
static int train_fresh(dpk_handle* h, const char* who) {
    if (h->train && h->w.inst && h->train->host_stale)
        return fail(h, DPK_E_STATE, std::string(who) + ": the persistent sampler's weights are behind the trained parameters "
                                                       "(dpk_train_apply ran since); call dpk_train_sync first");
    return DPK_OK;
}
