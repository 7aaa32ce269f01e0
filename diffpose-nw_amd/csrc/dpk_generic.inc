// dpk_generic.inc — the GCNdiff / GCNpose forward for model shapes no sampler instance is compiled for.
//
// The persistent sampler (dpk_sampler.inc) is built for the shape every reference config uses
// (configs/human36m_*.yml:9-16: hid_dim 96, n_head 4, n_pts 17, coords [5,5] / [2,3]) and for GCNdiff at four
// other widths (dpk_kernels.hip: INSTANCES).  A config with any other hid_dim, n_head or n_pts
// (models/gcndiff.py:55-99 builds GCNdiff from any of them), and every handle made under DPK_FORCE_GENERIC=1
// or (the other widths) DPK_GEN_FUSED=0, gets a GenModel and runs here instead: the same layer sequence as plain HIP kernels over activations in HBM, one
// launch per op, fp32 throughout (the reference's order of operations per op; GEMM sums on the fp32 MFMA):
//   ChebConv   cheb_basis [X | T1 X | T2 X] -> gemm (ChebConv.py:74-88, stacked K = 3*in); every gemm on
//              the fp32 matrix cores (v_mfma_f32_16x16x4_f32)
//   LayerNorm  one wave per row, unbiased std, eps on the std (GraFormer.py:58-70)
//   MHA        gemm (QKV) -> attention (one thread per pose/head/query) -> gemm (+x) (GraFormer.py:99-140)
//   GraphNet   graph (L_g X) -> gemm relu -> graph -> gemm (+x) (GraFormer.py:162-201)
//   ResChebGC  cheb_basis -> gemm relu (+temb_proj) -> cheb_basis -> gemm relu (+x) (gcndiff.py:39-53)
//   temb       one workgroup per timestep (gcndiff.py:15-33, :103-106); DDIM update per element.
// Included by dpk_kernels.hip after the handle helpers (it uses dpk_handle, Sched, fail, HIPCHK).
// Limits: n_pts <= 32 (one 32-bit key-mask word per pose), hid_dim a multiple of n_head and, for GCNdiff,
// at least 4 (the timestep embedding divides by hid_dim / 2 - 1; dpk_create refuses 2 and 3).
// Graph capture by the caller is refused on this path (its scratch is per-stream and grows on demand);
// dpk_sample records its own K-step loop as a hipGraph instead (gen_sample).

namespace dpkg {

constexpr int GJ_MAX = 32;
enum { G_BIAS = 0, G_RELU = 1, G_RESID = 2, G_RESID_RELU = 3, G_RELU_TEMB = 4 };

// C[M][N] (row stride ldc) = epilogue(A[M][K] (lda) x W[K][N] + bias) on the fp32 matrix cores:
// v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation).  A BM x 64 output tile per
// workgroup of 4 waves, each wave 32 x 64 (BM 128), 32 x 32 (BM 64) or 16 x 32 (BM 32) = NI x NJ MFMA tiles
// (gemm_choice picks BM per shape so the tiles spread evenly over the CUs); A and W staged through LDS in
// k-blocks of 32 (row strides 36 and 80 floats: the fragment reads below hit 64 distinct banks), the
// next k-block's global loads issued before the current block's MFMAs (register double buffer).
// VEC: 16-byte loads and LDS stores (K, N, lda multiples of 4 and 16-byte aligned A / W).  MFMA
// operand layout: lane l feeds row/column (l & 15) at k = (l >> 4) of each 4-k step; the accumulator
// holds rows 4 (l >> 4) + r, column (l & 15).
// G_RELU_TEMB adds tp[(row / rpp) * tp_stride + col] after the relu (tp_stride 0: one row for all).
constexpr int GKB = 32, GA_LD = 36, GW_LD = 80;   // GBN = 64 columns: dpk_genplan.inc
template <int BM, bool VEC>
__global__ void __launch_bounds__(256) gemm(const float* __restrict__ A, int lda, const float* __restrict__ W,
                                            const float* __restrict__ bias, float* C, int ldc, int M, int N, int K,
                                            int mode, const float* __restrict__ tp, int tp_stride, int rpp) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    // waves: BM 128 -> 4 x 1 of 32 x 64 each; BM 64 -> 2 x 2 of 32 x 32; BM 32 -> 2 x 2 of 16 x 32
    constexpr int NI = BM == 32 ? 1 : 2, NJ = BM == 128 ? 4 : 2, NA = BM / 32;   // MFMA tiles per wave; A float4s
    __shared__ __attribute__((aligned(16))) float As[BM * GA_LD];
    __shared__ __attribute__((aligned(16))) float Ws[GKB * GW_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * GBN;   // row tiles on x (no 65535 limit there)
    const int wr = BM == 128 ? 32 * wave : 16 * NI * (wave >> 1), wc = BM == 128 ? 0 : 32 * (wave & 1);
    const int li = lane & 15, lk = lane >> 4;
    f32x4 acc[NI][NJ];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // this thread's share of a k-block: A BM x 32 (NA float4), W 32 x 64 (2 float4)
    f32x4 ra[NA], rw[2];
    auto load = [&](int k0) {
#pragma unroll
        for (int it = 0; it < NA; ++it) {
            const int i = tid + it * 256, r = i >> 3, kq = (i & 7) * 4, m = m0 + r, k = k0 + kq;
            if (VEC) {
                ra[it] = (m < M && k < K) ? *reinterpret_cast<const f32x4*>(A + (size_t)m * lda + k) : f32x4{0.f, 0.f, 0.f, 0.f};
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) ra[it][e] = (m < M && k + e < K) ? A[(size_t)m * lda + k + e] : 0.f;
            }
        }
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int i = tid + it * 256, kk = i >> 4, nq = (i & 15) * 4, k = k0 + kk, n = n0 + nq;
            if (VEC) {
                rw[it] = (k < K && n < N) ? *reinterpret_cast<const f32x4*>(W + (size_t)k * N + n) : f32x4{0.f, 0.f, 0.f, 0.f};
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) rw[it][e] = (k < K && n + e < N) ? W[(size_t)k * N + n + e] : 0.f;
            }
        }
    };
    load(0);
    for (int k0 = 0; k0 < K; k0 += GKB) {
#pragma unroll
        for (int it = 0; it < NA; ++it) {
            const int i = tid + it * 256;
            *reinterpret_cast<f32x4*>(&As[(i >> 3) * GA_LD + (i & 7) * 4]) = ra[it];
        }
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int i = tid + it * 256;
            *reinterpret_cast<f32x4*>(&Ws[(i >> 4) * GW_LD + (i & 15) * 4]) = rw[it];
        }
        __syncthreads();
        if (k0 + GKB < K) load(k0 + GKB);      // in flight during this block's MFMAs
#pragma unroll
        for (int ks = 0; ks < GKB; ks += 4) {
            const int kq = ks + lk;
            float a[NI], b[NJ];
#pragma unroll
            for (int i = 0; i < NI; ++i) a[i] = As[(wr + 16 * i + li) * GA_LD + kq];
#pragma unroll
            for (int j = 0; j < NJ; ++j) b[j] = Ws[kq * GW_LD + wc + 16 * j + li];
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int n = n0 + wc + 16 * j + li;
        if (n >= N) continue;
        const float bn = bias[n];
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wr + 16 * i + 4 * lk + r;
                if (m >= M) continue;
                const float v = acc[i][j][r] + bn;
                float* c = C + (size_t)m * ldc + n;
                if (mode == G_BIAS) *c = v;
                else if (mode == G_RELU) *c = fmaxf(v, 0.f);
                else if (mode == G_RESID) *c = *c + v;
                else if (mode == G_RESID_RELU) *c = *c + fmaxf(v, 0.f);
                else *c = fmaxf(v, 0.f) + tp[(size_t)(m / rpp) * tp_stride + n];
            }
    }
}

// The same product for 16-byte-aligned operands, split over k (the default where it applies): a workgroup
// owns a 16 x (16 NJ) output tile, its 4 waves take the 16-k chunks c = w, w + 4, ... each, reading A rows and
// the weights straight into MFMA fragments (no LDS staging, no barrier in the k-loop: per-lane offsets fixed
// for the whole loop, the chunk in soffset, rows past M and k past K read as 0 by the buffer range check),
// the next chunk's loads in flight during the current chunk's MFMAs.  The four partial tiles meet in LDS and
// every thread finishes float4s of the tile (one 16-byte store each).  Many short k-loops in flight instead of
// a few long ones: these GEMMs are latency-bound (M = 17 x poses rows, K, N of a few hundred),
// 10-20 % faster than gemm<BM> at the hid-128 shapes (profiles/r04_gen_gemm_probe.txt).
// Wp: the weights packed by pack_fill, [KC = ceil(K/16)][NTp][64 lanes][4]: lane l, element s of chunk c and
// column tile t = W[16c + 4 (l >> 4) + s][16t + (l & 15)] (zero outside K x N; NTp = column tiles rounded
// up to NJ).  Needs K, N, lda, ldc multiples of 4, 16-byte aligned A, C, bias, tp, and M * lda * 4 + K * 4
// below 2^31 (the range-check sentinel SK_OOR).
template <int NJ>
__global__ void __launch_bounds__(256) gemm_sk(const float* __restrict__ A, int lda, const float* __restrict__ Wp,
                                               const float* __restrict__ bias, float* C, int ldc, int M, int N, int K,
                                               int mode, const float* __restrict__ tp, int tp_stride, int rpp) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    constexpr int TN = 16 * NJ, LDR = TN + 4, Q = TN / 4;
    __shared__ __attribute__((aligned(16))) float red[4][16 * LDR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int m0 = blockIdx.x * 16, t0 = blockIdx.y * NJ;
    const int NT16 = (N + 15) >> 4, NTp = (NT16 + NJ - 1) / NJ * NJ, KC = (K + 15) >> 4;
    const __amdgpu_buffer_rsrc_t ra =
        __builtin_amdgcn_make_buffer_rsrc((void*)A, (short)0, (int)((unsigned)M * (unsigned)lda * 4u), 0x00020000);
    const __amdgpu_buffer_rsrc_t rw =
        __builtin_amdgcn_make_buffer_rsrc((void*)(Wp + (size_t)t0 * 256), (short)0, 0x7fffffff, 0x00020000);
    const int m = m0 + li;
    const unsigned voa = m < M ? ((unsigned)m * (unsigned)lda + 4u * lk) * 4u : SK_OOR;
    const unsigned vow = lane * 16u;
    const int kt = K - 4 * lk;        // this lane's k-quad of chunk c is inside K while 16 c < kt
    f32x4 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    struct Frag {
        f32x4 a, b[NJ];
    };
    auto ld = [&](int c, Frag& f) {
        f.a = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ra, 16 * c < kt ? voa : SK_OOR, c * 64, 0));
        const int so = c * NTp * 1024;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            f.b[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rw, vow + j * 1024, so, 0));
    };
    auto mma = [&](const Frag& f) {   // operands swapped: lane ends with row li, columns 16 j + 4 lk + r
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.b[j][s], f.a[s], acc[j], 0, 0, 0);
    };
    const int nq = (KC - wave + 3) >> 2;   // chunks c = wave + 4 q, q < nq
    Frag x0, x1;
    if (nq > 0) ld(wave, x0);
    int q = 0;
    for (; q + 2 <= nq; q += 2) {
        ld(wave + 4 * (q + 1), x1);
        mma(x0);
        if (q + 2 < nq) ld(wave + 4 * (q + 2), x0);
        mma(x1);
    }
    if (q < nq) mma(x0);
#pragma unroll
    for (int j = 0; j < NJ; ++j) *reinterpret_cast<f32x4*>(&red[wave][li * LDR + 16 * j + 4 * lk]) = acc[j];
    __syncthreads();
    for (int e = tid; e < 16 * Q; e += 256) {
        const int r = e / Q, cq = e % Q, row = m0 + r, n = 16 * t0 + 4 * cq;
        if (row >= M || n >= N) continue;
        f32x4 v = *reinterpret_cast<const f32x4*>(&red[0][r * LDR + 4 * cq]);
#pragma unroll
        for (int w = 1; w < 4; ++w) v += *reinterpret_cast<const f32x4*>(&red[w][r * LDR + 4 * cq]);
        v += *reinterpret_cast<const f32x4*>(bias + n);
        f32x4* cp = reinterpret_cast<f32x4*>(C + (size_t)row * ldc + n);
        if (mode == G_RELU || mode == G_RESID_RELU || mode == G_RELU_TEMB) {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = fmaxf(v[i], 0.f);
        }
        if (mode == G_RESID || mode == G_RESID_RELU) v = *cp + v;
        else if (mode == G_RELU_TEMB) v += *reinterpret_cast<const f32x4*>(tp + (size_t)(row / rpp) * tp_stride + n);
        *cp = v;
    }
}

// sum over the 64 lanes of a wave (DPP row rotations, then the lane rows by permlane)
__device__ __forceinline__ float wave_sum(float v) { return dpk::sum4rows(dpk::row_sum(v)); }

// C[M][N] = epilogue(A x W + bias) for N <= 8 (the output ChebConv, coords 5): one wave per row, W in LDS
// (dynamic K*N floats), lane l summing k = l, l+64, ..., then a wave sum per column.  The 64-column MFMA
// tile would leave 59 of 64 columns idle.
__global__ void __launch_bounds__(256) gemm_narrow(const float* __restrict__ A, int lda, const float* __restrict__ W,
                                                   const float* __restrict__ bias, float* C, int ldc, int M, int N,
                                                   int K, int mode, const float* __restrict__ tp, int tp_stride,
                                                   int rpp) {
    extern __shared__ float wsm[];
    for (int i = threadIdx.x; i < K * N; i += 256) wsm[i] = W[i];
    __syncthreads();
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float* a = A + (size_t)row * lda;
    for (int k = lane; k < K; k += 64) {
        const float v = a[k];
#pragma unroll
        for (int n = 0; n < 8; ++n)
            if (n < N) acc[n] = fmaf(v, wsm[k * N + n], acc[n]);
    }
#pragma unroll
    for (int n = 0; n < 8; ++n) {
        if (n >= N) break;
        const float tot = wave_sum(acc[n]);
        if (lane == n) {
            const float v = tot + bias[n];
            float* c = C + (size_t)row * ldc + n;
            if (mode == G_BIAS) *c = v;
            else if (mode == G_RELU) *c = fmaxf(v, 0.f);
            else if (mode == G_RESID) *c = *c + v;
            else if (mode == G_RESID_RELU) *c = *c + fmaxf(v, 0.f);
            else *c = fmaxf(v, 0.f) + tp[(size_t)(row / rpp) * tp_stride + n];
        }
    }
}

// LayerNorm of GraFormer (GraFormer.py:67-70): a*(x-mean)/(std+eps)+b, std unbiased; a wave per row, the
// row read once into registers (D <= 64 * GLN_MAX; wider rows re-read it from global memory)
constexpr int GLN_MAX = 8;
__global__ void __launch_bounds__(256) layer_norm(const float* __restrict__ X, float* __restrict__ Y, int M, int D,
                                                  const float* __restrict__ ga, const float* __restrict__ gb) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    const float* x = X + (size_t)row * D;
    float* y = Y + (size_t)row * D;
    if (D <= 64 * GLN_MAX) {
        float v[GLN_MAX];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < GLN_MAX; ++i) {
            const int c = lane + 64 * i;
            v[i] = c < D ? x[c] : 0.f;
            s += v[i];
        }
        const float mean = wave_sum(s) / (float)D;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < GLN_MAX; ++i) {
            const float d = lane + 64 * i < D ? v[i] - mean : 0.f;
            q = fmaf(d, d, q);
        }
        const float sd = sqrtf(wave_sum(q) / (float)(D - 1));
#pragma unroll
        for (int i = 0; i < GLN_MAX; ++i) {
            const int c = lane + 64 * i;
            if (c < D) y[c] = ga[c] * (v[i] - mean) / (sd + 1e-6f) + gb[c];
        }
        return;
    }
    float s = 0.f;
    for (int c = lane; c < D; c += 64) s += x[c];
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
    for (int c = lane; c < D; c += 64) {
        const float d = x[c] - mean;
        q = fmaf(d, d, q);
    }
    const float sd = sqrtf(wave_sum(q) / (float)(D - 1));
    for (int c = lane; c < D; c += 64) y[c] = ga[c] * (x[c] - mean) / (sd + 1e-6f) + gb[c];
}

// Train-mode dropout masks (DropSite, dpk_genplan.inc): counter-based, recomputed wherever they are read, never
// stored.  One Philox call gives the four words of the elements 4 g .. 4 g + 3; element indices are 64-bit.
__device__ __forceinline__ void drop_group(const DropSite& d, long long g, uint32_t w[4]) {
    w[0] = (uint32_t)g;
    w[1] = (uint32_t)((unsigned long long)g >> 32);
    w[2] = d.dom;
    w[3] = 0xD809u;
    dpk::philox(w, d.k0, d.k1);
}
__device__ __forceinline__ bool drop_keep(const DropSite& d, const uint32_t w[4], int k) {
    const uint32_t v = k == 0 ? w[0] : k == 1 ? w[1] : k == 2 ? w[2] : w[3];
    return (v >> 8) >= d.thr;
}
// d.s where element i is kept, else 0, for a thread that walks ascending i: a new call only where i leaves the group
struct DropRow {
    long long g = -1;
    uint32_t w[4];
    __device__ __forceinline__ float factor(const DropSite& d, long long i) {
        if ((i >> 2) != g) {
            g = i >> 2;
            drop_group(d, g, w);
        }
        return drop_keep(d, w, (int)(i & 3)) ? d.s : 0.f;
    }
};

// o[i] = drop(x[i]) (ADD: res[i] + drop(x[i])) for the n elements from global element `base` of the site on: a kept
// value is x d.s, a dropped one 0.  x may be o (in place).  One thread per group of four global elements, the ends
// of the range clipped; vec (base a multiple of 4, 16-byte aligned arrays): whole groups as 16-byte accesses.
template <bool ADD>
__global__ void __launch_bounds__(256) drop_apply(const float* res, const float* x, float* o, long long n,
                                                  long long base, DropSite d, int vec) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const long long g = (base >> 2) + (long long)blockIdx.x * 256 + threadIdx.x;
    const long long lo = max(4 * g, base), hi = min(4 * g + 4, base + n);
    if (lo >= hi) return;
    uint32_t w[4];
    drop_group(d, g, w);
    if (vec && hi - lo == 4) {
        const long long e = lo - base;
        f32x4 v = *reinterpret_cast<const f32x4*>(x + e);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = drop_keep(d, w, k) ? v[k] * d.s : 0.f;
        if constexpr (ADD) v = *reinterpret_cast<const f32x4*>(res + e) + v;
        *reinterpret_cast<f32x4*>(o + e) = v;
        return;
    }
    for (long long i = lo; i < hi; ++i) {
        const float v = drop_keep(d, w, (int)(i & 3)) ? x[i - base] * d.s : 0.f;
        if constexpr (ADD) o[i - base] = res[i - base] + v;
        else o[i - base] = v;
    }
}
// keep[i - first] = 1 or 0 for the elements first .. first + n - 1 (dpk_dropout_mask)
__global__ void __launch_bounds__(256) drop_mask_bytes(unsigned char* __restrict__ keep, long long first, long long n,
                                                       DropSite d) {
    const long long g = (first >> 2) + (long long)blockIdx.x * 256 + threadIdx.x;
    const long long lo = max(4 * g, first), hi = min(4 * g + 4, first + n);
    if (lo >= hi) return;
    uint32_t w[4];
    drop_group(d, g, w);
    for (long long i = lo; i < hi; ++i) keep[i - first] = drop_keep(d, w, (int)(i & 3)) ? 1 : 0;
}

// The draws of one training step for poses pose0 .. pose0 + n - 1 of a batch of `batch` poses (dpk_train_draws), each a
// function of its seed and the global index alone.  Work item i < ne = n * pe is element i of e (global element
// pose0 * pe + i, the draw qsample_at takes for a NULL noise at pose0 = 0); item ne + k is the timestep of pose
// pose0 + k: the reference's antithetic pair cat([r, T - 1 - r])[:batch] with h = batch / 2 + 1 draws r, r the top 32
// bits of counter_word(t_seed, q) scaled to 0 .. T - 1 in integers (T <= 2^24: the product fits 64 bits, the float is
// exact).  ne or n is 0 for an output the caller does not ask for.  Plain 4-byte stores: the caller's arrays are 4-byte
// aligned and no more.
__global__ void __launch_bounds__(256) train_draws(float* __restrict__ e, float* __restrict__ t, long long ne, long long n,
                                                   long long e0, long long pose0, long long batch, int T,
                                                   unsigned long long e_seed, unsigned long long t_seed) {
    const long long stride = (long long)gridDim.x * 256;
    const long long end = ne + n;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < end; i += stride) {
        if (i < ne) {
            e[i] = dpk::normal_noise(e_seed, -1, e0 + i);
            continue;
        }
        const long long p = pose0 + (i - ne), h = batch / 2 + 1;
        const bool first = p < h;
        const unsigned long long w = dpk_counter::counter_word(t_seed, (unsigned long long)(first ? p : p - h));
        const long long r = (long long)(((w >> 32) * (unsigned long long)T) >> 32);
        t[i - ne] = (float)(first ? r : (long long)T - 1 - r);
    }
}

// Multi-head attention core (GraFormer.py:116-140): `ppb` poses per workgroup, their QKV rows
// [q | k | v] (J x 3D floats each) staged in LDS with coalesced loads (STAGE; dynamic LDS ppb * J * RW
// floats, used when that fits 64 KB), then one thread per (pose, head, query): scores / sqrt(dk), masked
// keys -1e9, softmax, P.V, every sum in the reference's order per query (d ascending, then keys
// ascending).  VEC (dk and D multiples of 4 and 8, `out` 16-byte aligned): 16-byte LDS reads and stores, LDS row stride
// RW = 3D + 4 (RW / 4 odd: the 16 lanes of a head reading rows q * RW hit disjoint bank quads);
// otherwise RW = 3D + 1 (odd: distinct banks for scalar reads).
// TRAIN (attention_train; the inference kernel is the body without it): dropout on the normalised probabilities
// before P.V, element ((pose0 + p) H + h) J J + q J + j of site `drop` (drop_factor).
template <bool STAGE, bool VEC, bool TRAIN>
__device__ __forceinline__ void attention_body(const float* __restrict__ qkv, float* __restrict__ out, int N, int J,
                                               int D, int H, unsigned mask, const unsigned* __restrict__ pmask,
                                               int ppb, const DropSite& drop, long long pose0) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) float lds_rows[];
    const int p0 = blockIdx.x * ppb, np = min(ppb, N - p0);
    const int RS = 3 * D;                                      // row stride in global memory
    const int RW = STAGE ? (VEC ? RS + 4 : RS + 1) : RS;       // in LDS
    const float* src = qkv + (size_t)p0 * J * RS;
    if (STAGE) {
        if (VEC && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {      // RS, RW multiples of 4: float4 rows
            const int RS4 = RS / 4, RW4 = RW / 4;
            for (int i = threadIdx.x; i < np * J * RS4; i += 256) {
                const int r = i / RS4;
                reinterpret_cast<f32x4*>(lds_rows)[r * RW4 + (i - r * RS4)] = reinterpret_cast<const f32x4*>(src)[i];
            }
        } else {
            for (int i = threadIdx.x; i < np * J * RS; i += 256) {
                const int r = i / RS;
                lds_rows[r * RW + (i - r * RS)] = src[i];
            }
        }
        __syncthreads();
    }
    const int dk = D / H;
    const float sq = sqrtf((float)dk);
    for (int t = threadIdx.x; t < np * H * J; t += 256) {
        const int pl = t / (H * J), hq = t - pl * (H * J), h = hq / J, q = hq - h * J;
        const int p = p0 + pl;
        const unsigned m = pmask ? pmask[p] : mask;
        const float* rows = (STAGE ? lds_rows : src) + (size_t)pl * J * RW;
        float sc[GJ_MAX];
        float mx = -INFINITY;
        for (int j = 0; j < J; ++j) {
            float s = 0.f;
            if constexpr (VEC) {
                const f32x4* qr = reinterpret_cast<const f32x4*>(rows + q * RW + h * dk);
                const f32x4* kr = reinterpret_cast<const f32x4*>(rows + j * RW + D + h * dk);
                for (int d4 = 0; d4 < dk / 4; ++d4) {
                    const f32x4 a = qr[d4], b = kr[d4];
                    s = fmaf(a[0], b[0], s);
                    s = fmaf(a[1], b[1], s);
                    s = fmaf(a[2], b[2], s);
                    s = fmaf(a[3], b[3], s);
                }
            } else {
                const float* qr = rows + q * RW + h * dk;
                const float* kr = rows + j * RW + D + h * dk;
                for (int d = 0; d < dk; ++d) s = fmaf(qr[d], kr[d], s);
            }
            s = ((m >> j) & 1u) ? s / sq : -1e9f;
            sc[j] = s;
            mx = fmaxf(mx, s);
        }
        float sum = 0.f;
        for (int j = 0; j < J; ++j) {
            sc[j] = expf(sc[j] - mx);
            sum += sc[j];
        }
        for (int j = 0; j < J; ++j) sc[j] = sc[j] / sum;
        if constexpr (TRAIN) {
            const long long i0 = (((pose0 + p) * H + h) * J + q) * J;
            DropRow row;
            for (int j = 0; j < J; ++j) sc[j] = sc[j] * row.factor(drop, i0 + j);
        }
        float* o = out + ((size_t)p * J + q) * D + h * dk;
        if constexpr (VEC) {
            for (int d4 = 0; d4 < dk / 4; ++d4) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                for (int j = 0; j < J; ++j) {
                    const f32x4 v = reinterpret_cast<const f32x4*>(rows + j * RW + 2 * D + h * dk)[d4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[e] = fmaf(sc[j], v[e], acc[e]);
                }
                reinterpret_cast<f32x4*>(o)[d4] = acc;
            }
        } else {
            for (int d = 0; d < dk; ++d) {
                float acc = 0.f;
                for (int j = 0; j < J; ++j) acc = fmaf(sc[j], rows[j * RW + 2 * D + h * dk + d], acc);
                o[d] = acc;
            }
        }
    }
}
template <bool STAGE, bool VEC>
__global__ void __launch_bounds__(256) attention(const float* __restrict__ qkv, float* __restrict__ out, int N, int J,
                                                 int D, int H, unsigned mask, const unsigned* __restrict__ pmask,
                                                 int ppb) {
    attention_body<STAGE, VEC, false>(qkv, out, N, J, D, H, mask, pmask, ppb, DropSite{}, 0);
}
template <bool STAGE, bool VEC>
__global__ void __launch_bounds__(256) attention_train(const float* __restrict__ qkv, float* __restrict__ out, int N,
                                                       int J, int D, int H, unsigned mask,
                                                       const unsigned* __restrict__ pmask, int ppb, DropSite drop,
                                                       long long pose0) {
    attention_body<STAGE, VEC, true>(qkv, out, N, J, D, H, mask, pmask, ppb, drop, pose0);
}

// Y[p][j][c] = sum_i Lm[j][i] X[p][i][c] (row strides ldx, ldy).  STAGE: one workgroup per pose, X_p and
// Lm staged in LDS (dynamic, J*C + J*J floats), one thread per (j, 4 channels) when C, ldx, ldy are
// multiples of 4 and Y is 16-byte aligned (16-byte LDS reads and global stores), else per (j, c); without STAGE one thread per
// output straight from global memory (poses too wide for 64 KB of LDS).  Sums over i ascending.
template <bool STAGE>
__global__ void __launch_bounds__(256) graph(const float* __restrict__ Lm, const float* __restrict__ X, int ldx,
                                             float* __restrict__ Y, int ldy, int N, int J, int C) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    if (STAGE) {
        extern __shared__ __attribute__((aligned(16))) float gsm[];
        float* xs = gsm;
        float* ls = gsm + J * C;
        const int p = blockIdx.x;
        const float* xp = X + (size_t)p * J * ldx;
        if (ldx == C && (C & 3) == 0 && (reinterpret_cast<uintptr_t>(xp) & 15) == 0) {   // dense rows: one copy
            for (int i = threadIdx.x; i < J * C / 4; i += 256)
                reinterpret_cast<f32x4*>(xs)[i] = reinterpret_cast<const f32x4*>(xp)[i];
        } else {
            for (int i = threadIdx.x; i < J * C; i += 256) {
                const int r = i / C;
                xs[i] = xp[(size_t)r * ldx + (i - r * C)];
            }
        }
        for (int i = threadIdx.x; i < J * J; i += 256) ls[i] = Lm[i];
        __syncthreads();
        // 16-byte stores to Y: As and Gs sit after the Chebyshev operand's 3 max(hid, coords_in) floats a
        // row, which is no multiple of 4 when the input is wider than hid_dim (coords 9 on hid 8)
        if ((C & 3) == 0 && (ldy & 3) == 0 && (reinterpret_cast<uintptr_t>(Y) & 15) == 0) {
            const int C4 = C / 4;
            for (int o = threadIdx.x; o < J * C4; o += 256) {
                const int j = o / C4, c4 = o - j * C4;
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                for (int i = 0; i < J; ++i) {
                    const float l = ls[j * J + i];
                    const f32x4 v = reinterpret_cast<const f32x4*>(xs + i * C)[c4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[e] = fmaf(l, v[e], acc[e]);
                }
                reinterpret_cast<f32x4*>(Y + ((size_t)p * J + j) * ldy)[c4] = acc;
            }
        } else {
            for (int o = threadIdx.x; o < J * C; o += 256) {
                const int j = o / C, c = o - j * C;
                float acc = 0.f;
                for (int i = 0; i < J; ++i) acc = fmaf(ls[j * J + i], xs[i * C + c], acc);
                Y[((size_t)p * J + j) * ldy + c] = acc;
            }
        }
        return;
    }
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int c = (int)(t % C);
    const long long pj = t / C;
    if (pj >= (long long)N * J) return;
    const int j = (int)(pj % J);
    const long long p = pj / J;
    const float* xp = X + (size_t)p * J * ldx + c;
    float acc = 0.f;
    for (int i = 0; i < J; ++i) acc = fmaf(Lm[j * J + i], xp[(size_t)i * ldx], acc);
    Y[(size_t)pj * ldy + c] = acc;
}

// Chebyshev operand Z[p][j] = [X | T1 X | T2 X] (3C floats per row) of X[p][j][C]; STAGE and the 4-channel
// form as graph (LDS J*C + 2*J*J floats)
template <bool STAGE>
__global__ void __launch_bounds__(256) cheb_basis(const float* __restrict__ T1, const float* __restrict__ T2,
                                                  const float* __restrict__ X, float* __restrict__ Z, int N, int J,
                                                  int C) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    if (STAGE) {
        extern __shared__ __attribute__((aligned(16))) float csm[];
        float* xs = csm;
        float* t1 = csm + J * C;
        float* t2 = t1 + J * J;
        const int p = blockIdx.x;
        const float* xp = X + (size_t)p * J * C;
        if ((C & 3) == 0 && ((reinterpret_cast<uintptr_t>(xp) | (reinterpret_cast<uintptr_t>(xs))) & 15) == 0) {
            for (int i = threadIdx.x; i < J * C / 4; i += 256)
                reinterpret_cast<f32x4*>(xs)[i] = reinterpret_cast<const f32x4*>(xp)[i];
        } else {
            for (int i = threadIdx.x; i < J * C; i += 256) xs[i] = xp[i];
        }
        for (int i = threadIdx.x; i < J * J; i += 256) {
            t1[i] = T1[i];
            t2[i] = T2[i];
        }
        __syncthreads();
        // 16-byte stores to Z: its rows are 3C floats, so the base decides (Zs sits after 2 M D floats of
        // scratch: 8-byte aligned only with hid_dim and the row count odd)
        if ((C & 3) == 0 && (reinterpret_cast<uintptr_t>(Z) & 15) == 0) {
            const int C4 = C / 4;
            for (int o = threadIdx.x; o < J * C4; o += 256) {
                const int j = o / C4, c4 = o - j * C4;
                f32x4 a1 = {0.f, 0.f, 0.f, 0.f}, a2 = {0.f, 0.f, 0.f, 0.f};
                for (int i = 0; i < J; ++i) {
                    const float u1 = t1[j * J + i], u2 = t2[j * J + i];
                    const f32x4 v = reinterpret_cast<const f32x4*>(xs + i * C)[c4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        a1[e] = fmaf(u1, v[e], a1[e]);
                        a2[e] = fmaf(u2, v[e], a2[e]);
                    }
                }
                f32x4* z = reinterpret_cast<f32x4*>(Z + ((size_t)p * J + j) * 3 * C);
                z[c4] = reinterpret_cast<const f32x4*>(xs + j * C)[c4];
                z[C4 + c4] = a1;
                z[2 * C4 + c4] = a2;
            }
        } else {
            for (int o = threadIdx.x; o < J * C; o += 256) {
                const int j = o / C, c = o - j * C;
                float a1 = 0.f, a2 = 0.f;
                for (int i = 0; i < J; ++i) {
                    const float v = xs[i * C + c];
                    a1 = fmaf(t1[j * J + i], v, a1);
                    a2 = fmaf(t2[j * J + i], v, a2);
                }
                float* z = Z + ((size_t)p * J + j) * 3 * C + c;
                z[0] = xs[o];
                z[C] = a1;
                z[2 * C] = a2;
            }
        }
        return;
    }
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int c = (int)(t % C);
    const long long pj = t / C;
    if (pj >= (long long)N * J) return;
    const int j = (int)(pj % J);
    const long long p = pj / J;
    const float* xp = X + (size_t)p * J * C + c;
    float a1 = 0.f, a2 = 0.f;
    for (int i = 0; i < J; ++i) {
        const float v = xp[(size_t)i * C];
        a1 = fmaf(T1[j * J + i], v, a1);
        a2 = fmaf(T2[j * J + i], v, a2);
    }
    float* z = Z + (size_t)pj * 3 * C + c;
    z[0] = xp[(size_t)j * C];
    z[C] = a1;
    z[2 * C] = a2;
}

// temb_proj_l(swish(dense1(swish(dense0(emb(t)))))) for every layer l (gcndiff.py:15-33, :46):
// one workgroup per t value; W0 [D][E], W1 [E][E], WP [L][E][D] (k-major), dynamic LDS D + 2E floats.
// STASH (the training forward): what the MLP's backward reads is kept per t value, emb [D], the pre-activations
// u0, u1 and the activations h0, h1 [E]; tproj is bitwise temb<false>'s.
struct TembStash {
    float *emb, *u0, *h0, *u1, *h1;
};
template <bool STASH>
__global__ void __launch_bounds__(256) temb(const float* __restrict__ W0, const float* __restrict__ B0,
                                            const float* __restrict__ W1, const float* __restrict__ B1,
                                            const float* __restrict__ WP, const float* __restrict__ BP,
                                            const float* __restrict__ tvals, int tstride, int D, int E, int L,
                                            float neg_scale, float* __restrict__ tproj, TembStash keep) {
    extern __shared__ float tsm[];
    float* emb = tsm;
    float* h0 = tsm + D;
    float* h1 = h0 + E;
    const float t = tvals[(size_t)blockIdx.x * tstride];
    const int half = D / 2;
    for (int i = threadIdx.x; i < D; i += 256) {
        if (i < 2 * half) {
            const int k = i < half ? i : i - half;
            const float arg = t * expf((float)k * neg_scale);
            emb[i] = i < half ? sinf(arg) : cosf(arg);
        } else {
            emb[i] = 0.f;   // odd hid_dim: F.pad (gcndiff.py:31-32)
        }
        if constexpr (STASH) keep.emb[(size_t)blockIdx.x * D + i] = emb[i];
    }
    __syncthreads();
    for (int o = threadIdx.x; o < E; o += 256) {
        float acc = 0.f;
        for (int k = 0; k < D; ++k) acc = fmaf(emb[k], W0[(size_t)k * E + o], acc);
        const float v = acc + B0[o];
        h0[o] = v * (1.0f / (1.0f + expf(-v)));
        if constexpr (STASH) keep.u0[(size_t)blockIdx.x * E + o] = v, keep.h0[(size_t)blockIdx.x * E + o] = h0[o];
    }
    __syncthreads();
    for (int o = threadIdx.x; o < E; o += 256) {
        float acc = 0.f;
        for (int k = 0; k < E; ++k) acc = fmaf(h0[k], W1[(size_t)k * E + o], acc);
        const float v = acc + B1[o];
        h1[o] = v * (1.0f / (1.0f + expf(-v)));
        if constexpr (STASH) keep.u1[(size_t)blockIdx.x * E + o] = v, keep.h1[(size_t)blockIdx.x * E + o] = h1[o];
    }
    __syncthreads();
    for (int o = threadIdx.x; o < L * D; o += 256) {
        const int l = o / D, c = o - l * D;
        const float* wp = WP + (size_t)l * E * D;
        float acc = 0.f;
        for (int k = 0; k < E; ++k) acc = fmaf(h1[k], wp[(size_t)k * D + c], acc);
        tproj[(size_t)blockIdx.x * L * D + o] = acc + BP[o];
    }
}

// DDIM update (common/utils_diff.py:59-65): z from the caller's draws of this step, or the fused
// kernel's noise keys (seed, step, element)
__global__ void __launch_bounds__(256) ddim(const float* xt, const float* __restrict__ et, float* xn,
                                            float* __restrict__ x0o, long long n, const float* __restrict__ cf,
                                            int step, float eta, unsigned long long seed,
                                            const float* __restrict__ noise) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float z = noise ? noise[i] : (eta != 0.f ? dpk::normal_noise(seed, step, i) : 0.f);
    float x0, x1;
    dpk::ddim_elem(cf, xt[i], et[i], z, x0, x1);
    xn[i] = x1;
    if (x0o) x0o[i] = x0;
}

// Hypothesis start x_T = x*sa + (e*scale)*sb (runners/diffpose_frame.py:359-363) for n = N * pe elements, the
// fused kernel's arithmetic and draws (dpk::qsample_at); xT2 (null or a second copy, the trajectory's xs[0])
__global__ void __launch_bounds__(256) qsample(const float* x, float* xT, float* xT2, long long n, int pe, float sa, float sb,
                                               const float* __restrict__ scale, int rows,
                                               const float* __restrict__ noise, unsigned long long seed) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int pose = (int)(i / pe);
    const float v = dpk::qsample_at(x[i], pose, (int)(i - (long long)pose * pe), pe, sa, sb, scale, rows, noise, seed);
    xT[i] = v;
    if (xT2) xT2[i] = v;
}

// ... at one timestep per pose (dpk_diff_loss; runners/diffpose_frame.py:216-222): pose p's roots are row t[p] of
// the schedule's table qtab [nt][2] = (sqrtf(abar[t+1]), sqrtf(1 - abar[t+1])), the index clamped to the table (a NaN
// compares false both times and reads row 0)
__global__ void __launch_bounds__(256) qsample_t(const float* __restrict__ x, float* __restrict__ xT, long long n,
                                                 int pe, const float* __restrict__ t, const float* __restrict__ qtab,
                                                 int nt, const float* __restrict__ scale, int rows,
                                                 const float* __restrict__ noise, unsigned long long seed) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int pose = (int)(i / pe);
    const float tf = t[pose];
    const int ti = tf >= 0.f ? (tf < (float)(nt - 1) ? (int)tf : nt - 1) : 0;
    xT[i] = dpk::qsample_at(x[i], pose, (int)(i - (long long)pose * pe), pe, qtab[2 * ti], qtab[2 * ti + 1], scale, rows,
                            noise, seed);
}

// The denoising objective per pose (runners/diffpose_frame.py:226, before the batch mean): one thread per pose adds
// (target - eps)^2 over the pose's pe elements in ascending order into one fp32 accumulator; target = e * scale is
// the product qsample_at noised x with (the same draws, the same scale row)
__global__ void __launch_bounds__(256) diff_loss(const float* __restrict__ eps, int N, int pe,
                                                 const float* __restrict__ scale, int rows,
                                                 const float* __restrict__ noise, unsigned long long seed,
                                                 float* __restrict__ loss) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
    const float* sc = scale ? scale + (size_t)(p % rows) * pe : nullptr;
    float acc = 0.f;
    for (int r = 0; r < pe; ++r) {
        const long long g = (long long)p * pe + r;
        const float e = noise ? noise[g] : dpk::normal_noise(seed, -1, g);
        const float target = e * (sc ? sc[r] : 1.0f);
        const float d = target - eps[g];
        acc = acc + d * d;
    }
    loss[p] = acc;
}

// GCNpose's uvxyz assembly (runners/diffpose_frame.py:337-342) and xyz output, as dpk_pose's
__global__ void __launch_bounds__(256) pose_out(const float* __restrict__ x2d, const float* __restrict__ y, int N,
                                                int J, int cin, int cout, float* __restrict__ xyz,
                                                float* __restrict__ uvxyz, int Hn, int root_mode) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int cw = cin + cout;
    const int c = (int)(t % cw);
    const long long pj = t / cw;
    if (pj >= (long long)N * J) return;
    const int j = (int)(pj % J);
    const long long p = pj / J;
    float v;
    if (c < cin) {
        v = x2d[(size_t)pj * cin + c];
    } else {
        const float raw = y[(size_t)pj * cout + (c - cin)];
        if (xyz) xyz[(size_t)pj * cout + (c - cin)] = raw;
        if (root_mode == 0) v = j == 0 ? 0.f : raw;
        else if (root_mode == 1) v = raw - y[(size_t)p * J * cout + (c - cin)];
        else v = raw;
    }
    if (uvxyz)
        for (int hh = 0; hh < Hn; ++hh) uvxyz[((size_t)hh * N + p) * J * cw + (size_t)j * cw + c] = v;
}

}  // namespace dpkg

// ---------------------------------------------------------------------------------------
// Host side of the generic path
// The generic path's K-step loop recorded as one hipGraph (north_star: the K-step loop as a hipGraph;
// on this path a step is 13 launches per layer plus 6): recorded on the handle's own stream, replayed
// with one hipGraphLaunch on the caller's stream.  It reads only handle-owned memory (the caller
// stream's scratch with the state x_t inside it, the schedule, the weights) plus the per-pose mask
// array by address, so the key is everything baked into it.
struct GenGraphKey {
    hipStream_t st;
    const float* scratch;
    uint64_t sched_serial;
    int N;
    unsigned mask;
    const unsigned* pmask;
    uint64_t seed;
    bool operator==(const GenGraphKey& o) const {
        return st == o.st && scratch == o.scratch && sched_serial == o.sched_serial && N == o.N && mask == o.mask &&
               pmask == o.pmask && seed == o.seed;
    }
};
struct GenGraph {
    GenGraphKey key;
    hipGraphExec_t exec = nullptr;
    uint64_t last_use = 0;
};
// A weight arena on the device with the gemm_sk copies of its GEMM blocks (dpk_genplan.inc: pack_plan, pack_fill):
// the forward's over the staging, the backward's over the transposed arena.  Grow-only: a new upload of the same
// shape reuses the allocations.
struct GemmArena {
    float* dev = nullptr;      // device arena
    float* devp = nullptr;     // device packed arena
    size_t dev_floats = 0, devp_floats = 0;   // allocated
    std::vector<GenPack> packs;
    std::vector<float> hp;     // host staging of the packed arena
    static int put(dpk_handle* h, float*& d, size_t& cap, const float* src, size_t n) {
        if (cap < n) {
            if (d) HIPCHK(h, hipFree(d));
            d = nullptr, cap = 0;
            HIPCHK(h, hipMalloc(&d, n * 4));
            cap = n;
        }
        if (n) HIPCHK(h, hipMemcpy(d, src, n * 4, hipMemcpyHostToDevice));
        return DPK_OK;
    }
    // the caller has drained the device: launches in flight may read the arena
    int upload(dpk_handle* h, const float* host, size_t floats, const std::vector<PackBlock>& blocks) {
        const size_t pf = pack_plan(blocks, packs);
        pack_fill(packs, host, pf, hp);
        const int rc = put(h, dev, dev_floats, host, floats);
        return rc ? rc : put(h, devp, devp_floats, hp.data(), hp.size());
    }
    void free() {
        if (dev) (void)hipFree(dev);
        if (devp) (void)hipFree(devp);
        dev = devp = nullptr, dev_floats = devp_floats = 0;
    }
};
struct GenModel {
    const Stage& s;            // the handle's host staging of the weights and the graph; arena.dev is its device copy
    GemmArena arena;
    std::vector<GenGraph> graphs;   // recorded K-step loops (at most GEN_GRAPHS, least recently used out)
    uint64_t use_clock = 0;
    unsigned forms = 0;        // dpkg::GenForm bits of the kernel forms launched (or recorded) since the last read
};
constexpr size_t GEN_GRAPHS = 8;

static void gen_drop_graphs(GenModel* g, const float* scratch) {   // scratch null: all (device drained)
    std::vector<GenGraph> keep;
    for (auto& gg : g->graphs) {
        if (!scratch || gg.key.scratch == scratch) (void)hipGraphExecDestroy(gg.exec);
        else keep.push_back(gg);
    }
    g->graphs.swap(keep);
}
// the handle's scratch pool is about to replace the buffer `old` of a stream it has synced (null: the stream
// had none yet): the loops recorded over it go first
static void gen_scratch_replaced(void* g, const float* old) { gen_drop_graphs(static_cast<GenModel*>(g), old); }

static GenModel* gen_new(const Stage& s) { return new GenModel{s}; }

static int gen_graph_count(const GenModel* g) { return g ? (int)g->graphs.size() : 0; }

// the forms launched since the last call (0 without a GenModel), cleared
static unsigned gen_take_forms(GenModel* g) {
    if (!g) return 0;
    const unsigned f = g->forms;
    g->forms = 0;
    return f;
}

static void gen_free(GenModel* g) {
    if (!g) return;
    (void)hipDeviceSynchronize();
    gen_drop_graphs(g, nullptr);
    g->arena.free();
    delete g;
}

static int gen_upload(dpk_handle* h, GenModel* g) {
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());   // launches in flight may read the arena
    return g->arena.upload(h, g->s.h.data(), g->s.floats, gen_pack_blocks(g->s));
}

// n floats of scratch for a call off the shipped shape (call_scratch; per-op handles, and the timestep
// projections of the other widths' instances), a captured call's refusals in floats.  The pool costs one more
// scratch-sized buffer per such handle, its spare.
static int gen_scratch(dpk_handle* h, hipStream_t st, bool cap, size_t n, float** out, const char* who) {
    ScratchBuf buf;
    ScratchStatus why;
    const int rc = call_scratch(h, st, cap, n, who, buf, why);
    *out = buf.p;
    if (why == SCRATCH_NO_SPARE)
        return fail(h, rc, std::string(who) + ": a captured generic-shape call needs " + std::to_string(n) +
                               " floats of scratch and the spare holds " + std::to_string(buf.cap) +
                               "; make the same call once uncaptured before the capture");
    if (why == SCRATCH_SHARED_TOO_SMALL)
        return fail(h, rc, std::string(who) + ": the captured calls of one stream share the scratch of the capture's "
                                              "first generic call; warm up with the largest call before capturing");
    return rc;
}

// The ops of one call over N poses, as launches on st: each asks dpk_genplan.inc which form runs, at which grid and
// LDS size, notes the form's bit in `forms` and launches it.  Built once per call (the A/B switches DPK_GEN_GEMM and
// DPK_GEN_BM are read here, so they hold for every GEMM of the call, the backward's included); the inference
// forward, the training forward and the backward's dX GEMMs all go through it.
struct GenOps {
    const Stage& s;
    const float* W;            // the forward's device arena
    hipStream_t st;
    int N, n_cu;
    unsigned mask;
    const unsigned* pmask;
    unsigned& forms;           // dpkg::GenForm bits
    GenSwitches sw;
    GenOps(const GenModel* g, hipStream_t st_, int N_, unsigned mask_, const unsigned* pmask_, int n_cu_, unsigned& forms_)
        : s(g->s), W(g->arena.dev), st(st_), N(N_), n_cu(n_cu_), mask(mask_), pmask(pmask_), forms(forms_),
          sw(gen_switches(getenv("DPK_GEN_GEMM"), getenv("DPK_GEN_BM"))) {}
    int M() const { return N * s.J; }

    // c [rows][Nn] (row stride ldc) = epilogue(a [rows][K] x the block at offset w of `ar` + bias); tpl, tps:
    // G_RELU_TEMB's rows.  packed false: the block has no gemm_sk copy of its own (the timestep MLP's stacked
    // projections [L D][E], whose L parts have)
    void gemm(const GemmArena& ar, const float* a, int rows, int K, size_t w, const float* bias, float* c, int ldc, int Nn,
              int mode, const float* tpl = nullptr, int tps = 0, bool packed = true) const {
        const float* Wb = ar.dev + w;
        const GenPack* pk = packed ? find_pack(ar.packs, w, K, Nn) : nullptr;
        const auto at = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
        const GemmChoice g =
            gemm_choice(rows, K, Nn, ldc, at(a), at(Wb), at(bias), at(c), at(tpl), tps, pk ? pk->NJ : 0, n_cu, sw);
        forms |= g.form;
        const dim3 grid(g.gx, g.gy);
#define DPKG_GEMM(KERNEL_, W_) \
    hipLaunchKernelGGL(KERNEL_, grid, dim3(256), g.lds, st, a, K, W_, bias, c, ldc, rows, Nn, K, mode, tpl, tps, s.J)
        if (g.kind == GEMM_NARROW) DPKG_GEMM(dpkg::gemm_narrow, Wb);
        else if (g.kind == GEMM_SK4) DPKG_GEMM(dpkg::gemm_sk<4>, ar.devp + pk->off);
        else if (g.kind == GEMM_SK2) DPKG_GEMM(dpkg::gemm_sk<2>, ar.devp + pk->off);
        else if (g.bm == 128 && g.vec) DPKG_GEMM((dpkg::gemm<128, true>), Wb);
        else if (g.bm == 128) DPKG_GEMM((dpkg::gemm<128, false>), Wb);
        else if (g.bm == 64 && g.vec) DPKG_GEMM((dpkg::gemm<64, true>), Wb);
        else if (g.bm == 64) DPKG_GEMM((dpkg::gemm<64, false>), Wb);
        else if (g.vec) DPKG_GEMM((dpkg::gemm<32, true>), Wb);
        else DPKG_GEMM((dpkg::gemm<32, false>), Wb);
#undef DPKG_GEMM
    }
    // Z = [X | T1 X | T2 X] of xin [N][J][C]
    void cheb(const float* xin, int C, float* Z) const {
        const StageChoice c = cheb_choice(N, s.J, C);
        forms |= c.stage ? dpkg::F_CHEB_T : dpkg::F_CHEB_F;
        auto* kernel = c.stage ? dpkg::cheb_basis<true> : dpkg::cheb_basis<false>;
        hipLaunchKernelGGL(kernel, dim3(c.blocks), dim3(256), c.lds, st, W + s.t1, W + s.t2, xin, Z, N, s.J, C);
    }
    // y = Lm xin with Lm a layer's Laplacian, or (bwd given: the backward, its form noted there) its transpose
    void graph(const float* Lm, const float* xin, int C, float* y, unsigned* bwd = nullptr) const {
        const StageChoice c = graph_choice(N, s.J, C);
        if (bwd) *bwd |= c.stage ? dpkg::B_GRAPH_T_STAGED : dpkg::B_GRAPH_T_GLOBAL;
        else forms |= c.stage ? dpkg::F_GRAPH_T : dpkg::F_GRAPH_F;
        auto* kernel = c.stage ? dpkg::graph<true> : dpkg::graph<false>;
        hipLaunchKernelGGL(kernel, dim3(c.blocks), dim3(256), c.lds, st, Lm, xin, C, y, C, N, s.J, C);
    }
    // (the vector form stores 16 bytes at a time to out: see graph on when gen_forward's As is not 16-byte aligned)
    void attention(const float* qkv, float* out) const {
        const AttnChoice a = attention_choice(N, s.J, s.D, s.H, reinterpret_cast<uintptr_t>(out));
        forms |= a.form;
        auto* kernel = !a.stage ? dpkg::attention<false, false> : a.vec ? dpkg::attention<true, true> : dpkg::attention<true, false>;
        hipLaunchKernelGGL(kernel, dim3(a.blocks), dim3(256), a.lds, st, qkv, out, N, s.J, s.D, s.H, mask, pmask, a.ppb);
    }
    // the same choice with dropout on the probabilities (the train-mode gradient call)
    void attention_train(const float* qkv, float* out, const dpkg::DropSite& d, long long pose0) const {
        const AttnChoice a = attention_choice(N, s.J, s.D, s.H, reinterpret_cast<uintptr_t>(out));
        forms |= a.form;
        auto* kernel = !a.stage ? dpkg::attention_train<false, false>
                       : a.vec  ? dpkg::attention_train<true, true>
                                : dpkg::attention_train<true, false>;
        hipLaunchKernelGGL(kernel, dim3(a.blocks), dim3(256), a.lds, st, qkv, out, N, s.J, s.D, s.H, mask, pmask, a.ppb, d,
                           pose0);
    }
    // o = drop(x), or res + drop(x) with res given, over n floats from global element `base` of the site
    void drop(const float* res, const float* x, float* o, long long n, long long base, const dpkg::DropSite& d) const {
        const auto al = [](const void* p) { return gen_al16(reinterpret_cast<uintptr_t>(p)); };
        const int vec = (base & 3) == 0 && al(x) && al(o) && (!res || al(res));
        const dim3 grid(gen_blocks(((base + n + 3) >> 2) - (base >> 2)));
        if (res) hipLaunchKernelGGL(dpkg::drop_apply<true>, grid, dim3(256), 0, st, res, x, o, n, base, d, vec);
        else hipLaunchKernelGGL(dpkg::drop_apply<false>, grid, dim3(256), 0, st, res, x, o, n, base, d, vec);
    }
    void layer_norm(const float* x, float* y, size_t ga, size_t gb) const {
        hipLaunchKernelGGL(dpkg::layer_norm, dim3((unsigned)((M() + 3) / 4)), dim3(256), 0, st, x, y, M(), s.D, W + ga, W + gb);
    }
    // timestep projections of `count` t values (stride tstride) into tproj [count][L][D]; keep: the training
    // forward's stash of the MLP's intermediates
    void temb(const float* tvals, int tstride, int count, float* tproj, const dpkg::TembStash* keep = nullptr) const {
        const float neg = -(float)(log(10000.0) / (double)(s.D / 2 - 1));
        const size_t lds = (size_t)(s.D + 2 * s.E) * 4;
        hipLaunchKernelGGL(keep ? dpkg::temb<true> : dpkg::temb<false>, dim3((unsigned)count), dim3(256), lds, st, W + s.d0w,
                           W + s.d0b, W + s.d1w, W + s.d1b, W + s.wtp, W + s.btp, tvals, tstride, s.D, s.E, s.L, neg, tproj,
                           keep ? *keep : dpkg::TembStash{});
    }
};

// One GCNdiff / GCNpose forward of op.N poses x (N, J, cin) -> y (N, J, cout).  tp: per-layer timestep
// projections, rows of L*D floats (tp_stride 0: one row for every pose, else L*D per pose); null for
// GCNpose.  S: gen_act_floats(N) floats of scratch.  Six buffers reused layer after layer, relu + temb and
// resid + relu fused into GEMM epilogues.
static void gen_forward(const GenModel* g, const GenOps& op, const float* x, const float* tp, int tp_stride, float* y,
                        float* S) {
    const Stage& s = g->s;
    const GemmArena& ar = g->arena;
    const int D = s.D, M = op.M();
    const float* W = ar.dev;
    float* Hs = S;
    float* Ys = Hs + (size_t)M * D;
    float* Zs = Ys + (size_t)M * D;
    float* As = Zs + (size_t)M * 3 * std::max(D, s.cin);
    float* Fs = As + (size_t)M * D;
    float* Gs = Fs + (size_t)M * 2 * D;
    op.cheb(x, s.cin, Zs);
    op.gemm(ar, Zs, M, 3 * s.cin, s.win, W + s.bin, Hs, D, D, dpkg::G_BIAS);
    for (int l = 0; l < s.L; ++l) {
        const GenLayer& o = s.lay[l];
        op.layer_norm(Hs, Ys, o.n0a, o.n0b);
        op.gemm(ar, Ys, M, D, o.wqkv, W + o.bqkv, Zs, 3 * D, 3 * D, dpkg::G_BIAS);
        op.attention(Zs, As);
        op.gemm(ar, As, M, D, o.wo, W + o.bo, Hs, D, D, dpkg::G_RESID);
        op.layer_norm(Hs, Ys, o.n1a, o.n1b);
        op.graph(W + o.lg, Ys, D, As);
        op.gemm(ar, As, M, D, o.w1, W + o.b1, Fs, 2 * D, 2 * D, dpkg::G_RELU);
        op.graph(W + o.lg, Fs, 2 * D, Gs);
        op.gemm(ar, Gs, M, 2 * D, o.w2, W + o.b2, Hs, D, D, dpkg::G_RESID);
        op.cheb(Hs, D, Zs);
        op.gemm(ar, Zs, M, 3 * D, o.wc1, W + o.bc1, As, D, D, tp ? dpkg::G_RELU_TEMB : dpkg::G_RELU,
                tp ? tp + (size_t)l * D : nullptr, tp_stride);
        op.cheb(As, D, Zs);
        op.gemm(ar, Zs, M, 3 * D, o.wc2, W + o.bc2, Hs, D, D, dpkg::G_RESID_RELU);
    }
    op.cheb(Hs, D, Zs);
    op.gemm(ar, Zs, M, 3 * D, s.wout, W + s.bout, y, s.cout, s.cout, dpkg::G_BIAS);
}

// One dpkg::qsample launch over N poses of pe floats (dpk_q_sample, and gen_sample's copy-in with the start on)
static void gen_qsample(hipStream_t st, const float* x, float* xT, float* xT2, int N, int pe, const StartSpec& s,
                        uint64_t seed) {
    const long long n = (long long)N * pe;
    hipLaunchKernelGGL(dpkg::qsample, dim3(gen_blocks(n)), dim3(256), 0, st, x, xT, xT2, n, pe, s.sa, s.sb, s.scale,
                       s.rows, s.noise, (unsigned long long)seed);
}

// dpk_sample on the generic path: one forward + DDIM update per step.  Without trajectory outputs or
// caller noise the loop is the recorded hipGraph over the state buffer xt in the scratch (x copied in,
// the final copied out); otherwise the launches go straight to the caller's stream, the state in `out`.
// DPK_GEN_GRAPH=0 turns the graph off (A/B).
static int gen_sample(dpk_handle* h, Sched* sc, const float* x, float* out, float* xs, float* x0s, int N,
                      uint64_t seed, const float* noise, const StartSpec* start, hipStream_t st, bool cap) {
    GenModel* g = h->gen;
    const int K = sc->K;
    const long long n = (long long)N * g->s.J * g->s.cin;
    const size_t act = gen_act_floats(g->s, N), tpf = (size_t)K * g->s.L * g->s.D;
    float* S = nullptr;
    int rc = gen_scratch(h, st, cap, act + 2 * (size_t)n + tpf, &S, "dpk_sample");
    if (rc) return rc;
    float* eps = S + act;
    float* tproj = eps + n;
    float* xt = tproj + tpf;
    auto body = [&](hipStream_t s_, float* cur) {
        const GenOps op(g, s_, N, h->mask, h->pmask, h->n_cu, g->forms);
        op.temb(sc->coef + 5, 6, K, tproj);
        for (int s = 0; s < K; ++s) {
            gen_forward(g, op, cur, tproj + (size_t)s * g->s.L * g->s.D, 0, eps, S);
            hipLaunchKernelGGL(dpkg::ddim, dim3(gen_blocks(n)), dim3(256), 0, s_, cur, eps, cur,
                               x0s ? x0s + (size_t)s * n : nullptr, n, sc->coef + s * 6, s, sc->eta,
                               (unsigned long long)seed, noise ? noise + (size_t)s * n : nullptr);
            if (xs) (void)hipMemcpyAsync(xs + (size_t)(s + 1) * n, cur, (size_t)n * 4, hipMemcpyDeviceToDevice, s_);
        }
    };
    const char* gg_env = getenv("DPK_GEN_GRAPH");
    // under the caller's capture the launches go into the caller's graph (no recorded loop of our own)
    bool graphed = !cap && !xs && !x0s && !noise && !(gg_env && atoi(gg_env) == 0);
    hipGraphExec_t ex = nullptr;
    // a full cache evicts its least recently used loop once the device has drained; while that drain is
    // refused (another thread capturing) this call launches directly instead of recording
    if (graphed && g->graphs.size() >= GEN_GRAPHS) {
        bool hit = false;
        const GenGraphKey key{st, S, sc->serial, N, h->mask, h->pmask, sc->eta != 0.f ? seed : 0};
        for (auto& gg : g->graphs) hit = hit || gg.key == key;
        if (!hit && !drain_relaxed()) graphed = false;
    }
    if (graphed) {
        // the seed is read only by eta's counter-based draws: at eta = 0 it is not part of the recorded
        // loop, so calls that differ only in seed (test_hyber passes seed + i per batch) share one graph
        const GenGraphKey key{st, S, sc->serial, N, h->mask, h->pmask, sc->eta != 0.f ? seed : 0};
        for (auto& gg : g->graphs)
            if (gg.key == key) {
                ex = gg.exec;
                gg.last_use = ++g->use_clock;
            }
        if (!ex) {
            if (g->graphs.size() >= GEN_GRAPHS) {   // evict the least recently used (the device has drained, above)
                size_t lru = 0;
                for (size_t i = 1; i < g->graphs.size(); ++i)
                    if (g->graphs[i].last_use < g->graphs[lru].last_use) lru = i;
                (void)hipGraphExecDestroy(g->graphs[lru].exec);
                g->graphs.erase(g->graphs.begin() + (long)lru);
            }
            hipGraph_t graph = nullptr;
            HIPCHK(h, hipStreamBeginCapture(h->aux, hipStreamCaptureModeThreadLocal));
            body(h->aux, xt);
            const hipError_t le = hipGetLastError();
            const hipError_t ce = hipStreamEndCapture(h->aux, &graph);
            if (le != hipSuccess || ce != hipSuccess) {
                if (graph) (void)hipGraphDestroy(graph);
                return fail(h, DPK_E_HIP, std::string("dpk_sample: recording the generic loop: ") +
                                              hipGetErrorString(le != hipSuccess ? le : ce));
            }
            const hipError_t ie = hipGraphInstantiate(&ex, graph, nullptr, nullptr, 0);
            (void)hipGraphDestroy(graph);
            if (ie != hipSuccess) return fail(h, DPK_E_HIP, std::string("dpk_sample: hipGraphInstantiate: ") + hipGetErrorString(ie));
            g->graphs.push_back(GenGraph{key, ex, ++g->use_clock});
        }
    }
    rc = profiled(h, st, cap, "dpk_sample", [&]() -> int {
        // the loop's state starts as x, or with the hypothesis start on as x_T (then xs[0] too): outside the
        // recorded loop either way
        float* state = graphed ? xt : out;
        if (start) {
            gen_qsample(st, x, state, xs, N, g->s.J * g->s.cin, *start, seed);
        } else {
            if (xs) HIPCHK(h, hipMemcpyAsync(xs, x, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
            // out_dev == x_dev (x = sample(x)) launched directly: the state is already in place
            if (state != x) HIPCHK(h, hipMemcpyAsync(state, x, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
        }
        if (graphed) {
            HIPCHK(h, hipGraphLaunch(ex, st));
            HIPCHK(h, hipMemcpyAsync(out, xt, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
        } else {
            body(st, out);
        }
        HIPCHK(h, hipGetLastError());
        return DPK_OK;
    });
    return rc ? rc : sched_note_use(h, sc, st, cap);
}

// One dpkg::qsample_t launch over N poses of pe floats, and one dpkg::diff_loss launch over them (dpk_diff_loss)
static void gen_qsample_t(hipStream_t st, const float* x, float* xT, int N, int pe, const float* t, const float* qtab,
                          int nt, const StartSpec& s, uint64_t seed) {
    const long long n = (long long)N * pe;
    hipLaunchKernelGGL(dpkg::qsample_t, dim3(gen_blocks(n)), dim3(256), 0, st, x, xT, n, pe, t, qtab, nt, s.scale, s.rows,
                       s.noise, (unsigned long long)seed);
}
static void gen_diff_loss(hipStream_t st, const float* eps, int N, int pe, const StartSpec& s, uint64_t seed,
                          float* loss) {
    hipLaunchKernelGGL(dpkg::diff_loss, dim3(gen_blocks(N)), dim3(256), 0, st, eps, N, pe, s.scale, s.rows, s.noise,
                       (unsigned long long)seed, loss);
}

// dpk_eps on the generic path: per-pose timestep projections, one forward.  S: gen_eps_floats(N) floats of the
// call's scratch, or null to take them here
static int gen_eps(dpk_handle* h, const float* x, const float* t, float* eps, int N, hipStream_t st, bool cap,
                   float* S = nullptr) {
    GenModel* g = h->gen;
    const size_t act = gen_act_floats(g->s, N);
    if (!S) {
        const int rc = gen_scratch(h, st, cap, gen_eps_floats(g->s, N), &S, "dpk_eps");
        if (rc) return rc;
    }
    float* tproj = S + act;
    return profiled(h, st, cap, "dpk_eps", [&]() -> int {
        const GenOps op(g, st, N, h->mask, h->pmask, h->n_cu, g->forms);
        op.temb(t, 1, N, tproj);
        gen_forward(g, op, x, tproj, g->s.L * g->s.D, eps, S);
        HIPCHK(h, hipGetLastError());
        return DPK_OK;
    });
}

// dpk_pose on the generic path: GCNpose forward (no timestep projection), then xyz / uvxyz
static int gen_pose(dpk_handle* h, const float* x2d, float* xyz, float* uvxyz, int N, int Hn, int root_mode,
                    hipStream_t st, bool cap) {
    GenModel* g = h->gen;
    const size_t act = gen_act_floats(g->s, N);
    float* S = nullptr;
    const int rc = gen_scratch(h, st, cap, act + (size_t)N * g->s.J * g->s.cout, &S, "dpk_pose");
    if (rc) return rc;
    float* y = S + act;
    return profiled(h, st, cap, "dpk_pose", [&]() -> int {
        gen_forward(g, GenOps(g, st, N, h->mask, h->pmask, h->n_cu, g->forms), x2d, nullptr, 0, y, S);
        hipLaunchKernelGGL(dpkg::pose_out, dim3(gen_blocks((long long)N * g->s.J * (g->s.cin + g->s.cout))), dim3(256), 0,
                           st, x2d, y, N, g->s.J, g->s.cin, g->s.cout, xyz, uvxyz, Hn, root_mode);
        HIPCHK(h, hipGetLastError());
        return DPK_OK;
    });
}
