// dpk_generic_bwd.inc — the gradient of the denoising objective (dpk_diff_loss_grad) on the per-op path: the
// forward of dpk_generic.inc run once more with what the backward needs kept in the call's scratch, then the
// backward as per-op HIP kernels, fp32 throughout, eval mode (no dropout).  Included by dpk_kernels.hip after
// dpk_generic.inc and dpk_grad_layout.inc.
//   training forward  gen_forward's launches (the same kernels and form choices, out of place), every GEMM operand,
//                     ReLU output and residual-stream value of every layer stored (bwd_plan: the stash)
//   dX GEMMs          dA = dC W^T on gemm / gemm_sk / gemm_narrow against the transposed arena (BwdArena)
//   dW GEMMs          dW = A^T dC: dw_partial, one [K][N] slab per DW_ROWS rows on v_mfma_f32_16x16x4_f32, the bias
//                     gradient (column sums) as row K of the slab; dw_reduce adds the slabs in
//                     ascending order and writes the torch layout (transposed for nn.Linear, QKV split in three)
//   the rest          plain-VALU kernels: ln_bwd, attention_bwd, graph on L_g^T, dlg_partial + dlg_chain (to A_hat),
//                     cheb_t, relu_bwd, joint_sum, swish_bwd, loss_grad
// Every sum over rows or poses is a store pass of partials over a fixed partition (DW_ROWS rows, DLG_POSES poses)
// and an ordered sum pass: no float atomics, so the same call gives bitwise the same gradients.

namespace dpkg {

constexpr int DW_ROWS = 128;     // rows of one dW slab
constexpr int DLG_POSES = 8;     // poses of one dL_g slab

// the backward's kernel forms, one bit each (dpk_debug_grad_forms; diffpose_amd/gcndiff.py GRAD_FORMS)
enum BwdForm : unsigned {
    B_DW_VEC = 1u << 0,
    B_DW_SCALAR = 1u << 1,
    B_ATTN_BWD_STAGED = 1u << 2,
    B_LN_BWD = 1u << 3,
    B_GRAPH_T_STAGED = 1u << 4,
    B_GRAPH_T_GLOBAL = 1u << 5,
    B_CHEB_T = 1u << 6,
    B_DLG_STAGED = 1u << 7,
    B_TEMB_BWD = 1u << 8,
    B_ATTN_BWD_GLOBAL = 1u << 9,
    B_DLG_GLOBAL = 1u << 10,
};

// P[slab][k][n] = sum over the slab's rows r (ascending, four at a time) of A[r][k] G[r][n]; slab s holds rows
// DW_ROWS s .. ; slab stride `ps` floats ((K + 1) N: row K is the column sum of G over the slab's rows, the bias
// gradient, kept by the waves of the first row of tiles: each lane adds its rows in ascending order, then the four
// lane rows meet in a fixed butterfly).  One wave per
// output tile, operands straight from global memory into MFMA fragments (A^T as the first operand: lane l feeds
// output row l & 15 with row r + (l >> 4) of A).
// VEC (K, N, lda, ldg multiples of 4, 16-byte aligned A, G, P): a 64 x 64 tile as 4 x 4 interleaved MFMA tiles, tile
// (e, f) holding k = k0 + 4 i + e, n = n0 + 4 j + f, so a lane loads one float4 of A and one of G per four rows and
// stores float4s; else a 16 x 32 tile from scalar loads.
template <bool VEC>
__global__ void __launch_bounds__(256) dw_partial(const float* __restrict__ A, int lda, const float* __restrict__ G,
                                                  int ldg, float* __restrict__ P, size_t ps, int M, int K, int N) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    const int r0 = blockIdx.x * DW_ROWS, r1 = min(M, r0 + DW_ROWS);
    float* Ps = P + (size_t)blockIdx.x * ps;
    const int tile = blockIdx.y * 4 + wave;
    if constexpr (VEC) {
        const int KT = (K + 63) >> 6, NT = (N + 63) >> 6;
        if (tile >= KT * NT) return;
        const int k0 = (tile / NT) * 64, n0 = (tile % NT) * 64;
        const int ka = k0 + 4 * li, nb = n0 + 4 * li;
        f32x4 acc[4][4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int f = 0; f < 4; ++f) acc[e][f] = f32x4{0.f, 0.f, 0.f, 0.f};
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        f32x4 cs = zero;
#pragma unroll 4
        for (int r = r0; r < r1; r += 4) {
            const int row = r + lk;
            const bool in = row < r1;
            const f32x4 a = in && ka < K ? *reinterpret_cast<const f32x4*>(A + (size_t)row * lda + ka) : zero;
            const f32x4 b = in && nb < N ? *reinterpret_cast<const f32x4*>(G + (size_t)row * ldg + nb) : zero;
            cs += b;
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int f = 0; f < 4; ++f) acc[e][f] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[f], acc[e][f], 0, 0, 0);
        }
        if (k0 == 0) {      // wave-uniform
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                cs[e] += __shfl_xor(cs[e], 16);
                cs[e] += __shfl_xor(cs[e], 32);
            }
            if (lk == 0 && nb < N) *reinterpret_cast<f32x4*>(Ps + (size_t)K * N + nb) = cs;
        }
        if (nb >= N) return;
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = k0 + 4 * (4 * lk + q) + e;
                if (k >= K) continue;
                *reinterpret_cast<f32x4*>(Ps + (size_t)k * N + nb) =
                    f32x4{acc[e][0][q], acc[e][1][q], acc[e][2][q], acc[e][3][q]};
            }
    } else {
        const int KT = (K + 15) >> 4, NT = (N + 31) >> 5;
        if (tile >= KT * NT) return;
        const int k0 = (tile / NT) * 16, n0 = (tile % NT) * 32;
        const int ka = k0 + li, nb0 = n0 + li, nb1 = n0 + 16 + li;
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        float cs0 = 0.f, cs1 = 0.f;
#pragma unroll 4
        for (int r = r0; r < r1; r += 4) {
            const int row = r + lk;
            const bool in = row < r1;
            const float a = in && ka < K ? A[(size_t)row * lda + ka] : 0.f;
            const float b0 = in && nb0 < N ? G[(size_t)row * ldg + nb0] : 0.f;
            const float b1 = in && nb1 < N ? G[(size_t)row * ldg + nb1] : 0.f;
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1, acc1, 0, 0, 0);
            cs0 += b0;
            cs1 += b1;
        }
        if (k0 == 0) {      // wave-uniform
            cs0 += __shfl_xor(cs0, 16);
            cs0 += __shfl_xor(cs0, 32);
            cs1 += __shfl_xor(cs1, 16);
            cs1 += __shfl_xor(cs1, 32);
            if (lk == 0 && nb0 < N) Ps[(size_t)K * N + nb0] = cs0;
            if (lk == 0 && nb1 < N) Ps[(size_t)K * N + nb1] = cs1;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = k0 + 4 * lk + q;
            if (k >= K) continue;
            if (nb0 < N) Ps[(size_t)k * N + nb0] = acc0[q];
            if (nb1 < N) Ps[(size_t)k * N + nb1] = acc1[q];
        }
    }
}

// P[slab * ps + off + n] = sum over the slab's rows of G[r][n]: 64 columns per workgroup, each wave one quarter of
// the slab's rows in ascending order, the four quarters added in order
__global__ void __launch_bounds__(256) colsum_partial(const float* __restrict__ G, int ldg, float* __restrict__ P,
                                                      size_t ps, size_t off, int M, int N) {
    __shared__ float part[4][64];
    const int c = threadIdx.x & 63, qd = threadIdx.x >> 6, n = blockIdx.y * 64 + c;
    const int r0 = blockIdx.x * DW_ROWS, r1 = min(M, r0 + DW_ROWS);
    const int q0 = r0 + qd * (DW_ROWS / 4), q1 = min(r1, q0 + DW_ROWS / 4);
    float acc = 0.f;
    if (n < N)
        for (int r = q0; r < q1; ++r) acc += G[(size_t)r * ldg + n];
    part[qd][c] = acc;
    __syncthreads();
    if (qd == 0 && n < N) P[(size_t)blockIdx.x * ps + off + n] = ((part[0][c] + part[1][c]) + part[2][c]) + part[3][c];
}

// p[0] + p[stride] + ... over n slabs in ascending order, the loads of eight slabs in flight
__device__ __forceinline__ float slab_sum(const float* __restrict__ p, size_t stride, int n) {
    float acc = 0.f;
    int s = 0;
    for (; s + 8 <= n; s += 8) {
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = p[(size_t)(s + i) * stride];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc += v[i];
    }
    for (; s < n; ++s) acc += p[(size_t)s * stride];
    return acc;
}

// The ordered sum pass of a dW: element (k, n) of the [K + 1][N] slabs summed over the slabs ascending, then
// written where torch keeps it.  Column n belongs to output segment j = n / Ns (QKV: three nn.Linear of Ns = D
// columns; else Ns = N), nn = n % Ns: rows k < K go to w[j][nn * K + k] (transpose: nn.Linear's [out][in]) or
// w[j][k * Ns + nn] (ChebConv's [3 in][out]); row K, the column sums, to b[j][nn].
struct DwDst {
    float* w[3];
    float* b[3];
};
__global__ void __launch_bounds__(256) dw_reduce(const float* __restrict__ P, size_t ps, int nslab, int K, int N,
                                                 int transpose, int Ns, DwDst d) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)(K + 1) * N) return;
    const int k = (int)(e / N), n = (int)(e - (long long)k * N);
    const float acc = slab_sum(P + (size_t)e, ps, nslab);
    const int j = n / Ns, nn = n - j * Ns;
    if (k < K) {
        if (d.w[j]) d.w[j][transpose ? (size_t)nn * K + k : (size_t)k * Ns + nn] = acc;
    } else if (d.b[j]) {
        d.b[j][nn] = acc;
    }
}

// LayerNorm backward (GraFormer.py:67-70: y = a (x - mean) / (sd + eps) + b, sd unbiased): a wave per row.
//   g = dy a;  dx = (g - mean(g)) / (sd + eps) - (x - mean) sum(g (x - mean)) / ((sd + eps)^2 (D - 1) sd)
// added into dX (the residual stream's gradient); T = dy (x - mean) / (sd + eps), whose column sums are a's
// gradient (dy's are b's).  mean and sd recomputed as layer_norm computes them.
__global__ void __launch_bounds__(256) ln_bwd(const float* __restrict__ X, const float* __restrict__ dY,
                                              const float* __restrict__ ga, float* __restrict__ dX,
                                              float* __restrict__ T, int M, int D) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    const float* x = X + (size_t)row * D;
    const float* dy = dY + (size_t)row * D;
    float s = 0.f;
    for (int c = lane; c < D; c += 64) s += x[c];
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
    for (int c = lane; c < D; c += 64) {
        const float d = x[c] - mean;
        q = fmaf(d, d, q);
    }
    const float sd = sqrtf(wave_sum(q) / (float)(D - 1));
    const float den = sd + 1e-6f;
    float s1 = 0.f, s2 = 0.f;
    for (int c = lane; c < D; c += 64) {
        const float g = dy[c] * ga[c];
        s1 += g;
        s2 = fmaf(g, x[c] - mean, s2);
    }
    s1 = wave_sum(s1) / (float)D;
    s2 = wave_sum(s2) / (den * den * (float)(D - 1) * sd);
    for (int c = lane; c < D; c += 64) {
        const float xc = x[c] - mean, g = dy[c] * ga[c];
        T[(size_t)row * D + c] = dy[c] * xc / den;
        dX[(size_t)row * D + c] += (g - s1) / den - xc * s2;
    }
}

// Attention backward (GraFormer.py:116-140): one workgroup per pose, `hb` heads per pass.  Pass 1, one thread per
// (head, query): the probabilities recomputed as attention computes them (into LDS), dP_j = dO . V_j, then
// dS_j = p_j (dP_j - sum p dP) / sqrt(dk), 0 for a masked key.  Pass 2, one thread per (head, row, d):
// dQ = dS K, dK = dS^T Q, dV = P^T dO, sums over keys / queries ascending.  Dynamic LDS 2 hb J J floats, and with
// `stage` the pose's rows [q | k | v | dO] behind them, J rows of (4 D) | 1 floats (an odd stride: the queries of a
// head read distinct banks); without it the rows are read from global memory (a pose too wide for 64 KB).
__global__ void __launch_bounds__(256) attention_bwd(const float* __restrict__ qkv, const float* __restrict__ dO,
                                                     float* __restrict__ dqkv, int J, int D, int H, unsigned mask,
                                                     const unsigned* __restrict__ pmask, int hb, int stage) {
    extern __shared__ __attribute__((aligned(16))) float absm[];
    float* Ps = absm;
    float* Ss = absm + (size_t)hb * J * J;
    const int p = blockIdx.x, dk = D / H;
    const unsigned m = pmask ? pmask[p] : mask;
    const float sq = sqrtf((float)dk);
    const float* rows = qkv + (size_t)p * J * 3 * D;
    const float* dor = dO + (size_t)p * J * D;
    int RS = 3 * D, DS = D;
    float* out = dqkv + (size_t)p * J * 3 * D;
    if (stage) {
        float* st = Ss + (size_t)hb * J * J;
        const int RW = (4 * D) | 1;
        for (int i = threadIdx.x; i < J * 3 * D; i += 256) {
            const int r = i / (3 * D);
            st[r * RW + (i - r * 3 * D)] = rows[i];
        }
        for (int i = threadIdx.x; i < J * D; i += 256) {
            const int r = i / D;
            st[r * RW + 3 * D + (i - r * D)] = dor[i];
        }
        __syncthreads();
        rows = st, dor = st + 3 * D, RS = RW, DS = RW;
    }
    for (int h0 = 0; h0 < H; h0 += hb) {
        const int nh = min(hb, H - h0);
        for (int t = threadIdx.x; t < nh * J; t += 256) {
            const int hl = t / J, q = t - hl * J, h = h0 + hl;
            float* pr = Ps + (size_t)t * J;
            float* sr = Ss + (size_t)t * J;
            const float* qr = rows + q * RS + h * dk;
            const float* go = dor + q * DS + h * dk;
            float mx = -INFINITY;
            for (int j = 0; j < J; ++j) {
                const float* kr = rows + j * RS + D + h * dk;
                float s = 0.f;
                for (int d = 0; d < dk; ++d) s = fmaf(qr[d], kr[d], s);
                s = ((m >> j) & 1u) ? s / sq : -1e9f;
                pr[j] = s;
                mx = fmaxf(mx, s);
            }
            float sum = 0.f;
            for (int j = 0; j < J; ++j) {
                const float e = expf(pr[j] - mx);
                pr[j] = e;
                sum += e;
            }
            float dot = 0.f;
            for (int j = 0; j < J; ++j) {
                const float pj = pr[j] / sum;
                pr[j] = pj;
                const float* vr = rows + j * RS + 2 * D + h * dk;
                float dp = 0.f;
                for (int d = 0; d < dk; ++d) dp = fmaf(go[d], vr[d], dp);
                sr[j] = dp;
                dot = fmaf(pj, dp, dot);
            }
            for (int j = 0; j < J; ++j) sr[j] = ((m >> j) & 1u) ? pr[j] * (sr[j] - dot) / sq : 0.f;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < nh * J * dk; e += 256) {
            const int hl = e / (J * dk), rem = e - hl * J * dk, j = rem / dk, d = rem - j * dk;
            const int c = (h0 + hl) * dk + d;
            const float* pb = Ps + (size_t)hl * J * J;
            const float* sb = Ss + (size_t)hl * J * J;
            float dq = 0.f, dkk = 0.f, dv = 0.f;
            for (int i = 0; i < J; ++i) {
                dq = fmaf(sb[j * J + i], rows[i * RS + D + c], dq);
                dkk = fmaf(sb[i * J + j], rows[i * RS + c], dkk);
                dv = fmaf(pb[i * J + j], dor[i * DS + c], dv);
            }
            out[j * 3 * D + c] = dq;
            out[j * 3 * D + D + c] = dkk;
            out[j * 3 * D + 2 * D + c] = dv;
        }
        __syncthreads();
    }
}

// P[slab][j][i] = sum over the slab's poses p (ascending) and channels c (ascending) of dY[p][j][c] X[p][i][c]:
// the GraphNet Laplacian's gradient of one of its two uses (Y = L_g X), DLG_POSES poses per workgroup.  STAGE: each
// pose's dY and X rows go through LDS (2 J (C | 1) floats: an odd row stride, the threads of a wave read distinct
// banks), every thread keeping its up to four (j, i) sums in registers; else straight from global memory.
template <bool STAGE>
__global__ void __launch_bounds__(256) dlg_partial(const float* __restrict__ dY, const float* __restrict__ X,
                                                   float* __restrict__ P, int N, int J, int C) {
    const int p0 = blockIdx.x * DLG_POSES, p1 = min(N, p0 + DLG_POSES);
    if constexpr (STAGE) {
        extern __shared__ __attribute__((aligned(16))) float dlsm[];
        const int CW = C | 1;
        float* ys = dlsm;
        float* xs = dlsm + (size_t)J * CW;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};      // J J <= 1024 = 4 x 256
        for (int p = p0; p < p1; ++p) {
            __syncthreads();
            const float* a = dY + (size_t)p * J * C;
            const float* b = X + (size_t)p * J * C;
            for (int i = threadIdx.x; i < J * C; i += 256) {
                const int r = i / C, c = i - r * C;
                ys[r * CW + c] = a[i];
                xs[r * CW + c] = b[i];
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = threadIdx.x + 256 * u;
                if (e >= J * J) break;
                const int j = e / J, i = e - j * J;
                float v = acc[u];
                for (int c = 0; c < C; ++c) v = fmaf(ys[j * CW + c], xs[i * CW + c], v);
                acc[u] = v;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = threadIdx.x + 256 * u;
            if (e < J * J) P[(size_t)blockIdx.x * J * J + e] = acc[u];
        }
        return;
    }
    for (int e = threadIdx.x; e < J * J; e += 256) {
        const int j = e / J, i = e - j * J;
        float acc = 0.f;
        for (int p = p0; p < p1; ++p) {
            const float* a = dY + ((size_t)p * J + j) * C;
            const float* b = X + ((size_t)p * J + i) * C;
            for (int c = 0; c < C; ++c) acc = fmaf(a[c], b[c], acc);
        }
        P[(size_t)blockIdx.x * J * J + e] = acc;
    }
}

// dA_hat from the dL_g slabs (summed ascending) through L_ij = d_i A_ij d_j, d_k = (colsum_k + 1e-5)^-1/2
// (GraFormer.py:174-178): dA_ij = dL_ij d_i d_j + dc_j, dc_k = -1/2 d_k^3 (sum_j dL_kj A_kj d_j + sum_i dL_ik d_i A_ik).
// One workgroup; dynamic LDS J J + 2 J floats.
__global__ void __launch_bounds__(256) dlg_chain(const float* __restrict__ P, int nslab, const float* __restrict__ Ah,
                                                 float* __restrict__ dA, int J) {
    extern __shared__ __attribute__((aligned(16))) float lcsm[];
    float* dL = lcsm;
    float* dd = lcsm + J * J;
    float* dc = dd + J;
    for (int e = threadIdx.x; e < J * J; e += 256) dL[e] = slab_sum(P + e, (size_t)J * J, nslab);
    for (int k = threadIdx.x; k < J; k += 256) {
        float r = 0.f;
        for (int i = 0; i < J; ++i) r += Ah[i * J + k];
        dd[k] = 1.0f / sqrtf(r + 1e-5f);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < J; k += 256) {
        float acc = 0.f;
        for (int j = 0; j < J; ++j) acc = fmaf(dL[k * J + j] * Ah[k * J + j], dd[j], acc);
        for (int i = 0; i < J; ++i) acc = fmaf(dL[i * J + k] * Ah[i * J + k], dd[i], acc);
        dc[k] = -0.5f * dd[k] * dd[k] * dd[k] * acc;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < J * J; e += 256) {
        const int i = e / J, j = e - i * J;
        dA[e] = dL[e] * dd[i] * dd[j] + dc[j];
    }
}

// The transposed Chebyshev product: dX[p][j][c] (+)= dZ0 + sum_i T1[i][j] dZ1[p][i][c] + sum_i T2[i][j] dZ2[p][i][c]
// for dZ [p][j] = [dZ0 | dZ1 | dZ2] (3C floats a row), one thread per output, sums over i ascending
__global__ void __launch_bounds__(256) cheb_t(const float* __restrict__ T1, const float* __restrict__ T2,
                                              const float* __restrict__ dZ, float* __restrict__ dX, int N, int J, int C,
                                              int accumulate) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int c = (int)(t % C);
    const long long pj = t / C;
    if (pj >= (long long)N * J) return;
    const int j = (int)(pj % J);
    const long long p = pj / J;
    const float* zp = dZ + (size_t)p * J * 3 * C + c;
    float a1 = 0.f, a2 = 0.f;
    for (int i = 0; i < J; ++i) {
        a1 = fmaf(T1[i * J + j], zp[(size_t)i * 3 * C + C], a1);
        a2 = fmaf(T2[i * J + j], zp[(size_t)i * 3 * C + 2 * C], a2);
    }
    const float v = zp[(size_t)j * 3 * C] + a1 + a2;
    float* o = dX + (size_t)pj * C + c;
    *o = accumulate ? *o + v : v;
}

// elementwise pieces
__global__ void __launch_bounds__(256) relu_bwd(const float* __restrict__ dOut, const float* __restrict__ R,
                                                float* __restrict__ dPre, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dPre[i] = R[i] > 0.f ? dOut[i] : 0.f;
}
__global__ void __launch_bounds__(256) add2(const float* __restrict__ a, const float* __restrict__ b,
                                            float* __restrict__ o, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) o[i] = a[i] + b[i];
}
// C1 = R1 + tp[pose][c] (the G_RELU_TEMB epilogue's addition, on the kept ReLU output)
__global__ void __launch_bounds__(256) add_temb(const float* __restrict__ R, const float* __restrict__ tp, int tps,
                                                float* __restrict__ o, long long n, int D, int J) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long row = i / D;
    o[i] = R[i] + tp[(size_t)(row / J) * tps + (int)(i - row * D)];
}
// dtp[p][c] (stride tps) = sum over the pose's joints (ascending) of dC[p][j][c]
__global__ void __launch_bounds__(256) joint_sum(const float* __restrict__ dC, float* __restrict__ dtp, int tps, int N,
                                                 int J, int D) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)N * D) return;
    const long long p = i / D;
    const int c = (int)(i - p * D);
    float acc = 0.f;
    for (int j = 0; j < J; ++j) acc += dC[((size_t)p * J + j) * D + c];
    dtp[(size_t)p * tps + c] = acc;
}
// du = dh d/du (u sigmoid(u))
__global__ void __launch_bounds__(256) swish_bwd(const float* __restrict__ dh, const float* __restrict__ u,
                                                 float* __restrict__ du, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = u[i], s = 1.0f / (1.0f + expf(-v));
    du[i] = dh[i] * (s + v * s * (1.0f - s));
}
// dEps = -2 weight (target - eps), target as diff_loss takes it
__global__ void __launch_bounds__(256) loss_grad(const float* __restrict__ eps, long long n, int pe,
                                                 const float* __restrict__ scale, int rows,
                                                 const float* __restrict__ noise, unsigned long long seed, float weight,
                                                 float* __restrict__ dEps) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    const long long p = g / pe;
    const int r = (int)(g - p * pe);
    const float e = noise ? noise[g] : dpk::normal_noise(seed, -1, g);
    const float target = e * (scale ? scale[(size_t)(p % rows) * pe + r] : 1.0f);
    dEps[g] = -2.0f * weight * (target - eps[g]);
}

// temb with what its backward reads kept: emb [D], the pre-activations u0, u1 and the activations h0, h1 [E] per
// pose; the arithmetic of temb (tproj is bitwise its)
__global__ void __launch_bounds__(256) temb_train(const float* __restrict__ W0, const float* __restrict__ B0,
                                                  const float* __restrict__ W1, const float* __restrict__ B1,
                                                  const float* __restrict__ WP, const float* __restrict__ BP,
                                                  const float* __restrict__ tvals, int D, int E, int L, float neg_scale,
                                                  float* __restrict__ tproj, float* __restrict__ emb_o,
                                                  float* __restrict__ u0_o, float* __restrict__ h0_o,
                                                  float* __restrict__ u1_o, float* __restrict__ h1_o) {
    extern __shared__ float ttsm[];
    float* emb = ttsm;
    float* h0 = ttsm + D;
    float* h1 = h0 + E;
    const size_t b = blockIdx.x;
    const float t = tvals[b];
    const int half = D / 2;
    for (int i = threadIdx.x; i < D; i += 256) {
        float v = 0.f;
        if (i < 2 * half) {
            const int k = i < half ? i : i - half;
            const float arg = t * expf((float)k * neg_scale);
            v = i < half ? sinf(arg) : cosf(arg);
        }
        emb[i] = v;
        emb_o[b * D + i] = v;
    }
    __syncthreads();
    for (int o = threadIdx.x; o < E; o += 256) {
        float acc = 0.f;
        for (int k = 0; k < D; ++k) acc = fmaf(emb[k], W0[(size_t)k * E + o], acc);
        const float v = acc + B0[o];
        h0[o] = v * (1.0f / (1.0f + expf(-v)));
        u0_o[b * E + o] = v;
        h0_o[b * E + o] = h0[o];
    }
    __syncthreads();
    for (int o = threadIdx.x; o < E; o += 256) {
        float acc = 0.f;
        for (int k = 0; k < E; ++k) acc = fmaf(h0[k], W1[(size_t)k * E + o], acc);
        const float v = acc + B1[o];
        h1[o] = v * (1.0f / (1.0f + expf(-v)));
        u1_o[b * E + o] = v;
        h1_o[b * E + o] = h1[o];
    }
    __syncthreads();
    for (int o = threadIdx.x; o < L * D; o += 256) {
        const int l = o / D, c = o - l * D;
        const float* wp = WP + (size_t)l * E * D;
        float acc = 0.f;
        for (int k = 0; k < E; ++k) acc = fmaf(h1[k], wp[(size_t)k * D + c], acc);
        tproj[b * L * D + o] = acc + BP[o];
    }
}

}  // namespace dpkg

// ---------------------------------------------------------------------------------------
// Host side

// What a handle keeps for dpk_diff_loss_grad, built on its first call and again after new weights or a new graph
struct BwdModel {
    GenModel* own = nullptr;     // a persistent-sampler handle's per-op model (a per-op handle uses its own)
    GradLayout lay;
    BwdArena arena;
    float* dev = nullptr;        // device: the transposed arena
    size_t dev_floats = 0;
    std::vector<GenPack> packs;  // gemm_sk copies of its GEMM blocks
    std::vector<float> hp;
    float* devp = nullptr;
    size_t devp_floats = 0;
    uint64_t serial = 0;         // dpk_handle::stage_serial it was built from (0: never)
    unsigned fforms = 0, bforms = 0;   // GenForm bits of the forward and dX launches; BwdForm bits
};

static void bwd_free(BwdModel* b) {
    if (!b) return;
    gen_free(b->own);
    if (b->dev) (void)hipFree(b->dev);
    if (b->devp) (void)hipFree(b->devp);
    delete b;
}

// gemm_sk's fragment order for the transposed blocks (gen_pack's rule and layout)
static void bwd_pack(BwdModel* b) {
    b->packs.clear();
    size_t off = 0;
    for (const BwdBlock& k : b->arena.blocks) {
        const int K = k.N, N = k.K;      // the transposed block is [N][K] of the forward's
        if (K % 4 || N % 4 || N <= 8) continue;
        const int NT16 = (N + 15) / 16, NJ = NT16 % 4 == 0 ? 4 : 2, NTp = (NT16 + NJ - 1) / NJ * NJ;
        b->packs.push_back(GenPack{k.w, off, K, N, NJ});
        off += (size_t)((K + 15) / 16) * NTp * 256;
    }
    b->hp.assign(off, 0.f);
    for (const GenPack& p : b->packs) {
        const int KC = (p.K + 15) / 16, NT16 = (p.N + 15) / 16, NTp = (NT16 + p.NJ - 1) / p.NJ * p.NJ;
        const float* W = b->arena.h.data() + p.w;
        float* dst = b->hp.data() + p.off;
        for (int c = 0; c < KC; ++c)
            for (int t = 0; t < NT16; ++t)
                for (int l = 0; l < 64; ++l)
                    for (int s = 0; s < 4; ++s) {
                        const int k = 16 * c + 4 * (l >> 4) + s, n = 16 * t + (l & 15);
                        if (k < p.K && n < p.N) dst[(((size_t)c * NTp + t) * 64 + l) * 4 + s] = W[(size_t)k * p.N + n];
                    }
    }
}

// One GEMM C = epilogue(A[M][K] W[K][N] + bias) in the form gen_forward's rule picks (the same predicates): W, bias
// device pointers, pk its gemm_sk copy or null
static void bwd_gemm(unsigned& forms, hipStream_t st, int n_cu, int J, const float* a, int M, int K, const float* W,
                     const GenPack* pk, const float* devp, const float* bias, float* c, int ldc, int Nn, int mode,
                     const float* tpl = nullptr, int tps = 0) {
    const long long nt = (Nn + dpkg::GBN - 1) / dpkg::GBN, cu = std::max(n_cu, 1);
    int bm = 128;
    long long best = -1;
    for (int cand : {128, 64, 32}) {
        const long long cost = ((M + cand - 1) / cand * nt + cu - 1) / cu * cand;
        if (best < 0 || cost < best) best = cost, bm = cand;
    }
    const dim3 grid((unsigned)((M + bm - 1) / bm), (unsigned)nt);
    auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    const bool vec = K % 4 == 0 && Nn % 4 == 0 && al16(a) && al16(W);
    if (Nn <= 8 && (size_t)K * Nn * 4 <= 65536) {
        forms |= dpkg::F_GEMM_NARROW;
        hipLaunchKernelGGL(dpkg::gemm_narrow, dim3((unsigned)((M + 3) / 4)), dim3(256), (size_t)K * Nn * 4, st, a, K, W, bias,
                           c, ldc, M, Nn, K, mode, tpl, tps, J);
        return;
    }
    if (pk && vec && ldc % 4 == 0 && al16(c) && al16(bias) && (!tpl || (al16(tpl) && tps % 4 == 0)) &&
        (size_t)M * K * 4 + (size_t)K * 4 < dpkg::SK_OOR) {
        const dim3 gs((unsigned)((M + 15) / 16), (unsigned)(((Nn + 15) / 16 + pk->NJ - 1) / pk->NJ));
        forms |= pk->NJ == 4 ? dpkg::F_GEMM_SK4 : dpkg::F_GEMM_SK2;
        if (pk->NJ == 4)
            hipLaunchKernelGGL(dpkg::gemm_sk<4>, gs, dim3(256), 0, st, a, K, devp + pk->off, bias, c, ldc, M, Nn, K, mode,
                               tpl, tps, J);
        else
            hipLaunchKernelGGL(dpkg::gemm_sk<2>, gs, dim3(256), 0, st, a, K, devp + pk->off, bias, c, ldc, M, Nn, K, mode,
                               tpl, tps, J);
        return;
    }
#define DPKG_GEMM(BM_, V_) hipLaunchKernelGGL((dpkg::gemm<BM_, V_>), grid, dim3(256), 0, st, a, K, W, bias, c, ldc, M, Nn, K, mode, tpl, tps, J)
    if (bm == 128) {
        forms |= vec ? dpkg::F_GEMM_128_VEC : dpkg::F_GEMM_128_SCALAR;
        if (vec) DPKG_GEMM(128, true);
        else DPKG_GEMM(128, false);
    } else if (bm == 64) {
        forms |= vec ? dpkg::F_GEMM_64_VEC : dpkg::F_GEMM_64_SCALAR;
        if (vec) DPKG_GEMM(64, true);
        else DPKG_GEMM(64, false);
    } else {
        forms |= vec ? dpkg::F_GEMM_32_VEC : dpkg::F_GEMM_32_SCALAR;
        if (vec) DPKG_GEMM(32, true);
        else DPKG_GEMM(32, false);
    }
#undef DPKG_GEMM
}

static const GenPack* find_pack(const std::vector<GenPack>& packs, size_t w, int K, int N) {
    for (const GenPack& p : packs)
        if (p.w == w && p.K == K && p.N == N) return &p;
    return nullptr;
}

// The call's scratch, in floats, every part on a 256-byte boundary.  Per layer the stash keeps 22 D floats a row
// (H, Y0, QKV 3D, A, H1, Y1, G1, F 2D, G2 2D, H2, Z1 3D, R1, Z2 3D, R2); beside the layers 3 cin + 4 D a row (the
// input's and the output's Chebyshev operands, the last H), and D + 4 E + L D floats a pose for the timestep MLP:
//   stash(N) = N J (22 D L + 4 D + 3 cin) + N (D + 4 E + L D)
// then the backward's working set: 10 D + 2 cout + cin floats a row, 2 E + L D a pose, the dW slabs and dL_g slabs.
struct BwdLayerBufs {
    float *H, *Y0, *QKV, *A, *H1, *Y1, *G1, *F, *G2, *H2, *Z1, *R1, *Z2, *R2;
};
struct BwdPlan {
    std::vector<BwdLayerBufs> lay;
    float *xt, *eps, *dEps, *Z0, *Hlast, *Zout, *C1;
    float *tproj, *dtp, *emb, *u0, *h0, *u1, *h1, *dh, *du;
    float *dH, *tD1, *tD2, *t3D, *t2Da, *t2Db, *Pdw, *Plg;
    size_t pdw_floats, stash_floats, floats;
};
static BwdPlan bwd_plan(const Stage& s, int N, float* base) {
    BwdPlan p;
    const size_t M = (size_t)N * s.J, D = s.D, E = s.E, L = s.L;
    size_t o = 0;
    auto take = [&](size_t n) {
        float* at = base + o;      // base null: sizes only
        o += (n + 63) / 64 * 64;
        return at;
    };
    p.lay.resize(L);
    p.Z0 = take(M * 3 * s.cin);
    for (auto& b : p.lay) {
        b.H = take(M * D), b.Y0 = take(M * D), b.QKV = take(M * 3 * D), b.A = take(M * D), b.H1 = take(M * D);
        b.Y1 = take(M * D), b.G1 = take(M * D), b.F = take(M * 2 * D), b.G2 = take(M * 2 * D), b.H2 = take(M * D);
        b.Z1 = take(M * 3 * D), b.R1 = take(M * D), b.Z2 = take(M * 3 * D), b.R2 = take(M * D);
    }
    p.Hlast = take(M * D), p.Zout = take(M * 3 * D);
    p.tproj = take((size_t)N * L * D), p.emb = take((size_t)N * D);
    p.u0 = take((size_t)N * E), p.h0 = take((size_t)N * E), p.u1 = take((size_t)N * E), p.h1 = take((size_t)N * E);
    p.stash_floats = o;
    p.xt = take(M * s.cin), p.eps = take(M * s.cout), p.dEps = take(M * s.cout), p.C1 = take(M * D);
    p.dtp = take((size_t)N * L * D), p.dh = take((size_t)N * E), p.du = take((size_t)N * E);
    p.dH = take(M * D), p.tD1 = take(M * D), p.tD2 = take(M * D), p.t3D = take(M * 3 * D);
    p.t2Da = take(M * 2 * D), p.t2Db = take(M * 2 * D);
    // the dW slabs: (K + 1) N floats per DW_ROWS rows, the largest of the row GEMMs (M rows) and the MLP's (N rows)
    const size_t sm = (M + dpkg::DW_ROWS - 1) / dpkg::DW_ROWS, sn = ((size_t)N + dpkg::DW_ROWS - 1) / dpkg::DW_ROWS;
    const size_t kn_rows = std::max(std::max((3 * D + 1) * D, (D + 1) * 3 * D),
                                    std::max((3 * (size_t)s.cin + 1) * D, (3 * D + 1) * (size_t)s.cout));
    p.pdw_floats = std::max(sm * kn_rows, sn * (E + 1) * E);
    p.Pdw = take(p.pdw_floats);
    p.Plg = take(2 * (((size_t)N + dpkg::DLG_POSES - 1) / dpkg::DLG_POSES) * s.J * s.J);
    p.floats = o;
    return p;
}

// (Re)build what the handle keeps for the backward: the per-op model of a persistent-sampler handle, the parameter
// layout, the transposed arena and its gemm_sk copies, uploaded.  Waits for the device (like a weight upload).
static int bwd_prepare(dpk_handle* h) {
    if (!h->bwd) h->bwd = new BwdModel();
    BwdModel* b = h->bwd;
    if (b->serial == h->stage_serial) return DPK_OK;
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->gen) {
        if (!b->own) b->own = gen_new(h->stage);
        const int rc = gen_upload(h, b->own);
        if (rc) return rc;
    }
    HIPCHK(h, hipDeviceSynchronize());
    b->lay = grad_layout(h->stage);
    bwd_arena_build(h->stage, b->arena);
    bwd_pack(b);
    if (b->dev_floats < b->arena.floats) {
        if (b->dev) HIPCHK(h, hipFree(b->dev));
        b->dev = nullptr, b->dev_floats = 0;
        HIPCHK(h, hipMalloc(&b->dev, b->arena.floats * 4));
        b->dev_floats = b->arena.floats;
    }
    HIPCHK(h, hipMemcpy(b->dev, b->arena.h.data(), b->arena.floats * 4, hipMemcpyHostToDevice));
    if (b->devp_floats < b->hp.size()) {
        if (b->devp) HIPCHK(h, hipFree(b->devp));
        b->devp = nullptr, b->devp_floats = 0;
        HIPCHK(h, hipMalloc(&b->devp, b->hp.size() * 4));
        b->devp_floats = b->hp.size();
    }
    if (!b->hp.empty()) HIPCHK(h, hipMemcpy(b->devp, b->hp.data(), b->hp.size() * 4, hipMemcpyHostToDevice));
    b->serial = h->stage_serial;
    return DPK_OK;
}

// dpk_diff_loss_grad once its arguments have passed: noising, the training forward, the loss, the backward
static int bwd_run(dpk_handle* h, const float* x0, const float* t, const StartSpec& spec, uint64_t seed, float weight,
                   float* loss, float* grads, int N, hipStream_t st) {
    BwdModel* b = h->bwd;
    GenModel* g = h->gen ? h->gen : b->own;
    const Stage& s = g->s;
    const Sched* sc = h->sched;
    const int D = s.D, E = s.E, J = s.J, L = s.L, M = N * J, cin = s.cin, cout = s.cout, pe = J * cin;
    float* S = nullptr;
    const size_t need = bwd_plan(s, N, nullptr).floats;
    int rc = gen_scratch(h, st, false, need, &S, "dpk_diff_loss_grad");
    if (rc) return rc;
    const BwdPlan p = bwd_plan(s, N, S);
    const float* W = g->dev;             // the forward's arena
    const float* WT = b->dev;            // the transposed arena
    const float* zero = WT + b->arena.zero;
    const GradLayout& gl = b->lay;
    const int n_cu = h->n_cu;
    const unsigned mask = h->mask;
    const unsigned* pmask = h->pmask;
    auto blocks = [](long long n) { return dim3(gen_blocks(n)); };
    auto fwd_gemm = [&](const float* a, int K, size_t w, size_t bias, float* c, int Nn, int mode) {
        bwd_gemm(b->fforms, st, n_cu, J, a, M, K, W + w, find_pack(g->packs, w, K, Nn), g->devp, W + bias, c, Nn, Nn, mode);
    };
    auto cheb = [&](const float* xin, int C, float* Z) {
        const size_t lds = ((size_t)J * C + 2 * J * J) * 4;
        b->fforms |= lds <= 65536 ? dpkg::F_CHEB_T : dpkg::F_CHEB_F;
        if (lds <= 65536)
            hipLaunchKernelGGL(dpkg::cheb_basis<true>, dim3((unsigned)N), dim3(256), lds, st, W + s.t1, W + s.t2, xin, Z, N, J, C);
        else
            hipLaunchKernelGGL(dpkg::cheb_basis<false>, blocks((long long)M * C), dim3(256), 0, st, W + s.t1, W + s.t2, xin, Z,
                               N, J, C);
    };
    // Y = Lm X with Lm the layer's Laplacian (forward) or its transpose (backward)
    auto graph = [&](const float* Lm, const float* xin, int C, float* yout, bool back) {
        const size_t lds = ((size_t)J * C + J * J) * 4;
        if (back) b->bforms |= lds <= 65536 ? dpkg::B_GRAPH_T_STAGED : dpkg::B_GRAPH_T_GLOBAL;
        else b->fforms |= lds <= 65536 ? dpkg::F_GRAPH_T : dpkg::F_GRAPH_F;
        if (lds <= 65536)
            hipLaunchKernelGGL(dpkg::graph<true>, dim3((unsigned)N), dim3(256), lds, st, Lm, xin, C, yout, C, N, J, C);
        else
            hipLaunchKernelGGL(dpkg::graph<false>, blocks((long long)M * C), dim3(256), 0, st, Lm, xin, C, yout, C, N, J, C);
    };
    auto copy = [&](float* dst, const float* src, size_t n) {
        return hipMemcpyAsync(dst, src, n * 4, hipMemcpyDeviceToDevice, st);
    };

    // ---- noising and the training forward
    gen_qsample_t(st, x0, p.xt, N, pe, t, sc->qtab, sc->nt, spec, seed);
    {
        const int half = D / 2;
        const float neg = -(float)(log(10000.0) / (double)(half - 1));
        hipLaunchKernelGGL(dpkg::temb_train, dim3((unsigned)N), dim3(256), (size_t)(D + 2 * E) * 4, st, W + s.d0w, W + s.d0b,
                           W + s.d1w, W + s.d1b, W + s.wtp, W + s.btp, t, D, E, L, neg, p.tproj, p.emb, p.u0, p.h0, p.u1,
                           p.h1);
    }
    cheb(p.xt, cin, p.Z0);
    fwd_gemm(p.Z0, 3 * cin, s.win, s.bin, p.lay.empty() ? p.Hlast : p.lay[0].H, D, dpkg::G_BIAS);
    for (int l = 0; l < L; ++l) {
        const GenLayer& o = s.lay[l];
        const BwdLayerBufs& y = p.lay[l];
        float* Hnext = l + 1 < L ? p.lay[l + 1].H : p.Hlast;
        hipLaunchKernelGGL(dpkg::layer_norm, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, y.H, y.Y0, M, D, W + o.n0a,
                           W + o.n0b);
        fwd_gemm(y.Y0, D, o.wqkv, o.bqkv, y.QKV, 3 * D, dpkg::G_BIAS);
        const bool avec = (D / s.H) % 4 == 0 && D % 8 == 0;      // every buffer of the plan is 256-byte aligned
        const size_t pose_bytes = (size_t)J * (3 * D + (avec ? 4 : 1)) * 4;
        const int ppb = std::max(1, std::min(256 / (s.H * J), (int)(65536 / pose_bytes)));
        const unsigned ab = (unsigned)((N + ppb - 1) / ppb);
        b->fforms |= pose_bytes > 65536 ? dpkg::F_ATTENTION_FF : avec ? dpkg::F_ATTENTION_TT : dpkg::F_ATTENTION_TF;
        if (pose_bytes > 65536)
            hipLaunchKernelGGL((dpkg::attention<false, false>), dim3((unsigned)N), dim3(256), 0, st, y.QKV, y.A, N, J, D, s.H,
                               mask, pmask, 1);
        else if (avec)
            hipLaunchKernelGGL((dpkg::attention<true, true>), dim3(ab), dim3(256), pose_bytes * ppb, st, y.QKV, y.A, N, J, D,
                               s.H, mask, pmask, ppb);
        else
            hipLaunchKernelGGL((dpkg::attention<true, false>), dim3(ab), dim3(256), pose_bytes * ppb, st, y.QKV, y.A, N, J, D,
                               s.H, mask, pmask, ppb);
        HIPCHK(h, copy(y.H1, y.H, (size_t)M * D));
        fwd_gemm(y.A, D, o.wo, o.bo, y.H1, D, dpkg::G_RESID);
        hipLaunchKernelGGL(dpkg::layer_norm, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, y.H1, y.Y1, M, D, W + o.n1a,
                           W + o.n1b);
        graph(W + o.lg, y.Y1, D, y.G1, false);
        fwd_gemm(y.G1, D, o.w1, o.b1, y.F, 2 * D, dpkg::G_RELU);
        graph(W + o.lg, y.F, 2 * D, y.G2, false);
        HIPCHK(h, copy(y.H2, y.H1, (size_t)M * D));
        fwd_gemm(y.G2, 2 * D, o.w2, o.b2, y.H2, D, dpkg::G_RESID);
        cheb(y.H2, D, y.Z1);
        fwd_gemm(y.Z1, 3 * D, o.wc1, o.bc1, y.R1, D, dpkg::G_RELU);
        hipLaunchKernelGGL(dpkg::add_temb, blocks((long long)M * D), dim3(256), 0, st, y.R1, p.tproj + (size_t)l * D, L * D,
                           p.C1, (long long)M * D, D, J);
        cheb(p.C1, D, y.Z2);
        fwd_gemm(y.Z2, 3 * D, o.wc2, o.bc2, y.R2, D, dpkg::G_RELU);
        hipLaunchKernelGGL(dpkg::add2, blocks((long long)M * D), dim3(256), 0, st, y.H2, y.R2, Hnext, (long long)M * D);
    }
    cheb(p.Hlast, D, p.Zout);
    fwd_gemm(p.Zout, 3 * D, s.wout, s.bout, p.eps, cout, dpkg::G_BIAS);
    if (loss) gen_diff_loss(st, p.eps, N, pe, spec, seed, loss);
    HIPCHK(h, hipGetLastError());

    // ---- the backward
    HIPCHK(h, hipMemsetAsync(grads, 0, gl.floats * 4, st));      // the padding between entries too
    // dW = A^T G over `rows` rows into the layout (see dw_reduce)
    auto dW = [&](const float* A, int lda, int rows, int K, const float* G, int ldg, int Nn, bool transpose, int Ns,
                  dpkg::DwDst dst) {
        const unsigned nslab = (unsigned)((rows + dpkg::DW_ROWS - 1) / dpkg::DW_ROWS);
        const size_t ps = (size_t)(K + 1) * Nn;
        auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
        const bool vec = K % 4 == 0 && Nn % 4 == 0 && lda % 4 == 0 && ldg % 4 == 0 && al16(A) && al16(G) && al16(p.Pdw);
        if (vec) {
            b->bforms |= dpkg::B_DW_VEC;
            const unsigned tiles = (unsigned)(((K + 63) / 64) * ((Nn + 63) / 64));
            hipLaunchKernelGGL(dpkg::dw_partial<true>, dim3(nslab, (tiles + 3) / 4), dim3(256), 0, st, A, lda, G, ldg, p.Pdw, ps,
                               rows, K, Nn);
        } else {
            b->bforms |= dpkg::B_DW_SCALAR;
            const unsigned tiles = (unsigned)(((K + 15) / 16) * ((Nn + 31) / 32));
            hipLaunchKernelGGL(dpkg::dw_partial<false>, dim3(nslab, (tiles + 3) / 4), dim3(256), 0, st, A, lda, G, ldg, p.Pdw,
                               ps, rows, K, Nn);
        }
        hipLaunchKernelGGL(dpkg::dw_reduce, blocks((long long)(K + 1) * Nn), dim3(256), 0, st, p.Pdw, ps, (int)nslab, K, Nn,
                           transpose ? 1 : 0, Ns, dst);
    };
    auto one = [&](size_t w, size_t bias) { return dpkg::DwDst{{grads + w, nullptr, nullptr}, {grads + bias, nullptr, nullptr}}; };
    // a vector's gradient: the column sums of G
    auto dvec = [&](const float* G, int rows, int Nn, size_t dst) {
        const unsigned nslab = (unsigned)((rows + dpkg::DW_ROWS - 1) / dpkg::DW_ROWS);
        hipLaunchKernelGGL(dpkg::colsum_partial, dim3(nslab, (unsigned)((Nn + 63) / 64)), dim3(256), 0, st, G, Nn, p.Pdw,
                           (size_t)Nn, (size_t)0, rows, Nn);
        hipLaunchKernelGGL(dpkg::dw_reduce, blocks(Nn), dim3(256), 0, st, p.Pdw, (size_t)Nn, (int)nslab, 0, Nn, 0, Nn,
                           dpkg::DwDst{{nullptr, nullptr, nullptr}, {grads + dst, nullptr, nullptr}});
    };
    // dA [rows][Kf] = G [rows][Nf] W^T for the forward block W [Kf][Nf] at arena offset w
    auto dX = [&](const float* G, int rows, int Nf, size_t w, int Kf, float* out) {
        bwd_gemm(b->fforms, st, n_cu, J, G, rows, Nf, WT + w, find_pack(b->packs, w, Nf, Kf), b->devp, zero, out, Kf, Kf,
                 dpkg::G_BIAS);
    };
    auto cheb_t = [&](const float* dZ, float* dXo, bool acc) {
        b->bforms |= dpkg::B_CHEB_T;
        hipLaunchKernelGGL(dpkg::cheb_t, blocks((long long)M * D), dim3(256), 0, st, W + s.t1, W + s.t2, dZ, dXo, N, J, D,
                           acc ? 1 : 0);
    };
    auto relu_bwd = [&](const float* dOut, const float* R, float* dPre, long long n) {
        hipLaunchKernelGGL(dpkg::relu_bwd, blocks(n), dim3(256), 0, st, dOut, R, dPre, n);
    };
    auto ln_bwd = [&](const float* X, const float* dY, size_t ga, size_t da, size_t db) {
        b->bforms |= dpkg::B_LN_BWD;
        hipLaunchKernelGGL(dpkg::ln_bwd, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, X, dY, W + ga, p.dH, p.tD1, M, D);
        dvec(p.tD1, M, D, da);
        dvec(dY, M, D, db);
    };
    const unsigned lgslabs = (unsigned)((N + dpkg::DLG_POSES - 1) / dpkg::DLG_POSES);
    auto dlg = [&](const float* dY, const float* X, int C, float* P) {
        const size_t lds = (size_t)2 * J * (C | 1) * 4;
        b->bforms |= lds <= 65536 ? dpkg::B_DLG_STAGED : dpkg::B_DLG_GLOBAL;
        if (lds <= 65536)
            hipLaunchKernelGGL(dpkg::dlg_partial<true>, dim3(lgslabs), dim3(256), lds, st, dY, X, P, N, J, C);
        else
            hipLaunchKernelGGL(dpkg::dlg_partial<false>, dim3(lgslabs), dim3(256), 0, st, dY, X, P, N, J, C);
    };
    const long long MD = (long long)M * D;

    hipLaunchKernelGGL(dpkg::loss_grad, blocks((long long)M * cout), dim3(256), 0, st, p.eps, (long long)M * cout, pe,
                       spec.scale, spec.rows, spec.noise, (unsigned long long)seed, weight, p.dEps);
    dW(p.Zout, 3 * D, M, 3 * D, p.dEps, cout, cout, false, cout, one(gl.wout, gl.bout));
    dX(p.dEps, M, cout, s.wout, 3 * D, p.t3D);
    cheb_t(p.t3D, p.dH, false);
    for (int l = L - 1; l >= 0; --l) {
        const GenLayer& o = s.lay[l];
        const BwdLayerBufs& y = p.lay[l];
        const GradLayer& q = gl.lay[l];
        // H3 = H2 + relu(Z2 Wc2 + bc2)
        relu_bwd(p.dH, y.R2, p.tD1, MD);
        dW(y.Z2, 3 * D, M, 3 * D, p.tD1, D, D, false, D, one(q.c2w, q.c2b));
        dX(p.tD1, M, D, o.wc2, 3 * D, p.t3D);
        cheb_t(p.t3D, p.tD2, false);                 // dC1
        // C1 = relu(Z1 Wc1 + bc1) + temb_proj_l
        hipLaunchKernelGGL(dpkg::joint_sum, blocks((long long)N * D), dim3(256), 0, st, p.tD2, p.dtp + (size_t)l * D, L * D, N,
                           J, D);
        relu_bwd(p.tD2, y.R1, p.tD1, MD);
        dW(y.Z1, 3 * D, M, 3 * D, p.tD1, D, D, false, D, one(q.c1w, q.c1b));
        dX(p.tD1, M, D, o.wc1, 3 * D, p.t3D);
        cheb_t(p.t3D, p.dH, true);                   // dH2
        // H2 = H1 + (L_g relu((L_g Y1) W1 + b1)) W2 + b2
        dW(y.G2, 2 * D, M, 2 * D, p.dH, D, D, true, D, one(q.f2w, q.f2b));
        dX(p.dH, M, D, o.w2, 2 * D, p.t2Da);         // dG2
        dlg(p.t2Da, y.F, 2 * D, p.Plg + (size_t)lgslabs * J * J);
        graph(WT + o.lg, p.t2Da, 2 * D, p.t2Db, true);    // dF
        relu_bwd(p.t2Db, y.F, p.t2Da, 2 * MD);
        dW(y.G1, D, M, D, p.t2Da, 2 * D, 2 * D, true, 2 * D, one(q.f1w, q.f1b));
        dX(p.t2Da, M, 2 * D, o.w1, D, p.tD1);        // dG1
        dlg(p.tD1, y.Y1, D, p.Plg);
        graph(WT + o.lg, p.tD1, D, p.tD2, true);     // dY1
        hipLaunchKernelGGL(dpkg::dlg_chain, dim3(1), dim3(256), (size_t)(J * J + 2 * J) * 4, st, p.Plg, (int)(2 * lgslabs),
                           WT + b->arena.ahat + (size_t)l * b->arena.jj4, grads + q.ahat, J);
        ln_bwd(y.H1, p.tD2, o.n1a, q.n1a, q.n1b);
        // H1 = H + attention(LN0(H)) Wo + bo
        dW(y.A, D, M, D, p.dH, D, D, true, D, one(q.lw[3], q.lb[3]));
        dX(p.dH, M, D, o.wo, D, p.tD1);              // dA
        {
            const int hb = std::max(1, std::min(std::min(s.H, 256 / J), 4096 / (J * J)));
            const size_t ps_lds = (size_t)2 * hb * J * J * 4, staged = ps_lds + (size_t)J * ((4 * D) | 1) * 4;
            const bool stage = staged <= 65536;
            b->bforms |= stage ? dpkg::B_ATTN_BWD_STAGED : dpkg::B_ATTN_BWD_GLOBAL;
            hipLaunchKernelGGL(dpkg::attention_bwd, dim3((unsigned)N), dim3(256), stage ? staged : ps_lds, st, y.QKV, p.tD1,
                               p.t3D, J, D, s.H, mask, pmask, hb, stage ? 1 : 0);
        }
        dW(y.Y0, D, M, D, p.t3D, 3 * D, 3 * D, true, D,
           dpkg::DwDst{{grads + q.lw[0], grads + q.lw[1], grads + q.lw[2]}, {grads + q.lb[0], grads + q.lb[1], grads + q.lb[2]}});
        dX(p.t3D, M, 3 * D, o.wqkv, D, p.tD2);       // dY0
        ln_bwd(y.H, p.tD2, o.n0a, q.n0a, q.n0b);
    }
    dW(p.Z0, 3 * cin, M, 3 * cin, p.dH, D, D, false, D, one(gl.win, gl.bin));
    // the timestep MLP, per pose: tproj_l = h1 WP_l + bp_l, h1 = swish(u1), u1 = h0 W1 + b1, h0 = swish(u0), u0 = emb W0 + b0
    b->bforms |= dpkg::B_TEMB_BWD;
    for (int l = 0; l < L; ++l)
        dW(p.h1, E, N, E, p.dtp + (size_t)l * D, L * D, D, true, D, one(gl.lay[l].tpw, gl.lay[l].tpb));
    bwd_gemm(b->fforms, st, n_cu, J, p.dtp, N, L * D, WT + s.wtp, nullptr, nullptr, zero, p.dh, E, E, dpkg::G_BIAS);
    hipLaunchKernelGGL(dpkg::swish_bwd, blocks((long long)N * E), dim3(256), 0, st, p.dh, p.u1, p.du, (long long)N * E);
    dW(p.h0, E, N, E, p.du, E, E, true, E, one(gl.d1w, gl.d1b));
    dX(p.du, N, E, s.d1w, E, p.dh);
    hipLaunchKernelGGL(dpkg::swish_bwd, blocks((long long)N * E), dim3(256), 0, st, p.dh, p.u0, p.du, (long long)N * E);
    dW(p.emb, D, N, D, p.du, E, E, true, E, one(gl.d0w, gl.d0b));
    HIPCHK(h, hipGetLastError());
    return DPK_OK;
}
