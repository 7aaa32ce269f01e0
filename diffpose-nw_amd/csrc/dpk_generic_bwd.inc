// dpk_generic_bwd.inc — the gradient of the denoising objective (dpk_diff_loss_grad) on the per-op path: the
// forward of dpk_generic.inc run once more with what the backward needs kept in the call's scratch, then the
// backward as per-op HIP kernels, fp32 throughout; eval mode, or train mode (dpk_diff_loss_grad_train: dropout at the
// reference's five sites per layer, counter-based masks recomputed where they are read).  Included by dpk_kernels.hip after
// dpk_generic.inc and dpk_grad_layout.inc; forms, grids and LDS sizes come from dpk_genplan.inc.
//   training forward  gen_forward's ops (GenOps: the same kernels and form choices, out of place), every GEMM operand,
//                     ReLU output and residual-stream value of every layer stored (bwd_plan: the stash)
//   dX GEMMs          dA = dC W^T, GenOps::gemm against the transposed arena (BwdArena)
//   dW GEMMs          dW = A^T dC: dw_partial, one [K][N] slab per DW_ROWS rows on v_mfma_f32_16x16x4_f32, the bias
//                     gradient (column sums) as row K of the slab; dw_reduce adds the slabs in
//                     ascending order and writes the torch layout (transposed for nn.Linear, QKV split in three)
//   the rest          plain-VALU kernels: ln_bwd, attention_bwd, graph on L_g^T, dlg_partial + dlg_chain (to A_hat),
//                     cheb_t, relu_bwd, joint_sum, swish_bwd, loss_grad
//   train mode        attention_train / attention_bwd_train, drop_apply (dpk_generic.inc), relu_drop_bwd: launched
//                     only at a site whose rate is not 0, in place of or beside the eval-mode launches (bwd_run)
// Every sum over rows or poses is a store pass of partials over a fixed partition (DW_ROWS rows, DLG_POSES poses)
// and an ordered sum pass: no float atomics, so the same call gives bitwise the same gradients.

namespace dpkg {

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
// TRAIN (attention_bwd_train; the eval-mode kernel is the body without it): the forward dropped probabilities of site
// `drop`, element ((pose0 + p) H + h) J J + q J + j, factor f = s or 0 recomputed from the counter: dP_j = (dO . V_j) f_j,
// dS from the unmasked p as above, and P f in LDS for pass 2's dV.
template <bool TRAIN>
__device__ __forceinline__ void attention_bwd_body(const float* __restrict__ qkv, const float* __restrict__ dO,
                                                   float* __restrict__ dqkv, int J, int D, int H, unsigned mask,
                                                   const unsigned* __restrict__ pmask, int hb, int stage,
                                                   const DropSite& drop, long long pose0) {
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
            const long long i0 = (((pose0 + p) * H + h) * J + q) * J;
            DropRow row;
            for (int j = 0; j < J; ++j) {
                const float pj = pr[j] / sum;
                pr[j] = pj;
                const float* vr = rows + j * RS + 2 * D + h * dk;
                float dp = 0.f;
                for (int d = 0; d < dk; ++d) dp = fmaf(go[d], vr[d], dp);
                if constexpr (TRAIN) dp *= row.factor(drop, i0 + j);
                sr[j] = dp;
                dot = fmaf(pj, dp, dot);
            }
            for (int j = 0; j < J; ++j) {
                sr[j] = ((m >> j) & 1u) ? pr[j] * (sr[j] - dot) / sq : 0.f;
                if constexpr (TRAIN) pr[j] *= row.factor(drop, i0 + j);
            }
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
__global__ void __launch_bounds__(256) attention_bwd(const float* __restrict__ qkv, const float* __restrict__ dO,
                                                     float* __restrict__ dqkv, int J, int D, int H, unsigned mask,
                                                     const unsigned* __restrict__ pmask, int hb, int stage) {
    attention_bwd_body<false>(qkv, dO, dqkv, J, D, H, mask, pmask, hb, stage, DropSite{}, 0);
}
__global__ void __launch_bounds__(256) attention_bwd_train(const float* __restrict__ qkv, const float* __restrict__ dO,
                                                           float* __restrict__ dqkv, int J, int D, int H, unsigned mask,
                                                           const unsigned* __restrict__ pmask, int hb, int stage,
                                                           DropSite drop, long long pose0) {
    attention_bwd_body<true>(qkv, dO, dqkv, J, D, H, mask, pmask, hb, stage, drop, pose0);
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
// relu_bwd behind a dropout of rate p on the ReLU output (R stored dropped and scaled: R > 0 is "positive and kept")
__global__ void __launch_bounds__(256) relu_drop_bwd(const float* __restrict__ dOut, const float* __restrict__ R,
                                                     float* __restrict__ dPre, long long n, float s) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dPre[i] = R[i] > 0.f ? dOut[i] * s : 0.f;
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

}  // namespace dpkg

// ---------------------------------------------------------------------------------------
// Host side

// What a handle keeps for dpk_diff_loss_grad, built on its first call and again after new weights or a new graph
struct BwdModel {
    GenModel* own = nullptr;     // a persistent-sampler handle's per-op model (a per-op handle uses its own)
    GradLayout lay;
    BwdArena arena;
    GemmArena dev;               // the transposed arena on the device, with the gemm_sk copies of its GEMM blocks
    uint64_t serial = 0;         // dpk_handle::stage_serial it was built from (0: never)
    unsigned fforms = 0, bforms = 0;   // GenForm bits of the forward and dX launches; BwdForm bits
};

static void bwd_free(BwdModel* b) {
    if (!b) return;
    gen_free(b->own);
    b->dev.free();
    delete b;
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
    std::vector<PackBlock> blocks;       // the transposed block is [N][K] of the forward's
    for (const BwdBlock& k : b->arena.blocks) blocks.push_back({k.w, k.N, k.K});
    const int rc = b->dev.upload(h, b->arena.h.data(), b->arena.floats, blocks);
    if (rc) return rc;
    b->serial = h->stage_serial;
    return DPK_OK;
}

// The dropout of one train-mode call (dpk_diff_loss_grad_train): the three rates, the seed and the global index of
// the call's first pose.  All rates 0 (the default): dpk_diff_loss_grad's launches, every one.
struct DropRun {
    float sublayer = 0.f, attn = 0.f, gconv = 0.f;
    uint64_t seed = 0;
    long long pose0 = 0;
    // thr = ceil(p 2^24) (the product is exact), s = 1 / (1 - p) in fp32, both taken here on the host
    dpkg::DropSite site(int layer, int id) const {
        const float p = id == dpkg::DROP_ATTN ? attn : id == dpkg::DROP_SUB0 || id == dpkg::DROP_SUB1 ? sublayer : gconv;
        dpkg::DropSite d;
        d.thr = (unsigned)ceilf(p * 16777216.0f);
        d.s = d.thr ? 1.0f / (1.0f - p) : 1.0f;
        d.dom = (unsigned)(layer * 8 + id);
        d.k0 = (unsigned)seed;
        d.k1 = (unsigned)(seed >> 32);
        return d;
    }
};

// dpk_diff_loss_grad(_train) once its arguments have passed: noising, the training forward, the loss, the backward
static int bwd_run(dpk_handle* h, const float* x0, const float* t, const StartSpec& spec, uint64_t seed, float weight,
                   float* loss, float* grads, int N, hipStream_t st, const DropRun& dr) {
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
    const GemmArena& ar = g->arena;      // the forward's arena
    const float* W = ar.dev;
    const float* WT = b->dev.dev;        // the transposed arena
    const float* zero = WT + b->arena.zero;
    const GradLayout& gl = b->lay;
    const GenOps op(g, st, N, h->mask, h->pmask, h->n_cu, b->fforms);
    auto blocks = [](long long n) { return dim3(gen_blocks(n)); };
    auto copy = [&](float* dst, const float* src, size_t n) {
        return hipMemcpyAsync(dst, src, n * 4, hipMemcpyDeviceToDevice, st);
    };

    // ---- noising and the training forward: gen_forward's ops, to be read beside it.  The two sequences stay two:
    // this one keeps every intermediate in a buffer of its own and leaves relu + temb and resid + relu out of the
    // GEMM epilogues (add_temb, add2), since the backward reads R1 and R2.
    gen_qsample_t(st, x0, p.xt, N, pe, t, sc->qtab, sc->nt, spec, seed);
    const dpkg::TembStash keep{p.emb, p.u0, p.h0, p.u1, p.h1};
    op.temb(t, 1, N, p.tproj, &keep);
    op.cheb(p.xt, cin, p.Z0);
    op.gemm(ar, p.Z0, M, 3 * cin, s.win, W + s.bin, p.lay.empty() ? p.Hlast : p.lay[0].H, D, D, dpkg::G_BIAS);
    // Train mode (dr): the five dropout sites of a layer fall on those seams.  p_attn is dropped inside
    // attention_train; a sublayer's GEMM writes its branch alone (G_BIAS) and drop_apply<true> adds the residual to the
    // dropped branch in place; a ChebConv's ReLU output is dropped in place, so R1 and R2 are stored masked and scaled.
    // A site whose rate is 0 runs the eval-mode launches.
    const long long MD = (long long)M * D, base = dr.pose0 * J * D;      // a [N, J, hid] site's elements of this call
    for (int l = 0; l < L; ++l) {
        const GenLayer& o = s.lay[l];
        const BwdLayerBufs& y = p.lay[l];
        float* Hnext = l + 1 < L ? p.lay[l + 1].H : p.Hlast;
        const dpkg::DropSite att = dr.site(l, dpkg::DROP_ATTN), sub0 = dr.site(l, dpkg::DROP_SUB0),
                             sub1 = dr.site(l, dpkg::DROP_SUB1), gc1 = dr.site(l, dpkg::DROP_GC1),
                             gc2 = dr.site(l, dpkg::DROP_GC2);
        if (att.thr) b->bforms |= dpkg::B_ATTN_TRAIN;
        if (sub0.thr || sub1.thr) b->bforms |= dpkg::B_DROP_ADD;
        if (gc1.thr || gc2.thr) b->bforms |= dpkg::B_RELU_DROP;
        op.layer_norm(y.H, y.Y0, o.n0a, o.n0b);
        op.gemm(ar, y.Y0, M, D, o.wqkv, W + o.bqkv, y.QKV, 3 * D, 3 * D, dpkg::G_BIAS);
        if (att.thr) op.attention_train(y.QKV, y.A, att, dr.pose0);
        else op.attention(y.QKV, y.A);
        if (sub0.thr) {
            op.gemm(ar, y.A, M, D, o.wo, W + o.bo, y.H1, D, D, dpkg::G_BIAS);
            op.drop(y.H, y.H1, y.H1, MD, base, sub0);
        } else {
            HIPCHK(h, copy(y.H1, y.H, (size_t)M * D));
            op.gemm(ar, y.A, M, D, o.wo, W + o.bo, y.H1, D, D, dpkg::G_RESID);
        }
        op.layer_norm(y.H1, y.Y1, o.n1a, o.n1b);
        op.graph(W + o.lg, y.Y1, D, y.G1);
        op.gemm(ar, y.G1, M, D, o.w1, W + o.b1, y.F, 2 * D, 2 * D, dpkg::G_RELU);
        op.graph(W + o.lg, y.F, 2 * D, y.G2);
        if (sub1.thr) {
            op.gemm(ar, y.G2, M, 2 * D, o.w2, W + o.b2, y.H2, D, D, dpkg::G_BIAS);
            op.drop(y.H1, y.H2, y.H2, MD, base, sub1);
        } else {
            HIPCHK(h, copy(y.H2, y.H1, (size_t)M * D));
            op.gemm(ar, y.G2, M, 2 * D, o.w2, W + o.b2, y.H2, D, D, dpkg::G_RESID);
        }
        op.cheb(y.H2, D, y.Z1);
        op.gemm(ar, y.Z1, M, 3 * D, o.wc1, W + o.bc1, y.R1, D, D, dpkg::G_RELU);
        if (gc1.thr) op.drop(nullptr, y.R1, y.R1, MD, base, gc1);
        hipLaunchKernelGGL(dpkg::add_temb, blocks((long long)M * D), dim3(256), 0, st, y.R1, p.tproj + (size_t)l * D, L * D,
                           p.C1, (long long)M * D, D, J);
        op.cheb(p.C1, D, y.Z2);
        op.gemm(ar, y.Z2, M, 3 * D, o.wc2, W + o.bc2, y.R2, D, D, dpkg::G_RELU);
        if (gc2.thr) op.drop(nullptr, y.R2, y.R2, MD, base, gc2);
        hipLaunchKernelGGL(dpkg::add2, blocks((long long)M * D), dim3(256), 0, st, y.H2, y.R2, Hnext, (long long)M * D);
    }
    op.cheb(p.Hlast, D, p.Zout);
    op.gemm(ar, p.Zout, M, 3 * D, s.wout, W + s.bout, p.eps, cout, cout, dpkg::G_BIAS);
    if (loss) gen_diff_loss(st, p.eps, N, pe, spec, seed, loss);
    HIPCHK(h, hipGetLastError());

    // ---- the backward
    HIPCHK(h, hipMemsetAsync(grads, 0, gl.floats * 4, st));      // the padding between entries too
    // dW = A^T G over `rows` rows into the layout (see dw_reduce)
    auto dW = [&](const float* A, int lda, int rows, int K, const float* G, int ldg, int Nn, bool transpose, int Ns,
                  dpkg::DwDst dst) {
        const auto at = [](const void* q) { return reinterpret_cast<uintptr_t>(q); };
        const DwChoice d = dw_choice(rows, K, Nn, lda, ldg, at(A), at(G), at(p.Pdw));
        b->bforms |= d.vec ? dpkg::B_DW_VEC : dpkg::B_DW_SCALAR;
        auto* kernel = d.vec ? dpkg::dw_partial<true> : dpkg::dw_partial<false>;
        hipLaunchKernelGGL(kernel, dim3(d.nslab, d.gy), dim3(256), 0, st, A, lda, G, ldg, p.Pdw, d.ps, rows, K, Nn);
        hipLaunchKernelGGL(dpkg::dw_reduce, blocks((long long)(K + 1) * Nn), dim3(256), 0, st, p.Pdw, d.ps, (int)d.nslab, K, Nn,
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
        op.gemm(b->dev, G, rows, Nf, w, zero, out, Kf, Kf, dpkg::G_BIAS);
    };
    auto cheb_t = [&](const float* dZ, float* dXo, bool acc) {
        b->bforms |= dpkg::B_CHEB_T;
        hipLaunchKernelGGL(dpkg::cheb_t, blocks((long long)M * D), dim3(256), 0, st, W + s.t1, W + s.t2, dZ, dXo, N, J, D,
                           acc ? 1 : 0);
    };
    auto relu_bwd = [&](const float* dOut, const float* R, float* dPre, long long n) {
        hipLaunchKernelGGL(dpkg::relu_bwd, blocks(n), dim3(256), 0, st, dOut, R, dPre, n);
    };
    // behind a ChebConv's dropout (R stored dropped and scaled), or relu_bwd where the site is off
    auto relu_drop_bwd = [&](const float* dOut, const float* R, float* dPre, const dpkg::DropSite& d) {
        if (!d.thr) return relu_bwd(dOut, R, dPre, MD);
        hipLaunchKernelGGL(dpkg::relu_drop_bwd, blocks(MD), dim3(256), 0, st, dOut, R, dPre, MD, d.s);
    };
    auto ln_bwd = [&](const float* X, const float* dY, size_t ga, size_t da, size_t db) {
        b->bforms |= dpkg::B_LN_BWD;
        hipLaunchKernelGGL(dpkg::ln_bwd, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, X, dY, W + ga, p.dH, p.tD1, M, D);
        dvec(p.tD1, M, D, da);
        dvec(dY, M, D, db);
    };
    const unsigned lgslabs = dlg_choice(N, J, D).blocks;
    auto dlg = [&](const float* dY, const float* X, int C, float* P) {
        const StageChoice c = dlg_choice(N, J, C);
        b->bforms |= c.stage ? dpkg::B_DLG_STAGED : dpkg::B_DLG_GLOBAL;
        auto* kernel = c.stage ? dpkg::dlg_partial<true> : dpkg::dlg_partial<false>;
        hipLaunchKernelGGL(kernel, dim3(c.blocks), dim3(256), c.lds, st, dY, X, P, N, J, C);
    };

    hipLaunchKernelGGL(dpkg::loss_grad, blocks((long long)M * cout), dim3(256), 0, st, p.eps, (long long)M * cout, pe,
                       spec.scale, spec.rows, spec.noise, (unsigned long long)seed, weight, p.dEps);
    dW(p.Zout, 3 * D, M, 3 * D, p.dEps, cout, cout, false, cout, one(gl.wout, gl.bout));
    dX(p.dEps, M, cout, s.wout, 3 * D, p.t3D);
    cheb_t(p.t3D, p.dH, false);
    for (int l = L - 1; l >= 0; --l) {
        const GenLayer& o = s.lay[l];
        const BwdLayerBufs& y = p.lay[l];
        const GradLayer& q = gl.lay[l];
        const dpkg::DropSite att = dr.site(l, dpkg::DROP_ATTN), sub0 = dr.site(l, dpkg::DROP_SUB0),
                             sub1 = dr.site(l, dpkg::DROP_SUB1);
        // H3 = H2 + drop(relu(Z2 Wc2 + bc2))
        relu_drop_bwd(p.dH, y.R2, p.tD1, dr.site(l, dpkg::DROP_GC2));
        dW(y.Z2, 3 * D, M, 3 * D, p.tD1, D, D, false, D, one(q.c2w, q.c2b));
        dX(p.tD1, M, D, o.wc2, 3 * D, p.t3D);
        cheb_t(p.t3D, p.tD2, false);                 // dC1
        // C1 = relu(Z1 Wc1 + bc1) + temb_proj_l
        hipLaunchKernelGGL(dpkg::joint_sum, blocks((long long)N * D), dim3(256), 0, st, p.tD2, p.dtp + (size_t)l * D, L * D, N,
                           J, D);
        relu_drop_bwd(p.tD2, y.R1, p.tD1, dr.site(l, dpkg::DROP_GC1));
        dW(y.Z1, 3 * D, M, 3 * D, p.tD1, D, D, false, D, one(q.c1w, q.c1b));
        dX(p.tD1, M, D, o.wc1, 3 * D, p.t3D);
        cheb_t(p.t3D, p.dH, true);                   // dH2
        // H2 = H1 + (L_g relu((L_g Y1) W1 + b1)) W2 + b2
        // (train mode: the branch's gradient is drop(dH2), into tD1, free here; the residual path keeps dH)
        const float* dB1 = p.dH;
        if (sub1.thr) op.drop(nullptr, p.dH, p.tD1, MD, base, sub1), dB1 = p.tD1;
        dW(y.G2, 2 * D, M, 2 * D, dB1, D, D, true, D, one(q.f2w, q.f2b));
        dX(dB1, M, D, o.w2, 2 * D, p.t2Da);          // dG2
        dlg(p.t2Da, y.F, 2 * D, p.Plg + (size_t)lgslabs * J * J);
        op.graph(WT + o.lg, p.t2Da, 2 * D, p.t2Db, &b->bforms);    // dF
        relu_bwd(p.t2Db, y.F, p.t2Da, 2 * MD);
        dW(y.G1, D, M, D, p.t2Da, 2 * D, 2 * D, true, 2 * D, one(q.f1w, q.f1b));
        dX(p.t2Da, M, 2 * D, o.w1, D, p.tD1);        // dG1
        dlg(p.tD1, y.Y1, D, p.Plg);
        op.graph(WT + o.lg, p.tD1, D, p.tD2, &b->bforms);     // dY1
        hipLaunchKernelGGL(dpkg::dlg_chain, dim3(1), dim3(256), (size_t)(J * J + 2 * J) * 4, st, p.Plg, (int)(2 * lgslabs),
                           WT + b->arena.ahat + (size_t)l * b->arena.jj4, grads + q.ahat, J);
        ln_bwd(y.H1, p.tD2, o.n1a, q.n1a, q.n1b);
        // H1 = H + attention(LN0(H)) Wo + bo
        // (train mode: drop(dH1) into tD2, free after ln_bwd)
        const float* dB0 = p.dH;
        if (sub0.thr) op.drop(nullptr, p.dH, p.tD2, MD, base, sub0), dB0 = p.tD2;
        dW(y.A, D, M, D, dB0, D, D, true, D, one(q.lw[3], q.lb[3]));
        dX(dB0, M, D, o.wo, D, p.tD1);               // dA
        {
            const AttnBwdChoice a = attention_bwd_choice(J, D, s.H);
            b->bforms |= a.stage ? dpkg::B_ATTN_BWD_STAGED : dpkg::B_ATTN_BWD_GLOBAL;
            if (att.thr)
                hipLaunchKernelGGL(dpkg::attention_bwd_train, dim3((unsigned)N), dim3(256), a.lds, st, y.QKV, p.tD1, p.t3D, J,
                                   D, s.H, h->mask, h->pmask, a.hb, a.stage ? 1 : 0, att, dr.pose0);
            else
                hipLaunchKernelGGL(dpkg::attention_bwd, dim3((unsigned)N), dim3(256), a.lds, st, y.QKV, p.tD1, p.t3D, J, D,
                                   s.H, h->mask, h->pmask, a.hb, a.stage ? 1 : 0);
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
    op.gemm(b->dev, p.dtp, N, L * D, s.wtp, zero, p.dh, E, E, dpkg::G_BIAS, nullptr, 0, false);
    hipLaunchKernelGGL(dpkg::swish_bwd, blocks((long long)N * E), dim3(256), 0, st, p.dh, p.u1, p.du, (long long)N * E);
    dW(p.h0, E, N, E, p.du, E, E, true, E, one(gl.d1w, gl.d1b));
    dX(p.du, N, E, s.d1w, E, p.dh);
    hipLaunchKernelGGL(dpkg::swish_bwd, blocks((long long)N * E), dim3(256), 0, st, p.dh, p.u0, p.du, (long long)N * E);
    dW(p.emb, D, N, D, p.du, E, E, true, E, one(gl.d0w, gl.d0b));
    HIPCHK(h, hipGetLastError());
    return DPK_OK;
}
