// dpk_train_layout.inc — the host description of dpk_train_apply's refresh: for every float of the four arenas the
// per-op forward and backward read (the forward arena, its gemm_sk copies, the transposed arena, its gemm_sk copies),
// where it comes from in the flat parameter array (dpk_param_layout: state_dict order, torch layouts).  One int32 per
// destination float:
//   >= 0           that index of the flat array (a copy; stage_load's transposes are in the index)
//   TRAIN_KEEP     not derived from the parameters, left as it is: the Chebyshev terms, the zero row, and the padding
//                  (between blocks, outside K x N of a gemm_sk copy, behind an A_hat row), which is zero and stays zero
//   <= TRAIN_LG    element e = TRAIN_LG - code of the GraphNet Laplacians [L][J][J]: computed from that layer's A_hat
//                  (train_lg below, stage_load's order), wherever the element stands (transposed, in fragment order)
// The per-float form rather than a block table: one gather kernel serves all four arenas, and the fragment order of
// the gemm_sk copies needs no second description on the device.  Plain C++ after dpk_stage.inc, dpk_genplan.inc and
// dpk_grad_layout.inc (tests/c/dpk_train_layout_check.cpp compiles them alone).

#include <stdio.h>
#include <stdlib.h>

constexpr int32_t TRAIN_KEEP = -1;
constexpr int32_t TRAIN_LG = -2;

struct TrainLayout {
    size_t F = 0;                            // the flat array's extent in floats
    int J = 0, L = 0;
    std::vector<int32_t> fwd, fwdp, bwd, bwdp;   // the four arenas' sources
    std::vector<int32_t> ahat;               // each layer's A_hat in the flat array
};

// dst [K][N] (row stride ldd) of `idx` from the flat block at src: [K][N] as it is, or (trans) torch's (N, K)
static void train_block(std::vector<int32_t>& idx, size_t dst, size_t src, int K, int N, int ldd, bool trans) {
    for (int k = 0; k < K; ++k)
        for (int n = 0; n < N; ++n)
            idx[dst + (size_t)k * ldd + n] = (int32_t)(src + (trans ? (size_t)n * K + k : (size_t)k * N + n));
}
// pack_fill on sources: the gemm_sk copies of `arena`'s blocks
static void train_pack(const std::vector<GenPack>& packs, const std::vector<int32_t>& arena, size_t floats,
                       std::vector<int32_t>& out) {
    out.assign(floats, TRAIN_KEEP);
    for (const GenPack& p : packs) {
        const int KC = (p.K + 15) / 16, NT16 = (p.N + 15) / 16, NTp = pack_ntp(p.N, p.NJ);
        for (int c = 0; c < KC; ++c)
            for (int t = 0; t < NT16; ++t)
                for (int l = 0; l < 64; ++l)
                    for (int q = 0; q < 4; ++q) {
                        const int k = 16 * c + 4 * (l >> 4) + q, n = 16 * t + (l & 15);
                        if (k < p.K && n < p.N)
                            out[p.off + (((size_t)c * NTp + t) * 64 + l) * 4 + q] = arena[p.w + (size_t)k * p.N + n];
                    }
    }
}

static TrainLayout train_layout(const Stage& s) {
    TrainLayout t;
    const GradLayout g = grad_layout(s);
    const int D = s.D, E = s.E, J = s.J, L = s.L;
    t.F = g.floats, t.J = J, t.L = L;
    // ---- the forward arena: stage_load
    t.fwd.assign(s.floats, TRAIN_KEEP);
    std::vector<int32_t>& f = t.fwd;
    for (int l = 0; l < L; ++l) {
        const GenLayer& o = s.lay[l];
        const GradLayer& y = g.lay[l];
        for (int j = 0; j < 3; ++j) {            // [in][q | k | v]
            train_block(f, o.wqkv + (size_t)j * D, y.lw[j], D, D, 3 * D, true);
            train_block(f, o.bqkv + (size_t)j * D, y.lb[j], 1, D, D, false);
        }
        train_block(f, o.wo, y.lw[3], D, D, D, true), train_block(f, o.bo, y.lb[3], 1, D, D, false);
        train_block(f, o.w1, y.f1w, D, 2 * D, 2 * D, true), train_block(f, o.b1, y.f1b, 1, 2 * D, 2 * D, false);
        train_block(f, o.w2, y.f2w, 2 * D, D, D, true), train_block(f, o.b2, y.f2b, 1, D, D, false);
        train_block(f, o.wc1, y.c1w, 3 * D, D, D, false), train_block(f, o.bc1, y.c1b, 1, D, D, false);
        train_block(f, o.wc2, y.c2w, 3 * D, D, D, false), train_block(f, o.bc2, y.c2b, 1, D, D, false);
        train_block(f, o.n0a, y.n0a, 1, D, D, false), train_block(f, o.n0b, y.n0b, 1, D, D, false);
        train_block(f, o.n1a, y.n1a, 1, D, D, false), train_block(f, o.n1b, y.n1b, 1, D, D, false);
        for (int e = 0; e < J * J; ++e) f[o.lg + e] = TRAIN_LG - (int32_t)(l * J * J + e);
        train_block(f, s.wtp + (size_t)l * E * D, y.tpw, E, D, D, true);
        train_block(f, s.btp + (size_t)l * D, y.tpb, 1, D, D, false);
        t.ahat.push_back((int32_t)y.ahat);
    }
    train_block(f, s.win, g.win, 3 * s.cin, D, D, false), train_block(f, s.bin, g.bin, 1, D, D, false);
    train_block(f, s.wout, g.wout, 3 * D, s.cout, s.cout, false), train_block(f, s.bout, g.bout, 1, s.cout, s.cout, false);
    train_block(f, s.d0w, g.d0w, D, E, E, true), train_block(f, s.d0b, g.d0b, 1, E, E, false);
    train_block(f, s.d1w, g.d1w, E, E, E, true), train_block(f, s.d1b, g.d1b, 1, E, E, false);
    // ---- its gemm_sk copies
    std::vector<GenPack> packs;
    const size_t pf = pack_plan(gen_pack_blocks(s), packs);
    train_pack(packs, t.fwd, pf, t.fwdp);
    // ---- the transposed arena: bwd_arena_build
    BwdArena a;
    bwd_arena_build(s, a);                       // for its offsets
    t.bwd.assign(a.floats, TRAIN_KEEP);
    std::copy(t.fwd.begin(), t.fwd.end(), t.bwd.begin());
    for (const BwdBlock& b : a.blocks)
        for (int k = 0; k < b.K; ++k)
            for (int n = 0; n < b.N; ++n) t.bwd[b.w + (size_t)n * b.K + k] = t.fwd[b.w + (size_t)k * b.N + n];
    for (int l = 0; l < L; ++l)
        for (int e = 0; e < J * J; ++e) t.bwd[a.ahat + (size_t)l * a.jj4 + e] = t.ahat[l] + e;
    // ---- and its copies
    std::vector<PackBlock> tb;
    for (const BwdBlock& k : a.blocks) tb.push_back({k.w, k.N, k.K});
    const size_t pb = pack_plan(tb, packs);
    train_pack(packs, t.bwd, pb, t.bwdp);
    return t;
}

// Element (i, j) of a layer's GraphNet Laplacian from its A_hat [J][J], stage_load's operations in its order: column
// sums over the rows ascending in fp32, d = 1 / sqrtf(sum + 1e-5f), (d_i a_ij) d_j.  (The refresh kernel is this
// function on the device; division and square root are correctly rounded on both.)
static inline float train_lg(const float* ahat, int J, int i, int j) {
    float ri = 0.f, rj = 0.f;
    for (int k = 0; k < J; ++k) ri += ahat[k * J + i], rj += ahat[k * J + j];
    const float di = 1.0f / sqrtf(ri + 1e-5f), dj = 1.0f / sqrtf(rj + 1e-5f);
    return (di * ahat[i * J + j]) * dj;
}
// One arena refreshed on the host: what the refresh kernel does to each of the four
static void train_gather(const TrainLayout& t, const std::vector<int32_t>& idx, const float* params, float* dst) {
    const int JJ = t.J * t.J;
    for (size_t i = 0; i < idx.size(); ++i) {
        const int32_t c = idx[i];
        if (c >= 0) dst[i] = params[c];
        else if (c <= TRAIN_LG) {
            const int e = TRAIN_LG - c;
            dst[i] = train_lg(params + t.ahat[e / JJ], t.J, e % JJ / t.J, e % JJ % t.J);
        }
    }
}

// A float as the decimal its writer meant: the shortest one that rounds to it (0.999f is 0.999), in double.  The
// optimiser's constants 1 - beta are taken from these: 1 - (double)0.999f is off 0.001 by 1.3e-5 of its value.
static double train_decimal(float v) {
    if (!(v == v) || v - v != 0.f) return (double)v;
    char buf[32];
    for (int p = 1; p <= 9; ++p) {
        snprintf(buf, sizeof buf, "%.*g", p, (double)v);
        if (strtof(buf, nullptr) == v) return strtod(buf, nullptr);
    }
    return (double)v;
}
// What the host works out for step k of Adam, as torch's single-tensor path does: in double, each rounded once
struct TrainStep {
    float step_size, bc2_sqrt;
};
static TrainStep train_step_consts(double beta1, double beta2, float lr, int64_t k) {
    const double bc1 = 1.0 - pow(beta1, (double)k), bc2 = 1.0 - pow(beta2, (double)k);
    return TrainStep{(float)((double)lr / bc1), (float)sqrt(bc2)};
}
