// dpk_stage.inc — the host staging of one model, for any shape: its weights as row-major W_eff[k][n] blocks
// and its graph's Chebyshev terms in one float arena, filled from a state_dict and an adjacency.  Every
// handle holds one (dpk_handle::stage); the per-op path's kernels read a device copy of it, and each sampler
// instance packs its own arena from it (dpk_pack.inc).
// Plain C++ (no HIP), so a CPU-only build compiles it too (tests/c/dpk_pack_check.cpp).
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

struct GenLayer {
    size_t wqkv, bqkv, wo, bo, n0a, n0b, n1a, n1b, w1, b1, w2, b2, lg, wc1, bc1, wc2, bc2;
};
struct Stage {
    int D = 0, H = 0, J = 0, L = 0, cin = 0, cout = 0, kind = 0, E = 0;   // kind 0: GCNdiff, 1: GCNpose
    std::vector<GenLayer> lay;
    size_t win = 0, bin = 0, wout = 0, bout = 0, t1 = 0, t2 = 0, d0w = 0, d0b = 0, d1w = 0, d1b = 0;
    size_t wtp = 0, btp = 0;   // every layer's temb_proj: [L][E][D] (k-major), [L][D]
    size_t floats = 0;
    std::vector<float> h;      // the arena (offsets above, each 16-byte aligned)
    std::vector<float> ahat;   // every layer's A_hat as loaded, [L][J*J]: the gradient goes back through lg to it
};

// What a sampler instance's pack_model makes of a Stage: its weight arena and timestep-MLP arena in the
// instance's layouts (dpk_layout.inc), the half-width copies of the GEMM weights for each of gemm modes 1 and 2
// the instance has (else empty), and what the host decides from the values
struct Packed {
    std::vector<float> arena, temb;
    std::vector<uint16_t> a16;   // split-fp16 GEMM weights (gemm mode 1)
    std::vector<uint16_t> abf;   // bf16 GEMM weights (gemm mode 2), same layout
    bool sparse = false;         // the adjacency fits the compiled H36M Chebyshev pattern (sparse kernels)
    bool w16_ok = true;          // the GEMM weights fit the split-fp16 packing (|w| < 1015)
};

// The shape and pack half of a sampler instance's descriptor (SHAPE in dpk_genfused.inc, one per instance
// namespace; SamplerInst in dpk_kernels.hip adds the launch half)
struct InstShape {
    int D, NH, J, NL;            // hid_dim, n_head, n_pts of the tile, the most layers a launch runs
    int Jmin;                    // fewest joints of a GCNdiff model it runs (below J: padded tiles, dpk_layout.inc)
    int P, NW, NT, lds_bytes;    // poses, waves and threads per workgroup; static LDS
    size_t tp;                   // floats of timestep projections per step (sample) or pose (eps): NL * D
    int modes;                   // bit m set: has gemm mode m's kernels and arena (0 fp32: always; 1 f16x3; 2 bf16)
    bool pose;                   // has the GCNpose kernels (coords 2 -> 3)
    int cin, cout;               // GCNdiff coords
    size_t arena_floats, temb_floats, arena16_bytes, arenabf_bytes;   // the half-width two: 0 without their mode
    // half: also the half-width arenas of the modes the instance has (and w16_ok); false: neither
    void (*pack)(const Stage& s, Packed& out, bool half);
    constexpr bool has_mode(int m) const { return m >= 0 && m < 3 && (modes >> m & 1); }
    // does this instance run a model of this shape?  kind 1 (GCNpose) is coords 2 -> 3 by definition, and J joints
    // alone; GCNdiff also on Jmin..J-1 joints, as padded tiles
    bool fits(int Dm, int Hm, int Jm, int Lm, int cin_, int cout_, int kind) const {
        return Dm == D && Hm == NH && Lm >= 1 && Lm <= NL &&
               (kind == 0 ? Jm >= Jmin && Jm <= J && cin_ == cin && cout_ == cout : Jm == J && pose);
    }
};

static void stage_init(Stage& s, int D, int H, int J, int L, int cin, int cout, int kind) {
    s.D = D, s.H = H, s.J = J, s.L = L, s.cin = cin, s.cout = cout, s.kind = kind, s.E = 4 * D;
    size_t o = 0;
    auto take = [&](size_t n) {
        const size_t at = o;
        o += (n + 3) / 4 * 4;
        return at;
    };
    s.lay.resize(L);
    for (auto& l : s.lay) {
        l.wqkv = take((size_t)D * 3 * D), l.bqkv = take(3 * D), l.wo = take((size_t)D * D), l.bo = take(D);
        l.n0a = take(D), l.n0b = take(D), l.n1a = take(D), l.n1b = take(D);
        l.w1 = take((size_t)D * 2 * D), l.b1 = take(2 * D), l.w2 = take((size_t)2 * D * D), l.b2 = take(D);
        l.lg = take((size_t)J * J), l.wc1 = take((size_t)3 * D * D), l.bc1 = take(D), l.wc2 = take((size_t)3 * D * D);
        l.bc2 = take(D);
    }
    s.win = take((size_t)3 * cin * D), s.bin = take(D), s.wout = take((size_t)3 * D * cout), s.bout = take(cout);
    s.t1 = take((size_t)J * J), s.t2 = take((size_t)J * J);
    s.d0w = take((size_t)D * s.E), s.d0b = take(s.E), s.d1w = take((size_t)s.E * s.E), s.d1b = take(s.E);
    s.wtp = take((size_t)L * s.E * D), s.btp = take((size_t)L * D);
    s.floats = o;
    s.h.assign(o, 0.f);
}

// Chebyshev terms of the normalised Laplacian, fp32 in the reference's operation order
// (ChebConv.py:114-130, :90-112): d = rowsum^-1/2; L = I - (d_i g_ij) d_j; T1 = L, T2 = 2 L@L - I.
static void stage_set_graph(Stage& s, const float* adj) {
    const int J = s.J;
    std::vector<float> d(J), L((size_t)J * J);
    for (int i = 0; i < J; ++i) {
        float r = 0.f;
        for (int j = 0; j < J; ++j) r += adj[i * J + j];
        d[i] = 1.0f / sqrtf(r);
    }
    for (int i = 0; i < J; ++i)
        for (int j = 0; j < J; ++j) L[i * J + j] = (i == j ? 1.f : 0.f) - (d[i] * adj[i * J + j]) * d[j];
    for (int i = 0; i < J; ++i)
        for (int j = 0; j < J; ++j) {
            float acc = 0.f;
            for (int k = 0; k < J; ++k) acc += L[i * J + k] * L[k * J + j];
            s.h[s.t1 + i * J + j] = L[i * J + j];
            s.h[s.t2 + i * J + j] = 2.f * acc - (i == j ? 1.f : 0.f);
        }
}

// Weights from a state_dict (keys and sizes of models/gcndiff.py / gcnpose.py for this shape; a leading
// "module." is dropped); nn.Linear (out, in) and ChebConv (3, 1, in, out) weights stored k-major [in][out].
// All or nothing: false, with `err` naming the first key that is missing or has the wrong size, leaves the
// staging as it was.
static bool stage_load(Stage& s, const char* const* names, const float* const* ptrs, const int64_t* numels, int n,
                       std::string& err) {
    std::unordered_map<std::string, std::pair<const float*, int64_t>> sd;
    for (int i = 0; i < n; ++i) {
        std::string k = names[i];
        if (k.rfind("module.", 0) == 0) k = k.substr(7);
        sd[k] = {ptrs[i], numels[i]};
    }
    auto get = [&](const std::string& k, int64_t numel) -> const float* {
        auto it = sd.find(k);
        if (it == sd.end()) {
            if (err.empty()) err = "missing key " + k;
            return nullptr;
        }
        if (it->second.second != numel) {
            if (err.empty()) err = "size mismatch for " + k;
            return nullptr;
        }
        return it->second.first;
    };
    err.clear();
    const int D = s.D, E = s.E, J = s.J;
    std::vector<float> fresh = s.h;     // keeps the graph's terms
    std::vector<float> fresh_ahat((size_t)s.L * J * J);
    float* A = fresh.data();
    for (int l = 0; l < s.L; ++l) {
        const GenLayer& o = s.lay[l];
        const std::string at = "atten_layers." + std::to_string(l) + ".", gc = "gconv_layers." + std::to_string(l) + ".";
        const float* w[4];
        const float* b[4];
        for (int j = 0; j < 4; ++j) {
            w[j] = get(at + "self_attn.linears." + std::to_string(j) + ".weight", (int64_t)D * D);
            b[j] = get(at + "self_attn.linears." + std::to_string(j) + ".bias", (int64_t)D);
            if (!w[j] || !b[j]) return false;
        }
        const float* ahat = get(at + "feed_forward.A_hat", (int64_t)J * J);
        const float* f1w = get(at + "feed_forward.gconv1.fc.weight", (int64_t)2 * D * D);
        const float* f1b = get(at + "feed_forward.gconv1.fc.bias", (int64_t)2 * D);
        const float* f2w = get(at + "feed_forward.gconv2.fc.weight", (int64_t)2 * D * D);
        const float* f2b = get(at + "feed_forward.gconv2.fc.bias", (int64_t)D);
        const float* n0a = get(at + "sublayer.0.norm.a_2", D);
        const float* n0b = get(at + "sublayer.0.norm.b_2", D);
        const float* n1a = get(at + "sublayer.1.norm.a_2", D);
        const float* n1b = get(at + "sublayer.1.norm.b_2", D);
        const float* c1w = get(gc + "gconv1.gconv.weight", (int64_t)3 * D * D);
        const float* c1b = get(gc + "gconv1.gconv.bias", D);
        const float* c2w = get(gc + "gconv2.gconv.weight", (int64_t)3 * D * D);
        const float* c2b = get(gc + "gconv2.gconv.bias", D);
        if (!ahat || !f1w || !f1b || !f2w || !f2b || !n0a || !n0b || !n1a || !n1b || !c1w || !c1b || !c2w || !c2b)
            return false;
        std::copy(ahat, ahat + (size_t)J * J, fresh_ahat.begin() + (size_t)l * J * J);
        for (int k = 0; k < D; ++k)
            for (int n = 0; n < 3 * D; ++n) A[o.wqkv + (size_t)k * 3 * D + n] = w[n / D][(size_t)(n % D) * D + k];
        for (int n = 0; n < 3 * D; ++n) A[o.bqkv + n] = b[n / D][n % D];
        for (int k = 0; k < D; ++k)
            for (int n = 0; n < D; ++n) A[o.wo + (size_t)k * D + n] = w[3][(size_t)n * D + k];
        for (int k = 0; k < D; ++k)
            for (int n = 0; n < 2 * D; ++n) A[o.w1 + (size_t)k * 2 * D + n] = f1w[(size_t)n * D + k];
        for (int k = 0; k < 2 * D; ++k)
            for (int n = 0; n < D; ++n) A[o.w2 + (size_t)k * D + n] = f2w[(size_t)n * 2 * D + k];
        for (size_t i = 0; i < (size_t)3 * D * D; ++i) {   // (3,1,in,out) is already [3*in][out]
            A[o.wc1 + i] = c1w[i];
            A[o.wc2 + i] = c2w[i];
        }
        for (int c = 0; c < D; ++c) {
            A[o.bo + c] = b[3][c], A[o.b2 + c] = f2b[c], A[o.bc1 + c] = c1b[c], A[o.bc2 + c] = c2b[c];
            A[o.n0a + c] = n0a[c], A[o.n0b + c] = n0b[c], A[o.n1a + c] = n1a[c], A[o.n1b + c] = n1b[c];
        }
        for (int c = 0; c < 2 * D; ++c) A[o.b1 + c] = f1b[c];
        // GraphNet Laplacian (GraFormer.py:174-178): c_k = colsum_k + 1e-5; L = c_i^-1/2 A_ij c_j^-1/2
        std::vector<float> dh(J);
        for (int k = 0; k < J; ++k) {
            float r = 0.f;
            for (int i = 0; i < J; ++i) r += ahat[i * J + k];
            dh[k] = 1.0f / sqrtf(r + 1e-5f);
        }
        for (int i = 0; i < J; ++i)
            for (int j = 0; j < J; ++j) A[o.lg + i * J + j] = (dh[i] * ahat[i * J + j]) * dh[j];
        if (s.kind == 0) {     // GCNpose's _ResChebGC has no temb_proj (models/ChebConv.py:154-165)
            const float* tpw = get(gc + "temb_proj.weight", (int64_t)D * E);
            const float* tpb = get(gc + "temb_proj.bias", D);
            if (!tpw || !tpb) return false;
            for (int k = 0; k < E; ++k)
                for (int n = 0; n < D; ++n) A[s.wtp + ((size_t)l * E + k) * D + n] = tpw[(size_t)n * E + k];
            for (int c = 0; c < D; ++c) A[s.btp + (size_t)l * D + c] = tpb[c];
        }
    }
    const float* wi = get("gconv_input.weight", (int64_t)3 * s.cin * D);
    const float* bi = get("gconv_input.bias", D);
    const float* wout = get("gconv_output.weight", (int64_t)3 * D * s.cout);
    const float* bout = get("gconv_output.bias", s.cout);
    if (!wi || !bi || !wout || !bout) return false;
    std::copy(wi, wi + (size_t)3 * s.cin * D, A + s.win);
    std::copy(bi, bi + D, A + s.bin);
    std::copy(wout, wout + (size_t)3 * D * s.cout, A + s.wout);
    std::copy(bout, bout + s.cout, A + s.bout);
    if (s.kind == 0) {         // GCNpose carries temb.dense too (gcnpose.py:94-98) but never uses it
        const float* d0w = get("temb.dense.0.weight", (int64_t)E * D);
        const float* d0b = get("temb.dense.0.bias", E);
        const float* d1w = get("temb.dense.1.weight", (int64_t)E * E);
        const float* d1b = get("temb.dense.1.bias", E);
        if (!d0w || !d0b || !d1w || !d1b) return false;
        for (int k = 0; k < D; ++k)
            for (int o = 0; o < E; ++o) A[s.d0w + (size_t)k * E + o] = d0w[(size_t)o * D + k];
        for (int k = 0; k < E; ++k)
            for (int o = 0; o < E; ++o) A[s.d1w + (size_t)k * E + o] = d1w[(size_t)o * E + k];
        std::copy(d0b, d0b + E, A + s.d0b);
        std::copy(d1b, d1b + E, A + s.d1b);
    }
    s.h.swap(fresh);
    s.ahat.swap(fresh_ahat);
    return true;
}
