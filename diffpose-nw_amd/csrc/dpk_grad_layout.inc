// dpk_grad_layout.inc — the host side of dpk_diff_loss_grad that needs no device: where each parameter's
// gradient stands in the flat output array (the state_dict's names, order and torch layouts:
// diffpose_amd/weights.py param_shapes), and the second weight arena the dX GEMMs read, every GEMM block of the
// staging transposed in place.  Plain C++ after dpk_stage.inc (tests/c/dpk_grad_layout_check.cpp compiles the two
// alone).

struct GradEntry {
    std::string name;
    int64_t offset, numel;     // floats; offsets are multiples of 4
};
struct GradLayer {
    size_t c1w, c1b, c2w, c2b, tpw, tpb;                                     // gconv_layers.l
    size_t lw[4], lb[4], ahat, f1w, f1b, f2w, f2b, n0a, n0b, n1a, n1b;      // atten_layers.l
};
struct GradLayout {
    std::vector<GradEntry> e;
    std::vector<GradLayer> lay;
    size_t win = 0, bin = 0, wout = 0, bout = 0, d0w = 0, d0b = 0, d1w = 0, d1b = 0;
    size_t floats = 0;         // the array's extent: the last entry's offset + numel
};

// GCNdiff's parameters in state_dict order (models/gcndiff.py:55-99)
static GradLayout grad_layout(const Stage& s) {
    GradLayout g;
    const size_t D = s.D, E = s.E, J = s.J;
    size_t o = 0;
    auto add = [&](const std::string& name, size_t n) {
        const size_t at = o;
        g.e.push_back(GradEntry{name, (int64_t)at, (int64_t)n});
        g.floats = at + n;
        o += (n + 3) / 4 * 4;
        return at;
    };
    g.lay.resize(s.L);
    g.win = add("gconv_input.weight", 3 * s.cin * D);
    g.bin = add("gconv_input.bias", D);
    for (int l = 0; l < s.L; ++l) {
        const std::string p = "gconv_layers." + std::to_string(l) + ".";
        GradLayer& y = g.lay[l];
        y.c1w = add(p + "gconv1.gconv.weight", 3 * D * D), y.c1b = add(p + "gconv1.gconv.bias", D);
        y.c2w = add(p + "gconv2.gconv.weight", 3 * D * D), y.c2b = add(p + "gconv2.gconv.bias", D);
        y.tpw = add(p + "temb_proj.weight", D * E), y.tpb = add(p + "temb_proj.bias", D);
    }
    for (int l = 0; l < s.L; ++l) {
        const std::string p = "atten_layers." + std::to_string(l) + ".";
        GradLayer& y = g.lay[l];
        for (int j = 0; j < 4; ++j) {
            y.lw[j] = add(p + "self_attn.linears." + std::to_string(j) + ".weight", D * D);
            y.lb[j] = add(p + "self_attn.linears." + std::to_string(j) + ".bias", D);
        }
        y.ahat = add(p + "feed_forward.A_hat", J * J);
        y.f1w = add(p + "feed_forward.gconv1.fc.weight", 2 * D * D), y.f1b = add(p + "feed_forward.gconv1.fc.bias", 2 * D);
        y.f2w = add(p + "feed_forward.gconv2.fc.weight", 2 * D * D), y.f2b = add(p + "feed_forward.gconv2.fc.bias", D);
        y.n0a = add(p + "sublayer.0.norm.a_2", D), y.n0b = add(p + "sublayer.0.norm.b_2", D);
        y.n1a = add(p + "sublayer.1.norm.a_2", D), y.n1b = add(p + "sublayer.1.norm.b_2", D);
    }
    g.wout = add("gconv_output.weight", 3 * D * s.cout);
    g.bout = add("gconv_output.bias", s.cout);
    g.d0w = add("temb.dense.0.weight", E * D), g.d0b = add("temb.dense.0.bias", E);
    g.d1w = add("temb.dense.1.weight", E * E), g.d1b = add("temb.dense.1.bias", E);
    return g;
}

// A GEMM block W[K][N] of the staging at offset w; the transposed arena holds W^T [N][K] at the same offset
struct BwdBlock {
    size_t w;
    int K, N;
};
// The staging with every GEMM block and every layer's GraphNet Laplacian transposed in place (dA = dC W^T runs the
// forward's GEMM kernels on it, dX = L_g^T dY the forward's graph kernel), then a row of zeros (those kernels add a
// bias) and every layer's A_hat as loaded (stride jj4 floats).  The Chebyshev terms stay as they are.
struct BwdArena {
    std::vector<BwdBlock> blocks;
    size_t zero = 0, zero_n = 0, ahat = 0, jj4 = 0, floats = 0;
    std::vector<float> h;
};
static void bwd_arena_build(const Stage& s, BwdArena& a) {
    const int D = s.D, E = s.E, J = s.J;
    a.blocks.clear();
    for (const GenLayer& o : s.lay) {
        a.blocks.push_back({o.wqkv, D, 3 * D}), a.blocks.push_back({o.wo, D, D});
        a.blocks.push_back({o.w1, D, 2 * D}), a.blocks.push_back({o.w2, 2 * D, D});
        a.blocks.push_back({o.lg, J, J});
        a.blocks.push_back({o.wc1, 3 * D, D}), a.blocks.push_back({o.wc2, 3 * D, D});
    }
    a.blocks.push_back({s.win, 3 * s.cin, D}), a.blocks.push_back({s.wout, 3 * D, s.cout});
    a.blocks.push_back({s.d0w, D, E}), a.blocks.push_back({s.d1w, E, E});
    for (int l = 0; l < s.L; ++l) a.blocks.push_back({s.wtp + (size_t)l * E * D, E, D});
    a.zero = s.floats;
    a.zero_n = (size_t)(std::max(std::max(3 * D, 3 * s.cin), std::max(E, s.L * D)) + 3) / 4 * 4;
    a.ahat = a.zero + a.zero_n;
    a.jj4 = ((size_t)J * J + 3) / 4 * 4;
    a.floats = a.ahat + (size_t)s.L * a.jj4;
    a.h.assign(a.floats, 0.f);
    std::copy(s.h.begin(), s.h.end(), a.h.begin());
    for (const BwdBlock& b : a.blocks)
        for (int k = 0; k < b.K; ++k)
            for (int n = 0; n < b.N; ++n) a.h[b.w + (size_t)n * b.K + k] = s.h[b.w + (size_t)k * b.N + n];
    if (s.ahat.size() == (size_t)s.L * J * J)
        for (int l = 0; l < s.L; ++l)
            std::copy(s.ahat.begin() + (size_t)l * J * J, s.ahat.begin() + (size_t)(l + 1) * J * J,
                      a.h.begin() + a.ahat + (size_t)l * a.jj4);
}
