// dpk_pack.inc — one sampler instance's arenas from the host staging (dpk_stage.inc).  Host-only plain C++,
// included inside each instance namespace after dpk_layout.inc, so every unqualified constant below is
// that instance's; a CPU-only build compiles it too (tests/c/dpk_pack_check.cpp).

// Pack W_eff (K x N, W_eff(k, n)) into MFMA B-fragment blocks [NC][KB][64][4].
template <class F>
static void pack_blocks(float* dst, int Kreal, int Nreal, int KB, int NC, F w) {
    for (int ct = 0; ct < NC; ++ct)
        for (int kb = 0; kb < KB; ++kb)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 4; ++j) {
                    const int k = kb * 16 + 4 * (lane >> 4) + j;
                    const int n = ct * 16 + (lane & 15);
                    dst[((size_t)(ct * KB + kb) * 64 + lane) * 4 + j] = (k < Kreal && n < Nreal) ? w(k, n) : 0.f;
                }
}

// Host fp32 -> bf16, round to nearest even (finite inputs).
static inline uint16_t bf16_rne(float v) {
    uint32_t u = __builtin_bit_cast(uint32_t, v);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
static inline float bf16_to_f32(uint16_t b) { return __builtin_bit_cast(float, (uint32_t)b << 16); }

// Split W_eff * W16_SCALE into 16x16x32 B fragments for the half-width-operand GEMMs (gemmh_pass):
// lane l holds column n = ct*16 + (l&15) at the 8 k of its lane group g = l>>4 in the order
// 4g..4g+3, 16+4g..16+4g+3 of the 32-block (the A fragments' order: two fp32 16x16x4 fragments).
// BF = false (gemm mode 1, f16x3): blocks [NC][KB32][hi 1 KiB | lo 1 KiB], hi = fp16(v) (RNE),
//   lo = fp16(v - hi) (v - hi is exact in fp32, Sterbenz);
// BF = true (gemm mode 2, bf16): blocks [NC][KB32][1 KiB] of bf16(v) (RNE).
template <bool BF = false, class F>
static float pack16(uint16_t* dst, int Kreal, int Nreal, int KB32, int NC, F w) {
    constexpr size_t blk = BF ? 512 : 1024;      // uint16 per block
    float wmax = 0.f;
    for (int ct = 0; ct < NC; ++ct)
        for (int kb = 0; kb < KB32; ++kb)
            for (int lane = 0; lane < 64; ++lane)
                for (int i = 0; i < 8; ++i) {
                    const int g = lane >> 4;
                    const int k = kb * 32 + (i < 4 ? 4 * g + i : 16 + 4 * g + (i - 4));
                    const int n = ct * 16 + (lane & 15);
                    const float v = (k < Kreal && n < Nreal) ? w(k, n) * W16_SCALE : 0.f;
                    wmax = fmaxf(wmax, fabsf(v));
                    const size_t base = (size_t)(ct * KB32 + kb) * blk;
                    if constexpr (BF) {
                        dst[base + lane * 8 + i] = bf16_rne(v);
                    } else {
                        const _Float16 hi = (_Float16)v;
                        const _Float16 lo = (_Float16)(v - (float)hi);
                        dst[base + lane * 8 + i] = __builtin_bit_cast(uint16_t, hi);
                        dst[base + 512 + lane * 8 + i] = __builtin_bit_cast(uint16_t, lo);
                    }
                }
    return wmax;
}

// Everything the instance's kernels read, repacked from the staging `s` (a model of this instance's width,
// 17 joints, at most NL layers; GCNdiff, or GCNpose with coords 2 -> 3): layers past s.L stay zero.
// A staging of n = s.J < 17 joints (GCNdiff on padded tiles): its graph matrices (T1, T2, every layer's L_g,
// all normalised at size n by the staging) are read at stride n and zero-embedded into the 17 x 17 blocks, so a
// padded row neither gives to nor takes from a real one; such a model runs the dense-graph kernels.
// half: also the split-fp16 and bf16 copies of the layer GEMMs' weights, each where the instance has its gemm
// mode (MODE_F16X3, MODE_BF16), and w16_ok.
static void pack_model(const Stage& s, Packed& out, bool half) {
    const bool f16 = half && MODE_F16X3, bf = half && MODE_BF16;
    const float* S = s.h.data();
    const int cin = s.cin, cout = s.cout;
    out.arena.assign(ARENA_FLOATS, 0.f);
    out.temb.assign(TEMB_FLOATS, 0.f);
    out.a16.assign(f16 ? ARENA16_BYTES / 2 : 0, 0);
    out.abf.assign(bf ? ARENA16_BYTES / 4 : 0, 0);     // bf16 blocks: half the bytes
    float* A = out.arena.data();
    float w16max = 0.f;             // largest |64 w| of the split-fp16 GEMM weights
    const int n = s.J;              // the model's joints (<= J)
    // a J x J matrix from the staging's n x n one: zeros outside
    auto embed = [&](size_t at, float* dst) {
        for (int i = 0; i < J; ++i)
            for (int j = 0; j < J; ++j) dst[i * J + j] = (i < n && j < n) ? S[at + (size_t)i * n + j] : 0.f;
    };
    std::vector<float> LG(J * J), T1v(J * J), T2v(J * J);
    for (int l = 0; l < s.L; ++l) {
        const GenLayer& o = s.lay[l];
        float* Lw = A + (size_t)l * LAYER_FLOATS;
        auto at = [&](size_t base, int ld) { return [=](int k, int n) { return S[base + (size_t)k * ld + n]; }; };
        // QKV GEMM with LN0's affine folded in (the LN phase writes (x - mean) / (std + eps)):
        // W' = diag(a) W, bias c = b W + b_qkv (summed in double)
        auto wqkv = [&](int k, int n) { return S[o.n0a + k] * S[o.wqkv + (size_t)k * 3 * D + n]; };
        auto wo = at(o.wo, D), w1 = at(o.w1, 2 * D), w2 = at(o.w2, D);
        auto wc1 = at(o.wc1, D), wc2 = at(o.wc2, D);     // ChebConv: [x | T1x | T2x] rows, the reference's order
        pack_blocks(Lw + OFF_QKV, D, D3, KB_D, 3 * NCD, wqkv);
        for (int n = 0; n < D3; ++n) {
            double cs = 0.0;
            for (int k = 0; k < D; ++k) cs += (double)S[o.n0b + k] * (double)S[o.wqkv + (size_t)k * 3 * D + n];
            Lw[OFF_CQKV + n] = (float)(cs + (double)S[o.bqkv + n]);
            Lw[OFF_BQKV + n] = S[o.bqkv + n];
        }
        pack_blocks(Lw + OFF_O, D, D, KB_D, NCD, wo);
        pack_blocks(Lw + OFF_FC1, D, D2, KB_D, 2 * NCD, w1);
        pack_blocks(Lw + OFF_FC2, D2, D, KB_D2, NCD, w2);
        pack_blocks(Lw + OFF_C1, D3, D, KB_D3, NCD, wc1);
        pack_blocks(Lw + OFF_C2, D3, D, KB_D3, NCD, wc2);
        if (f16 || bf) {            // the fp32 mode's operands, in the half-width packings the instance reads
            uint16_t* L16 = f16 ? out.a16.data() + (size_t)l * LAYER16_BYTES / 2 : nullptr;
            uint16_t* Lb = bf ? out.abf.data() + (size_t)l * LAYER16_BYTES / 4 : nullptr;
            auto both = [&](int o16, int K, int N, int KB32, int NC, auto w) {
                if (f16) w16max = fmaxf(w16max, pack16(L16 + o16 / 2, K, N, KB32, NC, w));
                if (bf) (void)pack16<true>(Lb + o16 / 4, K, N, KB32, NC, w);
            };
            both(O16_QKV, D, D3, KB32_D, 3 * NCD, wqkv);
            both(O16_O, D, D, KB32_D, NCD, wo);
            both(O16_FC1, D, D2, KB32_D, 2 * NCD, w1);
            both(O16_FC2, D2, D, KB32_D2, NCD, w2);
            both(O16_C1, D3, D, KB32_D3, NCD, wc1);
            both(O16_C2, D3, D, KB32_D3, NCD, wc2);
        }
        for (int c = 0; c < D; ++c) {
            Lw[OFF_BO + c] = S[o.bo + c];
            Lw[OFF_BFC2 + c] = S[o.b2 + c];
            Lw[OFF_BC1 + c] = S[o.bc1 + c];
            Lw[OFF_BC2 + c] = S[o.bc2 + c];
            Lw[OFF_LN0A + c] = S[o.n0a + c];
            Lw[OFF_LN0B + c] = S[o.n0b + c];
            Lw[OFF_LN1A + c] = S[o.n1a + c];
            Lw[OFF_LN1B + c] = S[o.n1b + c];
        }
        for (int c = 0; c < D2; ++c) Lw[OFF_BFC1 + c] = S[o.b1 + c];
        embed(o.lg, LG.data());
        for (int i = 0; i < J * J; ++i) Lw[OFF_LG + i] = LG[i];
        for (int q = 0; q < 5; ++q)
            for (int ln = 0; ln < 64; ++ln) {
                const int i = 4 * q + (ln >> 4);
                Lw[OFF_LGF + q * 64 + ln] = i < J ? LG[(ln & 15) * J + i] : 0.f;
                Lw[OFF_LGF + (5 + q) * 64 + ln] = i < J ? LG[16 * J + i] : 0.f;
            }
    }
    // fp16 hi parts must stay finite: |64 w| below the largest fp16 (65504), with margin
    out.w16_ok = w16max < 65000.f;
    // input ChebConv: rows k = order * CIN + channel of the 5-channel tile ([3 cin][D] staging rows;
    // GCNpose's channels 2-4 are zero); output ChebConv as Y = x [W0 | W1 | W2] (D -> 3 cout columns),
    // out = Y0 + T1 Y1 + T2 Y2 in the kernel
    pack_blocks(A + OFF_WIN, 3 * CIN, D, 1, NCD, [&](int k, int n) {
        const int ord = k / CIN, c = k % CIN;
        return c < cin ? S[s.win + ((size_t)ord * cin + c) * D + n] : 0.f;
    });
    pack_blocks(A + OFF_WOUT, D, 3 * cout, KB_D, 1,
                [&](int k, int n) { return S[s.wout + ((size_t)(n / cout) * D + k) * cout + n % cout]; });
    for (int c = 0; c < D; ++c) A[OFF_BIN + c] = S[s.bin + c];
    for (int c = 0; c < 16; ++c) A[OFF_BOUT + c] = c < cout ? S[s.bout + c] : 0.f;
    // Chebyshev terms: dense, and the H36M-sparse forms, used when every nonzero lies inside the compiled pattern
    embed(s.t1, T1v.data());
    embed(s.t2, T2v.data());
    const float* T1 = T1v.data();
    const float* T2 = T2v.data();
    for (int i = 0; i < J * J; ++i) {
        A[OFF_CHEB + i] = T1[i];
        A[OFF_CHEB + J * J + i] = T2[i];
    }
    bool fits = true;
    for (int i = 0; i < J; ++i)
        for (int j = 0; j < J; ++j) {
            bool in1 = false, in2 = false;
            for (int k = 0; k < SPAT.n1[i]; ++k) in1 = in1 || SPAT.c1[i][k] == j;
            for (int k = 0; k < SPAT.n2[i]; ++k) in2 = in2 || SPAT.c2[i][k] == j;
            if ((!in1 && T1[i * J + j] != 0.f) || (!in2 && T2[i * J + j] != 0.f)) fits = false;
        }
    for (int i = 0; i < J; ++i) {
        for (int k = 0; k < SPAT.n1[i]; ++k) A[OFF_CHEBS + SPAT.o1[i] + k] = T1[i * J + SPAT.c1[i][k]];
        for (int k = 0; k < SPAT.n2[i]; ++k)
            A[OFF_CHEBS + SPAT.nnz1 + SPAT.o2[i] + k] = T2[i * J + SPAT.c2[i][k]];
        // padded rows of the same values for the output ChebConv: (value bits, row offset j'*LD2)
        float* row = &A[OFF_CHEBT + (size_t)i * (SPT1 + SPT2) * 2];
        for (int k = 0; k < SPT1 + SPT2; ++k) {
            const bool t1 = k < SPT1;
            const int kk = t1 ? k : k - SPT1;
            const int n = t1 ? SPAT.n1[i] : SPAT.n2[i];
            const int col = kk < n ? (t1 ? SPAT.c1[i][kk] : SPAT.c2[i][kk]) : i;
            row[2 * k] = kk < n ? (t1 ? T1 : T2)[i * J + col] : 0.f;
            const int32_t off = col * LD2;
            memcpy(&row[2 * k + 1], &off, 4);
        }
    }
    out.sparse = fits && n == J;    // fewer joints: the dense kernels (the padded ones are built for them alone)
    if (s.kind != 0) return;    // GCNpose has no timestep MLP
    // timestep MLP, transposed [in][out] (the staging rows are already [in][out])
    float* T = out.temb.data();
    for (size_t i = 0; i < (size_t)D * E; ++i) T[TOFF_W0 + i] = S[s.d0w + i];
    for (size_t i = 0; i < (size_t)E * E; ++i) T[TOFF_W1 + i] = S[s.d1w + i];
    for (int c = 0; c < E; ++c) {
        T[TOFF_B0 + c] = S[s.d0b + c];
        T[TOFF_B1 + c] = S[s.d1b + c];
    }
    for (size_t i = 0; i < (size_t)s.L * E * D; ++i) T[TOFF_WP + i] = S[s.wtp + i];
    for (size_t i = 0; i < (size_t)s.L * D; ++i) T[TOFF_BP + i] = S[s.btp + i];
}
