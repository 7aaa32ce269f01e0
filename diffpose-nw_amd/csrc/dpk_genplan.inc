// dpk_genplan.inc — everything about a per-op launch (dpk_generic.inc, dpk_generic_bwd.inc) that is decided on the
// host: which form of a kernel runs, its grid and dynamic LDS, the gemm_sk weight copies, the scratch layouts.
// One rule for the forward, the training forward and the backward.  Plain C++ after dpk_stage.inc (no HIP:
// tests/c/dpk_genplan_check.cpp compiles the two alone); pointers enter as addresses, only their alignment counts.

namespace dpkg {

constexpr int GBN = 64;                    // columns of a gemm<BM, VEC> tile
constexpr unsigned SK_OOR = 0x80000000u;   // gemm_sk's out-of-range offset: its A operand must end below it
constexpr int DW_ROWS = 128;               // rows of one dW slab
constexpr int DLG_POSES = 8;               // poses of one dL_g slab
constexpr size_t LDS_MAX = 65536;          // dynamic LDS of a staged form

// The kernel forms the forward's ops choose between per call (from the shape, the batch and pointer alignment),
// one bit each: GenModel::forms (BwdModel::fforms for a gradient call) collects the bits of what was launched,
// dpk_debug_generic_forms reads and clears them (test hook; diffpose_amd/gcndiff.py GENERIC_FORMS names the bits in
// this order).
enum GenForm : unsigned {
    F_GEMM_NARROW = 1u << 0,
    F_GEMM_SK4 = 1u << 1,
    F_GEMM_SK2 = 1u << 2,
    F_GEMM_128_VEC = 1u << 3,
    F_GEMM_128_SCALAR = 1u << 4,
    F_GEMM_64_VEC = 1u << 5,
    F_GEMM_64_SCALAR = 1u << 6,
    F_GEMM_32_VEC = 1u << 7,
    F_GEMM_32_SCALAR = 1u << 8,
    F_ATTENTION_TT = 1u << 9,     // attention<STAGE, VEC>
    F_ATTENTION_TF = 1u << 10,
    F_ATTENTION_FF = 1u << 11,
    F_GRAPH_T = 1u << 12,         // graph<STAGE>
    F_GRAPH_F = 1u << 13,
    F_CHEB_T = 1u << 14,          // cheb_basis<STAGE>
    F_CHEB_F = 1u << 15,
};

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
    B_ATTN_TRAIN = 1u << 11,      // attention_train / attention_bwd_train: a nonzero rate on p_attn
    B_DROP_ADD = 1u << 12,        // drop_apply<true>: a nonzero rate on the sublayers' outputs
    B_RELU_DROP = 1u << 13,       // drop_apply<false> on a ChebConv's ReLU output: a nonzero rate there
};

// One dropout site of a train-mode gradient call (dpk_diff_loss_grad_train): element i of the site's tensor (its flat
// index over the whole batch) keeps its value, times s, iff word i & 3 of Philox4x32-10 at counter
// {i >> 2 lo, i >> 2 hi, dom, 0xD809} under the key {k0, k1}, shifted right by 8, is at least thr.  thr 0: the site is
// off (the eval-mode launches run in its place).
struct DropSite {
    unsigned thr = 0;
    float s = 1.0f;
    unsigned dom = 0;             // layer * 8 + site
    unsigned k0 = 0, k1 = 0;      // drop_seed's two halves
};
enum DropSiteId { DROP_ATTN = 0, DROP_SUB0 = 1, DROP_SUB1 = 2, DROP_GC1 = 3, DROP_GC2 = 4, DROP_SITES = 5 };

}  // namespace dpkg

static inline unsigned gen_blocks(long long n) { return (unsigned)((n + 255) / 256); }
static inline bool gen_al16(uintptr_t p) { return (p & 15) == 0; }

// ---- the GEMM rule

// The A/B switches: DPK_GEN_GEMM=lds puts the LDS-staged gemm<BM> where gemm_sk would run, DPK_GEN_BM=128|64|32
// fixes gemm<BM>'s tile height (any other value: the rule's own).  From the variables' values, null when unset.
struct GenSwitches {
    bool sk = true;
    int bm = 0;
};
static GenSwitches gen_switches(const char* gemm, const char* bm) {
    GenSwitches s;
    s.sk = !(gemm && strcmp(gemm, "lds") == 0);
    const int v = bm ? atoi(bm) : 0;
    s.bm = v == 128 || v == 64 || v == 32 ? v : 0;
    return s;
}

enum GemmKind { GEMM_NARROW, GEMM_SK4, GEMM_SK2, GEMM_LDS };
struct GemmChoice {
    GemmKind kind;
    int bm;            // gemm<BM, VEC>'s; the other kinds ignore both
    bool vec;
    unsigned gx, gy;   // grid
    size_t lds;        // dynamic LDS bytes (gemm_narrow's copy of W)
    unsigned form;     // the GenForm bit
};
// C[M][N] (row stride ldc) = epilogue(A[M][K] W[K][N] + bias): a, w, bias, c and tp (0: no timestep rows) are the
// operands' addresses, pack_nj the NJ of W's gemm_sk copy or 0 without one.
static GemmChoice gemm_choice(int M, int K, int N, int ldc, uintptr_t a, uintptr_t w, uintptr_t bias, uintptr_t c,
                              uintptr_t tp, int tp_stride, int pack_nj, int n_cu, GenSwitches sw) {
    GemmChoice g;
    // the row-tile height whose tiles finish soonest when dealt out to the CUs (a tile's time taken as
    // proportional to its height): ceil(tiles / CUs) x BM; the taller tile wins ties
    const long long nt = (N + dpkg::GBN - 1) / dpkg::GBN, cu = std::max(n_cu, 1);
    g.bm = 128;
    long long best = -1;
    for (int cand : {128, 64, 32}) {
        const long long cost = ((M + cand - 1) / cand * nt + cu - 1) / cu * cand;
        if (best < 0 || cost < best) best = cost, g.bm = cand;
    }
    if (sw.bm) g.bm = sw.bm;
    // 16-byte operand loads when every row start is 16-byte aligned (the arena's blocks are, by take())
    g.vec = K % 4 == 0 && N % 4 == 0 && gen_al16(a) && gen_al16(w);
    if (N <= 8 && (size_t)K * N * 4 <= dpkg::LDS_MAX) {
        g.kind = GEMM_NARROW, g.gx = (unsigned)((M + 3) / 4), g.gy = 1, g.lds = (size_t)K * N * 4;
        g.form = dpkg::F_GEMM_NARROW;
        return g;
    }
    g.lds = 0;
    if (pack_nj && g.vec && sw.sk && ldc % 4 == 0 && gen_al16(c) && gen_al16(bias) &&
        (!tp || (gen_al16(tp) && tp_stride % 4 == 0)) && (size_t)M * K * 4 + (size_t)K * 4 < dpkg::SK_OOR) {
        g.kind = pack_nj == 4 ? GEMM_SK4 : GEMM_SK2;
        g.gx = (unsigned)((M + 15) / 16), g.gy = (unsigned)(((N + 15) / 16 + pack_nj - 1) / pack_nj);
        g.form = pack_nj == 4 ? dpkg::F_GEMM_SK4 : dpkg::F_GEMM_SK2;
        return g;
    }
    g.kind = GEMM_LDS, g.gx = (unsigned)((M + g.bm - 1) / g.bm), g.gy = (unsigned)nt;
    g.form = g.bm == 128 ? (g.vec ? dpkg::F_GEMM_128_VEC : dpkg::F_GEMM_128_SCALAR)
             : g.bm == 64 ? (g.vec ? dpkg::F_GEMM_64_VEC : dpkg::F_GEMM_64_SCALAR)
                          : (g.vec ? dpkg::F_GEMM_32_VEC : dpkg::F_GEMM_32_SCALAR);
    return g;
}

// ---- gemm_sk's weight copies

// A GEMM weight block [K][N] of an arena (offset w) ...
struct PackBlock {
    size_t w;
    int K, N;
};
// ... repacked into gemm_sk's fragment order at offset off of the packed arena
struct GenPack {
    size_t w, off;
    int K, N, NJ;
};
static inline int pack_ntp(int N, int NJ) { return ((N + 15) / 16 + NJ - 1) / NJ * NJ; }

// Which blocks get a copy, where, and the packed arena's floats: none for K or N off a multiple of 4 or N <= 8
// (gemm_sk never runs there); NJ = 4 column tiles per workgroup where the column tiles divide by 4 (N = 128, 256,
// 384, ...), else 2, the column tiles padded to a multiple of NJ
static size_t pack_plan(const std::vector<PackBlock>& blocks, std::vector<GenPack>& packs) {
    packs.clear();
    size_t off = 0;
    for (const PackBlock& b : blocks) {
        if (b.K % 4 || b.N % 4 || b.N <= 8) continue;
        const int NJ = ((b.N + 15) / 16) % 4 == 0 ? 4 : 2;
        packs.push_back(GenPack{b.w, off, b.K, b.N, NJ});
        off += (size_t)((b.K + 15) / 16) * pack_ntp(b.N, NJ) * 256;
    }
    return off;
}
// The copies of `arena`'s blocks into hp (pack_plan's floats, zero outside K x N): [KC = ceil(K/16)][NTp][64 lanes][4],
// lane l, element s of chunk c and column tile t = W[16c + 4 (l >> 4) + s][16t + (l & 15)]
static void pack_fill(const std::vector<GenPack>& packs, const float* arena, size_t floats, std::vector<float>& hp) {
    hp.assign(floats, 0.f);
    for (const GenPack& p : packs) {
        const int KC = (p.K + 15) / 16, NT16 = (p.N + 15) / 16, NTp = pack_ntp(p.N, p.NJ);
        const float* W = arena + p.w;
        float* dst = hp.data() + p.off;
        for (int c = 0; c < KC; ++c)
            for (int t = 0; t < NT16; ++t)
                for (int l = 0; l < 64; ++l)
                    for (int s = 0; s < 4; ++s) {
                        const int k = 16 * c + 4 * (l >> 4) + s, n = 16 * t + (l & 15);
                        if (k < p.K && n < p.N) dst[(((size_t)c * NTp + t) * 64 + l) * 4 + s] = W[(size_t)k * p.N + n];
                    }
    }
}
static const GenPack* find_pack(const std::vector<GenPack>& packs, size_t w, int K, int N) {
    for (const GenPack& p : packs)
        if (p.w == w && p.K == K && p.N == N) return &p;
    return nullptr;
}
// the staging's GEMM blocks the forward may run on gemm_sk: the hidden-width weights, and the input ChebConv's
static std::vector<PackBlock> gen_pack_blocks(const Stage& s) {
    std::vector<PackBlock> b;
    const int D = s.D;
    for (const GenLayer& o : s.lay) {
        b.push_back({o.wqkv, D, 3 * D}), b.push_back({o.wo, D, D}), b.push_back({o.w1, D, 2 * D});
        b.push_back({o.w2, 2 * D, D}), b.push_back({o.wc1, 3 * D, D}), b.push_back({o.wc2, 3 * D, D});
    }
    b.push_back({s.win, 3 * s.cin, D});
    return b;
}

// ---- staged in LDS, or straight from global memory

// a kernel with a form that stages a pose (or a slab of poses) in LDS and one that does not
struct StageChoice {
    bool stage;
    size_t lds;        // dynamic LDS bytes
    unsigned blocks;
};
static StageChoice stage_choice(size_t lds, unsigned staged_blocks, unsigned global_blocks) {
    const bool st = lds <= dpkg::LDS_MAX;
    return StageChoice{st, st ? lds : 0, st ? staged_blocks : global_blocks};
}
// cheb_basis<STAGE> over N poses of J x C: X_p, T1 and T2 staged, a workgroup per pose
static StageChoice cheb_choice(int N, int J, int C) {
    return stage_choice(((size_t)J * C + 2 * J * J) * 4, (unsigned)N, gen_blocks((long long)N * J * C));
}
// graph<STAGE>: X_p and the Laplacian staged
static StageChoice graph_choice(int N, int J, int C) {
    return stage_choice(((size_t)J * C + J * J) * 4, (unsigned)N, gen_blocks((long long)N * J * C));
}
// dlg_partial<STAGE>: a pose's dY and X rows staged at an odd stride, a workgroup per DLG_POSES poses either way
static StageChoice dlg_choice(int N, int J, int C) {
    const unsigned slabs = (unsigned)((N + dpkg::DLG_POSES - 1) / dpkg::DLG_POSES);
    return stage_choice((size_t)2 * J * (C | 1) * 4, slabs, slabs);
}

// attention<STAGE, VEC>: poses per workgroup enough (head, query) threads to fill 256, within 64 KB of LDS; the
// vector form stores 16 bytes at a time to `out`
struct AttnChoice {
    bool stage, vec;
    int ppb;
    unsigned blocks;
    size_t lds;
    unsigned form;
};
static AttnChoice attention_choice(int N, int J, int D, int H, uintptr_t out) {
    AttnChoice a;
    a.vec = (D / H) % 4 == 0 && D % 8 == 0 && gen_al16(out);
    const size_t pose_bytes = (size_t)J * (3 * D + (a.vec ? 4 : 1)) * 4;
    a.stage = pose_bytes <= dpkg::LDS_MAX;
    if (!a.stage) {
        a.vec = false, a.ppb = 1, a.blocks = (unsigned)N, a.lds = 0, a.form = dpkg::F_ATTENTION_FF;
        return a;
    }
    a.ppb = std::max(1, std::min(256 / (H * J), (int)(dpkg::LDS_MAX / pose_bytes)));
    a.blocks = (unsigned)((N + a.ppb - 1) / a.ppb);
    a.lds = pose_bytes * a.ppb;
    a.form = a.vec ? dpkg::F_ATTENTION_TT : dpkg::F_ATTENTION_TF;
    return a;
}

// attention_bwd: hb heads per pass (2 hb J J floats of probabilities and score gradients), the pose's
// [q | k | v | dO] rows staged behind them when that fits
struct AttnBwdChoice {
    int hb;
    bool stage;
    size_t lds;
};
static AttnBwdChoice attention_bwd_choice(int J, int D, int H) {
    AttnBwdChoice a;
    a.hb = std::max(1, std::min(std::min(H, 256 / J), 4096 / (J * J)));
    const size_t ps = (size_t)2 * a.hb * J * J * 4, staged = ps + (size_t)J * ((4 * D) | 1) * 4;
    a.stage = staged <= dpkg::LDS_MAX;
    a.lds = a.stage ? staged : ps;
    return a;
}

// dw_partial<VEC> of A [rows][K] (lda) and G [rows][N] (ldg) into the slabs at p: a slab per DW_ROWS rows on x, four
// tiles (64 x 64, or 16 x 32 scalar) per workgroup on y; ps floats per slab
struct DwChoice {
    bool vec;
    unsigned nslab, gy;
    size_t ps;
};
static DwChoice dw_choice(int rows, int K, int N, int lda, int ldg, uintptr_t a, uintptr_t g, uintptr_t p) {
    DwChoice d;
    d.vec = K % 4 == 0 && N % 4 == 0 && lda % 4 == 0 && ldg % 4 == 0 && gen_al16(a) && gen_al16(g) && gen_al16(p);
    d.nslab = (unsigned)((rows + dpkg::DW_ROWS - 1) / dpkg::DW_ROWS);
    const unsigned tiles = d.vec ? (unsigned)(((K + 63) / 64) * ((N + 63) / 64)) : (unsigned)(((K + 15) / 16) * ((N + 31) / 32));
    d.gy = (tiles + 3) / 4;
    d.ps = (size_t)(K + 1) * N;
    return d;
}

// ---- scratch

// floats of activation scratch for N poses (gen_forward's buffers)
static size_t gen_act_floats(const Stage& s, int N) {
    const size_t M = (size_t)N * s.J, D = s.D;
    // Zs holds a Chebyshev operand [X | T1X | T2X] of the hidden width or of the input (3 * cin)
    const size_t Z = 3 * std::max(D, (size_t)s.cin);
    return M * (D + D + Z + D + 2 * D + 2 * D) + M * (size_t)std::max(s.cout, 4);
}
// floats of scratch one gen_eps call over N poses takes: the forward's activations, then the per-pose projections
static size_t gen_eps_floats(const Stage& s, int N) { return gen_act_floats(s, N) + (size_t)N * s.L * s.D; }

// The gradient call's scratch, in floats, every part on a 256-byte boundary.  Per layer the stash keeps 22 D floats a
// row (H, Y0, QKV 3D, A, H1, Y1, G1, F 2D, G2 2D, H2, Z1 3D, R1, Z2 3D, R2); beside the layers 3 cin + 4 D a row (the
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
        float* at = base ? base + o : nullptr;      // base null: sizes only
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
