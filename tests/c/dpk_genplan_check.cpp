// The per-op path's host-side launch rule as a stand-alone program (tests/test_genplan_cpu.py): csrc/dpk_stage.inc and
// csrc/dpk_genplan.inc alone, no HIP.  One line per case: the GEMM rule at each predicate's edge, the tile-height
// rule, the gemm_sk pack plan and packer against a naive restatement, the staged-or-global choices and bwd_plan.
#include <stdio.h>
#include <stdlib.h>

#include "../../diffpose-nw_amd/csrc/dpk_stage.inc"
#include "../../diffpose-nw_amd/csrc/dpk_genplan.inc"

static const char* form_name(unsigned f) {
    static const char* names[] = {"gemm_narrow",    "gemm_sk<4>",      "gemm_sk<2>",    "gemm<128,vec>", "gemm<128,scalar>", "gemm<64,vec>",
                                  "gemm<64,scalar>", "gemm<32,vec>",    "gemm<32,scalar>", "attention<TT>", "attention<TF>",  "attention<FF>"};
    for (int i = 0; i < 12; ++i)
        if (f == 1u << i) return names[i];
    return "?";
}

// operand addresses: 16-byte aligned unless a case moves one by 4 bytes
struct Gemm {
    int M = 119, K = 32, N = 32, ldc = 32;
    uintptr_t a = 0x10000, w = 0x20000, bias = 0x30000, c = 0x40000, tp = 0;
    int tps = 0, nj = 2, n_cu = 256;
    GenSwitches sw;
};
static void gemm_line(const char* name, const Gemm& q) {
    const GemmChoice g = gemm_choice(q.M, q.K, q.N, q.ldc, q.a, q.w, q.bias, q.c, q.tp, q.tps, q.nj, q.n_cu, q.sw);
    printf("%s %s bm=%d vec=%d grid=%ux%u lds=%zu\n", name, form_name(g.form), g.bm, (int)g.vec, g.gx, g.gy, g.lds);
}
static void switch_line(const char* name, const char* gemm, const char* bm) {
    const GenSwitches s = gen_switches(gemm, bm);
    printf("%s sk=%d bm=%d\n", name, (int)s.sk, s.bm);
}

static void gemm_cases() {
    Gemm q;
    gemm_line("gemm_base", q);
    q = Gemm(), q.K = 96, q.N = 8, q.ldc = 8, q.nj = 0, gemm_line("gemm_n8", q);
    q.N = 9, q.ldc = 9, gemm_line("gemm_n9", q);
    q = Gemm(), q.K = 2048, q.N = 8, q.ldc = 8, q.nj = 0, gemm_line("gemm_narrow_lds_at", q);        // K N 4 = 65536
    q.K = 3277, q.N = 5, q.ldc = 5, gemm_line("gemm_narrow_lds_past", q);                              // 65540
    q = Gemm(), q.K = 30, gemm_line("gemm_k_off", q);
    q = Gemm(), q.N = 30, gemm_line("gemm_n_off", q);
    q = Gemm(), q.a += 4, gemm_line("gemm_a_off", q);
    q = Gemm(), q.w += 4, gemm_line("gemm_w_off", q);
    q = Gemm(), q.c += 4, gemm_line("gemm_c_off", q);
    q = Gemm(), q.bias += 4, gemm_line("gemm_bias_off", q);
    q = Gemm(), q.tp = 0x50000, q.tps = 32, gemm_line("gemm_tp", q);
    q.tp += 4, gemm_line("gemm_tp_off", q);
    q = Gemm(), q.tp = 0x50000, q.tps = 34, gemm_line("gemm_tps_off", q);
    q = Gemm(), q.ldc = 34, gemm_line("gemm_ldc_off", q);
    q = Gemm(), q.nj = 0, gemm_line("gemm_unpacked", q);
    q = Gemm(), q.N = 128, q.ldc = 128, q.nj = 4, gemm_line("gemm_nj4", q);
    q = Gemm(), q.K = 4096, q.M = 131070, gemm_line("gemm_oor_below", q);      // (M + 1) K 4 = 2^31 - 16384
    q.M = 131071, gemm_line("gemm_oor_at", q);                                  // 2^31: and a three-way tie of heights
    q = Gemm(), q.sw = gen_switches("lds", nullptr), gemm_line("gemm_switch_lds", q);
    for (const char* bm : {"128", "64", "32", "48"}) {
        q = Gemm(), q.M = 153, q.sw = gen_switches("lds", bm);
        gemm_line((std::string("gemm_bm") + bm).c_str(), q);
    }
    q = Gemm(), q.sw = gen_switches(nullptr, "64"), gemm_line("gemm_bm64_sk", q);   // gemm_sk has no tile height
    switch_line("switch_unset", nullptr, nullptr);
    switch_line("switch_lds_64", "lds", "64");
    switch_line("switch_other", "sk", "48");
    // tile heights (no packed copy, so gemm<BM> runs)
    q = Gemm(), q.nj = 0, q.n_cu = 200, gemm_line("tile_119_200cu", q);
    q.n_cu = 256, gemm_line("tile_119_256cu", q);
    q = Gemm(), q.nj = 0, q.M = 128, q.n_cu = 1, gemm_line("tile_tie", q);         // 1 x 128 = 2 x 64 = 4 x 32
    q.M = 129, gemm_line("tile_129_1cu", q);                                        // 256, 192, 160
}

// hp against the layout's definition: element (k, n) at ((c NTp + t) 64 + l) 4 + s, k = 16c + 4 (l >> 4) + s,
// n = 16t + (l & 15); everything else zero
static bool pack_matches(const std::vector<GenPack>& packs, const std::vector<float>& arena, const std::vector<float>& hp) {
    std::vector<float> want(hp.size(), 0.f);
    for (const GenPack& p : packs) {
        const int NTp = ((p.N + 15) / 16 + p.NJ - 1) / p.NJ * p.NJ;
        for (int k = 0; k < p.K; ++k)
            for (int n = 0; n < p.N; ++n) {
                const int c = k / 16, l = 16 * ((k % 16) / 4) + n % 16, s = k % 4, t = n / 16;
                want[p.off + (((size_t)c * NTp + t) * 64 + l) * 4 + s] = arena[p.w + (size_t)k * p.N + n];
            }
    }
    return want == hp;
}

static void pack_cases() {
    // forward blocks, then one [20][48] block held transposed as the backward's arena holds it: [48][20]
    const int dims[5][2] = {{15, 32}, {36, 32}, {516, 1548}, {128, 384}, {48, 20}};
    std::vector<PackBlock> blocks;
    size_t o = 0;
    for (auto& d : dims) blocks.push_back({o, d[0], d[1]}), o += ((size_t)d[0] * d[1] + 3) / 4 * 4;
    std::vector<float> arena(o);
    uint32_t x = 99u;
    for (float& v : arena) x = x * 1664525u + 1013904223u, v = (float)(x >> 8) / 16777216.0f + 0.25f;   // never 0
    std::vector<GenPack> packs;
    std::vector<float> hp;
    const size_t floats = pack_plan(blocks, packs);
    pack_fill(packs, arena.data(), floats, hp);
    for (const GenPack& p : packs) printf("pack_%dx%d off=%zu NJ=%d\n", p.K, p.N, p.off, p.NJ);
    printf("pack_total packs=%zu floats=%zu match=%d skipped=%d found=%d\n", packs.size(), floats, (int)pack_matches(packs, arena, hp),
           (int)(find_pack(packs, 0, 15, 32) == nullptr),
           (int)(find_pack(packs, blocks[2].w, 516, 1548) == &packs[1] && !find_pack(packs, blocks[2].w, 516, 1544)));

    // gen_pack_blocks of the hid-32 g16 shape against the arithmetic gen_pack had before this file existed
    Stage s;
    stage_init(s, 32, 2, 17, 2, 5, 5, 0);
    std::vector<GenPack> was;
    size_t off = 0;
    auto add = [&](size_t w, int K, int N) {
        if (K % 4 || N % 4 || N <= 8) return;
        const int NT16 = (N + 15) / 16, NJ = NT16 % 4 == 0 ? 4 : 2, NTp = (NT16 + NJ - 1) / NJ * NJ;
        was.push_back(GenPack{w, off, K, N, NJ});
        off += (size_t)((K + 15) / 16) * NTp * 256;
    };
    for (const GenLayer& l : s.lay) {
        add(l.wqkv, 32, 96), add(l.wo, 32, 32), add(l.w1, 32, 64), add(l.w2, 64, 32);
        add(l.wc1, 96, 32), add(l.wc2, 96, 32);
    }
    add(s.win, 15, 32);
    const size_t now_floats = pack_plan(gen_pack_blocks(s), packs);
    bool same = packs.size() == was.size() && now_floats == off;
    for (size_t i = 0; same && i < was.size(); ++i)
        same = packs[i].w == was[i].w && packs[i].off == was[i].off && packs[i].K == was[i].K && packs[i].N == was[i].N &&
               packs[i].NJ == was[i].NJ;
    printf("pack_g16 packs=%zu floats=%zu same=%d\n", packs.size(), now_floats, (int)same);
}

static void stage_line(const char* name, const StageChoice& c) {
    printf("%s stage=%d lds=%zu blocks=%u\n", name, (int)c.stage, c.lds, c.blocks);
}
static void attn_line(const char* name, int N, int J, int D, int H, uintptr_t out) {
    const AttnChoice a = attention_choice(N, J, D, H, out);
    printf("%s %s ppb=%d blocks=%u lds=%zu\n", name, form_name(a.form), a.ppb, a.blocks, a.lds);
}
static void choice_cases() {
    attn_line("attn_w320", 5, 17, 320, 8, 0x1000);            // 17 x 964 floats: 16 bytes past 64 KB
    attn_line("attn_tt", 7, 17, 24, 2, 0x1000);
    attn_line("attn_tf", 7, 17, 36, 4, 0x1000);
    attn_line("attn_out_off", 7, 17, 24, 2, 0x1004);
    const AttnBwdChoice b = attention_bwd_choice(17, 320, 8), b2 = attention_bwd_choice(17, 32, 2),
                        b3 = attention_bwd_choice(32, 36, 4);
    printf("attn_bwd_w320 hb=%d stage=%d lds=%zu\n", b.hb, (int)b.stage, b.lds);
    printf("attn_bwd_g16 hb=%d stage=%d lds=%zu\n", b2.hb, (int)b2.stage, b2.lds);
    printf("attn_bwd_j32 hb=%d stage=%d lds=%zu\n", b3.hb, (int)b3.stage, b3.lds);
    stage_line("dlg_w320_2hid", dlg_choice(2, 17, 640));
    stage_line("dlg_w320_hid", dlg_choice(2, 17, 320));
    stage_line("dlg_n9", dlg_choice(9, 17, 32));
    stage_line("graph_w260_2hid", graph_choice(5, 32, 520));
    stage_line("graph_w260_hid", graph_choice(5, 32, 260));
    stage_line("cheb_w516_hid", cheb_choice(5, 32, 516));
    stage_line("cheb_w516_input", cheb_choice(5, 32, 5));
    const DwChoice v = dw_choice(119, 96, 32, 96, 32, 0x1000, 0x2000, 0x3000), sc = dw_choice(119, 96, 32, 96, 32, 0x1000, 0x2004, 0x3000),
                   k = dw_choice(680, 15, 32, 15, 32, 0x1000, 0x2000, 0x3000);
    printf("dw_vec vec=%d grid=%ux%u ps=%zu\n", (int)v.vec, v.nslab, v.gy, v.ps);
    printf("dw_g_off vec=%d grid=%ux%u ps=%zu\n", (int)sc.vec, sc.nslab, sc.gy, sc.ps);
    printf("dw_k15 vec=%d grid=%ux%u ps=%zu\n", (int)k.vec, k.nslab, k.gy, k.ps);
}

// bwd_plan's parts in the order it takes them, sizes from the comment above BwdLayerBufs
static void plan_line(const char* name, int D, int H, int L, int J, int cin, int N) {
    Stage s;
    stage_init(s, D, H, J, L, cin, cin, 0);
    std::vector<float> mem(bwd_plan(s, N, nullptr).floats + 64);
    float* base = mem.data() + (64 - (reinterpret_cast<uintptr_t>(mem.data()) / 4) % 64) % 64;     // 256-byte aligned
    const BwdPlan p = bwd_plan(s, N, base), z = bwd_plan(s, N, nullptr);
    const size_t M = (size_t)N * J, E = s.E, d = D, l = L, c = cin, n = N;
    std::vector<std::pair<float*, size_t>> parts;
    parts.push_back({p.Z0, M * 3 * c});
    for (const BwdLayerBufs& b : p.lay)
        for (auto q : std::initializer_list<std::pair<float*, size_t>>{{b.H, 1}, {b.Y0, 1}, {b.QKV, 3}, {b.A, 1}, {b.H1, 1}, {b.Y1, 1}, {b.G1, 1},
                                                                       {b.F, 2}, {b.G2, 2}, {b.H2, 1}, {b.Z1, 3}, {b.R1, 1}, {b.Z2, 3}, {b.R2, 1}})
            parts.push_back({q.first, M * d * q.second});
    parts.insert(parts.end(), {{p.Hlast, M * d}, {p.Zout, M * 3 * d}, {p.tproj, n * l * d}, {p.emb, n * d}, {p.u0, n * E}, {p.h0, n * E},
                               {p.u1, n * E}, {p.h1, n * E}});
    const size_t n_stash = parts.size();
    parts.insert(parts.end(), {{p.xt, M * c}, {p.eps, M * c}, {p.dEps, M * c}, {p.C1, M * d}, {p.dtp, n * l * d}, {p.dh, n * E}, {p.du, n * E},
                               {p.dH, M * d}, {p.tD1, M * d}, {p.tD2, M * d}, {p.t3D, M * 3 * d}, {p.t2Da, M * 2 * d}, {p.t2Db, M * 2 * d},
                               {p.Pdw, p.pdw_floats}, {p.Plg, 2 * ((n + 7) / 8) * J * J}});
    bool aligned = true, ordered = true;
    size_t at = 0, stash = 0, raw_stash = 0;
    for (size_t i = 0; i < parts.size(); ++i) {
        aligned = aligned && (reinterpret_cast<uintptr_t>(parts[i].first) & 255) == 0;
        ordered = ordered && parts[i].first == base + at;       // each part starts where the one before, rounded up, ends
        at += (parts[i].second + 63) / 64 * 64;
        if (i + 1 == n_stash) stash = at;
        if (i < n_stash) raw_stash += parts[i].second;
    }
    const bool formula = raw_stash == n * J * (22 * d * l + 4 * d + 3 * c) + n * (d + 4 * E + l * d);
    printf("%s stash=%zu floats=%zu aligned=%d ordered=%d stash_ok=%d floats_ok=%d formula=%d null_same=%d\n", name, p.stash_floats, p.floats,
           (int)aligned, (int)ordered, (int)(stash == p.stash_floats), (int)(at == p.floats), (int)formula,
           (int)(z.floats == p.floats && z.stash_floats == p.stash_floats && z.pdw_floats == p.pdw_floats && z.Z0 == nullptr));
}

int main() {
    gemm_cases();
    pack_cases();
    choice_cases();
    plan_line("plan_g16_n1", 32, 2, 2, 17, 5, 1);
    plan_line("plan_g16_n40", 32, 2, 2, 17, 5, 40);
    plan_line("plan_odd", 15, 3, 2, 17, 5, 7);
    return 0;
}
