// CPU check of the host packer for padded tiles: a GCNdiff model of n < 17 joints packed into a sampler
// instance's 17-joint arena (dpk_pack.inc: graph matrices read at stride n and zero-embedded), and which
// configs the instance table accepts for such models.  tests/test_pack_padded_cpu.py builds this with the host
// sanitizers; every check prints one line, a failure is the exit code.
// Plain C++, no HIP: clang++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined
#include <stdio.h>

#include "../../diffpose-nw_amd/csrc/dpk_stage.inc"

// the table's instances (dpk_kernels.hip: INSTANCES), as tests/c/dpk_pack_check.cpp includes them
#define DPK_P 4
namespace dpk {
#include "../../diffpose-nw_amd/csrc/dpk_layout.inc"
#include "../../diffpose-nw_amd/csrc/dpk_genfused.inc"
}  // namespace dpk
#undef DPK_P
#undef DPK_D
#undef DPK_NH
#define DPK_P 2
#define DPK_D 128
#define DPK_NH 8
namespace dpkw {
#include "../../diffpose-nw_amd/csrc/dpk_layout.inc"
#include "../../diffpose-nw_amd/csrc/dpk_genfused.inc"
}  // namespace dpkw
#undef DPK_NH
#define DPK_NH 4
namespace dpkw4 {
#include "../../diffpose-nw_amd/csrc/dpk_layout.inc"
#include "../../diffpose-nw_amd/csrc/dpk_genfused.inc"
}  // namespace dpkw4
#undef DPK_P
#undef DPK_D
#undef DPK_NH
#define DPK_P 4
#define DPK_D 64
#define DPK_NH 2
namespace dpkn {
#include "../../diffpose-nw_amd/csrc/dpk_layout.inc"
#include "../../diffpose-nw_amd/csrc/dpk_genfused.inc"
}  // namespace dpkn
#undef DPK_NH
#define DPK_NH 4
namespace dpkn4 {
#include "../../diffpose-nw_amd/csrc/dpk_layout.inc"
#include "../../diffpose-nw_amd/csrc/dpk_genfused.inc"
}  // namespace dpkn4
static const InstShape* const SHAPES[] = {&dpk::SHAPE, &dpkw::SHAPE, &dpkw4::SHAPE, &dpkn::SHAPE, &dpkn4::SHAPE};

struct Lcg {
    uint64_t s;
    float next() {   // 16 bits of a 64-bit LCG as a float in [-0.5, 0.5), exact in fp32
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        return (float)((int)((s >> 40) & 0xffff) - 32768) * (1.0f / 65536.0f);
    }
};

struct StateDict {
    std::vector<std::string> names;
    std::vector<std::vector<float>> data;
    std::vector<int64_t> numels;
    void add(Lcg& r, const std::string& name, size_t n, float scale, float shift = 0.f) {
        std::vector<float> v(n);
        for (float& x : v) x = scale * r.next() + shift;
        names.push_back(name);
        data.push_back(std::move(v));
        numels.push_back((int64_t)n);
    }
};

// the keys and sizes of models/gcndiff.py at hid D, J joints, L layers.  The A_hat entries are drawn last, from
// a generator of their own, so two dicts of one seed and different J share every other value
static StateDict make_state_dict(int D, int J, int L, uint64_t seed) {
    Lcg r{seed}, ra{seed ^ 0x9e3779b97f4a7c15ULL};
    StateDict sd;
    const size_t d = (size_t)D, e = 4 * d;
    for (int l = 0; l < L; ++l) {
        const std::string at = "atten_layers." + std::to_string(l) + ".", gc = "gconv_layers." + std::to_string(l) + ".";
        for (int j = 0; j < 4; ++j) {
            sd.add(r, at + "self_attn.linears." + std::to_string(j) + ".weight", d * d, 0.25f);
            sd.add(r, at + "self_attn.linears." + std::to_string(j) + ".bias", d, 0.125f);
        }
        sd.add(ra, at + "feed_forward.A_hat", (size_t)J * J, 1.0f, 0.75f);   // positive column sums
        sd.add(r, at + "feed_forward.gconv1.fc.weight", 2 * d * d, 0.25f);
        sd.add(r, at + "feed_forward.gconv1.fc.bias", 2 * d, 0.125f);
        sd.add(r, at + "feed_forward.gconv2.fc.weight", 2 * d * d, 0.25f);
        sd.add(r, at + "feed_forward.gconv2.fc.bias", d, 0.125f);
        sd.add(r, at + "sublayer.0.norm.a_2", d, 0.5f, 1.0f);
        sd.add(r, at + "sublayer.0.norm.b_2", d, 0.25f);
        sd.add(r, at + "sublayer.1.norm.a_2", d, 0.5f, 1.0f);
        sd.add(r, at + "sublayer.1.norm.b_2", d, 0.25f);
        sd.add(r, gc + "gconv1.gconv.weight", 3 * d * d, 0.25f);
        sd.add(r, gc + "gconv1.gconv.bias", d, 0.125f);
        sd.add(r, gc + "gconv2.gconv.weight", 3 * d * d, 0.25f);
        sd.add(r, gc + "gconv2.gconv.bias", d, 0.125f);
        sd.add(r, gc + "temb_proj.weight", d * e, 0.25f);
        sd.add(r, gc + "temb_proj.bias", d, 0.125f);
    }
    sd.add(r, "gconv_input.weight", 3 * 5 * d, 0.25f);
    sd.add(r, "gconv_input.bias", d, 0.125f);
    sd.add(r, "gconv_output.weight", 3 * d * 5, 0.25f);
    sd.add(r, "gconv_output.bias", 5, 0.125f);
    sd.add(r, "temb.dense.0.weight", e * d, 0.25f);
    sd.add(r, "temb.dense.0.bias", e, 0.125f);
    sd.add(r, "temb.dense.1.weight", e * e, 0.25f);
    sd.add(r, "temb.dense.1.bias", e, 0.125f);
    return sd;
}

// a chain 0-1-...-(n-1) with self loops plus the chord 0-(n-1) (n > 2): no sub-graph of the H36M tree
static std::vector<float> ring_adjacency(int n) {
    std::vector<float> a((size_t)n * n, 0.f);
    for (int i = 0; i < n; ++i) a[i * n + i] = 1.f;
    for (int i = 0; i + 1 < n; ++i) a[i * n + i + 1] = a[(i + 1) * n + i] = 1.f;
    if (n > 2) a[n - 1] = a[(n - 1) * n] = 1.f;
    return a;
}

static bool load(Stage& s, const StateDict& sd) {
    std::vector<const char*> np;
    std::vector<const float*> dp;
    for (auto& n : sd.names) np.push_back(n.c_str());
    for (auto& v : sd.data) dp.push_back(v.data());
    std::string err;
    const bool ok = stage_load(s, np.data(), dp.data(), sd.numels.data(), (int)np.size(), err);
    if (!ok) printf("load failed: %s\n", err.c_str());
    return ok;
}

// The arena packed from an n-joint staging against the arena of a 17-joint staging of the same weights whose
// T1, T2 and every layer's L_g were overwritten with the zero-embedded n-joint ones: float for float.
static int run_embed(const char* tag, const InstShape& sh, int L, int n, uint64_t seed) {
    const int D = sh.D, H = sh.NH;
    Stage sn, s17;
    stage_init(sn, D, H, n, L, 5, 5, 0);
    stage_init(s17, D, H, 17, L, 5, 5, 0);
    stage_set_graph(sn, ring_adjacency(n).data());
    stage_set_graph(s17, ring_adjacency(17).data());
    if (!load(sn, make_state_dict(D, n, L, seed)) || !load(s17, make_state_dict(D, 17, L, seed))) return 1;
    auto embed = [&](size_t from, size_t to) {
        for (int i = 0; i < 17; ++i)
            for (int j = 0; j < 17; ++j)
                s17.h[to + (size_t)i * 17 + j] = (i < n && j < n) ? sn.h[from + (size_t)i * n + j] : 0.f;
    };
    embed(sn.t1, s17.t1);
    embed(sn.t2, s17.t2);
    for (int l = 0; l < L; ++l) embed(sn.lay[l].lg, s17.lay[l].lg);
    // every other staged value is the same in both (one seed): the two arenas can only differ in the graph terms
    bool same_w = true;
    for (size_t i = 0; i < (size_t)D * 3 * D; ++i) same_w = same_w && sn.h[sn.lay[0].wqkv + i] == s17.h[s17.lay[0].wqkv + i];
    Packed pn, p17;
    sh.pack(sn, pn, true);
    sh.pack(s17, p17, true);
    const bool arena = pn.arena.size() == sh.arena_floats && pn.arena.size() == p17.arena.size() &&
                       memcmp(pn.arena.data(), p17.arena.data(), pn.arena.size() * 4) == 0;
    const bool rest = pn.temb == p17.temb && pn.a16 == p17.a16 && pn.abf == p17.abf;
    // the embedded graph terms are not all zero (a packer that dropped them would pass the comparison above
    // only if the 17-joint side dropped them too)
    bool nonzero = false;
    for (int i = 0; i < n * n; ++i) nonzero = nonzero || sn.h[sn.t2 + i] != 0.f;
    const bool ok = same_w && arena && rest && nonzero && !pn.sparse;
    printf("%s same_weights=%d arena_equal=%d others_equal=%d sparse=%d ok=%d\n", tag, (int)same_w, (int)arena, (int)rest,
           (int)pn.sparse, (int)ok);
    return ok ? 0 : 1;
}

// An n-joint sub-tree of the H36M skeleton (its first n joints) fits the compiled sparse pattern once embedded;
// the padded kernels are dense ones, so the packer must still say sparse = false.
static int run_subtree(const char* tag, int n) {
    static const int edges[16][2] = {{0, 1}, {1, 2}, {2, 3}, {0, 4}, {4, 5}, {5, 6}, {0, 7}, {7, 8},
                                     {8, 9}, {9, 10}, {8, 11}, {11, 12}, {12, 13}, {8, 14}, {14, 15}, {15, 16}};
    std::vector<float> a((size_t)n * n, 0.f);
    for (int i = 0; i < n; ++i) a[i * n + i] = 1.f;
    for (auto& e : edges)
        if (e[0] < n && e[1] < n) a[e[0] * n + e[1]] = a[e[1] * n + e[0]] = 1.f;
    Stage s;
    stage_init(s, 96, 4, n, 1, 5, 5, 0);
    stage_set_graph(s, a.data());
    if (!load(s, make_state_dict(96, n, 1, 3))) return 1;
    Packed p;
    dpk::SHAPE.pack(s, p, false);
    printf("%s sparse=%d\n", tag, (int)p.sparse);
    return p.sparse ? 1 : 0;
}

// which configs the table's entries accept: a GCNdiff shape on 2..17 joints exactly its own entry, GCNpose 17
// joints alone, other widths none
static int run_table_fits() {
    auto accepts = [](int D, int H, int J, int L, int kind) {      // bit i: entry i accepts
        int bits = 0;
        for (int i = 0; i < 5; ++i)
            if (SHAPES[i]->fits(D, H, J, L, kind ? 2 : 5, kind ? 3 : 5, kind)) bits |= 1 << i;
        return bits;
    };
    static const int shapes[5][2] = {{96, 4}, {128, 8}, {128, 4}, {64, 2}, {64, 4}};
    bool ok = true;
    for (int i = 0; i < 5; ++i)
        for (int n : {2, 15, 16, 17})
            for (int L : {1, 5}) ok = ok && accepts(shapes[i][0], shapes[i][1], n, L, 0) == 1 << i;
    ok = ok && accepts(48, 4, 16, 1, 0) == 0;                       // no instance of that width
    ok = ok && accepts(96, 4, 16, 4, 1) == 0 && accepts(96, 4, 17, 4, 1) == 1;   // GCNpose: 17 joints alone
    ok = ok && accepts(96, 4, 1, 1, 0) == 0 && accepts(96, 4, 18, 1, 0) == 0 && accepts(96, 4, 16, 6, 0) == 0;
    printf("table ok=%d\n", (int)ok);
    return ok ? 0 : 1;
}

int main() {
    int rc = 0;
    rc |= run_table_fits();
    rc |= run_embed("embed-h96-n16", dpk::SHAPE, 3, 16, 11);
    rc |= run_embed("embed-h96-n2", dpk::SHAPE, 2, 2, 12);
    rc |= run_embed("embed-h128-n16", dpkw::SHAPE, 1, 16, 13);
    rc |= run_embed("embed-h64-n2", dpkn::SHAPE, 2, 2, 14);
    rc |= run_subtree("subtree-n16", 16);
    return rc;
}
