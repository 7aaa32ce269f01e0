// CPU check of the host weight packer: the staging (dpk_stage.inc) and every sampler instance's
// pack_model (dpk_pack.inc over dpk_layout.inc) on state dicts from a fixed integer LCG.  Prints one
// FNV-1a-64 digest per packed buffer; tests/test_pack_cpu.py builds this with the host sanitizers and
// compares the digests with the ones recorded from the loaders this packer replaced.  Also checks which
// configs the instance table accepts (the shape halves of its descriptors); a failure there is the exit code.
// Plain C++, no HIP: clang++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined
#include <stdio.h>

#include "../../diffpose-nw_amd/csrc/dpk_stage.inc"

// the table's instances (dpk_kernels.hip: INSTANCES), each one's layout, packer and the shape half of its
// descriptor (SHAPE, dpk_genfused.inc)
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

// ---- inputs: state dicts and adjacencies from a fixed integer LCG (no file input) ----
struct Lcg {
    uint64_t s;
    // 16 bits of a 64-bit LCG (Knuth's MMIX constants) as a float in [-0.5, 0.5), exact in fp32
    float next() {
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        return (float)((int)((s >> 40) & 0xffff) - 32768) * (1.0f / 65536.0f);
    }
};

struct StateDict {
    std::vector<std::string> names;
    std::vector<std::vector<float>> data;
    std::vector<int64_t> numels;
    // n values scale * u + shift, u in [-0.5, 0.5)
    void add(Lcg& r, const std::string& name, size_t n, float scale, float shift = 0.f) {
        std::vector<float> v(n);
        for (float& x : v) x = scale * r.next() + shift;
        names.push_back(name);
        data.push_back(std::move(v));
        numels.push_back((int64_t)n);
    }
    int find(const std::string& name) const {
        for (size_t i = 0; i < names.size(); ++i)
            if (names[i] == name) return (int)i;
        return -1;
    }
    void erase(const std::string& name) {
        const int i = find(name);
        names.erase(names.begin() + i);
        data.erase(data.begin() + i);
        numels.erase(numels.begin() + i);
    }
    std::vector<const char*> name_ptrs() const {
        std::vector<const char*> p;
        for (auto& s : names) p.push_back(s.c_str());
        return p;
    }
    std::vector<const float*> data_ptrs() const {
        std::vector<const float*> p;
        for (auto& v : data) p.push_back(v.data());
        return p;
    }
};

// the keys and sizes of models/gcndiff.py (kind 0) / gcnpose.py (kind 1) at hid D, J joints, L layers
static StateDict make_state_dict(int D, int J, int L, int cin, int cout, int kind, uint64_t seed) {
    Lcg r{seed};
    StateDict sd;
    const size_t d = (size_t)D, e = 4 * d;
    for (int l = 0; l < L; ++l) {
        const std::string at = "atten_layers." + std::to_string(l) + ".", gc = "gconv_layers." + std::to_string(l) + ".";
        for (int j = 0; j < 4; ++j) {
            sd.add(r, at + "self_attn.linears." + std::to_string(j) + ".weight", d * d, 0.25f);
            sd.add(r, at + "self_attn.linears." + std::to_string(j) + ".bias", d, 0.125f);
        }
        sd.add(r, at + "feed_forward.A_hat", (size_t)J * J, 1.0f, 0.75f);   // positive column sums
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
        if (kind == 0) {
            sd.add(r, gc + "temb_proj.weight", d * e, 0.25f);
            sd.add(r, gc + "temb_proj.bias", d, 0.125f);
        }
    }
    sd.add(r, "gconv_input.weight", 3 * (size_t)cin * d, 0.25f);
    sd.add(r, "gconv_input.bias", d, 0.125f);
    sd.add(r, "gconv_output.weight", 3 * d * cout, 0.25f);
    sd.add(r, "gconv_output.bias", (size_t)cout, 0.125f);
    if (kind == 0) {
        sd.add(r, "temb.dense.0.weight", e * d, 0.25f);
        sd.add(r, "temb.dense.0.bias", e, 0.125f);
        sd.add(r, "temb.dense.1.weight", e * e, 0.25f);
        sd.add(r, "temb.dense.1.bias", e, 0.125f);
    }
    return sd;
}

// the 17-joint Human3.6M skeleton with self loops, plus optionally one more (symmetric) edge
static std::vector<float> make_adjacency(int extra_a = -1, int extra_b = -1) {
    static const int edges[16][2] = {{0, 1}, {1, 2}, {2, 3}, {0, 4}, {4, 5}, {5, 6}, {0, 7}, {7, 8},
                                     {8, 9}, {9, 10}, {8, 11}, {11, 12}, {12, 13}, {8, 14}, {14, 15}, {15, 16}};
    std::vector<float> a(17 * 17, 0.f);
    for (int i = 0; i < 17; ++i) a[i * 17 + i] = 1.f;
    for (auto& e : edges) a[e[0] * 17 + e[1]] = a[e[1] * 17 + e[0]] = 1.f;
    if (extra_a >= 0) a[extra_a * 17 + extra_b] = a[extra_b * 17 + extra_a] = 1.f;
    return a;
}

static uint64_t fnv1a(const void* p, size_t bytes) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    uint64_t h = 14695981039346656037ULL;
    for (size_t i = 0; i < bytes; ++i) h = (h ^ b[i]) * 1099511628211ULL;
    return h;
}
template <class T>
static uint64_t digest(const std::vector<T>& v) { return fnv1a(v.data(), v.size() * sizeof(T)); }

static bool load(Stage& s, const StateDict& sd, std::string& err) {
    const auto np = sd.name_ptrs();
    const auto dp = sd.data_ptrs();
    return stage_load(s, np.data(), dp.data(), sd.numels.data(), (int)np.size(), err);
}

// graph, then weights, then the instance's pack: one line of digests
template <class Pack>
static int run(const char* tag, int D, int H, int L, int kind, uint64_t seed, const std::vector<float>& adj, bool big,
               bool half_modes, Pack pack) {
    const int cin = kind ? 2 : 5, cout = kind ? 3 : 5;
    Stage s;
    stage_init(s, D, H, 17, L, cin, cout, kind);
    StateDict sd = make_state_dict(D, 17, L, cin, cout, kind, seed);
    if (big) sd.data[sd.find("atten_layers.0.self_attn.linears.3.weight")][0] = 1016.0f;
    stage_set_graph(s, adj.data());
    std::string err;
    if (!load(s, sd, err)) {
        printf("%s load failed: %s\n", tag, err.c_str());
        return 1;
    }
    Packed p;
    pack(s, p, half_modes);
    printf("%s arena=%016llx temb=%016llx", tag, (unsigned long long)digest(p.arena), (unsigned long long)digest(p.temb));
    if (half_modes) printf(" a16=%016llx abf=%016llx", (unsigned long long)digest(p.a16), (unsigned long long)digest(p.abf));
    else if (!p.a16.empty() || !p.abf.empty()) printf(" unexpected-half-arenas");
    printf(" sparse=%d w16_ok=%d\n", (int)p.sparse, (int)p.w16_ok);
    return 0;
}

// (g) a failed load names the key and leaves the staging as it was
static int run_failed_loads() {
    Stage s;
    stage_init(s, 96, 4, 17, 5, 5, 5, 0);
    stage_set_graph(s, make_adjacency().data());
    std::string err;
    if (!load(s, make_state_dict(96, 17, 5, 5, 5, 0, 1), err)) return 1;
    const uint64_t before = digest(s.h);
    StateDict other = make_state_dict(96, 17, 5, 5, 5, 0, 7);     // other values: a partial write would show
    StateDict missing = other, wrong = other;
    missing.erase("gconv_layers.3.gconv2.gconv.bias");
    const int i = wrong.find("atten_layers.4.feed_forward.gconv2.fc.weight");
    wrong.data[i].pop_back();
    wrong.numels[i] -= 1;
    const bool ok1 = load(s, missing, err);
    printf("g-missing ok=%d unchanged=%d err=%s\n", (int)ok1, (int)(digest(s.h) == before), err.c_str());
    const bool ok2 = load(s, wrong, err);
    printf("g-wrong ok=%d unchanged=%d err=%s\n", (int)ok2, (int)(digest(s.h) == before), err.c_str());
    const bool ok3 = load(s, other, err);
    printf("g-full ok=%d unchanged=%d\n", (int)ok3, (int)(digest(s.h) == before));
    return 0;
}

// (h) which configs the table's entries accept: every compiled GCNdiff shape exactly one, GCNpose the shipped
// entry only, anything else none
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
        for (int L = 1; L <= 5; ++L) ok = ok && accepts(shapes[i][0], shapes[i][1], 17, L, 0) == 1 << i;
    for (int L = 1; L <= 5; ++L) ok = ok && accepts(96, 4, 17, L, 1) == 1;
    ok = ok && accepts(48, 4, 16, 1, 0) == 0 && accepts(96, 4, 17, 6, 0) == 0 && accepts(128, 8, 17, 5, 1) == 0;
    printf("h-table ok=%d\n", (int)ok);
    return ok ? 0 : 1;
}

int main() {
    const std::vector<float> h36m = make_adjacency(), dense = make_adjacency(3, 6);
    int rc = 0;
    rc |= run("a", 96, 4, 5, 0, 1, h36m, false, true, dpk::SHAPE.pack);
    rc |= run("b", 96, 4, 3, 0, 2, dense, false, true, dpk::SHAPE.pack);
    rc |= run("c", 96, 4, 4, 1, 3, h36m, false, true, dpk::SHAPE.pack);
    rc |= run("d", 96, 4, 5, 0, 1, h36m, true, true, dpk::SHAPE.pack);
    rc |= run("e", 128, 8, 3, 0, 5, h36m, false, false, dpkw::SHAPE.pack);
    rc |= run("f", 64, 2, 5, 0, 6, h36m, false, false, dpkn::SHAPE.pack);
    rc |= run_failed_loads();
    rc |= run_table_fits();
    return rc;
}
