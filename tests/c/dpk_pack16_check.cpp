// CPU check of the split-fp16 (gemm mode 1) weight arena at the widths other than the shipped one
// (tests/test_pack_half_widths_cpu.py builds and runs this under the host sanitizers).  For dpkw, dpkw4, dpkn
// and dpkn4 it packs an LCG state dict with pack(s, p, true) and reads the arena back by the layout that
// dpk_layout.inc documents and the kernel's B-fragment loads follow (gemmh_pass), written out here on its own:
//   layer l at l * LAYER16_BYTES, GEMM block set X at O16_X, block (ct, kb) at (ct * KB32 + kb) * 2 KiB,
//   the block = [hi 1 KiB | lo 1 KiB], lane l's 8 halves at l * 16 bytes: column n = 16 ct + (l & 15),
//   k = 32 kb + 4 g + i (i < 4) or 32 kb + 16 + 4 g + (i - 4) (i >= 4), g = l >> 4.
// Every element W_eff[k][n] of the six GEMMs of every layer must be there exactly once with
// (hi + lo) / 64 = W_eff[k][n] within the split's rounding (bound below), the layers past the model's zero.
#include <math.h>
#include <stdio.h>

#include "../../diffpose-nw_amd/csrc/dpk_stage.inc"

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
#undef DPK_NH
#undef DPK_D
#undef DPK_P
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

// what the reader below needs of one instance's layout
struct Lay {
    const char* name;
    int D, NH, NL;
    int o16[6];                   // QKV, O, fc1, fc2, Cheb1, Cheb2
    int layer_bytes, arena_bytes;
    const InstShape* shape;
};
#define LAY(ns)                                                                                               \
    Lay {                                                                                                     \
        #ns, ns::D, ns::NH, ns::NL, {ns::O16_QKV, ns::O16_O, ns::O16_FC1, ns::O16_FC2, ns::O16_C1, ns::O16_C2}, \
            ns::LAYER16_BYTES, ns::ARENA16_BYTES, &ns::SHAPE                                                  \
    }
static const Lay LAYS[4] = {LAY(dpkw), LAY(dpkw4), LAY(dpkn), LAY(dpkn4)};

// 16 bits of a 64-bit LCG (Knuth's MMIX constants) as a float in [-0.5, 0.5)
struct Lcg {
    uint64_t s;
    float next() {
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
    std::vector<float>& at(const std::string& name) {
        for (size_t i = 0; i < names.size(); ++i)
            if (names[i] == name) return data[i];
        static std::vector<float> none;
        return none;
    }
};

// GCNdiff's keys at hid D, 17 joints, L layers, coords 5 -> 5; weights of a few scales, so the split sees
// values whose lo part is fp16-normal, fp16-subnormal and zero
static StateDict make_state_dict(int D, int L, uint64_t seed) {
    Lcg r{seed};
    StateDict sd;
    const size_t d = (size_t)D, e = 4 * d;
    for (int l = 0; l < L; ++l) {
        const std::string at = "atten_layers." + std::to_string(l) + ".", gc = "gconv_layers." + std::to_string(l) + ".";
        for (int j = 0; j < 4; ++j) {
            sd.add(r, at + "self_attn.linears." + std::to_string(j) + ".weight", d * d, j == 1 ? 8.0f : 0.25f);
            sd.add(r, at + "self_attn.linears." + std::to_string(j) + ".bias", d, 0.125f);
        }
        sd.add(r, at + "feed_forward.A_hat", 17 * 17, 1.0f, 0.75f);
        sd.add(r, at + "feed_forward.gconv1.fc.weight", 2 * d * d, 0.25f);
        sd.add(r, at + "feed_forward.gconv1.fc.bias", 2 * d, 0.125f);
        sd.add(r, at + "feed_forward.gconv2.fc.weight", 2 * d * d, 1e-4f);
        sd.add(r, at + "feed_forward.gconv2.fc.bias", d, 0.125f);
        sd.add(r, at + "sublayer.0.norm.a_2", d, 0.5f, 1.0f);
        sd.add(r, at + "sublayer.0.norm.b_2", d, 0.25f);
        sd.add(r, at + "sublayer.1.norm.a_2", d, 0.5f, 1.0f);
        sd.add(r, at + "sublayer.1.norm.b_2", d, 0.25f);
        sd.add(r, gc + "gconv1.gconv.weight", 3 * d * d, 0.25f);
        sd.add(r, gc + "gconv1.gconv.bias", d, 0.125f);
        sd.add(r, gc + "gconv2.gconv.weight", 3 * d * d, 0.02f);
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

static std::vector<float> h36m_adjacency() {
    static const int edges[16][2] = {{0, 1}, {1, 2}, {2, 3}, {0, 4}, {4, 5}, {5, 6}, {0, 7}, {7, 8},
                                     {8, 9}, {9, 10}, {8, 11}, {11, 12}, {12, 13}, {8, 14}, {14, 15}, {15, 16}};
    std::vector<float> a(17 * 17, 0.f);
    for (int i = 0; i < 17; ++i) a[i * 17 + i] = 1.f;
    for (auto& e : edges) a[e[0] * 17 + e[1]] = a[e[1] * 17 + e[0]] = 1.f;
    return a;
}

static bool stage_model(Stage& s, const Lay& y, int L, StateDict& sd) {
    stage_init(s, y.D, y.NH, 17, L, 5, 5, 0);
    stage_set_graph(s, h36m_adjacency().data());
    std::vector<const char*> np;
    std::vector<const float*> dp;
    for (auto& n : sd.names) np.push_back(n.c_str());
    for (auto& v : sd.data) dp.push_back(v.data());
    std::string err;
    if (stage_load(s, np.data(), dp.data(), sd.numels.data(), (int)np.size(), err)) return true;
    printf("%s load failed: %s\n", y.name, err.c_str());
    return false;
}

static double half_bits(uint16_t b) { return (double)__builtin_bit_cast(_Float16, b); }

// The bound.  v = 64 w in fp32 (a power-of-two scale: exact below overflow).  hi = fp16(v), round to nearest:
// r = v - hi is exact in fp32 and |r| <= 2^-11 |v| where hi is fp16-normal, |r| <= 2^-25 (half the subnormal
// spacing 2^-24) otherwise.  lo = fp16(r) leaves |r - lo| <= 2^-11 |r| <= 2^-22 |v| where lo is normal and
// <= 2^-25 where it is subnormal.  So |v - (hi + lo)| <= max(2^-22 |v|, 2^-25), hi + lo summed exactly (double),
// and after the division by 64: |w - (hi + lo) / 64| <= max(2^-22 |w|, 2^-31).
static double split_bound(double w) { return fmax(ldexp(fabs(w), -22), ldexp(1.0, -31)); }

static int check_instance(const Lay& y, int L, uint64_t seed) {
    const int D = y.D;
    StateDict sd = make_state_dict(D, L, seed);
    Stage s;
    if (!stage_model(s, y, L, sd)) return 1;
    Packed p;
    y.shape->pack(s, p, true);
    const bool sized = p.a16.size() * 2 == (size_t)y.arena_bytes && y.shape->arena16_bytes == (size_t)y.arena_bytes &&
                       y.arena_bytes == y.NL * y.layer_bytes && y.arena_bytes > 0;
    printf("%s a16_bytes=%zu expected=%d sized=%d abf_empty=%d abf_bytes=%zu w16_ok=%d\n", y.name, p.a16.size() * 2,
           y.arena_bytes, (int)sized, (int)p.abf.empty(), y.shape->arenabf_bytes, (int)p.w16_ok);
    if (!sized) return 1;
    // the six GEMMs: K x N and where the staging holds W_eff[k][n] (row stride N); QKV carries LN0's gain
    const float* S = s.h.data();
    const int K[6] = {D, D, D, 2 * D, 3 * D, 3 * D}, N[6] = {3 * D, D, 2 * D, D, D, D};
    // the block sets tile the layer exactly, in this order
    bool tiled = y.o16[0] == 0;
    for (int g = 0; g < 6; ++g) {
        const int end = y.o16[g] + (N[g] / 16) * (K[g] / 32) * 2048;
        tiled = tiled && end == (g < 5 ? y.o16[g + 1] : y.layer_bytes);
    }
    long bad = 0, dup = 0, missing = 0, checked = 0, sub_lo = 0, zero_lo = 0;
    double worst = 0.0;    // largest error / bound
    for (int l = 0; l < L; ++l) {
        const GenLayer& o = s.lay[l];
        const size_t base[6] = {o.wqkv, o.wo, o.w1, o.w2, o.wc1, o.wc2};
        for (int g = 0; g < 6; ++g) {
            const int KB32 = K[g] / 32, NC = N[g] / 16;
            std::vector<int> seen((size_t)K[g] * N[g], 0);
            const uint16_t* blk0 = p.a16.data() + ((size_t)l * y.layer_bytes + y.o16[g]) / 2;
            for (int ct = 0; ct < NC; ++ct)
                for (int kb = 0; kb < KB32; ++kb) {
                    const uint16_t* blk = blk0 + (size_t)(ct * KB32 + kb) * 1024;     // 2 KiB = 1024 halves
                    for (int lane = 0; lane < 64; ++lane)
                        for (int i = 0; i < 8; ++i) {
                            const int grp = lane >> 4;
                            const int k = kb * 32 + (i < 4 ? 4 * grp + i : 16 + 4 * grp + (i - 4));
                            const int n = ct * 16 + (lane & 15);
                            const uint16_t hb = blk[lane * 8 + i], lb = blk[512 + lane * 8 + i];
                            float w = S[base[g] + (size_t)k * N[g] + n];
                            if (g == 0) w = S[o.n0a + k] * w;
                            const double got = (half_bits(hb) + half_bits(lb)) / 64.0;
                            const double err = fabs(got - (double)w), bound = split_bound(w);
                            worst = fmax(worst, err / bound);
                            if (!(err <= bound)) ++bad;
                            ++seen[(size_t)k * N[g] + n];
                            ++checked;
                            if ((lb & 0x7fff) == 0) ++zero_lo;
                            else if ((lb & 0x7c00) == 0) ++sub_lo;
                        }
                }
            for (int c : seen) {
                if (c == 0) ++missing;
                if (c > 1) ++dup;
            }
        }
    }
    long nonzero_past = 0;      // layers past the model's: zero blocks
    for (size_t i = (size_t)L * y.layer_bytes / 2; i < p.a16.size(); ++i) nonzero_past += p.a16[i] != 0;
    printf("%s-values layers=%d checked=%ld bad=%ld missing=%ld dup=%ld tiled=%d past=%ld worst_over_bound=%.3f "
           "sub_lo=%d zero_lo=%d\n",
           y.name, L, checked, bad, missing, dup, (int)tiled, nonzero_past, worst, (int)(sub_lo > 0), (int)(zero_lo > 0));
    // a GEMM weight at 1016.0 (64 w = 65024, past the split's range) turns w16_ok off; without the half-width
    // arenas nothing is packed or judged
    sd.at("gconv_layers.0.gconv2.gconv.weight")[5] = 1016.0f;
    Stage s2;
    if (!stage_model(s2, y, L, sd)) return 1;
    Packed big, none;
    y.shape->pack(s2, big, true);
    y.shape->pack(s2, none, false);
    printf("%s-range w16_ok=%d plain_a16_empty=%d plain_abf_empty=%d\n", y.name, (int)big.w16_ok, (int)none.a16.empty(),
           (int)none.abf.empty());
    return 0;
}

int main() {
    int rc = 0;
    // dpkw at 3 of its 5 layers (the rest of the arena stays zero), the others at 5, 2 and 5
    static const int layers[4] = {3, 5, 2, 5};
    for (int i = 0; i < 4; ++i) rc |= check_instance(LAYS[i], layers[i], 11 + i);
    return rc;
}
