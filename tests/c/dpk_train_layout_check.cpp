// The host description of dpk_train_apply's refresh as a stand-alone program (tests/test_device_optim_cpu.py):
// csrc/dpk_stage.inc, dpk_genplan.inc, dpk_grad_layout.inc and dpk_train_layout.inc alone, no HIP.  For the shape on the
// command line it fills a flat parameter array (dpk_param_layout's order, zero padding) from an LCG, builds the four
// arenas twice -- through stage_load + pack_fill + bwd_arena_build + pack_fill, as a weight load does, and through
// train_layout's per-float sources from the flat array, as the refresh does -- and compares them bit for bit.  Every
// destination float must be sourced, or unchanged and either zero padding, a Chebyshev term or the zero row.
//   dpk_train_layout_check D H J L coords
#include <stdio.h>
#include <stdlib.h>

#include "../../diffpose-nw_amd/csrc/dpk_stage.inc"
#include "../../diffpose-nw_amd/csrc/dpk_genplan.inc"
#include "../../diffpose-nw_amd/csrc/dpk_grad_layout.inc"
#include "../../diffpose-nw_amd/csrc/dpk_train_layout.inc"

static long differ(const char* what, const std::vector<float>& got, const std::vector<float>& want) {
    long bad = got.size() == want.size() ? 0 : 1;
    for (size_t i = 0; i < got.size() && i < want.size(); ++i)
        if (memcmp(&got[i], &want[i], 4) != 0 && bad++ == 0) printf("%s: first mismatch at %zu: %a, expected %a\n", what, i, got[i], want[i]);
    printf("%s floats %zu mismatches %ld\n", what, want.size(), bad);
    return bad;
}

int main(int argc, char** argv) {
    if (argc != 6) {
        fprintf(stderr, "usage: %s D H J L coords\n", argv[0]);
        return 2;
    }
    const int D = atoi(argv[1]), H = atoi(argv[2]), J = atoi(argv[3]), L = atoi(argv[4]), C = atoi(argv[5]);
    Stage s;
    stage_init(s, D, H, J, L, C, C, 0);
    const GradLayout g = grad_layout(s);
    // the flat array: LCG values in (-0.5, 0.5); A_hat gets a large diagonal so the column sums stay positive
    std::vector<float> flat(g.floats, 0.f);
    std::vector<const char*> names;
    std::vector<const float*> ptrs;
    std::vector<int64_t> numels;
    uint32_t x = 4242u + 7u * (uint32_t)D + (uint32_t)J;
    for (const GradEntry& e : g.e) {
        float* v = flat.data() + e.offset;
        for (int64_t i = 0; i < e.numel; ++i) {
            x = x * 1664525u + 1013904223u;
            v[i] = (float)(x >> 8) / 16777216.0f - 0.5f;
        }
        if (e.name.size() > 5 && e.name.compare(e.name.size() - 5, 5, "A_hat") == 0)
            for (int j = 0; j < J; ++j) v[(size_t)j * J + j] += 1.5f + (float)J;
        names.push_back(e.name.c_str()), ptrs.push_back(v), numels.push_back(e.numel);
    }
    std::vector<float> adj((size_t)J * J, 0.f);
    for (int i = 0; i < J; ++i)
        for (int j = 0; j < J; ++j) adj[(size_t)i * J + j] = (i == j || i + 1 == j || j + 1 == i) ? 1.0f / 3.0f : 0.f;
    stage_set_graph(s, adj.data());
    // ---- as a weight load builds them
    std::string err;
    if (!stage_load(s, names.data(), ptrs.data(), numels.data(), (int)names.size(), err)) {
        printf("load failed: %s\n", err.c_str());
        return 1;
    }
    std::vector<GenPack> fpk, bpk;
    std::vector<float> want_fp, want_bp;
    pack_fill(fpk, s.h.data(), pack_plan(gen_pack_blocks(s), fpk), want_fp);
    BwdArena a;
    bwd_arena_build(s, a);
    std::vector<PackBlock> tb;
    for (const BwdBlock& k : a.blocks) tb.push_back({k.w, k.N, k.K});
    pack_fill(bpk, a.h.data(), pack_plan(tb, bpk), want_bp);
    // ---- as the refresh builds them: from arenas that hold what does not come from the parameters (the graph's
    // terms, zeros elsewhere), every sourced float poisoned first so that an unsourced one shows
    const TrainLayout t = train_layout(s);
    long bad = t.F == g.floats && (int)t.ahat.size() == L ? 0 : 1;
    Stage blank;
    stage_init(blank, D, H, J, L, C, C, 0);
    stage_set_graph(blank, adj.data());
    struct Arena {
        const char* name;
        const std::vector<int32_t>& idx;
        const std::vector<float>& want;
        std::vector<float> got;
    } arenas[4] = {{"forward", t.fwd, s.h, blank.h},
                   {"forward_packed", t.fwdp, want_fp, std::vector<float>(want_fp.size(), 0.f)},
                   {"transposed", t.bwd, a.h, std::vector<float>(a.floats, 0.f)},
                   {"transposed_packed", t.bwdp, want_bp, std::vector<float>(want_bp.size(), 0.f)}};
    std::copy(blank.h.begin(), blank.h.end(), arenas[2].got.begin());
    for (Arena& r : arenas) {
        if (r.idx.size() != r.want.size()) {
            printf("%s: %zu sources for %zu floats\n", r.name, r.idx.size(), r.want.size());
            return 1;
        }
        long sourced = 0, lg = 0, kept_nonzero = 0;
        for (size_t i = 0; i < r.idx.size(); ++i) {
            const int32_t c = r.idx[i];
            if (c >= 0 && (size_t)c >= t.F) bad++, printf("%s: source %d of float %zu is past the flat array\n", r.name, c, i);
            if (c <= TRAIN_LG && TRAIN_LG - c >= L * J * J) bad++, printf("%s: Laplacian element %d of float %zu\n", r.name, TRAIN_LG - c, i);
            if (c != TRAIN_KEEP) r.got[i] = -12345.0f, ++sourced;
            if (c <= TRAIN_LG) ++lg;
            if (c == TRAIN_KEEP && r.want[i] != 0.f) ++kept_nonzero;
        }
        if (bad) return 1;
        train_gather(t, r.idx, flat.data(), r.got.data());
        bad += differ(r.name, r.got, r.want);
        printf("%s sourced %ld laplacian %ld kept_nonzero %ld\n", r.name, sourced, lg, kept_nonzero);
    }
    // the unchanged floats that are not zero are the Chebyshev terms, in the two arenas that hold them
    long cheb = 0;
    for (int e = 0; e < 2 * J * J; ++e) cheb += s.h[(e < J * J ? s.t1 : s.t2 - J * J) + e] != 0.f;
    printf("cheb_nonzero %ld\n", cheb);
    // every parameter is read by the forward arena
    std::vector<char> used(t.F, 0);
    for (int32_t c : t.fwd)
        if (c >= 0) used[c] = 1;
    for (int l = 0; l < L; ++l)
        for (int e = 0; e < J * J; ++e) used[t.ahat[l] + e] = 1;
    long unused = 0;
    for (const GradEntry& e : g.e)
        for (int64_t i = 0; i < e.numel; ++i) unused += !used[e.offset + i];
    printf("unused_params %ld\n", unused);
    // the Laplacian restated: stage_load's, bit for bit
    long lgbad = 0;
    for (int l = 0; l < L; ++l)
        for (int i = 0; i < J; ++i)
            for (int j = 0; j < J; ++j) {
                const float v = train_lg(flat.data() + t.ahat[l], J, i, j);
                lgbad += memcmp(&v, &s.h[s.lay[l].lg + i * J + j], 4) != 0;
            }
    printf("laplacian mismatches %ld\n", lgbad);
    // the decimal reading of the optimiser's constants
    const bool dec = train_decimal(0.9f) == 0.9 && train_decimal(0.999f) == 0.999 && train_decimal(0.5f) == 0.5 &&
                     train_decimal(0.f) == 0.0 && train_decimal(1e-8f) == 1e-8;
    printf("decimal %s\n", dec ? "ok" : "wrong");
    return bad || lgbad || unused || !dec ? 1 : 0;
}
