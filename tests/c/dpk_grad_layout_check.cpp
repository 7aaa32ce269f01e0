// The host half of dpk_diff_loss_grad as a stand-alone program (tests/test_diff_grad_cpu.py): csrc/dpk_stage.inc and
// csrc/dpk_grad_layout.inc alone, no HIP.  For the shape on the command line it prints the gradient layout table
// and the transposed arena's block list, loads an LCG-built state dict whose keys are the table's names through
// stage_load, and writes the staging, the transposed arena and the state dict's values as raw float32 files.
//   dpk_grad_layout_check D H J L coords OUTDIR
#include <stdio.h>
#include <stdlib.h>

#include "../../diffpose-nw_amd/csrc/dpk_stage.inc"
#include "../../diffpose-nw_amd/csrc/dpk_grad_layout.inc"

static bool dump(const std::string& path, const std::vector<float>& v) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(v.data(), sizeof(float), v.size(), f) == v.size();
    return fclose(f) == 0 && ok;
}

int main(int argc, char** argv) {
    if (argc != 7) {
        fprintf(stderr, "usage: %s D H J L coords OUTDIR\n", argv[0]);
        return 2;
    }
    const int D = atoi(argv[1]), H = atoi(argv[2]), J = atoi(argv[3]), L = atoi(argv[4]), C = atoi(argv[5]);
    const std::string out = argv[6];
    Stage s;
    stage_init(s, D, H, J, L, C, C, 0);
    const GradLayout g = grad_layout(s);
    // a state dict of the table's names: LCG values in (-0.5, 0.5); A_hat gets a unit diagonal so column sums stay positive
    std::vector<std::vector<float>> vals(g.e.size());
    std::vector<const char*> names;
    std::vector<const float*> ptrs;
    std::vector<int64_t> numels;
    uint32_t x = 12345u + 7u * (uint32_t)D + (uint32_t)J;
    std::vector<float> flat;
    for (size_t i = 0; i < g.e.size(); ++i) {
        vals[i].resize((size_t)g.e[i].numel);
        for (float& v : vals[i]) {
            x = x * 1664525u + 1013904223u;
            v = (float)(x >> 8) / 16777216.0f - 0.5f;
        }
        const std::string& nm = g.e[i].name;
        if (nm.size() > 5 && nm.compare(nm.size() - 5, 5, "A_hat") == 0)
            for (int j = 0; j < J; ++j) vals[i][(size_t)j * J + j] += 1.5f + (float)J;
        names.push_back(nm.c_str());
        ptrs.push_back(vals[i].data());
        numels.push_back(g.e[i].numel);
        flat.insert(flat.end(), vals[i].begin(), vals[i].end());
        printf("entry %zu %s %lld %lld\n", i, nm.c_str(), (long long)g.e[i].offset, (long long)g.e[i].numel);
    }
    printf("floats %zu\n", g.floats);
    std::vector<float> adj((size_t)J * J, 0.f);
    for (int i = 0; i < J; ++i)
        for (int j = 0; j < J; ++j) adj[(size_t)i * J + j] = (i == j || i + 1 == j || j + 1 == i) ? 1.0f / 3.0f : 0.f;
    stage_set_graph(s, adj.data());
    std::string err;
    if (!stage_load(s, names.data(), ptrs.data(), numels.data(), (int)names.size(), err)) {
        printf("load failed: %s\n", err.c_str());
        return 1;
    }
    BwdArena a;
    bwd_arena_build(s, a);
    for (const BwdBlock& b : a.blocks) printf("block %zu %d %d\n", b.w, b.K, b.N);
    printf("arena %zu %zu %zu %zu %zu %zu\n", s.floats, a.zero, a.zero_n, a.ahat, a.jj4, a.floats);
    if (!dump(out + "/stage.bin", s.h) || !dump(out + "/trans.bin", a.h) || !dump(out + "/sd.bin", flat)) return 1;
    return 0;
}
