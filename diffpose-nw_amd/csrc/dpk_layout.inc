// dpk_layout.inc — the compile-time model shape, workgroup tile, LDS carve and weight-arena layout of one
// sampler instance, and the H36M Chebyshev sparsity pattern.  Plain constexpr (no HIP): included at the top
// of dpk_sampler.inc inside each instance namespace (the including file sets DPK_P, and DPK_D / DPK_NH for
// widths other than the shipped one), and by the host packer (dpk_pack.inc), which a CPU-only build compiles
// too (tests/c/dpk_pack_check.cpp).

// ---------------------------------------------------------------------------------------
// compile-time model shape (configs/human36m_diffpose_uvxyz_cpn.yml:9-16; other widths: DPK_D, DPK_NH)
#ifndef DPK_D
#define DPK_D 96
#endif
#ifndef DPK_NH
#define DPK_NH 4
#endif
constexpr int J = 17;        // joints (n_pts)
constexpr int D = DPK_D;     // hid_dim
constexpr int D2 = 2 * D;    // GraphNet hidden (2*hid)
constexpr int D3 = 3 * D;    // QKV / Chebyshev-stacked width
constexpr int E = 4 * D;     // emd_dim = 4*hid
constexpr int NL = 5;        // num_layer (the most layers a launch runs; fewer at run time)
constexpr int NH = DPK_NH;   // n_head
constexpr int DK = D / NH;   // d_k
static_assert(D % 32 == 0 && D <= 128 && (DK == 24 || DK == 16 || DK == 32), "widths: multiples of 32 up to 128, d_k 16, 24 or 32");
constexpr int NCD = D / 16;  // 16-column tiles of a D-wide output (6 at the shipped shape)
constexpr int CIN = 5;       // coords_dim[0]
constexpr int COUT = 5;      // coords_dim[1]
constexpr int PE = J * CIN;  // floats per pose (85)

// Which gemm modes the instance has kernels and an arena for, beside fp32 (mode 0).  Mode 1 (f16x3, the
// half-width-operand GEMMs of dpk_sampler.inc) is parametrised on the width and compiled for every instance
// unless its namespace sets DPK_F16X3 0 (an instance where it measured no faster than fp32, or did not fit its
// registers); mode 2 (bf16) also changes attention, written for d_k 24: the shipped shape alone.
#ifndef DPK_F16X3
#define DPK_F16X3 1
#endif
constexpr bool MODE_F16X3 = DPK_F16X3 != 0;
constexpr bool MODE_BF16 = D == 96 && NH == 4;
constexpr int GEMM_MODES = 1 | (MODE_F16X3 ? 2 : 0) | (MODE_BF16 ? 4 : 0);   // bit m: gemm mode m

// Padded tiles: a GCNdiff skeleton of 2..16 joints rides in the 17-row pose blocks of this instance, its graph
// terms zero-embedded by pack_model and the rows past its joint count dead (dpk_sampler.inc: the PAD kernels,
// dense graph, fp32 and f16x3).  Compiled for every table entry's primary tile; the sibling tiles (8 waves, the
// 2-pose tail tile) set DPK_PADDED 0: launch_sampler runs a padded handle on plain primary tiles.
#ifndef DPK_PADDED
#define DPK_PADDED 1
#endif
constexpr bool PADDED = DPK_PADDED != 0;
constexpr int J_MIN = PADDED ? 2 : J;        // fewest joints a GCNdiff handle of this instance may have

// workgroup tile.  DPK_P (poses per workgroup) is set by the including file: 4 for the main sampler (one
// workgroup per CU), 2 for the half-size tail tiles that balance the last round of a batch (launch_sampler)
// and for the width-128 instances.  Both run one workgroup per CU, 4 waves (one per SIMD).  DPK_NW 8 (4-pose
// tiles of the shipped shape only, namespace dpk8): two waves per SIMD on the same tile; waves w and w + 4
// share a SIMD and split its GEMM column tiles, waves 2p and 2p + 1 share pose p in the per-pose phases.
constexpr int P = DPK_P;     // poses per workgroup
constexpr int R = P * J;     // 68 (34) rows
static_assert(P == 4 || P == 2, "4 or 2 poses per workgroup");
#ifdef DPK_NW
constexpr int NW = DPK_NW;   // waves per workgroup
#else
constexpr int NW = 4;
#endif
static_assert(NW == 4 || (NW == 8 && P == 4), "4 waves, or 8 on a 4-pose tile");
constexpr int NSUB = NW / 4; // waves per SIMD: the GEMM roles are those of wave & 3, sub-wave wave >> 2
constexpr int NT = 64 * NW;  // threads
// LDS row strides ≡ 40 (mod 64) dwords: conflict-free b128 A reads and epilogue writes
constexpr int stride40(int n) { return n + (104 - n % 64) % 64; }
constexpr int LDX = stride40(D);    // D-wide buffers (104 at D = 96)
constexpr int LD2 = stride40(D3);   // 3D-wide buffer (296 at D = 96)
static_assert(LDX % 64 == 40 && LD2 % 64 == 40 && LDX >= D && LD2 >= D3, "row strides");

// LDS carve (floats)
constexpr int SM_XS = 0;                    // residual stream   [R][LDX]
constexpr int SM_B1 = SM_XS + R * LDX;      // 96-wide scratch   [R][LDX]
constexpr int SM_B2 = SM_B1 + R * LDX;      // 288-wide scratch  [R][LD2]
constexpr int SM_XST = SM_B2 + R * LD2;     // pose state x_t    [R][5]
constexpr int SM_LNP = SM_XST + ((R * CIN + 3) / 4) * 4;   // LayerNorm gains/shifts of all layers [NL][4][D]
constexpr int SM_TC = SM_LNP + NL * 4 * D;                 // dense T1/T2 (dense graphs)
constexpr int SM_TS = SM_TC + 2 * J * J;                   // padded sparse T1/T2 rows (output ChebConv)
constexpr int SM_FLOATS = SM_TS + J * (5 + 9) * 2;
static_assert(SM_FLOATS * 4 <= 160 * 1024, "LDS budget");

// packed-weight blocks: one block = 16 cols x 16 k = 64 lanes x float4
constexpr int BLK = 256;
constexpr int KB_D = D / 16, KB_D2 = D2 / 16, KB_D3 = D3 / 16;   // 6, 12, 18
// per-layer offsets (floats) in the weight arena
constexpr int OFF_QKV = 0;                                  // [18 ct][6 kb]  (at D = 96)
constexpr int OFF_O = OFF_QKV + 3 * NCD * KB_D * BLK;       // [6][6]
constexpr int OFF_FC1 = OFF_O + NCD * KB_D * BLK;           // [12][6]
constexpr int OFF_FC2 = OFF_FC1 + 2 * NCD * KB_D * BLK;     // [6][12]
constexpr int OFF_C1 = OFF_FC2 + NCD * KB_D2 * BLK;         // [6][18]
constexpr int OFF_C2 = OFF_C1 + NCD * KB_D3 * BLK;          // [6][18]
constexpr int OFF_BQKV = OFF_C2 + NCD * KB_D3 * BLK;
constexpr int OFF_BO = OFF_BQKV + D3;
constexpr int OFF_BFC1 = OFF_BO + D;
constexpr int OFF_BFC2 = OFF_BFC1 + D2;
constexpr int OFF_BC1 = OFF_BFC2 + D;
constexpr int OFF_BC2 = OFF_BC1 + D;
constexpr int OFF_LN0A = OFF_BC2 + D;
constexpr int OFF_LN0B = OFF_LN0A + D;
constexpr int OFF_LN1A = OFF_LN0B + D;
constexpr int OFF_LN1B = OFF_LN1A + D;
constexpr int OFF_LG = OFF_LN1B + D;                        // 17x17
constexpr int OFF_LGF = ((OFF_LG + J * J + 63) / 64) * 64;  // graph_mma operands: [5 k][64 lanes] L^T, then row 16
constexpr int OFF_CQKV = OFF_LGF + 2 * 5 * 64;             // LN0 folded into QKV: c = b_LN0 W + b_qkv [288]
constexpr int LAYER_FLOATS = ((OFF_CQKV + D3 + 63) / 64) * 64;
constexpr int OFF_WIN = NL * LAYER_FLOATS;                  // [6 ct][1 kb]  (K=15 padded to 16)
constexpr int OFF_WOUT = OFF_WIN + NCD * 1 * BLK;           // [1 ct][18 kb] (N=5 padded to 16)
constexpr int OFF_BIN = OFF_WOUT + 1 * KB_D3 * BLK;
constexpr int OFF_BOUT = OFF_BIN + D;                       // 16 (5 used)
constexpr int OFF_CHEB = OFF_BOUT + 16;                     // dense T1 [17x17] then T2 [17x17]
constexpr int OFF_CHEBS = OFF_CHEB + 2 * J * J;             // H36M-sparse T1 (49) then T2 (87) values
// the same H36M-sparse T1 / T2 as padded rows for the output ChebConv: per joint j,
// SPT1 (value, row offset) pairs of T1 then SPT2 of T2, padding (0, j's offset); pack_model
constexpr int SPT1 = 5, SPT2 = 9;                           // max nonzeros per row of T1 / T2 (degree 4)
constexpr int OFF_CHEBT = OFF_CHEBS + 136;
constexpr int CHEBT_FLOATS = J * (SPT1 + SPT2) * 2;
constexpr int ARENA_FLOATS = ((OFF_CHEBT + CHEBT_FLOATS + 63) / 64) * 64;

// Split-fp16 GEMM arena (gemm mode 1): per layer, each GEMM's weights x W16_SCALE split into
// fp16 hi + lo parts, packed as 16x16x32 B fragments: block (16 cols x 32 k) = [hi 1 KiB | lo 1 KiB],
// lane l holding W[k = kb*32 + 8*(l>>4) + i][n = ct*16 + (l&15)] in half i = 0..7.  Byte offsets.
constexpr float W16_SCALE = 64.0f;            // keeps the lo parts of O(0.01) weights in fp16's normal range
constexpr int BLK16 = 2048;
constexpr int KB32_D = D / 32, KB32_D2 = D2 / 32, KB32_D3 = D3 / 32;   // 3, 6, 9
constexpr int O16_QKV = 0;                                             // [18 ct][3 kb]  (at D = 96)
constexpr int O16_O = O16_QKV + 3 * NCD * KB32_D * BLK16;              // [6][3]
constexpr int O16_FC1 = O16_O + NCD * KB32_D * BLK16;                  // [12][3]
constexpr int O16_FC2 = O16_FC1 + 2 * NCD * KB32_D * BLK16;            // [6][6]
constexpr int O16_C1 = O16_FC2 + NCD * KB32_D2 * BLK16;                // [6][9]
constexpr int O16_C2 = O16_C1 + NCD * KB32_D3 * BLK16;                 // [6][9]
constexpr int LAYER16_BYTES = O16_C2 + NCD * KB32_D3 * BLK16;
constexpr int ARENA16_BYTES = NL * LAYER16_BYTES;

// timestep-MLP arena (transposed nn.Linear weights: [in][out])
constexpr int TOFF_W0 = 0;                    // [96][384]
constexpr int TOFF_B0 = TOFF_W0 + D * E;
constexpr int TOFF_W1 = TOFF_B0 + E;          // [384][384]
constexpr int TOFF_B1 = TOFF_W1 + E * E;
constexpr int TOFF_WP = TOFF_B1 + E;          // [5][384][96]
constexpr int TOFF_BP = TOFF_WP + NL * E * D; // [5][96]
constexpr int TEMB_FLOATS = TOFF_BP + NL * D;

constexpr float SQRT_DK = DK == 24 ? 4.898979485566356f : DK == 32 ? 5.656854249492381f : 4.0f;   // float(math.sqrt(d_k))
constexpr float LN_EPS = 1e-6f;                         // LayerNorm eps (GraFormer.py:60)
// ---------------------------------------------------------------------------------------
// Chebyshev terms T1 = L, T2 = 2L^2 - I of the H36M skeleton (runners/diffpose_frame.py:120-124)
// are sparse (49 / 87 of 289 entries).  Their pattern is derived here at compile time from the
// edge list; pack_model() (dpk_pack.inc) checks a given adjacency against it and packs the nonzero values
// (row-major over the pattern) — any other graph runs the dense path.
constexpr int H36M_EDGES[16][2] = {{0, 1}, {1, 2}, {2, 3}, {0, 4}, {4, 5}, {5, 6}, {0, 7}, {7, 8},
                                   {8, 9}, {9, 10}, {8, 11}, {11, 12}, {12, 13}, {8, 14}, {14, 15}, {15, 16}};
struct SparsePattern {
    int n1[J], c1[J][J], o1[J];
    int n2[J], c2[J][J], o2[J];
    int nnz1, nnz2;
};
constexpr SparsePattern make_pattern() {
    SparsePattern sp{};
    bool a[J][J] = {};
    for (int i = 0; i < J; ++i) a[i][i] = true;
    for (int e = 0; e < 16; ++e) {
        a[H36M_EDGES[e][0]][H36M_EDGES[e][1]] = true;
        a[H36M_EDGES[e][1]][H36M_EDGES[e][0]] = true;
    }
    int t1 = 0, t2 = 0;
    for (int i = 0; i < J; ++i) {
        sp.n1[i] = 0;
        sp.n2[i] = 0;
        sp.o1[i] = t1;
        sp.o2[i] = t2;
        for (int j = 0; j < J; ++j) {
            bool two = false;
            for (int k = 0; k < J; ++k) two = two || (a[i][k] && a[k][j]);
            if (a[i][j]) sp.c1[i][sp.n1[i]++] = j;
            if (two) sp.c2[i][sp.n2[i]++] = j;
        }
        t1 += sp.n1[i];
        t2 += sp.n2[i];
    }
    sp.nnz1 = t1;
    sp.nnz2 = t2;
    return sp;
}
constexpr SparsePattern SPAT = make_pattern();
static_assert(SPAT.nnz1 == 49 && SPAT.nnz2 == 87, "H36M Chebyshev sparsity");
