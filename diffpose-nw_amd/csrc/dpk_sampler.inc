// dpk_sampler.inc — the sampler kernel and its device phases for one tile size and model width.
// Included by dpk_kernels.hip seven times, each inside a namespace of its own: dpk with DPK_P 4 (68-row tiles,
// the main grid), dpk8 (the same tile on 8 waves, DPK_NW 8) and dpk2 with DPK_P 2 (34-row tiles for the last,
// partial round of a large batch) at the shipped shape (hid 96 / 4 heads); dpkw / dpkw4 (DPK_D 128, DPK_NH
// 8 / 4, DPK_P 2) and dpkn / dpkn4 (DPK_D 64, DPK_NH 2 / 4, DPK_P 4), the samplers of the other widths; the host
// reaches every one through the instance table (dpk_kernels.hip: INSTANCES).  The shape,
// tile, LDS-carve and arena-layout constants are dpk_layout.inc's (shared with the host packer,
// dpk_pack.inc); everything here depends on P only through P, R and the LDS carve, and on the width through
// D, NH and those constants.

#include "dpk_layout.inc"

// a phase's mid-point hook (DPK_PRE_MID): issues the next GEMM's B prefetch behind the phase's MFMAs
struct NoHook {
    __device__ __forceinline__ void operator()() const {}
};
#ifndef DPK_PRE_MID
#define DPK_PRE_MID 14   // fp32 GEMM B prefetch issued right behind the preceding phase's MFMAs: 2 O (attention's
                         // score MFMAs), 4 fc1 (graph1's), 8 C1 (graph2's)
#endif
// 8 waves, per GEMM mode (_W8 fp32, _W8F f16x3, _W8B bf16; DPK_MID / DPK_LATE are used in sample_kernel only,
// where G16 is the GEMM mode).  fp32 keeps the 4-wave placement (paired A/B: +1.2 % over 4 waves, +0.5 % with
// the placement below).  The half-width modes keep only fc1's there: O's and C1's, held across attention and
// graph2 + cheb_prep, pushed the f16x3 kernel past its 256 registers, and bf16 measured faster without them
// (+1.5 % against +1.2 %: the SIMD's other wave covers their latency); profiles/w8_ab_placement.txt
#ifndef DPK_PRE_MID_W8
#define DPK_PRE_MID_W8 DPK_PRE_MID
#endif
#ifndef DPK_PRE_MID_W8F
#define DPK_PRE_MID_W8F 4
#endif
#ifndef DPK_PRE_MID_W8B
#define DPK_PRE_MID_W8B 4
#endif
#define DPK_W8SEL(a, f, b) (G16 == 0 ? (a) : G16 == 1 ? (f) : (b))
#define DPK_MID(bit) \
    (((NSUB == 2 ? DPK_W8SEL(DPK_PRE_MID_W8, DPK_PRE_MID_W8F, DPK_PRE_MID_W8B) : DPK_PRE_MID) & (bit)) != 0)

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// packed fp32 fma (v_pk_fma_f32: two lanes of work per instruction)
__device__ __forceinline__ f32x2 pfma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f32x2 splat2(float x) { return f32x2{x, x}; }
// x in both halves of a VGPR pair, so packed ops take it as an operand (a splatted scalar is
// otherwise often split back into two v_sub_f32 / v_mul_f32 per pair)
__device__ __forceinline__ f32x2 vpair(float x) {
    f32x2 p = {x, x};
    asm volatile("" : "+v"(p));
    return p;
}
// packed x + ns (ns = -s: LLVM selects v_pk_add_f32 for a packed add, but splits a packed
// subtract into two v_sub_f32) and x * r on 4 values, with pair operands
__device__ __forceinline__ f32x4 padd4(f32x4 x, f32x2 ns) {
    const f32x2 lo = f32x2{x[0], x[1]} + ns, hi = f32x2{x[2], x[3]} + ns;
    return f32x4{lo[0], lo[1], hi[0], hi[1]};
}
__device__ __forceinline__ f32x4 pmul4(f32x4 x, f32x2 r) {
    const f32x2 lo = f32x2{x[0], x[1]} * r, hi = f32x2{x[2], x[3]} * r;
    return f32x4{lo[0], lo[1], hi[0], hi[1]};
}

// half-width operand vectors (gemm modes 1, 2: gemmh_pass)
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

// Kernel modes: the K-step sampler (GCNdiff + DDIM), one GCNdiff eps evaluation, or one
// GCNpose forward (models/gcnpose.py:101-113: the same backbone without the timestep
// embedding, coords 2 -> 3), which also builds the sampler's uvxyz input
// (runners/diffpose_frame.py:337-342).
enum { M_SAMPLE = 0, M_EPS = 1, M_POSE = 2 };
constexpr int CIN_POSE = 2, COUT_POSE = 3;

using SampleArgs = ::dpk_shared::SampleArgs;
constexpr int TRACE_SLOTS = 256;

// ---------------------------------------------------------------------------------------
// counter-based normal noise for eta > 0 (Philox4x32-10 + Box-Muller)
__device__ __forceinline__ void philox(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[1] = (uint32_t)p1;
        c[3] = (uint32_t)p0;
        c[0] = n0;
        c[2] = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

__device__ __forceinline__ float normal_noise(unsigned long long seed, int step, long long idx) {
    uint32_t c[4] = {(uint32_t)idx, (uint32_t)((unsigned long long)idx >> 32), (uint32_t)step, 0x5EEDu};
    philox(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float u1 = ((float)(c[0] >> 8) + 1.0f) * (1.0f / 16777216.0f);   // (0, 1]
    const float u2 = (float)(c[1] >> 8) * (1.0f / 16777216.0f);            // [0, 1)
    return sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
}

// DDIM update for one element (common/utils_diff.py:59-65), fp32, no contraction:
// x0 = (xt - et*sqrt(1-at)) / sqrt(at);  x' = sqrt(an)*x0 + c1*z + c2*et
__device__ __forceinline__ void ddim_elem(const float* cf, float xt, float et, float z, float& x0, float& xn) {
    x0 = (xt - et * cf[0]) / cf[1];
    xn = (cf[2] * x0 + cf[3] * z) + cf[4] * et;
}

// Hypothesis start for one element (runners/diffpose_frame.py:359-363): x_T = x*sqrt(a) + (e*noise_scale)*sqrt(1-a)
// with a = alpha_bar[t_start + 1], fp32 in the reference's order, no contraction: four roundings.
__device__ __forceinline__ float qsample_elem(float x, float e, float scale, float sa, float sb) {
    return (x * sa) + ((e * scale) * sb);
}
// ... for element r of pose `pose` (pe floats per pose): e from the caller's [N][pe] draws or counter-based at
// step -1 (eta's per-step draws use steps 0..K-1), keyed by the global element index alone; scale row
// pose % rows (the reference's hypothesis-major repeat), null = ones (e * 1 is e)
__device__ __forceinline__ float qsample_at(float x, int pose, int r, int pe, float sa, float sb,
                                            const float* __restrict__ scale, int rows,
                                            const float* __restrict__ noise, unsigned long long seed) {
    const long long g = (long long)pose * pe + r;
    const float e = noise ? noise[g] : normal_noise(seed, -1, g);
    const float sc = scale ? scale[(size_t)(pose % rows) * pe + r] : 1.0f;
    return qsample_elem(x, e, sc, sa, sb);
}

// DPP row (16-lane) rotations and all-reduces
template <int J>
__device__ __forceinline__ float row_ror(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, x), __builtin_bit_cast(int, x),
                                                                 0x120 + J, 0xf, 0xf, false));
}

// Sum over the 4 lane rows (l, l^16, l^32, l^48), result in every lane, on the VALU: a
// v_permlane32_swap / v_permlane16_swap of two copies of v leaves (v, partner) split across
// the two registers, so their sum is v + partner in every lane (tools/permlane_probe.hip; the
// clang builtins return a mis-assigned pair on this toolchain, hence the inline asm).  Replaces
// two LDS-crossbar shuffles.
__device__ __forceinline__ float sum4rows(float v) {
    float a = v, b = v;
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    const float s1 = a + b;
    float c = s1, d = s1;
    asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(c), "+v"(d));
    return c + d;
}

// sum4rows of two values at once, 3 permlane swaps instead of 4 (and no copies for the first):
// rows 0,1 / 2,3 hold x / y half-sums after the first swap, totals after the second, and a
// last permlane32 swap broadcasts each to all four rows.  Same association as sum4rows.
__device__ __forceinline__ void sum4rows2(float& x, float& y) {
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(x), "+v"(y));
    float c = x + y, d = c;
    asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(c), "+v"(d));
    x = c + d;
    y = x;
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(x), "+v"(y));
}
__device__ __forceinline__ void max4rows2(float& x, float& y) {
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(x), "+v"(y));
    float c = fmaxf(x, y), d = c;
    asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(c), "+v"(d));
    x = fmaxf(c, d);
    y = x;
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(x), "+v"(y));
}

// Reduce-scatter of 4 registers over the 4 lane rows: lane l returns the sum over rows of
// register (l>>4) at row position l&15, summed ((row0 + row2) + (row1 + row3)) like sum4rows.
// 3 permlane swaps for 4 values instead of sum4rows' 8 (tools/rs4_probe.hip checks the map).
__device__ __forceinline__ float rs4rows(float v0, float v1, float v2, float v3) {
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(v0), "+v"(v2));
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(v1), "+v"(v3));
    float a = v0 + v2, b = v1 + v3;
    asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    return a + b;
}

// MFMA result -> inline-asm reader.  hipcc pads the wait states between an MFMA and a compiler-visible
// reader of its D registers, but not for a reader inside inline asm (MI355X guide §5.7 item 2): the
// permlane swaps above carry only the VALU-write -> permlane pad (s_nop 1).  Where they take MFMA
// accumulators directly (the fp32 GEMM tail rows' rs4rows, attention's denominator swap), mfma_pad runs first: an
// s_nop tied to the accumulators by "+v" operands, so in any schedule the MFMAs that wrote them issue before
// it and the swaps after it (tools/asm_hazard_check.py checks the built schedule).  Counts (tools/mfma_hazard_probe.hip, hipcc's own pads for a VALU reader on
// gfx950: s_nop 3 after v_mfma_f32_4x4x1_16b_f32, 4 after the 4x4x4_16b f16/bf16 forms, 7 after the
// 16x16x16 / 16x16x32 bf16 / f16 forms, 9 after v_mfma_f32_16x16x4_f32), raised to the guide's XDL table
// where that is larger (2 passes: 6 states, 8 passes: 12).  Round 5 relied on schedule distance instead
// (the woven epilogue's LAG of two tiles), which a one-tile lag or a woven tail epilogue broke; with the
// pads both give bitwise the shipped results (profiles/r06_hazard_ab.txt).
constexpr int PAD_MFMA4 = 5;     // s_nop count after a 4x4 MFMA (6 wait states)
constexpr int PAD_MFMA16 = 11;   // after a 16x16 MFMA (12 wait states)
template <int N, int K>
__device__ __forceinline__ void mfma_pad(f32x4 (&v)[K]) {
    static_assert(K >= 1 && K <= 8, "mfma_pad: 1..8 accumulators");
    if constexpr (K == 1) asm volatile("s_nop %1" : "+v"(v[0]) : "i"(N));
    else if constexpr (K == 2) asm volatile("s_nop %2" : "+v"(v[0]), "+v"(v[1]) : "i"(N));
    else if constexpr (K == 3) asm volatile("s_nop %3" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]) : "i"(N));
    else if constexpr (K == 4) asm volatile("s_nop %4" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]) : "i"(N));
    else if constexpr (K == 5)
        asm volatile("s_nop %5" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]) : "i"(N));
    else if constexpr (K == 6)
        asm volatile("s_nop %6" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]) : "i"(N));
    else if constexpr (K == 7)
        asm volatile("s_nop %7"
                     : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6])
                     : "i"(N));
    else
        asm volatile("s_nop %8"
                     : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7])
                     : "i"(N));
}

// Launder a value through an empty asm so LLVM cannot hoist per-thread address math out
// of the K-step / layer loops of the persistent kernel (hoisted, it stays live across
// every phase and spills).
__device__ __forceinline__ int opaque(int x) {
    asm volatile("" : "+v"(x));
    return x;
}
// The same for a wave-uniform value (SGPR): per-pose row offsets derived from the wave index are
// recomputed per call instead of being hoisted out of the step loop as one SGPR per row, which
// spilled to VGPR lanes (a v_readlane and two address adds per row store in cheb_prep).
__device__ __forceinline__ int opaque_s(int x) {
    asm volatile("" : "+s"(x));
    return x;
}

// ---------------------------------------------------------------------------------------
// GEMM over the workgroup's 68 rows.  Rows 0..63 are 4 MFMA row tiles (v_mfma_f32_16x16x4_f32);
// the 4 leftover rows 64..67 ("tail") run on v_mfma_f32_4x4x1_16b_f32 inside the same k-loop,
// fed by the B fragments already in registers (TM_MFMA4 below; in a QKV-shaped k-block the 20
// tail MFMAs cost 8.8 cycles each beside the 72 16x16x4 ones, tools/mfma_mix_probe.hip; VALU
// FMAs for these rows (v4) cost ~10 cycles each, a padded 16-row tile 25 % of the GEMM).
//
// MFMA operand maps: lane l holds A[row rt*16+(l&15)][k = kb*16 + 4*(l>>4) + j] for sub-step j,
// and the packed B block holds W[k = same][n = ct*16 + (l&15)] (a consistent permutation of k).
// Tail: the 4x4x1 accumulators hold partial sums per k-slice (lane group), reduce-scattered by
// permlane swaps in the epilogue (rs4rows).
//
// B blocks are fetched with buffer loads: one VGPR offset (lane*16) shared by every load and the
// block offset in SGPR soffset, so the k-loop does no VALU address arithmetic.  A comes from one
// LDS buffer per GEMM (the Chebyshev GEMMs read [T1X | T2X | X] from B2, see cheb_prep), which
// keeps the loop body a single basic block: loads are unconditional (last pair peeled) and the
// compiler emits exact vmcnt/lgkmcnt waits instead of draining at a join.
struct BSrc {
    __amdgpu_buffer_rsrc_t rsrc;
    int voff;      // lane * 16
    int sbase;     // byte offset of this wave's first column tile (wave-uniform)
    __device__ __forceinline__ f32x4 load(int blk) const {
        return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, sbase + blk * 1024, 0));
    }
};

// Tile offsets of the B blocks (tile_offsets below): a per-tile VGPR offset (lane*16 + the tile's
// byte offset) with the k-block in soffset / the immediate field, so the tile offsets stay in VGPRs
// across the persistent loop instead of SGPRs, which the kernel's SGPR budget spilled to VGPR lanes
// (a v_readlane + 5 wait states before every B load, round 2).
__device__ __forceinline__ f32x4 bload(const BSrc& s, int toff, int kb) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(s.rsrc, toff, kb * 1024, 0));
}

// Packed B-fragment blocks of a GEMM with NC column tiles and KB k-blocks: [NC][KB][64 lanes][4].
template <int NC, int KB>
__device__ __forceinline__ BSrc bsrc(const float* Bp, int ct0, int lane) {
    BSrc s;
    // range: the rest of the weight arena, so the layer's bias vectors (stored after its weight
    // blocks) load through the same descriptor (gemm_wave)
    s.rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)Bp, (short)0, 0x7fffffff, 0x00020000);
    s.voff = lane * 16;
    s.sbase = ct0 * KB * 1024;
    return s;
}

// Tail modes: TM_VALU — TR tail rows per wave on the VALU (scalar fma per MFMA);
// TM_MFMA4 — all 4 tail rows on v_mfma_f32_4x4x1_16b_f32 for NQ = ceil(NCW/2) of the wave's
// column tiles.  The 4x4x1 form reads the SAME B fragment as the 16x16x4 MFMAs (block b = l>>2
// holds W[k = kb*16 + 4*(l>>4) + j][col 4*(b&3) + (l&3)]), and its A operand is one float per
// lane: tail row l&3 at the lane group's k.  D reg r of lane l = partial sum (tail row r,
// column l&15, k-slice l>>4).  The two waves of a column half split the tail column tiles: the
// second wave processes its tiles rotated by NQ (rotation lives in SGPR load offsets and store
// addresses only), so the tail tiles are local indices 0..NQ-1 for both.
enum { TM_NONE = 0, TM_VALU = 1, TM_MFMA4 = 2 };

// TRANS: the MFMA computes the transposed tile (operands swapped: the packed weight fragment
// is the A operand, the activation fragment the B operand; both registers are unchanged), so
// lane l ends up with 4 consecutive COLUMNS 4*(l>>4)..+3 of row l&15 and the epilogue moves
// one 16-byte vector per tile (ds_write_b128 / ds_read_b128) instead of four 4-byte ones.
// NQO: the tail tiles among the NCW (default: the first half, rounded up).
template <int NR, int NCW, int TM, int TR, int KB, bool TRANS = true, int NQO = (NCW + 1) / 2>
struct GemmTile {
    static constexpr int TA = TM == TM_VALU ? TR : 1;    // tail A fragments per ring slot
    static constexpr int NQ = TM == TM_MFMA4 ? NQO : 1;
    f32x4 acc[NR][NCW];
    float tl[NCW][TA];      // TM_VALU: tail partial sums over this lane's k's
    f32x4 tacc[NQ];         // TM_MFMA4: 4x4x1 accumulators
    int aoff[NR], toff[TA];

    __device__ __forceinline__ void loadA(f32x4 (&a)[NR], f32x4 (&t)[TA], const float* A, int kb) const {
#pragma unroll
        for (int i = 0; i < NR; ++i) a[i] = *reinterpret_cast<const f32x4*>(A + aoff[i] + kb * 16);
        if constexpr (TM != TM_NONE) {
#pragma unroll
            for (int i = 0; i < TA; ++i) t[i] = *reinterpret_cast<const f32x4*>(A + toff[i] + kb * 16);
        }
    }
    __device__ __forceinline__ static void loadB(f32x4 (&b)[NCW], const BSrc& s, const int (&soff)[NCW], int kb) {
#pragma unroll
        for (int c = 0; c < NCW; ++c) b[c] = bload(s, soff[c], kb);
    }
    // FIRST: the GEMM's first k-step takes C = 0 as an inline constant (no accumulator zeroing:
    // ~100 v_accvgpr_write per wave and GEMM otherwise)
    template <bool FIRST = false>
    __device__ __forceinline__ void mma(const f32x4 (&a)[NR], const f32x4 (&t)[TA], const f32x4 (&b)[NCW]) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int i = 0; i < NR; ++i)
#pragma unroll
                for (int c = 0; c < NCW; ++c) {
                    const f32x4 cin = (FIRST && j == 0) ? z : acc[i][c];
                    acc[i][c] = TRANS ? __builtin_amdgcn_mfma_f32_16x16x4f32(b[c][j], a[i][j], cin, 0, 0, 0)
                                      : __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][j], b[c][j], cin, 0, 0, 0);
                }
            if constexpr (TM == TM_VALU) {
#pragma unroll
                for (int c = 0; c < NCW; ++c)
#pragma unroll
                    for (int r = 0; r < TR; ++r) tl[c][r] = fmaf(t[r][j], b[c][j], tl[c][r]);
            } else if constexpr (TM == TM_MFMA4) {
#pragma unroll
                for (int q = 0; q < NQ; ++q)
                    tacc[q] = __builtin_amdgcn_mfma_f32_4x4x1f32(b[q][j], t[0][j], (FIRST && j == 0) ? z : tacc[q], 0, 0, 0);
            }
        }
    }
    // keep the ring's program order: this half's MFMAs, then its slot's loads; nothing crosses
    // (otherwise the scheduler sinks the loads next to their consumers)
    __device__ __forceinline__ static void schedule_half() { __builtin_amdgcn_sched_barrier(0); }
};

// B fragments of a GEMM's first two k-blocks, loaded before the phase that precedes the GEMM
// (weights do not depend on activations) so the L2 latency hides under that phase.
template <int NCW>
struct BPre {
    f32x4 b0[NCW], b1[NCW];
};

// Wave roles in the workgroup GEMM: column half ch(w) and index within the pair of waves that
// share it, pr(w).  68 rows: wave w = row tiles 2*(w>>1)+{0,1} of column half w&1; 34 rows:
// row tile w&1 of column half w>>1.
// 8 waves (NSUB = 2): waves w and w + 4 run on one SIMD and share the role of wave w & 3; they split its
// column tiles (in the rotated local order) into [0, NCW/2) for sub-wave 0 and [NCW/2, NCW) for sub-wave 1,
// each with the tail rows of those of its tiles that are tail tiles (local index < ceil(NCW/2)).  Every
// output element is still one k-ordered MFMA chain: the GEMM outputs are bitwise those of 4 waves.
__device__ __forceinline__ int gemm_ch(int wave) { return R == 68 ? (wave & 1) : (wave >> 1); }
__device__ __forceinline__ int gemm_pr(int wave) { return R == 68 ? (NSUB == 1 ? wave >> 1 : (wave & 3) >> 1) : (wave & 1); }
// column tiles of the sub-wave holding the most, of a role's N: what a prefetch struct is sized for
constexpr int sub_max(int n) { return NSUB == 1 ? n : n - n / 2; }

// Column rotation of wave `wave` within its column half (TM_MFMA4 tail split, see GemmTile).
template <int NCW>
__device__ __forceinline__ int col_rot(int wave) { return gemm_pr(wave) ? (NCW + 1) / 2 : 0; }

// SGPR byte offsets of the wave's NCW column tiles' first k-block, rotation applied.
template <int NCW, int KB>
__device__ __forceinline__ void tile_offsets(int (&soff)[NCW], const BSrc& s, int rot) {
#pragma unroll
    for (int c = 0; c < NCW; ++c) {
        const int cc = c + rot;
        soff[c] = s.voff + s.sbase + (cc >= NCW ? cc - NCW : cc) * KB * 1024;
    }
}

template <int NC, int KB, int NPRE = 2>
__device__ __forceinline__ BPre<sub_max(NC / 2)> gemm_prefetch(const float* Bp, int wave, int lane) {
    constexpr int NCW = NC / 2, NP = sub_max(NCW);
    const BSrc s = bsrc<NC, KB>(Bp, gemm_ch(wave) * NCW, lane);
    if constexpr (NSUB == 1) {
        int soff[NCW];
        tile_offsets<NCW, KB>(soff, s, col_rot<NCW>(wave));
        BPre<NCW> pre;
#pragma unroll
        for (int c = 0; c < NCW; ++c) {
            pre.b0[c] = bload(s, soff[c], 0);
            pre.b1[c] = (KB > 1 && NPRE > 1) ? bload(s, soff[c], 1) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        return pre;
    }
    // the sub-wave's first local tile and tile count (wave-uniform)
    const int c0 = NSUB == 1 ? 0 : (wave >> 2) * (NCW / 2), nown = NSUB == 1 ? NCW : (wave >> 2 ? NCW - NCW / 2 : NCW / 2);
    const int rot = col_rot<NCW>(wave);
    BPre<NP> pre;
#pragma unroll
    for (int c = 0; c < NP; ++c) {
        const int cc = c0 + c + rot;
        const int toff = s.voff + s.sbase + (cc >= NCW ? cc - NCW : cc) * KB * 1024;
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        pre.b0[c] = z;
        pre.b1[c] = z;
        if (NSUB == 1 || c < nown) {
            pre.b0[c] = bload(s, toff, 0);
            if constexpr (KB > 1 && NPRE > 1) pre.b1[c] = bload(s, toff, 1);
        }
    }
    return pre;
}

#ifndef DPK_PRE_LATE
#define DPK_PRE_LATE 5   // fp32 GEMM B prefetch issued after the preceding VALU phase (before its barrier), per GEMM:
                         // 1 QKV (after LN0), 2 O (after attention), 4 fc1 (after LN1+graph1), 8 C1 (after
                         // graph2+cheb_prep), 16 C2 (after cheb_prep2)
#endif
#ifndef DPK_PRE_LATE_W8
#define DPK_PRE_LATE_W8 DPK_PRE_LATE
#endif
#ifndef DPK_PRE_LATE_W8F
#define DPK_PRE_LATE_W8F 15
#endif
#ifndef DPK_PRE_LATE_W8B
#define DPK_PRE_LATE_W8B 15
#endif
#define DPK_LATE(bit) \
    (((NSUB == 2 ? DPK_W8SEL(DPK_PRE_LATE_W8, DPK_PRE_LATE_W8F, DPK_PRE_LATE_W8B) : DPK_PRE_LATE) & (bit)) != 0)
#ifndef DPK_FC1_NPRE
#define DPK_FC1_NPRE 2   // fp32 fc1: k-blocks of B prefetched ahead of the GEMM
#endif
#ifndef DPK_QKV_NPRE
#define DPK_QKV_NPRE 1   // fp32 QKV: k-blocks of B prefetched ahead of the GEMM (1: the second loads in its prologue)
#endif
// Epilogue modes (out = acc + bias[col]):
//   E_STORE       dst = out                       (QKV, gconv_input)
//   E_STORE_RELU  dst = relu(out)                 (GraphNet fc1)
//   E_RESID       dst = dst + out                 (attention O-proj)
//   E_RESID_RELU  dst = dst + relu(out)           (Cheb2 of _ResChebGC_diff)
//   E_CHEB1       dst = relu(out) + tproj[col]    (Cheb1 + temb_proj injection)
//   E_STORE_NB    dst = acc (no bias)             (GraphNet fc2 before its graph product)
// Bias / temb columns are loaded into registers before the k-loop and residual values are
// read in one batch, so the epilogue is LDS + VALU only (no per-element global round trip).
enum { E_STORE = 0, E_STORE_RELU, E_RESID, E_RESID_RELU, E_CHEB1, E_STORE_NB };

struct EpiArgs {
    float* dst;
    int ldd;
    const float* bias;
    const float* tproj;     // E_CHEB1: temb_proj row (sample mode) or per-pose base (eps mode)
    int tproj_pose_stride;  // 0: one row for all poses; else floats between consecutive poses
    int pose0;              // global index of the workgroup's first pose (eps mode clamp)
    int pose_max;           // N-1
};

// 1/d to ~0.5 ulp: v_rcp_f32 plus one Newton step
__device__ __forceinline__ float rcp_nr(float d) {
    const float r = __builtin_amdgcn_rcpf(d);
    return fmaf(r, fmaf(-d, r, 1.0f), r);
}

template <int MODE>
__device__ __forceinline__ float epi_value(float acc, float bias, float tp, float old) {
    const float v = acc + bias;
    if constexpr (MODE == E_STORE_NB) return acc;
    else if constexpr (MODE == E_STORE) return v;
    else if constexpr (MODE == E_STORE_RELU) return fmaxf(v, 0.f);
    else if constexpr (MODE == E_RESID) return old + v;
    else if constexpr (MODE == E_RESID_RELU) return old + fmaxf(v, 0.f);
    else return fmaxf(v, 0.f) + tp;
}

// the same on 4 columns as packed-f32 vector ops (v_pk_add_f32); identical roundings
// (NB: the bias is already in v, as the half-width GEMMs' epilogue folds it into the rescale)
template <int MODE, bool NB = false>
__device__ __forceinline__ f32x4 epi_value4(f32x4 acc, f32x4 bias, f32x4 tp, f32x4 old) {
    if constexpr (MODE == E_STORE_NB) return acc;
    f32x4 v = acc;
    if constexpr (!NB) v = acc + bias;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    if constexpr (MODE == E_STORE) return v;
    else if constexpr (MODE == E_STORE_RELU) return __builtin_elementwise_max(v, z);
    else if constexpr (MODE == E_RESID) return old + v;
    else if constexpr (MODE == E_RESID_RELU) return old + __builtin_elementwise_max(v, z);
    else return __builtin_elementwise_max(v, z) + tp;
}

__device__ __forceinline__ float tproj_at(const EpiArgs& e, int row, int col, float tcol) {
    if (e.tproj_pose_stride == 0) return tcol;
    const int pose = min(e.pose0 + row / J, e.pose_max);
    return e.tproj[(size_t)pose * e.tproj_pose_stride + col];
}


// One wave: row tiles [rt0, rt0+NR) on MFMA plus the tail (TM) over NCW column tiles from ct0,
// visited in rotated order (local tile c = global ct0 + (c + rot) mod NCW); S-slot register ring
// (first ring pass peeled, last pass with the epilogue constants).
// XS2: k-blocks 0 .. 2S-1 of A come from AX (row stride ldx) instead of A: the Chebyshev GEMMs'
// T0 = x block is read where x lives (cheb_prep XSKIP).  Those k-blocks are loaded only by the
// prologue and the peeled first ring pass, so the choice is compile-time.
// C0, NCS (8 waves): the wave computes the local tiles [C0, C0 + NCS) of the role's NCW0 (in the rotated
// order), and the tail rows of those of them that are tail tiles (local index < ceil(NCW0/2)).
template <int NR, int NCW0, int TM0, int TR, int NC, int KB, int MODE, bool XS2 = false, int NPRE = 2, int C0 = 0,
          int NCS = NCW0, int NPW = NCW0>
__device__ __forceinline__ void gemm_wave(const float* A, int lda, const float* Bp, int rt0, int ct0, int rot,
                                          int trow0, bool tail_dup, int lane, const EpiArgs& e,
                                          const BPre<NPW>& pre, const float* AX = nullptr, int ldx = 0) {
    constexpr int NCW = NCS;                       // the wave's own tiles: local tile C0 + c
    constexpr int NQF = (NCW0 + 1) / 2;            // tail tiles of the role
    constexpr int TQ = NQF - C0 < 0 ? 0 : (NQF - C0 > NCS ? NCS : NQF - C0);   // ... of this wave
    constexpr int TM = (TM0 == TM_MFMA4 && TQ == 0) ? TM_NONE : TM0;
    static_assert(C0 >= 0 && NCS >= 1 && C0 + NCS <= NCW0 && NPW >= NCS, "sub-wave tile range");
    using T = GemmTile<NR, NCW, TM, TR, KB, true, TQ>;
    constexpr int TA = T::TA, NQ = T::NQ;
    static_assert(KB == 1 || KB % 2 == 0, "k-blocks in pairs");
    lane = opaque(lane);
    T g;   // accumulators: set by the first k-step (mma<true>)
#pragma unroll
    for (int c = 0; c < NCW; ++c)
#pragma unroll
        for (int r = 0; r < TA; ++r) g.tl[c][r] = 0.f;
    const int rl = lane & 15, kq = (lane >> 4) * 4;
#pragma unroll
    for (int i = 0; i < NR; ++i) g.aoff[i] = ((rt0 + i) * 16 + rl) * lda + kq;
    if constexpr (TM == TM_MFMA4) {
        g.toff[0] = (trow0 + (lane & 3)) * lda + kq;
    } else {
#pragma unroll
        for (int i = 0; i < TA; ++i) g.toff[i] = (trow0 + i) * lda + kq;
    }
    int xoff[NR], xtoff = 0;
    if constexpr (XS2) {
        static_assert(TM0 == TM_MFMA4, "XS2: 4x4x1 tail rows");
#pragma unroll
        for (int i = 0; i < NR; ++i) xoff[i] = ((rt0 + i) * 16 + rl) * ldx + kq;
        xtoff = (trow0 + (lane & 3)) * ldx + kq;
    }
    int gcol[NCW];                                  // global column tile of local tile c (uniform)
#pragma unroll
    for (int c = 0; c < NCW; ++c) {
        const int cc = C0 + c + rot;
        gcol[c] = ct0 + (cc >= NCW0 ? cc - NCW0 : cc);
    }
    // bias (and sample-mode temb projection) of this lane's 4 output columns per tile, and of the
    // tail tiles (TM_MFMA4: after the k-slice reduce-scatter lane l holds tail row l&3, column tcol
    // of the tile).  The bias vectors sit after the weight blocks in the layer's arena, so they load
    // through the GEMM's own buffer descriptor (a uniform byte offset, no 64-bit VALU address math);
    // issued with the last ring pass (or after the prologue's A reads for one-pass GEMMs), whose MFMAs
    // cover their L2 latency.
    const BSrc src = bsrc<NC, KB>(Bp, ct0, lane);
    int soff[NCW];
    if constexpr (NCS == NCW0) {
        tile_offsets<NCW, KB>(soff, src, rot);
    } else {
#pragma unroll
        for (int c = 0; c < NCW; ++c) soff[c] = src.voff + src.sbase + (gcol[c] - ct0) * KB * 1024;
    }
    const int tcol = 4 * ((lane >> 2) & 3) + (lane >> 4);
    f32x4 bias4[NCW], tp4[NCW];
    float tbias[NQ], ttp[NQ];
    auto load_epi_consts = [&]() {
        const unsigned kqu = (unsigned)kq, tcu = (unsigned)tcol;
        const int boff = (int)(e.bias - Bp) * 4;    // byte offset of the bias vector from the weight blocks
#pragma unroll
        for (int c = 0; c < NCW; ++c) {
            const float* pt = e.tproj + gcol[c] * 16;
            if constexpr (MODE == E_STORE_NB) bias4[c] = f32x4{0.f, 0.f, 0.f, 0.f};
            else bias4[c] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(src.rsrc, kq * 4, boff + gcol[c] * 64, 0));
            tp4[c] = (MODE == E_CHEB1 && e.tproj_pose_stride == 0) ? *reinterpret_cast<const f32x4*>(pt + kqu)
                                                                   : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            tbias[q] = 0.f;
            ttp[q] = 0.f;
            if constexpr (TM == TM_MFMA4) {
                if constexpr (MODE != E_STORE_NB)
                    tbias[q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(src.rsrc, tcol * 4, boff + gcol[q] * 64, 0));
                if (MODE == E_CHEB1 && e.tproj_pose_stride == 0) ttp[q] = (e.tproj + gcol[q] * 16)[tcu];
            }
        }
    };
    // S-stage register ring: slot st holds k-block kb+st; its refill (k-block kb+st+S) is issued
    // right after its MFMAs, so loads run S-1 slots ahead of use.  3 slots where a slot is
    // short (NCW <= 6: 24-48 MFMAs, below the loaded L2 latency), 2 for the 9-tile QKV halves.
    // XS2: the x block (k-blocks 0 .. D/16-1) is loaded by the prologue and the peeled first pass only,
    // so it must be one or two ring passes: 4 slots at D = 128 (x = k-blocks 0..7) and at D = 64 (0..3)
    constexpr int KBX = D / 16;
    constexpr int S = (KB == 1) ? 1
                      : (XS2 && (KBX == 8 || KBX == 4)) ? 4
                      : (NCW <= 6 && KB % 3 == 0) ? 3 : 2;
    static_assert(KB == 1 || KB % S == 0, "ring slots divide the k-blocks");
    static_assert(!XS2 || (KB > 2 * S && (KBX == S || KBX == 2 * S)), "XS2: the x block is one or two ring passes");
    f32x4 as[S][NR], ts[S][TA], bs[S][NCW];
    // A k-block kb of slot st: from AX for kb < 2S (XS2), else from A
    auto loadA = [&](int st, int kb) {
        if (XS2 && kb < KBX) {
#pragma unroll
            for (int i = 0; i < NR; ++i) as[st][i] = *reinterpret_cast<const f32x4*>(AX + xoff[i] + kb * 16);
            if constexpr (TM != TM_NONE) ts[st][0] = *reinterpret_cast<const f32x4*>(AX + xtoff + kb * 16);
        } else {
            g.loadA(as[st], ts[st], A, kb);
        }
    };
    // residual epilogues: the wave's own output tiles of dst (its rows 64..67 columns too), read
    // before the last ring pass so the epilogue waits on no LDS round trip (the GEMM's A operand
    // is never dst, and no other wave writes these tiles before this wave's epilogue)
    constexpr bool RES = MODE == E_RESID || MODE == E_RESID_RELU;
    const int trow = trow0 + (lane & 3);
    // address of the lane's 4 columns of output tile (row tile i, local column tile c) in dst.
    // rot is 0 or R0 = ceil(NCW/2), so tiles c < NCW - R0 sit at (ct0 + rot + c) and the others at
    // (ct0 + c - (rot ? NCW - R0 : 0)): two per-row VGPR bases, and every tile's offset from its base
    // is the compile-time c * 16 floats (the store's immediate field) instead of a spilled SGPR tile
    // offset read back and added per store
    constexpr int R0 = (NCW0 + 1) / 2;
    auto tile_ptr = [&](int i, int c) -> float* {
        const int row = (rt0 + i) * 16 + rl;
        float* rb = e.dst + row * e.ldd + kq + ct0 * 16;
        return (C0 + c < NCW0 - R0 ? rb + rot * 16 : rb - (rot ? (NCW0 - R0) * 16 : 0)) + (C0 + c) * 16;
    };
    f32x4 old[NR][NCW];
    float oldt[NQ];
    auto load_old = [&]() {
        if constexpr (RES) {
#pragma unroll
            for (int i = 0; i < NR; ++i)
#pragma unroll
                for (int c = 0; c < NCW; ++c)
                    old[i][c] = *reinterpret_cast<const f32x4*>(tile_ptr(i, c));
            if constexpr (TM == TM_MFMA4) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) oldt[q] = e.dst[min(trow, R - 1) * e.ldd + gcol[q] * 16 + tcol];
            }
        }
    };
    // NPRE: k-blocks the caller prefetched (gemm_prefetch); the ring's other slots load here
    constexpr int NP = S > 1 ? NPRE : 1;
#pragma unroll
    for (int c = 0; c < NCW; ++c) {
        bs[0][c] = pre.b0[c];
        if constexpr (NP > 1) bs[1][c] = pre.b1[c];
    }
    DPK_GEMM_HOOK(0);
#pragma unroll
    for (int st = NP; st < S; ++st) T::loadB(bs[st], src, soff, st);
#pragma unroll
    for (int st = 0; st < S; ++st) loadA(st, st);
    if constexpr (KB > S) {
        // first ring pass peeled: its k-step 0 starts the accumulators from C = 0
#pragma unroll
        for (int st = 0; st < S; ++st) {
            if (st == 0) g.template mma<true>(as[0], ts[0], bs[0]);
            else g.mma(as[st], ts[st], bs[st]);
            T::loadB(bs[st], src, soff, st + S);
            loadA(st, st + S);
            T::schedule_half();
        }
#pragma unroll 1
        for (int kb = S; kb < KB - S; kb += S) {
#pragma unroll
            for (int st = 0; st < S; ++st) {
                g.mma(as[st], ts[st], bs[st]);
                T::loadB(bs[st], src, soff, kb + st + S);
                g.loadA(as[st], ts[st], A, kb + st + S);
                T::schedule_half();
            }
        }
        load_old();
        load_epi_consts();      // with the last ring pass
#pragma unroll
        for (int st = 0; st < S; ++st) g.mma(as[st], ts[st], bs[st]);
    } else {
        __builtin_amdgcn_sched_barrier(0);
        load_epi_consts();      // after the prologue's A reads, which the first MFMA waits on
        load_old();
#pragma unroll
        for (int st = 0; st < S; ++st) {
            if (st == 0) g.template mma<true>(as[st], ts[st], bs[st]);
            else g.mma(as[st], ts[st], bs[st]);
        }
    }
    DPK_GEMM_HOOK(1);
    // keep the epilogue after the last MFMAs: spread into their issue gaps, each VALU cluster costs
    // 8 cycles of switching beyond its own issue (tools/mfma_filler_probe.hip)
    __builtin_amdgcn_sched_barrier(0);
    auto tproj4 = [&](int row, int col4, const f32x4& uniform4) -> f32x4 {
        if constexpr (MODE != E_CHEB1) return f32x4{0.f, 0.f, 0.f, 0.f};
        if (e.tproj_pose_stride == 0) return uniform4;
        const int pose = min(e.pose0 + row / J, e.pose_max);
        return *reinterpret_cast<const f32x4*>(e.tproj + (size_t)pose * e.tproj_pose_stride + col4);
    };
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const int row = (rt0 + i) * 16 + rl;
#pragma unroll
        for (int c = 0; c < NCW; ++c) {
            const int col4 = gcol[c] * 16 + kq;
            const f32x4 tp = tproj4(row, col4, tp4[c]);
            *reinterpret_cast<f32x4*>(tile_ptr(i, c)) =
                epi_value4<MODE>(g.acc[i][c], bias4[c], tp, RES ? old[i][c] : f32x4{0.f, 0.f, 0.f, 0.f});
        }
    }
    if constexpr (TM == TM_VALU) {
        static_assert(TM != TM_VALU, "gemm_wave computes transposed tiles; VALU tails are gemm_out's");
    } else if constexpr (TM == TM_MFMA4) {
        // reduce-scatter the 4 k-slices: lane l then holds tail row l&3, column tcol of tile q
        const int row = trow;
        mfma_pad<PAD_MFMA4>(g.tacc);   // rs4rows reads the 4x4x1 accumulators inside asm
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const float v = rs4rows(g.tacc[q][0], g.tacc[q][1], g.tacc[q][2], g.tacc[q][3]);
            // the value is formed on every lane and only the store is skipped (dup tile / rows past
            // R): with the whole computation under the branch, LLVM sank the last tile's bias load
            // (issued before the k-loop) into it, so the waves that store waited out an L2 round trip
            // in the epilogue of QKV, O and gconv_input while their partners went on to the barrier
            const bool skip = (C0 + q == NQF - 1 && tail_dup) || row >= R;
            const int col = gcol[q] * 16 + tcol;
            const float tp = MODE == E_CHEB1 ? tproj_at(e, min(row, R - 1), col, ttp[q]) : 0.f;
            float val = epi_value<MODE>(v, tbias[q], tp, RES ? oldt[q] : 0.f);
            asm volatile("" : "+v"(val));   // formed here, on every lane: nothing sinks into the branch
            if (!skip) e.dst[row * e.ldd + col] = val;
        }
    }
    DPK_GEMM_HOOK(2);
}

// Whole-workgroup GEMM with NC output col tiles.  Wave w (of 4): row tiles 2*(w>>1) and
// 2*(w>>1)+1 and column half w&1 on the 16x16x4 MFMA; the 4 tail rows 64..67 of that column
// half on 4x4x1 MFMAs, split between the half's two waves (rotated column order for w>>1 = 1).
template <int NC, int KB, int MODE, bool XS2 = false, int NPRE = 2>
__device__ __forceinline__ void gemm_wg(const float* A, int lda, const float* Bp, int wave, int lane,
                                        const EpiArgs& e, const BPre<sub_max(NC / 2)>& pre,
                                        const float* AX = nullptr, int ldx = 0) {
    static_assert(NC % 2 == 0 && (R == 68 || R == 34), "row tiles x 2 column halves + tail rows");
    constexpr int NCW = NC / 2;
    constexpr int NRW = R == 68 ? 2 : 1;            // row tiles per wave
    const int pr = gemm_pr(wave);
    const bool dup = (NCW & 1) && pr == 1;
    if constexpr (NSUB == 1) {
        gemm_wave<NRW, NCW, TM_MFMA4, 0, NC, KB, MODE, XS2, NPRE>(A, lda, Bp, NRW * pr, gemm_ch(wave) * NCW,
                                                                 col_rot<NCW>(wave), R - R % 16, dup, lane, e, pre, AX, ldx);
    } else {
        constexpr int N0 = NCW / 2, N1 = NCW - N0;
        if (wave < 4)
            gemm_wave<NRW, NCW, TM_MFMA4, 0, NC, KB, MODE, XS2, NPRE, 0, N0, N1>(
                A, lda, Bp, NRW * pr, gemm_ch(wave) * NCW, col_rot<NCW>(wave), R - R % 16, dup, lane, e, pre, AX, ldx);
        else
            gemm_wave<NRW, NCW, TM_MFMA4, 0, NC, KB, MODE, XS2, NPRE, N0, N1, N1>(
                A, lda, Bp, NRW * pr, gemm_ch(wave) * NCW, col_rot<NCW>(wave), R - R % 16, dup, lane, e, pre, AX, ldx);
    }
}

// global column tile of local tile c of a pass starting at ctp, rotated by rot
template <int PW>
__device__ __forceinline__ int pass_col(int ctp, int c, int rot) {
    const int cc = c + rot;
    return ctp + (cc >= PW ? cc - PW : cc);
}

// ---------------------------------------------------------------------------------------
// Half-width-operand GEMMs of gemm modes 1 (f16x3) and 2 (bf16), round 5.  The activations stay
// the fp32 rows the fp32 mode keeps in LDS (every producer phase — LayerNorm, attention, the graph
// and Chebyshev products, the GEMM epilogues — is the fp32 mode's code), and the GEMM forms its
// v_mfma_f32_16x16x32_{bf16,f16} A fragments in registers from them: bf16 = one v_cvt_pk_bf16_f32
// per pair; f16x3 = hi = v_cvt_pk_f16_f32, lo = fp16(v - hi) (v - hi is exact in fp32).  Round 4 had
// each producer write [hi | lo] split rows instead, which cost every VALU phase and epilogue its
// conversions and twice the stores (r05_base phase trace: the split-row phases ran 26 % longer than
// the same phases of the fp32 mode).
// k order inside a 32-block: lane group g holds k = 4g..4g+3 and 16+4g..16+4g+3 (halves i < 4 and
// i >= 4 of its 8 operand values), so a fragment is two ds_read_b128 of an fp32 row at exactly the
// fp32 mode's conflict-free addresses (row strides ≡ 40 mod 64 dwords, gemm_wave); the packed weights
// use the same permutation (pack16, dpk_kernels.hip).
// Weights: f16x3 blocks [NC][KB32][hi 1 KiB | lo 1 KiB] (x W16_SCALE), bf16 blocks [NC][KB32][1 KiB].
#ifndef DPK_HS_BF
#define DPK_HS_BF 3      // bf16 column-half GEMMs with K > 96: B ring slots
#endif
#ifndef DPK_PWQ16
#define DPK_PWQ16 3      // f16x3 QKV at hid 96: column tiles per pass (of the wave's 9)
#endif
#ifndef DPK_PWF16
#define DPK_PWF16 3      // f16x3 fc1 at hid 96: column tiles per pass (of the wave's 6)
#endif
// The f16x3 column tiles per pass at each width, of the wave's 3 NCD / 2 (QKV), NCD (fc1) and NCD / 2 (O, fc2, the
// two Chebyshev GEMMs) column tiles.  A pass holds NRW x PW accumulator tiles (NRW = 2 row tiles on 4-pose
// workgroups, 1 on 2-pose ones) and an S-slot ring of PW hi + lo B fragments; a GEMM of several passes keeps its
// converted A fragments (ar[KB32][NRW + 1], 8 VGPRs each).  hid 96: the round-5 table (6 accumulator tiles a
// pass), for both graph patterns.  hid 64 (4-pose tiles, KB32_D = 2) and hid 128 (2-pose tiles, KB32_D = 4, one
// row tile a wave): the sparse-graph kernels' table is the measured one (profiles/f16x3_widths_bench.txt) and
// every one of them reports no scratch (make resources).  The dense-graph kernels spill whatever the table, as
// the fp32 ones do (52 - 84 bytes of scratch a lane at these widths): theirs is narrowed to 3 (QKV) and 2 tiles a
// pass, where their scratch is at the fp32 kernels' level (36 - 92 bytes; 228 - 484 with the sparse table).
#ifndef DPK_PW64
#define DPK_PW64 3, 4, 2     // hid 64, H36M-sparse graph: QKV (of 6), fc1 (of 4), the D-column GEMMs (of 2)
#endif
#ifndef DPK_PW128
#define DPK_PW128 6, 4, 4    // hid 128, H36M-sparse graph: QKV (of 12), fc1 (of 8), the D-column GEMMs (of 4)
#endif
template <bool SPARSE>
struct HPW {
    static constexpr int W64[3] = {DPK_PW64}, W128[3] = {DPK_PW128}, DENSE[3] = {3, 2, 2};
    static constexpr int pick(int i) { return !SPARSE ? DENSE[i] : D == 64 ? W64[i] : W128[i]; }
    static constexpr int QKV = D == 96 ? DPK_PWQ16 : pick(0);
    static constexpr int FC1 = D == 96 ? DPK_PWF16 : pick(1);
    static constexpr int O = D == 96 ? 3 : pick(2), FC2 = O, CHEB = O;
};
static_assert(D == 96 || D == 64 || D == 128, "HPW: a pass table per compiled width");
#ifndef DPK_PWF16_W8
#define DPK_PWF16_W8 6   // f16x3 fc1 on 8 waves
#endif
#ifndef DPK_PWQ16_W8
#define DPK_PWQ16_W8 9   // f16x3 QKV on 8 waves: column tiles per pass (of the SIMD's 9, split between its two waves)
#endif
constexpr int BLKB = 1024;
template <int G>
constexpr int blkh() { return G == 1 ? BLK16 : BLKB; }
// byte offset of GEMM block set `o16` (an O16_* offset) of layer l in the mode's arena
template <int G>
constexpr int offh(int l, int o16) { return G == 1 ? l * LAYER16_BYTES + o16 : (l * LAYER16_BYTES + o16) / 2; }
constexpr int ARENAB_BYTES = ARENA16_BYTES / 2;

template <int G>
struct AFr {
    f16x8 h, l;      // l: f16x3 only
};

__device__ __forceinline__ f16x8 cat2x4(f16x2 a, f16x2 b, f16x2 c, f16x2 d) {
    const f16x4 ab = __builtin_shufflevector(a, b, 0, 1, 2, 3), cd = __builtin_shufflevector(c, d, 0, 1, 2, 3);
    return __builtin_shufflevector(ab, cd, 0, 1, 2, 3, 4, 5, 6, 7);
}
// fragment from the lane's 8 fp32 values (k halves lo4 = 4g.., hi4 = 16+4g..)
template <int G>
__device__ __forceinline__ void acvt(const f32x4& lo4, const f32x4& hi4, AFr<G>& o) {
    const f32x2 v[4] = {f32x2{lo4[0], lo4[1]}, f32x2{lo4[2], lo4[3]}, f32x2{hi4[0], hi4[1]}, f32x2{hi4[2], hi4[3]}};
    f16x2 h[4], l[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        if constexpr (G == 2) {
            h[p] = __builtin_bit_cast(f16x2, __builtin_convertvector(v[p], bf16x2));
        } else {
            h[p] = __builtin_convertvector(v[p], f16x2);
            l[p] = __builtin_convertvector(v[p] - __builtin_convertvector(h[p], f32x2), f16x2);
        }
    }
    o.h = cat2x4(h[0], h[1], h[2], h[3]);
    if constexpr (G == 1) o.l = cat2x4(l[0], l[1], l[2], l[3]);
}

struct BSrcH {
    __amdgpu_buffer_rsrc_t rsrc;
    __device__ __forceinline__ f16x8 load(int voff, int soff) const {
        return __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff, 0));
    }
};
template <int G, int NC, int KB32>
__device__ __forceinline__ BSrcH bsrch(const char* Bp) {
    BSrcH s;
    s.rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)Bp, (short)0, NC * KB32 * blkh<G>(), 0x00020000);
    return s;
}

// B fragments of a pass's first two k-blocks (issued before the phase that precedes the GEMM)
template <int G, int PW>
struct BPreH {
    f16x8 h[2][PW], l[2][G == 1 ? PW : 1];
};
// the wave's tiles of pass `ps`: ctp + ((c + rot) mod PW), rot = ceil(PW/2) for the second wave of a
// column half (the tail tiles split between the pair, as gemm_wave)
template <int PW>
__device__ __forceinline__ int passh_rot(int wave) { return gemm_pr(wave) ? (PW + 1) / 2 : 0; }
template <int G, int NC, int KB32, int PW>
__device__ __forceinline__ BPreH<G, sub_max(PW)> gemmh_prefetch(const char* Bp, int wave, int lane, int ps = 0) {
    constexpr int BK = blkh<G>(), NP = sub_max(PW);
    const BSrcH s = bsrch<G, NC, KB32>(Bp);
    const int ctp = gemm_ch(wave) * (NC / 2) + ps * PW, rot = passh_rot<PW>(wave);
    BPreH<G, NP> pre;
    if constexpr (NSUB == 1) {
#pragma unroll
        for (int c = 0; c < PW; ++c) {
            const int voff = lane * 16 + pass_col<PW>(ctp, c, rot) * KB32 * BK;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                pre.h[k][c] = s.load(voff, k * BK);
                if constexpr (G == 1) pre.l[k][c] = s.load(voff, k * BK + 1024);
            }
        }
        return pre;
    }
    // 8 waves: the sub-wave's local tiles [c0, c0 + nown) of the pass (gemm_wave's split)
    const int c0 = (wave >> 2) * (PW / 2), nown = wave >> 2 ? PW - PW / 2 : PW / 2;
#pragma unroll
    for (int c = 0; c < NP; ++c) {
        const int voff = lane * 16 + pass_col<PW>(ctp, c0 + c, rot) * KB32 * BK;
        if (NSUB == 1 || c < nown) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                pre.h[k][c] = s.load(voff, k * BK);
                if constexpr (G == 1) pre.l[k][c] = s.load(voff, k * BK + 1024);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                pre.h[k][c] = f16x8{};
                if constexpr (G == 1) pre.l[k][c] = f16x8{};
            }
        }
    }
    return pre;
}

// One pass: the wave's NR row tiles (rt0..) and the 4 tail rows (trow0..) against PW column tiles of
// the pass, the k-loop fully unrolled over KB32 32-blocks with an S-slot register ring for B (from L2)
// and one k-block of look-ahead for the fp32 A rows (LDS), converted at the top of their k-block.
// The wave computes the tail rows of the first ceil(PW/2) of its (rotated) tiles, the column half's
// other wave the rest.  XS2: the 96 columns of k-blocks 0..2 come from AX (row stride ldx) — the
// Chebyshev GEMMs' T0 = x block where x lives (cheb_prep XSKIP).  AR: 0 A converted here; 1 converted
// here and kept in ar[KB32][NR+1] for the later passes of the same GEMM (f16x3, K = 96); 2 taken from ar.
// C0, NCS (8 waves): the wave computes the pass's local tiles [C0, C0 + NCS) and the tail tile against those of
// them that are tail tiles (local index < ceil(PW0/2)), as gemm_wave.
template <int G, int NR, int PW0, int NC, int KB32, int MODE, bool XS2, int S, int AR, int C0 = 0, int NCS = PW0,
          int NPW = PW0>
__device__ __forceinline__ void gemmh_pass(const float* A, int lda, const float* AX, int ldx, const BSrcH& src,
                                           int rt0, int ctp, int rot, int trow0, bool tail_dup, int lane,
                                           const EpiArgs& e, const BPreH<G, NPW>& pre, AFr<G> (*ar)[NR + 1]) {
    constexpr int BK = blkh<G>();
    constexpr int PW = NCS;                       // the wave's own tiles: local tile C0 + c
    constexpr int NQF = (PW0 + 1) / 2;            // tail tiles of the pass
    constexpr int TQ = NQF - C0 < 0 ? 0 : (NQF - C0 > NCS ? NCS : NQF - C0);   // ... of this wave
    constexpr int NQ = TQ > 0 ? TQ : 1;
    static_assert(C0 >= 0 && NCS >= 1 && C0 + NCS <= PW0 && NPW >= NCS, "sub-wave tile range");
    // The tail rows (trow0..): a padded 16-row tile on the same 16x16x32 MFMAs as the row tiles (rows past R
    // clamped to R - 1 on load, their results discarded).  Round 6 (T16): instead of 4x4x4 MFMAs whose k-slice
    // partials were reduce-scattered over the lane rows: +3.6 % on config 3 (bf16 K=100), +1.8 % f16x3 --
    // one 16x16x32 costs 19 cycles beside the row tiles' where the two 4x4x4 it replaces cost 25
    // (profiles/r05_mfma_h_probe.txt), and the tail epilogue is the tiles' (no permlane swaps, no MFMA-result
    // pad, 16-byte stores); profiles/r06_t16_ab.txt
    constexpr int NA = NR + (TQ > 0 ? 1 : 0);   // row tiles + the tail tile
    static_assert(S >= 2 && S <= KB32, "ring slots");
    lane = opaque(lane);
    const int rl = lane & 15, g = lane >> 4, kq = g * 4;
    int gcol[PW], voff[PW];
#pragma unroll
    for (int c = 0; c < PW; ++c) {
        gcol[c] = pass_col<PW0>(ctp, C0 + c, rot);
        voff[c] = lane * 16 + gcol[c] * KB32 * BK;
    }
    // A fragment sources: row tiles then the tail tile.  Row x stride as a 24-bit
    // multiply (v_mad_u32_u24): LLVM otherwise forms these with v_mad_u64_u32, whose undefined high
    // addend half it allocated to a register still being loaded (the epilogue constants), and the first
    // LDS read of the GEMM then waited at vmcnt(0) for the whole L2 round trip
    int aoff[NR + 1], xoff[NR + 1];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        aoff[i] = (int)__umul24((unsigned)((rt0 + i) * 16 + rl), (unsigned)lda) + kq;
        xoff[i] = (int)__umul24((unsigned)((rt0 + i) * 16 + rl), (unsigned)ldx) + kq;
    }
    const int trow_a = min(trow0 + rl, R - 1);
    aoff[NR] = (int)__umul24((unsigned)trow_a, (unsigned)lda) + kq;
    xoff[NR] = (int)__umul24((unsigned)trow_a, (unsigned)ldx) + kq;
    f32x4 raw[NR + 1][2];
    auto loadA = [&](int kb) {
        if constexpr (AR != 2) {
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const float* p = (XS2 && kb * 32 < D) ? AX + xoff[i] + kb * 32 : A + aoff[i] + kb * 32;
                raw[i][0] = *reinterpret_cast<const f32x4*>(p);
                raw[i][1] = *reinterpret_cast<const f32x4*>(p + 16);
            }
        }
    };
    f16x8 bh[S][PW], bl[S][G == 1 ? PW : 1];
    auto loadB = [&](int st, int kb) {
#pragma unroll
        for (int c = 0; c < PW; ++c) {
            bh[st][c] = src.load(voff[c], kb * BK);
            if constexpr (G == 1) bl[st][c] = src.load(voff[c], kb * BK + 1024);
        }
    };
    // epilogue constants: bias / temb projection quads of the lane's columns, through a descriptor on
    // the fp32 arena (a uniform tile offset in soffset, no 64-bit VALU address math); issued one k-block
    // ahead of the woven last one, so its MFMAs cover their L2 latency
    f32x4 bias4[PW], tp4[PW];
    auto load_epi = [&]() {
        const __amdgpu_buffer_rsrc_t br = __builtin_amdgcn_make_buffer_rsrc((void*)e.bias, (short)0, 0x7fffffff, 0x00020000);
#pragma unroll
        for (int c = 0; c < PW; ++c) {
            bias4[c] = MODE == E_STORE_NB ? f32x4{0.f, 0.f, 0.f, 0.f}
                                          : __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(br, kq * 4, gcol[c] * 64, 0));
            tp4[c] = (MODE == E_CHEB1 && e.tproj_pose_stride == 0)
                         ? *reinterpret_cast<const f32x4*>(e.tproj + gcol[c] * 16 + kq)
                         : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    // the ring: slots 0, 1 from the prefetch, the rest loaded here
#pragma unroll
    for (int c = 0; c < PW; ++c) {
        bh[0][c] = pre.h[0][c];
        bh[1][c] = pre.h[1][c];
        if constexpr (G == 1) {
            bl[0][c] = pre.l[0][c];
            bl[1][c] = pre.l[1][c];
        }
    }
#pragma unroll
    for (int st = 2; st < S; ++st) loadB(st, st);
    loadA(0);
    DPK_GEMM_HOOK(0);
    f32x4 acc[NR][PW], tacc[NQ];
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    AFr<G> af[NR + 1];
    auto cvt = [&](int kb) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            if constexpr (AR == 2) af[i] = ar[kb][i];
            else acvt<G>(raw[i][0], raw[i][1], af[i]);
            if constexpr (AR == 1) ar[kb][i] = af[i];
        }
    };
    // residual epilogues: the old tiles read with the last k-block, so their LDS latency hides under its
    // MFMAs instead of sitting in the epilogue (each wave reads only what it writes)
    constexpr bool RES = MODE == E_RESID || MODE == E_RESID_RELU;
    f32x4 oldv[NR][PW], oldt[NQ];
    auto load_old = [&]() {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const float* rp = e.dst + __umul24((unsigned)((rt0 + i) * 16 + rl), (unsigned)e.ldd) + kq;
#pragma unroll
            for (int c = 0; c < PW; ++c) oldv[i][c] = *reinterpret_cast<const f32x4*>(rp + gcol[c] * 16);
        }
#pragma unroll
        for (int q = 0; q < TQ; ++q)
            oldt[q] = *reinterpret_cast<const f32x4*>(e.dst + __umul24((unsigned)trow_a, (unsigned)e.ldd) + gcol[q] * 16 + kq);
    };
    // The epilogue is woven into the last k-block: the epilogue of the tile LAG tiles earlier rides behind
    // each tile's last MFMAs (the half-width MFMAs leave the VALU and LDS free while they run); the tail
    // rows' epilogue follows the last tile's.  Round 5 found a lag of 1 and a woven tail epilogue wrong (the
    // last pose of every 4-pose tile): the then 4x4x4 tail's asm reduce-scatter read the MFMA results too
    // soon.  With mfma_pad both were bitwise the unwoven kernel (round 6, profiles/r06_hazard_ab.txt), and
    // both slower than this form: lag 1 -0.3 % (bf16 K=100) / -0.5 % (f16x3), woven tails -1.7 % / -1.2 %
    constexpr int LAG = 2;
    constexpr int KEPI = KB32 - 2;     // k-block that issues the epilogue constants
    constexpr float INV = 1.0f / W16_SCALE;
    const f32x2 inv2 = {INV, INV};
    auto epi_tile = [&](int i, int c) {
        const int row = (rt0 + i) * 16 + rl;
        float* p = e.dst + __umul24((unsigned)row, (unsigned)e.ldd) + kq + gcol[c] * 16;
        const f32x4 old = RES ? oldv[i][c] : z;
        f32x4 tp = tp4[c];
        if (MODE == E_CHEB1 && e.tproj_pose_stride != 0) {
            const int pose = min(e.pose0 + row / J, e.pose_max);
            tp = *reinterpret_cast<const f32x4*>(e.tproj + (size_t)pose * e.tproj_pose_stride + gcol[c] * 16 + kq);
        }
        // acc / 64 + bias as one fma per value (the scale is a power of two: the same bits as
        // the product then the sum), packed
        const f32x4 a = acc[i][c];
        const f32x2 lo = __builtin_elementwise_fma(f32x2{a[0], a[1]}, inv2, f32x2{bias4[c][0], bias4[c][1]});
        const f32x2 hi = __builtin_elementwise_fma(f32x2{a[2], a[3]}, inv2, f32x2{bias4[c][2], bias4[c][3]});
        const f32x4 v = f32x4{lo[0], lo[1], hi[0], hi[1]};
        *reinterpret_cast<f32x4*>(p) = epi_value4<MODE, true>(v, z, tp, old);
    };
    auto tail_mfmas = [&](int st, int kb) {
#pragma unroll
        for (int q = 0; q < TQ; ++q) {
            f32x4 t = kb == 0 ? z : tacc[q];
            const f16x8 th = af[NR].h;
            if constexpr (G == 2) {
                t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, bh[st][q]), __builtin_bit_cast(bf16x8, th), t, 0, 0, 0);
            } else {   // the row tiles' order: lo(w) hi(a), hi(w) lo(a), hi(w) hi(a)
                t = __builtin_amdgcn_mfma_f32_16x16x32_f16(bl[st][q], th, t, 0, 0, 0);
                t = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh[st][q], af[NR].l, t, 0, 0, 0);
                t = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh[st][q], th, t, 0, 0, 0);
            }
            tacc[q] = t;
        }
    };
    // the tail tile's epilogue: lane (g, m) holds out[tail row m][cols 4g..4g+3] of column tile q, as in
    // epi_tile; rows past R (and the duplicated last tile when PW is odd) store nothing
    auto epi_tail = [&](int q) {
        const int row = trow0 + rl;
        f32x4 tp = tp4[q];
        if (MODE == E_CHEB1 && e.tproj_pose_stride != 0) {
            const int pose = min(e.pose0 + min(row, R - 1) / J, e.pose_max);
            tp = *reinterpret_cast<const f32x4*>(e.tproj + (size_t)pose * e.tproj_pose_stride + gcol[q] * 16 + kq);
        }
        const f32x4 a = tacc[q];
        const f32x2 lo = __builtin_elementwise_fma(f32x2{a[0], a[1]}, inv2, f32x2{bias4[q][0], bias4[q][1]});
        const f32x2 hi = __builtin_elementwise_fma(f32x2{a[2], a[3]}, inv2, f32x2{bias4[q][2], bias4[q][3]});
        f32x4 o = epi_value4<MODE, true>(f32x4{lo[0], lo[1], hi[0], hi[1]}, z, tp, RES ? oldt[q] : z);
        asm volatile("" : "+v"(o));   // formed on every lane: nothing sinks into the store branch
        const bool skip = (C0 + q == NQF - 1 && tail_dup) || row >= R;
        if (!skip) *reinterpret_cast<f32x4*>(e.dst + __umul24((unsigned)row, (unsigned)e.ldd) + gcol[q] * 16 + kq) = o;
    };
#pragma unroll
    for (int kb = 0; kb < KB32; ++kb) {
        const int st = kb % S;
        cvt(kb);
        if (kb + 1 < KB32) loadA(kb + 1);       // the next k-block's rows land under this one's MFMAs
        if (kb == KEPI) {
            load_epi();
            if constexpr (RES) load_old();
        }
        // transposed tiles (cf. GemmTile TRANS): the weight fragment is the MFMA's A operand
        const bool weave_kb = kb + 1 == KB32;
#pragma unroll
        for (int tt = 0; tt < NR * PW; ++tt) {
            const int i = tt / PW, c = tt % PW;
            const f32x4 cin = kb == 0 ? z : acc[i][c];
            if constexpr (G == 2) {
                acc[i][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, bh[st][c]),
                                                                    __builtin_bit_cast(bf16x8, af[i].h), cin, 0, 0, 0);
            } else {
                // the two small products first: lo(w) hi(a), hi(w) lo(a), then hi(w) hi(a)
                f32x4 t = __builtin_amdgcn_mfma_f32_16x16x32_f16(bl[st][c], af[i].h, cin, 0, 0, 0);
                t = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh[st][c], af[i].l, t, 0, 0, 0);
                acc[i][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh[st][c], af[i].h, t, 0, 0, 0);
            }
            if (weave_kb && tt >= LAG) {
                epi_tile((tt - LAG) / PW, (tt - LAG) % PW);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        tail_mfmas(st, kb);
        if (kb + S < KB32) loadB(st, kb + S);
        __builtin_amdgcn_sched_barrier(0);
    }
    DPK_GEMM_HOOK(1);
#pragma unroll
    for (int tt = NR * PW > LAG ? NR * PW - LAG : 0; tt < NR * PW; ++tt) epi_tile(tt / PW, tt % PW);
#pragma unroll
    for (int q = 0; q < TQ; ++q) epi_tail(q);
    DPK_GEMM_HOOK(2);
}

// Whole-workgroup half-width-operand GEMM: gemm_wg's wave roles (row tiles x column halves, the tail
// rows split between the two waves of a half), the wave's NC/2 column tiles in passes of PW.
// pre: the first pass's first two B k-blocks (gemmh_prefetch).
template <int G, int NC, int KB32, int PW, int MODE, bool XS2 = false>
__device__ __forceinline__ void gemmh_wg(const float* A, int lda, const char* Bp, int wave, int lane, const EpiArgs& e,
                                         const BPreH<G, sub_max(PW)>& pre, const float* AX = nullptr, int ldx = 0) {
    static_assert(NC % 2 == 0 && (NC / 2) % PW == 0 && (R == 68 || R == 34), "passes of PW column tiles");
    constexpr int NCW = NC / 2, NRW = R == 68 ? 2 : 1, NPASS = NCW / PW;
    // ring slots: all of a K <= 96 GEMM's k-blocks in flight (3 at hid 96, also for the 9-tile bf16 QKV pass;
    // 2 at hid 64), 3 for a longer K, unless the pass is wide (registers: 2); DPK_HS_BF for the bf16
    // K = 192 / 288 GEMMs (one 1 KiB fragment per tile and slot).  Slot kb % S: S need not divide KB32
    constexpr int S = PW >= 6 ? ((G == 2 && KB32 == 3) ? 3 : 2)
                              : (KB32 <= 3 ? KB32 : (G == 2 ? (DPK_HS_BF < KB32 ? DPK_HS_BF : KB32) : 3));
    const int pr = gemm_pr(wave);
    const int rot = passh_rot<PW>(wave);
    const bool dup = (PW & 1) && pr == 1;
    const BSrcH src = bsrch<G, NC, KB32>(Bp);
    const int ct0 = gemm_ch(wave) * NCW;
    // the wave's local tiles [c0, c0 + ncs) of every pass (8 waves: the sub-wave's share, gemm_wave's split)
    auto passes = [&](auto c0_, auto ncs_) {
        constexpr int C0 = decltype(c0_)::value, NCS = decltype(ncs_)::value, NPW = sub_max(PW);
        if constexpr (NPASS == 1) {
            gemmh_pass<G, NRW, PW, NC, KB32, MODE, XS2, S, 0, C0, NCS, NPW>(A, lda, AX, ldx, src, NRW * pr, ct0, rot,
                                                                            R - R % 16, dup, lane, e, pre, nullptr);
        } else {
            // later passes reuse the first pass's converted A fragments (K = D: KB32 = 2, 3 or 4)
            AFr<G> ar[KB32][NRW + 1];
            gemmh_pass<G, NRW, PW, NC, KB32, MODE, XS2, S, 1, C0, NCS, NPW>(A, lda, AX, ldx, src, NRW * pr, ct0, rot,
                                                                            R - R % 16, dup, lane, e, pre, ar);
#pragma unroll
            for (int ps = 1; ps < NPASS; ++ps) {
                const BPreH<G, NPW> p2 = gemmh_prefetch<G, NC, KB32, PW>(Bp, wave, lane, ps);
                gemmh_pass<G, NRW, PW, NC, KB32, MODE, XS2, S, 2, C0, NCS, NPW>(A, lda, AX, ldx, src, NRW * pr,
                                                                                ct0 + ps * PW, rot, R - R % 16, dup, lane,
                                                                                e, p2, ar);
            }
        }
    };
    if constexpr (NSUB == 1 && NPASS == 1) {
        gemmh_pass<G, NRW, PW, NC, KB32, MODE, XS2, S, 0>(A, lda, AX, ldx, src, NRW * pr, ct0, rot, R - R % 16, dup,
                                                          lane, e, pre, nullptr);
    } else if constexpr (NSUB == 1) {
        // later passes reuse the first pass's converted A fragments (K = D: KB32 = 2, 3 or 4)
        AFr<G> ar[KB32][NRW + 1];
        gemmh_pass<G, NRW, PW, NC, KB32, MODE, XS2, S, 1>(A, lda, AX, ldx, src, NRW * pr, ct0, rot, R - R % 16, dup,
                                                          lane, e, pre, ar);
#pragma unroll
        for (int ps = 1; ps < NPASS; ++ps) {
            const BPreH<G, PW> p2 = gemmh_prefetch<G, NC, KB32, PW>(Bp, wave, lane, ps);
            gemmh_pass<G, NRW, PW, NC, KB32, MODE, XS2, S, 2>(A, lda, AX, ldx, src, NRW * pr, ct0 + ps * PW, rot,
                                                              R - R % 16, dup, lane, e, p2, ar);
        }
    } else {
        constexpr int N0 = PW / 2;
        if (wave < 4) passes(std::integral_constant<int, 0>{}, std::integral_constant<int, N0>{});
        else passes(std::integral_constant<int, N0>{}, std::integral_constant<int, PW - N0>{});
    }
}

// The half-width-operand GEMM of one layer op: its first pass's B prefetch and the GEMM (gemmh_wg)
template <int G, int NC, int KB32, int PW>
struct HGemm {
    using Pre = BPreH<G, sub_max(PW)>;
    __device__ __forceinline__ static Pre prefetch(const char* Bp, int wave, int lane) {
        return gemmh_prefetch<G, NC, KB32, PW>(Bp, wave, lane);
    }
    template <int MODE, bool XS2 = false>
    __device__ __forceinline__ static void run(const float* A, int lda, const char* Bp, int wave, int lane,
                                               const EpiArgs& e, const Pre& pre, const float* AX = nullptr, int ldx = 0) {
        gemmh_wg<G, NC, KB32, PW, MODE, XS2>(A, lda, Bp, wave, lane, e, pre, AX, ldx);
    }
};

// Output ChebConv (96->5, one col tile): waves 0-3, wave w = row tile w + tail row 64+w; the
// raw accumulators go to a functor (DDIM update).
template <int KB>
__device__ __forceinline__ BPre<1> out_prefetch(const float* Bp, int lane) {
    const BSrc s = bsrc<1, KB>(Bp, 0, lane);
    BPre<1> pre;
    pre.b0[0] = s.load(0);
    pre.b1[0] = s.load(1);
    return pre;
}

template <int KB, int NCOL, class Epi>
__device__ __forceinline__ void gemm_out(const float* A, int lda, const float* Bp, int wave, int lane, Epi epi,
                                         const BPre<1>& pre) {
    using T = GemmTile<1, 1, TM_VALU, 1, KB, false>;
    static_assert(KB % 2 == 0, "k-blocks in pairs");
    lane = opaque(lane);
    T g;
    g.acc[0][0] = f32x4{0.f, 0.f, 0.f, 0.f};
    g.tl[0][0] = 0.f;
    const int rl = lane & 15, kq = (lane >> 4) * 4;
    g.aoff[0] = (wave * 16 + rl) * lda + kq;
    g.toff[0] = (R - R % 16 + wave) * lda + kq;
    const BSrc src = bsrc<1, KB>(Bp, 0, lane);
    const int soff[1] = {src.voff};
    f32x4 a0[1], t0[1], b0[1] = {pre.b0[0]}, a1[1], t1[1], b1[1] = {pre.b1[0]};
    g.loadA(a0, t0, A, 0);
    g.loadA(a1, t1, A, 1);
#pragma unroll 1
    for (int kb = 0; kb < KB - 2; kb += 2) {
        g.mma(a0, t0, b0);
        T::loadB(b0, src, soff, kb + 2);
        g.loadA(a0, t0, A, kb + 2);
        g.mma(a1, t1, b1);
        T::loadB(b1, src, soff, kb + 3);
        g.loadA(a1, t1, A, kb + 3);
    }
    g.mma(a0, t0, b0);
    g.mma(a1, t1, b1);
    const float tv = sum4rows(g.tl[0][0]);
    if (rl < NCOL) {
#pragma unroll
        for (int r = 0; r < 4; ++r) epi(wave * 16 + kq + r, rl, g.acc[0][0][r]);
        if (kq == 0) epi(R - R % 16 + wave, rl, tv);
    }
}
// ---------------------------------------------------------------------------------------
// all-reduce over the 16 lanes of a DPP row (row_ror: before sum4rows)
__device__ __forceinline__ float row_sum(float v) {
    v += row_ror<8>(v);
    v += row_ror<4>(v);
    v += row_ror<2>(v);
    return v + row_ror<1>(v);
}

// LayerNorm of GraFormer (GraFormer.py:58-70): a*(x-mean)/(std_unbiased + eps) + b.
// Rows 0..63: a DPP quad (4 lanes) per row, 16 rows per wave; lane `part` of a row owns the
// 16-byte chunks part, part+4, ..., part+20 (interleaved across LDS banks).  Rows 64..67: wave w
// takes row 64+w, 16 lanes x 6 elements (columns 2*lane + 32*e), lanes 16..63 mirror 0..15.
// One-pass fp32 statistics shifted by the row's first element (below); the cross-lane sums are
// DPP all-reduces whose operands pair up commutatively, so every lane of a row holds bitwise the
// same mean/std.
__device__ __forceinline__ float quad_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, v), __builtin_bit_cast(int, v),
                                                               0xB1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]
    return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, v), __builtin_bit_cast(int, v),
                                                                     0x4E, 0xf, 0xf, false));   // [2,3,0,1]
}
// POSEMAP (4-pose tiles): wave w takes pose w's rows 17w..17w+15 on quads and 17w+16 as its
// tail row, so a wave = pose consumer (graph_mma) can follow without a workgroup barrier.
// AFFINE = false: (x - mean) / (std + eps) only (the gain/shift folded into the consumer's weights).
// 1/(std + eps) (a Newton-refined reciprocal) is folded into the gain: one fma per element.
template <bool POSEMAP = false, bool AFFINE = true>
__device__ __forceinline__ void layer_norm(const float* src, float* dst, const float* gain, const float* shift,
                                           int tid) {
    tid = opaque(tid);
    const int w = tid >> 6, lane = tid & 63;
    // a row's D columns: lane `part` of its quad holds 16-byte chunks part, part + 4, ... (LNC of
    // them); the tail row's 16 lanes hold LNT pairs each (2 * tl + 32 e)
    constexpr int LNC = D / 16, LNT = D / 32;
    static_assert(!POSEMAP || R == 68, "pose-mapped LayerNorm: 4-pose tiles");
    constexpr float RD = 1.0f / (float)D, RD1 = 1.0f / (float)(D - 1);
    // ---- rows 0..63: wave w rows 16w..16w+15; row 64 + w: the tail row of wave w
    constexpr int RM = R - R % 16, RT = R % 16;
    // 68 rows: 4 row tiles + one tail row per wave; 34 rows (P = 2): waves 0, 1 take row tile w
    // and tail row 32 + w, waves 2, 3 have no rows
    static_assert((RM == 64 && RT == 4) || (RM == 32 && RT == 2), "row tiles + one tail row per wave");
    if constexpr (RM != 64 || NW > 4)   // 34-row tiles: waves 2, 3 idle; 8 waves: waves 4..7
        if (w >= RT) return;
    const int row = (POSEMAP ? w * J : w * 16) + (lane >> 2), part = lane & 3;
    const int trow = POSEMAP ? w * J + 16 : RM + w;
    const float* s = src + row * LDX;
    const int tl = lane & 15;
    const float* st = src + trow * LDX;
    // the row chunks, and the gains/shifts of the lane's columns, all issued up front: the
    // normalisation then waits on no LDS round trip (one per chunk when they were read there)
    f32x4 v[LNC], gv[LNC], sv[LNC];
    f32x2 u[LNT], tg[LNT], tsh[LNT];
#pragma unroll
    for (int e = 0; e < LNC; ++e) v[e] = *reinterpret_cast<const f32x4*>(s + 4 * (part + 4 * e));
#pragma unroll
    for (int e = 0; e < LNT; ++e) u[e] = *reinterpret_cast<const f32x2*>(st + 2 * tl + 32 * e);
    const float c0 = s[0], tc0 = st[0];
    if constexpr (AFFINE) {
#pragma unroll
        for (int e = 0; e < LNC; ++e) {
            gv[e] = *reinterpret_cast<const f32x4*>(gain + 4 * (part + 4 * e));
            sv[e] = *reinterpret_cast<const f32x4*>(shift + 4 * (part + 4 * e));
        }
#pragma unroll
        for (int e = 0; e < LNT; ++e) {
            tg[e] = *reinterpret_cast<const f32x2*>(gain + 2 * tl + 32 * e);
            tsh[e] = *reinterpret_cast<const f32x2*>(shift + 2 * tl + 32 * e);
        }
    }
    // One pass over the row, shifted by its first element c0 (every lane of the row reads the same
    // value): S1 = sum(x - c0), S2 = sum((x - c0)^2); mean = c0 + S1/96, var = (S2 - S1^2/96)/95
    // (unbiased, GraFormer.py:64).  With the shift inside the row's range the two sums stay of the
    // order of the variance, so the one-pass form loses nothing measurable against the two-pass
    // one, and the two reductions share one DPP chain.  Its worst case is a row whose outlier IS
    // element 0 (S2 = 96x the variance's numerator): with gconv_input.bias[0] + 10 eps is 4.3e-6 off
    // the fp64 oracle, against 1.3e-6 with the same outlier in channel 7, still inside the 5e-6 bar
    // (tests/test_gpu_input_regimes.py, bias+10_ch0 / _ch7).
    f32x4 d1 = {0.f, 0.f, 0.f, 0.f}, d2 = {0.f, 0.f, 0.f, 0.f};
    const f32x2 nc0 = vpair(-c0);
#pragma unroll
    for (int e = 0; e < LNC; ++e) {
        const f32x4 d = padd4(v[e], nc0);
        d1 += d;
        d2 = __builtin_elementwise_fma(d, d, d2);
    }
    f32x2 e1 = {0.f, 0.f}, e2 = {0.f, 0.f};
    // scalars that meet packed pairs go in as real pairs (vpair): LLVM otherwise reads the scalar's
    // register through op_sel with an unrelated register as the pair's high half, and the wait it
    // inserts for that half (a global load in flight, e.g. graph1's fragments issued just before
    // LN1) stalled the whole LayerNorm on L2 latency
    const f32x2 ntc0 = vpair(-tc0);
#pragma unroll
    for (int e = 0; e < LNT; ++e) {
        const f32x2 d = u[e] + ntc0;
        e1 += d;
        e2 = __builtin_elementwise_fma(d, d, e2);
    }
    const float s1 = quad_sum((d1[0] + d1[1]) + (d1[2] + d1[3]));
    const float s2 = quad_sum((d2[0] + d2[1]) + (d2[2] + d2[3]));
    const float t1 = row_sum(e1[0] + e1[1]);
    const float t2 = row_sum(e2[0] + e2[1]);
    const float mean = fmaf(s1, RD, c0), tmean = fmaf(t1, RD, tc0);
    const float var = fmaxf(fmaf(-s1 * RD, s1, s2), 0.f) * RD1;
    const float tvar = fmaxf(fmaf(-t1 * RD, t1, t2), 0.f) * RD1;
    const float den = __builtin_amdgcn_sqrtf(var) + LN_EPS, tden = __builtin_amdgcn_sqrtf(tvar) + LN_EPS;   // v_sqrt_f32 (1 ulp)
    const float rcp = rcp_nr(den), trcp = rcp_nr(tden);
    const f32x2 nmean = vpair(-mean), rcpp = vpair(rcp);
    const f32x2 ntmean = vpair(-tmean), trcpp = vpair(trcp);
    float* d = dst + row * LDX;
#pragma unroll
    for (int e = 0; e < LNC; ++e) {
        const int c = 4 * (part + 4 * e);
        f32x4 t;
        if constexpr (!AFFINE) t = pmul4(padd4(v[e], nmean), rcpp);
        else t = __builtin_elementwise_fma(padd4(v[e], nmean), pmul4(gv[e], rcpp), sv[e]);
        *reinterpret_cast<f32x4*>(d + c) = t;
    }
    // the tail row: lanes 16..63 mirror 0..15 and store nothing
    float* dt = dst + trow * LDX;
#pragma unroll
    for (int e = 0; e < LNT; ++e) {
        const int c = 2 * tl + 32 * e;
        f32x2 t;
        if constexpr (!AFFINE) t = (u[e] + ntmean) * trcpp;
        else t = __builtin_elementwise_fma(u[e] + ntmean, tg[e] * trcpp, tsh[e]);
        if (lane < 16) *reinterpret_cast<f32x2*>(dt + c) = t;
    }
}

// four fp32 values as a bf16x4 MFMA operand (round to nearest even)
__device__ __forceinline__ s16x4 bf4(float a, float b, float c, float d) {
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    const unsigned lo = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a, b}, bf16x2));
    const unsigned hi = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{c, d}, bf16x2));
    return __builtin_bit_cast(s16x4, u32x2{lo, hi});
}

// 4-head attention over the 17 joints of each pose (GraFormer.py:99-140, without the projections)
// on the matrix cores (v_mfma_f32_16x16x4_f32).  Wave w = pose w, the 4
// heads in turn.  Lane (g = l>>4, c = l&15) loads query/key row c at its 6 feature dims
// {4g..4g+3, 16+2g, 17+2g}, the k-slice it feeds to the MFMAs, so:
//   scores   S^T = K Q^T   (6 MFMAs): lane (g, c) ends with S[query c][keys 4g..4g+3];
//   key 16 / query 16      per-lane partial dot products over the lane's dims, summed over
//                          the 4 lane rows (permlane), so lane (g, c) also holds S[c][16],
//                          S[16][c] and S[16][16];
//   softmax  per query c: its 4 keys in registers, max/sum over the lane rows by permlane;
//   P.V      O^T = V^T P^T (4 MFMAs per 16-wide column tile; lane row g feeds keys 4g..4g+3,
//            the permuted order the scores left them in), so lane (g, c) ends with
//            O[query c][dims 4g..4g+3] of the tile: one 16-byte store; key 16 added by FMA;
//   query 16 lane (g, c) forms p16[c] * V[c][6g..6g+5], summed over the DPP row.
// The reference's arithmetic (scores / sqrt(d_k), masked keys -1e9, softmax, P.V) in fp32, with
// the scale taken as one multiply by log2(e)/sqrt(d_k) and exp(x) as 2^x (v_exp_f32): the
// softmax is invariant to the base, so only roundings and summation orders differ.
// GA = 2 (gemm mode 2, BASELINE config 3's bf16 study): the score and P.V products on
// v_mfma_f32_16x16x32_bf16 / 16x16x16_bf16 from bf16-rounded Q, K, V and probabilities (fp32
// accumulate; the softmax and the normalisation stay fp32), joint 16's products included (A16): 4 + 4
// MFMAs per head instead of 12 + 8 f32 MFMAs and the key-16 / query-16 VALU sums.  Lane group g's 8 score operands are dims {4g..4g+3} and {16+4g..16+4g+3} (zero
// past d_k), the same k-permutation on both operands.
// PADK (padded tiles: a pose of nk < 17 joints, rows nk..16 dead): keys nk..16 are excluded hard, probability
// exactly 0, on top of their mask bits being 0: the soft fill alone would leave a query whose keys are all
// masked uniform over 17 keys where the nk-joint reference is uniform over nk.
template <int GA = 0, bool PADK = false, class Hook = NoHook>
__device__ __forceinline__ void attention_mma(const float* qkv, float* out, unsigned mask, int wave, int lane,
                                              const Hook& hook = Hook{}, int nk = J) {
    static_assert(GA == 0 || DK == 24, "bf16 attention: d_k 24");
    static_assert(GA == 0 || !PADK, "padded tiles: fp32 attention");
    // A16 (mode 2): the 17th joint's products on the matrix cores too: key 16's scores S[c][16] and
    // S[16][16] as a 16x16x32 bf16 product with key 16's row broadcast as the A operand (every output row
    // is the same dot products), and query 16's P.V with its probabilities broadcast as the B operand
    // (every output column is O[16][.]; V's ones rows give its denominator) -- instead of per-lane fp32
    // partial dot products summed over the lane rows by permlane swaps.  Round 6: +2.7 % on config 3 (bf16,
    // K=100), and the study's MPJPE delta on 1,024 frames 4.5e-3 -> 3.0e-3 mm (the 17th joint's products now
    // round like the other joints'), profiles/r06_attn_ab.txt
    constexpr bool A16 = GA == 2;
    lane = opaque(lane);
    // 4-pose tiles: wave w = pose w, all 4 heads; 2-pose tiles: waves 2p, 2p+1 = pose p, heads
    // {0,1} and {2,3} (the heads are independent: same arithmetic per head either way)
    constexpr int WPP = NW / P, HW = NH / WPP;
    static_assert(WPP * P == NW && HW * WPP == NH, "waves per pose");
    wave = opaque_s(wave);
    const int pose = WPP == 1 ? wave : wave / WPP;
    const int hoff = WPP == 1 ? 0 : (wave % WPP) * HW * DK;
    if (pose >= P) return;
    const int g = lane >> 4, c = lane & 15;
    constexpr float LOG2E = 1.4426950408889634f;
    const float sl = (1.0f / SQRT_DK) * LOG2E;      // scores in log2 units: exp(s/sqrt(dk)) = 2^(dot*sl)
    const float* prow = qkv + pose * J * LD2 + hoff;
    float* orow = out + pose * J * LDX + hoff;
    const bool kok16 = ((mask >> 16) & 1u) != 0u;
    bool kokr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) kokr[r] = ((mask >> (4 * g + r)) & 1u) != 0u;
    // scores / sqrt(d_k), masked keys -1e9 (GraFormer.py:104-106), kept in log2 units (scaled by
    // log2 e with the 1/sqrt(d_k)) so the softmax's exp is one v_exp_f32 (2^x) of (score - max) <= 0
    // as fma(dot, ok ? sl : 0, ok ? 0 : -1e9): dot * sl exactly for kept keys (fma with a zero addend is
    // the rounded product), exactly -1e9 for masked ones
    auto scale = [&](float dot, bool ok) { return fmaf(dot, ok ? sl : 0.f, ok ? 0.f : -1e9f); };
    auto ex = [&](float x) { return __builtin_amdgcn_exp2f(x); };
    // The 4 heads are independent: every stage below runs over all of them before the next
    // stage, so the in-order issue interleaves 4 dependency chains (MFMA accumulations,
    // permlane reductions, exp) instead of waiting out one head's latencies at a time.
    f32x4 q4[HW], k4[HW], Q4[HW], K4[HW], V4a[HW], V4b[HW];
    f32x2 q2[HW], k2[HW], Q2[HW], K2[HW];
    f32x4 qh[HW], kh[HW], Qh[HW], Kh[HW];     // GA == 2, d_k 32: dims 16 + 4g..16 + 4g + 3
    float va[HW][4], vb[HW][4];
#pragma unroll
    for (int h = 0; h < HW; ++h) {
        const float* rc = prow + h * DK + c * LD2;
        const float* r16 = prow + h * DK + 16 * LD2;
        q4[h] = *reinterpret_cast<const f32x4*>(rc + 4 * g);
        k4[h] = *reinterpret_cast<const f32x4*>(rc + D + 4 * g);
        Q4[h] = *reinterpret_cast<const f32x4*>(r16 + 4 * g);
        K4[h] = *reinterpret_cast<const f32x4*>(r16 + D + 4 * g);
        if constexpr (GA == 2 || DK == 32) {   // dims 16 + 4g.. (d_k 24: lane groups 2, 3 re-read 16..23)
            // loaded unconditionally, with selects: at d_k 24 the lane groups past d_k get zeros in the key
            // operands only (kb's high half below, Kh here), so their products are zeros whatever the query
            // values (round 6, with A16: +0.5 % over exec-masked loads; without A16 it measured -0.7 %)
            const int o2 = 16 + 4 * (DK == 32 ? g : (g & 1));
            qh[h] = *reinterpret_cast<const f32x4*>(rc + o2);
            kh[h] = *reinterpret_cast<const f32x4*>(rc + D + o2);
            Qh[h] = *reinterpret_cast<const f32x4*>(r16 + o2);
            Kh[h] = *reinterpret_cast<const f32x4*>(r16 + D + o2);
            if constexpr (DK == 24) Kh[h] = g < 2 ? Kh[h] : f32x4{0.f, 0.f, 0.f, 0.f};
        } else if constexpr (DK == 24) {       // (d_k 16: dims 4g..4g+3 are all of the lane group's)
            q2[h] = *reinterpret_cast<const f32x2*>(rc + 16 + 2 * g);
            k2[h] = *reinterpret_cast<const f32x2*>(rc + D + 16 + 2 * g);
            Q2[h] = *reinterpret_cast<const f32x2*>(r16 + 16 + 2 * g);
            K2[h] = *reinterpret_cast<const f32x2*>(r16 + D + 16 + 2 * g);
        }
    }
    // ---- scores S^T = K Q^T and, with query 16's row broadcast to every column,
    //      S16 = K q16 (6 MFMAs each per head): lane (g, c) holds S[c][4g+r] and S[16][4g+r]
    f32x4 st[HW], st16[HW];
    f32x4 sk16[HW], skk[HW];                    // A16: S[c][16], S[16][16] (every register the same)
#pragma unroll
    for (int h = 0; h < HW; ++h) {
        st[h] = f32x4{0.f, 0.f, 0.f, 0.f};
        st16[h] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // V operands: column tile 0 (dims 0..15) and 1 (dims 16..23 in rows c < 8, ones in rows
    // c >= 8: those rows of P.V come out as the softmax denominators, below); d_k 16: tile 1 is all
    // ones, so every row of its product is a denominator
    auto load_v = [&]() {
#pragma unroll
        for (int h = 0; h < HW; ++h) {
            const float* vbase = prow + h * DK + 2 * D;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                va[h][r] = vbase[(4 * g + r) * LD2 + c];
                if constexpr (DK == 32) {
                    vb[h][r] = vbase[(4 * g + r) * LD2 + 16 + c];
                } else if constexpr (DK == 24) {
                    const float v1 = vbase[(4 * g + r) * LD2 + 16 + (c & 7)];   // unconditional load, then select
                    vb[h][r] = c < 8 ? v1 : 1.0f;
                } else {
                    vb[h][r] = 1.0f;
                }
            }
            V4a[h] = *reinterpret_cast<const f32x4*>(vbase + 16 * LD2 + 4 * g);
            if constexpr (DK == 24) V4b[h] = *reinterpret_cast<const f32x4*>(vbase + 16 * LD2 + 16 + 4 * (g & 1));
            if constexpr (DK == 32) V4b[h] = *reinterpret_cast<const f32x4*>(vbase + 16 * LD2 + 16 + 4 * g);
        }
    };
    if constexpr (GA == 2) {
#pragma unroll
        for (int h = 0; h < HW; ++h) {
            AFr<2> fk, fq, fQ;
            acvt<2>(k4[h], kh[h], fk);
            acvt<2>(q4[h], qh[h], fq);
            acvt<2>(Q4[h], Qh[h], fQ);
            if constexpr (DK == 24) {     // lane groups 2, 3: dims 24..31 of the k-slice are past d_k
                typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
                u32x4 kw = __builtin_bit_cast(u32x4, fk.h);
                kw[2] = g < 2 ? kw[2] : 0u;
                kw[3] = g < 2 ? kw[3] : 0u;
                fk.h = __builtin_bit_cast(f16x8, kw);
            }
            const bf16x8 kb = __builtin_bit_cast(bf16x8, fk.h);
            st[h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kb, __builtin_bit_cast(bf16x8, fq.h), st[h], 0, 0, 0);
            st16[h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kb, __builtin_bit_cast(bf16x8, fQ.h), st16[h], 0, 0, 0);
            if constexpr (A16) {
                AFr<2> fK;                          // key 16's row (Kh: zero past d_k), the same in every lane row
                acvt<2>(K4[h], Kh[h], fK);
                const bf16x8 k16 = __builtin_bit_cast(bf16x8, fK.h);
                const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
                sk16[h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k16, __builtin_bit_cast(bf16x8, fq.h), z4, 0, 0, 0);
                skk[h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k16, __builtin_bit_cast(bf16x8, fQ.h), z4, 0, 0, 0);
            }
        }
    } else {
#pragma unroll
    for (int m = 0; m < DK / 4; ++m)
#pragma unroll
        for (int h = 0; h < HW; ++h) {
            const float kk = m < 4 ? k4[h][m & 3] : DK == 32 ? kh[h][m & 3] : k2[h][m & 1];
            const float qq = m < 4 ? q4[h][m & 3] : DK == 32 ? qh[h][m & 3] : q2[h][m & 1];
            const float QQ = m < 4 ? Q4[h][m & 3] : DK == 32 ? Qh[h][m & 3] : Q2[h][m & 1];
            st[h] = __builtin_amdgcn_mfma_f32_16x16x4f32(kk, qq, st[h], 0, 0, 0);
            st16[h] = __builtin_amdgcn_mfma_f32_16x16x4f32(kk, QQ, st16[h], 0, 0, 0);
        }
    }
    if constexpr (!__is_same(Hook, NoHook)) {
        __builtin_amdgcn_sched_barrier(0);
        hook();
        __builtin_amdgcn_sched_barrier(0);
    }
    load_v();
    // ---- key 16 by partial dots over this lane's 6 dims, summed over the lane rows:
    //      S[c][16] and S[16][16]
    float s_c16[HW], s_1616[HW];
    if constexpr (A16) {
#pragma unroll
        for (int h = 0; h < HW; ++h) {
            s_c16[h] = scale(sk16[h][0], kok16);
            s_1616[h] = scale(skk[h][0], kok16);
        }
    } else {
#pragma unroll
    for (int h = 0; h < HW; ++h) {
        float pa = 0.f, pc = 0.f;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            pa = fmaf(q4[h][m], K4[h][m], pa);
            pc = fmaf(Q4[h][m], K4[h][m], pc);
        }
        if constexpr (GA == 2 || DK == 32) {
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                pa = fmaf(qh[h][m], Kh[h][m], pa);
                pc = fmaf(Qh[h][m], Kh[h][m], pc);
            }
        } else if constexpr (DK == 24) {
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                pa = fmaf(q2[h][m], K2[h][m], pa);
                pc = fmaf(Q2[h][m], K2[h][m], pc);
            }
        }
        s_c16[h] = pa;
        s_1616[h] = pc;
    }
#pragma unroll
    for (int h = 0; h < HW; ++h) {
        sum4rows2(s_c16[h], s_1616[h]);
        s_c16[h] = scale(s_c16[h], kok16);
        s_1616[h] = scale(s_1616[h], kok16);
    }
    }
    // ---- softmax of query c and of query 16 over keys 4g+r (this lane) and 16
    float p[HW][4], p16[HW], u[HW][4], u16[HW], mx[HW], my[HW];
#pragma unroll
    for (int h = 0; h < HW; ++h) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            p[h][r] = scale(st[h][r], kokr[r]);
            u[h][r] = scale(st16[h][r], kokr[r]);
        }
    }
    // The max shift only guards 2^x against overflow / total underflow.  When
    // every score of the wave (masked keys' dot products included) is within +-64 in log2 units
    // and some key is kept, 2^score lies in [2^-64, 2^64] and the unshifted softmax is the same
    // quotient (one wave vote instead of the lane-row max reductions); else the shifted form.
    // the MFMA dots are unscaled, s_c16 / s_1616 already in log2 units
    float big = 0.f, big2 = 0.f;
#pragma unroll
    for (int h = 0; h < HW; ++h) {
#pragma unroll
        for (int r = 0; r < 4; ++r) big = fmaxf(big, fmaxf(fabsf(st[h][r]), fabsf(st16[h][r])));
        big2 = fmaxf(big2, fmaxf(fabsf(s_c16[h]), fabsf(s_1616[h])));
    }
    big = fmaxf(big * sl, big2);
    const bool shift = (mask & ((1u << J) - 1u)) == 0u || __builtin_amdgcn_ballot_w64(!(big <= 64.f)) != 0;
    if (!shift) {
#pragma unroll
        for (int h = 0; h < HW; ++h) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                p[h][r] = ex(p[h][r]);
                u[h][r] = ex(u[h][r]);
            }
            p16[h] = ex(s_c16[h]);
            u16[h] = ex(s_1616[h]);
        }
    } else {
#pragma unroll
    for (int h = 0; h < HW; ++h) {
        mx[h] = fmaxf(fmaxf(p[h][0], p[h][1]), fmaxf(p[h][2], p[h][3]));
        my[h] = fmaxf(fmaxf(u[h][0], u[h][1]), fmaxf(u[h][2], u[h][3]));
    }
#pragma unroll
    for (int h = 0; h < HW; ++h) {
        max4rows2(mx[h], my[h]);
        mx[h] = fmaxf(mx[h], s_c16[h]);
        my[h] = fmaxf(my[h], s_1616[h]);
    }
    // unnormalised probabilities; the denominators come out of the P.V products (ones rows)
#pragma unroll
    for (int h = 0; h < HW; ++h) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            p[h][r] = ex(p[h][r] - mx[h]);
            u[h][r] = ex(u[h][r] - my[h]);
        }
        p16[h] = ex(s_c16[h] - mx[h]);
        u16[h] = ex(s_1616[h] - my[h]);
    }
    }
    if constexpr (PADK) {
        // dead keys out of numerators and denominators alike (their V rows are finite: 0 * v = 0); key 16 is
        // dead on every padded tile
#pragma unroll
        for (int h = 0; h < HW; ++h) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool live = 4 * g + r < nk;
                p[h][r] = live ? p[h][r] : 0.f;
                u[h][r] = live ? u[h][r] : 0.f;
            }
            p16[h] = 0.f;
            u16[h] = 0.f;
        }
    }
    // ---- O^T = V^T P^T over keys 0..15 (4 MFMAs per column tile), then key 16 by FMA;
    //      query 16: this lane's keys 4g+r against V columns c and 16+c, summed over lane rows
    f32x4 oa[HW], ob[HW];
    f32x4 oa16[HW], ob16[HW];                   // A16: query 16's P.V (every column the same)
    float ya[HW], yb[HW];
#pragma unroll
    for (int h = 0; h < HW; ++h) {
        oa[h] = f32x4{0.f, 0.f, 0.f, 0.f};
        ob[h] = f32x4{0.f, 0.f, 0.f, 0.f};
        ya[h] = 0.f;
        yb[h] = 0.f;
    }
    if constexpr (GA == 2) {
        // keys 4g..4g+3 of the lane are exactly the 16x16x16 operand's k-slice of lane group g
#pragma unroll
        for (int h = 0; h < HW; ++h) {
            const s16x4 pb = bf4(p[h][0], p[h][1], p[h][2], p[h][3]);
            const s16x4 vab = bf4(va[h][0], va[h][1], va[h][2], va[h][3]), vbb = bf4(vb[h][0], vb[h][1], vb[h][2], vb[h][3]);
            oa[h] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(vab, pb, oa[h], 0, 0, 0);
            ob[h] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(vbb, pb, ob[h], 0, 0, 0);
            if constexpr (A16) {
                const s16x4 ub = bf4(u[h][0], u[h][1], u[h][2], u[h][3]);
                const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
                oa16[h] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(vab, ub, z4, 0, 0, 0);
                ob16[h] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(vbb, ub, z4, 0, 0, 0);
            }
        }
    } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int h = 0; h < HW; ++h) {
            oa[h] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[h][r], p[h][r], oa[h], 0, 0, 0);
            ob[h] = __builtin_amdgcn_mfma_f32_16x16x4f32(vb[h][r], p[h][r], ob[h], 0, 0, 0);
        }
    }
    if constexpr (!A16) {
        // query 16's products as one VALU cluster after the MFMAs (between them each costs 12 cycles)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int h = 0; h < HW; ++h) {
                ya[h] = fmaf(u[h][r], va[h][r], ya[h]);
                yb[h] = fmaf(u[h][r], vb[h][r], yb[h]);
            }
#pragma unroll
        for (int h = 0; h < HW; ++h) sum4rows2(ya[h], yb[h]);
    }
    // denominators: query c's over keys 0..15 sits in ob rows 8..15 (lane rows g >= 2), moved to
    // lane rows 0,1 by one permlane32 swap; query 16's over keys 0..15 is yb of lanes c >= 8,
    // moved to lanes c < 8 of the DPP row by a rotation by 8; key 16 added to both
    float rs[HW], rs16[HW];
    if constexpr (DK == 24) mfma_pad<PAD_MFMA16>(ob);   // the swap below reads the P.V accumulators inside asm
    if constexpr (A16) mfma_pad<PAD_MFMA16>(ob16);
#pragma unroll
    for (int h = 0; h < HW; ++h) {
        float den, den16;
        if constexpr (DK == 32) {       // no spare V rows: the lane's 4 probabilities summed over the lane rows
            float sp = (p[h][0] + p[h][1]) + (p[h][2] + p[h][3]), su = (u[h][0] + u[h][1]) + (u[h][2] + u[h][3]);
            sum4rows2(sp, su);
            den = sp + p16[h];
            den16 = su + u16[h];
        } else if constexpr (DK == 24) {
            float sa = ob[h][0], sb = ob[h][0];
            asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(sa), "+v"(sb));
            den = (g < 2 ? sb : ob[h][0]) + p16[h];
            if constexpr (A16) {        // query 16's over keys 0..15: ob16's ones rows, moved the same way
                float ta = ob16[h][0], tb = ob16[h][0];
                asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(ta), "+v"(tb));
                den16 = (g < 2 ? tb : ob16[h][0]) + u16[h];
            } else {
                const float yr = row_ror<8>(yb[h]);
                den16 = (c < 8 ? yr : yb[h]) + u16[h];
            }
        } else {                        // d_k 16: every lane's ob / yb is the sum over keys 0..15
            den = ob[h][0] + p16[h];
            den16 = yb[h] + u16[h];
        }
        rs[h] = __builtin_amdgcn_rcpf(den);
        rs16[h] = __builtin_amdgcn_rcpf(den16);
    }
    // ---- stores: O[c][h*24 + 4g..] (tile 0), O[c][h*24 + 16 + 4g..] (tile 1, g < 2);
    //      O[16][h*24 + c] and O[16][h*24 + 16 + c] (c < 8) from lane row 0
#pragma unroll
    for (int h = 0; h < HW; ++h) {
        const f32x4 p4 = {p16[h], p16[h], p16[h], p16[h]};
        oa[h] = __builtin_elementwise_fma(p4, V4a[h], oa[h]) * rs[h];
        const float* v16 = prow + h * DK + 16 * LD2 + 2 * D;
        const int col = h * DK;
        *reinterpret_cast<f32x4*>(orow + c * LDX + col + 4 * g) = oa[h];
        if constexpr (A16) {            // O[16][dims 4g..] from lane (g, 0) of each lane row
            const f32x4 u4 = {u16[h], u16[h], u16[h], u16[h]};
            const f32x4 o16a = __builtin_elementwise_fma(u4, V4a[h], oa16[h]) * rs16[h];
            const f32x4 o16b = __builtin_elementwise_fma(u4, V4b[h], ob16[h]) * rs16[h];
            if (c == 0) *reinterpret_cast<f32x4*>(orow + 16 * LDX + col + 4 * g) = o16a;
            if (c == 0 && g < 2) *reinterpret_cast<f32x4*>(orow + 16 * LDX + col + 16 + 4 * g) = o16b;
        } else if (g == 0) {
            orow[16 * LDX + col + c] = fmaf(u16[h], v16[c], ya[h]) * rs16[h];
        }
        if constexpr (DK == 24) {
            ob[h] = __builtin_elementwise_fma(p4, V4b[h], ob[h]) * rs[h];
            if (g < 2) *reinterpret_cast<f32x4*>(orow + c * LDX + col + 16 + 4 * g) = ob[h];
            if (!A16 && g == 1 && c < 8) orow[16 * LDX + col + 16 + c] = fmaf(u16[h], v16[16 + c], yb[h]) * rs16[h];
        } else if constexpr (DK == 32) {
            ob[h] = __builtin_elementwise_fma(p4, V4b[h], ob[h]) * rs[h];
            *reinterpret_cast<f32x4*>(orow + c * LDX + col + 16 + 4 * g) = ob[h];
            if (g == 1) orow[16 * LDX + col + 16 + c] = fmaf(u16[h], v16[16 + c], yb[h]) * rs16[h];
        }
    }
}

// --- graph products -------------------------------------------------------------------

// Chebyshev prologue: B2 = [T1 src | T2 src | src] (ChebConv.py:83, term order rotated so the
// K=288 GEMM reads one buffer; the packed weights follow the same order).
// Wave w = pose w, lane = column pair (lanes 48..63 idle), so a wave reads only rows its own
// earlier LDS writes produced when it follows graph_mma (no workgroup barrier in between).
// SPARSE: compile-time pattern, packed values (scalar loads); dense: 17x17 from the arena.
// Sums run over increasing i in both (identical bits).
// XSKIP (fp32 GEMM mode, Cheb1/Cheb2): write [- | T1 src | T2 src] and let the GEMM read the
// T0 = src part from src itself (gemm_wave XS2), saving a third of the stores.
template <bool SPARSE, bool XSKIP = false>
__device__ __forceinline__ void cheb_prep(const float* __restrict__ cw, const float* src, float* b2, int wave,
                                          int lane) {
    lane = opaque(lane);
    // 4-pose tiles: wave w = pose w, lane = column pair; 2-pose tiles: waves 2p, 2p+1 = pose p,
    // columns 0..47 and 48..95 (the split graph_mma uses, so graph2 + cheb_prep1 stay barrier-free)
    constexpr int WPP = NW / P, G = 2, ng = D / G / WPP;
    static_assert(ng <= 64 && P <= NW, "one pose per wave, one column pair per lane");
    wave = opaque_s(wave);
    const int p = WPP == 1 ? wave : wave / WPP;
    if (p >= P || lane >= ng) return;
    const int c = lane * G + (WPP == 1 ? 0 : (wave % WPP) * (D / WPP));
    // one VGPR base per buffer, rows at compile-time offsets (folded into the ds_read/ds_write
    // offset field; per-row SGPR offsets were hoisted out of the step loop and spilled)
    const float* sp = src + opaque(p * J * LDX + c);
    float* dp = b2 + opaque(p * J * LD2 + c);
    f32x2 v[J];
#pragma unroll
    for (int i = 0; i < J; ++i) v[i] = *reinterpret_cast<const f32x2*>(sp + i * LDX);
    // T1 x = L x; T2 x = (2 L^2 - I) x by the Chebyshev recurrence 2 L (L x) - x (ChebConv.py:90-112
    // builds T2 as a matrix first; the recurrence needs L's 49 nonzeros twice instead of T2's 87)
    auto lx = [&](int j, const f32x2 (&u)[J]) {
        f32x2 acc = {0.f, 0.f};
        if constexpr (SPARSE) {
#pragma unroll
            for (int k = 0; k < SPAT.n1[j]; ++k) acc = pfma(splat2(cw[SPAT.o1[j] + k]), u[SPAT.c1[j][k]], acc);
        } else {
#pragma unroll
            for (int i = 0; i < J; ++i) acc = pfma(splat2(cw[j * J + i]), u[i], acc);
        }
        return acc;
    };
    f32x2 t1[J];
#pragma unroll
    for (int j = 0; j < J; ++j) t1[j] = lx(j, v);
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const f32x2 t2 = pfma(splat2(2.0f), lx(j, t1), -v[j]);
        if constexpr (XSKIP) {
            *reinterpret_cast<f32x2*>(dp + j * LD2 + D) = t1[j];
            *reinterpret_cast<f32x2*>(dp + j * LD2 + 2 * D) = t2;
        } else {
            *reinterpret_cast<f32x2*>(dp + j * LD2) = t1[j];
            *reinterpret_cast<f32x2*>(dp + j * LD2 + D) = t2;
            *reinterpret_cast<f32x2*>(dp + j * LD2 + 2 * D) = v[j];
        }
    }
}

// GraphNet product on the matrix cores: wave w = pose w computes out^T = X^T L^T for its 17
// rows with v_mfma_f32_16x16x4_f32 (M = 96 columns in 6 tiles, N = joints 0..15, K = joints in
// 5 steps of 4, rows past 16 clamped and multiplied by zero), so lane l ends with out[j = l&15]
// [c .. c+3] (16-byte stores).  Joint 16 (the 17th output row) from the same A fragments:
// per-lane partial sums over the lane's k-slice, summed over the 4 lane groups by permlane.
// LF: the layer's fragments (OFF_LGF): [s][lane] = L[lane&15][4s + (lane>>4)] and
// [5 + s][lane] = L[16][4s + (lane>>4)] (0 past joint 16).
//   RESID:     dst (stride LDX) += out + bias          (graph2: x + L (Y W2^T) + b2)
//   else:      dst (stride LDX) = out (in place allowed: each wave reads its rows before writing)
// The fragments are loaded one phase ahead (gfrag_load) so their L2 latency hides there.
// BIAS (graph2): also the lane's fc2 bias columns, so the RESID epilogue waits on no global load.
struct GFrag {
    float lb[5], l16[5];
    f32x4 b4[NCD];
    float b1[2];    // 6 tiles per wave: joint-16 row's bias of column cl of tiles g and 4 + (g & 1) (graph_mma's map)
    bf16x8 lh;      // GA == 2: L[cl][4g..4g+3], L[cl][16] (g = 0) as the bf16 operand's k-slice of lane group g
    bf16x8 ll;      // GA == 2: the bf16 residual L - lh (L to ~16 bits in two products)
    float m16[5];   // GA == 2: L[16][4g..4g+3], L[16][16] (g = 0) for joint 16's output row (fp32)
};
__device__ __forceinline__ GFrag gfrag_load(const float* __restrict__ LF, int lane) {
    GFrag f;
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        f.lb[s] = LF[s * 64 + lane];
        f.l16[s] = LF[(5 + s) * 64 + lane];
    }
    return f;
}
// GA == 2 operands straight from the layer's row-major L_g (OFF_LG): the 16x16x32 bf16 product's k-slice
// of lane group g is joints {4g..4g+3} and {16 + 4g..}, of which only joint 16 (g = 0) exists.  L_g as a
// bf16 hi + lo pair: a single bf16-rounded L_g biases every layer and step alike (round 5: config 3's
// MPJPE delta 1.7e-3 -> 5.6e-2 mm), the pair holds it to ~16 bits
__device__ __forceinline__ GFrag gfrag_load_h(const float* __restrict__ LG, int lane) {
    GFrag f;
    const int g = lane >> 4, cl = lane & 15;
    const float* Lr = LG + cl * J + 4 * g;
    const float* L16 = LG + 16 * J + 4 * g;
    f32x4 lo, hi = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        lo[e] = Lr[e];
        f.m16[e] = L16[e];
    }
    const float l_c16 = LG[cl * J + 16], l_1616 = LG[16 * J + 16];
    hi[0] = g == 0 ? l_c16 : 0.f;
    f.m16[4] = g == 0 ? l_1616 : 0.f;
    AFr<2> fr;
    acvt<2>(lo, hi, fr);
    f.lh = __builtin_bit_cast(bf16x8, fr.h);
    // residuals of the rounding (exact in fp32), rounded to bf16 in turn
    const bf16x8 h = f.lh;
    f32x4 rlo, rhi;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        rlo[e] = lo[e] - (float)h[e];
        rhi[e] = hi[e] - (float)h[4 + e];
    }
    AFr<2> fl;
    acvt<2>(rlo, rhi, fl);
    f.ll = __builtin_bit_cast(bf16x8, fl.h);
    return f;
}
// the bias part alone (issued a phase earlier than the fragments, see the kernel)
// Two waves per pose (2-pose tiles): the wave's own TW column tiles (t0 = TW (wave & 1)) in b4[0..TW);
// graph_mma indexes b4 with compile-time tile numbers only (a runtime t0 + t index put the array in
// scratch memory)
__device__ __forceinline__ void gbias_load(GFrag& f, const float* __restrict__ bias, int lane, int wave) {
    constexpr int TW = NCD / (NW / P);
    if constexpr (TW < NCD) bias += 16 * TW * (wave & 1);
    const int g = lane >> 4, cl = lane & 15;
#pragma unroll
    for (int t = 0; t < NCD; ++t)
        f.b4[t] = t < TW ? *reinterpret_cast<const f32x4*>(bias + 16 * t + 4 * g) : f32x4{0.f, 0.f, 0.f, 0.f};
    f.b1[0] = TW == 6 ? bias[16 * g + cl] : 0.f;
    f.b1[1] = TW == 6 ? bias[16 * (4 + (g & 1)) + cl] : 0.f;
}

// GA = 2 (gemm mode 2): the 16 output joints' product as two v_mfma_f32_16x16x32_bf16 per column tile
// from bf16-rounded X and L_g's hi + lo pair (gfrag_load_h), fp32 accumulate; joint 16's row stays fp32.
template <bool RESID, int GA = 0, class Hook = NoHook>
__device__ __forceinline__ void graph_mma(const GFrag& f, const float* src, float* dst,
                                          const float* __restrict__ bias, int wave, int lane, const Hook& hook = Hook{}) {
    lane = opaque(lane);
    // 4-pose tiles: wave w = pose w, column tiles 0..5; 2-pose tiles: waves 2p, 2p+1 = pose p,
    // column tiles 0..2 and 3..5 (cheb_prep splits its columns the same way)
    constexpr int WPP = NW / P, TW = NCD / WPP;
    static_assert(TW == 6 || TW == 4 || TW == 3, "graph_mma: 3, 4 or 6 column tiles per wave");
    static_assert(GA == 0 || GA == 2, "fp32 or bf16 graph product");
    wave = opaque_s(wave);
    const int pose = WPP == 1 ? wave : wave / WPP;
    const int t0 = WPP == 1 ? 0 : (wave % WPP) * TW;
    if (pose >= P) return;
    const int g = lane >> 4, cl = lane & 15;
    const float(&lb)[5] = f.lb;
    const float(&l16)[5] = f.l16;
    const float* xp = src + pose * J * LDX + cl + 16 * t0;
    const int row_j = pose * J + cl, row16 = pose * J + 16;
    // joint 16's output row: 6 tiles: lane row g ends with column cl of tiles g and 4 + (g & 1)
    // (reduce-scatter below; rows 2, 3 hold a duplicate of the second and store nothing);
    // 3 tiles: lane row g < 3 ends with tile t0 + g (row 3 a duplicate)
    const int c16a = 16 * (t0 + (TW == 3 ? min(g, 2) : g)) + cl, c16b = 16 * (4 + (g & 1)) + cl;
    // RESID: the residual rows this lane updates, read before the MFMAs (dst != src)
    f32x4 old[TW];
    float old16a = 0.f, old16b = 0.f, b16a = 0.f;
    if constexpr (RESID) {
#pragma unroll
        for (int t = 0; t < TW; ++t) old[t] = *reinterpret_cast<const f32x4*>(dst + row_j * LDX + 16 * (t0 + t) + 4 * g);
        old16a = dst[row16 * LDX + c16a];
        if constexpr (TW == 6) old16b = dst[row16 * LDX + c16b];
        else b16a = bias[c16a];
    }
    f32x4 acc[TW];
    float p16[TW];
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    if constexpr (GA != 0) {
        // lane (g, cl): joints 4g..4g+3 (and 16 for g = 0) of column cl of each tile
        f32x4 xa[TW];
        float x16[TW];
#pragma unroll
        for (int t = 0; t < TW; ++t) {
#pragma unroll
            for (int e = 0; e < 4; ++e) xa[t][e] = xp[(4 * g + e) * LDX + 16 * t];
            x16[t] = xp[16 * LDX + 16 * t];
        }
#pragma unroll
        for (int t = 0; t < TW; ++t) {
            AFr<2> fx;
            acvt<2>(xa[t], f32x4{g == 0 ? x16[t] : 0.f, 0.f, 0.f, 0.f}, fx);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fx.h), f.lh, z, 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fx.h), f.ll, acc[t], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        hook();
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < TW; ++t) {
            float v = f.m16[4] * x16[t];
#pragma unroll
            for (int e = 0; e < 4; ++e) v = fmaf(f.m16[e], xa[t][e], v);
            p16[t] = v;
        }
    } else {
        float a[TW][5];
#pragma unroll
        for (int s = 0; s < 5; ++s) {
            const int row = min(4 * s + g, J - 1);
#pragma unroll
            for (int t = 0; t < TW; ++t) a[t][s] = xp[row * LDX + 16 * t];
        }
        // k-steps outer, tiles inner: consecutive MFMAs are independent (no 5-deep dependent chain
        // per tile); the first k-step starts from C = 0.  The MFMAs back to back, then joint 16's FMAs
        // as one VALU cluster (spread into the MFMA issue gaps each costs 12 cycles instead of 4,
        // tools/mfma_filler_probe.hip)
#pragma unroll
        for (int s = 0; s < 5; ++s)
#pragma unroll
            for (int t = 0; t < TW; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][s], lb[s], s == 0 ? z : acc[t], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        hook();
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 5; ++s)
#pragma unroll
            for (int t = 0; t < TW; ++t) p16[t] = s == 0 ? l16[0] * a[t][0] : fmaf(l16[s], a[t][s], p16[t]);
    }
#pragma unroll
    for (int t = 0; t < TW; ++t) {
        const int c0 = 16 * (t0 + t) + 4 * g;
        if constexpr (RESID) {
            *reinterpret_cast<f32x4*>(dst + row_j * LDX + c0) = old[t] + (acc[t] + f.b4[t]);
        } else {
            *reinterpret_cast<f32x4*>(dst + row_j * LDX + c0) = acc[t];
        }
    }
    // joint 16: the per-lane partial sums reduce-scattered over the 4 lane rows (rs4rows: lane
    // row g gets register g's total; same summation order as sum4rows), 6 permlanes for 6 tiles
    if constexpr (TW == 6) {
        const float va = rs4rows(p16[0], p16[1], p16[2], p16[3]);    // tile g
        const float vb = rs4rows(p16[4], p16[5], p16[4], p16[5]);    // tile 4 + (g & 1)
        if constexpr (RESID) {
            dst[row16 * LDX + c16a] = old16a + (va + f.b1[0]);
            if (g < 2) dst[row16 * LDX + c16b] = old16b + (vb + f.b1[1]);
        } else {
            dst[row16 * LDX + c16a] = va;
            if (g < 2) dst[row16 * LDX + c16b] = vb;
        }
    } else if constexpr (TW == 4) {
        const float va = rs4rows(p16[0], p16[1], p16[2], p16[3]);    // tile t0 + g
        if constexpr (RESID) dst[row16 * LDX + c16a] = old16a + (va + b16a);
        else dst[row16 * LDX + c16a] = va;
    } else {
        const float va = rs4rows(p16[0], p16[1], p16[2], p16[2]);    // tile t0 + g (g = 3: duplicate)
        if (g < 3) {
            if constexpr (RESID) dst[row16 * LDX + c16a] = old16a + (va + b16a);
            else dst[row16 * LDX + c16a] = va;
        }
    }
}

// ---------------------------------------------------------------------------------------
// gconv_input prologue: B1[:, 0:16] = [x | T1 x | T2 x | 0] for the 5 pose channels.
template <bool SPARSE>
__device__ __forceinline__ void input_prep(const float* __restrict__ cw, const float* xst, float* b1, int tid) {
    tid = opaque(tid);
    if (tid >= P * CIN) return;
    const int p = tid / CIN, c = tid - p * CIN;
    float v[J];
#pragma unroll
    for (int i = 0; i < J; ++i) v[i] = xst[(p * J + i) * CIN + c];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        float a1 = 0.f, a2 = 0.f;
        if constexpr (SPARSE) {
#pragma unroll
            for (int k = 0; k < SPAT.n1[j]; ++k) a1 = fmaf(cw[SPAT.o1[j] + k], v[SPAT.c1[j][k]], a1);
#pragma unroll
            for (int k = 0; k < SPAT.n2[j]; ++k) a2 = fmaf(cw[SPAT.nnz1 + SPAT.o2[j] + k], v[SPAT.c2[j][k]], a2);
        } else {
#pragma unroll
            for (int i = 0; i < J; ++i) {
                a1 = fmaf(cw[j * J + i], v[i], a1);
                a2 = fmaf(cw[J * J + j * J + i], v[i], a2);
            }
        }
        float* rowp = b1 + (p * J + j) * LDX;
        rowp[c] = v[j];
        rowp[CIN + c] = a1;
        rowp[2 * CIN + c] = a2;
        if (c == 0) rowp[3 * CIN] = 0.f;
    }
}

// ---------------------------------------------------------------------------------------
__device__ __forceinline__ float swishf(float x) { return x * (1.0f / (1.0f + expf(-x))); }
// Timestep MLP (gcndiff.py:15-33, :103-106) and per-layer temb_proj(swish(.)) (:46, :51):
// tproj[slot][l][:] for slot t-values (one per DDIM step, or one per pose in eps mode).
// Batch-invariant in the sampler: all rows of a step share t, so it is computed once per step.

__global__ void __launch_bounds__(256) temb_kernel(const float* __restrict__ tw, const float* __restrict__ tvals,
                                                   int tstride, float* __restrict__ tproj) {
    __shared__ float emb[D];
    __shared__ float h0[E];
    __shared__ float h1[E];
    const int tid = threadIdx.x;
    const float t = tvals[(size_t)blockIdx.x * tstride];
    const float neg_scale = -(float)(9.210340371976184 / (double)(D / 2 - 1));   // -(log(10000)/(half-1)), fp32 scalar
    if (tid < D) {
        const int k = tid < D / 2 ? tid : tid - D / 2;
        const float f = expf((float)k * neg_scale);
        const float arg = t * f;
        emb[tid] = tid < D / 2 ? sinf(arg) : cosf(arg);
    }
    __syncthreads();
    for (int o = tid; o < E; o += 256) {
        float acc = 0.f;
        for (int k = 0; k < D; ++k) acc = fmaf(emb[k], tw[TOFF_W0 + k * E + o], acc);
        h0[o] = swishf(acc + tw[TOFF_B0 + o]);
    }
    __syncthreads();
    for (int o = tid; o < E; o += 256) {
        float acc = 0.f;
        for (int k = 0; k < E; ++k) acc = fmaf(h0[k], tw[TOFF_W1 + k * E + o], acc);
        h1[o] = swishf(acc + tw[TOFF_B1 + o]);     // swish(temb) as consumed by every temb_proj
    }
    __syncthreads();
    for (int o = tid; o < NL * D; o += 256) {
        const int l = o / D, c = o - l * D;
        const float* wp = tw + TOFF_WP + (size_t)l * E * D;
        float acc = 0.f;
        for (int k = 0; k < E; ++k) acc = fmaf(h1[k], wp[k * D + c], acc);
        tproj[(size_t)blockIdx.x * NL * D + o] = acc + tw[TOFF_BP + o];
    }
}

// ---------------------------------------------------------------------------------------
// Step-split tiles (SampleArgs.split_n).  Tile j's handoff word flags[j] holds (token << 2) | state
// during a launch and 0 between launches:
//   RUN      the first half has claimed the tile (it claims before its first step);
//   PUB      the first half has stored x_t at step split_k to x_out and released it (agent scope);
//   ABANDON  the second half found the first half not yet started and took the whole tile itself.
// The second half takes PUB (and resets the word), waits without bound while it reads RUN (a running
// workgroup always finishes: first halves wait for nothing), and otherwise, after a short idle wait,
// swaps in ABANDON and runs all K steps from x_in.  A first half that then starts finds ABANDON,
// resets the word and leaves without writing anything.  Every path leaves the word 0 at the end of
// the launch, so a captured launch (a fixed token) replays cleanly, and no dispatch order is assumed:
// with the dispatcher's in-order start the first halves are long running when their second halves
// arrive, and the fallback only costs time if that ever fails.
constexpr unsigned SPL_RUN = 1u, SPL_PUB = 2u, SPL_ABANDON = 3u;
constexpr int SPL_IDLE_POLLS = 4096;    // ~7 ms of s_sleep(64) before a second half gives up waiting

// first half, before its first step: claim the tile; false = its second half already took it
__device__ __forceinline__ bool split_claim(const SampleArgs& a, int j, int tid) {
    __shared__ int ok;
    if (tid == 0) {
        if (a.split_dbg == 1)      // test hook (dpk_debug_split): start ~100 ms late
            for (int it = 0; it < 30000; ++it) __builtin_amdgcn_s_sleep(127);
        const unsigned run = (a.token << 2) | SPL_RUN, ab = (a.token << 2) | SPL_ABANDON;
        int res = -1;
        while (res < 0) {
            unsigned v = __hip_atomic_load(a.flags + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (v == ab) {
                __hip_atomic_store(a.flags + j, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                res = 0;
            } else if (__hip_atomic_compare_exchange_strong(a.flags + j, &v, run, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                            __HIP_MEMORY_SCOPE_AGENT)) {
                res = 1;
            }
        }
        ok = res;
    }
    __syncthreads();
    return ok != 0;
}
__device__ __forceinline__ void split_publish(const SampleArgs& a, int j, int tid) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");   // this thread's x_out stores, device-visible
    __syncthreads();
    if (tid == 0)
        __hip_atomic_store(a.flags + j, (a.token << 2) | SPL_PUB, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
// second half: true = x_t is in x_out; false = run steps [0, K) from x_in (the first half will not)
__device__ __forceinline__ bool split_wait(const SampleArgs& a, int j, int tid) {
    __shared__ int ok;
    if (tid == 0) {
        const unsigned run = (a.token << 2) | SPL_RUN, pub = (a.token << 2) | SPL_PUB;
        const unsigned ab = (a.token << 2) | SPL_ABANDON;
        int idle = a.split_dbg ? 0 : SPL_IDLE_POLLS;
        int res = -1;
        while (res < 0) {
            unsigned v = __hip_atomic_load(a.flags + j, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            if (v == pub) {
                __hip_atomic_store(a.flags + j, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                res = 1;
            } else if (v == run || idle > 0) {
                if (v != run) --idle;
                __builtin_amdgcn_s_sleep(64);
            } else if (__hip_atomic_compare_exchange_strong(a.flags + j, &v, ab, __ATOMIC_ACQUIRE, __ATOMIC_RELAXED,
                                                            __HIP_MEMORY_SCOPE_AGENT)) {
                if (a.split_stats) __hip_atomic_fetch_add(a.split_stats, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                res = 0;
            }
        }
        ok = res;
    }
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");    // every thread reads x_out after the acquire
    return ok != 0;
}

// ---------------------------------------------------------------------------------------
// The sampler: K DDIM steps (or one eps evaluation, or one GCNpose forward) for P poses
// per workgroup.
template <int MODE, bool SPARSE, int G16, int ZM = 0, bool START = false, bool PAD = false>
// ZM, the z of the DDIM update (sample mode): 0 counter-based draws when eta != 0, else 0; 1 the caller's
// buffer (dpk_sample_noise).  Separate instantiations: the buffer read is not in the usual launch.
// START (sample mode): the hypothesis start of dpk_sample_start in the tile's load of x_in.  A template flag and not
// a launch-uniform branch on SampleArgs.start_on: the branch is a dozen instructions ahead of the step loop, yet with
// it in the one kernel f16x3 measured 0.48 % slower than the parent build in 9 of 9 alternating pairs (fp32 equal,
// bf16 K=100 0.41 % faster: code placement, profiles/hypothesis_start_ab.txt); START = false compiles the parent's kernel.
// PAD (sample and eps modes, dense graph, fp32 and f16x3): a handle of a.n_pts = 2..16 joints on this tile.  LDS row
// p*17 + j holds joint j of the tile's pose p when j < a.n_pts and is dead otherwise: global element
// ((pose0 + p) * n_pts + j) * 5 + c for every load and store, the caller's draws and the counter-based ones alike;
// the dead rows of the pose state are written as 0 at every step, and attention excludes the dead keys
// (attention_mma PADK).  The packed graph terms are zero-embedded (dpk_pack.inc), so no live row reads a dead one.
// A template flag for START's reason: PAD = false compiles the 17-joint kernels as they were.
// `arena` is a separate restrict kernel argument: the compiler can then prove the weight arena
// is never written during the launch and turns its wave-uniform loads (Laplacians, Chebyshev
// terms, LayerNorm gains, biases) into scalar s_load (in the SampleArgs struct it cannot, and
// every such value became a vector load with its L2 latency exposed).
// G16: GEMMs on the split-fp16 path (gemm mode 1) with weights from `arena16`.
__global__ void __launch_bounds__(NT, 1) sample_kernel(SampleArgs a, const float* __restrict__ arena,
                                                               const char* __restrict__ arena16) {
    constexpr bool EPS_MODE = MODE == M_EPS;
    constexpr bool POSE = MODE == M_POSE;
    static_assert(!PAD || (PADDED && !SPARSE && !POSE && G16 != 2), "padded tiles: GCNdiff, dense graph, fp32 or f16x3");
    __shared__ __attribute__((aligned(16))) float sm[SM_FLOATS];
    float* XS = sm + SM_XS;
    float* B1 = sm + SM_B1;
    float* B2 = sm + SM_B2;
    float* XST = sm + SM_XST;
    float* LNP = sm + SM_LNP;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform (SGPR)
    // which tile and which steps this workgroup runs (SampleArgs: step-split last round)
    int tile = blockIdx.x, s_beg = 0, s_end = MODE == M_SAMPLE ? a.K : 1, half = 0;
    if constexpr (MODE == M_SAMPLE) {
        if (a.split_n) {
            const int b = blockIdx.x, n = a.split_n;
            if (b < n) {
                tile = a.split_full + b;
                s_end = a.split_k;
                half = 1;
            } else if (b < n + a.split_full) {
                tile = b - n;
            } else {
                tile = a.split_full + (b - n - a.split_full);
                s_beg = a.split_k;
                half = 2;
            }
        }
    }
    const int pose0 = a.pose_off + tile * P;
    const int npose = min(P, a.N - pose0);
    const int nvalid = npose * PE;
    // PAD: joints and floats per pose in global memory; element i = (p*17 + j)*5 + c of the tile's pose state is
    // live when p < npose and j < nj, and then global element gmap(i) of the [N][nj][5] arrays
    const int nj = PAD ? a.n_pts : J, pe = PAD ? a.n_pts * CIN : PE;
    auto live = [&](int i) { return i < nvalid && i % PE < pe; };
    auto gmap = [&](int i) { return (size_t)(pose0 + i / PE) * pe + i % PE; };
    const float* W = arena;
    // the Chebyshev constants of input_prep / cheb_prep: the packed H36M-sparse values (uniform scalar
    // loads), or the dense T1 | T2 from their LDS copy (staged below for the output phase): as scalar
    // loads, their 578 loop-invariant values were hoisted into SGPRs and spilled (1.3k SGPR spills at hid 64)
    const float* CW = SPARSE ? W + OFF_CHEBS : sm + SM_TC;
    // key mask of the pose this wave's attention handles (attention_mma: wave / (NW/P)): per pose from
    // dpk_set_pose_masks, else the handle's one
    unsigned kmask = a.mask;
    if (a.pmask) kmask = a.pmask[min(pose0 + wave / (NW / P), a.N - 1)];
    if constexpr (PAD) kmask &= (1u << nj) - 1u;

    if constexpr (POSE) {
        // uv into channels 0-1 of the 5-channel tile; the packed input weight is zero for 2-4
        for (int i = tid; i < R * CIN; i += NT) {
            const int row = i / CIN, c = i - row * CIN;
            XST[i] = (c < CIN_POSE && row < npose * J) ? a.x_in[((size_t)pose0 * J + row) * CIN_POSE + c] : 0.f;
        }
    } else {
        const float* src = a.x_in;
        bool start = false;   // block-uniform: this load is of x_in and the hypothesis start is on
        if constexpr (MODE == M_SAMPLE) {
            if (half == 1 && !split_claim(a, tile - a.split_full, tid)) return;   // the second half took it
            start = START;
            if (half == 2) {
                // second half of a step-split tile: x_t at step split_k from the first half (the start is
                // in it already), or (it never started) the whole tile from x_in
                if (split_wait(a, tile - a.split_full, tid)) {
                    src = a.x_out;
                    start = false;
                } else {
                    s_beg = 0;
                }
            }
        }
        bool noised = false;   // block-uniform: this load gave x_t of the denoising loss (eps mode, dpk_diff_loss)
        if constexpr (EPS_MODE) {
            if (a.loss_t) {
                // x_t of the tile's live rows at each pose's own timestep: row clamp(t) of the schedule's roots (a
                // NaN compares false both times and reads row 0); the PAD and the 17-joint forms of START's load
                for (int i = tid; i < R * CIN; i += NT) {
                    float v = 0.f;
                    if (PAD ? live(i) : i < nvalid) {
                        const int p = i / PE, pose = pose0 + p;
                        const size_t g = PAD ? gmap(i) : (size_t)pose0 * PE + i;
                        const float tf = a.loss_t[pose];
                        const int ti = tf >= 0.f ? (tf < (float)(a.loss_nt - 1) ? (int)tf : a.loss_nt - 1) : 0;
                        v = qsample_at(a.x_in[g], pose, i - p * PE, pe, a.loss_qtab[2 * ti], a.loss_qtab[2 * ti + 1],
                                       a.start_scale, a.start_scale_rows, a.start_noise, a.seed);
                        if (a.loss_xt) a.loss_xt[g] = v;
                    }
                    XST[i] = v;
                }
                noised = true;
            }
        }
        if (noised) {
        } else if (PAD && START && start) {
            for (int i = tid; i < R * CIN; i += NT) {
                float v = 0.f;
                if (live(i)) {
                    const size_t g = gmap(i);
                    v = qsample_at(a.x_in[g], pose0 + i / PE, i % PE, pe, a.start_sa, a.start_sb, a.start_scale,
                                   a.start_scale_rows, a.start_noise, a.seed);
                    if (a.xs) a.xs[g] = v;
                }
                XST[i] = v;
            }
        } else if constexpr (PAD) {
            for (int i = tid; i < R * CIN; i += NT) XST[i] = live(i) ? src[gmap(i)] : 0.f;
        } else if (START && start) {
            // x_T of the tile's valid rows (padded rows stay 0); it is xs[0] of the trajectory
            for (int i = tid; i < R * CIN; i += NT) {
                float v = 0.f;
                if (i < nvalid) {
                    const int p = i / PE;
                    const size_t g = (size_t)pose0 * PE + i;
                    v = qsample_at(a.x_in[g], pose0 + p, i - p * PE, PE, a.start_sa, a.start_sb, a.start_scale,
                                   a.start_scale_rows, a.start_noise, a.seed);
                    if (a.xs) a.xs[g] = v;
                }
                XST[i] = v;
            }
        } else {
            for (int i = tid; i < R * CIN; i += NT) XST[i] = i < nvalid ? src[(size_t)pose0 * PE + i] : 0.f;
        }
    }
    // LayerNorm parameters of every layer, staged once per launch (the per-lane column slices
    // are not wave-uniform, and as global loads their L2 latency sat on the LN critical path)
    static_assert(OFF_LN0B == OFF_LN0A + D && OFF_LN1A == OFF_LN0A + 2 * D && OFF_LN1B == OFF_LN0A + 3 * D, "LN block");
    for (int i = tid; i < NL * 4 * D; i += NT) LNP[i] = W[(i / (4 * D)) * LAYER_FLOATS + OFF_LN0A + i % (4 * D)];
    for (int i = tid; i < 2 * J * J; i += NT) sm[SM_TC + i] = W[OFF_CHEB + i];
    if constexpr (SPARSE)
        for (int i = tid; i < CHEBT_FLOATS; i += NT)
            reinterpret_cast<int*>(sm)[SM_TS + i] = reinterpret_cast<const int*>(W)[OFF_CHEBT + i];
    __syncthreads();

#if DPK_TRACE
    if ((tid & 63) == 0) {
        ::dpk::tr_row[wave] = nullptr;
        ::dpk::tr_ix[wave] = 0;
    }
#define DPK_STAMP()                                                                                       \
    do {                                                                                                  \
        if ((tid & 63) == 0)                                                                              \
            ::dpk::tr_row[wave] = (a.trace && s == a.trace_step)                                                 \
                               ? a.trace + ((size_t)blockIdx.x * NW + wave) * TRACE_SLOTS                 \
                               : nullptr;                                                                 \
        ::dpk::tr_stamp();                                                                                       \
    } while (0)
#define BAR()          \
    do {               \
        DPK_STAMP();   \
        __syncthreads(); \
        DPK_STAMP();   \
    } while (0)
#else
#define BAR() __syncthreads()
#endif
    // two waves per SIMD: the second (waves 4..7) at a higher static priority, so the pair does not issue
    // in lockstep and one's MFMAs cover the other's waits
    if constexpr (NSUB == 2)
        if (wave >= 4) __builtin_amdgcn_s_setprio(1);
#pragma unroll 1
    for (int s = s_beg; s < s_end; ++s) {
        // ---- gconv_input: ChebConv 5->96 (gcndiff.py:108)
        {
            const BPre<sub_max(NCD / 2)> pre = gemm_prefetch<NCD, 1>(W + OFF_WIN, wave, lane);
            input_prep<SPARSE>(CW, XST, B1, tid);
            BAR();
            const EpiArgs e{XS, LDX, W + OFF_BIN, nullptr, 0, pose0, a.N - 1};
            gemm_wg<NCD, 1, E_STORE>(B1, LDX, W + OFF_WIN, wave, lane, e, pre);
        }
        BAR();

#pragma unroll 1
        for (int l = 0; l < a.num_layers; ++l) {
            const float* LW = W + l * LAYER_FLOATS;
            // half-width-operand GEMM weights of this layer (gemm modes 1, 2; offh); block set X at O16_X / GH
            constexpr int GH = G16 ? G16 : 1;              // (instantiations with G16 = 0 never read LH)
            const char* LH = arena16 + offh<GH>(l, 0);
            // column tiles per pass of the half-width GEMMs (HPW; f16x3: registers)
            constexpr int PWQ = G16 == 2 ? 9 : (NSUB == 2 ? DPK_PWQ16_W8 : HPW<SPARSE>::QKV);
            constexpr int PWF = G16 == 2 ? 6 : (NSUB == 2 ? DPK_PWF16_W8 : HPW<SPARSE>::FC1);
            constexpr int GG = G16 == 2 ? 2 : 0;           // attention's and the graph products' arithmetic
            // ---- x = x + MHA(LN0(x))   (GraAttenLayer, GraFormer.py:94-95)
            {
                // LN0's gain/shift live in the QKV weights and bias (c = b_LN0 W + b_qkv, dpk_load_weights)
                const EpiArgs e{B2, LD2, LW + OFF_CQKV, nullptr, 0, pose0, a.N - 1};
                using HQ = HGemm<GH, 3 * NCD, KB32_D, PWQ>;
                BPre<sub_max(3 * NCD / 2)> pre;
                typename HQ::Pre preh;
                if constexpr (G16 == 0 && !DPK_LATE(1)) pre = gemm_prefetch<3 * NCD, KB_D, DPK_QKV_NPRE>(LW + OFF_QKV, wave, lane);
                if (DPK_RUN(8)) layer_norm<false, false>(XS, B1, LNP + l * 4 * D, LNP + l * 4 * D + D, tid);
                if constexpr (G16) {
                    __builtin_amdgcn_sched_barrier(0);
                    preh = HQ::prefetch(LH + O16_QKV / GH, wave, lane);
                } else if constexpr (DPK_LATE(1)) {
                    __builtin_amdgcn_sched_barrier(0);
                    pre = gemm_prefetch<3 * NCD, KB_D, DPK_QKV_NPRE>(LW + OFF_QKV, wave, lane);
                }
                BAR();
                if (DPK_RUN(16 | 32)) {
                    if constexpr (G16) HQ::template run<E_STORE>(B1, LDX, LH + O16_QKV / GH, wave, lane, e, preh);
                    else gemm_wg<3 * NCD, KB_D, E_STORE, false, DPK_QKV_NPRE>(B1, LDX, LW + OFF_QKV, wave, lane, e, pre);
                }
            }
            BAR();
            {
                const EpiArgs e{XS, LDX, LW + OFF_BO, nullptr, 0, pose0, a.N - 1};
                using HO = HGemm<GH, NCD, KB32_D, HPW<SPARSE>::O>;
                BPre<sub_max(NCD / 2)> pre;
                typename HO::Pre preh;
                auto o_pre = [&]() {
                    if constexpr (G16) preh = HO::prefetch(LH + O16_O / GH, wave, lane);
                    else pre = gemm_prefetch<NCD, KB_D>(LW + OFF_O, wave, lane);
                };
                if constexpr (!DPK_LATE(2) && !DPK_MID(2)) o_pre();
                if (DPK_RUN(1)) {
                    if constexpr (DPK_MID(2)) attention_mma<GG, PAD>(B2, B1, kmask, wave, lane, o_pre, nj);
                    else attention_mma<GG, PAD>(B2, B1, kmask, wave, lane, NoHook{}, nj);
                }
                if constexpr (DPK_LATE(2)) {
                    __builtin_amdgcn_sched_barrier(0);
                    o_pre();
                }
                BAR();
                if (DPK_RUN(16 | 64)) {
                    if constexpr (G16) HO::template run<E_RESID>(B1, LDX, LH + O16_O / GH, wave, lane, e, preh);
                    else gemm_wg<NCD, KB_D, E_RESID>(B1, LDX, LW + OFF_O, wave, lane, e, pre);
                }
            }
            BAR();
            // ---- x = x + GraphNet(LN1(x)) = x + L (relu((L LN1(x)) W1^T + b1) W2^T) + b2
            //      (GraFormer.py:189-201; fc2's product with L applied after the GEMM)
            GFrag gb;   // graph2's fc2 bias: issued here, beside fc1's first B blocks
            gbias_load(gb, LW + OFF_BFC2, lane, wave);
            {
                using HF = HGemm<GH, 2 * NCD, KB32_D, PWF>;
                BPre<sub_max(NCD)> pre;
                typename HF::Pre preh;
                auto f_pre = [&]() {
                    if constexpr (G16) preh = HF::prefetch(LH + O16_FC1 / GH, wave, lane);
                    else pre = gemm_prefetch<2 * NCD, KB_D, DPK_FC1_NPRE>(LW + OFF_FC1, wave, lane);
                };
                // one wave per pose: LN1's rows of pose w are read back by the same wave's graph1, no barrier
                constexpr bool LN1_OWN = R == 68 && NW == P;
                constexpr bool FC1_MID = DPK_MID(4) && LN1_OWN;   // graph1 right after LN1
                if constexpr (!DPK_LATE(4) && !FC1_MID) f_pre();
                const GFrag gf = GG != 0 ? gfrag_load_h(LW + OFF_LG, lane) : gfrag_load(LW + OFF_LGF, lane);
                if constexpr (LN1_OWN) {
                    // LN1 rows of pose w by wave w, read back by the same wave's graph1: no barrier
                    // (LDS operations of one wave complete in order; the asm keeps the compiler's order)
                    if (DPK_RUN(8)) layer_norm<true>(XS, B1, LNP + l * 4 * D + 2 * D, LNP + l * 4 * D + 3 * D, tid);
                    asm volatile("" ::: "memory");
                    if constexpr (FC1_MID) {
                        if (DPK_RUN(2)) graph_mma<false, GG>(gf, B1, B1, nullptr, wave, lane, f_pre);
                    } else if (DPK_RUN(2)) graph_mma<false, GG>(gf, B1, B1, nullptr, wave, lane);
                } else {
                    // (8 waves: the pose-mapped rows on waves 0..3, so every row is normalised by the lanes that
                    // normalise it on 4 waves, bitwise; graph1's two waves per pose wait at the barrier)
                    if (DPK_RUN(8)) layer_norm<R == 68>(XS, B1, LNP + l * 4 * D + 2 * D, LNP + l * 4 * D + 3 * D, tid);
                    BAR();
                    if (DPK_RUN(2)) graph_mma<false, GG>(gf, B1, B1, nullptr, wave, lane);
                }
                if constexpr (DPK_LATE(4) && !FC1_MID) {
                    __builtin_amdgcn_sched_barrier(0);
                    f_pre();
                }
                BAR();
                if (DPK_RUN(16 | 128)) {
                    const EpiArgs e{B2, LD2, LW + OFF_BFC1, nullptr, 0, pose0, a.N - 1};
                    if constexpr (G16) HF::template run<E_STORE_RELU>(B1, LDX, LH + O16_FC1 / GH, wave, lane, e, preh);
                    else gemm_wg<2 * NCD, KB_D, E_STORE_RELU, false, DPK_FC1_NPRE>(B1, LDX, LW + OFF_FC1, wave, lane, e, pre);
                }
            }
            GFrag gf2 = GG != 0 ? gfrag_load_h(LW + OFF_LG, lane) : gfrag_load(LW + OFF_LGF, lane);   // graph2's operands, a GEMM ahead
#pragma unroll
            for (int t = 0; t < NCD; ++t) gf2.b4[t] = gb.b4[t];
            gf2.b1[0] = gb.b1[0];
            gf2.b1[1] = gb.b1[1];
            {
                const EpiArgs e{B1, LDX, nullptr, nullptr, 0, pose0, a.N - 1};
                if constexpr (G16) {
                    using H2 = HGemm<GH, NCD, KB32_D2, HPW<SPARSE>::FC2>;
                    const typename H2::Pre pre = H2::prefetch(LH + O16_FC2 / GH, wave, lane);
                    BAR();
                    if (DPK_RUN(16 | 256)) H2::template run<E_STORE_NB>(B2, LD2, LH + O16_FC2 / GH, wave, lane, e, pre);
                } else {
                    const BPre<sub_max(NCD / 2)> pre = gemm_prefetch<NCD, KB_D2>(LW + OFF_FC2, wave, lane);
                    BAR();
                    if (DPK_RUN(16 | 256)) gemm_wg<NCD, KB_D2, E_STORE_NB>(B2, LD2, LW + OFF_FC2, wave, lane, e, pre);
                }
            }
            {
                const float* tp = a.tproj + (MODE == M_SAMPLE ? (size_t)s * NL * D : 0) + l * D;
                const EpiArgs e{B1, LDX, LW + OFF_BC1, tp, EPS_MODE ? NL * D : 0, pose0, a.N - 1};
                using HC = HGemm<GH, NCD, KB32_D3, HPW<SPARSE>::CHEB>;
                BPre<sub_max(NCD / 2)> pre;
                typename HC::Pre preh;
                auto c1_pre = [&]() {
                    if constexpr (G16) preh = HC::prefetch(LH + O16_C1 / GH, wave, lane);
                    else pre = gemm_prefetch<NCD, KB_D3>(LW + OFF_C1, wave, lane);
                };
                if constexpr (!DPK_LATE(8) && !DPK_MID(8)) c1_pre();
                BAR();
                // ---- _ResChebGC_diff (gcndiff.py:47-53): x + relu(Cheb2(relu(Cheb1(x)) + temb_proj));
                //      cheb_prep reads only its own wave's rows of XS (wave = pose): no barrier
                if constexpr (DPK_MID(8)) {
                    if (DPK_RUN(2)) graph_mma<true, GG>(gf2, B1, XS, LW + OFF_BFC2, wave, lane, c1_pre);
                } else if (DPK_RUN(2)) graph_mma<true, GG>(gf2, B1, XS, LW + OFF_BFC2, wave, lane);
                if (DPK_RUN(4)) cheb_prep<SPARSE, true>(CW, XS, B2, wave, lane);
                if constexpr (DPK_LATE(8)) {
                    __builtin_amdgcn_sched_barrier(0);
                    c1_pre();
                }
                BAR();
                if (DPK_RUN(16 | 512)) {
                    if constexpr (G16) HC::template run<E_CHEB1, true>(B2, LD2, LH + O16_C1 / GH, wave, lane, e, preh, XS, LDX);
                    else gemm_wg<NCD, KB_D3, E_CHEB1, true>(B2, LD2, LW + OFF_C1, wave, lane, e, pre, XS, LDX);
                }
            }
            {
                const EpiArgs e{XS, LDX, LW + OFF_BC2, nullptr, 0, pose0, a.N - 1};
                using HC = HGemm<GH, NCD, KB32_D3, HPW<SPARSE>::CHEB>;
                BPre<sub_max(NCD / 2)> pre;
                typename HC::Pre preh;
                auto c2_pre = [&]() {
                    if constexpr (G16) preh = HC::prefetch(LH + O16_C2 / GH, wave, lane);
                    else pre = gemm_prefetch<NCD, KB_D3>(LW + OFF_C2, wave, lane);
                };
                if constexpr (!DPK_LATE(16)) c2_pre();
                BAR();
                if (DPK_RUN(4)) cheb_prep<SPARSE, true>(CW, B1, B2, wave, lane);
                if constexpr (DPK_LATE(16)) {
                    __builtin_amdgcn_sched_barrier(0);
                    c2_pre();
                }
                BAR();
                if (DPK_RUN(16 | 1024)) {
                    if constexpr (G16) HC::template run<E_RESID_RELU, true>(B2, LD2, LH + O16_C2 / GH, wave, lane, e, preh, B1, LDX);
                    else gemm_wg<NCD, KB_D3, E_RESID_RELU, true>(B2, LD2, LW + OFF_C2, wave, lane, e, pre, B1, LDX);
                }
            }
            BAR();
        }
        // ---- gconv_output: ChebConv 96->5 (gcndiff.py:112), then the DDIM update
        //      (pose: ChebConv 96->3, gcnpose.py:112, kept in B1 for the uvxyz assembly).
        //      sum_k T_k x W_k computed as sum_k T_k (x W_k): one K=96 GEMM Y = x [W0 | W1 | W2]
        //      (3*cout columns, one tile) into B2, then the 17x17 products on the 3*cout columns.
        constexpr int COUTK = POSE ? COUT_POSE : COUT;
        constexpr int NOUT = P * J * COUTK, NIT = (NOUT + NT - 1) / NT;
        const BPre<1> preo = out_prefetch<KB_D>(W + OFF_WOUT, lane);
        float bo[NIT];                                  // output bias of this thread's outputs, a GEMM ahead
#pragma unroll
        for (int k = 0; k < NIT; ++k) bo[k] = W[OFF_BOUT + (tid + k * NT) % COUTK];
        if (wave < R / 16)
            gemm_out<KB_D, 3 * COUTK>(XS, LDX, W + OFF_WOUT, wave, lane,
                                      [&](int r, int c, float v) { B2[r * LD2 + c] = v; }, preo);
        BAR();
        {
            float cf[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
            if constexpr (MODE == M_SAMPLE) {
                const float* cfp = a.coef + s * 6;
#pragma unroll
                for (int i = 0; i < 5; ++i) cf[i] = cfp[i];                  // uniform: SGPRs
            }
            const float* T1d = sm + SM_TC;
            const float* T2d = T1d + J * J;
            // per-step thread index: the addresses below are recomputed per step instead of being
            // hoisted out of the step loop (held across every layer, they take registers)
            const int tid_o = opaque(tid);
#pragma unroll
            for (int k = 0; k < NIT; ++k) {
                const int idx = tid_o + k * NT;
                if (idx >= NOUT) break;
                const int p = idx / (J * COUTK), rem = idx - p * (J * COUTK);
                const int j = rem / COUTK, c = rem - j * COUTK;
                const float* yp = B2 + p * J * LD2;
                float a1 = 0.f, a2 = 0.f;
                if constexpr (SPARSE) {
                    // row j's nonzeros in ascending column order, then (0, j) padding: the dense loop's fma
                    // chain minus its exact zero products, so the sums are bitwise the same.  The entries
                    // are read as integers: the row offsets (small integers) as float bits are denormals,
                    // which a float-typed path does not carry through intact (measured: wrong results)
                    typedef int i32x2 __attribute__((ext_vector_type(2)));
                    const i32x2* ts = reinterpret_cast<const i32x2*>(sm + SM_TS) + j * (SPT1 + SPT2);
#pragma unroll
                    for (int q = 0; q < SPT1; ++q) {
                        const i32x2 e = ts[q];
                        a1 = fmaf(__builtin_bit_cast(float, e[0]), yp[e[1] + COUTK + c], a1);
                    }
#pragma unroll
                    for (int q = 0; q < SPT2; ++q) {
                        const i32x2 e = ts[SPT1 + q];
                        a2 = fmaf(__builtin_bit_cast(float, e[0]), yp[e[1] + 2 * COUTK + c], a2);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < J; ++i) {
                        a1 = fmaf(T1d[j * J + i], yp[i * LD2 + COUTK + c], a1);
                        a2 = fmaf(T2d[j * J + i], yp[i * LD2 + 2 * COUTK + c], a2);
                    }
                }
                const float et = ((yp[j * LD2 + c] + a1) + a2) + bo[k];
                const int r = p * J + j;
                const int oidx = r * CIN + c;          // same as r*COUT+c (coords 5 -> 5)
                const bool valid = PAD ? live(oidx) : oidx < nvalid;
                const size_t gidx = PAD ? gmap(oidx) : (size_t)pose0 * PE + oidx;
                if (POSE) {
                    B1[r * LDX + c] = et;
                } else if (EPS_MODE) {
                    if (valid && a.x_out) a.x_out[gidx] = et;
                    if (a.loss_out) {
                        // fl(d * d), d = target - eps, staged in B1 (free in eps mode) at the pose state's index;
                        // target = e * scale from the arrays x_t was noised with: the same product
                        float dd = 0.f;
                        if (valid) {
                            const float e = a.start_noise ? a.start_noise[gidx] : normal_noise(a.seed, -1, (long long)gidx);
                            const float sc = a.start_scale ? a.start_scale[(size_t)((pose0 + p) % a.start_scale_rows) * pe + (oidx - p * PE)] : 1.0f;
                            const float d = e * sc - et;
                            dd = d * d;
                        }
                        B1[oidx] = dd;
                    }
                } else {
                    // c1 * z: the caller's per-step draws (the reference's randn_like, utils_diff.py:65)
                    // or counter-based noise
                    float z = 0.f;
                    if constexpr (ZM == 1) z = valid ? a.noise[(size_t)s * a.N * pe + gidx] : 0.f;
                    else z = a.eta != 0.f ? normal_noise(a.seed, s, (long long)gidx) : 0.f;
                    float x0, xn;
                    ddim_elem(cf, XST[oidx], et, z, x0, xn);
                    XST[oidx] = (PAD && !valid) ? 0.f : xn;
                    if (valid) {
                        if (a.x0s) a.x0s[(size_t)s * a.N * pe + gidx] = x0;
                        if (a.xs) a.xs[(size_t)(s + 1) * a.N * pe + gidx] = xn;
                    }
                }
            }
        }
        BAR();
    }
    if constexpr (MODE == M_SAMPLE) {
        if constexpr (PAD) {
            for (int i = tid; i < nvalid; i += NT)
                if (live(i)) a.x_out[gmap(i)] = XST[i];
        } else {
            for (int i = tid; i < nvalid; i += NT) a.x_out[(size_t)pose0 * PE + i] = XST[i];
        }
        if (half == 1) split_publish(a, tile - a.split_full, tid);
    } else if constexpr (POSE) {
        // inputs_xyz = model_pose(input_2d); inputs_xyz -= root; input_uvxyz = cat(uv, xyz).repeat(H)
        // (runners/diffpose_frame.py:337-342).  root_mode 0 = what the reference's aliased in-place
        // `x[:, :, :] -= x[:, :1, :]` yields on CPU torch (only the root row is zeroed).
        if (a.x_out)
            for (int i = tid; i < npose * J * COUT_POSE; i += NT) {
                const int row = i / COUT_POSE, c = i - row * COUT_POSE;
                a.x_out[(size_t)pose0 * J * COUT_POSE + i] = B1[row * LDX + c];
            }
        if (a.uvxyz)
            for (int i = tid; i < npose * PE; i += NT) {
                const int row = i / CIN, c = i - row * CIN;
                float v;
                if (c < CIN_POSE) {
                    v = XST[i];
                } else {
                    const float raw = B1[row * LDX + (c - CIN_POSE)];
                    const int j = row % J;
                    if (a.root_mode == 0) v = j == 0 ? 0.f : raw;
                    else if (a.root_mode == 1) v = raw - B1[(row - j) * LDX + (c - CIN_POSE)];
                    else v = raw;
                }
                for (int hh = 0; hh < a.H; ++hh) a.uvxyz[((size_t)hh * a.N + pose0) * PE + i] = v;
            }
    } else {
        // the denoising loss (after the epilogue's barrier): one lane per valid pose adds its n_pts * 5 staged
        // squares in ascending element order into one accumulator
        if (a.loss_out && tid < npose) {
            const float* sq = B1 + tid * PE;
            float acc = 0.f;
            for (int i = 0; i < pe; ++i) acc = acc + sq[i];
            a.loss_out[pose0 + tid] = acc;
        }
    }
}

#undef BAR
#undef DPK_STAMP
