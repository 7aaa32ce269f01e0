// The persistent sampler's host side for one instance: included by dpk_kernels.hip inside every instance
// namespace right after dpk_sampler.inc (dpk / dpk8 / dpk2: the shipped shape's 4-pose tile on 4 and 8 waves
// and its 2-pose tile; dpkw / dpkw4: hid 128 with 8 / 4 heads, 2-pose tiles; dpkn / dpkn4: hid 64 with 2 / 4
// heads, 4-pose tiles), so every unqualified shape constant below is that instance's.  What the host knows an
// instance by (SamplerInst, dpk_kernels.hip: INSTANCES) is made of SHAPE (plain C++: a CPU-only build that
// includes this file after dpk_layout.inc compiles it too, tests/c/dpk_pack_check.cpp) and, in HIP builds,
// fused_temb and launch_sample; which kernel modes exist for which instance is decided beside the table.
#include "dpk_pack.inc"

// the GCNpose kernels (coords 2 -> 3) are compiled for the shipped shape's 4-wave tiles alone
constexpr InstShape SHAPE = {D, NH, J, NL, J_MIN, P, NW, NT, SM_FLOATS * 4, (size_t)NL * D, GEMM_MODES, MODE_BF16 && NW == 4,
                             CIN, COUT, ARENA_FLOATS, TEMB_FLOATS, MODE_F16X3 ? ARENA16_BYTES : 0,
                             MODE_BF16 ? ARENA16_BYTES / 2 : 0, pack_model};

#ifdef __HIPCC__
static void fused_temb(const float* temb, const float* t, int stride, int count, float* out, hipStream_t st) {
    hipLaunchKernelGGL(temb_kernel, dim3((unsigned)count), dim3(256), 0, st, temb, t, stride, out);
}

// One sample_kernel launch of `blocks` workgroups for the graph pattern (sparse: the compiled H36M one),
// the noise source (the caller's draws, ZM = 1, or counter-based) and the GEMM mode gm (0 fp32 from W;
// 1 f16x3 / 2 bf16 from W16: each compiled where the instance's descriptor has the mode, SHAPE.modes; a mode it
// lacks never gets here, check_ready refuses it).  ST: the hypothesis start (dpk_sample_start, M_SAMPLE only).
// PD: the padded-tile kernels (a.n_pts < 17; dense graph, fp32 and f16x3: bf16 is refused for such a handle).
// Each launch site leaves the census word of the instantiation it names (dpk_shared::kernel_id of this namespace's
// tile, DPK_TILE_ID, and the site's own template arguments) in last_kernel.
using ::dpk_shared::kernel_id;
using ::dpk_shared::last_kernel;
constexpr int TILE_ID = DPK_TILE_ID;
template <int MODE, bool SP, int ZM, bool ST = false, bool PD = false>
static void launch_gemm_mode(int gm, dim3 grid, size_t shmem, hipStream_t st, const SampleArgs& a, const float* W,
                             const char* W16) {
    if constexpr (SHAPE.has_mode(1)) {
        if (gm == 1) {
            hipLaunchKernelGGL((sample_kernel<MODE, SP, 1, ZM, ST, PD>), grid, dim3(NT), shmem, st, a, W, W16);
            last_kernel = kernel_id(TILE_ID, MODE, SP, 1, ZM, ST, PD);
            return;
        }
    }
    if constexpr (SHAPE.has_mode(2) && !PD) {
        if (gm == 2) {
            hipLaunchKernelGGL((sample_kernel<MODE, SP, 2, ZM, ST, PD>), grid, dim3(NT), shmem, st, a, W, W16);
            last_kernel = kernel_id(TILE_ID, MODE, SP, 2, ZM, ST, PD);
            return;
        }
    }
    hipLaunchKernelGGL((sample_kernel<MODE, SP, 0, ZM, ST, PD>), grid, dim3(NT), shmem, st, a, W, W16);
    last_kernel = kernel_id(TILE_ID, MODE, SP, 0, ZM, ST, PD);
}
template <int MODE>
static void launch_sample(bool sparse, int gm, int blocks, size_t shmem, hipStream_t st, const SampleArgs& a,
                          const float* W, const char* W16) {
    const dim3 grid((unsigned)blocks);
    if constexpr (PADDED && MODE != M_POSE) {
        if (a.n_pts != J) {     // a padded handle: its arena is never sparse (pack_model)
            if constexpr (MODE == M_SAMPLE) {
                if (a.start_on) {
                    if (a.noise) launch_gemm_mode<MODE, false, 1, true, true>(gm, grid, shmem, st, a, W, W16);
                    else launch_gemm_mode<MODE, false, 0, true, true>(gm, grid, shmem, st, a, W, W16);
                    return;
                }
                if (a.noise) {
                    launch_gemm_mode<MODE, false, 1, false, true>(gm, grid, shmem, st, a, W, W16);
                    return;
                }
            }
            launch_gemm_mode<MODE, false, 0, false, true>(gm, grid, shmem, st, a, W, W16);
            return;
        }
    }
    if constexpr (MODE == M_SAMPLE) {
        if (a.start_on) {
            if (a.noise) {
                if (sparse) launch_gemm_mode<MODE, true, 1, true>(gm, grid, shmem, st, a, W, W16);
                else launch_gemm_mode<MODE, false, 1, true>(gm, grid, shmem, st, a, W, W16);
            } else {
                if (sparse) launch_gemm_mode<MODE, true, 0, true>(gm, grid, shmem, st, a, W, W16);
                else launch_gemm_mode<MODE, false, 0, true>(gm, grid, shmem, st, a, W, W16);
            }
            return;
        }
        if (a.noise) {
            if (sparse) launch_gemm_mode<MODE, true, 1>(gm, grid, shmem, st, a, W, W16);
            else launch_gemm_mode<MODE, false, 1>(gm, grid, shmem, st, a, W, W16);
            return;
        }
    }
    if (sparse) launch_gemm_mode<MODE, true, 0>(gm, grid, shmem, st, a, W, W16);
    else launch_gemm_mode<MODE, false, 0>(gm, grid, shmem, st, a, W, W16);
}

// The census words of every sample_kernel the launchers above instantiate for kernel mode MODE, by their own
// predicates: the padded kernels where PADDED and not for M_POSE, dense graph only; ZM and START in sample mode only;
// fp32 always, f16x3 and bf16 where SHAPE has the mode, bf16 never padded.  It names no kernel, so it compiles none.
template <int MODE>
static void list_mode(std::vector<uint32_t>& out) {
    constexpr int flags = MODE == M_SAMPLE ? 2 : 1;    // values ZM and START take
    for (int pd = 0; pd < ((PADDED && MODE != M_POSE) ? 2 : 1); ++pd)
        for (int sp = pd ? 0 : 1; sp >= 0; --sp)
            for (int stt = 0; stt < flags; ++stt)
                for (int zm = 0; zm < flags; ++zm)
                    for (int gm = 0; gm < 3; ++gm)
                        if (gm == 0 || (SHAPE.has_mode(gm) && !(gm == 2 && pd)))
                            out.push_back(kernel_id(TILE_ID, MODE, sp != 0, gm, zm, stt != 0, pd != 0));
}
// ... for the kernel modes this tile's descriptor has a launcher for (SamplerInst::kernels)
static void list_kernels(const SamplerInst& self, std::vector<uint32_t>& out) {
    if (self.launch[M_SAMPLE]) list_mode<M_SAMPLE>(out);
    if (self.launch[M_EPS]) list_mode<M_EPS>(out);
    if (self.launch[M_POSE]) list_mode<M_POSE>(out);
}
#endif
