// dpk_counter.inc — the counter-based 64-bit word behind the library's uniform draws: splitmix64's output mixer on
// seed + 0x9E3779B97F4A7C15 * (ctr + 1) mod 2^64, i.e. splitmix64's (ctr + 1)-th output for `seed`.  The GMM sampler's
// counter_uniform (csrc/dpk_gmm.hip) takes its top 53 bits, dpk_train_draws' timesteps its top 32
// (tests/counter_draws.py restates it as counter_word; diffpose_amd/schedule.py as word).
#pragma once
#include <stdint.h>

namespace dpk_counter {

__host__ __device__ __forceinline__ uint64_t counter_word(uint64_t seed, uint64_t ctr) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (ctr + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

}  // namespace dpk_counter
