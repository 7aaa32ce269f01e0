"""A numpy restatement of the two counter-based generators the kernels draw from, the schedule and seeds the
draw tests run, and the bar a normal draw is held to (tests/test_counter_draws_cpu.py on the CPU,
tests/test_gpu_counter_draws.py on the GPU).  Everything is a function of its arguments; nothing here touches
a GPU or torch.

1. ``normal_noise(seed, step, idx)`` (csrc/dpk_sampler.inc): Philox4x32-10 on the counter
   {idx lo, idx hi, (uint32)step, 0x5EED} under the key {seed lo, seed hi}; from its first two output words
       u1 = ((c0 >> 8) + 1) / 2^24   in (0, 1]
       u2 = (c1 >> 8) / 2^24         in [0, 1)
       z  = sqrt(-2 ln u1) * cos(2 pi u2)
   in fp32 with 2 pi as 6.283185307179586f.  step = -1 (the hypothesis start's e) enters as 0xFFFFFFFF; eta's
   per-step z use steps 0..K-1.  ``normal_ref`` is the same function with the floating-point part in float64 and
   the true 2 pi; ``normal_f32`` is the kernel's fp32 order in numpy float32 (the CPU test's own check of the bar).
2. ``counter_uniform(seed, ctr)`` (csrc/dpk_gmm.hip): splitmix64's output mixer on
   seed + 0x9E3779B97F4A7C15 * (ctr + 1) mod 2^64, then (z >> 11) * 2^-53: exact in float64, so ``uniform_ref`` is
   compared bit for bit.  The GMM sampler's ctr is f * n_pts + j, the output position (not the source frame).

The bar (derived, not measured).  For one draw of radius r = sqrt(-2 ln u1):

    draw_bar(r, recover) = r * (theta + 6 * 2^-24) + recover,      theta = 2^-22 + 1.75e-7

  * the integer part is exact, and so are u1 and u2 in fp32 (24-bit integers times 2^-24), so the kernel's z
    differs from the float64 one only through the five fp32 operations after them;
  * theta bounds the angle's error: the fp32 product 2 pi * u2 lies in [4, 8) at its largest, where half an ulp
    is 2^-22, and the float32 constant 6.283185307179586f = 6.2831854820251465 is 1.75e-7 above 2 pi, which
    times u2 -> 1 is 1.75e-7.  |d cos| <= |d angle|, times r;
  * 6 * 2^-24 * r covers, in order: logf (1 ulp of ln u1: r = sqrt(-2 ln u1) moves by half that relative error,
    counted whole), sqrtf (1 ulp), cosf (2 ulp of a value <= 1), the final product (1/2 ulp), and slack.  The
    library is built without a fast-math flag, so these are the accurate library functions;
  * ``recover`` is what reading the draw back out of fp32 outputs adds (below), at most 1e-6 by the choice of
    schedule.
Across a run this is about 1e-6 at typical r and at most 4.5e-6 at the largest r there is, sqrt(48 ln 2) = 5.77
(u1 = 2^-24).  A generator that is wrong in its integer part (a round missing, a key or counter word dropped or
taken locally, sin for cos) misses by O(1) on most elements; a u1 drawn from [0, 1) misses by about 1 / (r k) at
u1 = k 2^-24, over 1e-3 for the smallest u1 among 1e5 draws.  If an MI355X run exceeds the bar, that is a finding
to explain, not a bar to widen.

Reading a draw back without amplification.  The GPU tests run models whose output layer is zero, so eps is
exactly 0 in every GEMM mode and a step is x0 = fl(xt / cf1), xn = fl(fl(cf2 x0) + fl(cf3 z)) with
(cf1, cf2, cf3) = (sqrt(at), sqrt(an), c1) of schedule.ddim_coeffs.  Then z = (xn - cf2 x0) / cf3 in float64 is
the draw up to ``recover_step`` = 2^-23 (|cf2 x0| + |xn|) / cf3: the two roundings are each half an ulp, of
fl(cf3 z) <= |cf2 x0| + |xn| (+ its own rounding) and of xn, and x0 is read from the output, so its own rounding
does not enter.  From x = 0, step 0 is xn = fl(cf3 z); the start from x = 0 is fl(fl(e scale) sb).  The last
step's c1 is 0 (alpha-bar of t = -1 is 1), so its draw enters nothing: steps 0..K-2 are read.  For recover <= 1e-6
at step 1, cf2 x0 must stay small against cf3 z there, i.e. step 0 must add much less noise than step 1: BETAS
below is small above t = 25 and large below it (the kernels take any beta table).  The CPU test asserts the
condition for every element the GPU tests read, from the coefficients and the reference draws alone.

Out of reach: element indices at or above 2^32 (the counter's second word) would need tens of GiB per call; the
CPU test covers that word on the restatement only.
"""
from __future__ import annotations

import numpy as np

_M32 = np.uint64(0xFFFFFFFF)
_M64 = (1 << 64) - 1
TWO24 = 16777216.0
PE = 85                              # floats per 17-joint pose (the per-op shape's 16 joints: 80)

# ---------------------------------------------------------------------------------------
# the cases both test files run
T_START = 50
ETA = 1.0
SEQ3 = (0, 25, 50)                   # K = 3: steps 0 and 1 carry draws
SEQ2 = (0, 50)                       # K = 2: the per-op recorded loop
SEQ10 = tuple(range(0, 50, 5))       # K = 10: dpk_ddim_update at steps 0, 1, K - 2
SEEDS = (0, 7, 1 << 32, (1 << 32) + 7, (1 << 64) - 1)      # and -1, which the wrappers mask to 2^64 - 1
SEED_C = (1 << 40) + 12345           # sampler cases: both key words in use


def betas() -> np.ndarray:
    """51 betas: 0.05 at t = 0, 0.02 at t = 1..25, 4e-6 above.  With SEQ3 at eta = 1, step 0 (t 50 -> 25) adds
    noise of standard deviation c1 = 1.0e-2 and step 1 (25 -> 0) of 0.22, so step 1's recovery error stays
    under 1e-6 (module docstring); 1 - alpha-bar at T_START is 0.43."""
    b = np.full(51, 4e-6, np.float64)
    b[0] = 0.05
    b[1:26] = 0.02
    return b.astype(np.float32)


def coeffs(seq, eta: float = ETA) -> np.ndarray:
    """schedule.ddim_coeffs of ``seq`` under ``betas()``: [K, 6] float32 (sqrt(1-at), cf1, cf2, cf3, c2, t)"""
    from diffpose_amd.schedule import alpha_bar_table, ddim_coeffs

    return ddim_coeffs(alpha_bar_table(betas()), list(seq), eta)


def start_sb(t_start: int = T_START) -> float:
    """sqrtf(1 - alpha_bar[t_start + 1]) as the host computes it for the hypothesis start"""
    from diffpose_amd.schedule import alpha_bar_table

    a = alpha_bar_table(betas())[t_start + 1]
    return float(np.sqrt(np.float32(np.float32(1.0) - a), dtype=np.float32))


# ---------------------------------------------------------------------------------------
# Philox4x32-10 and the normal draw

def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., Random123), vectorised: uint64 arithmetic masked to 32 bits.  Counter and key
    words broadcast against each other; returns the four output words as uint32 arrays."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(np.asarray(v, dtype=np.uint64) & _M32
                                                   for v in (c0, c1, c2, c3, k0, k1)))
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = m0 * c0                 # < 2^64: both factors are below 2^32
        p1 = m1 * c2
        n0 = (p1 >> s32) ^ c1 ^ k0
        n2 = (p0 >> s32) ^ c3 ^ k1
        c1 = p1 & _M32
        c3 = p0 & _M32
        c0, c2 = n0, n2
        k0 = (k0 + w0) & _M32
        k1 = (k1 + w1) & _M32
    return tuple(v.astype(np.uint32) for v in (c0, c1, c2, c3))


def philox_words(seed, step, idx):
    """the first two output words of normal_noise's Philox call"""
    seed = int(seed) & _M64
    idx = np.asarray(idx)
    if idx.dtype != np.uint64:
        assert np.all(idx >= 0)
        idx = idx.astype(np.uint64)
    o = philox4x32_10(idx & _M32, idx >> np.uint64(32), int(step) & 0xFFFFFFFF, 0x5EED,
                      seed & 0xFFFFFFFF, seed >> 32)
    return o[0], o[1]


def normal_ref(seed, step, idx):
    """(z, r): normal_noise(seed, step, idx) with its floating-point part in float64, and the draw's radius
    r = sqrt(-2 ln u1).  ``seed`` any int (taken mod 2^64), ``step`` >= -1, ``idx`` an array of element indices."""
    c0, c1 = philox_words(seed, step, idx)
    u1 = ((c0 >> np.uint32(8)).astype(np.float64) + 1.0) / TWO24
    u2 = (c1 >> np.uint32(8)).astype(np.float64) / TWO24
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * u2), r


def normal_f32(seed, step, idx):
    """normal_noise in numpy float32, in the kernel's order and with its constant 6.283185307179586f"""
    f = np.float32
    c0, c1 = philox_words(seed, step, idx)
    u1 = ((c0 >> np.uint32(8)).astype(f) + f(1.0)) * f(1.0 / TWO24)
    u2 = (c1 >> np.uint32(8)).astype(f) * f(1.0 / TWO24)
    z = np.sqrt(f(-2.0) * np.log(u1)) * np.cos(f(6.283185307179586) * u2)
    assert z.dtype == f
    return z


# ---------------------------------------------------------------------------------------
# splitmix64 and the uniform draw

def splitmix64_mix(z):
    """splitmix64's output mixer on uint64 words"""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def counter_word(seed, ctr):
    """the 64-bit word behind counter_uniform(seed, ctr): splitmix64's (ctr + 1)-th output for ``seed``"""
    ctr = np.atleast_1d(np.asarray(ctr)).astype(np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & _M64) + np.uint64(0x9E3779B97F4A7C15) * (ctr + np.uint64(1))
    return splitmix64_mix(z)


def uniform_ref(seed, ctr):
    """counter_uniform(seed, ctr): float64 in [0, 1), a multiple of 2^-53.  ``seed`` any int (mod 2^64)."""
    return (counter_word(seed, ctr) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


# ---------------------------------------------------------------------------------------
# the bar and the recovery error

THETA = 2.0 ** -22 + 1.75e-7
RECOVER_MAX = 1e-6


def draw_bar(r, recover):
    """the per-element bar on |z_gpu - z_ref| for a draw of radius r read back with error <= recover"""
    return np.asarray(r, np.float64) * (THETA + 6.0 * 2.0 ** -24) + recover


def recover_step(cf, x0, xn):
    """bound on |(xn - cf2 x0) / cf3 - z| for xn = fl(fl(cf2 x0) + fl(cf3 z)) in fp32, cf one row of coeffs()"""
    cf = np.asarray(cf, np.float64)
    return 2.0 ** -23 * (np.abs(cf[2] * np.asarray(x0, np.float64)) + np.abs(np.asarray(xn, np.float64))) / cf[3]


def recover_z(cf, x0, xn):
    """z = (xn - cf2 x0) / cf3 in float64"""
    cf = np.asarray(cf, np.float64)
    return (np.asarray(xn, np.float64) - cf[2] * np.asarray(x0, np.float64)) / cf[3]


def model_steps(seed, n, seq=SEQ3, x=None):
    """The fp32 trajectory of a zero-eps model from x = 0 (or x) with the reference draws rounded to fp32:
    lists xs [K + 1] and x0s [K] of float32 [n] over the global elements 0..n-1, and the float64 draws and radii
    of steps 0..K-2.  Used for the recovery condition and the expected magnitudes, not as the GPU's yardstick."""
    f = np.float32
    cf = coeffs(seq)
    idx = np.arange(n, dtype=np.int64)
    xs, x0s, zs = [np.zeros(n, f) if x is None else np.asarray(x, f)], [], []
    for k in range(len(seq)):
        z, r = normal_ref(seed, k, idx)
        x0 = xs[-1] / cf[k, 1]
        xn = (cf[k, 2] * x0 + cf[k, 3] * z.astype(f)) + cf[k, 4] * f(0)
        assert x0.dtype == f and xn.dtype == f
        x0s.append(x0)
        xs.append(xn)
        if k < len(seq) - 1:
            zs.append((z, r))
    return xs, x0s, zs
