"""CPU: pins tests/counter_draws.py, the restatement the GPU draw tests compare the kernels with: published
known-answer vectors for Philox4x32-10 and splitmix64, the moments and the separation of its streams, that the
fp32 order of the kernel stays inside the bar on the CPU already, and that the schedule the GPU tests run lets
every draw be read back to 1e-6.

The statistical bars are the project's: over n independent standard normals the sample mean has standard
deviation 1/sqrt(n) and the sample variance sqrt(2/n), five of each is the bar; 5/sqrt(n) likewise for the
correlation of two independent streams.
"""
import numpy as np

import counter_draws as C

N6 = 1_000_000
R_MAX = float(np.sqrt(48.0 * np.log(2.0)))          # u1 = 2^-24


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10"""
    f = 0xFFFFFFFF
    for ctr, key, want in (
        ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
        ((f, f, f, f), (f, f), "408f276d 41c83b0e a20bc7c6 6d5451fd"),
        ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
         "d16cfe09 94fdcceb 5001e420 24126ea1"),
    ):
        out = C.philox4x32_10(*ctr, *key)
        assert all(o.dtype == np.uint32 for o in out)
        assert _hex(out) == want
    # vectorised: the three at once give the three
    out = C.philox4x32_10([0, f, 0x243F6A88], [0, f, 0x85A308D3], [0, f, 0x13198A2E], [0, f, 0x03707344],
                          [0, f, 0xA4093822], [0, f, 0x299F31D0])
    assert _hex(o[2] for o in out) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    assert _hex(o[0] for o in out) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"


def test_splitmix64_known_answers_and_the_uniform_grid():
    w = C.counter_word(0, np.arange(3))
    assert [f"{int(v):016x}" for v in w] == ["e220a8397b1dcdaf", "6e789e6aa1b965f4", "06c45d188009454f"]
    assert np.array_equal(C.uniform_ref(0, np.arange(3)), (w >> np.uint64(11)).astype(np.float64) / 2.0 ** 53)
    for seed in (0, 7, (1 << 64) - 1, -1):
        u = C.uniform_ref(seed, np.arange(200_000))
        assert u.dtype == np.float64 and u.min() >= 0.0 and u.max() < 1.0
        k = u * 2.0 ** 53
        assert np.array_equal(k, np.floor(k))
        assert abs(u.mean() - 0.5) <= 5.0 / np.sqrt(12.0 * u.size)
    assert np.array_equal(C.uniform_ref(-1, np.arange(100)), C.uniform_ref((1 << 64) - 1, np.arange(100)))
    # the counter is ctr + 1: ctr = 0 is not the bare seed's mix, and consecutive counters are one apart
    assert np.array_equal(C.counter_word(5, np.arange(1, 9)),
                          C.counter_word((5 + 0x9E3779B97F4A7C15) % (1 << 64), np.arange(8)))


def test_counter_and_key_layout():
    """The normal draw's Philox call, word for word, at a point where every word is non-trivial"""
    seed, step, idx = (0x299F31D0 << 32) | 0xA4093822, 0x13198A2E, (0x85A308D3 << 32) | 0x243F6A88
    want = C.philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x5EED, 0xA4093822, 0x299F31D0)
    c0, c1 = int(want[0]), int(want[1])
    z, r = C.normal_ref(seed, step, np.array([idx], dtype=np.uint64))
    u1, u2 = ((c0 >> 8) + 1) / 2.0 ** 24, (c1 >> 8) / 2.0 ** 24
    assert r[0] == np.sqrt(-2.0 * np.log(u1)) and z[0] == r[0] * np.cos(2.0 * np.pi * u2)
    # step -1 is 0xFFFFFFFF; the seed is taken mod 2^64
    i = np.arange(1000)
    assert np.array_equal(C.normal_ref(3, -1, i)[0], C.normal_ref(3, 0xFFFFFFFF, i)[0])
    assert np.array_equal(C.normal_ref(-1, 2, i)[0], C.normal_ref((1 << 64) - 1, 2, i)[0])
    assert not np.array_equal(C.normal_ref(-1, 2, i)[0], C.normal_ref((1 << 32) - 1, 2, i)[0])
    # u1 = 1 (c0 >> 8 = 2^24 - 1) is r = 0, u1 = 2^-24 the largest radius; neither is a log of 0
    assert np.sqrt(-2.0 * np.log(1.0 / C.TWO24)) == R_MAX
    assert float(C.draw_bar(R_MAX, C.RECOVER_MAX)) < 5.5e-6 and float(C.draw_bar(R_MAX, 0.0)) < 4.5e-6


def test_moments_of_normal_ref():
    for seed, step, lo in ((0, 0, 0), ((1 << 40) + 3, -1, 0), (7, 3, 1 << 32)):
        z, r = C.normal_ref(seed, step, np.arange(lo, lo + N6, dtype=np.uint64))
        assert np.isfinite(z).all() and r.min() >= 0.0 and r.max() <= R_MAX
        mean, var = float(z.mean()), float(z.var(ddof=1))
        print(f"seed {seed} step {step}: mean {mean:.3e} var-1 {var - 1:.3e} max r {r.max():.3f}")
        assert abs(mean) <= 5.0 / np.sqrt(N6)
        assert abs(var - 1.0) <= 5.0 * np.sqrt(2.0 / N6)


def test_normal_f32_stays_inside_the_bar():
    """the kernel's fp32 order, in numpy's float32 functions, against the float64 reference: every element within
    draw_bar(r, 0), over 2.1e6 draws of which 1e5 sit at element indices above 2^32"""
    worst, rmax = 0.0, 0.0
    for seed, step, lo, n in ((0, 0, 0, N6), (C.SEED_C, 1, 0, N6), (7, -1, (1 << 32) + 5, 100_000)):
        idx = np.arange(lo, lo + n, dtype=np.uint64)
        z, r = C.normal_ref(seed, step, idx)
        d = np.abs(C.normal_f32(seed, step, idx).astype(np.float64) - z)
        bar = C.draw_bar(r, 0.0)
        k = int(np.argmax(r))
        print(f"seed {seed} step {step}: max |f32 - f64| {d.max():.3e}, max ratio {np.max(d / bar):.3f}; "
              f"largest r {r[k]:.3f}: {d[k]:.3e} of {bar[k]:.3e}")
        assert np.all(d <= bar)
        worst, rmax = max(worst, float(np.max(d / bar))), max(rmax, float(r.max()))
    assert rmax > 4.9          # the tail is in the set
    assert worst > 0.05        # and the bar is of the error's order, not orders above it


def _corr(a, b):
    return float(np.mean((a - a.mean()) * (b - b.mean())) / (a.std() * b.std()))


def test_stream_separation():
    n = 200_000
    bar = 5.0 / np.sqrt(n)
    i = np.arange(n)
    s = 21
    base = C.normal_ref(s, 0, i)[0]
    pairs = {
        "seed s, s + 1": (base, C.normal_ref(s + 1, 0, i)[0]),
        "seed s, s + 2^32": (base, C.normal_ref(s + (1 << 32), 0, i)[0]),
        "step -1, 0": (C.normal_ref(s, -1, i)[0], base),
        "step 0, 1": (base, C.normal_ref(s, 1, i)[0]),
        "step -1, 1": (C.normal_ref(s, -1, i)[0], C.normal_ref(s, 1, i)[0]),
        "index i, i + 1": (base[:-1], base[1:]),
        "index i, i + 2^32": (base, C.normal_ref(s, 0, i.astype(np.uint64) + np.uint64(1 << 32))[0]),
    }
    for name, (a, b) in pairs.items():
        c = _corr(a, b)
        print(f"{name}: corr {c:.3e} (bar {bar:.3e})")
        assert abs(c) <= bar, name
        assert not np.array_equal(a, b)


def test_the_schedule_lets_every_draw_be_read_back():
    """recover <= 1e-6 on every element the GPU tests read, from the coefficients alone: for any draws with
    r <= R_MAX, and (tighter, printed) for the reference's draws of the largest sampler case."""
    ulp = 2.0 ** -23
    grow = 1.0 + 2.0 ** -22                      # fp32 roundings of the bounded quantities themselves
    for seq in (C.SEQ3, C.SEQ2, C.SEQ10):
        cf = C.coeffs(seq).astype(np.float64)
        assert np.isfinite(cf).all()
        assert np.all(cf[:-1, 3] > 0) and cf[-1, 3] == 0.0       # every step but the last draws
        assert cf[-1, 2] == 1.0                                   # alpha-bar of t = -1 is 1: the last cf2 x0 is exact
        # from x_t = 0: xn = fl(cf3 z), one rounding
        assert ulp * R_MAX * grow <= C.RECOVER_MAX
    # the start from x = 0, with or without a scale: fl(fl(e scale) sb), two half-ulp roundings
    assert 0.3 < C.start_sb() < 1.0
    assert ulp * R_MAX * grow <= C.RECOVER_MAX
    # the recorded loop, K = 2: out = fl(1 * fl(fl(cf3 z0) / cf1')), two half-ulp roundings
    # step 1 of K = 3 after a step 0 from x = 0: |cf2 x0| <= rho cf3' R, |xn| <= (rho + 1) cf3' R
    cf = C.coeffs(C.SEQ3).astype(np.float64)
    rho = cf[1, 2] * cf[0, 3] / (cf[1, 1] * cf[1, 3])
    worst = ulp * (2.0 * rho + 1.0) * R_MAX * grow
    print(f"SEQ3: c1 {cf[0, 3]:.4e}, {cf[1, 3]:.4e}; rho {rho:.4f}; worst-case recover at step 1 {worst:.3e}")
    assert worst <= C.RECOVER_MAX
    n = 1100 * C.PE
    xs, x0s, zs = C.model_steps(C.SEED_C, n)
    for k in (0, 1):
        rec = C.recover_step(cf[k], x0s[k], xs[k + 1])
        z = C.recover_z(cf[k], x0s[k], xs[k + 1])
        d = np.abs(z - zs[k][0])
        print(f"step {k}: max recover {rec.max():.3e}, max |recovered - drawn| {d.max():.3e}")
        assert rec.max() <= C.RECOVER_MAX
        assert np.all(d <= rec + 2.0 ** -24 * np.abs(zs[k][0]))   # + the draw's own rounding to fp32
