"""GPU: every site that draws a counter-based random number, against tests/counter_draws.py, the numpy
restatement of the two generators (pinned on the CPU by tests/test_counter_draws_cpu.py).

Normal draws (``normal_noise``: Philox4x32-10 + Box-Muller) are read back from outputs of models whose output
layer is zero, so eps is exactly 0 in every GEMM mode and a step is x0 = fl(xt / cf1),
xn = fl(fl(cf2 x0) + fl(cf3 z)): z = (xn - cf2 x0) / cf3 in float64, to within ``recover`` <= 1e-6 under the
schedule counter_draws.betas() (derivation in that module's docstring, asserted there from the coefficients and
here again from the outputs).  Every element of every output read is compared with ``normal_ref`` at its
global (seed, step, element) under the derived per-element bar ``draw_bar(r, recover)``; each case records
max(|z_gpu - z_ref| / draw_bar) (conftest.record_delta, bar 1), MI355X values in
profiles/counter_draws_deltas.txt.  Where two sites promise the same draw (the fused sampler's step and
``dpk_ddim_update``, ``dpk_q_sample`` and the sampler's start, tail plans, tiles, batch sizes) they are also
compared bitwise.  Uniform draws (``counter_uniform``, the seeded GMM component choice) are exact in float64, so
``batch(seed=s)`` must equal ``batch(u=uniform_ref(s, position))`` bit for bit.

The cases, by the sites they reach:
  a  dpk::ddim_kernel (dpk_ddim_update) on the hid-96 handle, 1024 poses, steps 0, 1, K - 2, six seeds that
     exercise both key words and the wrapper's masking of -1;
  b  the same entry point on a per-op handle (it launches the same kernel there), and dpkg::ddim, which only
     the per-op sampler loop launches: sample(trajectory=True) on that handle (in case c's list);
  c  the fused sampler's ZM = 0 kernels: five persistent shapes in every GEMM mode the handle has, 4- and
     8-wave tiles at hid 96, a non-H36M adjacency (dense kernels); N = 7 is one full 4-pose tile and a 3-pose
     partial one;
  d  tail plans "four", "two_pose", "step_split" at N = 1, 2, 3, 5 and 1100 (step-split halves), the recompute
     path of a second half (debug_split(1)), and sample(x[:n]) == sample(x)[:n];
  e  the hypothesis start's e (step -1) through the sampler and dpk_q_sample, with and without a scale;
  f  the per-op path's recorded K-step loop, replayed from a cache of 8 loops keyed by seed;
  g  the GMM sampler's seeded component choice.
Element indices at or above 2^32 (the counter's second word) would need tens of GiB per call and are covered on
the restatement only.
"""
import functools
import os
from types import SimpleNamespace as ns

import numpy as np
import pytest
import torch

import counter_draws as C
from conftest import record_delta
from diffpose_amd._lib import DpkError
from diffpose_amd.gcndiff import H36M_EDGES, HipGCNdiff, adj_mx_from_edges
from diffpose_amd.gmm import PoseGeneratorGMM
from diffpose_amd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu

CHAIN16 = tuple((i, i + 1) for i in range(15))
DENSE_EDGES = tuple(H36M_EDGES) + ((3, 16), (6, 13))
# name: hid, heads, layers, joints, edges, GEMM-mode bits (dpk_gemm_modes) — the five persistent-sampler
# shapes, hid 96 on a non-H36M adjacency, and a per-op shape
SHAPES = {
    "h96n4": (96, 4, 5, 17, H36M_EDGES, 0b111),
    "h128n8": (128, 8, 3, 17, H36M_EDGES, 0b011),
    "h128n4": (128, 4, 3, 17, H36M_EDGES, 0b011),
    "h64n2": (64, 2, 2, 17, H36M_EDGES, 0b011),
    "h64n4": (64, 4, 2, 17, H36M_EDGES, 0b011),
    "dense": (96, 4, 5, 17, DENSE_EDGES, 0b111),
    "perop": (48, 4, 1, 16, CHAIN16, 0b001),
}
PERSISTENT = ("h96n4", "h128n8", "h128n4", "h64n2", "h64n4")
MODES = ("fp32", "f16x3", "bf16")
BETAS = torch.from_numpy(C.betas())
SEQ3, SEQ2, SEQ10 = list(C.SEQ3), list(C.SEQ2), list(C.SEQ10)


def ends_session(fn):
    """A library / HIP error is no parity miss: run nothing more on the device."""
    @functools.wraps(fn)
    def run(*a, **k):
        try:
            return fn(*a, **k)
        except DpkError as e:
            pytest.exit(f"counter_draws/{fn.__name__}: {e}", returncode=3)
    return run


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _modes(name):
    return [m for i, m in enumerate(MODES) if (SHAPES[name][5] >> i) & 1]


@pytest.fixture(scope="module")
def models(dev):
    """One model per shape for the whole module, its output layer zero: eps is exactly 0 whatever the input,
    the timestep and the GEMM mode, which is asserted here so that a later miss cannot be the network's."""
    made = {}

    def get(name):
        if name not in made:
            hid, heads, layers, npts, edges, bits = SHAPES[name]
            cfg = ns(model=ns(hid_dim=hid, emd_dim=hid, coords_dim=[5, 5], num_layer=layers, n_head=heads,
                              dropout=0.25, n_pts=npts))
            m = HipGCNdiff(adj_mx_from_edges(npts, edges), cfg, device=dev)
            made[name] = m
            sd = dict(synthetic_state_dict(hid=hid, n_layers=layers, n_pts=npts))
            for k in ("gconv_output.weight", "gconv_output.bias"):
                sd[k] = np.zeros_like(np.asarray(sd[k]))
            m.load_state_dict(sd)
            assert m.gemm_modes() == bits, (name, m.gemm_modes())
            g = torch.Generator().manual_seed(5)
            x = torch.randn(7, npts, 5, generator=g).to(dev)
            t = torch.tensor([0.0, 3.0, 10.0, 25.0, 49.0, 50.0, 50.0], device=dev)
            for mode in _modes(name):
                m.set_gemm_mode(mode)
                try:
                    for xx in (x, torch.zeros_like(x)):
                        eps = m(xx, None, t)
                        assert eps.shape == xx.shape and bool((eps == 0).all()), (name, mode)
                finally:
                    m.set_gemm_mode("fp32")
        return made[name]

    yield get
    for m in made.values():
        m.close()


def _np(t):
    return t.detach().cpu().double().numpy().reshape(-1)


def _check(tag, z, recover, seed, step, first=0):
    """All of z (float64, the draws read back, element ``first`` onwards) against normal_ref under the
    per-element bar; records and returns the largest ratio."""
    idx = np.arange(first, first + z.size, dtype=np.int64)
    ref, r = C.normal_ref(seed, step, idx)
    recover = np.broadcast_to(np.asarray(recover, np.float64), z.shape)
    assert np.isfinite(z).all(), tag
    assert float(recover.max()) <= C.RECOVER_MAX, (tag, float(recover.max()))
    bar = C.draw_bar(r, recover)
    d = np.abs(z - ref)
    ratio = np.where(bar > 0, d / np.where(bar > 0, bar, 1.0), np.where(d == 0, 0.0, np.inf))   # r = 0: z = 0 exactly
    k = int(np.argmax(ratio))
    ok = record_delta(float(ratio[k]), 1.0, tag)
    assert ok, f"{tag}: element {first + k}: got {z[k]!r}, want {ref[k]!r} (r {r[k]:.3f}, bar {bar[k]:.3e}); " \
               f"{int((ratio > 1).sum())} of {z.size} over the bar"
    return float(ratio[k])


def _read_steps(tag, xs, x0s, seq, seed, steps, first=0):
    """the draws of ``steps`` out of a zero-eps trajectory, each against the reference"""
    cf = C.coeffs(seq)
    for k in steps:
        x0, xn = _np(x0s[k]), _np(xs[k + 1])
        _check(f"{tag}/step{k}", C.recover_z(cf[k], x0, xn), C.recover_step(cf[k], x0, xn), seed, k, first)


# ---------------------------------------------------------------------------------------
# a, b. dpk_ddim_update

@pytest.mark.parametrize("name", ["h96n4", "perop"])
@ends_session
def test_ddim_update_draws(dev, models, name):
    """x_t = eps = 0: x' = fl(cf3 z), x0 = 0.  1024 poses; steps 0, 1 and K - 2 of K = 10 at eta = 1."""
    m = models(name)
    npts = SHAPES[name][3]
    zero = torch.zeros(1024, npts, 5, device=dev)
    n = zero.numel()
    assert n == 1024 * 85 or name != "h96n4"
    m.set_schedule(SEQ10, BETAS, C.ETA)
    cf = C.coeffs(SEQ10)
    idx = np.arange(n)
    for step in (0, 1, len(SEQ10) - 2):
        got = {}
        for seed in C.SEEDS + (-1,):
            xn, x0 = m.ddim_update(zero, zero, step, seed=seed)
            assert bool((x0 == 0).all())
            got[seed] = xn
            z = C.recover_z(cf[step], 0.0, _np(xn))
            _check(f"counter_draws/ddim_update/{name}/seed{seed}/step{step}", z,
                   C.recover_step(cf[step], 0.0, _np(xn)), seed % (1 << 64), step)
        assert torch.equal(got[-1], got[(1 << 64) - 1])
        assert not torch.equal(got[0], got[1 << 32]) and not torch.equal(got[7], got[(1 << 32) + 7])
        c0 = np.concatenate([C.philox_words(s, step, idx)[0] >> np.uint32(8) for s in C.SEEDS])
        print(f"{name} step {step}: smallest u1 read = {int(c0.min()) + 1} * 2^-24")


# ---------------------------------------------------------------------------------------
# c. the fused sampler (and the per-op loop's dpkg::ddim), K = 3, eta = 1, from x = 0

CASES_C = ([("h96n4", mode, w) for mode in MODES for w in (4, 8)]
           + [(name, mode, 0) for name in PERSISTENT[1:] for mode in MODES[:2]]
           + [("dense", "fp32", 0), ("perop", "fp32", 0)])


def test_case_list_covers_every_mode_of_every_shape():
    for name in SHAPES:
        if name != "dense":
            assert {mode for n_, mode, _ in CASES_C if n_ == name} == set(_modes(name)), name


@pytest.mark.parametrize("name,mode,waves", CASES_C)
@ends_session
def test_sampler_step_draws(dev, models, name, mode, waves):
    m = models(name)
    npts = SHAPES[name][3]
    N = 7
    zero = torch.zeros(N, npts, 5, device=dev)
    seed = C.SEED_C
    m.set_gemm_mode(mode)
    if waves:
        m.set_tile_waves(waves)
    try:
        xs, x0s = m.sample(zero, SEQ3, BETAS, eta=C.ETA, seed=seed, trajectory=True)
        out = m.sample(zero, SEQ3, BETAS, eta=C.ETA, seed=seed)
        # the host loop's update fed the sampler's own x_t and a zero eps (the schedule is bound by sample)
        ups = [m.ddim_update(xs[k], zero, k, seed=seed) for k in range(3)]
    finally:
        m.set_gemm_mode("fp32")
        if waves:
            m.set_tile_waves(0)
    assert bool((xs[0] == 0).all()) and bool((x0s[0] == 0).all())
    _read_steps(f"counter_draws/sampler/{name}/{mode}/w{waves}", xs, x0s, SEQ3, seed, (0, 1))
    for k in range(3):
        assert torch.equal(ups[k][0], xs[k + 1]), (k, "x'")
        assert torch.equal(ups[k][1], x0s[k]), (k, "x0")
    # the last step's c1 is 0 and its cf2 is 1: its (finite) draw enters nothing
    assert torch.equal(xs[3], x0s[2]) and torch.equal(out, xs[3])


# ---------------------------------------------------------------------------------------
# d. tail plans, step-split halves, batch sizes

@ends_session
def test_tail_plans_and_batch_sizes(dev, models):
    """1,100 poses = 275 tiles: on a 256-CU device one full round and 19 tiles, which plan "step_split" runs as
    two halves each; debug_split(1) makes every second half recompute from x_in.  Every pose draws by its global
    element index under every plan, so the plans agree bitwise (eps is 0, the tiles' GEMM shapes do not enter)."""
    m = models("h96n4")
    seed = C.SEED_C
    big = torch.zeros(1100, 17, 5, device=dev)

    def run(n):
        xs, x0s = m.sample(big[:n].contiguous(), SEQ3, BETAS, eta=C.ETA, seed=seed, trajectory=True)
        return xs, x0s

    try:
        first = None
        for plan in ("four", "two_pose", "step_split", "step_split/recompute"):
            m.set_tail_plan(plan.split("/")[0])
            m.debug_split(1 if plan.endswith("recompute") else 0)
            xs, x0s = run(1100)
            _read_steps(f"counter_draws/plans/{plan}/n1100", xs, x0s, SEQ3, seed, (0, 1))
            if first is None:
                first = (xs, x0s)
            assert torch.equal(xs, first[0]) and torch.equal(x0s, first[1]), plan
            if plan.endswith("recompute"):
                print("second halves that recomputed:", m.debug_split(0, read=True))
                continue
            for n in (1, 2, 3, 5):
                pxs, px0s = run(n)
                _read_steps(f"counter_draws/plans/{plan}/n{n}", pxs, px0s, SEQ3, seed, (0, 1))
                assert torch.equal(pxs, xs[:, :n]) and torch.equal(px0s, x0s[:, :n]), (plan, n)
    finally:
        m.debug_split(0)
        m.set_tail_plan("step_split")


# ---------------------------------------------------------------------------------------
# e. the hypothesis start's draws (step -1)

def _read_start(tag, xT, seed, scale=None):
    """e = x_T / (scale sb) from x = 0: x_T = fl(fl(e scale) sb), two half-ulp roundings"""
    sb = C.start_sb()
    den = sb if scale is None else _np(scale) * sb
    v = _np(xT)
    _check(tag, v / den, 2.0 ** -23 * np.abs(v / den), seed, -1)


@pytest.mark.parametrize("name,waves", [(n_, 0) for n_ in PERSISTENT] + [("h96n4", 8), ("perop", 0)])
@ends_session
def test_start_draws_in_the_sampler(dev, models, name, waves):
    """xs[0] of a start-on call from x = 0 with no scale and no caller noise; the steps after it, which cannot be
    read back from a non-zero x_t under this schedule, are the host loop's update of the same (seed, step), bitwise."""
    m = models(name)
    npts = SHAPES[name][3]
    zero = torch.zeros(7, npts, 5, device=dev)
    seed = C.SEED_C + 1
    if waves:
        m.set_tile_waves(waves)
    try:
        xs, x0s = m.sample(zero, SEQ3, BETAS, eta=C.ETA, seed=seed, trajectory=True, t_start=C.T_START)
        ups = [m.ddim_update(xs[k], zero, k, seed=seed) for k in range(3)]
        alone = m.q_sample(zero, C.T_START, seed=seed)
    finally:
        if waves:
            m.set_tile_waves(0)
    _read_start(f"counter_draws/start/sampler/{name}/w{waves}", xs[0], seed)
    assert torch.equal(alone, xs[0])
    for k in range(3):
        assert torch.equal(ups[k][0], xs[k + 1]) and torch.equal(ups[k][1], x0s[k]), k


@pytest.mark.parametrize("name", ["h96n4", "perop"])
@ends_session
def test_start_draws_alone_and_under_a_scale(dev, models, name):
    """dpk_q_sample over 300 poses (several blocks; on the per-op handle pe = 16 * 5, the index still the global
    element), and with a [F, J, 5] scale of non-trivial values over N = 4 F poses: the draw is the unscaled one
    of the global index, not of the scale row."""
    m = models(name)
    npts = SHAPES[name][3]
    m.set_schedule(SEQ3, BETAS, C.ETA)
    for seed in (0, (1 << 32) + 7, -1):
        xT = m.q_sample(torch.zeros(300, npts, 5, device=dev), C.T_START, seed=seed)
        _read_start(f"counter_draws/start/q_sample/{name}/seed{seed}", xT, seed % (1 << 64))
    F = 5
    seed = C.SEED_C + 2
    g = torch.Generator().manual_seed(9)
    rows = (0.25 + 2.0 * torch.rand((F, npts, 5), generator=g)) * (1 - 2 * (torch.rand((F, npts, 5), generator=g) < 0.3).float())
    zero = torch.zeros(4 * F, npts, 5, device=dev)
    full = rows.repeat(4, 1, 1)
    xT = m.q_sample(zero, C.T_START, start_scale=rows.to(dev), seed=seed)
    _read_start(f"counter_draws/start/q_sample_scaled/{name}", xT, seed, full)
    xs, _ = m.sample(zero, SEQ3, BETAS, eta=C.ETA, seed=seed, trajectory=True, t_start=C.T_START,
                     start_scale=rows.to(dev))
    _read_start(f"counter_draws/start/sampler_scaled/{name}", xs[0], seed, full)
    assert torch.equal(xs[0], xT)


# ---------------------------------------------------------------------------------------
# f. the per-op path's recorded loop

@ends_session
def test_recorded_loop_carries_its_own_seed(dev, models):
    """Without a trajectory the per-op K-step loop is a recorded graph, cached per seed at eta != 0, 8 entries.
    Seeds 1..10, then 1 again: eleven calls, two evictions, the last a re-recording of the first.  K = 2 from
    x = 0: out = fl(1 * fl(fl(cf3 z0) / cf1')), so z0 = out cf1' / cf3 to two half-ulp roundings."""
    m = models("perop")
    zero = torch.zeros(7, 16, 5, device=dev)
    cf = C.coeffs(SEQ2).astype(np.float64)
    assert cf[1, 2] == 1.0 and cf[1, 3] == 0.0
    outs = []
    for seed in list(range(1, 11)) + [1]:
        out = m.sample(zero, SEQ2, BETAS, eta=C.ETA, seed=seed).clone()
        v = _np(out)
        _check(f"counter_draws/recorded_loop/seed{seed}/call{len(outs)}", v * cf[1, 1] / cf[0, 3],
               2.0 ** -23 * np.abs(v) * cf[1, 1] / cf[0, 3], seed, 0)
        outs.append(out)
    assert torch.equal(outs[-1], outs[0])
    for a in range(10):
        for b in range(a + 1, 10):
            assert not torch.equal(outs[a], outs[b])
    if os.environ.get("DPK_GEN_GRAPH") is None:
        assert m.debug_resources()["generic_loop_graphs"] == 8


# ---------------------------------------------------------------------------------------
# g. the GMM sampler's seeded component choice

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kn", [1, 7, 64])
@pytest.mark.parametrize("J", [17, 16, 21])
def test_gmm_seeded_choice_is_the_counter_uniform(dev, J, kn, dtype):
    """batch(seed=s) is batch(u=U) with U[f, j] = uniform_ref(s, f * J + j), f the output position: exact.
    31 positions (J * 31 threads: no multiple of 256, up to 3 blocks) over 12 source frames, with repeats and
    indices past the source count; Dirichlet weights."""
    rng = np.random.Generator(np.random.PCG64(100 * J + kn))
    n_src, F = 12, 31
    w = rng.dirichlet(np.ones(kn), size=(n_src, J))
    gm = np.concatenate([w[..., None], rng.uniform(-1, 1, size=(n_src, J, kn, 4))], axis=-1).astype(dtype)
    p3 = rng.normal(size=(n_src, J, 3)).astype(dtype)
    ds = PoseGeneratorGMM([p3], [gm], [["a"] * n_src], [np.zeros((n_src, 1), np.float32)], device=dev)
    idx = rng.integers(0, 3 * n_src, size=F)
    idx[:4] = [5, 5, n_src + 5, 0]
    assert (idx >= n_src).any() and len(set(idx % n_src)) < F
    ctr = np.arange(F * J)
    picks = []
    for seed in (0, 7, (1 << 64) - 1, -1):
        U = C.uniform_ref(seed, ctr).reshape(F, J)
        a = ds.batch(idx, seed=seed)
        b = ds.batch(idx, u=U)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), seed
        picks.append(a[0])
        if kn > 1:
            # the uniforms decide: those of the next counter pick other components somewhere
            c = ds.batch(idx, u=C.uniform_ref(seed, ctr + 1).reshape(F, J))
            assert not torch.equal(a[0], c[0])
    assert torch.equal(picks[2], picks[3])
    if kn > 1:
        assert not torch.equal(picks[0], picks[1])
