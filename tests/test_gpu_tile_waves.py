"""GPU: the 8-wave instance of the 4-pose sampler tile (dpk_set_tile_waves(h, 8), HipGCNdiff.set_tile_waves(8)).

Two waves per SIMD run the same 68-row tile: each SIMD's GEMM column tiles are split between its two waves
(every output element keeps its k-ordered MFMA chain), attention heads, graph-product tiles and Chebyshev
columns between the two waves of a pose (the 2-pose tile's split), and LayerNorm keeps its row map on waves
0..3.  No summation order changes, so the 8-wave outputs are asserted BITWISE equal to the 4-wave ones, in
every GEMM mode, besides the oracle bars of the existing tests of the same mode:
  * fp32 and f16x3: |x - x_ref| <= 5e-6 (tests/test_gpu_parity.py, tests/test_gpu_gemm_modes.py);
  * bf16: |x - x_ref| <= 4e-3 (the study bar of tests/test_gpu_bf16_tolerance.py).
All cases force ``set_tail_plan("four")`` unless they say otherwise.
"""
import pytest
import torch

from conftest import record_delta

from diffpose_amd.data import synthetic_batch
from diffpose_amd.gcndiff import H36M_EDGES, HipGCNdiff, adj_mx_from_edges
from diffpose_amd.weights import synthetic_state_dict
from helpers import betas as _betas, maxdiff as _maxdiff

pytestmark = pytest.mark.gpu

TOL = {"fp32": 5e-6, "f16x3": 5e-6, "bf16": 4e-3}
MODES = ("fp32", "f16x3", "bf16")


def _seq(k):
    """exactly k timesteps of T' = 50, evenly spaced"""
    return list(range(0, 50, 50 // k))[:k]


def _ones():
    return torch.ones(1, 1, 17, dtype=torch.bool, device="cuda:0")


@pytest.fixture(scope="module")
def model():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    m = HipGCNdiff(adj_mx_from_edges(), None, device="cuda:0")
    m.load_state_dict(synthetic_state_dict())
    m.set_tail_plan("four")
    m.set_tile_waves(8)
    yield m
    m.close()


@pytest.fixture(scope="module")
def x9():
    return torch.from_numpy(synthetic_batch(9, seed=88)[0])


@pytest.fixture(scope="module")
def oracle_finals(x9):
    """The CPU oracle's final x of the 9 poses after K = 3 and K = 2 steps (per pose: a prefix of the batch
    is the oracle of that prefix)."""
    from oracle import gcndiff_oracle as O

    P, adj = O.params_to_torch(synthetic_state_dict()), O.adjacency()
    ones = torch.ones(1, 1, 17, dtype=torch.bool)
    ref = {}
    for k in (3, 2):
        xs, _ = O.generalized_steps(x9, ones, _seq(k),
                                    lambda a, m, t: O.gcndiff_forward(P, adj, a, m, t), _betas())
        ref[k] = xs[-1]
    return ref


def _both(model, mode, fn):
    """fn() on the 8-wave and on the 4-wave instance in GEMM mode `mode`."""
    model.set_gemm_mode(mode)
    try:
        model.set_tile_waves(8)
        o8 = fn()
        o8 = tuple(t.clone() for t in o8) if isinstance(o8, tuple) else o8.clone()
        model.set_tile_waves(4)
        o4 = fn()
        o4 = tuple(t.clone() for t in o4) if isinstance(o4, tuple) else o4.clone()
    finally:
        model.set_tile_waves(8)
        model.set_gemm_mode("fp32")
    return o8, o4


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [3, 2])
@pytest.mark.parametrize("n", [4, 3, 9])
def test_oracle_parity_and_bitwise_vs_four_waves(model, x9, oracle_finals, mode, k, n):
    """One full tile, a partial tile (the absent pose computes on zero rows and is not stored) and two full
    tiles plus a partial one: within the mode's oracle bar, and bitwise the 4-wave instance's output."""
    xd = x9[:n].contiguous().cuda()
    seq = _seq(k)
    o8, o4 = _both(model, mode, lambda: model.sample(xd, seq, _betas(), mask=_ones()))
    assert torch.isfinite(o8).all()
    assert record_delta(_maxdiff(o8, oracle_finals[k][:n]), TOL[mode])
    assert torch.equal(o8, o4), (mode, k, n, _maxdiff(o8, o4))


@pytest.mark.parametrize("mode", MODES)
def test_run_to_run_bitwise(model, x9, mode):
    xd = x9.cuda()
    seq = _seq(3)
    model.set_gemm_mode(mode)
    try:
        a = model.sample(xd, seq, _betas(), mask=_ones()).clone()
        b = model.sample(xd, seq, _betas(), mask=_ones())
        assert torch.equal(a, b)
    finally:
        model.set_gemm_mode("fp32")


@pytest.mark.parametrize("mode", MODES)
def test_per_pose_key_masks_in_one_tile(model, x9, mode):
    """Four different key masks on the four poses of one tile (the wave -> pose index at two waves per pose):
    vs the oracle with the same masks, and bitwise vs the 4-wave instance."""
    from oracle import gcndiff_oracle as O

    m = torch.ones(4, 1, 17, dtype=torch.bool)
    m[1] = False
    m[1, 0, 16] = True            # key 16 alone
    m[2] = False
    m[2, 0, [3, 9]] = True        # two MFMA keys
    m[3, 0, [0, 5, 16]] = False
    x = x9[:4].contiguous()
    seq = _seq(3)
    o8, o4 = _both(model, mode, lambda: model.sample(x.cuda(), seq, _betas(), mask=m.cuda()))
    P, adj = O.params_to_torch(synthetic_state_dict()), O.adjacency()
    xs, _ = O.generalized_steps(x, m, seq, lambda a, mm, tt: O.gcndiff_forward(P, adj, a, mm, tt), _betas())
    assert record_delta(_maxdiff(o8, xs[-1]), TOL[mode])
    assert torch.equal(o8, o4)
    if mode == "fp32":      # (the model is back in fp32 mode here)
        ones = model.sample(x.cuda(), seq, _betas(), mask=_ones())
        assert torch.equal(ones[0], o8[0])
        for p in (1, 2, 3):
            assert _maxdiff(ones[p], o8[p]) > 1e-6, p       # each pose saw its own mask


def test_dense_graph_path(x9):
    """A non-H36M adjacency (dense Chebyshev path) on 8 waves: vs the oracle and bitwise vs 4 waves."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from oracle import gcndiff_oracle as O

    edges = tuple(H36M_EDGES) + ((3, 16), (6, 13))
    sd = synthetic_state_dict()
    m = HipGCNdiff(adj_mx_from_edges(17, edges), None, device="cuda:0")
    m.load_state_dict(sd)
    m.set_tail_plan("four")
    seq = _seq(3)
    try:
        m.set_tile_waves(8)
        o8 = m.sample(x9.cuda(), seq, _betas(), mask=_ones()).clone()
        m.set_tile_waves(4)
        o4 = m.sample(x9.cuda(), seq, _betas(), mask=_ones()).clone()
    finally:
        m.close()
    P, adj = O.params_to_torch(sd), O.adjacency(17, edges)
    xs, _ = O.generalized_steps(x9, torch.ones(1, 1, 17, dtype=torch.bool), seq,
                                lambda a, mm, tt: O.gcndiff_forward(P, adj, a, mm, tt), _betas())
    assert record_delta(_maxdiff(o8, xs[-1]), TOL["fp32"])
    assert torch.equal(o8, o4)


def test_caller_noise_and_trajectories(model, x9):
    """eta > 0 with the caller's draws and with xs / x0s requested, N = 4, K = 3: vs the oracle on the same
    draws, and bitwise vs 4 waves; counter-based draws bitwise vs 4 waves too."""
    from oracle import gcndiff_oracle as O

    x = x9[:4].contiguous()
    seq = _seq(3)
    z = torch.randn(3, 4, 17, 5, generator=torch.Generator().manual_seed(4))
    (xs8, x0s8), (xs4, x0s4) = _both(
        model, "fp32", lambda: model.sample(x.cuda(), seq, _betas(), mask=_ones(), eta=0.7, trajectory=True, noise=z.cuda()))
    assert xs8.shape == (4, 4, 17, 5) and x0s8.shape == (3, 4, 17, 5)
    assert torch.equal(xs8, xs4) and torch.equal(x0s8, x0s4)
    P, adj = O.params_to_torch(synthetic_state_dict()), O.adjacency()
    rxs, rx0s = O.generalized_steps(x, torch.ones(1, 1, 17, dtype=torch.bool), seq,
                                    lambda a, m, t: O.gcndiff_forward(P, adj, a, m, t), _betas(), eta=0.7, noise=z)
    assert record_delta(_maxdiff(xs8, torch.stack(rxs)), TOL["fp32"])
    assert record_delta(_maxdiff(x0s8, torch.stack(rx0s)), TOL["fp32"])
    c8, c4 = _both(model, "fp32", lambda: model.sample(x.cuda(), seq, _betas(), mask=_ones(), eta=0.7, seed=13))
    assert torch.equal(c8, c4)
    assert _maxdiff(c8, xs8[-1]) > 1e-4       # other draws


def test_step_split_bitwise_vs_plan_four(model):
    """Plan 2 at N = 4 n_cu + 4 (one full round and one step-split tile), K = 4, both halves on 8 waves:
    bitwise plan 0's output."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n = 4 * n_cu + 4
    xd = torch.from_numpy(synthetic_batch(n, seed=3)[0]).cuda()
    seq = _seq(4)
    ref = model.sample(xd, seq, _betas(), mask=_ones()).clone()
    try:
        model.set_tail_plan("step_split")
        out = model.sample(xd, seq, _betas(), mask=_ones())
        assert torch.equal(out, ref)
    finally:
        model.set_tail_plan("four")


def test_graph_capture_replays_eager(model, x9):
    # (no mask argument: a device mask would be copied to the host, which a capture forbids; None = all keys)
    dev = torch.device("cuda", 0)
    xd = x9.cuda()
    seq = _seq(3)
    eager = model.sample(xd, seq, _betas()).clone()
    out = torch.empty_like(xd)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        model.sample(xd, seq, _betas(), out=out)
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        model.sample(xd, seq, _betas(), out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    del g


def test_bad_tile_waves_raises(model):
    with pytest.raises(ValueError):
        model.set_tile_waves(6)
