"""GPU parity of the split-fp16 GEMM mode (dpk_set_gemm_mode(h, 1), "f16x3") on the persistent-sampler
instances of the other widths: dpkw (hid 128 / 8 heads) and dpkw4 (128 / 4) on 2-pose tiles, dpkn (hid 64 / 2
heads) and dpkn4 (64 / 4) on 4-pose tiles.

The bars are those of tests/test_gpu_gemm_modes.py, which are the fp32 mode's: 5e-6 elementwise on eps and on
trajectories.  Mode 1 forms every per-layer GEMM product from fp16 hi + lo parts of both operands (three
MFMAs, fp32 accumulation), so it loses about 2^-22 per product to fp32's 2^-24; a CPU restatement of the scheme
against the fp32 oracle stays below 7.2e-7 over K = 50 steps at these four shapes (tests/test_f16x3_scheme_cpu.py,
which runs it at K = 10).  Every achieved delta goes through record_delta.
"""
from types import SimpleNamespace as ns

import pytest
import torch

from conftest import record_delta

from diffpose_amd._lib import DpkError
from diffpose_amd.data import synthetic_batch
from diffpose_amd.gcndiff import H36M_EDGES, HipGCNdiff, adj_mx_from_edges
from diffpose_amd.schedule import make_seq
from diffpose_amd.weights import synthetic_state_dict
from helpers import betas as _betas, maxdiff as _maxdiff

pytestmark = pytest.mark.gpu

TOL = 5e-6
INSTANCES = [(128, 8), (128, 4), (64, 2), (64, 4)]                       # dpkw, dpkw4, dpkn, dpkn4
GOLDENS = {(128, 8): "g12_shape_h128_n8_l5_j17.npz", (128, 4): "g12_shape_h128_n4_l3_j17.npz",
           (64, 2): "g12_shape_h64_n2_l2_j17.npz", (64, 4): "g12_shape_h64_n4_l5_j17.npz"}
# the oracle's shapes: the goldens' layer counts, and hid 64 / 2 heads at 5 layers as well
ORACLE_SHAPES = [(128, 8, 5), (128, 4, 3), (64, 2, 2), (64, 2, 5), (64, 4, 5)]
DENSE_EDGES = tuple(H36M_EDGES) + ((3, 16), (6, 13))                     # outside the compiled Chebyshev pattern
CHAIN16 = tuple((i, i + 1) for i in range(15))


def _cfg(hid, heads, layers, npts=17):
    return ns(model=ns(hid_dim=hid, emd_dim=hid, coords_dim=[5, 5], num_layer=layers, n_head=heads, dropout=0.25,
                       n_pts=npts))


def _inputs(n, seed):
    return torch.from_numpy(synthetic_batch(n, seed=seed)[0])


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _model(dev, hid, heads, layers, edges=H36M_EDGES, sd=None, mode="f16x3"):
    m = HipGCNdiff(adj_mx_from_edges(17, edges), _cfg(hid, heads, layers), device=dev)
    m.load_state_dict(sd if sd is not None else synthetic_state_dict(hid=hid, n_layers=layers))
    m.set_gemm_mode(mode)
    return m


@pytest.fixture(scope="module")
def models(dev):
    """One mode-1 model per (hid, heads, layers, dense) for the whole module, closed at its end."""
    made = {}

    def get(hid, heads, layers, dense=False):
        key = (hid, heads, layers, dense)
        if key not in made:
            made[key] = _model(dev, hid, heads, layers, DENSE_EDGES if dense else H36M_EDGES)
        return made[key]

    yield get
    for m in made.values():
        m.close()


def _oracle(hid, heads, layers, edges=H36M_EDGES):
    from oracle import gcndiff_oracle as O

    P = O.params_to_torch(synthetic_state_dict(hid=hid, n_layers=layers))
    g = O.adjacency(17, edges)
    return O, lambda a, mk, t: O.gcndiff_forward(P, g, a, mk, t, n_layers=layers, heads=heads)


# ---------------------------------------------------------------------------------------
# 1. the reference's own fixtures at these shapes, in mode 1

@pytest.mark.parametrize("hid,heads", INSTANCES)
def test_reference_goldens_f16x3(dev, models, golden, hid, heads):
    g = golden(GOLDENS[(hid, heads)])
    assert (int(g["hid"]), int(g["n_head"]), int(g["n_pts"])) == (hid, heads, 17)
    m = models(hid, heads, int(g["num_layer"]))
    x, t = torch.from_numpy(g["x"]).to(dev), torch.from_numpy(g["t8"]).to(dev)
    ones = torch.ones(1, 1, 17, dtype=torch.bool, device=dev)
    assert record_delta(_maxdiff(m(x, ones, t, 0), torch.from_numpy(g["eps"])), TOL)
    assert record_delta(_maxdiff(m(x, torch.from_numpy(g["mask2"]).to(dev), t, 0), torch.from_numpy(g["eps_masked"])), TOL)
    seq = [int(s) for s in g["seq"]]
    xs, x0s = m.sample(x, seq, _betas(int(g["T"])), mask=ones, trajectory=True)
    assert record_delta(_maxdiff(xs, torch.from_numpy(g["xs"])), TOL)
    assert record_delta(_maxdiff(x0s, torch.from_numpy(g["x0s"])), TOL)
    out = m.sample(x, seq, _betas(int(g["T"])), mask=ones)
    assert torch.equal(out, xs[-1])
    assert m.debug_resources()["generic_loop_graphs"] == 0, "expected the fused persistent-sampler instance"


# ---------------------------------------------------------------------------------------
# 2. the oracle on 24 poses (12 two-pose tiles, 6 four-pose tiles)

@pytest.mark.parametrize("hid,heads,layers", ORACLE_SHAPES)
def test_eps_vs_oracle_f16x3(dev, models, hid, heads, layers):
    """eps with per-pose t (the per-pose projection stride of the Chebyshev epilogue), then with a handle-wide
    key mask and with per-pose masks."""
    _, fwd = _oracle(hid, heads, layers)
    m = models(hid, heads, layers)
    x = _inputs(24, seed=140 + hid)
    t = torch.arange(24, dtype=torch.float32) * 2.0
    ones = torch.ones(1, 1, 17, dtype=torch.bool)
    eps = m(x.to(dev), ones.to(dev), t.to(dev), 0)
    assert eps.shape == x.shape and record_delta(_maxdiff(eps, fwd(x, ones, t)), TOL)
    mk = ones.clone()
    mk[0, 0, [0, 16]] = False
    assert record_delta(_maxdiff(m(x.to(dev), mk.to(dev), t.to(dev), 0), fwd(x, mk, t)), TOL)
    per = torch.ones(24, 1, 17, dtype=torch.bool)
    per[::3, 0, 1::2] = False
    per[1::5, 0, :16] = False
    assert record_delta(_maxdiff(m(x.to(dev), per.to(dev), t.to(dev), 0), fwd(x, per, t)), TOL)


@pytest.mark.parametrize("hid,heads,layers", ORACLE_SHAPES)
def test_k50_final_vs_oracle_f16x3(dev, models, hid, heads, layers):
    """The whole K = 50 sampler on 40 poses."""
    O, fwd = _oracle(hid, heads, layers)
    m = models(hid, heads, layers)
    x = _inputs(40, seed=150 + hid)
    ones = torch.ones(1, 1, 17, dtype=torch.bool)
    seq = make_seq("uniform", 50, 50)
    out = m.sample(x.to(dev), seq, _betas(), mask=ones.to(dev))
    rxs, _ = O.generalized_steps(x, ones, seq, fwd, _betas())
    assert record_delta(_maxdiff(out, rxs[-1]), TOL)


@pytest.mark.parametrize("hid,heads,layers", ORACLE_SHAPES)
def test_dense_graph_vs_oracle_f16x3(dev, models, hid, heads, layers):
    """An adjacency outside the compiled H36M Chebyshev pattern (the dense-graph kernels): eps with per-pose t,
    and the K = 10 trajectory with eta = 0.5 on the caller's draws."""
    O, fwd = _oracle(hid, heads, layers, DENSE_EDGES)
    m = models(hid, heads, layers, dense=True)
    x = _inputs(24, seed=160 + hid)
    t = torch.arange(24, dtype=torch.float32) * 2.0
    ones = torch.ones(1, 1, 17, dtype=torch.bool)
    assert record_delta(_maxdiff(m(x.to(dev), ones.to(dev), t.to(dev), 0), fwd(x, ones, t)), TOL)
    seq = make_seq("uniform", 50, 10)
    xs, x0s = m.sample(x.to(dev), seq, _betas(), mask=ones.to(dev), trajectory=True)
    rxs, rx0s = O.generalized_steps(x, ones, seq, fwd, _betas())
    assert record_delta(_maxdiff(xs, torch.stack(rxs)), TOL) and record_delta(_maxdiff(x0s, torch.stack(rx0s)), TOL)
    z = torch.randn((10,) + tuple(x.shape), generator=torch.Generator().manual_seed(9))
    out = m.sample(x.to(dev), seq, _betas(), eta=0.5, mask=ones.to(dev), noise=z.to(dev))
    rz, _ = O.generalized_steps(x, ones, seq, fwd, _betas(), eta=0.5, noise=z)
    assert record_delta(_maxdiff(out, rz[-1]), TOL)


@pytest.mark.parametrize("hid,heads,layers", ORACLE_SHAPES)
def test_eta_with_caller_noise_vs_oracle_f16x3(dev, models, hid, heads, layers):
    """eta = 0.5 with the caller's draws (dpk_sample_noise: the ZM = 1 kernels), K = 10 with its trajectory."""
    O, fwd = _oracle(hid, heads, layers)
    m = models(hid, heads, layers)
    x = _inputs(24, seed=170 + hid)
    ones = torch.ones(1, 1, 17, dtype=torch.bool)
    seq = make_seq("uniform", 50, 10)
    z = torch.randn((10,) + tuple(x.shape), generator=torch.Generator().manual_seed(8))
    xs, x0s = m.sample(x.to(dev), seq, _betas(), eta=0.5, mask=ones.to(dev), trajectory=True, noise=z.to(dev))
    rxs, rx0s = O.generalized_steps(x, ones, seq, fwd, _betas(), eta=0.5, noise=z)
    assert record_delta(_maxdiff(xs, torch.stack(rxs)), TOL) and record_delta(_maxdiff(x0s, torch.stack(rx0s)), TOL)


# ---------------------------------------------------------------------------------------
# 3. ragged batches: partial tiles and the padded tail tile's discarded rows, at both tile sizes

@pytest.fixture(scope="module")
def full40(dev, models):
    """The K = 10 sample of a 40-pose batch per instance, computed once and left unchanged."""
    done = {}

    def get(hid, heads):
        if (hid, heads) not in done:
            xd = _inputs(40, seed=7).to(dev)
            out = models(hid, heads, 5).sample(xd, make_seq("uniform", 50, 10), _betas()).clone()
            done[(hid, heads)] = (xd, out)
        return done[(hid, heads)]

    return get


@pytest.mark.parametrize("n", [1, 3, 5, 37])
@pytest.mark.parametrize("hid,heads", INSTANCES)
def test_ragged_batches_are_batch_invariant_f16x3(dev, models, full40, hid, heads, n):
    xd, full = full40(hid, heads)
    part = models(hid, heads, 5).sample(xd[:n].contiguous(), make_seq("uniform", 50, 10), _betas())
    assert part.shape[0] == n and torch.equal(full[:n], part)


# ---------------------------------------------------------------------------------------
# 4. the mode is engaged, repeatable and exactly restored

@pytest.mark.parametrize("hid,heads", INSTANCES)
def test_mode_is_engaged_and_switching_is_exact(dev, hid, heads):
    m = _model(dev, hid, heads, 5)
    x = _inputs(24, seed=11).to(dev)
    t = (torch.arange(24, dtype=torch.float32) * 2.0).to(dev)
    ones = torch.ones(1, 1, 17, dtype=torch.bool, device=dev)
    seq = make_seq("uniform", 50, 10)
    e1, s1 = m(x, ones, t, 0).clone(), m.sample(x, seq, _betas(), mask=ones).clone()
    assert torch.equal(m(x, ones, t, 0), e1) and torch.equal(m.sample(x, seq, _betas(), mask=ones), s1)
    m.set_gemm_mode("fp32")
    e0, s0 = m(x, ones, t, 0).clone(), m.sample(x, seq, _betas(), mask=ones).clone()
    assert not torch.equal(e0, e1) and not torch.equal(s0, s1), "mode 1 gave the fp32 kernels' bits"
    assert record_delta(_maxdiff(e0, e1), TOL) and record_delta(_maxdiff(s0, s1), TOL)
    m.set_gemm_mode("f16x3")
    assert torch.equal(m(x, ones, t, 0), e1) and torch.equal(m.sample(x, seq, _betas(), mask=ones), s1)
    m.close()


# ---------------------------------------------------------------------------------------
# 5. under a caller's capture

def test_capture_replays_bitwise_f16x3(dev):
    """hid 128 / 4 heads in mode 1 inside torch.cuda.graph, after the uncaptured warm-up that sizes the capture's
    scratch for these instances' per-call timestep projections: replays equal eager bitwise."""
    m = _model(dev, 128, 4, 2)
    ones = torch.ones(1, 1, 17, dtype=torch.bool, device=dev)
    x = _inputs(30, seed=92).to(dev)
    t = (torch.arange(30, dtype=torch.float32) * 1.5).to(dev)
    seq = make_seq("uniform", 50, 5)
    eager = m.sample(x, seq, _betas(), mask=ones).clone()
    eps_eager = m(x, ones, t, 0).clone()
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        m.sample(x, seq, _betas(), mask=ones)
        m(x, ones, t, 0)
    torch.cuda.current_stream(dev).wait_stream(s)
    out, eps = torch.empty_like(x), torch.empty_like(x)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        m.sample(x, seq, _betas(), mask=ones, out=out)
        eps.copy_(m(x, ones, t, 0))
    for _ in range(2):
        out.zero_()
        eps.zero_()
        g.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(out, eager) and torch.equal(eps, eps_eager)
    del g
    m.close()


# ---------------------------------------------------------------------------------------
# 6. refusals and the mode query

@pytest.mark.parametrize("hid,heads", INSTANCES)
def test_out_of_range_weight_is_refused_in_mode_1(dev, hid, heads):
    sd = synthetic_state_dict(hid=hid, n_layers=2)
    key = "atten_layers.1.self_attn.linears.1.weight"
    sd[key] = sd[key].copy()
    sd[key][3, 5] = 2000.0
    m = _model(dev, hid, heads, 2, sd=sd, mode="fp32")
    x = _inputs(6, seed=1).to(dev)
    t = torch.full((6,), 10.0, device=dev)
    ones = torch.ones(1, 1, 17, dtype=torch.bool, device=dev)
    e0 = m(x, ones, t, 0)
    assert torch.isfinite(e0).all()
    m.set_gemm_mode("f16x3")
    with pytest.raises(DpkError, match="DPK_E_UNSUPPORTED.*split-fp16"):
        m(x, ones, t, 0)
    with pytest.raises(DpkError, match="DPK_E_UNSUPPORTED.*split-fp16"):
        m.sample(x, make_seq("uniform", 50, 3), _betas(), mask=ones)
    m.set_gemm_mode("fp32")
    assert torch.equal(m(x, ones, t, 0), e0)
    m.close()


@pytest.mark.parametrize("hid,heads", INSTANCES)
def test_bf16_is_refused_naming_mode_and_shape(dev, models, hid, heads):
    m = models(hid, heads, 5)
    x = _inputs(6, seed=1).to(dev)
    t = torch.full((6,), 10.0, device=dev)
    ones = torch.ones(1, 1, 17, dtype=torch.bool, device=dev)
    m.set_gemm_mode("bf16")                  # accepted at the set, refused at the call
    try:
        for call in (lambda: m(x, ones, t, 0), lambda: m.sample(x, make_seq("uniform", 50, 3), _betas(), mask=ones)):
            with pytest.raises(DpkError, match=rf"DPK_E_UNSUPPORTED.*gemm mode 2 \(bf16\).*hid {hid} / {heads} heads") as ei:
                call()
            assert ei.value.code == -2
    finally:
        m.set_gemm_mode("f16x3")
    assert torch.isfinite(m(x, ones, t, 0)).all()


def test_per_op_handle_refuses_mode_1(dev):
    m = HipGCNdiff(adj_mx_from_edges(16, CHAIN16), _cfg(48, 4, 1, 16), device=dev)
    m.load_state_dict(synthetic_state_dict(hid=48, n_layers=1, n_pts=16))
    x = _inputs(6, seed=1)[:, :16].contiguous().to(dev)
    t = torch.full((6,), 10.0, device=dev)
    ones = torch.ones(1, 1, 16, dtype=torch.bool, device=dev)
    assert m.gemm_modes() == 0b001
    m.set_gemm_mode("f16x3")
    with pytest.raises(DpkError, match=r"DPK_E_UNSUPPORTED.*gemm mode 1 \(f16x3\).*hid 48 / 4 heads / 16 joints"):
        m(x, ones, t, 0)
    m.set_gemm_mode("fp32")
    assert torch.isfinite(m(x, ones, t, 0)).all()
    m.close()


def test_gemm_modes_query(dev, models):
    for hid, heads in INSTANCES:
        assert models(hid, heads, 5).gemm_modes() == 0b011
    shipped = HipGCNdiff(adj_mx_from_edges(), None, device=dev)
    assert shipped.gemm_modes() == 0b111
    shipped.close()
