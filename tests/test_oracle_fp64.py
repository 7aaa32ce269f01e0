"""CPU: the float64 mode of the oracle (params_to_torch / adjacency with dtype=torch.float64, x and
betas cast to double), the checker of tests/test_gpu_input_regimes.py.

* It reproduces the reference's own double-precision K=50 finals (``out64`` of goldens g9 seed 0 / 1
  and g10) within 2e-7: measured 3.4e-8 .. 6.5e-8 (what remains is the reference's fp32 Chebyshev
  tables and timestep embedding), 3x margin, and still 5x under the reference's own fp32-vs-fp64
  gap there (1.1e-6 .. 1.3e-6).
* On the baseline regime its gap to the float32 oracle is that of two precisions of one model.
* The degenerate poses the metrics kernel is tested on are valid inputs of the SVD oracle.
"""
import numpy as np
import pytest
import torch

import edge_inputs as E
from oracle import gcndiff_oracle as O
from oracle import metrics_oracle as M
from diffpose_amd.weights import reference_init_state_dict, synthetic_state_dict


def _weights(name):
    if name.startswith("g9_refinit_seed"):
        return reference_init_state_dict(int(name[len("g9_refinit_seed"):].split(".")[0]))
    return synthetic_state_dict(seed=7)


@pytest.mark.parametrize("name", ["g9_refinit_seed0.npz", "g9_refinit_seed1.npz", "g10_synth_seed7.npz"])
def test_fp64_oracle_vs_reference_double_finals(golden, name):
    g = golden(name)
    P, graph = O.params_to_torch(_weights(name), torch.float64), O.adjacency(dtype=torch.float64)
    assert all(v.dtype == torch.float64 for v in P.values()) and graph.dtype == torch.float64
    fn = lambda xt, m, tt: O.gcndiff_forward(P, graph, xt, m, tt)  # noqa: E731
    xs, _ = O.generalized_steps(torch.from_numpy(g["x"]).double(), torch.ones(1, 1, 17, dtype=torch.bool),
                                [int(s) for s in g["seq"]], fn, E.betas(int(g["T"])).double())
    assert xs[-1].dtype == torch.float64
    d = float(np.abs(xs[-1].numpy() - g["out64"]).max())
    print(f"{name}: max|oracle64 - out64| = {d:.3e}")
    assert d <= 2e-7


def test_float32_default_is_unchanged():
    sd = synthetic_state_dict()
    P = O.params_to_torch(sd)
    assert all(v.dtype == torch.float32 and np.array_equal(v.numpy(), sd[k]) for k, v in P.items())
    assert O.adjacency().dtype == torch.float32
    assert torch.equal(O.adjacency(dtype=torch.float64), O.adjacency().double())


def test_oracle_gap_on_baseline():
    """g of eps and of the final lies in [1e-7, 3e-6].  (Intermediate xs / x0s carry one more term, printed
    here: sqrt(1 - abar) near abar = 1 from the float32 alpha table against the float64 one, relative
    3e-4 on a coefficient of 0.01; it cancels in the final, whose last two steps apply it with
    opposite signs.)"""
    o = E.diff_oracles("baseline")
    for k, (o32, o64, g) in o.items():
        assert o32.dtype == torch.float32 and o64.dtype == torch.float64
        print(f"baseline {k}: g = {g:.3e}")
    g_eps = o["eps"][2]
    g_final = float((o["xs"][0][-1].double() - o["xs"][1][-1]).abs().max())
    print(f"baseline final: g = {g_final:.3e}")
    assert 1e-7 <= g_eps <= 3e-6 and 1e-7 <= g_final <= 3e-6, (g_eps, g_final)


def test_every_regime_is_finite_in_both_oracles():
    """The regimes are inputs the model is conditioned on: both oracles are finite on all of them, so a
    non-finite GPU output is the kernel's."""
    for shape, names in ((E.COMPILED, E.REGIMES), (E.WIDE, E.SHAPE_REGIMES), (E.NARROW, E.SHAPE_REGIMES),
                         (E.PER_OP, E.SHAPE_REGIMES)):
        for name in names:
            for k, (o32, o64, g) in E.diff_oracles(name, shape).items():
                assert torch.isfinite(o32).all() and torch.isfinite(o64).all(), (shape[:2], name, k)


def test_gcnpose_fp64():
    for name in E.POSE_REGIMES:
        for k, (o32, o64, g) in E.pose_oracles(name).items():
            assert o64.dtype == torch.float64 and torch.isfinite(o64).all() and torch.isfinite(o32).all()
            print(f"gcnpose {name} {k}: g = {g:.3e}")
            if name == "baseline":
                assert 0 < g < 5e-6


def test_metrics_edge_inputs_in_the_svd_oracle():
    pred, tgt = E.metrics_edge_inputs()
    assert pred.shape == tgt.shape == (70, 17, 3) and pred.dtype == np.float32
    p2 = M.p_mpjpe_per_pose(pred.astype(np.float64), tgt.astype(np.float64))
    assert np.isfinite(p2).all()
    case = np.arange(70) % len(E.METRICS_CASES)
    by = {n: p2[case == i] for i, n in enumerate(E.METRICS_CASES)}
    print({n: float(v.max()) for n, v in by.items()})
    assert by["equal"].max() < 1e-12 and by["rot180_z"].max() < 1e-12
    assert by["similarity"].max() < 1e-6          # exact but for the float32 rounding of the inputs
    assert by["mirror_z"].min() > 0.1 and by["mirror_x_noise"].min() > 0.1
