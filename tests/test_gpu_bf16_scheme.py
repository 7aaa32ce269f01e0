"""GPU: gemm mode 2 (bf16) against a restatement of its own arithmetic (tests/bf16_scheme.py, forward_bf16 with
float64 accumulation), at hid 96 / 4 heads: does the kernel compute what include/diffpose_kernels.h and
DESIGN.md 3.1 / 4.2 say it computes?  The 5-layer study (tests/test_gpu_bf16_tolerance.py) says how far bf16 is
from fp32; a kernel that lost the L_g lo term, rounded joint 16's graph row, left the probabilities unrounded or
truncated its weights would pass there (all within 2.5e-2) and fails here.

The statistic is S = the median over poses of the per-pose max |gpu - restatement| on 1-layer models: the
kernel and the restatement differ by fp32 rounding and summation order, which now and then moves an activation
across a bf16 rounding boundary, after which that pose rounds independently downstream.  The median ignores
that minority and sees anything systematic.  Depth comes back by silencing: a 5-layer state dict with the output
projections of all layers but i zeroed is the 1-layer model of layer i exactly, run through layer i's slot of
the bf16 arena, the fp32 arena, the L_g tables and the timestep projections; its GPU output must equal the
1-layer handle's bitwise.

Per case:  S <= B (so at least half of the poses are within B), and every pose within 2 x own, own = max
|restatement - fp32 oracle| (a flipped pose is the restatement with some roundings taken independently).
B = sqrt(noise x nearest), both from the restatement alone (tests/test_bf16_scheme_cpu.py computes them and
checks each literal below against [10 noise, nearest / 10]; sample/K2, whose second evaluation starts from the
first one's flips, against [3.2 noise, nearest / 3.2]): noise is what fp32 rounding does to S, nearest the
smallest S of a deliberate departure from the scheme.  No bar was read off the kernel.  The regime cases use the
relative form (every figure divided by max(1, max |restatement|)); regimes x10, plus5, bias+10_ch0 and
refinit_x10 are left out because nearest / noise is 5.5, 5.8, 77 and 1.9 there (bf16_scheme.DROPPED_REGIMES).
Each S goes through conftest.record_delta (tag bf16_scheme/<case>).

Cases: dpk_eps on 64 poses (2-pose tiles, 4 waves) for each layer's weights as a 1-layer model and as the solo
layer of a 5-layer one, a handle mask without keys {0, 16}, per-pose masks (key 16 off, one key kept, none kept),
the reference's initialisers, a non-H36M adjacency (the dense Chebyshev path: in mode 2 it changes the fp32
Chebyshev products only, so the restatement is the same with the other graph) and three input regimes;
dpk_sample at K = 1 and K = 2 on 67 poses as 4-pose tiles (16 and a 3-pose tail) on 8 and on 4 waves, bitwise
equal to each other, and as the default plan's 2-pose tiles; dpk_pose on a 1-layer GCNpose.
"""
import functools
from types import SimpleNamespace as ns

import pytest
import torch

import bf16_scheme as B
from conftest import record_delta
from diffpose_amd._lib import DpkError
from diffpose_amd.gcndiff import HipGCNdiff
from diffpose_amd.gcnpose import HipGCNpose
from diffpose_amd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu

# case: (B, noise, nearest) from tests/bf16_scheme.py's figures(case); B = sqrt(noise x nearest)
BARS = {
    "one/0": (2.1e-5, 9.83e-7, 4.35e-4),
    "one/1": (2.0e-5, 9.54e-7, 4.16e-4),
    "one/2": (2.6e-5, 1.31e-6, 5.01e-4),
    "one/3": (9.5e-6, 1.97e-7, 4.58e-4),
    "one/4": (9.3e-6, 2.38e-7, 3.61e-4),
    "mask_handle": (1.9e-5, 8.64e-7, 4.06e-4),
    "mask_pose": (1.5e-5, 5.07e-7, 4.26e-4),
    "refinit": (5.0e-6, 1.19e-7, 2.13e-4),
    "dense": (1.1e-5, 2.38e-7, 4.65e-4),
    "regime/baseline": (2.1e-5, 9.83e-7, 4.35e-4),
    "regime/zeros": (1.1e-5, 5.07e-7, 2.20e-4),
    "regime/joints_equal": (9.5e-6, 2.01e-7, 4.53e-4),
    "sample/K1": (1.6e-6, 5.96e-8, 4.06e-5),
    "sample/K2": (1.5e-5, 3.22e-6, 6.79e-5),
    "pose": (2.3e-5, 1.40e-6, 3.77e-4),
}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _cfg(layers, coords=(5, 5)):
    return ns(model=ns(hid_dim=96, num_layer=layers, n_head=B.HEADS, n_pts=17, coords_dim=list(coords)))


def _eps(dev, name, sd=None, layers=1):
    """dpk_eps of a case in bf16 mode on a handle of its own; ``sd``: another state dict on the case's inputs."""
    c = B.case(name)
    m = HipGCNdiff(c["adj"], _cfg(layers), device=dev)
    try:
        m.load_state_dict(c["sd"] if sd is None else sd)
        m.set_gemm_mode("bf16")
        return m(c["x"].to(dev), c["mask"].to(dev), c["t"].to(dev), 0).cpu()
    except DpkError as e:          # a library / HIP error is no parity miss: run nothing more on the device
        pytest.exit(f"bf16_scheme/{name}: {e}", returncode=3)
    finally:
        m.close()


@functools.lru_cache(maxsize=None)
def _eps_one(dev, i):
    return _eps(dev, f"one/{i}")


def _check(name, gpu, tag=None):
    """S <= B through record_delta, at least half of the poses within B, every pose within 2 own."""
    ref, own = B.reference(name)
    bar, sc = BARS[name][0], B.scale(name)
    assert gpu.shape == ref.shape and bool(torch.isfinite(gpu).all()), name
    pp = B.per_pose(gpu, ref, B.pose_dim(name))
    s, within, worst = float(pp.median()) / sc, float((pp / sc <= bar).double().mean()), float(pp.max())
    print(f"{tag or name}: S {s:.3e}  B {bar:.3e}  poses within B {within:.2f}  worst pose {worst:.3e}  2 own {2 * own:.3e}")
    assert record_delta(s, bar, f"bf16_scheme/{tag or name}")
    assert within >= 0.5
    assert worst <= 2.0 * own


@pytest.mark.parametrize("i", range(5))
def test_each_layers_weights_as_a_one_layer_model(dev, i):
    _check(f"one/{i}", _eps_one(dev, i))


@pytest.mark.parametrize("i", range(5))
def test_solo_layer_of_five_is_the_one_layer_model(dev, i):
    """Layer i alone live in a 5-layer handle: every per-layer table read at slot i."""
    gpu = _eps(dev, f"one/{i}", sd=B.solo_layer_state_dict(synthetic_state_dict(), i), layers=5)
    assert torch.equal(gpu, _eps_one(dev, i))
    _check(f"one/{i}", gpu, tag=f"solo/{i}")


@pytest.mark.parametrize("name", ["mask_handle", "mask_pose"])
def test_masks(dev, name):
    _check(name, _eps(dev, name))


def test_reference_initialisers(dev):
    _check("refinit", _eps(dev, "refinit"))


def test_dense_graph_path(dev):
    _check("dense", _eps(dev, "dense"))


@pytest.mark.parametrize("regime", B.REGIMES)
def test_input_regimes(dev, regime):
    _check(f"regime/{regime}", _eps(dev, f"regime/{regime}"))


@pytest.mark.parametrize("k", [1, 2])
def test_sample_on_both_tile_instances(dev, k):
    """x0s and the final of dpk_sample: 4-pose tiles on 8 and on 4 waves (bitwise equal), then the default
    plan, which runs 67 poses as 2-pose tiles (fp32 rounding apart from the 4-pose tiles: S alone)."""
    name = f"sample/K{k}"
    c = B.case(name)
    m = HipGCNdiff(c["adj"], _cfg(1), device=dev)
    try:
        m.load_state_dict(c["sd"])
        m.set_gemm_mode("bf16")
        x, mask = c["x"].to(dev), c["mask"].to(dev)

        def run():
            xs, x0s = m.sample(x, c["seq"], c["betas"], mask=mask, trajectory=True)
            assert torch.equal(xs[0], x)
            return torch.cat([x0s, xs[-1:]]).cpu()

        m.set_tail_plan("four")
        m.set_tile_waves(8)
        o8 = run()
        m.set_tile_waves(4)
        o4 = run()
        m.set_tail_plan("step_split")
        m.set_tile_waves(0)
        o2 = run()
    except DpkError as e:
        pytest.exit(f"bf16_scheme/{name}: {e}", returncode=3)
    finally:
        m.close()
    assert torch.equal(o8, o4)
    _check(name, o8, tag=f"{name}/w8")
    _check(name, o4, tag=f"{name}/w4")
    _check(name, o2, tag=f"{name}/two_pose")


def test_gcnpose_one_layer(dev):
    """dpk_pose runs mode 2 on the hid-96 instance (dpk_gemm_modes 0b111): the backbone without the timestep input."""
    c = B.case("pose")
    m = HipGCNpose(c["adj"], _cfg(1, (2, 3)), device=dev)
    try:
        m.load_state_dict(c["sd"])
        assert m.gemm_modes() == 0b111
        m.set_gemm_mode("bf16")
        xyz = m(c["x"].to(dev), c["mask"].to(dev)).cpu()
    except DpkError as e:
        pytest.exit(f"bf16_scheme/pose: {e}", returncode=3)
    finally:
        m.close()
    _check("pose", xyz)
