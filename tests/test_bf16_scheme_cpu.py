"""CPU: where the bars of tests/test_gpu_bf16_scheme.py come from, and that they tell gemm mode 2's documented
arithmetic from its neighbours.  tests/bf16_scheme.py restates the mode in torch; for every case the GPU file
runs, with S(a, b) the median over poses of the per-pose max |a - b| and ref = forward_bf16(acc=float64):
  noise    the larger of S(forward_bf16(acc=float32), ref) and S(forward_bf16 with each layer's input times
           (1 + 1e-6 z), ref): what fp32 rounding and summation order alone do to the statistic;
  nearest  the minimum over the departures (bf16_scheme.DEPARTS) of S(forward_bf16(depart=d), ref);
  own      max |ref - fp32 oracle|.
Asserted per case: nearest / noise >= 100; own > 0 (another arithmetic than the oracle's); no noise variant has
more than half of its poses beyond sqrt(noise x nearest); and the literal bar of the GPU file lies within
[10 noise, nearest / 10].  The figures are printed (pytest -s).  The cases tests/sampler_cells.py adds for the
kernel table (bf16_scheme.KERNEL_CASES) are re-measured under the same conditions, with their bars there.

sample/K2 is the exception the two-step cascade makes: a pose that met a rounding flip in the first evaluation
enters the second with another input, so about 45 % of the poses of the 1e-6 variant are off and its median
sits at the edge of that minority (noise 3.2e-6 against 6e-8 at K = 1, nearest 6.8e-5: ratio 21).  Its bar is
derived by the same rule, sqrt(noise x nearest), which then lies sqrt(21) = 4.6 from either side; the CPU
conditions for it are ratio >= 10 and the literal within [sqrt(10) noise, nearest / sqrt(10)].

Also here: a 5-layer state dict with all but layer i silenced (solo_layer_state_dict) gives bitwise the 1-layer
model of layer i, through forward_bf16 and through the fp32 oracle, which is what lets the GPU file reach every
layer slot of the per-layer tables with a 1-layer bar.
"""
import math

import pytest
import torch

import bf16_scheme as B
from diffpose_amd.weights import synthetic_state_dict
from oracle import gcndiff_oracle as O
from test_gpu_bf16_scheme import BARS

RATIO = {"sample/K2": 10.0}       # every other case: 100


@pytest.fixture(autouse=True, scope="module")
def _threads():
    torch.set_num_threads(max(1, min(8, torch.get_num_threads())))


def test_every_gpu_case_has_a_bar():
    assert set(BARS) == set(B.ALL_CASES)
    assert BARS["sample/K2"][0] > BARS["sample/K1"][0]


@pytest.mark.parametrize("name", B.ALL_CASES)
def test_bar_separates_the_scheme_from_its_neighbours(name):
    noise, nearest, own, beyond, dep = B.figures(name)
    bar = BARS[name][0]
    print(f"{name}: noise {noise:.3e}  nearest {nearest:.3e}  ratio {nearest / noise:.0f}  own {own:.3e}  "
          f"bar {bar:.3e}  noise poses beyond sqrt(noise nearest) {beyond:.2f}")
    print("    " + "  ".join(f"{d} {v:.2e}" for d, v in dep.items()))
    need = RATIO.get(name, 100.0)
    assert nearest / noise >= need
    assert own > 0.0
    assert beyond <= 0.5
    m = math.sqrt(need)
    assert m * noise <= bar <= nearest / m
    for (case, d), why in B.BLIND.items():
        if case == name:
            assert 0.0 < dep[d] < 100.0 * noise, (d, dep[d], why)


@pytest.mark.parametrize("name", B.KERNEL_CASES)
def test_kernel_table_cases_are_remeasured(name):
    """The cases tests/sampler_cells.py adds for the bf16 kernels no case above reaches (bf16_scheme.KERNEL_CASES):
    one with a bar (BF16_BARS) meets the conditions above (the two-step sample/K2 cases those of sample/K2); one
    recorded as dropped (BF16_DROPPED) still has no bar, like the dropped regimes below."""
    from sampler_cells import BF16_BARS, BF16_DROPPED, BF16_NEED

    noise, nearest, own, beyond, _ = B.figures(name)
    need = BF16_NEED.get(name, RATIO["sample/K2"])
    print(f"{name}: noise {noise:.3e}  nearest {nearest:.3e}  ratio {nearest / noise:.1f}  need {need:.0f}  own {own:.3e}  "
          f"noise poses beyond sqrt(noise nearest) {beyond:.2f}")
    assert own > 0.0
    assert (name in BF16_BARS) != (name in BF16_DROPPED)
    if name in BF16_DROPPED:
        assert nearest / noise < need       # once this fails the case belongs in sampler_cells.BF16_BARS
        return
    assert nearest / noise >= need
    assert beyond <= 0.5
    m = math.sqrt(need)
    assert m * noise <= BF16_BARS[name][0] <= nearest / m


@pytest.mark.parametrize("regime", sorted(B.DROPPED_REGIMES))
def test_dropped_regimes_have_no_bar(regime):
    noise, nearest, _, _, _ = B.figures("regime/" + regime)
    print(f"regime/{regime}: noise {noise:.3e}  nearest {nearest:.3e}  ratio {nearest / noise:.1f}")
    assert nearest / noise < 100.0      # once this fails the regime belongs in bf16_scheme.REGIMES


@pytest.mark.parametrize("i", range(5))
def test_a_silenced_layer_is_the_identity_bitwise(i):
    sd5 = synthetic_state_dict()
    solo = O.params_to_torch(B.solo_layer_state_dict(sd5, i))
    one = O.params_to_torch(B.one_layer_state_dict(sd5, i))
    g, ones = O.adjacency(), torch.ones(1, 1, 17, dtype=torch.bool)
    x, t = B.eps_inputs()
    with torch.no_grad():
        assert torch.equal(B.forward_bf16(solo, g, x, ones, t, 5, B.HEADS), B.forward_bf16(one, g, x, ones, t, 1, B.HEADS))
        assert torch.equal(B.forward_bf16(one, g, x, ones, t, 1, B.HEADS), B.reference(f"one/{i}")[0])
        assert torch.equal(O.gcndiff_forward(solo, g, x, ones, t, 5, B.HEADS), O.gcndiff_forward(one, g, x, ones, t, 1, B.HEADS))
    for j in range(5):                  # the silencing touches nothing of layer i and nothing but the projections
        for k, v in B.solo_layer_state_dict(sd5, i).items():
            if f"_layers.{j}." in k:
                same = bool((v == sd5[k]).all())
                assert same == (j == i or not any(k == s.format(j) for s in B._SILENCED)), k
