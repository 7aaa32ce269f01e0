"""CPU: the checker of tests/caller_memory.py finds each way a kernel can break the caller-memory contract.

A torch stand-in for an entry point (out = 2 x + noise, slice by slice) runs on Guarded arrays on the CPU, once
correctly and once with each sin planted; the checker must report the sin, naming the array and the kind, and
nothing else.  This is the evidence that tests/test_gpu_caller_memory.py would fail on a subtly wrong kernel,
gathered without asking a GPU to go wrong.  The case table and the inputs of the handle-free cases are checked
here too: the tile arithmetic each row's name promises, and that the oracle accepts the GMM weights.
"""
import numpy as np
import pytest
import torch

import caller_memory as CM

N, J = 5, 17
TILE = 4 * J * 5


def _arrays(misaligned=False, null_xs=False):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, J, 5, generator=g)
    z = torch.randn(2, N, J, 5, generator=g)
    kw = dict(tile=TILE, misaligned=misaligned)
    a = dict(x=CM.Guarded("x", x.shape, role="in", data=x, **kw),
             noise=CM.Guarded("noise", z.shape, role="in", data=z, slices=2, **kw),
             out=CM.Guarded("out", x.shape, **kw),
             xs=CM.Guarded("xs", z.shape, slices=2, null=null_xs, **kw),
             index=CM.Guarded("index", (N,), dtype=torch.int64, role="in", data=torch.arange(N) - 2, **kw),
             p1=CM.Guarded("p1", (N,), dtype=torch.float64, **kw),
             status=CM.Guarded("status", (1,), dtype=torch.int32, **kw))
    return a, x, z


def _stand_in(a, sin=None):
    """the correct call, then at most one planted violation"""
    x, z = a["x"].view(), a["noise"].view()
    a["out"].view().copy_(2 * x + z[1])
    if not a["xs"].null:
        a["xs"].view().copy_(2 * x.unsqueeze(0) + z)
    a["p1"].view().copy_(x.double().sum(dim=(1, 2)))
    a["status"].view().zero_()
    o = a["out"]
    if sin == "before":
        o.buf[o.pre - 1] = 1.0
    elif sin == "after":
        a["xs"].buf[a["xs"].pre + a["xs"].numel] = 1.0
    elif sin == "unwritten":
        o.raw[o.pre + o.numel - 1] = o.pattern              # the last pose's last element: as torch.empty left it
    elif sin == "input":
        a["noise"].body[7] += 1.0
    elif sin == "guard-read":
        # the last pose's sum runs one element past the end of x (a float NaN widened to double keeps no bits of
        # the double pattern; one that reached a float output unchanged would read as "unwritten": both fail)
        a["p1"].body[N - 1] = a["p1"].body[N - 1] + a["x"].buf[a["x"].pre + a["x"].numel].double()
    elif sin == "nan-over-guard":
        a["p1"].buf[a["p1"].pre + a["p1"].numel + 1] = float("nan")
    elif sin == "int-guard":
        a["status"].buf[a["status"].pre + 1] = 0
    elif sin == "null":
        a["xs"].buf[a["xs"].pre + 3] = 0.5
    elif sin == "value":
        o.body[11] = torch.nextafter(o.body[11], torch.tensor(float("inf")))


def _expected(x, z):
    return dict(out=2 * x + z[1], xs=2 * x.unsqueeze(0) + z, p1=x.double().sum(dim=(1, 2)),
                status=torch.zeros(1, dtype=torch.int32))


@pytest.mark.parametrize("misaligned", [False, True])
def test_a_correct_stand_in_passes(misaligned):
    a, x, z = _arrays(misaligned)
    _stand_in(a)
    bad, _ = CM.violations(a.values(), _expected(x, z))
    assert bad == []
    CM.check(list(a.values()), _expected(x, z), tag="clean")
    for g in a.values():
        assert g.alignment() == g.itemsize if misaligned else g.alignment() >= 64, (g.name, g.alignment())
        assert g.post >= 64


SINS = [("before", "out", "guard-before"), ("after", "xs", "guard-after"), ("unwritten", "out", "unwritten"),
        ("input", "noise", "input-modified"), ("guard-read", "p1", "poisoned"),
        ("nan-over-guard", "p1", "guard-after"), ("int-guard", "status", "guard-after"), ("value", "out", "mismatch")]


@pytest.mark.parametrize("sin,array,kind", SINS, ids=[s[0] for s in SINS])
def test_each_planted_violation_is_reported_by_name(sin, array, kind):
    a, x, z = _arrays()
    _stand_in(a, sin)
    bad, _ = CM.violations(a.values(), _expected(x, z))
    assert [(v.array, v.kind) for v in bad] == [(array, kind)], bad
    with pytest.raises(AssertionError, match=f"{array}: {kind}"):
        CM.check(list(a.values()), _expected(x, z), tag=sin)


def test_every_kind_of_violation_is_planted_somewhere():
    assert {k for _, _, k in SINS} | {"touched"} == set(CM.VIOLATION_KINDS)


def test_a_null_output_must_stay_untouched():
    a, x, z = _arrays(null_xs=True)
    assert a["xs"].ptr is None
    _stand_in(a)
    assert CM.violations(a.values(), _expected(x, z))[0] == []
    _stand_in(a, "null")
    bad, _ = CM.violations(a.values(), _expected(x, z))
    assert [(v.array, v.kind) for v in bad] == [("xs", "touched")]


def test_a_bar_admits_rounding_and_nothing_more():
    a, x, z = _arrays()
    _stand_in(a, "value")
    want = _expected(x, z)
    want["out"] = (want["out"], 5e-6)
    bad, deltas = CM.violations(a.values(), want)
    assert bad == [] and 0 < deltas["out"][0] <= 5e-6
    a["out"].body[11] += 1e-3
    bad, _ = CM.violations(a.values(), want)
    assert [(v.array, v.kind) for v in bad] == [("out", "mismatch")]
    a["out"].body[11] = float("nan")                      # a NaN is no small difference
    kinds = {v.kind for v in CM.violations(a.values(), want)[0]}
    assert kinds == {"poisoned"}


def test_an_in_place_array_is_an_output():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(N, J, 5, generator=g)
    io = CM.Guarded("x", x.shape, role="inout", data=x, tile=TILE)
    io.view().mul_(2)
    assert CM.violations([io, io], {"x": 2 * x})[0] == []
    assert [v.kind for v in CM.violations([io], {"x": x})[0]] == ["mismatch"]


def test_the_patterns_are_what_the_contract_says():
    f = CM.Guarded("f", (3,), device="cpu")
    d = CM.Guarded("d", (3,), dtype=torch.float64)
    assert bool(torch.isnan(f.buf).all()) and bool(torch.isnan(d.buf).all())
    assert int(f.raw[0]) == 0x7FC0DEAD and int(d.raw[0]) == 0x7FF8DEADDEADBEEF
    assert int(CM.Guarded("i", (3,), dtype=torch.int64).raw[0]) & 0xFFFFFFFF == 0xDEADBEEF
    m = CM.Guarded("m", (3,), dtype=torch.int32, pattern=-1)
    assert int(m.raw[-1]) == -1 and m.post == 64


def test_the_case_table():
    """each row's pose count reaches the tiles its name promises on a 256-CU device, and on a smaller one"""
    for cu in (256, 64):
        tiles = lambda name: -(-CM.n_poses(CM.ROWS[name], cu) // 4)  # noqa: E731
        assert CM.n_poses(CM.ROWS["four"], cu) == 5 and tiles("four") == 2
        assert CM.n_poses(CM.ROWS["mixed"], cu) == 4 * cu + 3              # a full round, then 3 poses <= 2 CU
        for name in ("split", "split8", "splitfb"):
            q, r = divmod(tiles(name), cu)
            assert (q, r) == (1, 2) and 2 * r <= cu and CM.n_poses(CM.ROWS[name], cu) % 4 == 1
    assert set(CM.INPLACE_ROWS) | set(CM.UPDATE_ROWS) <= set(CM.ROWS)
    assert [CM.scale_rows(n) for n in (3, 5, 7, 1027, 1029, 259, 261)] == [1, 1, 1, 13, 3, 7, 3]
    for n, j in ((5, 17), (7, 16), (1029, 17)):
        m = CM.pose_masks(n, j)
        assert m.shape == (n, 1, j) and m.sum(-1).min() >= j - 2 and not m.all(-1).any()


@pytest.mark.parametrize("joints", CM.GMM_JOINTS)
@pytest.mark.parametrize("kernel_n", CM.GMM_KERNELS)
def test_the_oracle_accepts_the_gmm_weights(joints, kernel_n):
    """the Dirichlet draws of PCG64(5), rounded to float32 for that entry point, pass numpy's sum-to-1 test, and
    the index wraps both ways"""
    inp = CM.gmm_inputs(joints, kernel_n)
    assert inp["index"].min() < 0 and inp["index"].max() >= CM.GMM_SRC
    for dtype in (np.float32, np.float64):
        uv, ns = CM.gmm_expected(inp, dtype)
        assert uv.shape == ns.shape == (CM.GMM_F, joints, 5) and uv.dtype == np.float32
        assert np.isfinite(uv).all() and (ns[..., 2:] == 1).all()
    assert (CM.GMM_F * joints) % 256 != 0
