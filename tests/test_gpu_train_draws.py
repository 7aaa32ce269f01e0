"""GPU: dpk_train_draws, the draws of one training step as functions of (seed, global index): known answers against
the numpy restatement (tests/train_run_cases.py on tests/counter_draws.py: e inside counter_draws.draw_bar(r, 0) per
element, the derived bar of that module; t exact), shard invariance and equality with the loss calls' internal draw
(both bitwise), the caller-memory contract through guard words (tests/caller_memory.py), every refusal, and a
captured call."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import caller_memory as CM
import counter_draws as C
import diff_grad_cases as GC
import dropout_cases as DC
import train_run_cases as TC
from conftest import record_delta
from diffpose_amd import _lib
from diffpose_amd._lib import DpkError
from diffpose_amd.data import shard_frames
from diffpose_amd.gcndiff import HipGCNdiff, adj_mx_from_edges

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
T_SEED = (1 << 44) + 77
BIG_POSE0 = 50529027                  # x 85 = 2^32 - 1: the call's elements straddle the counter's second word


def ends_session(fn):
    """A library / HIP error is no parity miss: run nothing more on the device."""
    @functools.wraps(fn)
    def run(*a, **k):
        try:
            return fn(*a, **k)
        except DpkError as e:
            pytest.exit(f"train_draws/{fn.__name__}: {e}", returncode=3)
        except RuntimeError as e:
            if "HIP error" in str(e) or "hipError" in str(e):
                pytest.exit(f"train_draws/{fn.__name__}: {e}", returncode=3)
            raise
    return run


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _raw(e_seed, t_seed, T, batch, pose0, n, pf, e_ptr, t_ptr, stream=None):
    return _lib.lib().dpk_train_draws(ctypes.c_uint64(e_seed & M64), ctypes.c_uint64(t_seed & M64), T, batch, pose0, n,
                                      pf, e_ptr, t_ptr, stream)


def _draw(dev, e_seed, t_seed, T, batch, pose0, n, pf):
    e = torch.empty(n * pf, dtype=torch.float32, device=dev)
    t = torch.empty(n, dtype=torch.float32, device=dev)
    rc = _raw(e_seed, t_seed, T, batch, pose0, n, pf, e.data_ptr(), t.data_ptr())
    if rc:
        raise DpkError("dpk_train_draws", rc)
    return e, t


# ---------------------------------------------------------------------------------------
# 5. known answers

@pytest.mark.parametrize("pf", [85, 80])
@ends_session
def test_e_known_answers(dev, pf):
    n = 37
    ok = True
    for seed in C.SEEDS:
        for pose0, batch in ((0, n), (5, n + 9)):
            e, _ = _draw(dev, seed, T_SEED, 51, batch, pose0, n, pf)
            z, r = TC.e_ref(seed, pose0, n, pf)
            ratio = np.abs(e.cpu().numpy().astype(np.float64) - z) / C.draw_bar(r, 0.0)
            ok = record_delta(float(ratio.max()), 1.0, f"train_draws/e/pf{pf}/seed{seed}/pose0_{pose0}") and ok
    assert ok


@ends_session
def test_e_across_the_second_counter_word(dev):
    pf, n = 85, 2
    assert BIG_POSE0 * pf == (1 << 32) - 1
    e, t = _draw(dev, C.SEED_C, T_SEED, 51, BIG_POSE0 + n, BIG_POSE0, n, pf)
    z, r = TC.e_ref(C.SEED_C, BIG_POSE0, n, pf)
    ratio = np.abs(e.cpu().numpy().astype(np.float64) - z) / C.draw_bar(r, 0.0)
    assert record_delta(float(ratio.max()), 1.0, "train_draws/e/across_2^32")
    # a counter whose second word is dropped would repeat the draws of elements 0.. from the second element on
    low, _ = TC.e_ref(C.SEED_C, 0, n, pf)
    assert np.abs(e.cpu().numpy()[1:] - low[:n * pf - 1]).max() > 1.0
    assert np.array_equal(t.cpu().numpy().astype(np.int64), TC.t_rule(T_SEED, 51, BIG_POSE0 + n, BIG_POSE0, n))


@pytest.mark.parametrize("T,batch", [(51, 37), (51, 1024), (1, 5), (2, 2)])
@ends_session
def test_t_exact(dev, T, batch):
    for seed in C.SEEDS:
        _, t = _draw(dev, 3, seed, T, batch, 0, batch, 85)
        got = t.cpu().numpy()
        assert np.array_equal(got, TC.t_rule(seed, T, batch).astype(np.float32)), (seed, T, batch)
        assert got.min() >= 0 and got.max() <= T - 1


# ---------------------------------------------------------------------------------------
# 6. shard invariance, bitwise

@ends_session
def test_shards_are_slices_of_the_batch(dev):
    pf = 85
    for batch, shards in ((5, DC.G17_SHARDS), (37, tuple(shard_frames(37, 3, r) for r in range(3)))):
        e, t = _draw(dev, C.SEED_C, T_SEED, 51, batch, 0, batch, pf)
        assert [s[0] for s in shards] + [shards[-1][1]] == sorted({v for s in shards for v in s})
        for lo, hi in shards:
            es, ts = _draw(dev, C.SEED_C, T_SEED, 51, batch, lo, hi - lo, pf)
            assert torch.equal(es, e[lo * pf:hi * pf]) and torch.equal(ts, t[lo:hi]), (batch, lo, hi)


# ---------------------------------------------------------------------------------------
# 7. equality with the internal draw, bitwise

@pytest.fixture(scope="module")
def models(dev):
    made = {}

    def get(name):
        if name not in made:
            shape = GC.CASES[name][0]
            m = HipGCNdiff(adj_mx_from_edges(shape[3], shape[4]), TC.run_config(shape), device=dev)
            m.load_state_dict(GC.inputs(name)["sd"])
            made[name] = m
        return made[name]

    yield get
    for m in made.values():
        m.close()


@pytest.mark.parametrize("name", ["g16", "h96", "pad15"])
@ends_session
def test_equals_the_internal_draw(dev, models, name):
    m, i = models(name), GC.inputs(name)
    n, J = i["x0"].shape[0], i["x0"].shape[1]
    x0, sc = i["x0"].to(dev), i["scale"].to(dev)
    for seed in (C.SEED_C, C.SEEDS[-1]):
        e, _ = _draw(dev, seed, T_SEED, 51, n, 0, n, J * 5)
        e = e.view(n, J, 5)
        loss_a, xt_a, _ = m.diffusion_loss(x0, i["t"], i["betas"], noise_scale=sc, noise=None, seed=seed,
                                           return_parts=True)
        loss_b, xt_b, _ = m.diffusion_loss(x0, i["t"], i["betas"], noise_scale=sc, noise=e, seed=seed + 1,
                                           return_parts=True)
        assert torch.equal(xt_a, xt_b) and torch.equal(loss_a, loss_b), (name, seed)
        la, ga = m.diffusion_loss_grad(x0, i["t"], i["betas"], noise_scale=sc, noise=None, seed=seed)
        lb, gb = m.diffusion_loss_grad(x0, i["t"], i["betas"], noise_scale=sc, noise=e, seed=seed + 1)
        assert torch.equal(ga.flat, gb.flat) and torch.equal(la, lb), (name, seed)
    assert bool(xt_a.isfinite().all()) and not torch.equal(xt_a, x0)


# ---------------------------------------------------------------------------------------
# 8. caller memory and refusals

def _arrays(dev, n, pf, role="out", null_e=False, null_t=False):
    e = CM.Guarded("e", (n * pf,), device=dev, role=role, misaligned=True, null=null_e)
    t = CM.Guarded("t", (n,), device=dev, role=role, misaligned=True, null=null_t)
    assert all(a.alignment() == 4 for a in (e, t) if not a.null)
    return e, t


@ends_session
def test_caller_memory(dev):
    n, pf, batch, pose0 = 37, 85, 50, 6
    want_e, want_t = _draw(dev, C.SEED_C, T_SEED, 51, batch, pose0, n, pf)
    for tag, null_e, null_t in (("full", False, False), ("null_e", True, False), ("null_t", False, True)):
        e, t = _arrays(dev, n, pf, null_e=null_e, null_t=null_t)
        assert _raw(C.SEED_C, T_SEED, 51, batch, pose0, n, pf, e.ptr, t.ptr) == 0
        CM.check([e, t], {"e": want_e, "t": want_t}, tag=f"train_draws/memory/{tag}")
    # one pose, one float per pose: the smallest extents
    e, t = _arrays(dev, 1, 1)
    assert _raw(C.SEED_C, T_SEED, 51, 1, 0, 1, 1, e.ptr, t.ptr) == 0
    w1, t1 = _draw(dev, C.SEED_C, T_SEED, 51, 1, 0, 1, 1)
    CM.check([e, t], {"e": w1, "t": t1}, tag="train_draws/memory/one")
    # n = 0 touches nothing, with pointers or without
    e, t = _arrays(dev, n, pf, role="untouched")
    assert _raw(C.SEED_C, T_SEED, 51, batch, pose0, 0, pf, e.ptr, t.ptr) == 0
    assert _raw(C.SEED_C, T_SEED, 51, batch, batch, 0, pf, e.ptr, t.ptr) == 0
    assert _raw(C.SEED_C, T_SEED, 51, batch, pose0, 0, pf, None, None) == 0
    CM.check([e, t], tag="train_draws/memory/n0")


@ends_session
def test_refusals_write_nothing(dev):
    n, pf, batch, pose0 = 5, 85, 8, 2
    e, t = _arrays(dev, n, pf, role="untouched")
    ok = dict(T=51, batch=batch, pose0=pose0, n=n, pf=pf)
    for bad in (dict(T=0), dict(T=-3), dict(T=(1 << 24) + 1), dict(batch=0), dict(batch=-1), dict(pose0=-1),
                dict(n=-1), dict(pose0=4), dict(n=7), dict(pf=0), dict(pf=-85)):
        a = dict(ok, **bad)
        assert _raw(1, 2, a["T"], a["batch"], a["pose0"], a["n"], a["pf"], e.ptr, t.ptr) == -1, bad
    assert _raw(1, 2, 51, batch, pose0, n, pf, None, None) == -1
    CM.check([e, t], tag="train_draws/refusals")
    # the largest T is taken
    _, tt = _draw(dev, 1, 2, 1 << 24, batch, 0, batch, 1)
    assert np.array_equal(tt.cpu().numpy(), TC.t_rule(2, 1 << 24, batch).astype(np.float32))


@ends_session
def test_captured_call_replays_to_the_same_bits(dev):
    n, pf, batch, pose0 = 37, 85, 50, 6
    want_e, want_t = _draw(dev, C.SEED_C, T_SEED, 51, batch, pose0, n, pf)
    e = torch.zeros(n * pf, dtype=torch.float32, device=dev)
    t = torch.zeros(n, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = _raw(C.SEED_C, T_SEED, 51, batch, pose0, n, pf, e.data_ptr(), t.data_ptr(),
                  torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    for _ in range(2):
        e.zero_()
        t.zero_()
        g.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(e, want_e) and torch.equal(t, want_t)
    del g
