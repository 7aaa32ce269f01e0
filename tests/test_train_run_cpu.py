"""CPU: the training run, ``runner.Diffpose.train`` (runners/diffpose_frame.py:156-268), without a GPU: the restated
draw rule of dpk_train_draws, the package's seed words, and — with tests/train_run_cases.py's stand-ins for the device
part of a step, the optimiser and the dataset — the loop, the learning-rate schedule, the reference's checkpoint list
and the resume."""
import os

import numpy as np
import pytest
import torch

import counter_draws as C
import train_run_cases as TC
from diffpose_amd import _lib
from diffpose_amd.schedule import train_epoch_permutation, train_step_seeds, word
from diffpose_amd.weights import load_checkpoint, param_shapes


# ---------------------------------------------------------------------------------------
# 1. the draw rule and the seed words

def test_t_rule_range_pairs_and_coverage():
    T, batch = 51, 1024
    h = batch // 2 + 1
    for seed in C.SEEDS:
        t = TC.t_rule(seed, T, batch)
        assert t.dtype == np.int64 and t.shape == (batch,) and t.min() >= 0 and t.max() <= T - 1
        pairs = batch - h
        assert np.array_equal(t[:pairs] + t[h:], np.full(pairs, T - 1))
        counts = np.bincount(t, minlength=T)
        assert counts.min() >= 9, (seed, counts.min())         # every timestep occurs; the rarest 9 times or more
        # a shard's rows are the batch's rows
        assert np.array_equal(TC.t_rule(seed, T, batch, 300, 411), t[300:711])


@pytest.mark.parametrize("T,batch", TC.T_EDGES)
def test_t_rule_edge_shapes(T, batch):
    h = batch // 2 + 1
    assert 2 * h > batch
    for seed in C.SEEDS:
        t = TC.t_rule(seed, T, batch)
        assert t.shape == (batch,) and t.min() >= 0 and t.max() <= T - 1
        assert np.array_equal(t[:batch - h] + t[h:], np.full(batch - h, T - 1))
        # the first h entries are the draws themselves: the top 32 bits of the word, scaled
        w = C.counter_word(seed, np.arange(min(h, batch)))
        assert [int(v) for v in t[:h]] == [((int(x) >> 32) * T) >> 32 for x in w]
    if T == 1:
        assert not TC.t_rule(7, T, batch).any()


def test_word_is_counter_word():
    counters = [0, 1] + [4 * s + k for s in (1, 2, 9, 10 ** 6) for k in range(4)] + [2 ** 62 + ep for ep in (0, 1, 59)]
    for seed in C.SEEDS + (-1, TC.RUN_SEED):
        want = C.counter_word(seed, np.array(counters, dtype=np.uint64))
        assert [word(seed, c) for c in counters] == [int(v) for v in want]
    assert train_step_seeds(TC.RUN_SEED, 5) == tuple(word(TC.RUN_SEED, 20 + k) for k in range(4))
    p = train_epoch_permutation(TC.RUN_SEED, 2, TC.FRAMES)
    g = torch.Generator().manual_seed(word(TC.RUN_SEED, 2 ** 62 + 2) & (2 ** 63 - 1))
    assert torch.equal(p, torch.randperm(TC.FRAMES, generator=g)) and sorted(p.tolist()) == list(range(TC.FRAMES))
    assert not torch.equal(p, train_epoch_permutation(TC.RUN_SEED, 1, TC.FRAMES))


def test_library_refuses_before_any_device_call():
    """dpk_train_draws' refusals need no device (the library loads without one); version 105 exports it"""
    L = _lib.lib()
    assert L.dpk_version() >= 105
    ok = dict(T=51, batch=8, pose0=2, n=3, pf=85)
    one = 1                                                # any non-NULL address: a refused call touches nothing
    for bad in (dict(T=0), dict(T=(1 << 24) + 1), dict(batch=0), dict(pose0=-1), dict(n=-1), dict(pose0=6),
                dict(pf=0)):
        a = dict(ok, **bad)
        assert L.dpk_train_draws(1, 2, a["T"], a["batch"], a["pose0"], a["n"], a["pf"], one, one, None) == -1, bad
    assert L.dpk_train_draws(1, 2, 51, 8, 2, 3, 85, None, None, None) == -1
    assert L.dpk_train_draws(1, 2, 51, 8, 2, 0, 85, None, None, None) == 0        # n = 0 touches nothing
    assert L.dpk_train_draws(1, 2, 51, 8, 8, 0, 85, one, one, None) == 0


# ---------------------------------------------------------------------------------------
# 2. and 3.: the run on stand-ins

def _runner(tmp, ema=True, n_epochs=TC.EPOCHS):
    from diffpose_amd import runner as R
    import diff_grad_cases as GC

    cfg = TC.run_config(GC.CASES["h96"][0], ema=ema, n_epochs=n_epochs)
    args = R.default_args(seed=TC.RUN_SEED, log_path=str(tmp))
    return R.Diffpose(args, cfg, device="cpu")


def _train(tmp, ema=True, n_epochs=TC.EPOCHS, resume=None, calls=None):
    r = _runner(tmp, ema, n_epochs)
    opt, data = TC.StubAdam(ema=ema), TC.StubData()
    out = r.train(data, eval_batches=lambda: TC.eval_batches(), resume=resume, optimizer=opt,
                  step_grads=TC.stub_step_grads(opt.total, calls), frame_errors=TC.stub_frame_errors)
    return r, opt, data, out


@pytest.mark.parametrize("ema", [True, False])
def test_checkpoint_format(tmp_path, ema):
    calls = []
    r, opt, data, (best_epoch, best_p1) = _train(tmp_path, ema=ema, calls=calls)
    assert data.checks == TC.EPOCHS and opt.step_count == TC.EPOCHS * TC.STEPS_PER_EPOCH
    assert (r.best_epoch, r.best_p1) == (best_epoch, best_p1) and 0 < best_p1 < 1000
    # the batches: every epoch is a permutation of the frames in 8 + 8 + 7, the seeds follow the global step
    for ep in range(TC.EPOCHS):
        mine = calls[ep * 3:ep * 3 + 3]
        assert [c[3] for c in mine] == [8, 8, 7] and [(c[1], c[2]) for c in mine] == [(0, 8), (0, 8), (0, 7)]
        assert sum((c[0] for c in mine), []) == train_epoch_permutation(TC.RUN_SEED, ep, TC.FRAMES).tolist()
        assert [c[4] for c in mine] == [train_step_seeds(TC.RUN_SEED, ep * 3 + i + 1) for i in range(3)]
    shapes = param_shapes(hid=96, n_layers=2, n_pts=17)
    for epoch in range(TC.EPOCHS):
        path = os.path.join(tmp_path, f"ckpt_{epoch}.pth")
        states = torch.load(path, weights_only=True)
        assert isinstance(states, list) and len(states) == (5 if ema else 4)
        assert list(states[0]) == ["module." + k for k in shapes]
        assert all(tuple(states[0]["module." + k].shape) == tuple(s) and not states[0]["module." + k].is_cuda
                   for k, s in shapes.items())
        sd = load_checkpoint(path, kind="diff", n_layers=2)
        assert list(sd) == list(shapes)
        ps = [torch.nn.Parameter(torch.zeros(s)) for s in shapes.values()]
        adam = torch.optim.Adam(ps, lr=1.0)
        adam.load_state_dict(states[1])
        assert adam.param_groups[0]["lr"] == states[1]["param_groups"][0]["lr"] == TC.lr_after(epoch)
        assert torch.equal(adam.state[ps[3]]["exp_avg"], states[1]["state"][3]["exp_avg"])
        assert states[2:4] == [epoch, (epoch + 1) * TC.STEPS_PER_EPOCH]
        if ema:
            assert list(states[4]) == list(shapes)
    last = torch.load(os.path.join(tmp_path, "ckpt.pth"), weights_only=True)
    assert TC.states_equal(last, torch.load(os.path.join(tmp_path, f"ckpt_{TC.EPOCHS - 1}.pth"), weights_only=True))
    # the learning rate each step ran with: the initial one through epoch 0 (decayed by gamma^0), gamma^1 after epoch 2
    assert opt.lrs == [TC.LR] * 9 and opt.param_groups[0]["lr"] == TC.LR * TC.GAMMA
    # the epoch's loss: the AverageMeter over update(batch mean, B) of the stand-in's integers
    perm = train_epoch_permutation(TC.RUN_SEED, TC.EPOCHS - 1, TC.FRAMES).tolist()
    assert r.epoch_loss_diff == pytest.approx(sum(3 + f % 4 for f in perm) / TC.FRAMES, rel=1e-15)
    assert [e["epoch"] for e in r.train_log] == [0, 1, 2]


def test_resume_continues_the_run(tmp_path):
    a_dir, b_dir = tmp_path / "a", tmp_path / "b"
    ra, oa, _, out_a = _train(a_dir)
    _train(b_dir, n_epochs=1)
    rb, ob, _, out_b = _train(b_dir, resume=os.path.join(b_dir, "ckpt_0.pth"))
    assert ob.step_count == oa.step_count == 9
    for k in ("params", "exp_avg", "exp_avg_sq", "ema"):
        assert torch.equal(getattr(oa, k), getattr(ob, k)), k
    assert oa.lrs[3:] == ob.lrs and [e["lr"] for e in ra.train_log[1:]] == [e["lr"] for e in rb.train_log]
    assert [e["loss_diff"] for e in ra.train_log[1:]] == [e["loss_diff"] for e in rb.train_log]
    sa = torch.load(os.path.join(a_dir, "ckpt_2.pth"), weights_only=True)
    sb = torch.load(os.path.join(b_dir, "ckpt_2.pth"), weights_only=True)
    assert TC.states_equal(sa, sb) and sa[2:4] == [2, 9]
    # best_p1 restarts at 1000 on a resume: the best of epochs 1.. only
    assert out_b == min(((e["epoch"], e["p1"]) for e in rb.train_log), key=lambda v: v[1])
    assert out_a == min(((e["epoch"], e["p1"]) for e in ra.train_log), key=lambda v: v[1])
