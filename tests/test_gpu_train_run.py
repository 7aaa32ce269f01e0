"""GPU: the training run, ``runner.Diffpose.train`` (runners/diffpose_frame.py:156-268), and the wait-free batch path
``PoseGeneratorGMM.batch_device``, on the small run of tests/train_run_cases.py (23 frames, batches of 8, 3 epochs,
decay 2, evaluation on 6 frames with 2 timesteps).  The run is compared bitwise with a loop written out here from
calls that have tests of their own; a resumed run with the uninterrupted one; the shards of a step with the gradient's
existing bars against the float64 autograd model (tests/diff_grad_cases.py); and the run under an initialised RCCL
job of one rank with the plain one."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import diff_grad_cases as GC
import diff_loss_cases as LC
import train_run_cases as TC
from conftest import record_delta
from diffpose_amd import _lib
from diffpose_amd._lib import DpkError
from diffpose_amd.gmm import PoseGeneratorGMM
from diffpose_amd.schedule import word
from helpers import free_port as _free_port

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
ARRAYS = ("params", "exp_avg", "exp_avg_sq", "ema")
# case name -> the args flag of train_step's dropout rule
RUNS = {"g16": dict(train_dropout=True), "h96": dict(train_without_dropout=True)}


def ends_session(fn):
    """A library / HIP error is no parity miss: run nothing more on the device."""
    @functools.wraps(fn)
    def run(*a, **k):
        try:
            return fn(*a, **k)
        except DpkError as e:
            pytest.exit(f"train_run/{fn.__name__}: {e}", returncode=3)
        except RuntimeError as e:
            if "HIP error" in str(e) or "hipError" in str(e):
                pytest.exit(f"train_run/{fn.__name__}: {e}", returncode=3)
            raise
    return run


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def data17(dev):
    return PoseGeneratorGMM(*TC.dataset_arrays(17, np.float32), device=dev)


def _runner(name, dev, log_path, n_epochs=TC.EPOCHS):
    from diffpose_amd.runner import Diffpose, default_args

    cfg = TC.run_config(GC.CASES[name][0], n_epochs=n_epochs)
    r = Diffpose(default_args(seed=TC.RUN_SEED, log_path=str(log_path), **RUNS[name]), cfg, device=dev)
    r.create_diffusion_model(state_dict=GC.inputs(name)["sd"])
    r.create_pose_model()
    return r


def _state(opt):
    out = {k: opt._get(k)[0].clone() for k in ARRAYS}
    out["step_count"] = opt.step_count
    return out


def _train(name, dev, data, log_path, n_epochs=TC.EPOCHS, resume=None):
    """one ``train`` on a fresh runner: (arrays, train_log, (best_epoch, best_p1))"""
    r = _runner(name, dev, log_path, n_epochs)
    try:
        out = r.train(data, eval_batches=lambda: TC.eval_batches(), resume=resume)
        opt = r.model_diff._trainer
        assert opt is not None and (r.best_epoch, r.best_p1) == out
        return _state(opt), r.train_log, out
    finally:
        r.model_diff.close()
        r.model_pose.close()


@pytest.fixture(scope="module")
def runs(dev, data17, tmp_path_factory):
    """the uninterrupted 3-epoch run of each case, made once: name -> (arrays, train_log, out, log dir)"""
    made = {}

    def get(name):
        if name not in made:
            d = tmp_path_factory.mktemp(f"run_{name}")
            made[name] = _train(name, dev, data17, d) + (d,)
        return made[name]

    return get


# ---------------------------------------------------------------------------------------
# 9. batch_device

@pytest.mark.parametrize("joints,dtype", [(17, np.float32), (16, np.float64)])
@ends_session
def test_batch_device_is_batch(dev, joints, dtype):
    ds = PoseGeneratorGMM(*TC.dataset_arrays(joints, dtype), device=dev)
    for idx, seed in (([3, 0, 22, 7, 7, 45, -1], 11), (list(range(TC.FRAMES)), (1 << 63) + 5), ([4], 0)):
        uv, ns = ds.batch(idx, seed=seed)[:2]
        uv_d, ns_d = ds.batch_device(torch.tensor(idx, dtype=torch.int64, device=dev), seed)
        assert uv_d.shape == (len(idx), joints, 5) and torch.equal(uv_d, uv) and torch.equal(ns_d, ns), (idx, seed)
    ds.check_status()                                            # nothing to raise
    uv_d, ns_d = ds.batch_device(torch.empty(0, dtype=torch.int64, device=dev), 3)
    assert uv_d.shape == (0, joints, 5) and ns_d.shape == (0, joints, 5)
    with pytest.raises(ValueError, match="int64"):
        ds.batch_device(torch.tensor([1, 2], dtype=torch.int32, device=dev), 3)


@ends_session
def test_check_status_raises_what_batch_raises(dev):
    p3, gmm, acts, cam = TC.dataset_arrays(17, np.float32)
    neg = [g.copy() for g in gmm]
    neg[0][2, 5, 0, 0] = -0.25
    off = [g.copy() for g in gmm]
    off[1][1, 3, 1, 0] += 0.5
    for arrays, text, frame in ((neg, "not non-negative", 2), (off, "do not sum to 1", TC.FRAMES // 2 + 1)):
        ds = PoseGeneratorGMM(p3, arrays, acts, cam, device=dev)
        with pytest.raises(ValueError, match=text):
            ds.batch([frame], seed=1)
        ds.batch_device(torch.tensor([frame], dtype=torch.int64, device=dev), 1)
        ds.batch_device(torch.tensor([0, 9], dtype=torch.int64, device=dev), 2)      # a clean call keeps the flag
        with pytest.raises(ValueError, match=text):
            ds.check_status()
        ds.check_status()                                        # read and cleared
        ds.batch_device(torch.tensor([0, 9], dtype=torch.int64, device=dev), 2)
        ds.check_status()


# ---------------------------------------------------------------------------------------
# 10. the run is its parts, bitwise

def _draws(dev, e_seed, t_seed, T, B, J):
    e = torch.empty(B, J, 5, dtype=torch.float32, device=dev)
    t = torch.empty(B, dtype=torch.float32, device=dev)
    rc = _lib.lib().dpk_train_draws(ctypes.c_uint64(e_seed & M64), ctypes.c_uint64(t_seed & M64), T, B, 0, B, J * 5,
                                    e.data_ptr(), t.data_ptr(), None)
    assert rc == 0
    return e, t


def _written_out(name, dev, data, log_path):
    """the run as a loop of its parts: (arrays, [epoch_loss_diff])"""
    r = _runner(name, dev, log_path)
    m, cfg, seed = r.model_diff, r.config, TC.RUN_SEED
    try:
        opt = m.device_optimizer(cfg)
        betas = r.betas.cpu().numpy()
        drop = dict(dropout=True) if RUNS[name].get("train_dropout") else {}
        step, losses = 0, []
        for ep in range(TC.EPOCHS):
            g = torch.Generator().manual_seed(word(seed, 2 ** 62 + ep) & (2 ** 63 - 1))
            perm = torch.randperm(len(data), generator=g)
            total = count = 0.0
            for i in range(TC.STEPS_PER_EPOCH):
                step += 1
                rows = perm[i * TC.BATCH:(i + 1) * TC.BATCH]
                B = rows.numel()
                uvxyz, scale = data.batch(rows.numpy(), seed=word(seed, 4 * step))[:2]
                e, t = _draws(dev, word(seed, 4 * step + 1), word(seed, 4 * step + 2), r.num_timesteps, B, r.n_pts)
                if drop:
                    drop["dropout_seed"] = word(seed, 4 * step + 3)
                loss, grads = m.diffusion_loss_grad(uvxyz, t, betas, noise_scale=scale, noise=e, mask=r.src_mask,
                                                    weight=1.0 / B, **drop)
                opt.step(grads.flat)
                total += float(loss.sum(dtype=torch.float64)) / B * B      # AverageMeter.update(batch mean, B)
                count += B
            losses.append(total / count)
            if ep % TC.DECAY == 0:
                opt.param_groups[0]["lr"] = TC.LR * TC.GAMMA ** (ep / TC.DECAY)
        return _state(opt), losses
    finally:
        m.close()
        r.model_pose.close()


@pytest.mark.parametrize("name", list(RUNS))
@ends_session
def test_run_is_its_parts(dev, data17, runs, tmp_path, name):
    got, log, out, log_dir = runs(name)
    want, losses = _written_out(name, dev, data17, tmp_path)
    assert got["step_count"] == want["step_count"] == TC.EPOCHS * TC.STEPS_PER_EPOCH == 9
    for k in ARRAYS:
        assert torch.equal(got[k], want[k]), (name, k)
    assert [e["loss_diff"] for e in log] == losses
    assert [e["lr"] for e in log] == [TC.lr_after(ep) for ep in range(TC.EPOCHS)]
    assert all(np.isfinite(e["p1"]) and e["p1"] > 0 for e in log) and 0 < out[1] < 1000
    # the steps moved the parameters, and the files hold these arrays
    initial = GC.inputs(name)["sd"]
    r = _runner(name, dev, tmp_path)
    try:
        layout, total = r.model_diff.param_layout()
    finally:
        r.model_diff.close()
        r.model_pose.close()
    states = torch.load(os.path.join(log_dir, "ckpt_2.pth"), weights_only=True)
    assert len(states) == 5 and states[2:4] == [2, 9]
    moved = 0
    for i, (k, off, num) in enumerate(layout):
        assert torch.equal(states[0]["module." + k].reshape(-1), got["params"][off:off + num].cpu()), k
        assert torch.equal(states[4][k].reshape(-1), got["ema"][off:off + num].cpu()), k
        assert torch.equal(states[1]["state"][i]["exp_avg"].reshape(-1), got["exp_avg"][off:off + num].cpu()), k
        assert torch.equal(states[1]["state"][i]["exp_avg_sq"].reshape(-1), got["exp_avg_sq"][off:off + num].cpu()), k
        moved += int(not np.array_equal(states[0]["module." + k].numpy(), np.asarray(initial[k], dtype=np.float32)))
    assert moved > len(layout) // 2
    assert states[1]["param_groups"][0]["lr"] == TC.lr_after(2)
    assert sorted(os.listdir(log_dir)) == sorted(["ckpt.pth"] + [f"ckpt_{e}.pth" for e in range(TC.EPOCHS)])


# ---------------------------------------------------------------------------------------
# 11. resume on the device

@ends_session
def test_resume_on_the_device(dev, data17, runs, tmp_path):
    full, log, out, _ = runs("g16")
    _train("g16", dev, data17, tmp_path, n_epochs=1)
    got, log_b, out_b = _train("g16", dev, data17, tmp_path, resume=os.path.join(tmp_path, "ckpt_0.pth"))
    assert got["step_count"] == full["step_count"] == 9
    for k in ARRAYS:
        assert torch.equal(got[k], full[k]), k
    assert log_b == log[1:]
    # best_p1 restarts at 1000 on a resume: the best of epochs 1.. of the uninterrupted run
    best = min(log[1:], key=lambda e: e["p1"])
    assert out_b == (best["epoch"], best["p1"])


# ---------------------------------------------------------------------------------------
# 12. shards add up to the batch

@ends_session
def test_shards_add_up(dev, data17, tmp_path):
    from diffpose_amd.schedule import train_epoch_permutation, train_step_seeds

    name = "g16"
    r = _runner(name, dev, tmp_path)
    m = r.model_diff
    try:
        rows = train_epoch_permutation(TC.RUN_SEED, 0, TC.FRAMES)[:TC.BATCH].to(dev)
        seeds = train_step_seeds(TC.RUN_SEED, 1)
        B = TC.BATCH
        whole_loss, whole = r._step_grads(data17, rows, 0, B, B, seeds, False)
        whole = whole.clone()
        e, t = r.train_draws(seeds[1], seeds[2], B)
        total = torch.zeros_like(whole)
        loss_sum = 0.0
        for lo, hi in ((0, 3), (3, B)):
            es, ts = r.train_draws(seeds[1], seeds[2], B, lo, hi)
            assert torch.equal(es, e[lo:hi]) and torch.equal(ts, t[lo:hi])
            ls, flat = r._step_grads(data17, rows, lo, hi, B, seeds, False)
            total += flat
            loss_sum += float(ls)
        # the step's own inputs, read back: the float64 autograd model and its bars at them
        uvxyz, scale = data17.batch_device(rows, seeds[0])
        x0, sc, e_h, t_h = uvxyz.cpu(), scale.cpu(), e.cpu(), t.cpu()
        base = GC.inputs(name)
        betas = r.betas.cpu()
        i = dict(sd=base["sd"], adj=base["adj"], layers=base["layers"], heads=base["heads"], x0=x0, e=e_h, scale=sc,
                 t=t_h, betas=betas, mask=base["mask"], x_t=LC.x_t_ref(x0, e_h, sc, t_h, betas),
                 target=LC.target_ref(e_h, sc))
        ref = GC.references(i)                                   # weight None: the batch mean, 1 / B
        layout, _ = m.param_layout()
        ok = True
        for tag, flat in (("shards", total), ("whole", whole)):
            for k, off, num in layout:
                got = flat[off:off + num].cpu().double().view(ref["g64"][k].shape)
                ok = record_delta(float((got - ref["g64"][k]).abs().max()), ref["bar"][k],
                                  f"train_run/shards_add_up/{tag}/{k}") and ok
        assert ok
        want = float(ref["loss64"].sum())
        assert abs(loss_sum - want) <= float(ref["loss_bar"].sum()) and abs(float(whole_loss) - want) <= float(ref["loss_bar"].sum())
    finally:
        m.close()
        r.model_pose.close()


# ---------------------------------------------------------------------------------------
# 13. RCCL at world size 1

_RCCL = r"""
import tempfile, numpy as np, torch, torch.distributed as dist
import diff_grad_cases as GC, train_run_cases as TC
from diffpose_amd.gmm import PoseGeneratorGMM
from diffpose_amd.runner import Diffpose, default_args
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
data = PoseGeneratorGMM(*TC.dataset_arrays(17, np.float32), device=dev)

def run():
    with tempfile.TemporaryDirectory() as d:
        cfg = TC.run_config(GC.CASES["g16"][0], n_epochs=2)
        r = Diffpose(default_args(seed=TC.RUN_SEED, log_path=d, train_dropout=True), cfg, device=dev)
        r.create_diffusion_model(state_dict=GC.inputs("g16")["sd"])
        r.create_pose_model()
        out = r.train(data, eval_batches=lambda: TC.eval_batches())
        opt = r.model_diff._trainer
        arrays = [opt._get(k)[0].cpu() for k in ("params", "exp_avg", "exp_avg_sq", "ema")]
        res = (out, r.train_log, opt.step_count, r._world())
        r.model_diff.close(); r.model_pose.close()
        return arrays, res

plain_a, plain = run()
assert plain[3] == (1, 0, False) and plain[2] == 6
dist.init_process_group("nccl", device_id=dev)
got_a, got = run()                                  # the distributed path: both all-reduces run over RCCL
assert got[3] == (1, 0, True)
assert got[:3] == plain[:3], (got[:3], plain[:3])
assert all(torch.equal(a, b) for a, b in zip(got_a, plain_a))
dist.barrier()
dist.destroy_process_group()
print("TRAIN_RCCL_OK", plain[0])
"""


def test_train_over_rccl_world1_equals_plain_run():
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "diffpose-nw_amd"), ROOT, os.path.join(ROOT, "tests"),
                                         env.get("PYTHONPATH", "")])
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    r = subprocess.run([sys.executable, "-c", _RCCL], cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "TRAIN_RCCL_OK" in r.stdout
