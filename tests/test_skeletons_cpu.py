"""CPU: skeletons other than 17 joints around the sampler — the oracles against the reference's own
results at 16 and 21 joints (golden g13, tools/gen_goldens_skeletons.py), the three ``_n`` entry points of
the C ABI (exported, and refusing before any device call), the synthetic batches, the per-action
accounting on another action list, and ``runner.Diffpose`` at ``n_pts = 16`` (constructor check, and the
frame-sharded ``test_hyber`` over gloo with a per-frame stand-in for the kernels, bit-equal to one process).
"""
import hashlib
import json
import os
import re
import subprocess
from types import SimpleNamespace as ns

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import GOLDEN
from helpers import free_port as _free_port

from diffpose_amd import _lib, metrics
from diffpose_amd.data import synthetic_batch, synthetic_eval_batches
from diffpose_amd.gmm import numpy_atol

NEW = ("dpk_pose_metrics_n", "dpk_gmm_sample_n", "dpk_gmm_sample_f64_n")
CHAIN16 = [(i, i + 1) for i in range(15)]
WORLD = 2


# ---- the oracles on g13 -------------------------------------------------------------------------
def test_g13_files_are_the_recorded_ones():
    meta = json.load(open(os.path.join(GOLDEN, "meta_g13.json")))
    assert sorted(meta["sha256"]) == ["g13_gmm_j16.npz", "g13_metrics_j16.npz", "g13_metrics_j21.npz"]
    for name, sha in meta["sha256"].items():
        assert hashlib.sha256(open(os.path.join(GOLDEN, name), "rb").read()).hexdigest() == sha, name


@pytest.mark.parametrize("J", [16, 21])
def test_oracle_metrics_match_reference_g13(golden, J):
    """As tests/test_metrics_cpu.py::test_oracle_metrics_match_reference on g7: equal, not close."""
    from oracle import metrics_oracle as M

    g = golden(f"g13_metrics_j{J}.npz")
    pred, tgt = g["pred"], g["tgt"]
    assert pred.shape == (24, J, 3)
    assert np.array_equal(M.p_mpjpe_per_pose(pred.copy(), tgt.copy()), g["per_pose_p2"])
    assert np.array_equal(M.mpjpe_per_pose(torch.from_numpy(pred), torch.from_numpy(tgt)).numpy(), g["per_pose_p1"])
    assert M.p_mpjpe(pred.copy(), tgt.copy()) == g["loss_p2"]
    assert M.mpjpe(torch.from_numpy(pred), torch.from_numpy(tgt)).item() == g["loss_p1"]


@pytest.mark.parametrize("tag", ["", "_f64"])
def test_oracle_gmm_items_match_reference_g13(golden, tag):
    """As tests/test_gmm_cpu.py::test_gmm_items_match_reference_golden on g8, from float32 and float64 arrays."""
    from oracle import gmm_oracle as G

    g = golden("g13_gmm_j16.npz")
    gmm = g["gmm" + tag]
    assert gmm.shape == (6, 16, 5, 5) and gmm.dtype == (np.float64 if tag else np.float32)
    p3 = g["poses_3d" + tag].copy()
    p3 = p3 - p3[:, :1]
    atol = numpy_atol(gmm.dtype)
    for n, idx in enumerate(g["indices"]):
        uv, s = G.gmm_item(p3, gmm, int(idx), g["u"][n], atol)
        assert np.array_equal(uv, g["uvxyz" + tag][n])
        assert np.array_equal(s, g["noise_scale" + tag][n])
        assert np.array_equal(uv[:, :2], g["pose_2d" + tag][n]) and np.array_equal(uv[:, 2:], g["pose_3d" + tag][n])
    assert not np.array_equal(g["uvxyz"], g["uvxyz_f64"])      # the two dtypes are two fixtures


# ---- C ABI --------------------------------------------------------------------------------------
def test_new_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    syms = set(re.findall(r"\bT (dpk_\w+)", out))
    for name in NEW:
        assert name in syms and name in _lib.EXPORTS, name


def test_argument_validation_without_gpu():
    L = _lib.lib()
    m = L.dpk_pose_metrics_n
    for n_pts in (1, 33, 0, -17):
        assert m(None, None, 4, 1, n_pts, 0, None, None, None, None) == -1
        assert m(None, None, 0, 1, n_pts, 0, None, None, None, None) == -1       # before the F = 0 return
    for n_pts in (2, 16, 17, 32):
        assert m(None, None, 0, 1, n_pts, 0, None, None, None, None) == 0        # F = 0: nothing to do
        assert m(None, None, -1, 1, n_pts, 0, None, None, None, None) == -1
        assert m(None, None, 4, 0, n_pts, 0, None, None, None, None) == -1       # H = 0
        assert m(None, None, 4, 1, n_pts, 3, None, None, None, None) == -1       # root_mode 3
        assert m(None, None, 4, 1, n_pts, 0, None, None, None, None) == -1       # null outputs
    for fn in (L.dpk_gmm_sample_n, L.dpk_gmm_sample_f64_n):
        for n_pts in (1, 33):
            assert fn(None, None, 3, n_pts, 5, None, 4, None, 0, 1e-3, None, None, None, None) == -1
            assert fn(None, None, 3, n_pts, 5, None, 0, None, 0, 1e-3, None, None, None, None) == -1
        for n_pts in (2, 16, 32):
            assert fn(None, None, 3, n_pts, 5, None, 0, None, 0, 1e-3, None, None, None, None) == 0
            assert fn(None, None, 3, n_pts, 5, None, -1, None, 0, 1e-3, None, None, None, None) == -1
            assert fn(None, None, 0, n_pts, 5, None, 4, None, 0, 1e-3, None, None, None, None) == -1     # n_src
            assert fn(None, None, 3, n_pts, 0, None, 4, None, 0, 1e-3, None, None, None, None) == -1     # kernel_n
            assert fn(None, None, 3, n_pts, 65, None, 4, None, 0, 1e-3, None, None, None, None) == -1
            assert fn(None, None, 3, n_pts, 5, None, 4, None, 0, 1e-3, None, None, None, None) == -1     # null arrays


# ---- synthetic batches --------------------------------------------------------------------------
def test_synthetic_eval_batches_other_joint_counts():
    got = list(synthetic_eval_batches(50, 20, seed=3, num_pts=16))
    assert [b[0].shape for b in got] == [(20, 16, 2), (20, 16, 2), (10, 16, 2)]
    assert [b[1].shape for b in got] == [(20, 16, 3), (20, 16, 3), (10, 16, 3)]
    assert all(b[0].dtype == np.float32 and b[1].dtype == np.float32 and len(b[2]) == len(b[0]) for b in got)
    x, tgt = synthetic_batch(50, seed=3, num_pts=16)
    assert np.array_equal(np.concatenate([b[0] for b in got]), x[:, :, :2])
    assert np.array_equal(np.concatenate([b[1] for b in got]), tgt)
    assert np.all(tgt[:, 0] == 0)
    # the 17-joint default: the same stream with and without the new argument
    old = list(synthetic_eval_batches(50, 20, seed=3))
    new = list(synthetic_eval_batches(50, 20, seed=3, num_pts=17))
    for a, b in zip(old, new):
        assert a[0].shape[1:] == (17, 2) and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert a[2] == b[2]
    x17, t17 = synthetic_batch(50, seed=3)
    assert np.array_equal(np.concatenate([b[0] for b in old]), x17[:, :, :2])
    assert np.array_equal(np.concatenate([b[1] for b in old]), t17)
    # another action list
    acts = [a for b in synthetic_eval_batches(8, 8, seed=3, num_pts=16, actions=["Jog", "Box"]) for a in b[2]]
    assert acts == ["Jog 1"] * 4 + ["Box 1"] * 4


# ---- the accounting on another action list ------------------------------------------------------
@pytest.mark.parametrize("J", [16, 21])
def test_action_accounting_with_a_custom_action_list(golden, J):
    """As tests/test_metrics_cpu.py::test_action_accounting_matches_reference, on g13's own action list
    (not metrics.TEST_ACTIONS) and joint count."""
    from oracle import metrics_oracle as M

    g = golden(f"g13_metrics_j{J}.npz")
    names = [str(a) for a in g["action_names"]]
    assert not set(names) <= set(metrics.TEST_ACTIONS)
    pred, tgt = g["pred"], g["tgt"]
    acts = [str(a) for a in g["actions"]]
    err = metrics.define_error_list(names)
    assert list(err) == names
    for lo, hi in g["bounds"]:
        p1 = M.mpjpe_per_pose(torch.from_numpy(pred[lo:hi]), torch.from_numpy(tgt[lo:hi])).double().numpy()
        p2 = M.p_mpjpe_per_pose(pred[lo:hi].copy(), tgt[lo:hi].copy()).astype(np.float64)
        metrics.test_calculation(p1, p2, acts[lo:hi], err, n_joints=J)
    for i, a in enumerate(names):
        assert abs(err[a]["p1"].avg - g["action_p1"][i]) <= 1e-6 * max(1.0, g["action_p1"][i])
        assert abs(err[a]["p2"].avg - g["action_p2"][i]) <= 1e-6 * max(1.0, g["action_p2"][i])
    p1, p2 = metrics.print_error(None, err, 1)
    # the reference books fp32 torch scalars; ours books float64 of the same per-frame values
    assert abs(p1 - float(g["p1"])) <= 1e-4 and abs(p2 - float(g["p2"])) <= 1e-4
    seen = {metrics.action_name(a) for a in acts}
    assert len(seen) == 3 and all(err[a]["p1"].count == 0 for a in names if a not in seen)

    # the same through runner.Diffpose.test_hyber with config.data.actions, the per-frame errors handed in
    from diffpose_amd import runner as R

    def oracle_errors(input_2d, targets_3d, H, seq, i, noise, root_mode):
        lo, hi = g["bounds"][i]
        assert np.array_equal(targets_3d, tgt[lo:hi]) and input_2d.shape == (hi - lo, J, 2)
        return (M.mpjpe_per_pose(torch.from_numpy(pred[lo:hi]), torch.from_numpy(tgt[lo:hi])).double(),
                torch.from_numpy(M.p_mpjpe_per_pose(pred[lo:hi].copy(), tgt[lo:hi].copy()).astype(np.float64)))

    edges = [(0, j) for j in range(1, J)]
    d = R.Diffpose(R.default_args(), _config(J, edges, names), device="cpu")
    batches = [(np.zeros((hi - lo, J, 2), np.float32), tgt[lo:hi], acts[lo:hi]) for lo, hi in g["bounds"]]
    q1, q2 = d.test_hyber(batches=batches, is_train=True, frame_errors=oracle_errors)
    assert (q1, q2) == (p1, p2) and list(d.action_error_sum) == names


# ---- runner -------------------------------------------------------------------------------------
ACT = ["Walking", "Jog", "Gestures", "Box"]


def _config(n_pts=16, edges=CHAIN16, actions=ACT):
    from diffpose_amd import runner as R

    cfg = R.default_config(test_times=3, test_timesteps=4, test_num_diffusion_timesteps=50)
    cfg.model.n_pts = n_pts
    cfg.data = ns(dataset="humaneva", num_joints=n_pts)
    if edges is not None:
        cfg.data.edges = edges
    if actions is not None:
        cfg.data.actions = actions
    return cfg


def test_runner_needs_edges_for_another_skeleton():
    from diffpose_amd import runner as R

    args = R.default_args(noise="torch-cpu")
    with pytest.raises(ValueError, match="edges"):
        R.Diffpose(args, _config(edges=None), device="cpu")
    with pytest.raises(ValueError, match="edges"):
        R.Diffpose(args, _config(edges=[(0, 1), (1, 16)]), device="cpu")       # joint 16 of 16
    d = R.Diffpose(args, _config(), device="cpu")
    assert d.n_pts == 16 and d.src_mask.shape == (1, 1, 16) and d.actions == ACT
    assert d._adj().shape == (16, 16) and np.allclose(d._adj().sum(1), 1.0)
    # the default batches follow n_pts and the action list (_stub checks the 16-joint shapes)
    p1, p2 = d.test_hyber(is_train=True, n_frames=20, frame_errors=_stub)
    assert p1 > 0 and p2 > 0 and [a for a, v in d.action_error_sum.items() if v["p1"].count] == ACT
    d17 = R.Diffpose(args, R.default_config(), device="cpu")                   # the default: H36M, 17 joints
    assert d17.n_pts == 17 and d17.src_mask.shape == (1, 1, 17) and d17.actions == metrics.TEST_ACTIONS
    from diffpose_amd.gcndiff import adj_mx_from_edges

    assert np.array_equal(d17._adj(), adj_mx_from_edges())


def _batches():
    rng = np.random.Generator(np.random.PCG64(1316))
    out = []
    for b, (n, mixed) in enumerate([(10, False), (7, True), (1, False), (5, True), (6, False)]):
        x2d = rng.normal(0, 0.3, size=(n, 16, 2)).astype(np.float32)
        tgt = rng.normal(0, 0.25, size=(n, 16, 3)).astype(np.float32)
        if mixed:
            acts = [ACT[int(k)] + f" {1 + int(k) % 2}" for k in rng.integers(0, len(ACT), size=n)]
        else:
            acts = [f"{ACT[b % len(ACT)]} 1"] * n
        out.append((x2d, tgt, acts, rng.uniform(0.5, 1.5, size=(n, 16, 5)).astype(np.float32)))
    return out


def _stub(input_2d, targets_3d, H, seq, i, noise, root_mode, start=None):
    """Per-frame values that depend only on the frame (and its rows of the noise, of the hypothesis
    start's draw and of noise_scale), float64."""
    x = torch.from_numpy(input_2d).double()
    t = torch.from_numpy(targets_3d).double()
    F = x.shape[0]
    assert x.shape[1:] == (16, 2) and t.shape[1:] == (16, 3)
    uv0 = torch.cat([x, torch.zeros(F, 16, 1, dtype=torch.float64)], dim=2)
    p1 = torch.norm(t - uv0, dim=-1).mean(-1) * 1e-3
    p2 = 0.5 * p1 + x.std(dim=(1, 2)) * 1e-3 if F else p1.clone()
    if noise is not None and F:
        p2 = p2 + noise.double().view(noise.shape[0], H, F, 16, 5).sum(dim=(0, 1, 3, 4)) * 1e-6
    if start is not None and F:
        e, scale = start
        assert e.shape == (H * F, 16, 5) and scale.shape == (F, 16, 5)
        p1 = p1 + (e.double().view(H, F, 16, 5) * torch.from_numpy(scale).double()).sum(dim=(0, 2, 3)) * 1e-6
    return p1, p2


def _run(eta, noise_start):
    from diffpose_amd import runner as R

    args = R.default_args(eta=eta, noise="torch-cpu", noise_start=noise_start)
    d = R.Diffpose(args, _config(), device="cpu")
    torch.manual_seed(5)
    p1, p2 = d.test_hyber(batches=_batches(), is_train=True, frame_errors=_stub)
    per_action = {a: (v["p1"].sum, v["p1"].count, v["p2"].sum, v["p2"].count) for a, v in d.action_error_sum.items()}
    return p1, p2, per_action, d.epoch_loss


def _worker(rank, port, cases, q):
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(root, "diffpose-nw_amd"), root):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(WORLD))
    torch.set_num_threads(1)
    try:
        dist.init_process_group("gloo", rank=rank, world_size=WORLD)
        q.put((rank, [_run(*c) for c in cases]))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # surface the failure in the parent
        q.put((rank, repr(e)))
        raise


def _spawn(cases):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, port, cases, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(WORLD):
            r, v = q.get(timeout=300)
            assert not isinstance(v, str), f"rank {r} failed: {v}"
            res[r] = v
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    return res


def test_test_hyber_sharded_16_joints_bit_equal():
    """tests/test_runner_dist_gloo.py's check on 16-joint batches with their own action list: eta 0 and 0.5,
    and the noised hypothesis start with a (B,16,5) noise_scale; one spawn of the two ranks for all cases."""
    cases = [(0.0, False), (0.5, False), (0.5, True)]
    single = [_run(*c) for c in cases]
    res = _spawn(cases)
    for r in range(WORLD):
        for c, one, got in zip(cases, single, res[r]):
            assert got[:2] == one[:2], f"{c} rank {r}: {got[:2]} vs {one[:2]}"
            assert got[2] == one[2], f"{c} rank {r}: per-action sums differ"
            assert got[3] == one[3]
    assert all(s[0] > 0 and s[1] > 0 for s in single)
    assert list(single[0][2]) == ACT                       # booked under the config's action list
    assert single[1][1] != single[0][1]                    # the noise reaches the stand-in
    assert single[2][0] != single[1][0]                    # and so do the start's draw and noise_scale
    # a noise_scale of the 17-joint shape is refused, naming the expected one
    from diffpose_amd import runner as R

    d = R.Diffpose(R.default_args(noise="torch-cpu", noise_start=True), _config(), device="cpu")
    bad = [b[:3] + (np.ones((len(b[0]), 17, 5), np.float32),) for b in _batches()]
    with pytest.raises(ValueError, match=r"\(10, 16, 5\)"):
        d.test_hyber(batches=bad, is_train=True, frame_errors=_stub)
