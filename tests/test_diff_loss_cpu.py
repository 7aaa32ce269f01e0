"""CPU: the denoising loss (dpk_diff_loss, HipGCNdiff.diffusion_loss, runner.Diffpose.diffusion_loss) without a
GPU — the timestep draw, the g15 fixture of the reference's training forward against the restatements the GPU test
holds the kernels to, the runner's distributed accounting over gloo, and the precondition of the GPU test's loss bar.
"""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import diff_loss_cases as D
import edge_inputs as E
from helpers import free_port as _free_port

WORLD = 2


# ---------------------------------------------------------------------------------------
# 1. the antithetic timestep draw

@pytest.mark.parametrize("n,T", [(8, 51), (9, 51), (1, 51), (2, 1000), (1024, 1000)])
def test_training_timesteps_is_the_reference_draw(n, T):
    """runners/diffpose_frame.py:216-218 under the same seed, bitwise; from the default generator and from one passed in"""
    from diffpose_amd.schedule import training_timesteps

    torch.manual_seed(1234 + n)
    t = torch.randint(low=0, high=T, size=(n // 2 + 1,))
    want = torch.cat([t, T - t - 1], dim=0)[:n]
    torch.manual_seed(1234 + n)
    got = training_timesteps(n, T)
    assert got.dtype == torch.int64 and got.shape == (n,) and torch.equal(got, want)
    assert int(got.min()) >= 0 and int(got.max()) <= T - 1
    g = torch.Generator().manual_seed(1234 + n)
    assert torch.equal(training_timesteps(n, T, generator=g), want)
    if n >= 2:      # antithetic: the mirrored half
        h = n // 2 + 1
        assert torch.equal(got[h:], (T - 1 - got[:n - h]))


# ---------------------------------------------------------------------------------------
# 2. the g15 fixture: the reference's training forward in eval mode

def test_g15_fixture_is_listed_with_its_hash():
    import hashlib
    import json

    from conftest import GOLDEN

    meta = json.load(open(os.path.join(GOLDEN, "meta_g15.json")))
    for name, sha in meta["sha256"].items():
        assert hashlib.sha256(open(os.path.join(GOLDEN, name), "rb").read()).hexdigest() == sha, name
    z = np.load(os.path.join(GOLDEN, "g15_train_forward.npz"), allow_pickle=False)
    assert sorted(z.files) == sorted(["x", "noise_scale", "e", "t", "betas", "x_t", "eps", "sums", "loss_diff"])
    assert z["x"].shape == (8, 17, 5) and z["t"].tolist() == meta["t"]
    # both halves of the antithetic draw, and both ends of the table
    assert 0 in z["t"] and 50 in z["t"]


def test_g15_restatements_match_the_reference(golden):
    """The table-based torch expression is the reference's x_t bitwise, the float32 oracle its eps bit for bit, and the
    per-pose sums are its sums: what the GPU test then holds dpk_diff_loss to is the reference's own forward."""
    from diffpose_amd.weights import synthetic_state_dict
    from oracle import gcndiff_oracle as O

    z = D.golden_g15(golden)
    t = z["t"].float()
    target = D.target_ref(z["e"], z["noise_scale"])
    x_t = D.x_t_ref(z["x"], z["e"], z["noise_scale"], t, z["betas"])
    assert torch.equal(x_t, z["x_t"]), float((x_t - z["x_t"]).abs().max())
    P, adj = O.params_to_torch(synthetic_state_dict()), O.adjacency()
    # on one thread, as the fixture's generator ran the reference: torch's CPU GEMMs split their sums by thread
    # count (7e-7 apart at 2 threads and more), so "the same ATen ops" are bit for bit only at the same count
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        with torch.no_grad():
            eps = O.gcndiff_forward(P, adj, x_t, torch.ones(1, 1, 17, dtype=torch.bool), t)
    finally:
        torch.set_num_threads(threads)
    assert torch.equal(eps, z["eps"]), float((eps - z["eps"]).abs().max())
    sums = (target - eps).square().sum(dim=(1, 2))
    assert torch.equal(sums, z["sums"])
    assert torch.equal(sums.mean(dim=0), z["loss_diff"])
    # the ordered fp32 sum the kernels compute is torch's sum up to the bar's rounding share
    ordered = D.ordered_sum32(target, eps)
    assert np.all(np.abs(ordered.astype(np.float64) - sums.double().numpy()) <= 85 * 2.0 ** -24 * sums.double().numpy())


# ---------------------------------------------------------------------------------------
# 3. the precondition of the GPU test's loss bar, on every GPU case's inputs

def _gpu_cases():
    for name in D.SHAPES:
        yield name, False
    yield "h96", True


@pytest.mark.parametrize("name,full_scale", list(_gpu_cases()))
def test_loss_bar_precondition(name, full_scale):
    """The float32 oracle's loss and the ordered float32 restatement of it lie within 1/8 of the bar
    1e-5 * (sum |d64| + loss64), and the oracle's own eps gap is at most G_CEILING: the bar has room for a kernel
    that is as good as the float32 oracle, and the eps bar max(5e-6, 8 g) is the standing one."""
    i, o = D.inputs(name, full_scale), D.oracles(name, full_scale)
    e32, e64, g = o["eps"]
    print(f"{name} full_scale={full_scale}: eps gap {g:.3e}")
    assert g <= E.G_CEILING
    assert np.all(o["bar"] > 0)
    ordered = D.ordered_sum32(i["target"], e32).astype(np.float64)
    for tag, v in (("loss32", o["loss32"]), ("ordered32", ordered)):
        ratio = float((np.abs(v - o["loss64"]) / o["bar"]).max())
        print(f"  {tag}: worst |loss - loss64| / bar = {ratio:.4f}")
        assert ratio <= 1.0 / 8.0, (name, tag, ratio)
    # the inputs reach what they are meant to: both ends of the table, a non-trivial scale, a loss of O(10..100)
    assert i["x_t"].shape == i["x0"].shape and not torch.equal(i["x_t"], i["x0"])
    assert float(o["loss64"].min()) > 1.0


def test_loss_bar_precondition_g15(golden):
    from diffpose_amd.gcndiff import adj_mx_from_edges
    from diffpose_amd.weights import synthetic_state_dict

    z = D.golden_g15(golden)
    target = D.target_ref(z["e"], z["noise_scale"])
    o = D.loss_oracle(synthetic_state_dict(), adj_mx_from_edges(), 5, 4, z["x_t"], target,
                      torch.ones(1, 1, 17, dtype=torch.bool), z["t"].float())
    assert o["eps"][2] <= E.G_CEILING
    ordered = D.ordered_sum32(target, o["eps"][0]).astype(np.float64)
    for v in (o["loss32"], ordered, z["sums"].double().numpy()):
        assert float((np.abs(v - o["loss64"]) / o["bar"]).max()) <= 1.0 / 8.0


def test_reference_expressions():
    """x_t_ref at a uniform t is edge_inputs.start_xT at that t_start, bitwise; ordered_sum32 is the plain loop"""
    i = D.inputs("h96")
    for ts in (0, 34, 50):
        a = D.x_t_ref(i["x0"], i["e"], i["scale"], torch.full((D.N,), float(ts)), i["betas"])
        assert torch.equal(a, E.start_xT(i["x0"], i["e"], i["scale"], ts, i["betas"]))
    tg, ep = i["target"][:2], i["x0"][:2]
    want = []
    for p in range(2):
        acc = np.float32(0)
        for a, b in zip(tg[p].reshape(-1).numpy(), ep[p].reshape(-1).numpy()):
            d = np.float32(a - b)
            acc = np.float32(acc + np.float32(d * d))
        want.append(acc)
    assert D.ordered_sum32(tg, ep).tolist() == want


def test_utils_diffusion_loss_generic_callable_is_the_reference_lines(golden):
    """utils_diff.diffusion_loss with a plain callable (the oracle) reproduces the fixture: x_t and eps bitwise, the
    sums equal."""
    from diffpose_amd.utils_diff import diffusion_loss
    from diffpose_amd.weights import synthetic_state_dict
    from oracle import gcndiff_oracle as O

    z = D.golden_g15(golden)
    P, adj = O.params_to_torch(synthetic_state_dict()), O.adjacency()
    model = lambda x, mk, t, cemd: O.gcndiff_forward(P, adj, x, mk, t)   # noqa: E731
    loss, x_t, eps = diffusion_loss(model, z["x"], z["t"], z["betas"], noise_scale=z["noise_scale"], noise=z["e"],
                                    mask=torch.ones(1, 1, 17, dtype=torch.bool), return_parts=True)
    # compute_alpha's table root is torch's float32 sqrt here, which the fixture's generator checked to be the
    # correctly rounded one at these timesteps
    assert torch.equal(eps, O.gcndiff_forward(P, adj, x_t, torch.ones(1, 1, 17, dtype=torch.bool), z["t"].float()))
    assert float((x_t - z["x_t"]).abs().max()) <= 2.0 ** -22
    assert np.allclose(loss.numpy(), z["sums"].numpy(), rtol=1e-5, atol=0)


# ---------------------------------------------------------------------------------------
# 4. the runner's epoch value over gloo, world size 2

def _batches():
    """(targets_uvxyz, noise_scale) batches: even, ragged (7 = 4 + 3), one pose (rank 1's shard empty), and 5"""
    rng = np.random.Generator(np.random.PCG64(515))
    out = []
    for n in (10, 7, 1, 5):
        x = rng.normal(0, 0.3, size=(n, 17, 5)).astype(np.float32)
        sc = (0.5 + rng.random(size=(n, 17, 5))).astype(np.float32)
        out.append((x, sc))
    return out


def _stub(x0, noise_scale, t, e, i):
    """A per-pose value that depends on every argument's rows of that pose alone, float32"""
    if x0.shape[0] == 0:
        return torch.empty(0, dtype=torch.float32)
    return ((e * noise_scale - 0.1 * x0) ** 2).sum(dim=(1, 2)) + t.float() * 0.25 + float(i)


def _run():
    from diffpose_amd import runner as R

    d = R.Diffpose(R.default_args(seed=77), R.default_config(), device="cpu")
    seen = []

    def stub(x0, noise_scale, t, e, i):
        seen.append((i, x0.shape[0]))
        return _stub(x0, noise_scale, t, e, i)

    return d.diffusion_loss(batches=_batches(), pose_losses=stub), seen


def _worker(rank, port, q):
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(root, "diffpose-nw_amd"), root, os.path.join(root, "tests")):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(WORLD))
    torch.set_num_threads(1)
    try:
        dist.init_process_group("gloo", rank=rank, world_size=WORLD)
        q.put((rank, _run()))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # surface the failure in the parent
        q.put((rank, repr(e)))
        raise


def test_runner_epoch_value_sharded_equals_single_process():
    single, seen = _run()
    assert seen == [(0, 10), (1, 7), (2, 1), (3, 5)]
    # the single-process value is the reference's accounting: update(batch mean, n), then the average
    from diffpose_amd.schedule import training_timesteps

    gen = torch.Generator().manual_seed(77)
    tot, cnt = 0.0, 0
    for i, (x, sc) in enumerate(_batches()):
        n = x.shape[0]
        e = torch.randn((n, 17, 5), generator=gen)
        t = training_timesteps(n, 51, generator=gen)
        tot += float(_stub(torch.from_numpy(x), torch.from_numpy(sc), t, e, i).mean()) * n
        cnt += n
    assert single == tot / cnt and single > 0

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, port, q)) for r in range(WORLD)]
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
    # ragged (4 + 3) and empty (1 + 0) shards
    assert res[0][1] == [(0, 5), (1, 4), (2, 1), (3, 3)] and res[1][1] == [(0, 5), (1, 3), (2, 0), (3, 2)]
    for r in range(WORLD):
        assert res[r][0] == single, (r, res[r][0], single)


def test_train_still_refuses():
    from diffpose_amd.gcndiff import HipGCNdiff

    m = HipGCNdiff.__new__(HipGCNdiff)
    with pytest.raises(NotImplementedError):
        m.train()
    assert hasattr(HipGCNdiff, "diffusion_loss")


def test_symbol_is_exported_and_declared():
    from diffpose_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "dpk_diff_loss" in _lib.EXPORTS
    header = open(os.path.join(root, "include", "diffpose_kernels.h")).read()
    assert "int dpk_diff_loss(dpk_handle* h, const float* x0_dev, const float* t_dev" in header
