"""CPU, world size 2 over gloo: the data-parallel loop of ``runner.Diffpose.train``.

Each rank runs the poses ``shard_frames(B, 2, rank)`` of every batch; one all-reduce per step adds the shards' flat
gradients, one per epoch the per-batch loss slots.  The device part of a step is tests/train_run_cases.py's stand-in,
a gradient and a loss that depend on the global frame index alone and are small integers in float32, so the sums are
exact in any order: both ranks must end with the single-process run's parameters, optimiser arrays and
``epoch_loss_diff`` bit for bit, and only rank 0 writes files.  Process handling as tests/test_runner_dist_gloo.py.
"""
import os
import tempfile

import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from helpers import free_port as _free_port

WORLD = 2


def _run(log_path):
    import diff_grad_cases as GC
    import train_run_cases as TC
    from diffpose_amd import runner as R

    cfg = TC.run_config(GC.CASES["h96"][0])
    r = R.Diffpose(R.default_args(seed=TC.RUN_SEED, log_path=log_path), cfg, device="cpu")
    opt, data, calls = TC.StubAdam(), TC.StubData(), []
    out = r.train(data, eval_batches=lambda: TC.eval_batches(), optimizer=opt,
                  step_grads=TC.stub_step_grads(opt.total, calls), frame_errors=TC.stub_frame_errors)
    shards = [(c[1], c[2], c[3]) for c in calls]
    return (out, [e["loss_diff"] for e in r.train_log], opt.params, opt.exp_avg, opt.exp_avg_sq, opt.ema, opt.lrs,
            shards, sorted(os.listdir(log_path)) if os.path.isdir(log_path) else [])


def _worker(rank, port, base, q):
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(root, "diffpose-nw_amd"), root, os.path.join(root, "tests")):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(WORLD))
    torch.set_num_threads(1)
    try:
        dist.init_process_group("gloo", rank=rank, world_size=WORLD)
        res = _run(os.path.join(base, f"rank{rank}"))
        q.put((rank, res))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # surface the failure in the parent
        q.put((rank, repr(e)))
        raise


def _spawn(base):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, port, base, q)) for r in range(WORLD)]
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


def test_two_ranks_equal_one_process_bit_for_bit():
    import train_run_cases as TC

    with tempfile.TemporaryDirectory() as base:
        single = _run(os.path.join(base, "single"))
        res = _spawn(base)
        want_files = sorted(["ckpt.pth"] + [f"ckpt_{e}.pth" for e in range(TC.EPOCHS)])
        assert single[8] == want_files
        for r in range(WORLD):
            out, losses, params, m, v, ema, lrs, shards, files = res[r]
            assert out == single[0] and losses == single[1] and lrs == single[6], r
            for got, want, name in ((params, single[2], "params"), (m, single[3], "exp_avg"),
                                    (v, single[4], "exp_avg_sq"), (ema, single[5], "ema")):
                assert torch.equal(got, want), (r, name)
            # the rank's shard of 8 + 8 + 7: the first rank takes the odd frame
            assert shards[:3] == ([(0, 4, 8), (0, 4, 8), (0, 4, 7)] if r == 0 else [(4, 8, 8), (4, 8, 8), (4, 7, 7)])
            assert files == (want_files if r == 0 else []), (r, files)
        a = torch.load(os.path.join(base, "single", "ckpt_2.pth"), weights_only=True)
        b = torch.load(os.path.join(base, "rank0", "ckpt_2.pth"), weights_only=True)
        assert TC.states_equal(a, b)
