"""CPU: the hypothesis start's interface (exports, version, refusals that return before any device call) and
the runner's sharding of its draws over a gloo world of 2.

With ``args.noise_start`` the runner keeps the reference's ``e = torch.randn_like(input_uvxyz)``
(runners/diffpose_frame.py:359) instead of dropping it, drawn for the whole batch before the per-step draws
at eta = 0 as well, and hands each rank the rows of its frames together with its rows of the batch's
noise_scale.  A stand-in for the HIP pose / sampler / metrics kernels records what ``start=`` it receives; every
rank's rows must equal the single-process rows of its frames bit for bit, and so must the per-step draws.
"""
import ctypes
import os

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from diffpose_amd import _lib
from diffpose_amd.data import shard_frames
from diffpose_amd.dist import shard_rows
from helpers import free_port as _free_port

WORLD = 2
H = 3
SIZES = (10, 7, 1, 5)


def test_version_and_exports():
    L = _lib.lib()
    assert L.dpk_version() >= 101
    assert {"dpk_sample_start", "dpk_q_sample"} <= set(_lib.EXPORTS)
    assert L.dpk_sample_start(None, None, None, None, None, 0, ctypes.c_uint64(0), None, 3, None, 1, None, None) == -1
    assert L.dpk_q_sample(None, None, None, 0, 3, None, 1, None, ctypes.c_uint64(0), None) == -1


def test_exports_still_match_the_header():
    import test_cabi

    test_cabi.test_exports_match_header()
    assert {"dpk_sample_start", "dpk_q_sample"} <= set(test_cabi.declared_functions())


def _batches(with_scale=True):
    rng = np.random.Generator(np.random.PCG64(78))
    out = []
    for n in SIZES:
        x2d = rng.normal(0, 0.3, size=(n, 17, 2)).astype(np.float32)
        tgt = rng.normal(0, 0.25, size=(n, 17, 3)).astype(np.float32)
        sc = np.ones((n, 17, 5), np.float32)
        sc[:, :, :2] = rng.uniform(0.25, 2.0, size=(n, 17, 2)).astype(np.float32)
        out.append((x2d, tgt, ["Walking 1"] * n, sc) if with_scale else (x2d, tgt, ["Walking 1"] * n))
    return out


def _run(eta, with_scale=True, noise_start=True):
    """(p1, p2) and, per batch, what the stand-in received: (e rows, scale rows, z rows) as numpy or None"""
    from diffpose_amd import runner as R

    cfg = R.default_config(test_times=H, test_timesteps=4, test_num_diffusion_timesteps=50)
    args = R.default_args(eta=eta, noise="torch-cpu", noise_start=noise_start)
    d = R.Diffpose(args, cfg, device="cpu")
    seen = []

    def stub(input_2d, targets_3d, H_, seq, i, noise, root_mode, **kw):
        assert (set(kw) == {"start"}) == noise_start and len(kw) == int(noise_start)
        e, sc = kw["start"] if noise_start else (None, None)
        seen.append(tuple(None if a is None else np.asarray(a).copy() for a in (e, sc, noise)))
        F = input_2d.shape[0]
        p1 = torch.from_numpy(np.linalg.norm(targets_3d.astype(np.float64), axis=-1).mean(-1) * 1e-3).reshape(F)
        if e is not None and F:
            p1 = p1 + e.double().view(H_, F, 17, 5).sum(dim=(0, 2, 3)) * 1e-6
        return p1, 0.5 * p1

    torch.manual_seed(5)
    p = d.test_hyber(batches=_batches(with_scale), is_train=True, frame_errors=stub)
    assert d.t_start == 50 and d.hypothesis_loss is None
    return p, seen


def _worker(rank, port, eta, q):
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(root, "diffpose-nw_amd"), root, os.path.join(root, "tests")):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(WORLD))
    torch.set_num_threads(1)
    try:
        dist.init_process_group("gloo", rank=rank, world_size=WORLD)
        q.put((rank, _run(eta)))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # surface the failure in the parent
        q.put((rank, repr(e)))
        raise


def _spawn(eta):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, port, eta, q)) for r in range(WORLD)]
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


def test_each_ranks_start_rows_are_its_frames_rows():
    for eta in (0.0, 0.5):
        p_single, single = _run(eta)
        res = _spawn(eta)
        for r in range(WORLD):
            p, seen = res[r]
            assert p == p_single, f"eta {eta} rank {r}: {p} vs {p_single}"
            assert len(seen) == len(single) == len(SIZES)
            for B, (e1, s1, z1), (e, sc, z) in zip(SIZES, single, seen):
                lo, hi = shard_frames(B, WORLD, r)
                rows = shard_rows(B, H, WORLD, r).numpy()
                assert e1.shape == (H * B, 17, 5) and s1.shape == (B, 17, 5)
                assert np.array_equal(e, e1[rows]) and np.array_equal(sc, s1[lo:hi])
                if eta == 0.0:
                    assert z is None and z1 is None
                else:
                    # make_seq("uniform", 50, 4) has K = 5 steps (0, 12, .., 48)
                    assert z1.shape == (5, H * B, 17, 5) and np.array_equal(z, z1[:, rows])
        # e is drawn at eta = 0 too, and before the per-step draws: the first batch's e does not depend on eta
        # (later batches follow the K draws eta > 0 consumes)
        if eta == 0.0:
            e_eta0 = single[0][0]
        else:
            assert np.array_equal(e_eta0, single[0][0]) and not np.array_equal(single[1][0][:7], e_eta0[:7])


def test_batches_without_a_scale_and_the_start_off():
    _, seen = _run(0.0, with_scale=False)
    assert all(s[1] is None and s[0] is not None for s in seen)
    # the start off: no keyword, the seven positional arguments alone, nothing drawn at eta = 0
    _, seen = _run(0.0, noise_start=False)
    assert all(s == (None, None, None) for s in seen)
    # and a 4-tuple batch is accepted there, its scale ignored
    _, seen = _run(0.5, noise_start=False)
    assert all(s[0] is None and s[1] is None and s[2] is not None for s in seen)
