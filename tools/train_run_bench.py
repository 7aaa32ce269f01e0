"""Time the training loop on the GPU at B = 1,024, hid 96 / 4 heads / 5 layers / 17 joints (the shipped shape), with a
DeviceAdam, over a resident GMM dataset of ``--calls`` batches (kernel_n = 5), three ways:

  (a) Diffpose.train_epoch over batches sampled on the device in advance: per step the draws of e and t on the CPU and
      their upload, dpk_diff_loss_grad, dpk_train_apply
  (b) Diffpose.train_epoch fed by PoseGeneratorGMM.batch(seed=) per step: (a) plus the GMM launch, its status read
      back and the host lists of actions and camera parameters
  (c) the inner loop of Diffpose.train: per step PoseGeneratorGMM.batch_device, dpk_train_draws, the gradient call with
      betas from the host, dpk_train_apply; the epoch's permutation drawn and uploaded once

(a) and (b) are the loops as they stood before ``train``; they are the yardstick, (c) is what is measured against them.
Alternating runs (a, b, c, a, ...), each a window of one epoch of ``--calls`` steps between device synchronises,
medians over ``--rounds`` windows after a warm-up window of each, in one process, on one handle and one optimiser.
``--sampler`` runs on a persistent-sampler handle instead of a per-op one (the gradient call is the same per-op model
there).

Usage:  python tools/train_run_bench.py [--batch 1024] [--rounds 9] [--calls 5] [--sampler]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffpose-nw_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--sampler", action="store_true")
    args = ap.parse_args()
    if not args.sampler:
        os.environ["DPK_FORCE_GENERIC"] = "1"      # read by dpk_create: the handle below runs per op

    import numpy as np
    import torch

    from diffpose_amd.gmm import PoseGeneratorGMM
    from diffpose_amd.runner import Diffpose, default_args, default_config
    from diffpose_amd.weights import synthetic_state_dict

    if not torch.cuda.is_available():
        raise SystemExit("train_run_bench needs a HIP device (no CPU fallback)")
    dev = torch.device("cuda", 0)
    B, calls, kn = args.batch, args.calls, 5
    frames = B * calls
    cfg = default_config(batch_size=B)
    cfg.optim = type(cfg.model)(optimizer="Adam", lr=1e-5, eps=1e-8, amsgrad=False, grad_clip=1.0)
    r = Diffpose(default_args(train_without_dropout=True), cfg, device=dev)
    r.create_diffusion_model(state_dict=synthetic_state_dict())
    opt = r.model_diff.device_optimizer(cfg, ema_rate=0.999)

    rng = np.random.Generator(np.random.PCG64(11))
    w = rng.dirichlet(np.ones(kn), size=(frames, 17))
    gmm = np.concatenate([w[..., None], rng.normal(0.0, 0.3, size=(frames, 17, kn, 2)),
                          rng.uniform(0.25, 2.25, size=(frames, 17, kn, 2))], axis=-1).astype(np.float32)
    p3 = rng.normal(0.0, 0.25, size=(frames, 17, 3)).astype(np.float32)
    data = PoseGeneratorGMM([p3], [gmm], [["Walking 1"] * frames], [np.zeros((frames, 9), np.float32)], device=dev)

    gen = torch.Generator().manual_seed(9)
    idx = [np.arange(i * B, (i + 1) * B) for i in range(calls)]
    ahead = [data.batch(ix, seed=3 + i)[:2] for i, ix in enumerate(idx)]
    state = {"epoch": 0, "step": 0}

    def loop_c():
        state["step"], _slots, _sizes = r._train_inner(data, opt, state["epoch"], state["step"])
        state["epoch"] += 1

    runs = {
        "a": lambda: r.train_epoch(ahead, opt, generator=gen),
        "b": lambda: r.train_epoch((data.batch(ix, seed=3 + i) for i, ix in enumerate(idx)), opt, generator=gen),
        "c": loop_c,
    }
    names = {"a": "train_epoch, batches made in advance", "b": "train_epoch, batch(seed=) per step",
             "c": "train()'s inner loop"}

    def window(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / calls * 1e3

    for fn in runs.values():
        window(fn)                                  # warm-up: code objects, scratch, the lazily built arenas
    ms = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, fn in runs.items():
            ms[k].append(window(fn))
    data.check_status()
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(f"train_run_bench B={B} hid 96 / 4 heads / 5 layers / 17 joints, "
          f"{'persistent-sampler' if args.sampler else 'per-op'} handle (fused={r.model_diff.fused}); medians of "
          f"{args.rounds} alternating windows of {calls} steps (ms per step, min .. max)")
    for k in runs:
        print(f"({k}) {names[k]:38s} {med[k]:9.3f}  ({min(ms[k]):.3f} .. {max(ms[k]):.3f})")
    print(f"(c) - (a) = {med['c'] - med['a']:+.3f} ms, (c) - (b) = {med['c'] - med['b']:+.3f} ms, "
          f"(b) - (a) = {med['b'] - med['a']:+.3f} ms")
    r.model_diff.close()


if __name__ == "__main__":
    main()
