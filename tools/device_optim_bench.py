"""Time the training step on the GPU at B = 1,024, hid 96 / 4 heads / 5 layers / 17 joints (the shipped shape), with the
optimiser on the host side (torch) and on the device:

  (a) Diffpose.train_step with torch.optim.Adam: draws, dpk_diff_loss_grad, 54 .grad assignments, clip_grad_norm_,
      optimizer.step(), the load_state_dict round trip
  (b) Diffpose.train_step with a DeviceAdam: draws, dpk_diff_loss_grad, dpk_train_apply; the loss read back as a float,
      as (a) does
  (c) the same with the per-pose losses left on the device (train_epoch's loop body: no host wait in the step)
  (d) dpk_train_apply alone on a fixed gradient: norm, clip + Adam + EMA, the refresh
  (e) dpk_diff_loss_grad alone

Alternating runs (a, b, c, d, e, a, ...), each a window of ``--calls`` calls between device synchronises, medians over
``--rounds`` windows after a warm-up window of each, in one process.  Two models: (a) on a per-op handle as
tools/diff_grad_bench.py measures it, (b)..(e) on a second per-op handle whose weights live on the device.
``--sampler`` runs both on persistent-sampler handles instead (the gradient call is the same per-op model there).

Usage:  python tools/device_optim_bench.py [--batch 1024] [--rounds 9] [--calls 5] [--sampler]
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
        os.environ["DPK_FORCE_GENERIC"] = "1"      # read by dpk_create: the handles below run per op

    import numpy as np
    import torch

    from diffpose_amd.data import synthetic_batch
    from diffpose_amd.runner import Diffpose, default_args, default_config
    from diffpose_amd.weights import synthetic_state_dict

    if not torch.cuda.is_available():
        raise SystemExit("device_optim_bench needs a HIP device (no CPU fallback)")
    dev = torch.device("cuda", 0)
    B = args.batch
    cfg = default_config(batch_size=B)
    cfg.optim = type(cfg.model)(optimizer="Adam", lr=1e-5, eps=1e-8, amsgrad=False, grad_clip=1.0)
    sd = synthetic_state_dict()
    ra, rb = (Diffpose(default_args(train_without_dropout=True), cfg, device=dev) for _ in range(2))
    ra.create_diffusion_model(state_dict=sd), rb.create_diffusion_model(state_dict=sd)
    x0 = torch.from_numpy(synthetic_batch(B, seed=7)[0])
    rng = np.random.Generator(np.random.PCG64(8))
    scale = torch.from_numpy((0.5 + rng.random(size=tuple(x0.shape))).astype(np.float32))
    g = torch.Generator().manual_seed(9)
    params = {k: torch.nn.Parameter(torch.from_numpy(v).to(dev)) for k, v in sd.items()}
    topt = torch.optim.Adam(list(params.values()), lr=1e-5)
    dopt = rb.model_diff.device_optimizer(cfg, ema_rate=0.999)
    _, fixed = rb.model_diff.diffusion_loss_grad(x0.to(dev), torch.zeros(B), rb.betas, noise_scale=scale.to(dev),
                                                 mask=rb.src_mask)
    x0d, scd = x0.to(dev), scale.to(dev)
    tz = torch.zeros(B)

    runs = {
        "a": lambda: ra.train_step(x0, scale, topt, params, generator=g),
        "b": lambda: rb.train_step(x0, scale, dopt, generator=g),
        "c": lambda: rb.train_step(x0, scale, dopt, generator=g, return_losses=True),
        "d": lambda: dopt.step(fixed),
        "e": lambda: rb.model_diff.diffusion_loss_grad(x0d, tz, rb.betas, noise_scale=scd, mask=rb.src_mask),
    }
    names = {"a": "train_step, torch.optim.Adam", "b": "train_step, DeviceAdam", "c": "train_step, DeviceAdam, no wait",
             "d": "dpk_train_apply", "e": "dpk_diff_loss_grad"}

    def window(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / args.calls * 1e3

    for fn in runs.values():
        window(fn)                                  # warm-up: code objects, scratch, the lazily built arenas
    ms = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, fn in runs.items():
            ms[k].append(window(fn))
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(f"device_optim_bench B={B} hid 96 / 4 heads / 5 layers / 17 joints, "
          f"{'persistent-sampler' if args.sampler else 'per-op'} handles (fused={rb.model_diff.fused}); medians of "
          f"{args.rounds} alternating windows of {args.calls} calls (ms per call, min .. max)")
    for k in runs:
        print(f"({k}) {names[k]:34s} {med[k]:9.3f}  ({min(ms[k]):.3f} .. {max(ms[k]):.3f})")
    print(f"(a) - (e) = {med['a'] - med['e']:.3f} ms outside the gradient call with torch's Adam, "
          f"(b) - (e) = {med['b'] - med['e']:.3f} ms with the device's; (a) / (b) = {med['a'] / med['b']:.2f}")
    rb.model_diff.close()
    ra.model_diff.close()


if __name__ == "__main__":
    main()
