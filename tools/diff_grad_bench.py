"""Time the gradient step on the GPU at B = 1,024, hid 96 / 4 heads / 5 layers / 17 joints (the shipped shape):

  (a) dpk_diff_loss on a per-op handle (DPK_FORCE_GENERIC=1): the forward the backward is built beside
  (b) dpk_diff_loss_grad: training forward + backward
  (c) a full Diffpose.train_step with Adam: draws, (b), .grad, optimizer.step(), the load_state_dict round trip

Alternating runs (a, b, c, a, b, c, ...), each a window of ``--calls`` calls between device synchronises, medians
over ``--rounds`` windows after a warm-up window of each.  Prints the three medians, (b) / (a), (c) - (b), and the
call's scratch (the handle's spare buffer, which every uncaptured call sizes).

``--profile``: a short run of (b) alone for ``rocprofv3 --kernel-trace --stats -- python tools/diff_grad_bench.py
--profile`` (a run of its own: tracing slows the host), whose per-kernel table goes beside these numbers in
profiles/diff_grad_bench.txt.

Usage:  python tools/diff_grad_bench.py [--batch 1024] [--rounds 9] [--calls 5] [--profile]
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
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    os.environ["DPK_FORCE_GENERIC"] = "1"          # read by dpk_create: the handles below run per op

    import numpy as np
    import torch

    from diffpose_amd.data import synthetic_batch
    from diffpose_amd.runner import Diffpose, default_args, default_config
    from diffpose_amd.schedule import training_timesteps
    from diffpose_amd.weights import synthetic_state_dict

    if not torch.cuda.is_available():
        raise SystemExit("diff_grad_bench needs a HIP device (no CPU fallback)")
    dev = torch.device("cuda", 0)
    B = args.batch
    cfg = default_config(batch_size=B)
    cfg.optim = type(cfg.model)(grad_clip=1.0)
    r = Diffpose(default_args(train_without_dropout=True), cfg, device=dev)
    sd = synthetic_state_dict()
    r.create_diffusion_model(state_dict=sd)
    m = r.model_diff
    assert m.fused == 0
    x0 = torch.from_numpy(synthetic_batch(B, seed=7)[0])
    rng = np.random.Generator(np.random.PCG64(8))
    scale = torch.from_numpy((0.5 + rng.random(size=tuple(x0.shape))).astype(np.float32))
    g = torch.Generator().manual_seed(9)
    e = torch.randn(tuple(x0.shape), generator=g).to(dev)
    t = training_timesteps(B, r.num_timesteps, generator=g)
    x0d, scd = x0.to(dev), scale.to(dev)
    params = {k: torch.nn.Parameter(torch.from_numpy(v).to(dev)) for k, v in sd.items()}
    opt = torch.optim.Adam(list(params.values()), lr=1e-5)

    def fwd():
        return m.diffusion_loss(x0d, t, r.betas, noise_scale=scd, noise=e, mask=r.src_mask)

    def grad():
        return m.diffusion_loss_grad(x0d, t, r.betas, noise_scale=scd, noise=e, mask=r.src_mask)

    def step():
        return r.train_step(x0, scale, opt, params, generator=g)

    if args.profile:
        for _ in range(3):
            grad()
        torch.cuda.synchronize(dev)
        return

    def window(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / args.calls * 1e3

    runs = {"a": fwd, "b": grad, "c": step}
    for fn in runs.values():
        window(fn)                                  # warm-up: code objects, scratch, the lazily built arenas
    ms = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, fn in runs.items():
            ms[k].append(window(fn))
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: (min(v), max(v)) for k, v in ms.items()}
    kib = m.debug_resources()["generic_spare_kib"]
    print(f"diff_grad_bench B={B} hid 96 / 4 heads / 5 layers / 17 joints, per-op handle; medians of {args.rounds} "
          f"alternating windows of {args.calls} calls (ms per call, min .. max)")
    print(f"(a) dpk_diff_loss            {med['a']:9.3f}  ({spread['a'][0]:.3f} .. {spread['a'][1]:.3f})")
    print(f"(b) dpk_diff_loss_grad       {med['b']:9.3f}  ({spread['b'][0]:.3f} .. {spread['b'][1]:.3f})")
    print(f"(c) train_step (Adam)        {med['c']:9.3f}  ({spread['c'][0]:.3f} .. {spread['c'][1]:.3f})")
    print(f"(b) / (a) = {med['b'] / med['a']:.2f}   (c) - (b) = {med['c'] - med['b']:.3f} ms")
    print(f"scratch of the call: {kib * 1024} bytes ({kib / 1024:.1f} MiB)")


if __name__ == "__main__":
    main()
