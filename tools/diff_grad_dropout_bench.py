"""Time the train-mode gradient call beside the eval-mode one on the GPU, tools/diff_grad_bench.py's method: B = 1,024,
hid 96 / 4 heads / 5 layers / 17 joints (the shipped shape) on a per-op handle.

  (b) dpk_diff_loss_grad                                    eval mode
  (t) dpk_diff_loss_grad_train at (0.25, 0.1, 0.1)          train mode, the reference's rates

Alternating runs (b, t, b, t, ...), each a window of ``--calls`` calls between device synchronises, medians over
``--rounds`` windows after a warm-up window of each; the call's scratch after (b) alone and after (t).

``--parent LIB``: the eval-mode call on another build of the library (the parent commit's) against this tree's, in
``--pairs`` alternating pairs of fresh processes (``one`` below), each the median of ``--rounds`` windows: the pairs'
differences beside the spread of each library's own medians.

  python tools/diff_grad_dropout_bench.py one      one JSON line for the library DPK_LIB names (or the in-tree one)

Usage:  python tools/diff_grad_dropout_bench.py [--batch 1024] [--rounds 9] [--calls 5] [--parent LIB] [--pairs 4]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffpose-nw_amd"))
RATES = (0.25, 0.1, 0.1)


def setup(B):
    os.environ["DPK_FORCE_GENERIC"] = "1"          # read by dpk_create: the handle below runs per op
    import numpy as np
    import torch

    from diffpose_amd.data import synthetic_batch
    from diffpose_amd.runner import Diffpose, default_args, default_config
    from diffpose_amd.schedule import training_timesteps
    from diffpose_amd.weights import synthetic_state_dict

    if not torch.cuda.is_available():
        raise SystemExit("diff_grad_dropout_bench needs a HIP device (no CPU fallback)")
    dev = torch.device("cuda", 0)
    r = Diffpose(default_args(train_without_dropout=True), default_config(batch_size=B), device=dev)
    r.create_diffusion_model(state_dict=synthetic_state_dict())
    m = r.model_diff
    assert m.fused == 0
    x0 = torch.from_numpy(synthetic_batch(B, seed=7)[0])
    rng = np.random.Generator(np.random.PCG64(8))
    scale = torch.from_numpy((0.5 + rng.random(size=tuple(x0.shape))).astype(np.float32))
    g = torch.Generator().manual_seed(9)
    e = torch.randn(tuple(x0.shape), generator=g).to(dev)
    t = training_timesteps(B, r.num_timesteps, generator=g)
    x0d, scd = x0.to(dev), scale.to(dev)

    def grad(**kw):
        return m.diffusion_loss_grad(x0d, t, r.betas, noise_scale=scd, noise=e, mask=r.src_mask, **kw)

    def window(fn, calls):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / calls * 1e3

    return m, grad, window


def one(args):
    m, grad, window = setup(args.batch)
    window(grad, args.calls)
    ms = [window(grad, args.calls) for _ in range(args.rounds)]
    print(json.dumps({"lib": os.environ.get("DPK_LIB", "in-tree"), "median": statistics.median(ms), "min": min(ms),
                      "max": max(ms)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="bench", choices=("bench", "one"))
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--pairs", type=int, default=4)
    args = ap.parse_args()
    if args.mode == "one":
        return one(args)

    m, grad, window = setup(args.batch)
    runs = {"b": grad, "t": lambda: grad(dropout=RATES, dropout_seed=12345)}
    window(runs["b"], args.calls)                    # warm-up: code objects, scratch, the lazily built arenas
    kib_eval = m.debug_resources()["generic_spare_kib"]
    window(runs["t"], args.calls)
    kib_train = m.debug_resources()["generic_spare_kib"]
    ms = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, fn in runs.items():
            ms[k].append(window(fn, args.calls))
    med = {k: statistics.median(v) for k, v in ms.items()}
    B = args.batch
    print(f"diff_grad_dropout_bench B={B} hid 96 / 4 heads / 5 layers / 17 joints, per-op handle; medians of {args.rounds} "
          f"alternating windows of {args.calls} calls (ms per call, min .. max)")
    print(f"(b) dpk_diff_loss_grad                     {med['b']:9.3f}  ({min(ms['b']):.3f} .. {max(ms['b']):.3f})")
    print(f"(t) dpk_diff_loss_grad_train {RATES}  {med['t']:9.3f}  ({min(ms['t']):.3f} .. {max(ms['t']):.3f})")
    print(f"(t) - (b) = {med['t'] - med['b']:.3f} ms   (t) / (b) = {med['t'] / med['b']:.3f}")
    print(f"scratch of the call: eval {kib_eval * 1024} bytes, train {kib_train * 1024} bytes "
          f"({kib_train / 1024:.1f} MiB)")
    if not args.parent:
        return
    libs = {"parent": os.path.abspath(args.parent), "tree": None}
    got = {k: [] for k in libs}
    for _ in range(args.pairs):
        for k, lib in libs.items():
            env = dict(os.environ)
            env.pop("DPK_LIB", None)
            if lib:
                env["DPK_LIB"] = lib
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "one", "--batch", str(B), "--rounds",
                                str(args.rounds), "--calls", str(args.calls)], env=env, capture_output=True, text=True,
                               timeout=300)
            if p.returncode != 0:
                raise SystemExit(f"{k}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            got[k].append(json.loads(p.stdout.strip().splitlines()[-1])["median"])
    print(f"eval-mode dpk_diff_loss_grad, {args.pairs} alternating pairs of fresh processes (median ms per call of each):")
    for k, v in got.items():
        print(f"  {k:7s} " + "  ".join(f"{x:.3f}" for x in v) + f"   median {statistics.median(v):.3f}  spread {max(v) - min(v):.3f}")
    diffs = [a - b for a, b in zip(got["tree"], got["parent"])]
    print("  tree - parent per pair: " + "  ".join(f"{d:+.3f}" for d in diffs) + f"   median {statistics.median(diffs):+.3f}")


if __name__ == "__main__":
    main()
