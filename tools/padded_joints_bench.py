"""Padded tiles against the per-op path at fewer than 17 joints (run on the GPU), for DPK_PAD_MIN
(csrc/dpk_kernels.hip) and profiles/padded_joints_bench.txt.

  python tools/padded_joints_bench.py [--pairs 9] [--calls 3] [--joints 4,8,12,16] [--out FILE]

B=1024, K=50, fp32.  Per cell (hid 96 / 4 heads / 5 layers, hid 128 / 8 / 5 and hid 64 / 2 / 2, each on a chain of
n = 4, 8, 12, 16 joints) two warmed handles of one library in one process: the padded instance
(DPK_PAD_MIN_JOINTS=2) and the per-op path (DPK_FORCE_GENERIC=1), alternating; each measurement is the mean time
of `calls` back-to-back dpk_sample calls between device syncs.  Prints every pair, the medians and the spread of
the per-pair ratio, then the f16x3 mode of the padded instance at n = 16 the same way against its fp32 mode.
"""
import os
import sys
import time
from types import SimpleNamespace as ns

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffpose-nw_amd"))
from diffpose_amd.data import synthetic_batch  # noqa: E402
from diffpose_amd.gcndiff import HipGCNdiff, adj_mx_from_edges  # noqa: E402
from diffpose_amd.schedule import get_beta_schedule, make_seq  # noqa: E402
from diffpose_amd.weights import synthetic_state_dict  # noqa: E402

SHAPES = [(96, 4, 5), (128, 8, 5), (64, 2, 2)]
JOINTS = [4, 8, 12, 16]


def make_model(hid, heads, layers, n, per_op):
    cfg = ns(model=ns(hid_dim=hid, emd_dim=hid, coords_dim=[5, 5], num_layer=layers, n_head=heads, dropout=0.0, n_pts=n))
    key, val = ("DPK_FORCE_GENERIC", "1") if per_op else ("DPK_PAD_MIN_JOINTS", "2")
    os.environ[key] = val
    try:
        m = HipGCNdiff(adj_mx_from_edges(n, tuple((i, i + 1) for i in range(n - 1))), cfg, device="cuda:0")
    finally:
        os.environ.pop(key, None)
    m.load_state_dict(synthetic_state_dict(hid=hid, n_layers=layers, n_pts=n))
    assert m.fused == (0 if per_op else 1)
    return m


def main():
    args = sys.argv[1:]

    def opt(name, default):
        return args[args.index(name) + 1] if name in args else default

    n_pairs, calls, out_path = int(opt("--pairs", 9)), int(opt("--calls", 3)), opt("--out", "")
    joints = [int(v) for v in opt("--joints", ",".join(str(n) for n in JOINTS)).split(",")]
    B, K = 1024, 50
    seq = make_seq("uniform", 50, K)
    b = torch.from_numpy(get_beta_schedule("linear", beta_start=1e-4, beta_end=1e-3, num_diffusion_timesteps=51)).float()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if out_path:
            with open(out_path, "w") as f:
                f.write("\n".join(lines) + "\n")

    def timed(m, x, mode="fp32"):
        m.set_gemm_mode(mode)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            m.sample(x, seq, b)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls * 1e3

    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    say(f"# {torch.cuda.get_device_name(0)}; B={B} K={K}; {n_pairs} alternating pairs, each the mean of {calls} calls "
        "between syncs; ms per call")
    say("# padded: the width's persistent instance on padded tiles; per-op: the same library with DPK_FORCE_GENERIC=1")
    summary = []
    for hid, heads, layers in SHAPES:
        for n in joints:
            x = torch.from_numpy(synthetic_batch(B, seed=1)[0])[:, :n].contiguous().cuda()
            pad, gen = make_model(hid, heads, layers, n, False), make_model(hid, heads, layers, n, True)
            d = float((pad.sample(x, seq, b) - gen.sample(x, seq, b)).abs().max())
            for _ in range(2):
                timed(pad, x), timed(gen, x)
            tp, tg = [], []
            tag = f"hid {hid:3d} / {heads} heads / {layers} layers  n {n:2d}"
            for i in range(n_pairs):
                tp.append(timed(pad, x))
                tg.append(timed(gen, x))
                say(f"{tag}  pair {i}: padded {tp[-1]:8.3f}  per-op {tg[-1]:8.3f}  ratio {tp[-1] / tg[-1]:.4f}")
            r = [p / g for p, g in zip(tp, tg)]
            say(f"{tag}  MEDIAN padded {med(tp):8.3f}  per-op {med(tg):8.3f}  ratio {med(r):.4f}  "
                f"(ratios {min(r):.4f}-{max(r):.4f}; max |padded - per-op| {d:.2e})")
            summary.append((tag, med(tp), med(tg), med(r), max(r)))
            if n == 16:
                for _ in range(2):
                    timed(pad, x, "f16x3")
                t32, t16 = [], []
                for i in range(n_pairs):
                    t32.append(timed(pad, x))
                    t16.append(timed(pad, x, "f16x3"))
                r16 = [a / c for a, c in zip(t16, t32)]
                say(f"{tag}  F16X3 padded fp32 {med(t32):8.3f}  f16x3 {med(t16):8.3f}  ratio {med(r16):.4f}  "
                    f"(ratios {min(r16):.4f}-{max(r16):.4f})")
                pad.set_gemm_mode("fp32")
            pad.close()
            gen.close()
    say("# summary: medians (ms), the median and the largest per-pair ratio padded / per-op")
    for tag, a, c, r, rmax in summary:
        say(f"{tag}  padded {a:8.3f}  per-op {c:8.3f}  ratio {r:.4f}  max {rmax:.4f}  "
            f"{'padded wins by more than 1 %' if r < 0.99 else 'no win of more than 1 %'}")


if __name__ == "__main__":
    main()
