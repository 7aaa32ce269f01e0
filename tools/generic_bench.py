"""Throughput of the generic-shape path (csrc/dpk_generic.inc) beside the persistent sampler, for
DESIGN.md (run on the GPU): B=1024, K=50, whole-call time between syncs, median of 5.
  python tools/generic_bench.py
  python tools/generic_bench.py HID HEADS LAYERS [force] [--gemm fp32|f16x3]     one shape, one GEMM mode
  python tools/generic_bench.py pairs [--pairs 9] [--calls 8]
The last form measures the f16x3 GEMM mode of the four width instances against their fp32 mode
(profiles/f16x3_widths_bench.txt): per shape one warmed model in one process, the two modes alternating, each
measurement the mean time of `calls` back-to-back calls between syncs; it prints every pair, the medians and the
spread of the pairs (min - max per mode, and of the per-pair ratio).
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


def make_model(hid, heads, layers, force=False, per_op=False):
    cfg = ns(model=ns(hid_dim=hid, emd_dim=hid, coords_dim=[5, 5], num_layer=layers, n_head=heads, dropout=0.0,
                      n_pts=17))
    if force:
        os.environ["DPK_FORCE_GENERIC"] = "1"
    if per_op:                     # the per-op launches even where a fused width instance exists
        os.environ["DPK_GEN_FUSED"] = "0"
    try:
        m = HipGCNdiff(adj_mx_from_edges(), cfg, device="cuda:0")
    finally:
        os.environ.pop("DPK_FORCE_GENERIC", None)
        os.environ.pop("DPK_GEN_FUSED", None)
    m.load_state_dict(synthetic_state_dict(hid=hid, n_layers=layers))
    return m


def workload(n, k):
    x = torch.from_numpy(synthetic_batch(n, seed=1)[0]).cuda()
    seq = make_seq("uniform", 50, k)
    b = torch.from_numpy(get_beta_schedule("linear", beta_start=1e-4, beta_end=1e-3, num_diffusion_timesteps=51)).float()
    return x, seq, b


def run(label, hid, heads, layers, force=False, n=1024, k=50, per_op=False, gemm="fp32"):
    m = make_model(hid, heads, layers, force=force, per_op=per_op)
    m.set_gemm_mode(gemm)
    x, seq, b = workload(n, k)
    m.sample(x, seq, b)
    ts = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.sample(x, seq, b)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    t = sorted(ts)[2]
    print(f"{label:48s} {t * 1e3:9.2f} ms  {n / t:10.0f} poses/s")
    m.close()


# the four width instances at 5 layers, and the shape DESIGN quotes for dpkn
PAIR_SHAPES = [("dpkw", 128, 8, 5), ("dpkw4", 128, 4, 5), ("dpkn", 64, 2, 5), ("dpkn4", 64, 4, 5), ("dpkn", 64, 2, 2)]


def pairs(n_pairs=9, calls=8, n=1024, k=50):
    """fp32 and f16x3 of each width instance, alternating on one warmed model."""
    x, seq, b = workload(n, k)

    def timed(m, mode):
        m.set_gemm_mode(mode)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            m.sample(x, seq, b)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls * 1e3

    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    print(f"# B={n} K={k}, {n_pairs} alternating pairs, each the mean of {calls} calls between syncs; ms per call")
    for inst, hid, heads, layers in PAIR_SHAPES:
        m = make_model(hid, heads, layers)
        for mode in ("fp32", "f16x3", "fp32", "f16x3"):          # warm both modes' kernels and scratch
            timed(m, mode)
        t32, t16 = [], []
        for i in range(n_pairs):
            t32.append(timed(m, "fp32"))
            t16.append(timed(m, "f16x3"))
            print(f"{inst:6s} hid {hid:3d} / {heads} heads / {layers} layers  pair {i}: fp32 {t32[-1]:8.3f}  f16x3 {t16[-1]:8.3f}"
                  f"  ratio {t16[-1] / t32[-1]:.4f}")
        r = [a / c for a, c in zip(t16, t32)]
        print(f"{inst:6s} hid {hid:3d} / {heads} heads / {layers} layers  MEDIAN fp32 {med(t32):8.3f} ms ({n / med(t32) * 1e3:8.0f} poses/s)"
              f"  f16x3 {med(t16):8.3f} ms ({n / med(t16) * 1e3:8.0f} poses/s)  ratio {med(r):.4f}")
        print(f"{inst:6s} hid {hid:3d} / {heads} heads / {layers} layers  SPREAD fp32 {min(t32):.3f}-{max(t32):.3f}"
              f"  f16x3 {min(t16):.3f}-{max(t16):.3f}  ratio {min(r):.4f}-{max(r):.4f}")
        m.close()


if __name__ == "__main__":
    args = sys.argv[1:]

    def opt(name, default):
        if name in args:
            i = args.index(name)
            v = args[i + 1]
            del args[i:i + 2]
            return v
        return default

    if args and args[0] == "pairs":
        pairs(int(opt("--pairs", 9)), int(opt("--calls", 8)))
        sys.exit(0)
    if args:                       # one shape: generic_bench.py HID HEADS LAYERS [force] [--gemm MODE]  (profiling runs)
        gemm = opt("--gemm", "fp32")
        hid, heads, layers = (int(v) for v in args[:3])
        run(f"hid {hid} / {heads} heads / {layers} layers, {gemm}", hid, heads, layers, force=len(args) > 3, gemm=gemm)
        sys.exit(0)
    run("persistent sampler, hid 96 / 4 heads / 5 layers", 96, 4, 5)
    run("generic path (forced), hid 96 / 4 heads / 5 layers", 96, 4, 5, force=True)
    run("generic path per-op, hid 64 / 2 heads / 2 layers", 64, 2, 2, per_op=True)
    run("fused sampler (dpkn), hid 64 / 2 heads / 2 layers", 64, 2, 2)
    run("generic path per-op, hid 64 / 2 heads / 5 layers", 64, 2, 5, per_op=True)
    run("fused sampler (dpkn), hid 64 / 2 heads / 5 layers", 64, 2, 5)
    run("generic path per-op, hid 128 / 8 heads / 5 layers", 128, 8, 5, per_op=True)
    run("fused wide sampler (dpkw), hid 128 / 8 heads / 5 layers", 128, 8, 5)
    run("generic path per-op, hid 128 / 4 heads / 5 layers", 128, 4, 5, per_op=True)
    run("fused sampler (dpkw4), hid 128 / 4 heads / 5 layers", 128, 4, 5)
    run("generic path per-op, hid 64 / 4 heads / 5 layers", 64, 4, 5, per_op=True)
    run("fused sampler (dpkn4), hid 64 / 4 heads / 5 layers", 64, 4, 5)
