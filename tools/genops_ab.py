"""Speed A/B of two libdpk builds on the per-op path and the gradient call (GPU box), each measurement in a fresh
process on the library DPK_LIB names:

  python tools/genops_ab.py one                       one JSON line for the library in DPK_LIB (or the in-tree one)
  python tools/genops_ab.py pairs A.so A2.so B.so     9 alternating rounds of A, A2 (a second copy of A), B; medians,
                                                      the A2 - A difference (A/A) and the B - A difference beside it

What `one` times, in milliseconds:
  sample_b1024   the per-op sampler at hid 128 / 8 heads / 5 layers, B = 1024, K = 50 (tools/generic_bench.py's row),
                 median of 5 calls
  grad_b1024     dpk_diff_loss_grad at the shipped shape on a per-op handle, B = 1024 (tools/diff_grad_bench.py's (b)),
                 median of 5 windows of 5 calls, per call
  eps_n16        per-op dpk_eps at N = 16: wall clock over 200 calls, per call (host launch cost is the whole time)
  sample_xs_n16  per-op dpk_sample with xs / x0s (direct launches) at N = 16, K = 10: wall clock over 200 calls, per call
"""
import json
import os
import statistics
import subprocess
import sys
import time


def one():
    import torch
    import generic_bench as G

    def wall(fn, calls):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls * 1e3

    out = {}
    m = G.make_model(128, 8, 5, per_op=True)
    x, seq, b = G.workload(1024, 50)
    m.sample(x, seq, b)
    out["sample_b1024"] = statistics.median(wall(lambda: m.sample(x, seq, b), 1) for _ in range(5))
    x16, seq10 = x[:16].contiguous(), G.make_seq("uniform", 50, 10)
    t16 = (torch.arange(16, device=x.device, dtype=torch.float32) * 3) % 51
    mask = torch.ones(1, 1, 17, dtype=torch.bool, device=x.device)
    m.set_schedule(seq10, b, 0.0)
    out["eps_n16"] = wall(lambda: m(x16, mask, t16), 200)
    out["sample_xs_n16"] = wall(lambda: m.sample(x16, seq10, b, trajectory=True), 200)
    m.close()
    m = G.make_model(96, 4, 5, force=True)
    t = (torch.arange(1024, dtype=torch.float32) * 7) % 51
    e = torch.randn(x.shape, generator=torch.Generator().manual_seed(3)).to(x.device)
    out["grad_b1024"] = statistics.median(wall(lambda: m.diffusion_loss_grad(x, t, b, noise=e), 5) for _ in range(5))
    m.close()
    print(json.dumps(out))


def pairs(libs, rounds=9):
    names = ["A", "A2", "B"]
    got = {n: [] for n in names}
    for r in range(rounds):
        order = list(zip(names, libs))
        order = order[r % 3:] + order[:r % 3]          # each library first, second and third equally often
        for n, lib in order:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "one"], env=dict(os.environ, DPK_LIB=lib),
                               capture_output=True, text=True, timeout=240)
            if p.returncode != 0:                       # nothing more on the device after a failed run
                sys.exit(f"round {r} {n} ({lib}): exit {p.returncode}\n{p.stdout}{p.stderr}")
            got[n].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(f"round {r} {n:2s} {p.stdout.strip().splitlines()[-1]}", flush=True)
    print(f"\nA = {libs[0]}\nA2 = {libs[1]}\nB = {libs[2]}\nmedians of {rounds} alternating rounds, ms")
    print(f"{'':16s}{'A':>10s}{'A2':>10s}{'B':>10s}{'A2 - A':>10s}{'B - A':>10s}{'A2-A pairs min..max':>24s}{'B-A pairs min..max':>24s}")
    ok = True
    for k in got["A"][0]:
        med = {n: statistics.median(g[k] for g in got[n]) for n in names}
        aa = [x[k] - y[k] for x, y in zip(got["A2"], got["A"])]
        ab = [x[k] - y[k] for x, y in zip(got["B"], got["A"])]
        inside = min(aa) <= med["B"] - med["A"] <= max(aa) or med["B"] <= med["A"]
        ok = ok and inside
        print(f"{k:16s}{med['A']:10.4f}{med['A2']:10.4f}{med['B']:10.4f}{med['A2'] - med['A']:+10.4f}{med['B'] - med['A']:+10.4f}"
              f"{min(aa):+12.4f}..{max(aa):+.4f}{min(ab):+12.4f}..{max(ab):+.4f}  {'within A/A' if inside else 'OUTSIDE A/A'}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.exit(pairs(sys.argv[2:5]) if sys.argv[1] == "pairs" else one())
