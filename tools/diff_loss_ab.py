"""Cost of dpk_diff_loss to the calls that were there before it, and of the call itself (run on the GPU), for
profiles/diff_loss_ab.txt.

  python tools/diff_loss_ab.py pairs --parent build/ab/parent.so [--pairs 9] [--out FILE]
  [DPK_LIB=lib.so] python tools/diff_loss_ab.py one

``one`` times, in one process on one library (DPK_LIB, else the in-tree build), hid 96 / 4 heads / 5 layers at
B = 1024 in fp32: dpk_eps at mixed per-pose t (the mean of 200 back-to-back calls between device syncs), dpk_sample
at K = 50 (the mean of 10) and, where the library has it, dpk_diff_loss with loss alone and with all three outputs,
as one fused launch and as the three-launch composition (DPK_LOSS_FUSED=0; 200 each); prints one JSON line.

``pairs`` runs ``one`` in fresh child processes, one at a time: per round the parent library, this library, and
the parent library again.  (parent, this) are the alternating pairs; (parent, parent again) of the same rounds give
the parent-against-parent spread a difference has to exceed to mean anything.  Stops at the first child that fails.
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffpose-nw_amd"))

B, K = 1024, 50


def one():
    import torch

    from diffpose_amd.data import synthetic_batch
    from diffpose_amd.gcndiff import HipGCNdiff, adj_mx_from_edges
    from diffpose_amd.schedule import get_beta_schedule, make_seq
    from diffpose_amd.weights import synthetic_state_dict

    dev = torch.device("cuda", 0)
    m = HipGCNdiff(adj_mx_from_edges(), None, device=dev)
    m.load_state_dict(synthetic_state_dict())
    x = torch.from_numpy(synthetic_batch(B, seed=5)[0]).to(dev)
    b = torch.from_numpy(get_beta_schedule("linear", beta_start=1e-4, beta_end=1e-3, num_diffusion_timesteps=51)).float()
    seq = make_seq("uniform", 50, K)
    t = (torch.arange(B, device=dev, dtype=torch.float32) % 51).contiguous()
    e = torch.randn(x.shape, generator=torch.Generator().manual_seed(3)).to(dev)
    sc = (0.5 + torch.rand((B // 4,) + tuple(x.shape[1:]), generator=torch.Generator().manual_seed(4))).to(dev)

    def timed(fn, calls):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls * 1e3

    res = {"lib": os.environ.get("DPK_LIB", "in-tree")}
    res["eps_ms"] = timed(lambda: m(x, None, t), 200)
    res["sample_ms"] = timed(lambda: m.sample(x, seq, b), 10)
    if "DPK_LIB" not in os.environ:          # the in-tree build has the call; an older library bound by DPK_LIB may not
        m.set_schedule(seq, b, 0.0)
        res["loss_ms"] = timed(lambda: m.diffusion_loss(x, t, b, noise_scale=sc, noise=e), 200)
        res["loss_parts_ms"] = timed(lambda: m.diffusion_loss(x, t, b, noise_scale=sc, noise=e, return_parts=True), 200)
        res["loss_counter_ms"] = timed(lambda: m.diffusion_loss(x, t, b, noise_scale=sc, noise=None, seed=7), 200)
        # the three-launch composition on the same handle (noising kernel, dpk_eps, sum kernel): what fusing replaces
        os.environ["DPK_LOSS_FUSED"] = "0"
        res["loss_three_ms"] = timed(lambda: m.diffusion_loss(x, t, b, noise_scale=sc, noise=e), 200)
        res["loss_three_counter_ms"] = timed(lambda: m.diffusion_loss(x, t, b, noise_scale=sc, noise=None, seed=7), 200)
        del os.environ["DPK_LOSS_FUSED"]
    m.close()
    print("RESULT " + json.dumps(res), flush=True)


def pairs(parent, n_pairs, out_path):
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if out_path:
            with open(out_path, "w") as f:
                f.write("\n".join(lines) + "\n")

    def child(lib):
        env = dict(os.environ)
        env.pop("DPK_LIB", None)
        if lib:
            env["DPK_LIB"] = os.path.abspath(lib)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "one"], env=env, capture_output=True, text=True,
                           timeout=240)
        if p.returncode != 0:
            say(f"# child on {lib or 'in-tree'} failed with status {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            sys.exit(1)
        return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])

    say(f"# hid 96 / 4 heads / 5 layers, B={B}, fp32; ms per call; every figure a fresh process: the mean of 200 dpk_eps "
        f"(10 dpk_sample, K={K}) calls between device syncs after 3 warm-up calls")
    say(f"# per round: parent ({parent}), this build, parent again")
    rows = []
    for i in range(n_pairs):
        a, n, a2 = child(parent), child(None), child(parent)
        rows.append((a, n, a2))
        say(f"round {i}: eps parent {a['eps_ms']:.4f} this {n['eps_ms']:.4f} parent' {a2['eps_ms']:.4f} | "
            f"sample parent {a['sample_ms']:.3f} this {n['sample_ms']:.3f} parent' {a2['sample_ms']:.3f} | "
            f"diff_loss {n.get('loss_ms', float('nan')):.4f} with x_t, eps out {n.get('loss_parts_ms', float('nan')):.4f} "
            f"counter-based e {n.get('loss_counter_ms', float('nan')):.4f} | three launches {n.get('loss_three_ms', float('nan')):.4f} "
            f"counter-based e {n.get('loss_three_counter_ms', float('nan')):.4f}")
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    for key in ("eps_ms", "sample_ms"):
        pa, th, pb = [r[0][key] for r in rows], [r[1][key] for r in rows], [r[2][key] for r in rows]
        ab = [t_ / p_ for t_, p_ in zip(th, pa)]
        aa = [q_ / p_ for q_, p_ in zip(pb, pa)]
        say(f"{key}: MEDIAN parent {med(pa + pb):.4f} this {med(th):.4f}; ratio this / parent per pair: median {med(ab):.4f} "
            f"({min(ab):.4f}-{max(ab):.4f}); parent' / parent per pair: median {med(aa):.4f} ({min(aa):.4f}-{max(aa):.4f})")
        inside = min(aa + [1 / v for v in aa]) <= med(ab) <= max(aa + [1 / v for v in aa])
        say(f"{key}: the median ratio this / parent {'lies within' if inside else 'LIES OUTSIDE'} the parent-against-parent spread")
    if "loss_ms" in rows[0][1]:
        lo, lp, lc, ep, l3, l3c = ([r[1][k] for r in rows] for k in ("loss_ms", "loss_parts_ms", "loss_counter_ms", "eps_ms",
                                                                    "loss_three_ms", "loss_three_counter_ms"))
        rr = [a_ / b_ for a_, b_ in zip(lo, l3)]
        say(f"dpk_diff_loss, one fused launch: MEDIAN {med(lo):.4f} (loss alone), {med(lp):.4f} (x_t and eps out), {med(lc):.4f} "
            f"(counter-based e); dpk_eps alone {med(ep):.4f}")
        say(f"dpk_diff_loss, three launches (DPK_LOSS_FUSED=0): MEDIAN {med(l3):.4f} (loss alone), {med(l3c):.4f} (counter-based "
            f"e); fused / three launches per round: median {med(rr):.4f} ({min(rr):.4f}-{max(rr):.4f})")


if __name__ == "__main__":
    argv = sys.argv[1:]
    if argv and argv[0] == "one":
        one()
    elif argv and argv[0] == "pairs":
        def opt(name, default):
            return argv[argv.index(name) + 1] if name in argv else default
        pairs(opt("--parent", "build/ab/parent.so"), int(opt("--pairs", 9)), opt("--out", ""))
    else:
        sys.exit(__doc__)
