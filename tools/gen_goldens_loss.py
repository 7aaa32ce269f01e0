"""Generate the g15 golden vectors (the forward of the training objective) from the REFERENCE itself.

Like tools/gen_goldens.py, this runs on the CPU in the build container only and imports the reference
read-only (``--ref``).  The reference's training step (runners/diffpose_frame.py:203-236) lives inside its
epoch loop and cannot be called; this tool runs its forward lines (:212-226) on the reference's own ``GCNdiff``
with the build's seeded synthetic weights, in eval mode (dropout off: the validation value of the objective),
under ``torch.manual_seed``, drawing ``e`` and then the antithetic ``t`` in the reference's order, for N = 8 poses
of the shipped shape (hid 96 / 4 heads / 5 layers / 17 joints) on the 51-step linear betas of the config.

``g15_train_forward.npz`` holds arrays only: the inputs ``x`` [8,17,5], ``noise_scale`` [8,17,5] (u, v entries
!= 1, as the GMM sampler's variances), the draws ``e`` (before the scale) and ``t``, and the reference's results
``x_t``, ``eps`` (its GCNdiff output), ``sums`` (the per-pose sums of :226, before the batch mean) and
``loss_diff``; ``betas`` beside them.  Its sha256 goes to ``meta_g15.json``.

torch's float32 ``sqrt`` is not the correctly rounded sqrtf on every CPU (tests/test_gpu_hypothesis_start.py,
``_sqrt32``), and the library takes sqrtf on the host.  The fixture must not depend on which CPU wrote it, so the
tool checks that at the drawn timesteps torch's two roots are the correctly rounded ones and refuses to write a
fixture otherwise (choose another ``--seed``).

Usage:  python tools/gen_goldens_loss.py [--ref DIR] [--out DIR] [--seed S]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import math
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffpose-nw_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N = 8
T = 51


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--seed", type=int, default=15)
    args = ap.parse_args()
    sys.path.insert(0, args.ref)
    sys.dont_write_bytecode = True

    import torch
    torch.set_num_threads(1)

    from common.utils_diff import get_beta_schedule
    from models.gcndiff import GCNdiff
    from models.GraFormer import adj_mx_from_edges

    from diffpose_amd.data import synthetic_batch
    from diffpose_amd.gcndiff import H36M_EDGES
    from diffpose_amd.weights import state_dict_sha256, synthetic_state_dict
    from gen_goldens_skeletons import savez

    cfg = types.SimpleNamespace(model=types.SimpleNamespace(
        hid_dim=96, emd_dim=96, coords_dim=[5, 5], num_layer=5, n_head=4, dropout=0.25, n_pts=17))
    adj = adj_mx_from_edges(num_pts=17, edges=torch.tensor(H36M_EDGES, dtype=torch.long), sparse=False)
    sd = synthetic_state_dict()
    model = GCNdiff(adj, cfg)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model.eval()
    src_mask = torch.tensor([[[True] * 17]])
    betas = torch.from_numpy(get_beta_schedule("linear", beta_start=1e-4, beta_end=1e-3,
                                               num_diffusion_timesteps=T)).float()

    x0 = torch.from_numpy(synthetic_batch(N, seed=1500)[0])
    g = torch.Generator().manual_seed(1501)
    noise_scale = torch.ones(N, 17, 5)
    noise_scale[:, :, :2] = 0.25 + 2.0 * torch.rand((N, 17, 2), generator=g)

    torch.manual_seed(args.seed)
    with torch.no_grad():
        # the training step's forward in the reference's order of draws and of operations: e first, then the
        # antithetic t (half the batch drawn, the other half mirrored), the scaled target, x_t, eps, the sums
        e_drawn = torch.randn_like(x0)
        half = torch.randint(low=0, high=T, size=(N // 2 + 1,))
        t = torch.cat([half, T - half - 1], dim=0)[:N]
        e = e_drawn * noise_scale
        a = torch.cumprod(1 - betas, dim=0)[t].view(N, 1, 1)
        x = x0 * a.sqrt() + e * (1.0 - a).sqrt()
        output_noise = model(x, src_mask, t.float(), 0)
        sums = ((e - output_noise) ** 2).sum(dim=(1, 2))
        loss_diff = sums.mean()

    for v, r in zip(a.reshape(-1).tolist() + (1.0 - a).reshape(-1).tolist(),
                    a.sqrt().reshape(-1).tolist() + (1.0 - a).sqrt().reshape(-1).tolist()):
        if np.float32(math.sqrt(v)) != np.float32(r):
            raise SystemExit(f"torch's float32 sqrt({v!r}) = {r!r} is not the correctly rounded root on this CPU; "
                             f"timesteps {t.tolist()}: choose another --seed")

    os.makedirs(args.out, exist_ok=True)
    name = "g15_train_forward.npz"
    savez(os.path.join(args.out, name), x=x0.numpy(), noise_scale=noise_scale.numpy(), e=e_drawn.numpy(),
          t=t.numpy(), betas=betas.numpy(), x_t=x.numpy(), eps=output_noise.numpy(), sums=sums.numpy(),
          loss_diff=loss_diff.numpy())
    meta = {"generator": "tools/gen_goldens_loss.py", "numpy": np.__version__, "torch": torch.__version__,
            "seed": args.seed, "weights_sha256": state_dict_sha256(sd), "t": t.tolist(),
            "sha256": {name: hashlib.sha256(open(os.path.join(args.out, name), "rb").read()).hexdigest()}}
    with open(os.path.join(args.out, "meta_g15.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    print(json.dumps(meta))


if __name__ == "__main__":
    main()
