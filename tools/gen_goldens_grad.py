"""Generate the g16 golden vectors (the backward of the training objective) from the REFERENCE itself.

Like tools/gen_goldens_loss.py, this runs on the CPU in the build container only and imports the reference
read-only (``--ref``).  It runs the forward lines of the reference's training step (runners/diffpose_frame.py:219-226)
and ``loss_diff.backward()`` (:229) on the reference's own ``GCNdiff`` at hid 32 / 2 heads / 2 layers / 17 joints with
the build's ``synthetic_state_dict(hid=32, n_layers=2)``, in eval mode (dropout off), for N = 5 poses at the fixed
timesteps t = [0, 7, 25, 50, 43] of the 51-step linear betas, with a noise scale whose u, v entries are not 1.

``g16_train_backward.npz`` holds arrays only: the inputs ``x`` [5,17,5], ``noise_scale``, the draws ``e`` (before the
scale), ``t`` and ``betas``; the reference's ``x_t``, ``eps``, ``sums`` (the per-pose sums of :226) and ``loss_diff``;
and every ``p.grad`` under ``grad.<state_dict name>``.  Its sha256 goes to ``meta_g16.json``.  No existing fixture
and no ``meta.json`` is touched.

torch's float32 ``sqrt`` is not the correctly rounded sqrtf on every CPU, and the library takes sqrtf on the host, so
the tool checks that at these timesteps torch's two roots are the correctly rounded ones and refuses to write a
fixture otherwise.

Usage:  python tools/gen_goldens_grad.py [--ref DIR] [--out DIR]
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

N = 5
T = 51
T_GRAD = [0, 7, 25, 50, 43]
HID, HEADS, LAYERS, JOINTS = 32, 2, 2, 17


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
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
    from diffpose_amd.weights import synthetic_state_dict
    from gen_goldens_skeletons import savez

    cfg = types.SimpleNamespace(model=types.SimpleNamespace(
        hid_dim=HID, emd_dim=HID, coords_dim=[5, 5], num_layer=LAYERS, n_head=HEADS, dropout=0.25, n_pts=JOINTS))
    adj = adj_mx_from_edges(num_pts=JOINTS, edges=torch.tensor(H36M_EDGES, dtype=torch.long), sparse=False)
    sd = synthetic_state_dict(hid=HID, n_layers=LAYERS)
    model = GCNdiff(adj, cfg)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model.eval()
    src_mask = torch.tensor([[[True] * JOINTS]])
    betas = torch.from_numpy(get_beta_schedule("linear", beta_start=1e-4, beta_end=1e-3,
                                               num_diffusion_timesteps=T)).float()

    x0 = torch.from_numpy(synthetic_batch(N, seed=1600)[0])
    g = torch.Generator().manual_seed(1601)
    noise_scale = torch.ones(N, JOINTS, 5)
    noise_scale[:, :, :2] = 0.25 + 2.0 * torch.rand((N, JOINTS, 2), generator=g)
    e_drawn = torch.randn(x0.shape, generator=g)
    t = torch.tensor(T_GRAD, dtype=torch.long)

    # the training step's forward and backward in the reference's order of operations (:219-229)
    e = e_drawn * noise_scale
    a = (1 - betas).cumprod(dim=0).index_select(0, t).view(-1, 1, 1)
    x = x0 * a.sqrt() + e * (1.0 - a).sqrt()
    output_noise = model(x, src_mask, t.float(), 0)
    sums = (e - output_noise).square().sum(dim=(1, 2))
    loss_diff = sums.mean(dim=0)
    model.zero_grad()
    loss_diff.backward()

    for v, r in zip(a.reshape(-1).tolist() + (1.0 - a).reshape(-1).tolist(),
                    a.sqrt().reshape(-1).tolist() + (1.0 - a).sqrt().reshape(-1).tolist()):
        if np.float32(math.sqrt(v)) != np.float32(r):
            raise SystemExit(f"torch's float32 sqrt({v!r}) = {r!r} is not the correctly rounded root on this CPU; "
                             f"timesteps {t.tolist()}")

    grads = {}
    for k, p in model.named_parameters():
        if p.grad is None:
            raise SystemExit(f"{k} has no gradient")
        grads["grad." + k] = p.grad.detach().numpy()
    missing = sorted(set(sd) - {k[5:] for k in grads})
    if missing:
        raise SystemExit(f"state_dict entries without a parameter: {missing}")

    os.makedirs(args.out, exist_ok=True)
    name = "g16_train_backward.npz"
    savez(os.path.join(args.out, name), x=x0.numpy(), noise_scale=noise_scale.numpy(), e=e_drawn.numpy(),
          t=t.numpy(), betas=betas.numpy(), x_t=x.detach().numpy(), eps=output_noise.detach().numpy(),
          sums=sums.detach().numpy(), loss_diff=loss_diff.detach().numpy(), **grads)
    meta = {"generator": "tools/gen_goldens_grad.py", "numpy": np.__version__, "torch": torch.__version__,
            "shape": [HID, HEADS, LAYERS, JOINTS], "t": t.tolist(), "tensors": len(grads),
            "sha256": {name: hashlib.sha256(open(os.path.join(args.out, name), "rb").read()).hexdigest()}}
    with open(os.path.join(args.out, "meta_g16.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    print(json.dumps(meta))


if __name__ == "__main__":
    main()
