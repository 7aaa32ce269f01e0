"""Generate the g17 golden vectors (the training objective's backward in train mode) from the REFERENCE itself.

Like tools/gen_goldens_grad.py, this runs on the CPU in the build container only and imports the reference read-only
(``--ref``).  It runs the g16 step (runners/diffpose_frame.py:219-229: the same ``x``, ``e``, ``noise_scale``, ``t`` at
hid 32 / 2 heads / 2 layers / 17 joints, N = 5) on the reference's own ``GCNdiff`` after ``model.train()`` (:195), with
``torch.nn.Dropout.forward`` replaced for the run by ``x * keep * s``: ``keep`` is the counter-based mask of the
library (tests/dropout_cases.keep_mask, the numpy restatement of include/diffpose_kernels.h's rule) for the site the
called module is, found by module identity through ``named_modules()``:

    atten_layers.l.self_attn.dropout -> (l, 0)   atten_layers.l.sublayer.0.dropout -> (l, 1)   ...sublayer.1.dropout -> (l, 2)
    gconv_layers.l.gconv1.dropout    -> (l, 3)   gconv_layers.l.gconv2.dropout     -> (l, 4)

and ``s`` the float32 1 / (1 - p) of the module's own rate ``p``, which must be the rate the library's caller passes for
that site: (0.25, 0.1, 0.1) = (config.model.dropout, MultiHeadedAttention's default, gcndiff.py:84's constant).  The
element index is the flat index in the tensor the module is given, pose0 = 0.  The number of patched calls must be
5 * layers.  This pins the placement of the five sites to the reference itself.

``g17_train_dropout.npz`` holds arrays only: the inputs ``x``, ``noise_scale``, ``e``, ``t``, ``betas``; ``rates``
(sublayer, attn, gconv) and ``drop_seed``; the reference's ``x_t``, ``eps``, ``sums``, ``loss_diff``; and every
``p.grad`` under ``grad.<state_dict name>``.  Its sha256 goes to ``meta_g17.json``.  No other fixture is touched.

Usage:  python tools/gen_goldens_dropout.py [--ref DIR] [--out DIR]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import math
import os
import re
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffpose-nw_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N = 5
T = 51
T_GRAD = [0, 7, 25, 50, 43]
HID, HEADS, LAYERS, JOINTS = 32, 2, 2, 17
RATES = (0.25, 0.1, 0.1)                 # sublayer, attn, gconv
DROP_SEED = (1 << 41) + 987654321

SITE_OF = ((r"atten_layers\.(\d+)\.self_attn\.dropout", 0), (r"atten_layers\.(\d+)\.sublayer\.0\.dropout", 1),
           (r"atten_layers\.(\d+)\.sublayer\.1\.dropout", 2), (r"gconv_layers\.(\d+)\.gconv1\.dropout", 3),
           (r"gconv_layers\.(\d+)\.gconv2\.dropout", 4))


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

    import dropout_cases as DC
    from diffpose_amd.data import synthetic_batch
    from diffpose_amd.gcndiff import H36M_EDGES
    from diffpose_amd.weights import synthetic_state_dict
    from gen_goldens_skeletons import savez

    assert (DC.REF_RATES, DC.SEED) == (RATES, DROP_SEED)
    cfg = types.SimpleNamespace(model=types.SimpleNamespace(
        hid_dim=HID, emd_dim=HID, coords_dim=[5, 5], num_layer=LAYERS, n_head=HEADS, dropout=RATES[0], n_pts=JOINTS))
    adj = adj_mx_from_edges(num_pts=JOINTS, edges=torch.tensor(H36M_EDGES, dtype=torch.long), sparse=False)
    sd = synthetic_state_dict(hid=HID, n_layers=LAYERS)
    model = GCNdiff(adj, cfg)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model.train()                                                    # runners/diffpose_frame.py:195
    src_mask = torch.tensor([[[True] * JOINTS]])
    betas = torch.from_numpy(get_beta_schedule("linear", beta_start=1e-4, beta_end=1e-3,
                                               num_diffusion_timesteps=T)).float()

    # the dropout modules by identity
    site_of = {}
    for name, mod in model.named_modules():
        if isinstance(mod, torch.nn.Dropout):
            hit = [(int(m.group(1)), site) for pat, site in SITE_OF for m in [re.fullmatch(pat, name)] if m]
            if len(hit) != 1:
                raise SystemExit(f"dropout module {name!r} is none of the five sites")
            site_of[id(mod)] = hit[0]
    if len(site_of) != 5 * LAYERS or len(set(site_of.values())) != 5 * LAYERS:
        raise SystemExit(f"{len(site_of)} dropout modules, expected {5 * LAYERS} distinct sites")

    x0 = torch.from_numpy(synthetic_batch(N, seed=1600)[0])
    g = torch.Generator().manual_seed(1601)
    noise_scale = torch.ones(N, JOINTS, 5)
    noise_scale[:, :, :2] = 0.25 + 2.0 * torch.rand((N, JOINTS, 2), generator=g)
    e_drawn = torch.randn(x0.shape, generator=g)
    t = torch.tensor(T_GRAD, dtype=torch.long)

    calls = []

    def patched(self, x):
        layer, site = site_of[id(self)]
        if not self.training:
            raise SystemExit("a dropout module in eval mode")
        if abs(self.p - DC.site_rate(site, RATES)) > 0:
            raise SystemExit(f"site {(layer, site)}: the module's rate {self.p} is not {DC.site_rate(site, RATES)}")
        if tuple(x.shape) != DC.site_shape(site, N, HEADS, JOINTS, HID):
            raise SystemExit(f"site {(layer, site)}: tensor {tuple(x.shape)}")
        keep = torch.from_numpy(DC.keep_mask(DROP_SEED, layer, site, self.p, 0, x.numel()).reshape(tuple(x.shape)))
        calls.append((layer, site, int(keep.sum()), keep.numel()))
        return x * keep.to(x.dtype) * DC.scale(self.p)

    # the training step's forward and backward in the reference's order of operations (:219-229)
    e = e_drawn * noise_scale
    a = (1 - betas).cumprod(dim=0).index_select(0, t).view(-1, 1, 1)
    x = x0 * a.sqrt() + e * (1.0 - a).sqrt()
    original = torch.nn.Dropout.forward
    torch.nn.Dropout.forward = patched
    try:
        output_noise = model(x, src_mask, t.float(), 0)
        sums = (e - output_noise).square().sum(dim=(1, 2))
        loss_diff = sums.mean(dim=0)
        model.zero_grad()
        loss_diff.backward()
    finally:
        torch.nn.Dropout.forward = original
    if len(calls) != 5 * LAYERS or sorted(c[:2] for c in calls) != sorted(site_of.values()):
        raise SystemExit(f"{len(calls)} patched dropout calls, expected one at each of the {5 * LAYERS} sites")
    for layer, site, kept, total in calls:
        if not 0 < kept < total:
            raise SystemExit(f"site {(layer, site)} keeps {kept} of {total}")

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
    name = "g17_train_dropout.npz"
    savez(os.path.join(args.out, name), x=x0.numpy(), noise_scale=noise_scale.numpy(), e=e_drawn.numpy(),
          t=t.numpy(), betas=betas.numpy(), rates=np.asarray(RATES, dtype=np.float64),
          drop_seed=np.asarray(DROP_SEED, dtype=np.uint64), x_t=x.detach().numpy(),
          eps=output_noise.detach().numpy(), sums=sums.detach().numpy(), loss_diff=loss_diff.detach().numpy(), **grads)
    meta = {"generator": "tools/gen_goldens_dropout.py", "numpy": np.__version__, "torch": torch.__version__,
            "shape": [HID, HEADS, LAYERS, JOINTS], "t": t.tolist(), "tensors": len(grads), "rates": list(RATES),
            "drop_seed": DROP_SEED, "kept": [list(c) for c in sorted(calls)],
            "sha256": {name: hashlib.sha256(open(os.path.join(args.out, name), "rb").read()).hexdigest()}}
    with open(os.path.join(args.out, "meta_g17.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    print(json.dumps(meta))


if __name__ == "__main__":
    main()
