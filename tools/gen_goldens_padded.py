"""Generate the g14 golden vectors (GCNdiff on skeletons below 17 joints at widths the persistent sampler is
compiled for) from the REFERENCE itself.

Imports the reference read-only (``--ref``, as tools/gen_goldens.py does) and copies nothing from it: its
``GCNdiff`` is built at each config, loaded with the build's generator weights at that shape, and run on CPU
(the shim ``torch.Tensor.cuda = identity`` keeps ``generalized_steps`` there).

* ``g14_shape_h96_n4_l2_j16.npz`` — hid 96 / 4 heads / 2 layers on a 16-joint tree (the H36M skeleton without
  its last joint);
* ``g14_shape_h64_n2_l1_j15.npz`` — hid 64 / 2 heads / 1 layer on a 15-joint tree (HumanEva's layout: a root,
  a neck with head and two arms, two legs).

Each holds 8 frames, shaped like g12: eps at 8 mixed t with the all-ones mask and with a two-key mask, and the
K=10 trajectory (xs, x0s) at eta 0.  The sha256 of every file and of the weights goes to ``meta_g14.json``.

Usage:  python tools/gen_goldens_padded.py [--ref DIR] [--out DIR]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffpose-nw_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

TREE16 = [(0, 1), (1, 2), (2, 3), (0, 4), (4, 5), (5, 6), (0, 7), (7, 8), (8, 9), (9, 10), (8, 11), (11, 12),
          (12, 13), (8, 14), (14, 15)]
TREE15 = [(0, 1), (1, 2), (2, 3), (3, 4), (1, 5), (5, 6), (6, 7), (0, 8), (8, 9), (9, 10), (0, 11), (11, 12),
          (12, 13), (1, 14)]
CASES = [(96, 4, 2, 16, TREE16), (64, 2, 1, 15, TREE15)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    sys.path.insert(0, args.ref)
    sys.dont_write_bytecode = True

    import torch
    torch.Tensor.cuda = lambda self, *a, **k: self          # CPU shim
    torch.set_num_threads(8)

    from models.gcndiff import GCNdiff
    from models.GraFormer import adj_mx_from_edges
    from common.utils_diff import generalized_steps, get_beta_schedule

    from diffpose_amd.data import synthetic_batch
    from diffpose_amd.weights import synthetic_state_dict
    from gen_goldens_skeletons import savez

    os.makedirs(args.out, exist_ok=True)
    b51 = torch.from_numpy(get_beta_schedule("linear", beta_start=0.0001, beta_end=0.001,
                                             num_diffusion_timesteps=51)).float()
    meta = {"generator": "tools/gen_goldens_padded.py", "torch": torch.__version__, "sha256": {},
            "weights_sha256": {}}
    for hid, nh, nl, npts, ed in CASES:
        cfg = types.SimpleNamespace(model=types.SimpleNamespace(
            hid_dim=hid, emd_dim=hid, coords_dim=[5, 5], num_layer=nl, n_head=nh, dropout=0.25, n_pts=npts))
        edges = torch.tensor(ed, dtype=torch.long)
        adj = adj_mx_from_edges(num_pts=npts, edges=edges, sparse=False)
        sd = synthetic_state_dict(hid=hid, n_layers=nl, n_pts=npts)
        model = GCNdiff(adj, cfg)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        model.eval()
        mask = torch.tensor([[[True] * npts]])
        mask2 = mask.clone()
        mask2[0, 0, 2] = False
        mask2[0, 0, npts - 1] = False
        x8, _ = synthetic_batch(8, seed=1400 + hid + npts, num_pts=npts)
        x8 = torch.from_numpy(x8)
        t8 = torch.tensor([49.0, 0.0, 12.0, 31.0, 7.0, 49.0, 25.0, 3.0])
        with torch.no_grad():
            eps = model(x8, mask, t8, 0)
            eps_masked = model(x8, mask2, t8, 0)
        seq10 = list(range(0, 50, 5))
        xs, x0s = generalized_steps(x8, mask, seq10, model, b51, eta=0.0)
        name = f"g14_shape_h{hid}_n{nh}_l{nl}_j{npts}.npz"
        savez(os.path.join(args.out, name), hid=hid, n_head=nh, num_layer=nl, n_pts=npts, edges=edges.numpy(),
              adj=adj.numpy(), x=x8.numpy(), t8=t8.numpy(), eps=eps.numpy(), mask2=mask2.numpy(),
              eps_masked=eps_masked.numpy(), seq=np.array(seq10), T=51, xs=torch.stack(xs).numpy(),
              x0s=torch.stack(x0s).numpy())
        meta["sha256"][name] = hashlib.sha256(open(os.path.join(args.out, name), "rb").read()).hexdigest()
        hh = hashlib.sha256()
        for k_, v_ in sd.items():             # the generator's layout order at this shape
            hh.update(k_.encode())
            hh.update(np.ascontiguousarray(v_, dtype="<f4").tobytes())
        meta["weights_sha256"][name] = hh.hexdigest()
    with open(os.path.join(args.out, "meta_g14.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    print(json.dumps(meta))


if __name__ == "__main__":
    main()
