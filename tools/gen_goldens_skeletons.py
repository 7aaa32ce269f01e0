"""Generate the g13 golden vectors (skeletons other than 17 joints) from the REFERENCE itself.

Like tools/gen_goldens.py, this runs on the CPU in the build container only and imports the reference
read-only (``--ref``).  The reference's metrics (common/loss.py, common/utils.py) and its GMM input
sampler (common/generators.py) take the joint count from the array shapes, so the fixtures are its own
results at 16 and 21 joints:

* ``g13_metrics_j16.npz``, ``g13_metrics_j21.npz`` — shaped like g7: 24 frames in 3 batches, the
  per-frame values of ``mpjpe_by_action_p1`` / ``_p2``, the batch ``mpjpe`` / ``p_mpjpe``, and
  ``test_calculation`` + ``print_error`` on an action list that is not H36M's;
* ``g13_gmm_j16.npz`` — shaped like g8: ``PoseGenerator_gmm`` items under ``np.random.seed``, kernel_n 5,
  6 source frames, from float32 and from float64 arrays, with the uniforms the draws consumed.

The sha256 of every file goes to ``meta_g13.json`` beside them.  The npz files hold arrays and names only.

Usage:  python tools/gen_goldens_skeletons.py [--ref DIR] [--out DIR]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the action lists of the two metrics fixtures (HumanEva's for 16 joints, hand gestures for 21)
ACTIONS = {16: ["Walking", "Jog", "Gestures", "Box", "ThrowCatch"],
           21: ["Grasp", "Pinch", "Point", "Wave"]}


def savez(path, **arrays):
    """np.savez with fixed zip timestamps, so that a second run writes the same bytes."""
    import zipfile

    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name, a in arrays.items():
            import io

            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    sys.path.insert(0, args.ref)
    sys.dont_write_bytecode = True

    import torch
    torch.set_num_threads(1)

    from common.generators import PoseGenerator_gmm
    from common.loss import mpjpe as loss_mpjpe, p_mpjpe as loss_p_mpjpe
    from common.utils import define_error_list, print_error, test_calculation
    from common.utils import p_mpjpe as utils_p_mpjpe

    os.makedirs(args.out, exist_ok=True)
    written = []

    # ---------------- metrics and per-action accounting at 16 and 21 joints ----------------
    for J in (16, 21):
        rng = np.random.Generator(np.random.PCG64(1300 + J))
        n = 24
        tgt = rng.normal(0.0, 0.25, size=(n, J, 3))
        tgt = tgt - tgt[:, :1]
        pred = np.empty_like(tgt)
        for i in range(n):                      # scaled, rotated (some reflected), shifted, noisy
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            if i % 5 == 0:
                q[:, 0] = -q[:, 0] if np.linalg.det(q) > 0 else q[:, 0]
            pred[i] = rng.uniform(0.7, 1.3) * tgt[i] @ q + rng.normal(0, 0.1, 3) + rng.normal(0, 0.03, (J, 3))
        tgt = tgt.astype(np.float32)
        pred = pred.astype(np.float32)
        names = ACTIONS[J]
        # 3 actions seen (the rest of the list enters the average with 0): a single-action batch
        # and two mixed ones
        acts = [names[0] + " 1"] * 8 + [names[int(k)] + ("" if k % 2 == 0 else f" {1 + int(k)}")
                                        for k in rng.integers(0, 3, size=n - 8)]
        bounds = [(0, 8), (8, 16), (16, 24)]
        err = define_error_list(names)
        for lo, hi in bounds:
            test_calculation(torch.from_numpy(pred[lo:hi]), torch.from_numpy(tgt[lo:hi]), acts[lo:hi], err, None, None)
        p1, p2 = print_error(None, err, 1)
        tp, tt = torch.from_numpy(pred), torch.from_numpy(tgt)
        per_pose_p1 = torch.mean(torch.norm(tp - tt, dim=2), dim=1).numpy()     # mpjpe_by_action_p1's dist
        name = f"g13_metrics_j{J}.npz"
        savez(os.path.join(args.out, name), pred=pred, tgt=tgt, actions=np.array(acts),
              bounds=np.array(bounds), per_pose_p1=per_pose_p1, per_pose_p2=utils_p_mpjpe(pred, tgt),
              loss_p2=np.float64(loss_p_mpjpe(pred, tgt)), loss_p1=np.float64(loss_mpjpe(tp, tt).item()),
              p1=np.float64(p1), p2=np.float64(p2), action_names=np.array(names),
              action_p1=np.array([err[a]["p1"].avg for a in names], dtype=np.float64),
              action_p2=np.array([err[a]["p2"].avg for a in names], dtype=np.float64))
        written.append(name)

    # ---------------- the GMM input sampler at 16 joints ----------------
    J, kn = 16, 5
    rng = np.random.Generator(np.random.PCG64(1316))
    lens = (2, 1, 3)
    p3s, gms, acts, cams = [], [], [], []
    for si, n in enumerate(lens):
        w = rng.dirichlet(np.ones(kn), size=(n, J))
        w[0, 0] = [1, 0, 0, 0, 0]                # one-hot rows and interior zeros
        w[0, 1] = [0, 0, 0, 0, 1]
        w[0, 2] = [0.5, 0, 0.25, 0, 0.25]
        g = np.empty((n, J, kn, 5))
        g[..., 0] = w
        g[..., 1:3] = rng.uniform(-1, 1, size=(n, J, kn, 2))
        g[..., 3:5] = rng.uniform(1e-4, 1e-2, size=(n, J, kn, 2))
        gms.append(g)
        p3s.append(rng.normal(0.0, 0.4, size=(n, J, 3)) + 1.0 / 3.0 + si)
        acts.append([f"Jog {si}"] * n)
        cams.append(rng.normal(size=(n, 9)).astype(np.float32))
    indices = [0, 3, 7, 5, 11, 2, 5]            # past the 6 frames too: the reference wraps them
    out = {}
    for tag, dt in (("", np.float32), ("_f64", np.float64)):
        # float32: the arrays as a loader hands them over; float64: as numpy holds them.  The float32
        # arrays are the float64 ones rounded, so the two item sets differ in the last bits of xyz
        p3d, gmd = [a.astype(dt) for a in p3s], [a.astype(dt) for a in gms]
        ds = PoseGenerator_gmm([a.copy() for a in p3d], [a.copy() for a in gmd], acts, cams)
        np.random.seed(1316)
        items = [ds[i] for i in indices]
        out.update({"poses_3d" + tag: np.concatenate(p3d), "gmm" + tag: np.concatenate(gmd),
                    "uvxyz" + tag: np.stack([it[0].numpy() for it in items]),
                    "noise_scale" + tag: np.stack([it[1].numpy() for it in items]),
                    "pose_2d" + tag: np.stack([it[2].numpy() for it in items]),
                    "pose_3d" + tag: np.stack([it[3].numpy() for it in items])})
        if not tag:
            out.update(actions=np.array([it[4] for it in items]),
                       camerapara=np.stack([it[5].numpy() for it in items]))
    np.random.seed(1316)
    u = np.random.random_sample((len(indices), J))      # one draw per choice() call, frame then joint
    savez(os.path.join(args.out, "g13_gmm_j16.npz"), lens=np.array(lens), indices=np.array(indices), u=u, **out)
    written.append("g13_gmm_j16.npz")

    meta = {"generator": "tools/gen_goldens_skeletons.py", "numpy": np.__version__, "torch": torch.__version__,
            "sha256": {n: hashlib.sha256(open(os.path.join(args.out, n), "rb").read()).hexdigest() for n in written}}
    with open(os.path.join(args.out, "meta_g13.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    print(json.dumps(meta))


if __name__ == "__main__":
    main()
