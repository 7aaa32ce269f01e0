"""Shared inputs, references and bars of the denoising-loss tests (tests/test_diff_loss_cpu.py on the CPU,
tests/test_gpu_diff_loss.py on the GPU).  Everything comes from fixed seeds; nothing here touches a GPU.

The call under test (dpk_diff_loss): for pose n with timestep t_n and element r

    target = fl(e * scale)                    scale row n % rows
    x_t    = fl(fl(x0 * sa[t_n]) + fl(target * sb[t_n]))
    eps    = GCNdiff(x_t, mask, t)
    loss_n = ordered fp32 sum over r of fl(d * d), d = fl(target - eps)

with sa[t] = sqrtf(abar[t + 1]), sb[t] = sqrtf(1 - abar[t + 1]) (fp32 subtraction) from schedule.alpha_bar_table.

The references: ``x_t_ref`` is that expression in torch float32 on the CPU, the roots taken as the float64 root
rounded once to float32 (the correctly rounded sqrtf, as edge_inputs.start_xT); ``ordered_sum32`` is the sum in
numpy float32, one operation at a time; ``oracles`` runs the float32 and the float64 oracle at the float32 x_t.

The loss bar against the float64 oracle, per pose: 1e-5 * (sum |d64| + loss64).  An eps error of at most 5e-6 (the
standing bar) moves sum d^2 by at most 2 * 5e-6 * sum |d| (plus 85 * 2.5e-11, nothing); the 85-term fp32 sum and its
85 squares round by at most 85 * 2^-24 * loss = 5.1e-6 loss in all; both rounded up to 1e-5.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import edge_inputs as E
from diffpose_amd.gcndiff import H36M_EDGES
from diffpose_amd.schedule import alpha_bar_table
from oracle import gcndiff_oracle as O

N = E.N                                              # 9: two full 4-pose tiles and a 1-pose tail
T_LOSS = [0, 1, 7, 24, 25, 49, 50, 50, 0]            # on 51-step betas: both ends of the table
CHAIN15 = tuple((i, i + 1) for i in range(14))
DENSE_EDGES = tuple(H36M_EDGES) + ((3, 16), (6, 13))
# name: (hid, heads, layers, joints, edges) — the GPU test's handles
SHAPES = {
    "h96": (96, 4, 2, 17, H36M_EDGES),               # 4-pose tiles; tail plans "four" and "two_pose"
    "dense": (96, 4, 2, 17, DENSE_EDGES),            # the dense Chebyshev kernels
    "h128n8": (128, 8, 2, 17, H36M_EDGES),           # 2-pose tiles
    "h64n2": (64, 2, 2, 17, H36M_EDGES),
    "pad15": (96, 4, 2, 15, CHAIN15),                # padded tiles: two dead rows per pose
    "perop": E.PER_OP,                               # (48, 4, 1, 16, chain)
}
LOSS_REL = 1e-5


def roots(b: torch.Tensor):
    """(sa, sb) [T] float32 of the betas ``b``: the correctly rounded sqrtf of abar[t + 1] and of fl(1 - abar[t + 1])"""
    a = alpha_bar_table(b.numpy())[1:]
    om = (np.float32(1.0) - a).astype(np.float32)
    return (torch.from_numpy(np.sqrt(a.astype(np.float64)).astype(np.float32)),
            torch.from_numpy(np.sqrt(om.astype(np.float64)).astype(np.float32)))


def target_ref(e: torch.Tensor, scale) -> torch.Tensor:
    """fl(e * scale), pose n reading row n % S of ``scale`` [S,J,5] (None: e)"""
    if scale is None:
        return e.clone()
    return e * scale.repeat(e.shape[0] // scale.shape[0], 1, 1)


def x_t_ref(x0, e, scale, t, b) -> torch.Tensor:
    """runners/diffpose_frame.py:219-222 at one timestep per pose, torch float32 on the CPU in the reference's order"""
    sa, sb = roots(b)
    idx = torch.as_tensor(t).long()
    return x0 * sa[idx].view(-1, 1, 1) + target_ref(e, scale) * sb[idx].view(-1, 1, 1)


def ordered_sum32(target, eps) -> np.ndarray:
    """acc = 0; for r ascending: d = fl(target_r - eps_r); acc = fl(acc + fl(d * d)), per pose, numpy float32"""
    tg = np.ascontiguousarray(torch.as_tensor(target).detach().cpu().numpy(), dtype=np.float32)
    ep = np.ascontiguousarray(torch.as_tensor(eps).detach().cpu().numpy(), dtype=np.float32)
    tg, ep = tg.reshape(tg.shape[0], -1), ep.reshape(ep.shape[0], -1)
    acc = np.zeros(tg.shape[0], np.float32)
    for r in range(tg.shape[1]):
        d = tg[:, r] - ep[:, r]
        acc = acc + d * d
        assert d.dtype == np.float32 and acc.dtype == np.float32
    return acc


@functools.lru_cache(maxsize=None)
def inputs(name: str, full_scale: bool = False) -> dict:
    """The baseline regime at the shape with the hypothesis start's draws: x0, e [9,J,5], scale [3,J,5] (or with
    ``full_scale`` nine distinct rows), t, betas, mask, and the references x_t and target.  Do not modify."""
    r = E.regime("baseline", SHAPES[name], start=True)
    scale = r["start_scale"]
    if full_scale:
        g = torch.Generator().manual_seed(91)
        scale = torch.ones_like(r["x"])
        scale[:, :, :2] = 0.25 + 2.0 * torch.rand((N, r["x"].shape[1], 2), generator=g)
    t = torch.tensor(T_LOSS, dtype=torch.float32)
    out = dict(r)
    out.update(x0=r["x"], e=r["start_noise"], scale=scale, t=t,
               x_t=x_t_ref(r["x"], r["start_noise"], scale, t, r["betas"]), target=target_ref(r["start_noise"], scale))
    return out


def loss_oracle(sd, adj, layers, heads, x_t, target, mask, t) -> dict:
    """eps and the per-pose loss at the float32 ``x_t`` from the float32 and the float64 oracle:
    {"eps": (o32, o64, g), "loss32", "loss64", "bar": LOSS_REL * (sum |d64| + loss64)} (float64 numpy, per pose)"""
    out = {}
    for dt in (torch.float32, torch.float64):
        P, g = O.params_to_torch(sd, dt), torch.from_numpy(np.asarray(adj)).to(dt)
        with torch.no_grad():
            eps = O.gcndiff_forward(P, g, x_t.to(dt), mask, t, n_layers=layers, heads=heads)
        d = target.to(dt) - eps
        out[dt] = (eps, (d * d).sum(dim=(1, 2)), d.abs().sum(dim=(1, 2)))
    e32, e64 = out[torch.float32][0], out[torch.float64][0]
    l64, a64 = out[torch.float64][1].numpy(), out[torch.float64][2].numpy()
    return {"eps": (e32, e64, float((e32.double() - e64).abs().max())),
            "loss32": out[torch.float32][1].double().numpy(), "loss64": l64, "bar": LOSS_REL * (a64 + l64)}


@functools.lru_cache(maxsize=None)
def oracles(name: str, full_scale: bool = False) -> dict:
    """loss_oracle of inputs(name, full_scale).  Computed once; do not modify."""
    i = inputs(name, full_scale)
    return loss_oracle(i["sd"], i["adj"], i["layers"], i["heads"], i["x_t"], i["target"], i["mask"], i["t"])


def golden_g15(load) -> dict:
    """The g15 fixture (tools/gen_goldens_loss.py) as torch tensors"""
    z = load("g15_train_forward.npz")
    return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}
