"""Shared inputs, references and bars of the denoising-loss gradient tests (tests/test_diff_grad_cpu.py on the CPU,
tests/test_gpu_diff_grad.py on the GPU).  Everything comes from fixed seeds; nothing here touches a GPU.

The call under test (dpk_diff_loss_grad) returns d(sum_n weight * loss_n) / d theta for every parameter of GCNdiff,
loss_n as in tests/diff_loss_cases.py.  The yardstick is torch.autograd through oracle/gcndiff_oracle.py, which is
differentiable as written, at the float32 x_t and target:

    g64   float64 parameters, the whole batch
    g32   float32, the whole batch
    gpp   float32, one pose at a time, the poses' gradients added in ascending order: a second summation order
    gap_p = max(max |g32 - g64|, max |gpp - g64|) per parameter tensor p

A tensor passes when max |gpu - g64| <= GAP_FACTOR * gap_p, GAP_FACTOR = edge_inputs.GAP_FACTOR = 8, the project's
standing margin for a different summation order.  The key biases (self_attn.linears.1.bias) have an exactly zero
gradient (softmax does not see a shift along the keys), so their own gap is rounding residue; their bar is
8 * max(own gap, the same layer's query-bias gap): the query bias sums the same score gradients.
The loss is held to diff_loss_cases' bar, LOSS_REL * (sum |d64| + loss64) per pose.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import diff_loss_cases as LC
import edge_inputs as E
from diffpose_amd.gcndiff import H36M_EDGES, adj_mx_from_edges
from diffpose_amd.weights import synthetic_state_dict
from oracle import gcndiff_oracle as O

GAP_FACTOR = E.GAP_FACTOR
G16_SHAPE = (32, 2, 2, 17, H36M_EDGES)
T_CYCLE = (0, 7, 25, 50, 43, 1, 49, 24, 33)          # on the 51-step betas: both ends of the table
# name: (shape, N); shape = (hid, heads, layers, joints, edges[, coords])
CASES = {
    "g16": (G16_SHAPE, 5),                                      # the fixture's inputs
    "odd": (E.GENERIC_FORM_SHAPES["odd"][0], 7),                # nothing a multiple of 4, d_k 5
    "perop": (E.PER_OP, 9),                                     # (48, 4, 1, 16-joint chain)
    "j32": (E.GENERIC_FORM_SHAPES["j32"][0], 3),                # bit 31 of the mask word, a 1,024-entry A_hat
    "w320": (E.GENERIC_FORM_SHAPES["w320"][0], 2),              # rows too wide to stage in attention_bwd, dlg_partial
    "h96": (LC.SHAPES["h96"], 9),                               # a persistent-sampler handle
    "pad15": (LC.SHAPES["pad15"], 9),                           # padded tiles
    "g16_n40": (G16_SHAPE, 40),                                 # M = 680 rows: six slabs of the dW store pass
    "g16_n1": (G16_SHAPE, 1),
}

BWD_FORMS = {"dw_partial<vec>", "dw_partial<scalar>", "attention_bwd<T>", "ln_bwd", "graph_t<T>", "cheb_t", "dlg<T>",
             "temb_bwd"}
# hid 320 on 17 joints: a pose's [q | k | v | dO] rows (17 x 1281 floats) and the 2 hid-wide dL_g operands (2 x 17 x 641)
# are past 64 KB of LDS, the hid-wide ones (2 x 17 x 321) are not
BWD_FORMS_W320 = (BWD_FORMS - {"attention_bwd<T>"}) | {"attention_bwd<F>", "dlg<F>"}
# the forms debug_grad_forms() reports; GEMM_FORMS derived by hand from gemm_choice's predicates (csrc/dpk_genplan.inc:
# one rule for gen_forward, the training forward and the dX GEMMs) on a device of at least 200 CUs: every GEMM has at most
# 119 rows, so 32-row tiles.  g16 (hid 32, E 128): the input ChebConv (K 15) and the output's dX (K 5) scalar, the
# hidden GEMMs and their transposes on gemm_sk (<4> where the columns are 64 or 128), the MLP's dtp GEMM (no packed
# copy) on gemm<32,vec>, d_k 16 on attention<TT>.  odd (hid 15, E 60): everything scalar but temb.dense.1's dX (60 x 60).
GEMM_FORMS = {
    "g16": {"gemm<32,scalar>", "gemm<32,vec>", "gemm_sk<2>", "gemm_sk<4>", "gemm_narrow", "attention<TT>", "graph<T>",
            "cheb_basis<T>"},
    "odd": {"gemm<32,scalar>", "gemm_narrow", "gemm_sk<4>", "attention<TF>", "graph<T>", "cheb_basis<T>"},
}


def golden_g16(load) -> dict:
    """The g16 fixture (tools/gen_goldens_grad.py) as torch tensors; gradients under "grad.<name>" """
    z = load("g16_train_backward.npz")
    return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


def state_dict_of(shape):
    hid, heads, layers, npts = shape[:4]
    kw = dict(hid=hid, n_layers=layers, n_pts=npts)
    if len(shape) > 5 and shape[5] != 5:
        kw["coords"] = (shape[5], shape[5])
    return synthetic_state_dict(**kw)


@functools.lru_cache(maxsize=None)
def inputs(name: str) -> dict:
    """x0, e [N,J,5], scale [S,J,5] (S = 1 where N is prime, else N's smallest divisor above 1; u, v entries != 1), t,
    betas, the all-ones mask, the model and the float32 references x_t and target.  Do not modify."""
    shape, n = CASES[name]
    hid, heads, layers, npts, edges = shape[:5]
    coords = 5 if len(shape) == 5 else shape[5]
    g = torch.Generator().manual_seed(1600 + 31 * hid + npts + n)
    x0 = 0.3 * torch.randn(n, npts, coords, generator=g)
    e = torch.randn(n, npts, coords, generator=g)
    rows = next((d for d in range(2, n) if n % d == 0), 1)
    scale = torch.ones(rows, npts, coords)
    scale[:, :, :2] = 0.25 + 2.0 * torch.rand(rows, npts, 2, generator=g)
    t = torch.tensor([T_CYCLE[i % len(T_CYCLE)] for i in range(n)], dtype=torch.float32)
    b = E.betas(51)
    return dict(sd=state_dict_of(shape), adj=adj_mx_from_edges(npts, edges), layers=layers, heads=heads, x0=x0, e=e,
                scale=scale, t=t, betas=b, mask=torch.ones(1, 1, npts, dtype=torch.bool),
                x_t=LC.x_t_ref(x0, e, scale, t, b), target=LC.target_ref(e, scale))


def g16_inputs(load) -> dict:
    """``inputs`` for the fixture's own arrays (its x, e, noise_scale [5 rows], t)"""
    z = golden_g16(load)
    t = z["t"].to(torch.float32)
    return dict(sd=state_dict_of(G16_SHAPE), adj=adj_mx_from_edges(17, H36M_EDGES), layers=2, heads=2, x0=z["x"],
                e=z["e"], scale=z["noise_scale"], t=t, betas=z["betas"], mask=torch.ones(1, 1, 17, dtype=torch.bool),
                x_t=LC.x_t_ref(z["x"], z["e"], z["noise_scale"], t, z["betas"]),
                target=LC.target_ref(z["e"], z["noise_scale"]))


def _mask_rows(mask, lo, hi):
    return mask if mask is None or mask.shape[0] == 1 else mask[lo:hi]


def autograd(i: dict, dtype, weight=None, mask=None, per_pose: bool = False, sd=None):
    """(per-pose losses, {name: gradient}) of sum_n weight * loss_n by torch.autograd through the oracle held in
    ``dtype``, at the float32 x_t and target of ``i``.  weight None: the reference's own expression,
    ``(e - eps).square().sum(dim=(1, 2)).mean(dim=0)`` (runners/diffpose_frame.py:226).  ``per_pose``: one backward
    per pose, the gradients added in ascending pose order in ``dtype``."""
    mask = i["mask"] if mask is None else mask
    n = i["x0"].shape[0]
    P = {k: v.clone().requires_grad_(True) for k, v in O.params_to_torch(i["sd"] if sd is None else sd, dtype).items()}
    g = torch.from_numpy(np.asarray(i["adj"])).to(dtype)
    x_t, target, t = i["x_t"].to(dtype), i["target"].to(dtype), i["t"]

    def sums(lo, hi):
        eps = O.gcndiff_forward(P, g, x_t[lo:hi], _mask_rows(mask, lo, hi), t[lo:hi], n_layers=i["layers"],
                                heads=i["heads"])
        return (target[lo:hi] - eps).square().sum(dim=(1, 2))

    names = list(P)
    if not per_pose:
        s = sums(0, n)
        total = s.mean(dim=0) if weight is None else (s * weight).sum()
        grads = torch.autograd.grad(total, [P[k] for k in names])
        return s.detach(), dict(zip(names, grads))
    acc = {k: torch.zeros_like(P[k]) for k in names}
    losses = []
    w = 1.0 / n if weight is None else weight
    for p in range(n):
        s = sums(p, p + 1)
        losses.append(s.detach())
        for k, gk in zip(names, torch.autograd.grad((s * w).sum(), [P[k] for k in names])):
            acc[k] = acc[k] + gk
    return torch.cat(losses), acc


def references(i: dict, weight=None, mask=None, sd=None) -> dict:
    """{"g64", "gap": {name: gap_p}, "bar": {name: bar_p}, "loss64", "loss_bar"} of one case (see the module docstring)"""
    l64, g64 = autograd(i, torch.float64, weight, mask, sd=sd)
    _, g32 = autograd(i, torch.float32, weight, mask, sd=sd)
    _, gpp = autograd(i, torch.float32, weight, mask, per_pose=True, sd=sd)
    gap = {k: max(float((g32[k].double() - g64[k]).abs().max()), float((gpp[k].double() - g64[k]).abs().max()))
           for k in g64}
    bar = {}
    for k, v in gap.items():
        if k.endswith("self_attn.linears.1.bias"):
            v = max(v, gap[k.replace("linears.1.bias", "linears.0.bias")])
        bar[k] = GAP_FACTOR * v
    mk = i["mask"] if mask is None else mask
    lo = LC.loss_oracle(i["sd"] if sd is None else sd, i["adj"], i["layers"], i["heads"], i["x_t"], i["target"], mk, i["t"])
    assert np.allclose(lo["loss64"], l64.numpy(), rtol=1e-12, atol=0)
    return dict(g64=g64, g32=g32, gap=gap, bar=bar, loss64=lo["loss64"], loss_bar=lo["bar"])


@functools.lru_cache(maxsize=None)
def case_references(name: str) -> dict:
    """references(inputs(name)) at the default weight.  Computed once; do not modify."""
    return references(inputs(name))
