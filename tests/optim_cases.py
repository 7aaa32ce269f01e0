"""Shared inputs, the float64 model and the bars of the device-side optimiser's tests (tests/test_device_optim_cpu.py on
the CPU, tests/test_gpu_device_optim.py on the GPU).  Everything comes from fixed seeds; nothing here touches a GPU.

The call under test (dpk_train_apply) is clip_grad_norm_ + torch.optim.Adam + the EMA of the reference's loop body on flat
fp32 arrays.  ``model64`` restates its five steps in float64 numpy (tests/test_device_optim_cpu.py pins it to
torch.optim.Adam in float64).  The yardstick of a device array X (params, exp_avg, exp_avg_sq, max_exp_avg_sq), per
parameter tensor p, after 1 step and after 5:

    gap_p = max |torch.optim.Adam in float32 on the CPU - model64|     (``torch32``: the reference's own arithmetic)
    bar_p = max(GAP_FACTOR * gap_p, one float32 ulp of max |model64| over the tensor)

GAP_FACTOR = edge_inputs.GAP_FACTOR = 8, the project's standing margin for another evaluation order; the ulp floor
because a five-element bias can have a lucky gap near 0 while one differently rounded final store is legitimate.
The gaps are computed on every run (``bars``), never stored.  gnorm: within one float32 ulp of the float64 norm.  The EMA
shadow: bitwise ``(1. - mu) * p + mu * shadow`` by torch on the CPU from the device's own p.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import diff_grad_cases as GC
import edge_inputs as E
from diffpose_amd.weights import param_shapes

GAP_FACTOR = E.GAP_FACTOR
LR, BETAS, EPS, MU = 1e-3, (0.9, 0.999), 1e-8, 0.999
STEPS = 5
ARRAYS = ("params", "exp_avg", "exp_avg_sq", "max_exp_avg_sq")
# clip_grad_norm_'s max_norm: active against the synthetic gradients' norm (>> 1), inactive, off
CLIPS = {"active": 1.0, "inactive": 1e9, "off": 0.0}


def layout_of(name: str):
    """((param name, offset, numel) ..., F): dpk_param_layout of a diff_grad_cases case, restated: state_dict order,
    offsets multiples of 4, F = the last entry's offset + numel"""
    shape = GC.CASES[name][0]
    hid, _heads, layers, npts = shape[:4]
    coords = 5 if len(shape) == 5 else shape[5]
    shapes = param_shapes(hid=hid, n_layers=layers, n_pts=npts, coords=(coords, coords))
    out, off = [], 0
    for k, s in shapes.items():
        n = int(np.prod(s))
        out.append((k, off, n))
        off += (n + 3) // 4 * 4
    return tuple(out), out[-1][1] + out[-1][2], shapes


@functools.lru_cache(maxsize=None)
def inputs(name: str) -> dict:
    """params (float32 flat, synthetic_state_dict's values, zero padding) and STEPS flat gradients: randn scaled by
    10^u, u uniform in [-6, 1], so exp_avg_sq spans twelve decades; zero in the padding.  Do not modify."""
    layout, F, shapes = layout_of(name)
    sd = GC.inputs(name)["sd"]
    p = np.zeros(F, dtype=np.float32)
    live = np.zeros(F, dtype=bool)
    for k, off, n in layout:
        p[off:off + n] = np.asarray(sd[k], dtype=np.float32).reshape(-1)
        live[off:off + n] = True
    g = torch.Generator().manual_seed(7700 + F % 1000)
    grads = []
    for _ in range(STEPS):
        v = torch.randn(F, generator=g, dtype=torch.float64) * 10.0 ** (torch.rand(F, generator=g, dtype=torch.float64) * 7 - 6)
        grads.append(np.where(live, v.numpy(), 0.0).astype(np.float32))
    return dict(layout=layout, F=F, shapes=shapes, params=p, grads=grads, sd=sd)


def model64(params, grads, lr=LR, betas=BETAS, eps=EPS, amsgrad=False, clip=0.0, mu=None, init=None):
    """dpk_train_apply's five steps in float64, one dict per step: gnorm, coef, params, exp_avg, exp_avg_sq,
    max_exp_avg_sq (with amsgrad), ema (with mu).  ``init``: a run resumed after ``init["step"]`` steps from its
    exp_avg, exp_avg_sq (and max_exp_avg_sq) instead of a fresh one."""
    p = np.asarray(params, dtype=np.float64).copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    vmax = np.zeros_like(p)
    k0 = 0
    if init is not None:
        m, v = np.asarray(init["exp_avg"], dtype=np.float64).copy(), np.asarray(init["exp_avg_sq"], dtype=np.float64).copy()
        if amsgrad:
            vmax = np.asarray(init["max_exp_avg_sq"], dtype=np.float64).copy()
        k0 = int(init["step"])
    shadow = p.copy()
    b1, b2 = betas
    out = []
    for k, g32 in enumerate(grads, start=k0 + 1):
        g = np.asarray(g32, dtype=np.float64)
        gnorm = float(np.sqrt(np.sum(g * g)))
        coef = min(clip / (gnorm + 1e-6), 1.0) if clip > 0 else 1.0
        g = g * coef
        m = m + (g - m) * (1 - b1)
        v = v * b2 + (g * g) * (1 - b2)
        used = v
        if amsgrad:
            vmax = np.maximum(vmax, v)
            used = vmax
        step_size, bc2_sqrt = lr / (1 - b1 ** k), np.sqrt(1 - b2 ** k)
        p = p - (step_size * m) / (np.sqrt(used) / bc2_sqrt + eps)
        st = dict(gnorm=gnorm, coef=coef, params=p.copy(), exp_avg=m.copy(), exp_avg_sq=v.copy())
        if amsgrad:
            st["max_exp_avg_sq"] = vmax.copy()
        if mu is not None:
            shadow = (1.0 - mu) * p + mu * shadow
            st["ema"] = shadow.copy()
        out.append(st)
    return out


def torch_adam(layout, shapes, params, grads, dtype, lr=LR, betas=BETAS, eps=EPS, amsgrad=False, clip=0.0, mu=None):
    """The reference's own step, torch on the CPU in ``dtype``: one tensor per parameter, clip_grad_norm_ (when clip > 0),
    torch.optim.Adam.step, EMAHelper.update's formula.  One dict of flat float64 arrays per step, as ``model64``; the
    padding stays zero.  Also returns the optimiser and the parameters (for state_dict interchange)."""
    F = len(params)
    ps = [torch.nn.Parameter(torch.from_numpy(np.asarray(params[off:off + n])).to(dtype).reshape(shapes[k]).clone())
          for k, off, n in layout]
    shadow = [q.detach().clone() for q in ps]
    opt = torch.optim.Adam(ps, lr=lr, betas=betas, eps=eps, amsgrad=amsgrad, weight_decay=0.0)
    out = []

    def flat(ts):
        a = np.zeros(F, dtype=np.float64)
        for (k, off, n), t in zip(layout, ts):
            a[off:off + n] = t.detach().double().reshape(-1).numpy()
        return a

    for g32 in grads:
        for (k, off, n), q in zip(layout, ps):
            q.grad = torch.from_numpy(np.asarray(g32[off:off + n])).to(dtype).reshape(shapes[k]).clone()
        gnorm = None
        if clip > 0:
            gnorm = float(torch.nn.utils.clip_grad_norm_(ps, clip))
        opt.step()
        st = dict(gnorm=gnorm, params=flat(ps), exp_avg=flat([opt.state[q]["exp_avg"] for q in ps]),
                  exp_avg_sq=flat([opt.state[q]["exp_avg_sq"] for q in ps]))
        if amsgrad:
            st["max_exp_avg_sq"] = flat([opt.state[q]["max_exp_avg_sq"] for q in ps])
        if mu is not None:
            with torch.no_grad():
                for s, q in zip(shadow, ps):
                    s.copy_((1. - mu) * q.detach() + mu * s)          # EMAHelper.update (models/ema.py)
            st["ema"] = flat(shadow)
        out.append(st)
    return out, opt, ps


def ulp32(x: float) -> float:
    return float(np.spacing(np.float32(abs(x))))


@functools.lru_cache(maxsize=None)
def bars(name: str, amsgrad: bool = False, clip: float = 0.0) -> dict:
    """{"m64": model64's steps, "gap": {(step, array, param): gap}, "bar": {...}} for steps 1 and STEPS of a case.
    Computed once per (case, amsgrad, clip); do not modify."""
    i = inputs(name)
    m64 = model64(i["params"], i["grads"], amsgrad=amsgrad, clip=clip, mu=MU)
    t32, _, _ = torch_adam(i["layout"], i["shapes"], i["params"], i["grads"], torch.float32, amsgrad=amsgrad, clip=clip)
    gap, bar = {}, {}
    for step in (1, STEPS):
        for arr in ARRAYS[:4 if amsgrad else 3]:
            a64, a32 = m64[step - 1][arr], t32[step - 1][arr]
            for k, off, n in i["layout"]:
                key = (step, arr, k)
                gap[key] = float(np.abs(a32[off:off + n] - a64[off:off + n]).max())
                bar[key] = max(GAP_FACTOR * gap[key], ulp32(float(np.abs(a64[off:off + n]).max())))
    return dict(m64=m64, gap=gap, bar=bar)


def within(got_flat, name: str, step: int, arr: str, ref: dict):
    """[(param, delta, bar)] of the tensors of device array ``arr`` (flat, any float dtype) outside their bars"""
    i = inputs(name)
    got = np.asarray(got_flat, dtype=np.float64)
    want = ref["m64"][step - 1][arr]
    miss = []
    for k, off, n in i["layout"]:
        d = float(np.abs(got[off:off + n] - want[off:off + n]).max())
        if not d <= ref["bar"][(step, arr, k)]:
            miss.append((k, d, ref["bar"][(step, arr, k)]))
    return miss


def ema_by_torch(p_flat32, shadow_flat32, mu=MU):
    """(1. - mu) * p + mu * shadow by torch on the CPU on float32 tensors: the bits EMAHelper.update leaves"""
    p, s = torch.as_tensor(p_flat32, dtype=torch.float32), torch.as_tensor(shadow_flat32, dtype=torch.float32)
    return (1. - mu) * p + mu * s
