"""DeviceAdam — clip_grad_norm_, torch.optim.Adam and the EMA of the reference's training loop
(runners/diffpose_frame.py:229-236) as one device-side step on a HipGCNdiff handle (dpk_train_* of
include/diffpose_kernels.h): the parameters, Adam's moments and the EMA shadow stay on the device for the run, and a step
is ``optimizer.step(grads)`` on the gradients of ``HipGCNdiff.diffusion_loss_grad``, with no host wait.

The state interchanges with torch's: ``state_dict()`` / ``load_state_dict()`` are ``torch.optim.Adam``'s format (the
reference's ``states[1]``), ``ema_state_dict()`` / ``load_ema_state_dict()`` ``EMAHelper.state_dict()``'s (``states[4]``).
The format code below needs no device (tests/test_device_optim_cpu.py).
"""
from __future__ import annotations

import ctypes
from collections import OrderedDict

import numpy as np
import torch

from . import _lib

WHICH = {"params": 0, "exp_avg": 1, "exp_avg_sq": 2, "max_exp_avg_sq": 3, "ema": 4}


def split_flat(flat, layout, shapes) -> "OrderedDict":
    """A flat array in dpk_param_layout's order as name -> view in the parameter's shape (``layout``: (name, offset,
    numel) triples, ``shapes``: weights.param_shapes)."""
    return OrderedDict((name, flat[off:off + num].reshape(shapes[name])) for name, off, num in layout)


def join_flat(tensors, layout, total: int, like=None):
    """The inverse: one flat float32 tensor of ``total`` floats, zero between entries, from name -> array (or a list in
    the layout's order)."""
    flat = torch.zeros(total, dtype=torch.float32) if like is None else torch.zeros_like(like)
    for i, (name, off, num) in enumerate(layout):
        v = tensors[i] if isinstance(tensors, (list, tuple)) else tensors[name]
        v = torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v).detach().to(torch.float32).reshape(-1)
        if v.numel() != num:
            raise ValueError(f"{name}: {v.numel()} values for a parameter of {num}")
        flat[off:off + num] = v.to(flat.device)
    return flat


def adam_state_dict(layout, shapes, step: int, arrays: dict, lr: float, betas, eps: float, amsgrad: bool) -> dict:
    """``torch.optim.Adam.state_dict()`` of one parameter group whose parameters are the layout's, in its order
    (``named_parameters`` order): ``arrays`` holds the flat "exp_avg", "exp_avg_sq" and, with amsgrad,
    "max_exp_avg_sq".  Before the first step the state is empty, as torch's is."""
    state = {}
    if step > 0:
        parts = {k: split_flat(torch.as_tensor(arrays[k]), layout, shapes) for k in arrays}
        for i, (name, _off, _num) in enumerate(layout):
            st = {"step": torch.tensor(float(step), dtype=torch.float32)}
            for k in ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if amsgrad else ()):
                st[k] = parts[k][name].clone()
            state[i] = st
    group = {"lr": float(lr), "betas": (float(betas[0]), float(betas[1])), "eps": float(eps), "weight_decay": 0,
             "amsgrad": bool(amsgrad), "maximize": False, "params": list(range(len(layout)))}
    return {"state": state, "param_groups": [group]}


def adam_arrays(sd: dict, layout, total: int, amsgrad: bool):
    """``adam_state_dict`` read back: (step, {name: flat array}, the parameter group) of a ``torch.optim.Adam`` state
    dict over the layout's parameters.  An empty state is step 0 with zero moments; otherwise every parameter must
    carry the same step."""
    groups = sd["param_groups"]
    if len(groups) != 1 or list(groups[0]["params"]) != list(range(len(layout))):
        raise ValueError(f"expected one parameter group over parameters 0..{len(layout) - 1} (named_parameters order)")
    group = groups[0]
    if group.get("weight_decay", 0) or group.get("maximize", False):
        raise NotImplementedError("DeviceAdam has no weight_decay and no maximize: keep such a run on torch.optim.Adam")
    if bool(group.get("amsgrad", False)) != bool(amsgrad):
        raise ValueError(f"the state dict's amsgrad = {group.get('amsgrad', False)}, this optimiser's {amsgrad}")
    keys = ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if amsgrad else ())
    state = sd["state"]
    if not state:
        return 0, {k: torch.zeros(total, dtype=torch.float32) for k in keys}, group
    if sorted(state) != list(range(len(layout))):
        raise ValueError("the state dict holds state for some parameters only")
    steps = {int(float(state[i]["step"])) for i in range(len(layout))}
    if len(steps) != 1:
        raise ValueError(f"the parameters' step counts differ: {sorted(steps)}")
    arrays = {k: join_flat([state[i][k] for i in range(len(layout))], layout, total) for k in keys}
    return steps.pop(), arrays, group


class DeviceAdam:
    """``HipGCNdiff.device_optimizer(...)``.  ``param_groups[0]["lr"]`` is read at every step, so the reference's
    ``lr_decay`` (common/utils.py) works on it unchanged."""

    def __init__(self, model, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, amsgrad: bool = False, grad_clip=None,
                 ema_rate=None):
        from .weights import param_shapes

        self.model = model
        self.betas = (float(betas[0]), float(betas[1]))
        self.eps, self.amsgrad = float(eps), bool(amsgrad)
        self.grad_clip = None if grad_clip is None else float(grad_clip)
        self.ema_rate = None if ema_rate is None else float(ema_rate)
        self.param_groups = [{"lr": float(lr), "betas": self.betas, "eps": self.eps, "weight_decay": 0,
                              "amsgrad": self.amsgrad}]
        self.layout, self.total = model.param_layout()
        self.shapes = param_shapes(hid=model.hid_dim, n_layers=model.num_layer, n_pts=model.n_pts, coords=model.coords_dim)
        cfg = _lib.DpkOptimConfig(self.betas[0], self.betas[1], self.eps, int(self.amsgrad),
                                  0.0 if self.grad_clip is None else self.grad_clip,
                                  -1.0 if self.ema_rate is None else self.ema_rate)
        _lib.check(model._h, "dpk_train_begin", _lib.lib().dpk_train_begin(model._h, ctypes.byref(cfg)))
        self._open = True
        self._stale = False      # the host staging and a persistent sampler's arenas are behind the device parameters
        model._trainer = self

    # -- the step -------------------------------------------------------------------
    def zero_grad(self, set_to_none: bool = True) -> None:
        """Nothing to clear: every gradient call writes every float of its own array."""

    def step(self, grads):
        """One clip + Adam + EMA step and the refresh of the weights the kernels read, on the current stream.  ``grads``:
        what ``diffusion_loss_grad`` returned (its ``.flat``) or a flat float32 device tensor in the same layout
        (all-reduced by the caller where there are several ranks).  Returns the gradient norm before clipping, a 0-d
        device tensor (``clip_grad_norm_``'s return value)."""
        m = self._model()
        flat = grads if torch.is_tensor(grads) else getattr(grads, "flat", None)
        if not (torch.is_tensor(flat) and flat.is_cuda and flat.dtype == torch.float32 and flat.dim() == 1
                and flat.numel() == self.total and flat.device == m.device):
            raise ValueError(f"grads must be diffusion_loss_grad's, or a flat float32 tensor of {self.total} floats on {m.device}")
        flat = flat.contiguous()
        gnorm = torch.empty((), dtype=torch.float32, device=m.device)
        stream = torch.cuda.current_stream(m.device).cuda_stream
        rc = _lib.lib().dpk_train_apply(m._h, flat.data_ptr(), ctypes.c_float(float(self.param_groups[0]["lr"])),
                                        gnorm.data_ptr(), stream)
        _lib.check(m._h, "dpk_train_apply", rc)
        self._stale = True
        return gnorm

    @property
    def step_count(self) -> int:
        return self._get("params")[1]

    # -- the arrays -----------------------------------------------------------------
    def _model(self):
        if not self._open:
            raise RuntimeError("this DeviceAdam is closed")
        return self.model

    def _get(self, which: str):
        m = self._model()
        out = torch.empty(self.total, dtype=torch.float32, device=m.device)
        step = ctypes.c_int64(0)
        stream = torch.cuda.current_stream(m.device).cuda_stream
        rc = _lib.lib().dpk_train_get(m._h, WHICH[which], out.data_ptr(), ctypes.byref(step), stream)
        _lib.check(m._h, "dpk_train_get", rc)
        return out, int(step.value)

    def _set(self, which: str, flat, step: int = -1) -> None:
        m = self._model()
        flat = flat.to(device=m.device, dtype=torch.float32).contiguous()
        stream = torch.cuda.current_stream(m.device).cuda_stream
        rc = _lib.lib().dpk_train_set(m._h, WHICH[which], flat.data_ptr(), int(step), stream)
        _lib.check(m._h, "dpk_train_set", rc)
        self._stale = self._stale or which == "params"
        flat.record_stream(torch.cuda.current_stream(m.device))

    def params_state_dict(self) -> "OrderedDict":
        """The parameters on the device, name -> tensor (views of one fresh flat copy): the model's ``state_dict()``
        while this optimiser is open."""
        return split_flat(self._get("params")[0], self.layout, self.shapes)

    def load_params(self, state_dict) -> None:
        """Overwrite the device parameters (a checkpoint's ``states[0]``; names with or without ``module.``)."""
        sd = {(k[7:] if k.startswith("module.") else k): v for k, v in state_dict.items()}
        self._set("params", join_flat(sd, self.layout, self.total))

    def state_dict(self) -> dict:
        arrays, step = {}, 0
        for k in ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if self.amsgrad else ()):
            flat, step = self._get(k)
            arrays[k] = flat.cpu()
        return adam_state_dict(self.layout, self.shapes, step, arrays, self.param_groups[0]["lr"], self.betas, self.eps,
                               self.amsgrad)

    def load_state_dict(self, sd: dict) -> None:
        step, arrays, group = adam_arrays(sd, self.layout, self.total, self.amsgrad)
        for k in ("betas", "eps"):
            mine = self.param_groups[0][k]
            if k in group and tuple(np.atleast_1d(group[k])) != tuple(np.atleast_1d(mine)):
                raise ValueError(f"the state dict's {k} = {group[k]}, this optimiser was opened with {mine}")
        for k, flat in arrays.items():
            self._set(k, flat, step)
        self.param_groups[0]["lr"] = float(group.get("lr", self.param_groups[0]["lr"]))

    def ema_state_dict(self) -> "OrderedDict":
        if self.ema_rate is None:
            raise RuntimeError("this DeviceAdam keeps no EMA shadow (ema_rate=None)")
        return split_flat(self._get("ema")[0], self.layout, self.shapes)

    def load_ema_state_dict(self, state_dict) -> None:
        if self.ema_rate is None:
            raise RuntimeError("this DeviceAdam keeps no EMA shadow (ema_rate=None)")
        sd = {(k[7:] if k.startswith("module.") else k): v for k, v in state_dict.items()}
        self._set("ema", join_flat(sd, self.layout, self.total))

    def ema_copy(self):
        """A new model of the same shape, graph and device loaded with the shadow (EMAHelper.ema_copy)."""
        m = self._model()
        cfg = _shape_config(m)
        twin = type(m)(m.adj, cfg, device=m.device)
        twin.load_state_dict({k: v.cpu() for k, v in self.ema_state_dict().items()})
        return twin

    # -- the handle's weights -------------------------------------------------------
    def sync(self) -> None:
        """dpk_train_sync: bring the host staging (and a persistent sampler's arenas) up to the device parameters.
        Waits for the device; ``sample``, ``forward`` and ``diffusion_loss`` call it when they need it."""
        m = self._model()
        _lib.check(m._h, "dpk_train_sync", _lib.lib().dpk_train_sync(m._h))
        self._stale = False

    def close(self) -> None:
        """dpk_train_end: the model keeps the trained weights and is an ordinary model again."""
        if not self._open:
            return
        m = self.model
        if getattr(m, "_h", None):
            final = {k: v.cpu().numpy() for k, v in self.params_state_dict().items()}
            _lib.check(m._h, "dpk_train_end", _lib.lib().dpk_train_end(m._h))
            m._state = final
        self._open = False
        if getattr(m, "_trainer", None) is self:
            m._trainer = None


def _shape_config(m):
    from types import SimpleNamespace as ns

    return ns(model=ns(hid_dim=m.hid_dim, emd_dim=m.hid_dim, coords_dim=list(m.coords_dim), num_layer=m.num_layer,
                       n_head=m.n_head, dropout=m.dropout, n_pts=m.n_pts))
