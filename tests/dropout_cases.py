"""Shared masks, train-mode oracle, references and bars of the dropout tests (tests/test_dropout_cpu.py on the CPU,
tests/test_gpu_dropout.py on the GPU).  Everything comes from fixed seeds; nothing here touches a GPU.

The call under test (dpk_diff_loss_grad_train) is dpk_diff_loss_grad with dropout at the reference's five sites per
layer, under counter-based masks (include/diffpose_kernels.h has the rule).  Here:

    keep_mask      the numpy restatement of the mask rule on counter_draws.philox4x32_10
    forward_train  GCNdiff.forward in train mode with given masks, composed from the oracle's own pieces
                   (oracle/gcndiff_oracle.py), the dropout sites placed as tools/gen_goldens_dropout.py finds them in
                   the reference by module identity (fixture g17)
    autograd / references   as tests/diff_grad_cases.py, through forward_train: g64, g32, per-pose g32, gap_p, and
                   bar_p = GAP_FACTOR (= 8) x gap_p with the key-bias rule unchanged; the loss is held to
                   diff_loss_cases' bar LOSS_REL * (sum |d64| + loss64) of the float64 train-mode forward.

A mask enters the oracle as ``x * keep * s`` with ``s`` the float32 value 1 / (1 - p) the library takes on the host, in
every dtype: the float64 yardstick is the gradient of the same function the device differentiates.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import counter_draws as C
import diff_grad_cases as GC
import diff_loss_cases as LC
from oracle import gcndiff_oracle as O

GAP_FACTOR = GC.GAP_FACTOR
SITES = ("attn", "sub0", "sub1", "gc1", "gc2")            # site ids 0..4
REF_RATES = (0.25, 0.1, 0.1)                               # (sublayer, attn, gconv): config.model.dropout, 0.1, 0.1
SEED = (1 << 41) + 987654321                               # both key words in use
G17_SHAPE = GC.G16_SHAPE
G17_SHARDS = ((0, 3), (3, 5))                              # N = 3 at pose0 = 0, N = 2 at pose0 = 3
ISOLATION_P = 0.25
ISOLATION = {"sublayer": (ISOLATION_P, 0.0, 0.0), "attn": (0.0, ISOLATION_P, 0.0), "gconv": (0.0, 0.0, ISOLATION_P)}
SHAPE_CASES = ("j32", "w320", "h96", "pad15", "g16_n40", "g16_n1")
# every (diff_grad_cases.CASES name, rates) the GPU tests run under SEED
GPU_CASES = tuple(("odd", r) for r in ISOLATION.values()) + tuple((n, REF_RATES) for n in SHAPE_CASES) + \
    (("perop", REF_RATES), ("g16", REF_RATES))
_M32 = 0xFFFFFFFF


def thr(p) -> int:
    """(uint32) ceilf(p * 16777216.0f): the product is an exact power-of-two scaling of float32(p)"""
    v = np.float32(p) * np.float32(16777216.0)
    assert v.dtype == np.float32
    return int(np.ceil(v))


def scale(p) -> float:
    """1.0f / (1.0f - p) in float32, as a Python float"""
    s = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    assert s.dtype == np.float32
    return float(s)


def site_rate(site: int, rates) -> float:
    sublayer, attn, gconv = rates
    return attn if site == 0 else sublayer if site in (1, 2) else gconv


def group_words(seed, layer, site, groups):
    """the four output words of the Philox call of each group g (elements 4 g .. 4 g + 3)"""
    seed = int(seed) & ((1 << 64) - 1)
    g = np.asarray(groups, dtype=np.uint64)
    return C.philox4x32_10(g & np.uint64(_M32), g >> np.uint64(32), int(layer) * 8 + int(site), 0xD809, seed & _M32,
                           seed >> 32)


def keep_mask(seed, layer, site, p, first, n) -> np.ndarray:
    """bool [n]: element i = first .. first + n - 1 of (layer, site) under ``seed`` keeps its value iff
    (w >> 8) >= thr(p), w word i & 3 of Philox4x32-10 at {(i >> 2) lo, hi, layer * 8 + site, 0xD809}"""
    first, n = int(first), int(n)
    if n == 0:
        return np.zeros(0, dtype=bool)
    g0, g1 = first >> 2, (first + n - 1) >> 2
    words = np.stack(group_words(seed, layer, site, np.arange(g0, g1 + 1, dtype=np.uint64)), axis=1).reshape(-1)
    w = words[first - 4 * g0: first - 4 * g0 + n]
    return (w >> np.uint32(8)) >= np.uint32(thr(p))


def site_shape(site: int, n, heads, joints, hid):
    return (n, heads, joints, joints) if site == 0 else (n, joints, hid)


def masks_for(shape, n, rates, seed, pose0: int = 0) -> dict:
    """{(layer, site): (keep bool tensor shaped like the site's tensor, s)} for every site with a nonzero rate, the
    ``n`` poses from global pose ``pose0``"""
    hid, heads, layers, joints = shape[:4]
    out = {}
    for layer in range(layers):
        for site in range(5):
            p = site_rate(site, rates)
            if p == 0:
                continue
            shp = site_shape(site, n, heads, joints, hid)
            per_pose = int(np.prod(shp[1:]))
            k = keep_mask(seed, layer, site, p, pose0 * per_pose, n * per_pose)
            out[(layer, site)] = (torch.from_numpy(k.reshape(shp)), scale(p))
    return out


def coverage(masks: dict) -> bool:
    """every mask has at least one kept and one dropped element"""
    return all(bool(k.any()) and not bool(k.all()) for k, _ in masks.values())


def _drop(x, masks, key, lo=None, hi=None):
    m = masks.get(key) if masks else None
    if m is None:
        return x
    keep, s = m
    if lo is not None:
        keep = keep[lo:hi]
    return x * keep.to(x.dtype) * s


def attention_train(x, mask, lin_w, lin_b, heads, drop):
    """O.multi_head_attention with ``drop`` on p_attn before P.V (models/GraFormer.py:110-113)"""
    nb = x.size(0)
    dk = x.size(-1) // heads
    if mask is not None:
        mask = mask.unsqueeze(1)
    q, k, v = [F.linear(x, lin_w[j], lin_b[j]).view(nb, -1, heads, dk).transpose(1, 2) for j in range(3)]
    scores = torch.matmul(q, k.transpose(-2, -1)) / math.sqrt(dk)
    if mask is not None:
        scores = scores.masked_fill(mask == 0, -1e9)
    p = drop(F.softmax(scores, dim=-1))
    o = torch.matmul(p, v).transpose(1, 2).contiguous().view(nb, -1, heads * dk)
    return F.linear(o, lin_w[3], lin_b[3])


def forward_train(p: dict, graph, x, mask, t, masks, n_layers: int = 5, heads: int = 4, lo=None, hi=None):
    """O.gcndiff_forward with the five dropout sites of every layer (``masks`` as ``masks_for`` gives them; a missing
    site is the identity; ``lo``, ``hi``: the rows of the masks that ``x`` holds)"""
    d = lambda v, key: _drop(v, masks, key, lo, hi)      # noqa: E731
    hid = p["gconv_input.weight"].shape[-1]
    temb = O.timestep_embedding(t, hid, dtype=p["gconv_input.weight"].dtype)
    temb = F.linear(temb, p["temb.dense.0.weight"], p["temb.dense.0.bias"])
    temb = O.swish(temb)
    temb = F.linear(temb, p["temb.dense.1.weight"], p["temb.dense.1.bias"])
    out = O.cheb_conv(x, graph, p["gconv_input.weight"], p["gconv_input.bias"])
    for i in range(n_layers):
        a = f"atten_layers.{i}."
        lw = [p[a + f"self_attn.linears.{j}.weight"] for j in range(4)]
        lb = [p[a + f"self_attn.linears.{j}.bias"] for j in range(4)]
        y = O.layer_norm(out, p[a + "sublayer.0.norm.a_2"], p[a + "sublayer.0.norm.b_2"])
        out = out + d(attention_train(y, mask, lw, lb, heads, lambda pa: d(pa, (i, 0))), (i, 1))
        y = O.layer_norm(out, p[a + "sublayer.1.norm.a_2"], p[a + "sublayer.1.norm.b_2"])
        out = out + d(O.graph_net(y, p[a + "feed_forward.A_hat"],
                                  p[a + "feed_forward.gconv1.fc.weight"], p[a + "feed_forward.gconv1.fc.bias"],
                                  p[a + "feed_forward.gconv2.fc.weight"], p[a + "feed_forward.gconv2.fc.bias"]), (i, 2))
        g = f"gconv_layers.{i}."
        h = F.relu(d(F.relu(O.cheb_conv(out, graph, p[g + "gconv1.gconv.weight"], p[g + "gconv1.gconv.bias"])), (i, 3)))
        h = h + F.linear(O.swish(temb), p[g + "temb_proj.weight"], p[g + "temb_proj.bias"])[:, None, :]
        h = F.relu(d(F.relu(O.cheb_conv(h, graph, p[g + "gconv2.gconv.weight"], p[g + "gconv2.gconv.bias"])), (i, 4)))
        out = out + h
    return O.cheb_conv(out, graph, p["gconv_output.weight"], p["gconv_output.bias"])


def autograd(i: dict, masks: dict, dtype, weight=None, mask=None, per_pose: bool = False):
    """diff_grad_cases.autograd through forward_train: (per-pose losses, per-pose sum |target - eps|, {name: gradient})"""
    mask = i["mask"] if mask is None else mask
    n = i["x0"].shape[0]
    P = {k: v.clone().requires_grad_(True) for k, v in O.params_to_torch(i["sd"], dtype).items()}
    g = torch.from_numpy(np.asarray(i["adj"])).to(dtype)
    x_t, target, t = i["x_t"].to(dtype), i["target"].to(dtype), i["t"]

    def sums(lo, hi):
        eps = forward_train(P, g, x_t[lo:hi], GC._mask_rows(mask, lo, hi), t[lo:hi], masks, n_layers=i["layers"],
                            heads=i["heads"], lo=lo, hi=hi)
        d = target[lo:hi] - eps
        return d.square().sum(dim=(1, 2)), d.detach().abs().sum(dim=(1, 2))

    names = list(P)
    if not per_pose:
        s, a = sums(0, n)
        total = s.mean(dim=0) if weight is None else (s * weight).sum()
        grads = torch.autograd.grad(total, [P[k] for k in names])
        return s.detach(), a, dict(zip(names, grads))
    acc = {k: torch.zeros_like(P[k]) for k in names}
    losses, absd = [], []
    w = 1.0 / n if weight is None else weight
    for q in range(n):
        s, a = sums(q, q + 1)
        losses.append(s.detach())
        absd.append(a)
        for k, gk in zip(names, torch.autograd.grad((s * w).sum(), [P[k] for k in names])):
            acc[k] = acc[k] + gk
    return torch.cat(losses), torch.cat(absd), acc


def references(i: dict, masks: dict, weight=None, mask=None) -> dict:
    """{"g64", "g32", "gap", "bar", "loss64", "loss_bar"} of one case in train mode (see the module docstring)"""
    l64, a64, g64 = autograd(i, masks, torch.float64, weight, mask)
    _, _, g32 = autograd(i, masks, torch.float32, weight, mask)
    _, _, gpp = autograd(i, masks, torch.float32, weight, mask, per_pose=True)
    gap = {k: max(float((g32[k].double() - g64[k]).abs().max()), float((gpp[k].double() - g64[k]).abs().max()))
           for k in g64}
    bar = {}
    for k, v in gap.items():
        if k.endswith("self_attn.linears.1.bias"):
            v = max(v, gap[k.replace("linears.1.bias", "linears.0.bias")])
        bar[k] = GAP_FACTOR * v
    l64, a64 = l64.numpy(), a64.numpy()
    return dict(g64=g64, g32=g32, gap=gap, bar=bar, loss64=l64, loss_bar=LC.LOSS_REL * (a64 + l64))


@functools.lru_cache(maxsize=None)
def case_masks(name: str, rates=REF_RATES, seed: int = SEED) -> dict:
    """the masks of diff_grad_cases.CASES[name] at ``rates`` under ``seed``, pose0 = 0.  Computed once; do not modify."""
    shape, n = GC.CASES[name]
    return masks_for(shape, n, rates, seed)


@functools.lru_cache(maxsize=None)
def case_references(name: str, rates=REF_RATES, seed: int = SEED) -> dict:
    """references(diff_grad_cases.inputs(name), case_masks(name, rates, seed)).  Computed once; do not modify."""
    return references(GC.inputs(name), case_masks(name, rates, seed))


def golden_g17(load) -> dict:
    """The g17 fixture (tools/gen_goldens_dropout.py) as torch tensors; gradients under "grad.<name>" """
    z = load("g17_train_dropout.npz")
    return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


def g17_inputs(load):
    """(``inputs``, masks, rates, seed) for the fixture's own arrays"""
    z = golden_g17(load)
    t = z["t"].to(torch.float32)
    i = dict(sd=GC.state_dict_of(G17_SHAPE), adj=GC.adj_mx_from_edges(17, GC.H36M_EDGES), layers=2, heads=2, x0=z["x"],
             e=z["e"], scale=z["noise_scale"], t=t, betas=z["betas"], mask=torch.ones(1, 1, 17, dtype=torch.bool),
             x_t=LC.x_t_ref(z["x"], z["e"], z["noise_scale"], t, z["betas"]),
             target=LC.target_ref(z["e"], z["noise_scale"]))
    rates = tuple(float(v) for v in z["rates"])
    seed = int(z["drop_seed"])
    return i, masks_for(G17_SHAPE, z["x"].shape[0], rates, seed), rates, seed
