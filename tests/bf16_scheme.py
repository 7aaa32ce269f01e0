"""A torch restatement of gemm mode 2 (bf16) at hid 96 / 4 heads / 17 joints, the cases the bf16 scheme
tests run, and the statistic they compare with (tests/test_bf16_scheme_cpu.py on the CPU,
tests/test_gpu_bf16_scheme.py on the GPU).  Everything comes from fixed seeds; nothing here touches a GPU.

``forward_bf16`` is written from what the project documents of the mode: dpk_set_gemm_mode's text in
include/diffpose_kernels.h, DESIGN.md 3.1 "GEMM modes" and 4.2, and the comments of csrc/dpk_sampler.inc
(attention_mma, gfrag_load_h, graph_mma, gemmh_pass) and csrc/dpk_pack.inc (pack16, bf16_rne, pack_model):
  layer GEMMs  QKV (LayerNorm 0's gain folded into the weight in fp32 before the rounding, its shift into the
               bias, summed in double), O, fc1, fc2 (GraphNet's second Laplacian product applied after the
               GEMM) and the two Chebyshev GEMMs on [x | T1 x | T2 x]: activations rounded to bf16 to
               nearest even, weights rounded to nearest even on the host, products summed in fp32, fp32 biases;
  attention    Q, K, V rounded to bf16; scores summed in fp32, times log2(e) / sqrt(d_k) in fp32 (masked keys
               exactly -1e9), p = 2^score without a max shift while every |score| of the wave is <= 64 and
               some key is kept and key 16 is not masked, 2^(score - max) otherwise; the probabilities of keys
               0..15 rounded to bf16, their P.V and (V's ones rows) their sum from one fp32-accumulated product;
               key 16's term is
               added to both by fp32 FMA from its unrounded probability and its unrounded V row ("O^T = V^T P^T
               over keys 0..15 ..., then key 16 by FMA", attention_mma), for query 16 as for the others; one
               fp32 division;
  graph        X rounded to bf16 against L_g as hi = bf16(L), lo = bf16(L - hi), two products into one fp32
               sum for output joints 0..15; output joint 16 from fp32 L_g and unrounded X;
  fp32         the input and output ChebConvs, the timestep MLP and projections, both LayerNorms, 2^x and the
               normalisation, T1 x = L x and T2 x = 2 L (L x) - x, and the DDIM update.
``acc`` is the dtype the restated products are summed in (float64 is the reference; float32 one of the two
noise variants).  ``depart`` names one deliberate departure from the scheme (DEPARTS); the departures exist
only to show that the bars tell the scheme from its neighbours.

Where this restatement follows the kernel's comments rather than the header's one-line summary:
  * key 16's P.V term and its share of the denominator are fp32 (csrc/dpk_sampler.inc, attention_mma: the
    `fma(p16, V4a, oa) * rs` stores and `den = ... + p16`).  The header and DESIGN.md said "attention's score
    and P.V products" on bf16 MFMA and "joint 16's products as well"; read from the code before any GPU run,
    DESIGN.md 3.1 now says which of joint 16's products those are.  The departure "k16_pv_bf16" is the other
    reading (key 16 rounded like keys 0..15).
Adjusted after a GPU number (the only one): the first GPU run agreed with this file to S = 1.5e-7 .. 5e-7 on every
case but the handle mask without keys {0, 16} (S 1.4e-3 on all poses, and 39 % of the per-pose-mask poses off:
exactly those with key 16 masked).
  * a pose whose key 16 is masked takes the max-shifted softmax (``k16_shifts``).  attention_mma's range test
    reads keys 0..15 from the raw dot products but key 16 from its score after the mask
    (`s_c16[h] = scale(sk16[h][0], kok16)`, then `big2 = fmaxf(big2, fmaxf(fabsf(s_c16[h]), fabsf(s_1616[h])))`
    and `shift = ... !(big <= 64.f)`), so its -1e9 fails the |score| <= 64 test where a masked key 0..15 does
    not.  Both forms are the same softmax; in mode 2 they round the probabilities of the other keys differently
    (2^score against 2^(score - max)).  The kernel's own comment says "masked keys' dot products included", so
    this was a gap in the documents, not in the arithmetic: DESIGN.md 3.1 now states it, the kernel is unchanged.

The statistic: S(a, b) = the median over poses of the per-pose max |a - b|.  A restatement and the kernel
differ by fp32 rounding and summation order only, but that is enough to move an activation across a bf16
rounding boundary now and then, after which that pose rounds independently downstream; S ignores the minority
of poses that met such a flip and sees anything systematic on all of them.
"""
from __future__ import annotations

import functools
import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

import edge_inputs as E
from diffpose_amd.data import synthetic_batch
from diffpose_amd.gcndiff import H36M_EDGES, adj_mx_from_edges
from diffpose_amd.weights import reference_init_state_dict, synthetic_state_dict
from helpers import betas as _betas
from oracle import gcndiff_oracle as O

HEADS = 4
N_EPS, N_SAMPLE = 64, 67                  # dpk_eps: 32 2-pose tiles; dpk_sample: 16 4-pose tiles and a 3-pose tail
SEED_X, SEED_SAMPLE, SEED_JITTER = 4242, 4343, 99
JITTER = 1e-6                             # ~8 fp32 ulps: LayerNorm, v_exp_f32 and MFMA summation order
DEPARTS = ("trunc", "lg_hi_only", "j16_graph_bf16", "p_unrounded", "attention_fp32", "gemm_tail_fp32",
           "weights_trunc", "k16_pv_bf16")
DENSE_EDGES = tuple(H36M_EDGES) + ((3, 16), (6, 13))      # outside the compiled Chebyshev pattern
REGIMES = ("baseline", "zeros", "joints_equal")
# Regimes left out of the GPU file: nearest / noise on the CPU is below 100 (a 1e-6 relative change of a
# layer's input already moves more than half of the poses across a rounding boundary), so no bar separates
# the scheme from its neighbours there.  The measured ratios; test_bf16_scheme_cpu.py re-measures them.
DROPPED_REGIMES = {"x10": 5.5, "plus5": 5.8, "bias+10_ch0": 77.0, "refinit_x10": 1.9}
LOG2E = np.float32(1.4426950408889634)


def rne(v):
    """fp32 -> bf16 -> fp32, round to nearest even (v_cvt_pk_bf16_f32; bf16_rne of csrc/dpk_pack.inc)."""
    return v.float().bfloat16().float()


def trunc(v):
    """fp32 with the low 16 bits cleared: the bf16 conversion that truncates."""
    return (v.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def _mm(a, b, acc):
    return torch.matmul(a.to(acc), b.to(acc)).float()


def forward_bf16(p, graph, x, mask, t, n_layers, heads, *, acc=torch.float64, depart=None, jitter=None,
                 kind="diff", heads_per_wave=2, k16_shifts=True):
    """eps (kind "diff") or xyz (kind "pose": GCNpose, no timestep input) in gemm mode 2's arithmetic.
    ``jitter`` = (s, generator): each layer's input times (1 + s z), z ~ N(0, 1), the second noise variant.
    ``heads_per_wave``: the heads whose scores decide the softmax's max shift together (2 on 2-pose tiles and
    on the 8-wave 4-pose tile, 4 on the 4-wave 4-pose tile; it matters only past |score| = 64)."""
    assert depart is None or depart in DEPARTS, depart
    act = trunc if depart == "trunc" else rne
    wr = trunc if depart == "weights_trunc" else rne
    hid = p["gconv_input.weight"].shape[-1]
    nb, dk = x.size(0), hid // heads
    basis = O.cheb_basis(graph, 3)
    sl = (np.float32(1.0) / np.float32(math.sqrt(dk))) * LOG2E

    def gemm(a, w_kn, b):
        """a [nb, 17, K] fp32 times w_kn [K, N] fp32 in the mode's arithmetic, plus the fp32 bias."""
        y = _mm(act(a), wr(w_kn), acc)
        if depart == "gemm_tail_fp32":
            y = torch.cat([y[:, :16], _mm(a[:, 16:], w_kn, acc)], dim=1)
        return y if b is None else y + b

    def cheb(h, w, b):
        t1 = _mm(basis[1], h, acc)
        t2 = (2.0 * torch.matmul(basis[1].to(acc), t1.to(acc)) - h.to(acc)).float()
        return gemm(torch.cat([h, t1, t2], dim=-1), w.reshape(3 * hid, hid), b)

    def attention(qkv):
        q, k, v = [z.view(nb, -1, heads, dk).transpose(1, 2) for z in qkv.split(hid, dim=-1)]   # [nb, h, 17, dk]
        rq = (lambda z: z) if depart == "attention_fp32" else act
        rp = (lambda z: z) if depart in ("attention_fp32", "p_unrounded") else act
        qb, kb, vb = rq(q), rq(k), rq(v)
        raw = _mm(qb, kb.transpose(-2, -1), acc) * sl                    # log2 units, fp32
        s = raw
        keep = torch.ones(nb, 1, 1, 17, dtype=torch.bool)
        if mask is not None:
            keep = (mask.unsqueeze(1) != 0).expand(nb, 1, 1, 17)
            s = torch.where(keep, raw, torch.full_like(raw, -1e9))
        grp = raw.abs().reshape(nb, heads // heads_per_wave, -1).amax(-1)               # per wave
        k17 = keep.reshape(nb, 17)
        shift = (grp > 64.0).repeat_interleave(heads_per_wave, dim=1) | ~k17.any(-1, keepdim=True)
        if k16_shifts:                   # key 16's score enters the range test after its mask: -1e9 is past 64
            shift = shift | ~k17[:, 16:]
        s = torch.where(shift[:, :, None, None], s - s.amax(-1, keepdim=True), s)
        pr = torch.exp2(s.double()).float()                              # unnormalised probabilities
        pk, vk = rp(pr[..., :16]), vb[..., :16, :]
        p16, v16 = pr[..., 16:], v[..., 16:, :]                          # key 16: fp32 FMA terms
        if depart == "k16_pv_bf16":
            p16, v16 = rp(p16), vb[..., 16:, :]
        num = (torch.matmul(pk.to(acc), vk.to(acc)) + p16.to(acc) * v16.to(acc)).float()
        den = (pk.to(acc).sum(-1, keepdim=True) + p16.to(acc)).float()
        return (num / den).transpose(1, 2).contiguous().view(nb, -1, hid)

    def graph_product(a_hat, xin):
        a = a_hat.numpy().astype(np.float32)
        dh = (np.float32(1.0) / np.sqrt(a.sum(0, dtype=np.float32) + np.float32(1e-5))).astype(np.float32)
        lg = torch.from_numpy((dh[:, None] * a) * dh[None, :])           # dpk_stage.inc's L_g, fp32
        hi = rne(lg)
        lo = torch.zeros_like(lg) if depart == "lg_hi_only" else rne(lg - hi)
        xb = act(xin).to(acc)
        y = (torch.matmul(hi.to(acc), xb) + torch.matmul(lo.to(acc), xb)).float()
        if depart != "j16_graph_bf16":
            y = torch.cat([y[:, :16], _mm(lg[16:], xin, acc)], dim=1)
        return y

    if kind == "diff":
        temb = O.timestep_embedding(t, hid)
        temb = O.swish(F.linear(temb, p["temb.dense.0.weight"], p["temb.dense.0.bias"]))
        temb = F.linear(temb, p["temb.dense.1.weight"], p["temb.dense.1.bias"])
    out = O.cheb_conv(x, graph, p["gconv_input.weight"], p["gconv_input.bias"])
    for i in range(n_layers):
        if jitter is not None:
            out = out * (1.0 + jitter[0] * torch.randn(out.shape, generator=jitter[1]))
        a = f"atten_layers.{i}."
        lw = [p[a + f"self_attn.linears.{j}.weight"] for j in range(4)]
        lb = [p[a + f"self_attn.linears.{j}.bias"] for j in range(4)]
        g0, s0 = p[a + "sublayer.0.norm.a_2"], p[a + "sublayer.0.norm.b_2"]
        n0 = (out - out.mean(-1, keepdim=True)) / (out.std(-1, keepdim=True) + 1e-6)   # LayerNorm 0 without its affine
        wqkv = torch.cat([w.t() for w in lw[:3]], dim=1)                 # [K = hid][3 hid]
        cq = (s0.double() @ wqkv.double() + torch.cat(lb[:3]).double()).float()
        o = attention(gemm(n0, g0[:, None] * wqkv, cq))
        out = out + gemm(o, lw[3].t(), lb[3])
        y = O.layer_norm(out, p[a + "sublayer.1.norm.a_2"], p[a + "sublayer.1.norm.b_2"])
        ah = p[a + "feed_forward.A_hat"]
        h = F.relu(gemm(graph_product(ah, y), p[a + "feed_forward.gconv1.fc.weight"].t(), p[a + "feed_forward.gconv1.fc.bias"]))
        out = out + (graph_product(ah, gemm(h, p[a + "feed_forward.gconv2.fc.weight"].t(), None))
                     + p[a + "feed_forward.gconv2.fc.bias"])
        g = f"gconv_layers.{i}."
        h = F.relu(cheb(out, p[g + "gconv1.gconv.weight"], p[g + "gconv1.gconv.bias"]))
        if kind == "diff":
            h = h + F.linear(O.swish(temb), p[g + "temb_proj.weight"], p[g + "temb_proj.bias"])[:, None, :]
        out = out + F.relu(cheb(h, p[g + "gconv2.gconv.weight"], p[g + "gconv2.gconv.bias"]))
    return O.cheb_conv(out, graph, p["gconv_output.weight"], p["gconv_output.bias"])


# ---- state dicts --------------------------------------------------------------------------------------
_SILENCED = ("atten_layers.{}.self_attn.linears.3.weight", "atten_layers.{}.self_attn.linears.3.bias",
             "atten_layers.{}.feed_forward.gconv2.fc.weight", "atten_layers.{}.feed_forward.gconv2.fc.bias",
             "gconv_layers.{}.gconv2.gconv.weight", "gconv_layers.{}.gconv2.gconv.bias")


def solo_layer_state_dict(sd, i, n_layers=5):
    """``sd`` with the three output projections (weights and biases) of every layer but ``i`` zeroed.  A zero
    weight gives a zero product, relu(0) = 0 and out + 0 = out, so such a layer is the identity exactly and the
    model is the 1-layer model of layer i, run through layer i's slot of every per-layer table."""
    out = OrderedDict((k, np.array(v, dtype=np.float32, copy=True)) for k, v in sd.items())
    for l in range(n_layers):
        if l != i:
            for k in _SILENCED:
                out[k.format(l)][...] = 0.0
    return out


def one_layer_state_dict(sd, i):
    """The 1-layer state dict made of ``sd``'s layer ``i`` (as layer 0) and its input / output / timestep parts."""
    out = OrderedDict()
    for k, v in sd.items():
        for pre in ("atten_layers.", "gconv_layers."):
            if k.startswith(pre):
                l, rest = k[len(pre):].split(".", 1)
                if int(l) == i:
                    out[pre + "0." + rest] = v
                break
        else:
            out[k] = v
    return out


# ---- the statistic --------------------------------------------------------------------------------------
def per_pose(a, b, pose_dim=0):
    """max |a - b| of each pose, float64; ``pose_dim`` is the pose axis (1 for stacked trajectories)."""
    d = (torch.as_tensor(a).detach().cpu().double() - torch.as_tensor(b).detach().cpu().double()).abs()
    d = d.movedim(pose_dim, 0)
    return d.reshape(d.shape[0], -1).amax(-1)


def S(a, b, pose_dim=0):
    """The median over poses of the per-pose max |a - b|."""
    return float(per_pose(a, b, pose_dim).median())


# ---- cases -------------------------------------------------------------------------------------------------
def eps_inputs(n=N_EPS, seed=SEED_X):
    x = torch.from_numpy(synthetic_batch(n, seed=seed)[0])
    t = torch.tensor([E.T_EPS[i % len(E.T_EPS)] for i in range(n)], dtype=torch.float32)
    return x, t


def pose_mask_batch(n=N_EPS):
    """Per-pose key masks: all kept, but key 16 off on every third pose, keys {0, 5} off on poses 1 mod 3,
    one key kept on pose 7 (key 16 alone on pose 8) and none on pose 11."""
    m = torch.ones(n, 1, 17, dtype=torch.bool)
    m[0::3, 0, 16] = False
    m[1::3, 0, 0] = False
    m[1::3, 0, 5] = False
    m[7, 0, :] = False
    m[7, 0, 3] = True
    m[8, 0, :] = False
    m[8, 0, 16] = True
    m[11, 0, :] = False
    return m


def _regime_x(kind, x):
    if kind == "x10":
        return x * 10.0
    if kind == "zeros":
        return torch.zeros_like(x)
    if kind == "joints_equal":
        return x[:, :1].expand_as(x).contiguous()
    if kind == "plus5":
        return x + 5.0
    return x


EPS_CASES = (tuple(f"one/{i}" for i in range(5)) + ("mask_handle", "mask_pose", "refinit", "dense")
             + tuple(f"regime/{r}" for r in REGIMES))
SAMPLE_CASES = ("sample/K1", "sample/K2")
ALL_CASES = EPS_CASES + SAMPLE_CASES + ("pose",)
# The cases tests/test_gpu_sampler_kernels.py adds so that every bf16 kernel of the persistent sampler has one
# (tests/sampler_cells.py holds their bars): the K = 2 sampler on the dense adjacency, with the caller's noise at
# eta 0.5, from the noised hypothesis start, in every combination the kernels are compiled in (flags after
# sample/K2 in this order), and GCNpose on the dense adjacency.
KERNEL_SAMPLE_FLAGS = tuple("".join(f) for f in
                            (("/dense" * d, "/noise" * z, "/start" * st) for d in (0, 1) for z in (0, 1) for st in (0, 1)))
KERNEL_CASES = tuple("sample/K2" + f for f in KERNEL_SAMPLE_FLAGS if f) + ("pose/dense",)
SEED_KERNEL = 4444                        # the caller's noise, the start's draws and its scale


@functools.lru_cache(maxsize=None)
def case(name):
    """One case: state_dict ``sd`` (1 layer), ``adj`` (float32 numpy), ``x``, ``t``, ``mask`` ([1,1,17] or
    [N,1,17] bool), ``kind``; the sampler cases also ``seq`` and ``betas``.  Do not modify."""
    ones = torch.ones(1, 1, 17, dtype=torch.bool)
    sd5 = synthetic_state_dict()
    c = dict(sd=one_layer_state_dict(sd5, 0), adj=adj_mx_from_edges(), mask=ones, kind="diff", layer=0)
    c["x"], c["t"] = eps_inputs()
    if name.startswith("one/"):
        c["layer"] = int(name[4:])
        c["sd"] = one_layer_state_dict(sd5, c["layer"])
    elif name == "mask_handle":
        c["mask"] = ones.clone()
        c["mask"][0, 0, [0, 16]] = False
    elif name == "mask_pose":
        c["mask"] = pose_mask_batch()
    elif name == "refinit":
        c["sd"] = one_layer_state_dict(reference_init_state_dict(0), 0)
    elif name == "dense":
        c["adj"] = adj_mx_from_edges(17, DENSE_EDGES)
    elif name.startswith("regime/"):
        r = name[len("regime/"):]
        c["sd"] = one_layer_state_dict(E.regime(r)["sd"], 0)
        xkind = r if r in E.INPUTS else r[len("refinit_"):] if r.startswith("refinit_") else "baseline"
        c["x"] = _regime_x(xkind, c["x"])
    elif name.startswith("sample/"):
        k = int(name.split("/")[1][1:])
        c["x"] = torch.from_numpy(synthetic_batch(N_SAMPLE, seed=SEED_SAMPLE)[0])
        c["t"] = None
        c["seq"], c["betas"] = {1: [30], 2: [12, 37]}[k], _betas(51)
        flags = name.split("/")[2:]
        assert name in SAMPLE_CASES or name in KERNEL_CASES, name
        g = torch.Generator().manual_seed(SEED_KERNEL)
        z, e = torch.randn((k,) + tuple(c["x"].shape), generator=g), torch.randn(c["x"].shape, generator=g)
        sc = torch.ones(1, 17, 5)
        sc[:, :, :2] = 0.25 + 2.0 * torch.rand((1, 17, 2), generator=g)
        if "dense" in flags:
            c["adj"] = adj_mx_from_edges(17, DENSE_EDGES)
        if "noise" in flags:             # the z of the DDIM update: the caller's draws at eta 0.5
            c["eta"], c["noise"] = E.ETA_NOISE, z
        if "start" in flags:             # x_in is what the kernel is given; the loop runs from x, the torch x_T
            c["start"] = dict(t_start=c["seq"][-1], start_scale=sc, start_noise=e)
            c["x_in"], c["x"] = c["x"], E.start_xT(c["x"], e, sc, c["seq"][-1], c["betas"])
    elif name == "pose/dense":
        c["kind"] = "pose"
        c["sd"] = one_layer_state_dict(synthetic_state_dict(kind="pose"), 0)
        c["adj"] = adj_mx_from_edges(17, DENSE_EDGES)
        c["x"] = c["x"][:, :, :2].contiguous()
        c["t"] = None
    elif name == "pose":
        c["kind"] = "pose"
        c["sd"] = one_layer_state_dict(synthetic_state_dict(kind="pose"), 0)
        c["x"] = c["x"][:, :, :2].contiguous()
        c["t"] = None
    else:
        raise KeyError(name)
    return c


def run(name, fwd=forward_bf16, **kw):
    """The case's output from ``fwd`` (forward_bf16 with ``kw``, or O.gcndiff_forward / O.gcnpose_forward
    through ``oracle``): eps [N,17,5], xyz [N,17,3], or for a sampler case the stack [x0s..., final] [K+1,N,17,5]
    (pose axis 1)."""
    c = case(name)
    P, g = O.params_to_torch(c["sd"]), torch.from_numpy(c["adj"])
    with torch.no_grad():
        if c["kind"] == "pose":
            return fwd(P, g, c["x"], c["mask"], None, 1, HEADS, kind="pose", **kw)
        if c["t"] is not None:
            return fwd(P, g, c["x"], c["mask"], c["t"], 1, HEADS, **kw)
        xs, x0s = O.generalized_steps(c["x"], c["mask"], c["seq"],
                                      lambda a, m, t: fwd(P, g, a, m, t, 1, HEADS, **kw), c["betas"],
                                      eta=c.get("eta", 0.0), noise=c.get("noise"))
        return torch.stack(x0s + [xs[-1]])


def oracle(p, graph, x, mask, t, n_layers, heads, kind="diff"):
    """The fp32 oracle with forward_bf16's signature."""
    if kind == "pose":
        return O.gcnpose_forward(p, graph, x, mask, n_layers, heads)
    return O.gcndiff_forward(p, graph, x, mask, t, n_layers, heads)


def pose_dim(name):
    return 1 if name.startswith("sample/") else 0


@functools.lru_cache(maxsize=None)
def reference(name):
    """forward_bf16(acc=float64) on the case, and ``own`` = max |it - the fp32 oracle|.  Do not modify."""
    ref = run(name)
    own = float((ref.double() - run(name, fwd=oracle).double()).abs().max())
    return ref, own


def scale(name):
    """What a regime case's figures are divided by: the restatement's output magnitude, at least 1."""
    if not name.startswith("regime/"):
        return 1.0
    return max(1.0, float(reference(name)[0].abs().max()))


# Departures a case cannot see, with the reason; test_bf16_scheme_cpu.py asserts that each is as small as said.
# (A departure that leaves a case's output bitwise unchanged is skipped without an entry: key 16's rounding
# where key 16 is masked on every pose, the probabilities' rounding where all joints, hence all scores, are equal.)
BLIND = {
    ("refinit", "lg_hi_only"): "A_hat = I at the reference's initialisation, so L_g = I / (1 + 1e-5): hi = I and "
                               "lo = -1e-5 I, the lo product is 1e-5 of the graph output (S 5.4e-6, 45 x noise)",
}


def figures(name):
    """(noise, nearest, own, the larger share of a noise variant's poses beyond sqrt(noise x nearest),
    {depart: S}) of a case, each S divided by scale(name).  ``nearest`` is the minimum over the departures that
    change the case's output at all and are not in BLIND; an inert departure's entry is exactly 0."""
    ref, own = reference(name)
    pd, sc = pose_dim(name), scale(name)
    gen = torch.Generator().manual_seed(SEED_JITTER)
    variants = [run(name, acc=torch.float32), run(name, jitter=(JITTER, gen))]
    noise = max(S(v, ref, pd) for v in variants) / sc
    dep = {}
    for d in DEPARTS:
        out = run(name, depart=d)
        dep[d] = 0.0 if torch.equal(out, ref) else max(S(out, ref, pd) / sc, 1e-300)
    nearest = min(v for d, v in dep.items() if v > 0.0 and (name, d) not in BLIND)
    b = math.sqrt(noise * nearest) * sc
    beyond = max(float((per_pose(v, ref, pd) > b).double().mean()) for v in variants)
    return noise, nearest, own, beyond, dep
