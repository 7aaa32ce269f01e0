"""CPU: where the 5e-6 bar of gemm mode 1 (f16x3) at the other widths comes from.  A restatement of the mode's
arithmetic in torch, against the fp32 oracle (oracle/gcndiff_oracle.py), at the four shapes whose
persistent-sampler instances run the mode (tests/test_gpu_gemm_modes_widths.py holds the GPU to the same bar).

The restatement follows the kernel's arrangement of one layer (csrc/dpk_sampler.inc):
  operands   a = hi + lo with hi = fp16(a), lo = fp16(a - hi); 64 w = hi + lo likewise (csrc/dpk_pack.inc);
  products   lo(w) hi(a) + hi(w) lo(a) + hi(w) hi(a), each product exact in fp32 (11 + 11 significand bits),
             summed in fp32, then / 64 and the bias;
  GEMMs      QKV (LayerNorm 0's gain folded into the weight, its shift into the bias), O, fc1, fc2 (GraphNet's
             second Laplacian product applied after the GEMM) and the two Chebyshev GEMMs on [x | T1 x | T2 x];
  fp32       the input and output ChebConvs, the timestep MLP and projections, LayerNorm, attention, the graph
             and Chebyshev products and the DDIM update.
Only the summation order inside a GEMM differs from the kernel's (fp32 rounding either way).  K = 10 steps on 8
poses keep it within seconds (max |d| 1.8e-7 to 3.0e-7); K = 50 on 24 poses gives 5.4e-7 to 7.2e-7 at these shapes.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from diffpose_amd.data import synthetic_batch
from diffpose_amd.schedule import make_seq
from diffpose_amd.weights import synthetic_state_dict
from helpers import betas as _betas, maxdiff as _maxdiff
from oracle import gcndiff_oracle as O

TOL = 5e-6
SHAPES = [(128, 8, 5), (128, 4, 3), (64, 2, 2), (64, 4, 5)]


def _split(v):
    hi = v.half().float()
    return hi, (v - hi).half().float()


def _gemm16(a, w_kn):
    """a [.., K] fp32 times w_kn [K, N] fp32 by the three-product fp16 split, fp32 accumulation."""
    ah, al = _split(a)
    wh, wl = _split(w_kn * 64.0)
    return (torch.matmul(ah, wl) + torch.matmul(al, wh) + torch.matmul(ah, wh)) / 64.0


def _forward16(p, graph, x, mask, t, n_layers, heads):
    hid = p["gconv_input.weight"].shape[-1]
    temb = O.timestep_embedding(t, hid)
    temb = O.swish(F.linear(temb, p["temb.dense.0.weight"], p["temb.dense.0.bias"]))
    temb = F.linear(temb, p["temb.dense.1.weight"], p["temb.dense.1.bias"])
    basis = O.cheb_basis(graph, 3)
    nb, dk = x.size(0), hid // heads

    def cheb16(h, w, b):
        op = torch.cat([h, torch.matmul(basis[1], h), torch.matmul(basis[2], h)], dim=-1)
        return _gemm16(op, w.reshape(3 * hid, hid)) + b

    out = O.cheb_conv(x, graph, p["gconv_input.weight"], p["gconv_input.bias"])
    for i in range(n_layers):
        a = f"atten_layers.{i}."
        lw = [p[a + f"self_attn.linears.{j}.weight"] for j in range(4)]
        lb = [p[a + f"self_attn.linears.{j}.bias"] for j in range(4)]
        g0, s0 = p[a + "sublayer.0.norm.a_2"], p[a + "sublayer.0.norm.b_2"]
        mu, sd = out.mean(-1, keepdim=True), out.std(-1, keepdim=True)
        n0 = (out - mu) / (sd + 1e-6)                                   # LayerNorm 0 without its affine
        wqkv = torch.cat([w.t() for w in lw[:3]], dim=1)                # [K = hid][3 hid]
        bqkv = torch.cat(lb[:3])
        cq = (s0.double() @ wqkv.double() + bqkv.double()).float()      # the folded bias, summed in double
        qkv = _gemm16(n0, g0[:, None] * wqkv) + cq
        q, k, v = [z.view(nb, -1, heads, dk).transpose(1, 2) for z in qkv.split(hid, dim=-1)]
        scores = torch.matmul(q, k.transpose(-2, -1)) / math.sqrt(dk)
        if mask is not None:
            scores = scores.masked_fill(mask.unsqueeze(1) == 0, -1e9)
        o = torch.matmul(F.softmax(scores, dim=-1), v).transpose(1, 2).contiguous().view(nb, -1, hid)
        out = out + (_gemm16(o, lw[3].t()) + lb[3])
        y = O.layer_norm(out, p[a + "sublayer.1.norm.a_2"], p[a + "sublayer.1.norm.b_2"])
        lap = O.graph_laplacian(p[a + "feed_forward.A_hat"], nb)
        h = F.relu(_gemm16(torch.bmm(lap, y), p[a + "feed_forward.gconv1.fc.weight"].t())
                   + p[a + "feed_forward.gconv1.fc.bias"])
        out = out + (torch.bmm(lap, _gemm16(h, p[a + "feed_forward.gconv2.fc.weight"].t()))
                     + p[a + "feed_forward.gconv2.fc.bias"])
        g = f"gconv_layers.{i}."
        h = F.relu(cheb16(out, p[g + "gconv1.gconv.weight"], p[g + "gconv1.gconv.bias"]))
        h = h + F.linear(O.swish(temb), p[g + "temb_proj.weight"], p[g + "temb_proj.bias"])[:, None, :]
        h = F.relu(cheb16(h, p[g + "gconv2.gconv.weight"], p[g + "gconv2.gconv.bias"]))
        out = out + h
    return O.cheb_conv(out, graph, p["gconv_output.weight"], p["gconv_output.bias"])


@pytest.mark.parametrize("hid,heads,layers", SHAPES)
def test_split_fp16_scheme_stays_within_the_fp32_bar(hid, heads, layers):
    torch.set_num_threads(max(1, min(8, torch.get_num_threads())))
    p = O.params_to_torch(synthetic_state_dict(hid=hid, n_layers=layers))
    graph = O.adjacency()
    x = torch.from_numpy(synthetic_batch(8, seed=300 + hid)[0])
    ones = torch.ones(1, 1, 17, dtype=torch.bool)
    seq = make_seq("uniform", 50, 10)
    ref, _ = O.generalized_steps(x, ones, seq, lambda a, m, t: O.gcndiff_forward(p, graph, a, m, t, layers, heads), _betas())
    got, _ = O.generalized_steps(x, ones, seq, lambda a, m, t: _forward16(p, graph, a, m, t, layers, heads), _betas())
    d = _maxdiff(torch.stack(got), torch.stack(ref))
    print(f"f16x3 scheme vs fp32 oracle, hid {hid} / {heads} heads / {layers} layers, K=10 on 8 poses: max |d| {d:.3e}")
    assert 0.0 < d <= TOL       # not the oracle's own arithmetic, and within the bar
    # one masked eps evaluation at mixed t
    mk = ones.clone()
    mk[0, 0, [0, 16]] = False
    t = torch.arange(8, dtype=torch.float32) * 6.0
    de = _maxdiff(_forward16(p, graph, x, mk, t, layers, heads), O.gcndiff_forward(p, graph, x, mk, t, layers, heads))
    print(f"   eps with a two-key mask: max |d| {de:.3e}")
    assert de <= TOL
