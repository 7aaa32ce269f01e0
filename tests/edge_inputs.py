"""Shared inputs of the numerical-edge tests (tests/test_oracle_fp64.py on the CPU,
tests/test_gpu_input_regimes.py and tests/test_gpu_pose_metrics.py on the GPU): the input / weight /
schedule / mask regimes outside the one every other parity test draws from, the float32 and float64
oracle runs on them, and the degenerate poses of the metrics kernel.  Everything comes from fixed
seeds; nothing here touches a GPU.

The check the GPU tests make with these: with o64 the float64 oracle, o32 the float32 oracle and
g = max|o32 - o64| (per output tensor), a kernel must satisfy max|gpu - o64| <= max(5e-6, 8 g).
5e-6 is the project's standing bar, 6.5x the oracle's own gap on the baseline regime (7.4e-7 ..
7.8e-7), and the kernels achieve about 1x that gap there; 8 g carries the same bar into regimes
whose outputs are not O(1) and never loosens the standing one.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from diffpose_amd.data import synthetic_batch
from diffpose_amd.gcndiff import H36M_EDGES, adj_mx_from_edges
from diffpose_amd.schedule import get_beta_schedule, make_seq
from diffpose_amd.weights import reference_init_state_dict, synthetic_state_dict
from oracle import gcndiff_oracle as O

N = 9                                          # two 4-pose tiles + a 1-pose tail (2-pose tiles: 4 + a tail)
T_EPS = [0, 1, 7, 24, 25, 49, 50, 500, 999]    # per-pose timesteps of the eps cases
ABS_BAR, GAP_FACTOR = 5e-6, 8.0
CHAIN16 = tuple((i, i + 1) for i in range(15))

# (hid, heads, layers, joints, edges): the compiled shape, the two fused wide instances and the per-op path
COMPILED = (96, 4, 5, 17, H36M_EDGES)
WIDE = (128, 8, 3, 17, H36M_EDGES)
NARROW = (64, 2, 2, 17, H36M_EDGES)
PER_OP = (48, 4, 1, 16, CHAIN16)

INPUTS = ("baseline", "x10", "x1000", "zeros", "x1e-6", "joints_equal", "plus5")
BIAS_CASES = tuple(f"bias{v:+d}_{c}" for v in (10, 100) for c in ("ch0", "ch7", "chlast"))
REGIMES = INPUTS + ("T1000",) + BIAS_CASES + ("refinit_x10", "refinit_x1000", "refinit_plus5",
                                                "mask_none_x10", "mask_one_x10")
# the regimes the other model shapes run: the ends of the input range and the bias outliers
SHAPE_REGIMES = ("baseline", "x1000", "plus5") + BIAS_CASES
# GEMM inputs of the f16x3 mode are documented below 65504 (include/diffpose_kernels.h): pixel-scale
# inputs are outside that mode's contract
F16X3_REGIMES = tuple(r for r in REGIMES if "x1000" not in r)
POSE_REGIMES = ("baseline", "x10", "x1000", "zeros", "joints_equal", "bias+10_ch0", "bias+10_ch7")


def bar(g: float) -> float:
    return max(ABS_BAR, GAP_FACTOR * g)


def betas(T: int = 51) -> torch.Tensor:
    return torch.from_numpy(get_beta_schedule("linear", beta_start=1e-4, beta_end=1e-3,
                                              num_diffusion_timesteps=T)).float()


def regime_x(kind: str, npts: int = 17) -> torch.Tensor:
    """The [9, npts, 5] float32 input of an input regime; synthetic_batch(9, seed=3) transformed."""
    x = torch.from_numpy(synthetic_batch(N, seed=3)[0])[:, :npts].contiguous()
    if kind == "baseline":
        return x
    if kind == "x10":
        return x * 10.0
    if kind == "x1000":
        return x * 1000.0
    if kind == "zeros":
        return torch.zeros_like(x)
    if kind == "x1e-6":
        return x * 1e-6
    if kind == "joints_equal":
        return x[:, :1].expand_as(x).contiguous()
    if kind == "plus5":
        return x + 5.0
    raise KeyError(kind)


def _bumped(sd, value: float, channel: int):
    sd = dict(sd)
    b = sd["gconv_input.bias"].copy()
    b[0, 0, channel] += np.float32(value)
    sd["gconv_input.bias"] = b
    return sd


def regime(name: str, shape=COMPILED, kind: str = "diff") -> dict:
    """One regime at a model shape: state_dict ``sd``, adjacency ``adj`` (float32 numpy), input
    ``x``, key ``mask`` [1,1,J] bool, schedule ``betas`` and ``seq`` (K = 3)."""
    hid, heads, layers, npts, edges = shape
    kw = {} if shape == COMPILED else dict(hid=hid, n_layers=layers, n_pts=npts)
    if kind == "pose":
        kw["kind"] = "pose"
    sd = synthetic_state_dict(**kw)
    mask = torch.ones(1, 1, npts, dtype=torch.bool)
    b, seq = betas(51), make_seq("uniform", 51, 3)                  # [0, 17, 34]
    xkind = "baseline"
    if name in INPUTS:
        xkind = name
    elif name == "T1000":
        b, seq = betas(1000), make_seq("uniform", 999, 3)           # [0, 333, 666] on a 1001-entry alpha table
    elif name.startswith("bias"):
        v, c = name[4:].split("_")
        sd = _bumped(sd, float(v), {"ch0": 0, "ch7": 7, "chlast": hid - 1}[c])
    elif name.startswith("refinit_"):
        assert shape == COMPILED and kind == "diff"
        sd, xkind = reference_init_state_dict(0), name[len("refinit_"):]
    elif name.startswith("mask_"):
        xkind = "x10"
        if name.startswith("mask_none"):
            mask[:] = False
        else:
            mask[:] = False
            mask[0, 0, 5] = True
    else:
        raise KeyError(name)
    x = regime_x(xkind, npts)
    if kind == "pose":
        x = x[:, :, :2].contiguous()
    return dict(sd=sd, adj=adj_mx_from_edges(npts, edges), x=x, mask=mask, betas=b, seq=seq,
                layers=layers, heads=heads)


def _gap(a, b) -> float:
    return float((a.double() - b.double()).abs().max())


@functools.lru_cache(maxsize=None)
def diff_oracles(name: str, shape=COMPILED) -> dict:
    """eps at T_EPS and the K=3 trajectory of a regime from the float32 and the float64 oracle:
    {"eps" | "xs" | "x0s": (o32, o64, g)}.  Computed once per (regime, shape); do not modify."""
    r = regime(name, shape)
    t = torch.tensor(T_EPS, dtype=torch.float32)
    out = {}
    for dt in (torch.float32, torch.float64):
        P, g = O.params_to_torch(r["sd"], dt), torch.from_numpy(r["adj"]).to(dt)
        fwd = lambda a, mk, tt: O.gcndiff_forward(P, g, a, mk, tt, n_layers=r["layers"], heads=r["heads"])  # noqa: E731
        with torch.no_grad():
            eps = fwd(r["x"].to(dt), r["mask"], t)
            xs, x0s = O.generalized_steps(r["x"].to(dt), r["mask"], r["seq"], fwd, r["betas"].to(dt))
        out[dt] = {"eps": eps, "xs": torch.stack(xs), "x0s": torch.stack(x0s)}
    return {k: (out[torch.float32][k], out[torch.float64][k], _gap(out[torch.float32][k], out[torch.float64][k]))
            for k in ("eps", "xs", "x0s")}


@functools.lru_cache(maxsize=None)
def pose_oracles(name: str) -> dict:
    """GCNpose's xyz and uvxyz(test_times=2, "relative") of a regime, float32 and float64 oracle."""
    r = regime(name, COMPILED, kind="pose")
    out = {}
    for dt in (torch.float32, torch.float64):
        P, g = O.params_to_torch(r["sd"], dt), torch.from_numpy(r["adj"]).to(dt)
        with torch.no_grad():
            xyz = O.gcnpose_forward(P, g, r["x"].to(dt), r["mask"])
            out[dt] = {"xyz": xyz, "uvxyz": O.build_uvxyz(r["x"].to(dt), xyz, 2, "relative")}
    return {k: (out[torch.float32][k], out[torch.float64][k], _gap(out[torch.float32][k], out[torch.float64][k]))
            for k in ("xyz", "uvxyz")}


# ---- degenerate poses for the metrics kernel ---------------------------------------------------
METRICS_CASES = ("generic", "equal", "similarity", "mirror_z", "mirror_x_noise", "rot180_z", "pred_planar",
                 "both_planar_mirrored", "collinear", "offset", "tiny")


def _rotation(rng) -> np.ndarray:
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def metrics_edge_inputs(F: int = 70, seed: int = 2024):
    """(pred [F,17,3], tgt [F,17,3]) float32; frame i holds case i mod 11 of METRICS_CASES.
    Targets ~ N(0, 0.3^2), PCG64(seed).  F = 70 covers two workgroups of the metrics kernel, the
    second partial."""
    rng = np.random.Generator(np.random.PCG64(seed))
    tgt = rng.normal(0.0, 0.3, size=(F, 17, 3))
    pred = np.empty_like(tgt)
    for i in range(F):
        t = tgt[i]
        noise = rng.normal(0.0, 0.05, size=(17, 3))
        c = i % len(METRICS_CASES)
        if c == 0:
            p = t + noise
        elif c == 1:
            p = t.copy()
        elif c == 2:
            p = 1.7 * t @ _rotation(rng).T + np.array([0.3, -2.0, 5.0])
        elif c == 3:
            p = t * np.array([1.0, 1.0, -1.0])
        elif c == 4:
            p = t * np.array([-1.0, 1.0, 1.0]) + noise
        elif c == 5:
            p = t * np.array([-1.0, -1.0, 1.0])
        elif c == 6:
            p = t + noise
            p[:, 2] = 0.0
        elif c == 7:
            t[:, 2] = 0.0
            p = t * np.array([-1.0, 1.0, 1.0]) + noise
            p[:, 2] = 0.0
        elif c == 8:
            p = np.outer(rng.normal(0.0, 0.3, size=17), np.array([0.6, -0.3, 0.74])) + np.array([0.1, 0.2, -0.1])
        elif c == 9:
            p = t + noise + np.array([0.5, -0.3, 5.0])
        else:
            t *= 1e-6
            p = t + 1e-6 * noise
        pred[i] = p
    return np.ascontiguousarray(pred, dtype=np.float32), np.ascontiguousarray(tgt, dtype=np.float32)
