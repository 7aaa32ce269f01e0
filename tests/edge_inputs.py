"""Shared inputs of the numerical-edge tests (tests/test_oracle_fp64.py and tests/test_generic_forms_cpu.py
on the CPU, tests/test_gpu_input_regimes.py, tests/test_gpu_pose_metrics.py and
tests/test_gpu_generic_forms.py on the GPU; tests/sampler_cells.py builds the persistent sampler's kernel table on
regime / diff_oracles with the caller's noise and the hypothesis start): the input / weight / schedule / mask regimes outside the one
every other parity test draws from, the model shapes that reach every kernel form of the per-op path, the
float32 and float64 oracle runs on them, and the degenerate poses of the metrics kernel.  Everything comes
from fixed seeds; nothing here touches a GPU.

The check the GPU tests make with these: with o64 the float64 oracle, o32 the float32 oracle and
g = max|o32 - o64| (per output tensor), a kernel must satisfy max|gpu - o64| <= max(5e-6, 8 g).
5e-6 is the project's standing bar, 6.5x the oracle's own gap on the baseline regime (7.4e-7 ..
7.8e-7), and the kernels achieve about 1x that gap there; 8 g carries the same bar into regimes
whose outputs are not O(1) and never loosens the standing one.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from diffpose_amd.data import synthetic_batch
from diffpose_amd.gcndiff import H36M_EDGES, adj_mx_from_edges
from diffpose_amd.schedule import alpha_bar_table, get_beta_schedule, make_seq
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


# ---- the per-op path's kernel forms (tests/test_gpu_generic_forms.py, tests/test_generic_forms_cpu.py) ----
# gen_forward (csrc/dpk_generic.inc) picks one form of each kernel per call from the shape, the batch and
# pointer alignment.  Each row below is a model shape (hid, heads, layers, joints, edges, coords), the batch
# sizes it runs at and, per batch size, the forms HipGCNdiff.debug_generic_forms() must report after one
# forward (dpk_eps) under DPK_GEN_FUSED=0, on a device of at least 200 CUs (the tile-height rule then says
# 32 rows for every GEMM here).  The sets are derived by hand from the predicates of csrc/dpk_genplan.inc (gemm_choice,
# attention_choice, graph_choice, cheb_choice: the rule gen_forward launches by; DESIGN.md, "The
# per-op path's kernel forms"), never read off a run.  Inputs: regime("forms", shape, n=N).
FORM_T = (0, 1, 7, 24, 49, 500, 999)          # per-pose timesteps, cycled to N


def _chain(j: int) -> tuple:
    return tuple((i, i + 1) for i in range(j - 1))


# the 32-joint chain closed to a ring plus the chords (i, (7 i + 3) % 32), i = 0, 3, ..., 30: a dense T2
RING32 = _chain(32) + ((31, 0),) + tuple((i, (7 * i + 3) % 32) for i in range(0, 32, 3))

_F_SCALAR = frozenset({"gemm<32,scalar>", "gemm_narrow", "attention<TF>", "graph<T>", "cheb_basis<T>"})
_F_D20 = frozenset({"gemm<32,scalar>", "gemm_sk<4>", "gemm_sk<2>", "gemm_narrow", "attention<TF>", "graph<T>",
                    "cheb_basis<T>"})
GENERIC_FORM_SHAPES = {
    # nothing a multiple of 4: every GEMM scalar (N, K in 15, 30, 45), d_k 5, the temb pad
    "odd": ((15, 3, 2, 17, H36M_EDGES, 5), {7: _F_SCALAR}),
    # coords 4 on odd hid and odd rows: cheb_basis's 4-channel branch with Z only 8-byte aligned
    "odd_c4": ((15, 3, 1, 17, H36M_EDGES, 4), {7: _F_SCALAR}),
    # hid % 8 = 4: scalar attention beside gemm_sk (QKV N = 60 on <4>; N = 20, 40 on <2>, 40 with a padded
    # tile; K tails 20 and 60); tproj = S + 205 M floats is 16-byte aligned at M = 8 x 17 and not at 7 x 17,
    # where the G_RELU_TEMB GEMM leaves gemm_sk for gemm<32,vec>
    "d20": ((20, 5, 2, 17, H36M_EDGES, 5), {7: _F_D20 | {"gemm<32,vec>"}, 8: _F_D20}),
    # d_k 1; every hid- and 2 hid-wide output on gemm_narrow; QKV (N = 12) on gemm_sk<2> with one k-chunk
    "dk1": ((4, 4, 2, 17, H36M_EDGES, 5), {7: frozenset({"gemm_narrow", "gemm_sk<2>", "attention<TF>", "graph<T>",
                                                         "cheb_basis<T>"})}),
    # the joint bound: bit 31 of the mask word
    "j32": ((36, 4, 1, 32, _chain(32), 5), {7: frozenset({"gemm<32,scalar>", "gemm_sk<2>", "gemm_narrow",
                                                          "attention<TF>", "graph<T>", "cheb_basis<T>"})}),
    # two joints; tproj = S + 14 x 405 floats: not 16-byte aligned
    "j2": ((40, 8, 1, 2, _chain(2), 5), {7: _F_D20 | {"gemm<32,vec>"}}),
    "j31c3": ((21, 7, 1, 31, _chain(31), 3), {7: _F_SCALAR}),
    # input ChebConv packed for gemm_sk (K = 36); output ChebConv N = 12 (ldc 12) on gemm<32,vec>
    "c12": ((36, 2, 2, 17, H36M_EDGES, 12), {7: frozenset({"gemm_sk<2>", "gemm<32,vec>", "attention<TF>", "graph<T>",
                                                           "cheb_basis<T>"})}),
    # an input wider than hid: the Chebyshev operand takes 27 floats a row, so As / Fs / Gs behind it are
    # 16-byte aligned at M = 8 x 17 and not at 7 x 17, where attention and graph must not store 16 bytes at
    # a time: attention<TF> for <TT>, and the N = 16 GEMM reads As with scalar loads (gemm_sk<2> stays for QKV)
    "c9": ((8, 2, 1, 17, H36M_EDGES, 9), {7: frozenset({"gemm<32,scalar>", "gemm_sk<2>", "gemm_narrow", "attention<TF>",
                                                        "graph<T>", "cheb_basis<T>"}),
                                          8: frozenset({"gemm<32,scalar>", "gemm_sk<2>", "gemm_narrow", "attention<TT>",
                                                        "graph<T>", "cheb_basis<T>"})}),
    # the staged vector attention (d_k 12, hid % 8 == 0) beside gemm<32,vec>; tproj unaligned
    "tt": ((24, 2, 1, 17, H36M_EDGES, 5), {7: frozenset({"gemm<32,scalar>", "gemm<32,vec>", "gemm_sk<2>",
                                                         "gemm_narrow", "attention<TT>", "graph<T>", "cheb_basis<T>"})}),
    # a pose's QKV rows past 64 KB of LDS at 17 joints; tproj unaligned
    "w320": ((320, 8, 1, 17, H36M_EDGES, 5), {5: frozenset({"gemm<32,scalar>", "gemm<32,vec>", "gemm_sk<4>",
                                                            "gemm_narrow", "attention<FF>", "graph<T>",
                                                            "cheb_basis<T>"})}),
    # graph<F> for the 2 hid operand and graph<T> for the hid operand in one layer
    "w260": ((260, 4, 1, 32, RING32, 5), {5: frozenset({"gemm<32,scalar>", "gemm_sk<2>", "gemm_narrow", "attention<FF>",
                                                        "graph<T>", "graph<F>", "cheb_basis<T>"})}),
    # cheb_basis<F> (the input's stays staged), graph<F> twice, layer_norm past 512, K = 516 (K % 16 = 4),
    # 97 column tiles padded to 98 on gemm_sk<2>
    "w516": ((516, 4, 1, 32, RING32, 5), {5: frozenset({"gemm<32,scalar>", "gemm_sk<2>", "gemm_narrow", "attention<FF>",
                                                        "graph<F>", "cheb_basis<T>", "cheb_basis<F>"})}),
}
FORM_CASES = tuple((k, n) for k, (_, per_n) in GENERIC_FORM_SHAPES.items() for n in per_n)
# the LDS-staged gemm<BM> pinned by DPK_GEN_GEMM=lds and DPK_GEN_BM: M = 9 x 17 = 153 rows, a partial second
# 128-row and a partial third 64-row tile.  odd: all scalar; d20: the input ChebConv (K = 15) stays scalar
FORM_BM_N = 9
FORM_BM_ROWS = {"odd": ("scalar",), "d20": ("vec", "scalar")}
FORM_NON_GEMM = frozenset({"gemm_narrow", "attention<TF>", "graph<T>", "cheb_basis<T>"})
# GCNpose per op: the input ChebConv has K = 6 (scalar), the output N = 3 (narrow)
FORM_POSE_SHAPE = (20, 5, 2, 21, _chain(21))
FORM_POSE_N = 7
FORM_POSE_FORMS = _F_D20
ALL_FORMS = frozenset({"gemm_narrow", "gemm_sk<4>", "gemm_sk<2>", "gemm<128,vec>", "gemm<128,scalar>", "gemm<64,vec>",
                       "gemm<64,scalar>", "gemm<32,vec>", "gemm<32,scalar>", "attention<TT>", "attention<TF>",
                       "attention<FF>", "graph<T>", "graph<F>", "cheb_basis<T>", "cheb_basis<F>"})
G_CEILING = 1e-5       # the oracle's own gap on every form case; above it 8 g would loosen the bar unnoticed


def form_masks_j32(n: int = 7):
    """The key masks of the j32 row: handle-wide without keys 0 and 31, and per pose bit 31 set on even
    poses and cleared on odd ones (key 3 cleared on the even ones), pose 5 keeping key 31 alone."""
    wide = torch.ones(1, 1, 32, dtype=torch.bool)
    wide[0, 0, [0, 31]] = False
    per = torch.ones(n, 1, 32, dtype=torch.bool)
    per[0::2, 0, 3] = False
    per[1::2, 0, 31] = False
    per[5, 0, :] = False
    per[5, 0, 31] = True
    return wide, per


def pack_pose_bits(per) -> np.ndarray:
    """uint32 word per pose, bit j = key j attends: the packing dpk_set_pose_masks documents, in numpy."""
    m = np.asarray(per).reshape(len(per), -1) != 0
    return (m.astype(np.uint32) << np.arange(m.shape[1], dtype=np.uint32)).sum(axis=1, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def form_mask_oracles() -> dict:
    """eps of the j32 row under form_masks_j32: {"wide" | "per": (o32, o64, g)}.  Do not modify."""
    shape, n = GENERIC_FORM_SHAPES["j32"][0], 7
    r = regime("forms", shape, n=n)
    masks = dict(zip(("wide", "per"), form_masks_j32(n)))
    out = {}
    for dt in (torch.float32, torch.float64):
        P, g = O.params_to_torch(r["sd"], dt), torch.from_numpy(r["adj"]).to(dt)
        with torch.no_grad():
            out[dt] = {k: O.gcndiff_forward(P, g, r["x"].to(dt), mk, r["t"], n_layers=r["layers"], heads=r["heads"])
                       for k, mk in masks.items()}
    return {k: (out[torch.float32][k], out[torch.float64][k], _gap(out[torch.float32][k], out[torch.float64][k]))
            for k in masks}


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


ETA_NOISE = 0.5        # eta of the sampler cases that pass the caller's noise
T_START = 34           # the hypothesis start's timestep: the first one the K = 3 sequence [0, 17, 34] executes
START_ROWS = 3         # rows of the start's noise scale: pose n reads row n % 3 (fewer rows than poses)


def start_xT(x, e, scale, t_start: int, b) -> torch.Tensor:
    """x_T = x * a.sqrt() + (e * scale) * (1 - a).sqrt(), a = alpha_bar[t_start + 1] of the betas ``b``
    (runners/diffpose_frame.py:355-363), in torch float32 on the CPU in the reference's order; pose n reads row
    n % S of ``scale`` [S,J,5].  The two square roots are the float64 root rounded once to float32, which is the
    correctly rounded sqrtf the library takes on the host (torch's float32 sqrt is not that on every CPU)."""
    a = torch.from_numpy(alpha_bar_table(b.numpy()))[t_start + 1].view(1, 1, 1)
    root = lambda v: torch.tensor(math.sqrt(float(v)), dtype=torch.float32).view(1, 1, 1)  # noqa: E731
    e = e * scale.repeat(x.shape[0] // scale.shape[0], 1, 1)
    return x * root(a) + e * root(1.0 - a)


def regime(name: str, shape=COMPILED, kind: str = "diff", n: int = N, noise: bool = False,
           start: bool = False) -> dict:
    """One regime at a model shape: state_dict ``sd``, adjacency ``adj`` (float32 numpy), input
    ``x``, per-pose timesteps ``t`` of the eps case, key ``mask`` [1,1,J] bool, schedule ``betas`` and
    ``seq`` (K = 3).  ``shape`` is (hid, heads, layers, joints, edges) with coords [5,5] ([2,3] for
    kind "pose"), or carries the GCNdiff coords as a sixth entry; every regime but "forms" is defined on
    n = 9 poses of 5 (2) channels.
    ``noise``: also ``eta`` = ETA_NOISE and the caller's draws ``noise`` [K,N,J,5] (else eta 0, noise None).
    ``start``: also the hypothesis start at ``t_start`` = T_START with ``start_scale`` [START_ROWS,J,5] (u, v
    entries != 1) and the draws ``start_noise`` [N,J,5], and ``x_T``, the torch expression the loop then starts
    from (start_xT); without it x_T is x."""
    r = _regime(name, shape, kind, n)
    r.update(eta=0.0, noise=None, x_T=r["x"])
    if noise or start:
        assert kind == "diff"
        g = torch.Generator().manual_seed(7000 + r["x"].shape[1])
        z = torch.randn((len(r["seq"]),) + tuple(r["x"].shape), generator=g)
        e = torch.randn(r["x"].shape, generator=g)
        sc = torch.ones((START_ROWS,) + tuple(r["x"].shape[1:]))
        sc[:, :, :2] = 0.25 + 2.0 * torch.rand((START_ROWS, r["x"].shape[1], 2), generator=g)
        if noise:
            r.update(eta=ETA_NOISE, noise=z)
        if start:
            assert r["x"].shape[0] % START_ROWS == 0
            r.update(t_start=T_START, start_scale=sc, start_noise=e, x_T=start_xT(r["x"], e, sc, T_START, r["betas"]))
    return r


def _regime(name: str, shape, kind: str, n: int) -> dict:
    hid, heads, layers, npts, edges = shape[:5]
    coords = 5 if len(shape) == 5 else shape[5]
    kw = {} if shape == COMPILED else dict(hid=hid, n_layers=layers, n_pts=npts)
    if kind == "pose":
        kw["kind"] = "pose"
    elif coords != 5:
        kw["coords"] = (coords, coords)
    sd = synthetic_state_dict(**kw)
    mask = torch.ones(1, 1, npts, dtype=torch.bool)
    b, seq = betas(51), make_seq("uniform", 51, 3)                  # [0, 17, 34]
    t = torch.tensor(T_EPS, dtype=torch.float32)
    if name == "forms":      # the per-op path's form shapes (GENERIC_FORM_SHAPES): any n, joints and coords
        x = torch.randn(n, npts, 2 if kind == "pose" else coords,
                        generator=torch.Generator().manual_seed(100 * hid + npts)) * 0.3
        t = torch.tensor([FORM_T[i % len(FORM_T)] for i in range(n)], dtype=torch.float32)
        return dict(sd=sd, adj=adj_mx_from_edges(npts, edges), x=x, t=t, mask=mask, betas=b, seq=seq,
                    layers=layers, heads=heads)
    assert n == N and (kind == "pose" or coords == 5), (name, shape, n)
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
    return dict(sd=sd, adj=adj_mx_from_edges(npts, edges), x=x, t=t, mask=mask, betas=b, seq=seq,
                layers=layers, heads=heads)


def _gap(a, b) -> float:
    return float((a.double() - b.double()).abs().max())


@functools.lru_cache(maxsize=None)
def diff_oracles(name: str, shape=COMPILED, n: int = N, noise: bool = False, start: bool = False) -> dict:
    """eps at the regime's per-pose t (T_EPS; FORM_T cycled for "forms") and the K=3 trajectory of a
    regime from the float32 and the float64 oracle: {"eps" | "xs" | "x0s": (o32, o64, g)}.  With ``noise`` /
    ``start`` the trajectory is the one of regime(..., noise, start): eta and the caller's draws, and the loop
    started from the float32 x_T (eps stays the forward at x).
    Computed once per (regime, shape, n, noise, start); do not modify."""
    r = regime(name, shape, n=n, noise=noise, start=start)
    t = r["t"]
    out = {}
    for dt in (torch.float32, torch.float64):
        P, g = O.params_to_torch(r["sd"], dt), torch.from_numpy(r["adj"]).to(dt)
        fwd = lambda a, mk, tt: O.gcndiff_forward(P, g, a, mk, tt, n_layers=r["layers"], heads=r["heads"])  # noqa: E731
        with torch.no_grad():
            eps = fwd(r["x"].to(dt), r["mask"], t)
            xs, x0s = O.generalized_steps(r["x_T"].to(dt), r["mask"], r["seq"], fwd, r["betas"].to(dt), eta=r["eta"],
                                          noise=None if r["noise"] is None else r["noise"].to(dt))
        out[dt] = {"eps": eps, "xs": torch.stack(xs), "x0s": torch.stack(x0s)}
    return {k: (out[torch.float32][k], out[torch.float64][k], _gap(out[torch.float32][k], out[torch.float64][k]))
            for k in ("eps", "xs", "x0s")}


@functools.lru_cache(maxsize=None)
def pose_oracles(name: str, shape=COMPILED, n: int = N, test_times: int = 2, root_mode: str = "relative") -> dict:
    """GCNpose's xyz and uvxyz(test_times, root_mode) of a regime, float32 and float64 oracle."""
    r = regime(name, shape, kind="pose", n=n)
    out = {}
    for dt in (torch.float32, torch.float64):
        P, g = O.params_to_torch(r["sd"], dt), torch.from_numpy(r["adj"]).to(dt)
        with torch.no_grad():
            xyz = O.gcnpose_forward(P, g, r["x"].to(dt), r["mask"], n_layers=r["layers"], heads=r["heads"])
            out[dt] = {"xyz": xyz, "uvxyz": O.build_uvxyz(r["x"].to(dt), xyz, test_times, root_mode)}
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
