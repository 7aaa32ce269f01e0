"""The caller-memory contract of include/diffpose_kernels.h as a checker and a table of cases, shared by
tests/test_caller_memory_cpu.py (the checker against torch stand-ins that break the contract once each) and
tests/test_gpu_caller_memory.py (every entry point through raw pointers).  No fixtures, and nothing here touches
a GPU at import.

``Guarded`` carves one caller array out of a larger 1-D buffer, [pre | body | post], the whole buffer filled with
one bit pattern: for float arrays a quiet NaN with a payload (a value read from a guard poisons what it feeds, and
the payload, compared through an integer view, still shows a NaN written over a guard), for integer arrays a
pattern of their own dtype.  ``pre`` is 64 elements, or 65 in the misaligned variant: a float pointer is then
4-byte aligned and no more, a double / int64 pointer 8-byte aligned and no more.  ``post`` is a whole tile of every
slice the array holds and never under 64 elements, so what a wrong tail tile writes lands in memory the test owns.

``violations`` / ``check`` look, after one synchronise, for
  guard-before / guard-after   a guard element of any array, inputs included, lost its pattern
  input-modified               an input body is not bitwise what was put in
  unwritten                    an output body element still holds the pattern
  poisoned                     an output element is NaN where the expected tensor is not (a guard was read)
  mismatch                     an output body differs from the expected tensor (bitwise, or beyond its bar)
  touched                      an optional output passed as NULL, or an array of a call over no poses, was written
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np
import torch

PRE, POST_MIN = 64, 64
NAN32, NAN64 = 0x7FC0DEAD, 0x7FF8DEADDEADBEEF
INT32_PATTERN, INT64_PATTERN = 0xDEADBEEF - (1 << 32), 0xDEADBEEFDEADBEEF - (1 << 64)
VIOLATION_KINDS = ("guard-before", "guard-after", "input-modified", "unwritten", "poisoned", "mismatch", "touched")

Violation = namedtuple("Violation", "array kind detail")


def default_pattern(dtype) -> int:
    return {torch.float32: NAN32, torch.float64: NAN64, torch.int32: INT32_PATTERN, torch.int64: INT64_PATTERN}[dtype]


class Guarded:
    """One caller array inside its guards.  ``role``: "in" (never written), "out" (every element written),
    "inout" (an in-place call: given data, then an output) or "untouched" (a valid pointer the call must not
    write: a call over no poses).  ``null``: an optional output passed as NULL (``ptr`` is None).  ``tile``:
    elements of one tile of one slice (4 poses x joints x channels); ``slices``: the leading K or H extent."""

    def __init__(self, name, shape, dtype=torch.float32, device="cpu", role="out", data=None, tile=0, slices=1,
                 misaligned=False, pattern=None, null=False):
        assert role in ("in", "out", "inout", "untouched") and (data is not None) == (role in ("in", "inout"))
        self.name, self.role, self.null, self.dtype = name, role, bool(null), dtype
        self.shape = tuple(int(s) for s in shape)
        self.numel = int(math.prod(self.shape))
        self.itemsize = torch.empty((), dtype=dtype).element_size()
        self.itype = {4: torch.int32, 8: torch.int64}[self.itemsize]
        self.pattern = default_pattern(dtype) if pattern is None else int(pattern)
        self.pre = PRE + (1 if misaligned else 0)
        self.post = max(POST_MIN, int(slices) * int(tile))
        self.raw = torch.full((self.pre + self.numel + self.post,), self.pattern, dtype=self.itype, device=device)
        self.buf = self.raw.view(dtype)
        self.body = self.buf[self.pre:self.pre + self.numel]
        self.given = None
        if data is not None:
            self.given = data.detach().to(device=device, dtype=dtype).reshape(-1).clone()
            assert self.given.numel() == self.numel, (name, tuple(data.shape), self.shape)
            self.body.copy_(self.given)

    @property
    def ptr(self):
        return None if self.null else self.buf.data_ptr() + self.pre * self.itemsize

    def alignment(self) -> int:
        """the largest power of two that divides the body's address"""
        p = self.buf.data_ptr() + self.pre * self.itemsize
        return p & -p

    def view(self):
        return self.body.view(self.shape)


def _first(mask) -> str:
    idx = torch.nonzero(mask.reshape(-1))
    return f"{int(idx.numel())} element(s), first at {int(idx[0])}"


def violations(arrays, expected=None):
    """(violations, deltas) of the Guarded ``arrays`` after a call.  ``expected``: array name -> tensor (bitwise) or
    (tensor, bar) (max |got - want| <= bar) for every "out" / "inout" array that is not null; ``deltas``: name ->
    (max |got - want|, bar) of the barred ones.  The caller synchronises first (``check`` does)."""
    expected = expected or {}
    out, deltas, seen = [], {}, set()
    for g in arrays:
        if id(g) in seen:
            continue
        seen.add(id(g))
        pre, n = g.pre, g.numel
        before, after = g.raw[:pre] != g.pattern, g.raw[pre + n:] != g.pattern
        if bool(before.any()):
            out.append(Violation(g.name, "guard-before", _first(before.flip(0)) + " before the body"))
        if bool(after.any()):
            out.append(Violation(g.name, "guard-after", _first(after) + " past the body"))
        body = g.raw[pre:pre + n]
        if g.null or g.role == "untouched":
            if bool((body != g.pattern).any()):
                out.append(Violation(g.name, "touched", _first(body != g.pattern)))
            continue
        if g.role == "in":
            changed = body != g.given.view(g.itype)
            if bool(changed.any()):
                out.append(Violation(g.name, "input-modified", _first(changed)))
            continue
        unwritten = body == g.pattern
        if bool(unwritten.any()):
            out.append(Violation(g.name, "unwritten", _first(unwritten)))
        want, bar = expected[g.name], None
        if isinstance(want, tuple):
            want, bar = want
        want = want.detach().to(device=g.raw.device, dtype=g.dtype).reshape(-1)
        assert want.numel() == n, (g.name, want.numel(), n)
        got = g.body
        poisoned = torch.zeros_like(unwritten)
        if g.dtype.is_floating_point:
            poisoned = torch.isnan(got) & ~torch.isnan(want) & ~unwritten
            if bool(poisoned.any()):
                out.append(Violation(g.name, "poisoned", _first(poisoned)))
        rest = ~unwritten & ~poisoned
        if bar is None:
            wrong = (body != want.view(g.itype)) & rest
            if bool(wrong.any()):
                d = (got.double() - want.double()).abs()[wrong]
                out.append(Violation(g.name, "mismatch", _first(wrong) + f", max |diff| {float(d.max()):.3e}"))
        else:
            d = (got.double() - want.double()).abs()
            d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
            delta = float(d[rest].max()) if bool(rest.any()) else 0.0
            deltas[g.name] = (delta, float(bar))
            if delta > bar:
                out.append(Violation(g.name, "mismatch", f"max |diff| {delta:.3e} > bar {bar:.3e}"))
    return out, deltas


def check(arrays, expected=None, tag="", record=None):
    """Synchronise once, then assert that ``violations`` finds none; ``record(delta, bar, tag)`` (conftest's
    record_delta) is told every barred comparison."""
    devs = {g.raw.device for g in arrays if g.raw.is_cuda}
    for d in devs:
        torch.cuda.synchronize(d)
    bad, deltas = violations(arrays, expected)
    for name, (delta, bar) in deltas.items():
        if record is not None:
            record(delta, bar, f"{tag}/{name}")
    assert not bad, tag + ": " + "; ".join(f"{v.array}: {v.kind} ({v.detail})" for v in bad)


# ---------------------------------------------------------------------------------------
# the case table: one row per path of the GCNdiff entry points (tests/test_gpu_caller_memory.py)

# n = (a, b): a * CU + b poses, CU the device's compute units (one 4-pose tile per CU per round).
# sample / eps: the tiles (diffpose_amd._lib.SAMPLER_TILES) the launch census must name, () on a per-op handle.
# calls: "eps", "traj" (dpk_sample with xs, x0s), "plain" (both NULL), "noise" (dpk_sample_noise, eta 0.5, the
# caller's draws), "start" (dpk_sample_start with xs).
Row = namedtuple("Row", "name hid heads layers joints graph plan waves gemm n ks sample eps split_dbg calls")
ALL_CALLS = ("eps", "traj", "plain", "noise", "start")


def _row(name, hid, heads, layers, joints, graph, plan, waves, n, sample, eps, gemm="fp32", ks=(3,), split_dbg=0,
         calls=ALL_CALLS):
    return Row(name, hid, heads, layers, joints, graph, plan, waves, gemm, n, ks, sample, eps, split_dbg, calls)


ROWS = {r.name: r for r in (
    # hid 96 / 4 heads / 17 joints: the tile, tail-plan and wave choices
    _row("four", 96, 4, 2, 17, "h36m", "four", 4, (0, 5), ("dpk",), ("dpk",)),
    _row("four8", 96, 4, 2, 17, "h36m", "four", 8, (0, 5), ("dpk8",), ("dpk",)),
    _row("two", 96, 4, 2, 17, "h36m", "two_pose", 4, (0, 5), ("dpk2",), ("dpk2",)),
    _row("mixed", 96, 4, 2, 17, "h36m", "two_pose", 4, (4, 3), ("dpk", "dpk2"), ("dpk", "dpk2")),
    _row("split", 96, 4, 2, 17, "h36m", "step_split", 4, (4, 5), ("dpk",), ("dpk", "dpk2"), ks=(2, 3)),
    _row("split8", 96, 4, 2, 17, "h36m", "step_split", 8, (4, 5), ("dpk8",), ("dpk", "dpk2"), ks=(2, 3)),
    _row("splitfb", 96, 4, 2, 17, "h36m", "step_split", 4, (4, 5), ("dpk",), ("dpk", "dpk2"), split_dbg=1),
    _row("dense", 96, 4, 2, 17, "dense", "four", 4, (0, 5), ("dpk",), ("dpk",)),
    _row("f16x3", 96, 4, 2, 17, "h36m", "four", 0, (0, 5), ("dpk",), (), gemm="f16x3", calls=("traj",)),
    _row("bf16", 96, 4, 2, 17, "h36m", "four", 0, (0, 5), ("dpk8",), (), gemm="bf16", calls=("traj",)),
    # the four other compiled widths (one tile each, no tail plans)
    _row("h128n8", 128, 8, 2, 17, "h36m", None, None, (0, 3), ("dpkw",), ("dpkw",)),
    _row("h128n4", 128, 4, 2, 17, "h36m", None, None, (0, 3), ("dpkw4",), ("dpkw4",)),
    _row("h64n2", 64, 2, 2, 17, "h36m", None, None, (0, 5), ("dpkn",), ("dpkn",)),
    _row("h64n4", 64, 4, 2, 17, "h36m", None, None, (0, 5), ("dpkn4",), ("dpkn4",)),
    # per op: edge_inputs.PER_OP (7 x 16 = 112 rows: three 32-row GEMM tiles and a partial fourth) and
    # edge_inputs.GENERIC_FORM_SHAPES["odd"] (nothing a multiple of 4)
    _row("perop48", 48, 4, 1, 16, "chain", None, None, (0, 7), (), ()),
    _row("perop_odd", 15, 3, 2, 17, "h36m", None, None, (0, 7), (), ()),
)}
INPLACE_ROWS = ("four", "split", "splitfb", "h128n8", "perop_odd")
UPDATE_ROWS = ("four", "h128n8", "perop48")           # dpk_q_sample and dpk_ddim_update(_noise)
PEROP_BAR = 5e-6                                      # the project's standing bar; per-op, misaligned pointers only
SEQS = {2: [0, 25], 3: [0, 17, 34]}                   # K timesteps of the 51-step linear schedule; the last runs first
ETA_NOISE = 0.5
DDIM_ELEMS = (1, 255, 257, 7 * 85)


def n_poses(row, cu: int) -> int:
    return row.n[0] * cu + row.n[1]


def scale_rows(n: int) -> int:
    """rows of the start's scale: 1 where n is prime, else n's smallest divisor above 1"""
    for d in range(2, int(math.isqrt(n)) + 1):
        if n % d == 0:
            return d
    return 1


def pose_masks(n: int, joints: int) -> np.ndarray:
    """[n, 1, joints] bool: pose i drops key (3 i + 1) % joints, odd poses also key (5 i) % joints"""
    m = np.ones((n, 1, joints), dtype=bool)
    i = np.arange(n)
    m[i, 0, (3 * i + 1) % joints] = False
    odd = i[1::2]
    m[odd, 0, (5 * odd) % joints] = False
    return m


def sampler_inputs(n: int, joints: int, k: int, seed: int = 0) -> dict:
    """x, per-pose t, the K step draws z, the start's draws e and its scale (scale_rows(n) rows, u and v
    entries != 1), CPU float32"""
    g = torch.Generator().manual_seed(9100 + 131 * joints + 7 * k + seed)
    x = 0.3 * torch.randn(n, joints, 5, generator=g)
    t_cycle = (0, 1, 7, 24, 49, 50, 33)
    t = torch.tensor([t_cycle[i % len(t_cycle)] for i in range(n)], dtype=torch.float32)
    z = torch.randn(k, n, joints, 5, generator=g)
    e = torch.randn(n, joints, 5, generator=g)
    rows = scale_rows(n)
    sc = torch.ones(rows, joints, 5)
    sc[:, :, :2] = 0.25 + 2.0 * torch.rand(rows, joints, 2, generator=g)
    return dict(x=x, t=t, z=z, e=e, scale=sc)


# ---------------------------------------------------------------------------------------
# dpk_gmm_sample_n / dpk_gmm_sample_f64_n

GMM_F, GMM_SRC, GMM_SEED = 31, 9, 5
GMM_JOINTS, GMM_KERNELS = (2, 17, 32), (1, 5, 64)


def gmm_inputs(joints: int, kernel_n: int, seed: int = GMM_SEED) -> dict:
    """float64 arrays of one dpk_gmm_sample case: gmm [9,J,kn,5] with Dirichlet weights, poses3d [9,J,3], an
    int64 index [31] that wraps and has negative entries, u [31,J]"""
    rng = np.random.Generator(np.random.PCG64(seed))
    w = rng.dirichlet(np.ones(kernel_n), size=(GMM_SRC, joints))
    gmm = np.concatenate([w[..., None], rng.uniform(-1, 1, size=(GMM_SRC, joints, kernel_n, 4))], axis=-1)
    p3 = rng.normal(0.0, 0.5, size=(GMM_SRC, joints, 3)) + 1.0 / 3.0
    index = rng.integers(-3 * GMM_SRC, 3 * GMM_SRC, size=GMM_F).astype(np.int64)
    index[0], index[1], index[2] = -1, GMM_SRC, -2 * GMM_SRC - 4
    u = rng.random((GMM_F, joints))
    return dict(gmm=gmm, poses3d=p3, index=index, u=u)


def gmm_expected(inp: dict, dtype) -> tuple:
    """(uvxyz, noise_scale) [31,J,5] float32 of oracle/gmm_oracle.py on the arrays held as ``dtype``; raises what
    numpy's choice raises when the oracle does not accept the weights"""
    from oracle.gmm_oracle import gmm_item

    atol = float(np.sqrt(np.finfo(np.float64).eps))
    if np.dtype(dtype) == np.float32:
        atol = max(atol, float(np.sqrt(np.finfo(np.float32).eps)))
    g, p3 = inp["gmm"].astype(dtype), inp["poses3d"].astype(dtype)
    rel = p3 - p3[:, :1]
    rows = [gmm_item(rel, g, int(f), inp["u"][i], atol) for i, f in enumerate(inp["index"])]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
