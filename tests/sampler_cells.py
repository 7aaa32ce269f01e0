"""The persistent sampler's kernels as a table of minimal cases: one cell per compiled
sample_kernel<MODE, SPARSE, G16, ZM, START, PAD> of the seven tile namespaces (csrc/dpk_kernels.hip), shared by
tests/test_sampler_kernels_cpu.py (the table against the library's own list and against the code object's
symbols, the oracle's gap on every cell's inputs) and tests/test_gpu_sampler_kernels.py (each cell run once, the
kernel it launched read back through dpk_debug_sampler_kernels, parity against the float64 oracle).  Nothing
here touches a GPU or the library.

A cell is a handle, the knobs that steer a call to one kernel, one call, and the kernel's name
(_lib.sampler_kernel_name: tile/mode/graph/gemm/z<ZM>[/start][/pad]), which is also the exact id set the call must
report.  Which knob reaches which template argument ("The persistent sampler's kernels"):
  tile    hid 96 / 4 heads: tail plan "four" with 4 waves -> dpk, with 8 waves -> dpk8 (dpk_sample only; on the
          dense graph on explicit request only), plan "two_pose" -> dpk2 (9, 64 or 67 poses are at most two per
          CU, so the whole batch is the tail round); dpk_eps and dpk_pose follow the same plans on 4 waves.  The
          other four widths have one tile each: dpkw 128 / 8, dpkw4 128 / 4, dpkn 64 / 2, dpkn4 64 / 4.
  SPARSE  the H36M adjacency; DENSE_EDGES (two more edges: outside the compiled Chebyshev pattern) for dense.
  G16     set_gemm_mode.
  ZM      1: eta 0.5 and the caller's noise tensor; 0: eta 0 (the counter-based draws at eta > 0 run the ZM = 0
          kernels too and are pinned by tests/test_gpu_counter_draws.py).
  START   t_start, a start_scale of fewer rows than poses and start_noise.
  PAD     a handle of the same width on a 15-joint chain: an odd count, two dead rows per pose.

fp32 and f16x3 cells: 2-layer models (the per-layer offsets of layer 1 are read), the "baseline" inputs of
edge_inputs.regime at N = 9 (two full 4-pose tiles and a 1-pose partial one; four 2-pose tiles and a partial one),
K = 3, per-pose t = T_EPS; the standing check max|gpu - o64| <= max(5e-6, 8 g).
bf16 cells (hid 96 / 4 heads only): the 1-layer cases and the statistic of tests/bf16_scheme.py at its own
N = 64 / 67 (the median needs the poses), with the bars of tests/test_gpu_bf16_scheme.py for the cases that file
has; the cases added here (bf16_scheme.KERNEL_CASES) measured no usable bar (BF16_DROPPED below), so their cells
assert every pose within 2 own, finiteness and the bitwise identities.
"""
from __future__ import annotations

from collections import namedtuple

import bf16_scheme as B
from diffpose_amd._lib import sampler_kernel_id, sampler_kernel_name
from diffpose_amd.gcndiff import H36M_EDGES

# primary tile of each compiled width -> (hid, heads); dpk8 and dpk2 are sibling tiles of dpk
WIDTHS = {"dpk": (96, 4), "dpkw": (128, 8), "dpkw4": (128, 4), "dpkn": (64, 2), "dpkn4": (64, 4)}
SIBLINGS = {"dpk8": "dpk", "dpk2": "dpk"}
TILES = ("dpk", "dpk8", "dpk2", "dpkw", "dpkw4", "dpkn", "dpkn4")
# tile -> (tail plan, tile waves) that reach it; the widths have one tile and keep their defaults
KNOBS = {"dpk": ("four", 4), "dpk8": ("four", 8), "dpk2": ("two_pose", 0)}
LAYERS = 2
DENSE_EDGES = B.DENSE_EDGES
CHAIN15 = tuple((i, i + 1) for i in range(14))
PAD_JOINTS = 15

# Kernels per namespace, by the rules of launch_sample / launch_gemm_mode (csrc/dpk_genfused.inc) and the DPK_INST
# table (csrc/dpk_kernels.hip).  With g the instance's gemm modes (3 at hid 96 / 4 heads, else 2):
#   sample  2 graphs x g x 2 ZM x 2 START = 8 g;  eps, pose  2 graphs x g each;
#   padded (primary tiles only; dense, fp32 and f16x3, no pose)  sample 2 x 2 ZM x 2 START = 8, eps 2.
# dpk = 24 + 6 + 6 + 10, dpk8 = 24 (sample only), dpk2 = 24 + 6 + 6, a width = 16 + 4 + 10.  A new instance, mode
# or flag changes these numbers here and in DESIGN.md before tests/test_sampler_kernels_cpu.py passes again.
COUNTS = {"dpk": 46, "dpk8": 24, "dpk2": 36, "dpkw": 30, "dpkw4": 30, "dpkn": 30, "dpkn4": 30}
TOTAL = 226

# (B, noise, nearest) of the bf16 cases added for this table (bf16_scheme.KERNEL_CASES) that have a bar, from
# bf16_scheme.figures(case) on the CPU, B = sqrt(noise x nearest).  tests/test_bf16_scheme_cpu.py re-measures every
# added case under the conditions that file sets: the two-step sampler cases those of sample/K2 (ratio >= 10, the
# literal within [sqrt(10) noise, nearest / sqrt(10)]), pose/dense those of the one-evaluation cases (ratio >= 100,
# within [10 noise, nearest / 10]).  None of the eight met its condition, so none has a bar today.
BF16_BARS = {
}
# Added cases whose nearest / noise ratio is below what their kind needs, with the measured ratio (like
# bf16_scheme.DROPPED_REGIMES): no bar separates the scheme from its neighbours there, so their cells are covered
# by the bitwise identities (8 waves == 4 waves, START == the plain kernel run from torch's x_T, out == the
# trajectory's last entry), by finiteness and by the scheme's bound on single poses, every pose within 2 own
# (own = max|restatement - fp32 oracle|: a flipped pose is the restatement with some roundings taken independently).
# The median sits at the edge of the flipped minority in all seven sampler cases (45 % of the poses flip at K = 2
# already without them); the dense Chebyshev path, the z term and the start each push a few more poses across.
BF16_DROPPED = {
    "sample/K2/start": 5.2, "sample/K2/noise": 6.5, "sample/K2/noise/start": 1.6, "sample/K2/dense": 2.4,
    "sample/K2/dense/start": 1.8, "sample/K2/dense/noise": 1.7, "sample/K2/dense/noise/start": 2.5,
    "pose/dense": 68.0,
}
BF16_NEED = {"pose/dense": 100.0}          # every sample/K2 case: 10


Cell = namedtuple("Cell", "name tile width mode sparse gemm zm start pad never_run")


def shape_of(cell) -> tuple:
    """(hid, heads, layers, joints, edges) of a fp32 / f16x3 cell's model (edge_inputs.regime's ``shape``)."""
    hid, heads = WIDTHS[cell.width]
    if cell.pad:
        return (hid, heads, LAYERS, PAD_JOINTS, CHAIN15)
    return (hid, heads, LAYERS, 17, tuple(H36M_EDGES) if cell.sparse else DENSE_EDGES)


def handle_key(cell) -> tuple:
    """What the cells that share a handle agree on: the model kind, the width, the graph; the bf16 cells run the
    1-layer models of tests/bf16_scheme.py on handles of their own."""
    kind = "pose" if cell.mode == "pose" else "diff"
    if cell.gemm == "bf16":
        return ("bf16", kind, cell.width, cell.sparse)
    return ("pad" if cell.pad else kind, kind, cell.width, cell.sparse)


def bf16_case(cell) -> str:
    """The bf16_scheme case a bf16 cell runs."""
    if cell.mode == "eps":
        return "one/0" if cell.sparse else "dense"
    if cell.mode == "pose":
        return "pose" if cell.sparse else "pose/dense"
    return "sample/K2" + ("" if cell.sparse else "/dense") + ("/noise" if cell.zm else "") + ("/start" if cell.start else "")


def _never_run(tile, mode, sparse, gemm, zm, start, pad) -> bool:
    """The families no other test file launches, as far as their sources show (they run last)."""
    if mode == "pose" and not sparse:
        return True                                    # GCNpose on a non-H36M adjacency
    if tile == "dpk" and mode in ("eps", "pose") and not pad and (gemm != "fp32" or not sparse):
        return True                                    # dpk_eps / dpk_pose on the 4-pose tile beyond fp32 sparse
    if start and not sparse and not pad:
        return True                                    # START on a dense graph, any width
    if start and zm and gemm == "f16x3" and tile in WIDTHS and tile != "dpk":
        return True                                    # START with the caller's noise in f16x3 at the widths
    if pad and gemm == "f16x3" and (zm or start):
        return True                                    # PAD in f16x3 with ZM = 1 or START
    if tile == "dpk8" and start and gemm == "bf16":
        return True                                    # the 8-wave tile with START in bf16
    return False


def _cells() -> tuple:
    out = []
    for tile in TILES:
        width = SIBLINGS.get(tile, tile)
        gemms = ("fp32", "f16x3") + (("bf16",) if width == "dpk" else ())
        modes = ("sample",) if tile == "dpk8" else ("sample", "eps", "pose") if width == "dpk" else ("sample", "eps")
        for pad in ((False, True) if tile in WIDTHS else (False,)):
            for mode in modes:
                if pad and mode == "pose":
                    continue
                flags = (0, 1) if mode == "sample" else (0,)
                for sparse in ((False,) if pad else (True, False)):
                    for gemm in gemms:
                        if pad and gemm == "bf16":
                            continue
                        for start in flags:
                            for zm in flags:
                                kid = sampler_kernel_id(tile, mode, sparse, gemm, zm, bool(start), pad)
                                out.append(Cell(sampler_kernel_name(kid), tile, width, mode, sparse, gemm, zm,
                                                bool(start), pad,
                                                _never_run(tile, mode, sparse, gemm, zm, bool(start), pad)))
    # the families other tests already run first, the never-run ones last (a fault there ends the session)
    return tuple(sorted(out, key=lambda c: c.never_run))


CELLS = _cells()
BY_NAME = {c.name: c for c in CELLS}
