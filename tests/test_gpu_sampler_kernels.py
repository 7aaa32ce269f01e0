"""GPU: every compiled kernel of the persistent sampler, run once and named by the library.

sample_kernel<MODE, SPARSE, G16, ZM, START, PAD> is compiled 226 times over seven tile namespaces; the host picks
one per launch (csrc/dpk_genfused.inc, launch_sampler in csrc/dpk_kernels.hip).  tests/sampler_cells.py holds one
minimal cell per kernel and the knobs that reach it; what a call launched is read back from the library
(debug_sampler_kernels, dpk_debug_sampler_kernels: written at the launch site from its own template arguments),
so a cell proves its kernel even after someone moves a threshold: it then fails on its id set, not silently on
nothing.  tests/test_sampler_kernels_cpu.py ties the table to the library's list and to the code object's symbols.

Per fp32 / f16x3 cell (2 layers, N = 9, K = 3, "baseline" inputs of edge_inputs.regime): the standing check
max|gpu - o64| <= max(5e-6, 8 g), finite wherever o32 is, on eps; on xs, x0s and the final; or on xyz and
uvxyz(test_times 2, root-relative).  Per bf16 cell: the 1-layer cases, the statistic and the assertions of
tests/test_gpu_bf16_scheme.py (S <= B, half of the poses within B, every pose within 2 own) where the case has a
bar; the cases added for this table all measured a nearest / noise ratio below what that file requires
(sampler_cells.BF16_DROPPED), so their cells assert every pose within 2 own, finiteness and the identities.
Identities, bitwise in every mode: the 8-wave tile equals the 4-wave tile for the same call; a START cell equals
the same tile's plain kernel run from torch's x_T, and its xs[0] is that x_T; out equals the trajectory's last
entry.  Deltas go through conftest.record_delta with tags kernels/<kernel name>/<tensor>;
profiles/sampler_kernels_deltas.jsonl keeps a run.

A library or HIP error ends the session (nothing more runs on the device); the cells of families no other test
file launches run last.
"""
from types import SimpleNamespace as ns

import pytest
import torch

import bf16_scheme as B
import edge_inputs as E
import sampler_cells as C
from conftest import record_delta
from test_gpu_bf16_scheme import BARS as BF16_FILE_BARS

from diffpose_amd import _lib
from diffpose_amd.gcndiff import HipGCNdiff, adj_mx_from_edges
from diffpose_amd.gcnpose import HipGCNpose

pytestmark = pytest.mark.gpu

# Kernels compiled but left out of the union below: none.  Only a family that faulted or hung on the device and
# whose cause was not found may be named here, with the reason, and its cells leave sampler_cells with it.
EXCLUDED = frozenset()

SEEN = {}          # cell name -> the kernels its call reported; test_every_compiled_kernel_ran needs every cell
_HANDLES = {}      # sampler_cells.handle_key -> model, for the module
_RUNS = {}         # cell name -> what its calls returned (a twin cell's outputs are reused by the identities)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    yield torch.device("cuda", 0)
    for m in _HANDLES.values():
        m.close()
    _HANDLES.clear()
    _RUNS.clear()


def _handle(dev, cell):
    """The cell's model with the cell's knobs set: about 20 handles serve the 226 cells."""
    key = C.handle_key(cell)
    if key not in _HANDLES:
        pose = cell.mode == "pose"
        if cell.gemm == "bf16":
            c = B.case(C.bf16_case(cell))
            hid, heads, layers, npts, adj, sd = 96, B.HEADS, 1, 17, c["adj"], c["sd"]
        else:
            shape = C.shape_of(cell)
            r = E.regime("baseline", shape, kind="pose" if pose else "diff")
            (hid, heads, layers, npts), adj, sd = shape[:4], r["adj"], r["sd"]
        cfg = ns(model=ns(hid_dim=hid, emd_dim=hid, coords_dim=[2, 3] if pose else [5, 5], num_layer=layers,
                          n_head=heads, dropout=0.25, n_pts=npts))
        m = (HipGCNpose if pose else HipGCNdiff)(adj, cfg, device=dev)
        _HANDLES[key] = m
        m.load_state_dict(sd)
        assert m.fused == 1, key
    m = _HANDLES[key]
    m.set_gemm_mode(cell.gemm)
    if cell.tile in C.KNOBS:
        plan, waves = C.KNOBS[cell.tile]
        m.set_tail_plan(plan)
        m.set_tile_waves(waves)
    return m


def _sample(m, dev, x, seq, betas, mask, eta, noise, start):
    """The trajectory call and the plain call of one cell, on the CPU: (xs, x0s, out)."""
    kw = dict(eta=eta, mask=mask.to(dev), noise=None if noise is None else noise.to(dev))
    if start is not None:
        kw.update(t_start=start["t_start"], start_scale=start["start_scale"].to(dev),
                  start_noise=start["start_noise"].to(dev))
    xs, x0s = m.sample(x.to(dev), seq, betas, trajectory=True, **kw)
    out = m.sample(x.to(dev), seq, betas, **kw)
    return xs.cpu(), x0s.cpu(), out.cpu()


def _run(dev, cell):
    """The cell's calls, once: its outputs on the CPU, the kernels they reported (``ids``) and, for a START cell,
    the plain kernel's outputs from torch's x_T (``plain``) with the kernels that run reported (``plain_ids``)."""
    if cell.name in _RUNS:
        return _RUNS[cell.name]
    res = {}
    try:
        m = _handle(dev, cell)
        m.debug_sampler_kernels()
        if cell.gemm == "bf16":
            c = B.case(C.bf16_case(cell))
            x, mask = c.get("x_in", c["x"]), c["mask"]
            if cell.mode == "eps":
                res["eps"] = m(x.to(dev), mask.to(dev), c["t"].to(dev), 0).cpu()
            elif cell.mode == "pose":
                res["xyz"] = m(x.to(dev), mask.to(dev)).cpu()
            else:
                args = (c["seq"], c["betas"], mask, c.get("eta", 0.0), c.get("noise"))
                x_T, start = c["x"], c.get("start")
        else:
            shape = C.shape_of(cell)
            r = E.regime("baseline", shape, kind="pose" if cell.mode == "pose" else "diff", noise=bool(cell.zm),
                         start=cell.start)
            x, mask = r["x"], r["mask"]
            if cell.mode == "eps":
                res["eps"] = m(x.to(dev), mask.to(dev), r["t"].to(dev), 0).cpu()
            elif cell.mode == "pose":
                res["xyz"] = m(x.to(dev), mask.to(dev)).cpu()
                res["uvxyz"] = m.uvxyz(x.to(dev), mask.to(dev), test_times=2, root_mode="relative").cpu()
            else:
                args = (r["seq"], r["betas"], mask, r["eta"], r["noise"])
                x_T, start = r["x_T"], ({k: r[k] for k in ("t_start", "start_scale", "start_noise")} if cell.start else None)
        if cell.mode == "sample":
            res["xs"], res["x0s"], res["out"] = _sample(m, dev, x, *args, start)
            res["x_T"] = x_T
        res["ids"] = m.debug_sampler_kernels()
        if cell.start:
            res["plain"] = _sample(m, dev, x_T, *args, None)
            res["plain_ids"] = m.debug_sampler_kernels()
    except RuntimeError as e:      # a library (DpkError) or HIP error, torch's included, is no parity miss:
                                   # run nothing more on the device
        pytest.exit(f"kernels/{cell.name}: {e}", returncode=3)
    _RUNS[cell.name] = res
    return res


def _check(tag, gpu, oracles):
    """max|gpu - o64| <= max(5e-6, 8 g), finite wherever o32 is; returns the failures as text."""
    o32, o64, g = oracles
    assert gpu.shape == o64.shape, (tag, gpu.shape, o64.shape)
    finite = bool(torch.isfinite(gpu[torch.isfinite(o32)]).all())
    d = float((gpu.double() - o64).abs().max()) if finite else float("inf")
    ok = record_delta(d, E.bar(g), tag)
    print(f"{tag}: delta {d:.3e}  g {g:.3e}  bar {E.bar(g):.3e}")
    return [] if ok and finite else [f"{tag}: delta {d:.3e} > bar {E.bar(g):.3e} (g {g:.3e})"]


def _check_bf16(tag, name, gpu):
    """tests/test_gpu_bf16_scheme.py's _check: S <= B, at least half of the poses within B, every pose within
    2 own; a case without a bar (sampler_cells.BF16_DROPPED) keeps the last and finiteness."""
    ref, own = B.reference(name)
    sc = B.scale(name)
    if not (gpu.shape == ref.shape and bool(torch.isfinite(gpu).all())):
        return [f"{tag}: shape {tuple(gpu.shape)} or a non-finite value"]
    pp = B.per_pose(gpu, ref, B.pose_dim(name))
    s, worst = float(pp.median()) / sc, float(pp.max())
    bad = []
    if name in C.BF16_DROPPED:
        print(f"{tag}: S {s:.3e} (no bar: nearest / noise {C.BF16_DROPPED[name]})  worst pose {worst:.3e}  2 own {2 * own:.3e}")
    else:
        bar = (C.BF16_BARS.get(name) or BF16_FILE_BARS[name])[0]
        within = float((pp / sc <= bar).double().mean())
        print(f"{tag}: S {s:.3e}  B {bar:.3e}  poses within B {within:.2f}  worst pose {worst:.3e}  2 own {2 * own:.3e}")
        if not record_delta(s, bar, f"{tag}/S"):
            bad.append(f"{tag}: S {s:.3e} > B {bar:.3e}")
        if within < 0.5:
            bad.append(f"{tag}: {within:.2f} of the poses within B")
    if not record_delta(worst, 2.0 * own, f"{tag}/worst_pose"):
        bad.append(f"{tag}: worst pose {worst:.3e} > 2 own {2 * own:.3e}")
    return bad


def _parity(cell, res):
    tag = f"kernels/{cell.name}"
    if cell.gemm == "bf16":
        name = C.bf16_case(cell)
        gpu = torch.cat([res["x0s"], res["xs"][-1:]]) if cell.mode == "sample" else res["eps" if cell.mode == "eps" else "xyz"]
        return _check_bf16(tag, name, gpu)
    shape = C.shape_of(cell)
    if cell.mode == "pose":
        o = E.pose_oracles("baseline", shape, E.N, 2, "relative")
        return _check(f"{tag}/xyz", res["xyz"], o["xyz"]) + _check(f"{tag}/uvxyz", res["uvxyz"], o["uvxyz"])
    o = E.diff_oracles("baseline", shape, E.N, bool(cell.zm), cell.start)
    if cell.mode == "eps":
        return _check(f"{tag}/eps", res["eps"], o["eps"])
    final = (o["xs"][0][-1], o["xs"][1][-1], E._gap(o["xs"][0][-1], o["xs"][1][-1]))
    return (_check(f"{tag}/xs", res["xs"], o["xs"]) + _check(f"{tag}/x0s", res["x0s"], o["x0s"]) +
            _check(f"{tag}/final", res["out"], final))


def _identities(dev, cell, res):
    """The bitwise identities include/diffpose_kernels.h promises, where both sides exist."""
    bad = []
    if cell.mode != "sample":
        return bad
    if not torch.equal(res["out"], res["xs"][-1]):
        bad.append(f"{cell.name}: out differs from the trajectory's last entry")
    if cell.start:
        if not torch.equal(res["xs"][0], res["x_T"]):
            bad.append(f"{cell.name}: xs[0] is not torch's x_T ({float((res['xs'][0] - res['x_T']).abs().max()):.3e})")
        plain = cell.name.replace("/start", "")
        if res["plain_ids"] != {plain}:
            bad.append(f"{cell.name}: the run from x_T reported {sorted(res['plain_ids'])}, not {plain}")
        for k, v in zip(("xs", "x0s", "out"), res["plain"]):
            a, b = (res[k][1:], v[1:]) if k == "xs" else (res[k], v)
            if not torch.equal(a, b):
                bad.append(f"{cell.name}: {k} differs from the plain kernel run from x_T by {float((a - b).abs().max()):.3e}")
    if cell.tile == "dpk8":
        twin = _run(dev, C.BY_NAME[cell.name.replace("dpk8/", "dpk/", 1)])
        for k in ("xs", "x0s", "out"):
            if not torch.equal(res[k], twin[k]):
                bad.append(f"{cell.name}: {k} differs from the 4-wave tile by {float((res[k] - twin[k]).abs().max()):.3e}")
    return bad


@pytest.mark.parametrize("cell", C.CELLS, ids=[c.name for c in C.CELLS])
def test_cell(dev, cell):
    """One compiled kernel: the call reports exactly this kernel, its outputs pass the cell's parity check and the
    identities hold bitwise."""
    res = _run(dev, cell)
    SEEN[cell.name] = res["ids"]
    assert res["ids"] == {cell.name}, f"launched {sorted(res['ids'])}, the cell pins {cell.name}"
    bad = _parity(cell, res) + _identities(dev, cell, res)
    assert not bad, "\n".join(bad)


def test_a_per_op_handle_reports_no_sampler_kernels(dev, monkeypatch):
    """DPK_FORCE_GENERIC=1 sends the shipped shape per op: its calls leave the census empty."""
    monkeypatch.setenv("DPK_FORCE_GENERIC", "1")
    r = E.regime("baseline")
    m = HipGCNdiff(adj_mx_from_edges(), None, device=dev)
    try:
        m.load_state_dict(r["sd"])
        assert m.fused == 0
        m(r["x"].to(dev), r["mask"].to(dev), r["t"].to(dev), 0)
        assert m.debug_sampler_kernels() == set()
    except RuntimeError as e:
        pytest.exit(f"kernels/per_op: {e}", returncode=3)
    finally:
        m.close()


def test_census_reads_clear_and_count_a_capture_when_recorded(dev):
    """A handle of the shipped shape with no knob set: 9 poses under the default plan run on the 2-pose tile
    alone; a read clears the census; eps and sample in a row report both kernels once; a captured launch is
    reported when it is recorded and its replays add nothing."""
    shape = (96, 4, C.LAYERS, 17, tuple(E.H36M_EDGES))
    r = E.regime("baseline", shape)
    cfg = ns(model=ns(hid_dim=96, emd_dim=96, coords_dim=[5, 5], num_layer=C.LAYERS, n_head=4, dropout=0.25, n_pts=17))
    m = HipGCNdiff(r["adj"], cfg, device=dev)
    try:
        m.load_state_dict(r["sd"])
        x, mask, t = r["x"].to(dev), r["mask"].to(dev), r["t"].to(dev)
        assert m.debug_sampler_kernels() == set()
        eager = m.sample(x, r["seq"], r["betas"], mask=mask).clone()
        assert m.debug_sampler_kernels() == {"dpk2/sample/sparse/fp32/z0"}
        assert m.debug_sampler_kernels() == set()
        m(x, mask, t, 0)
        m.sample(x, r["seq"], r["betas"], mask=mask)
        m.sample(x, r["seq"], r["betas"], mask=mask)
        assert m.debug_sampler_kernels() == {"dpk2/eps/sparse/fp32/z0", "dpk2/sample/sparse/fp32/z0"}
        out = torch.empty_like(x)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            m.sample(x, r["seq"], r["betas"], mask=mask, out=out)
        assert m.debug_sampler_kernels() == {"dpk2/sample/sparse/fp32/z0"}
        g.replay()
        torch.cuda.synchronize()
        assert m.debug_sampler_kernels() == set()
        assert torch.equal(out, eager)
        del g
    except RuntimeError as e:
        pytest.exit(f"kernels/census: {e}", returncode=3)
    finally:
        m.close()


def test_every_compiled_kernel_ran(dev):
    """The union of what the cells read back is every kernel compiled into the library.  Fails when a cell was
    deselected or did not get as far as reading its kernels: run the whole file."""
    missing = [c.name for c in C.CELLS if c.name not in SEEN]
    assert not missing, f"not run (the union needs every cell of this file): {missing[:8]} ... {len(missing)}"
    union = set().union(*SEEN.values())
    compiled = set(_lib.compiled_sampler_kernels())
    assert not EXCLUDED - compiled
    assert union == compiled - EXCLUDED, sorted(union ^ (compiled - EXCLUDED))
