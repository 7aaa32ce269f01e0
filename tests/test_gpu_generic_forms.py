"""GPU: the per-op path (csrc/dpk_generic.inc) at shapes that reach every kernel form its host side
chooses between, against the float64 oracle.

gen_forward picks, per call, one of 16 forms from the shape, the batch and pointer alignment: gemm_narrow,
gemm_sk<4|2>, gemm<128|64|32, vec|scalar>, attention<staged+vector | staged+scalar | unstaged>,
graph<staged|unstaged>, cheb_basis<staged|unstaged>.  The other GPU tests run that path at six shapes, all
with hid % 8 == 0, d_k % 4 == 0, hid <= 128 and poses that fit 64 KB of LDS, so most forms never ran.
edge_inputs.GENERIC_FORM_SHAPES lists the shapes here with the forms each must launch; what was launched is
read back from the library (HipGCNdiff.debug_generic_forms, dpk_debug_generic_forms), so a row proves its
form even after someone moves a threshold: the row then fails on its form set, not silently on nothing.

Per row and batch size, under DPK_GEN_FUSED=0: one forward at per-pose t = [0, 1, 7, 24, 49, 500, 999]
cycled, the K = 3 sampler with its trajectory, and the sampler without (the K-step loop recorded as a
hipGraph: bitwise the trajectory's last entry).  The check for eps, xs and x0s is the standing one
(tests/edge_inputs.py): max|gpu - o64| <= max(5e-6, 8 g), finite wherever o32 is, g = max|o32 - o64|
computed here on the CPU (tests/test_generic_forms_cpu.py keeps g under 1e-5).  Deltas go through
conftest.record_delta with tags forms/<row>/n<N>/<tensor>; profiles/generic_forms_deltas.jsonl keeps a run.

The pinned form sets assume a device of at least 200 CUs (an MI355X has 256): the tile-height rule of the
LDS-staged gemm then says 32 rows for every GEMM of these batches.
"""
from types import SimpleNamespace as ns

import numpy as np
import pytest
import torch

import edge_inputs as E
from conftest import record_delta

from diffpose_amd import _lib
from diffpose_amd._lib import DpkError
from diffpose_amd.gcndiff import HipGCNdiff, adj_mx_from_edges
from diffpose_amd.gcnpose import HipGCNpose

pytestmark = pytest.mark.gpu

SEEN = {}        # test id -> forms it read back; test_every_form_ran needs every id below
EXPECTED_IDS = ([f"row/{k}/n{n}" for k, n in E.FORM_CASES] +
                [f"bm/{k}/{bm}" for k in E.FORM_BM_ROWS for bm in (128, 64, 32)] + ["masks/j32", "pose"])


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _cfg(shape, coords=None):
    hid, heads, layers, npts = shape[:4]
    coords = (shape[5], shape[5]) if coords is None else coords
    return ns(model=ns(hid_dim=hid, emd_dim=hid, coords_dim=list(coords), num_layer=layers, n_head=heads,
                       dropout=0.25, n_pts=npts))


def _check(tag, gpu, oracles):
    """max|gpu - o64| <= max(5e-6, 8 g), finite wherever o32 is; returns the failures as text."""
    o32, o64, g = oracles
    gpu = gpu.detach().cpu()
    assert gpu.shape == o64.shape, (tag, gpu.shape, o64.shape)
    finite = bool(torch.isfinite(gpu[torch.isfinite(o32)]).all())
    d = float((gpu.double() - o64).abs().max()) if finite else float("inf")
    ok = record_delta(d, E.bar(g), tag)
    print(f"{tag}: delta {d:.3e}  g {g:.3e}  delta/g {d / g if g > 0 else float('nan'):.2f}  bar {E.bar(g):.3e}")
    return [] if ok and finite else [f"{tag}: delta {d:.3e} > bar {E.bar(g):.3e} (g {g:.3e})"]


def _run_row(dev, row, n, tag, want_forms):
    """eps, the K = 3 trajectory and the recorded loop of one row; returns the forms of all three calls."""
    shape = E.GENERIC_FORM_SHAPES[row][0]
    r = E.regime("forms", shape, n=n)
    o = E.diff_oracles("forms", shape, n)
    bad, seen = [], set()
    m = HipGCNdiff(r["adj"], _cfg(shape), device=dev)
    try:
        m.load_state_dict(r["sd"])
        assert m.gemm_modes() == 1, "expected a per-op handle"
        x, mask, t = r["x"].to(dev), r["mask"].to(dev), r["t"].to(dev)
        eps = m(x, mask, t, 0)
        first = m.debug_generic_forms()
        bad += _check(f"{tag}/eps", eps, o["eps"])
        xs, x0s = m.sample(x, r["seq"], r["betas"], mask=mask, trajectory=True)
        bad += _check(f"{tag}/xs", xs, o["xs"])
        bad += _check(f"{tag}/x0s", x0s, o["x0s"])
        out = m.sample(x, r["seq"], r["betas"], mask=mask)
        assert m.debug_resources()["generic_loop_graphs"] == 1, "expected the recorded K-step loop"
        if not torch.equal(out, xs[-1]):
            bad.append(f"{tag}: the recorded loop differs from the trajectory's last entry by "
                       f"{float((out - xs[-1]).abs().max()):.3e}")
        seen = first | m.debug_generic_forms()
    except RuntimeError as e:      # a library (DpkError) or HIP error, torch's included, is no parity miss:
                                   # run nothing more on the device
        pytest.exit(f"{tag}: {e}", returncode=3)
    finally:
        m.close()
    assert first == set(want_forms), f"{tag}: forms {sorted(first)} != pinned {sorted(want_forms)}"
    assert not bad, "\n".join(bad)
    return seen


@pytest.mark.parametrize("row,n", E.FORM_CASES, ids=[f"{k}-n{n}" for k, n in E.FORM_CASES])
def test_form_rows(dev, monkeypatch, row, n):
    """Each row of edge_inputs.GENERIC_FORM_SHAPES at each of its batch sizes: parity of eps / xs / x0s, the
    recorded loop bitwise, and after the first call exactly the pinned forms (d20: gemm<32,vec> at n = 7,
    where tproj is not 16-byte aligned, and absent at n = 8)."""
    monkeypatch.setenv("DPK_GEN_FUSED", "0")
    monkeypatch.delenv("DPK_GEN_GEMM", raising=False)
    monkeypatch.delenv("DPK_GEN_BM", raising=False)
    SEEN[f"row/{row}/n{n}"] = _run_row(dev, row, n, f"forms/{row}/n{n}", E.GENERIC_FORM_SHAPES[row][1][n])


@pytest.mark.parametrize("bm", [128, 64, 32])
@pytest.mark.parametrize("row", list(E.FORM_BM_ROWS))
def test_pinned_gemm_tiles(dev, monkeypatch, row, bm):
    """The LDS-staged gemm<BM, vec|scalar> pinned by DPK_GEN_GEMM=lds and DPK_GEN_BM at M = 9 x 17 = 153 rows
    (a partial second 128-row tile, a partial third 64-row tile), each against o64 with the same bar.  odd
    runs gemm<BM,scalar> alone, d20 gemm<BM,vec> plus gemm<BM,scalar> for its input ChebConv (K = 15)."""
    monkeypatch.setenv("DPK_GEN_FUSED", "0")
    monkeypatch.setenv("DPK_GEN_GEMM", "lds")
    monkeypatch.setenv("DPK_GEN_BM", str(bm))
    want = E.FORM_NON_GEMM | {f"gemm<{bm},{v}>" for v in E.FORM_BM_ROWS[row]}
    SEEN[f"bm/{row}/{bm}"] = _run_row(dev, row, E.FORM_BM_N, f"forms/{row}/lds{bm}/n{E.FORM_BM_N}", want)


def test_masks_at_32_joints(dev, monkeypatch):
    """j32: eps under a handle-wide mask without keys 0 and 31 and under per-pose masks that set and clear bit
    31 on alternating poses (one pose keeps key 31 alone), against the oracle's masked_fill broadcast; and
    the words the wrapper uploaded for the per-pose case, read back from the device, equal the numpy uint32
    packing (torch's int32 sum wraps through INT_MIN at bit 31)."""
    monkeypatch.setenv("DPK_GEN_FUSED", "0")
    shape, n = E.GENERIC_FORM_SHAPES["j32"][0], 7
    r = E.regime("forms", shape, n=n)
    o = E.form_mask_oracles()
    wide, per = E.form_masks_j32(n)
    bad = []
    m = HipGCNdiff(r["adj"], _cfg(shape), device=dev)
    try:
        m.load_state_dict(r["sd"])
        x, t = r["x"].to(dev), r["t"].to(dev)
        bad += _check("forms/j32/n7/eps_mask_wide", m(x, wide.to(dev), t, 0), o["wide"])
        bad += _check("forms/j32/n7/eps_mask_per", m(x, per.to(dev), t, 0), o["per"])
        bits = m._pose_bits.cpu().numpy()
        SEEN["masks/j32"] = m.debug_generic_forms()
    except RuntimeError as e:
        pytest.exit(f"forms/j32 masks: {e}", returncode=3)
    finally:
        m.close()
    assert bits.dtype == np.int32 and np.array_equal(bits.view(np.uint32), E.pack_pose_bits(per.numpy())), \
        [hex(int(v)) for v in bits.view(np.uint32)]
    assert not bad, "\n".join(bad)


def test_gcnpose_per_op(dev):
    """GCNpose on the per-op path at hid 20 / 5 heads / 2 layers on a 21-joint chain: forward and
    uvxyz(test_times=3) in the three root modes against the float64 oracle; the input ChebConv (K = 6) runs
    gemm<32,scalar>, the output (N = 3) gemm_narrow."""
    shape, n = E.FORM_POSE_SHAPE, E.FORM_POSE_N
    r = E.regime("forms", shape, kind="pose", n=n)
    bad = []
    m = HipGCNpose(r["adj"], _cfg(shape, coords=(2, 3)), device=dev)
    try:
        m.load_state_dict(r["sd"])
        x, mask = r["x"].to(dev), r["mask"].to(dev)
        xyz = m(x, mask)
        forms = m.debug_generic_forms()
        bad += _check("forms/gcnpose/n7/xyz", xyz, E.pose_oracles("forms", shape, n, 3, "raw")["xyz"])
        for mode in ("quirk", "relative", "raw"):
            uv = m.uvxyz(x, mask, test_times=3, root_mode=mode)
            bad += _check(f"forms/gcnpose/n7/uvxyz_{mode}", uv, E.pose_oracles("forms", shape, n, 3, mode)["uvxyz"])
        SEEN["pose"] = forms | m.debug_generic_forms()
    except RuntimeError as e:
        pytest.exit(f"forms/gcnpose: {e}", returncode=3)
    finally:
        m.close()
    assert forms == set(E.FORM_POSE_FORMS), sorted(forms)
    assert {"gemm<32,scalar>", "gemm_narrow"} <= forms
    assert not bad, "\n".join(bad)


def test_create_refuses_gcndiff_below_hid_4(dev):
    """hid_dim 2 and 3 divide by hid // 2 - 1 == 0 in the timestep embedding (the reference raises
    ZeroDivisionError): DPK_E_UNSUPPORTED for GCNdiff, with the wrapper's message; hid 4 is the dk1 row;
    GCNpose, which never evaluates the embedding, still takes hid 2."""
    import ctypes

    L = _lib.lib()
    for hid in (2, 3):
        h = ctypes.c_void_p()
        c = _lib.DpkConfig(hid, 1, 1, 17, 5, 5, dev.index)
        assert L.dpk_create(ctypes.byref(c), ctypes.byref(h)) == -2 and not h.value
        with pytest.raises(DpkError, match="hid_dim >= 4") as ei:
            HipGCNdiff(adj_mx_from_edges(), _cfg((hid, 1, 1, 17, None, 5)), device=dev)
        assert ei.value.code == -2
    h = ctypes.c_void_p()
    c = _lib.DpkConfig(2, 1, 1, 17, 2, 3, dev.index)
    assert L.dpk_create(ctypes.byref(c), ctypes.byref(h)) == 0 and h.value
    L.dpk_destroy(h)


def test_every_form_ran(dev):
    """The union of what the tests above read back is all 16 forms.  Fails when any of them was
    deselected or did not get as far as reading its forms: run the whole file."""
    missing = [i for i in EXPECTED_IDS if i not in SEEN]
    assert not missing, f"not run (the union needs every case of this file): {missing}"
    union = set().union(*SEEN.values())
    assert union == set(E.ALL_FORMS) == set(HipGCNdiff.GENERIC_FORMS), sorted(set(E.ALL_FORMS) ^ union)
