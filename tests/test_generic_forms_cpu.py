"""CPU: the oracle side of tests/test_gpu_generic_forms.py, which runs the per-op path
(csrc/dpk_generic.inc) at the shapes that reach every kernel form gen_forward chooses between
(edge_inputs.GENERIC_FORM_SHAPES).

The GPU bar there is max|gpu - o64| <= max(5e-6, 8 g) with g = max|o32 - o64| the float32 oracle's own
gap.  That bar is only as tight as g is small, so this file holds g down without a GPU: on every form case
both oracles are finite and g stays under 1e-5 for eps, xs and x0s (measured: 1.4e-7 .. 5.8e-7 for eps,
5.9e-7 .. 2.6e-6 for the K = 3 trajectory).  A g above 1e-5 would stretch the GPU bar past 8e-5 without
anyone having decided so: it fails here instead.  The per-pose key-mask words of the 32-joint row are
packed in numpy (bit 31 included) and pinned, so the GPU test has a fixed target for what the wrapper uploads.
"""
import numpy as np
import pytest
import torch

import edge_inputs as E


@pytest.mark.parametrize("row,n", E.FORM_CASES, ids=[f"{k}-n{n}" for k, n in E.FORM_CASES])
def test_form_case_oracles_finite_and_close(row, n):
    shape = E.GENERIC_FORM_SHAPES[row][0]
    o = E.diff_oracles("forms", shape, n)
    r = E.regime("forms", shape, n=n)
    assert o["eps"][1].shape == (n, shape[3], shape[5]) and o["xs"][1].shape == (4, n, shape[3], shape[5])
    assert r["t"].tolist() == [float(E.FORM_T[i % 7]) for i in range(n)]
    for k, (o32, o64, g) in o.items():
        assert o32.dtype == torch.float32 and o64.dtype == torch.float64
        assert bool(torch.isfinite(o32).all()) and bool(torch.isfinite(o64).all()), (row, k)
        print(f"forms/{row}/n{n}/{k}: g {g:.3e}")
        assert g < E.G_CEILING, f"forms/{row}/n{n}/{k}: the oracle's own gap {g:.3e} would loosen the GPU bar"


def test_form_pose_and_mask_oracles_finite_and_close():
    for mode in ("quirk", "relative", "raw"):
        o = E.pose_oracles("forms", E.FORM_POSE_SHAPE, E.FORM_POSE_N, 3, mode)
        assert o["xyz"][1].shape == (E.FORM_POSE_N, 21, 3) and o["uvxyz"][1].shape == (3 * E.FORM_POSE_N, 21, 5)
        for k, (o32, o64, g) in o.items():
            assert bool(torch.isfinite(o32).all()) and bool(torch.isfinite(o64).all()) and g < E.G_CEILING, (mode, k, g)
    full = E.diff_oracles("forms", E.GENERIC_FORM_SHAPES["j32"][0], 7)["eps"][1]
    for k, (o32, o64, g) in E.form_mask_oracles().items():
        assert bool(torch.isfinite(o32).all()) and bool(torch.isfinite(o64).all()) and g < E.G_CEILING, (k, g)
        # the masks matter: the masked eps is far from the unmasked one on the scale of the bar
        assert float((o64 - full).abs().max()) > 1e3 * E.ABS_BAR, k


def test_pinned_form_sets_are_well_formed():
    """Every pinned set holds exactly one attention form, names only known forms, and the rows together
    with the pinned-BM runs cover all of them (what the GPU file's last test then observes)."""
    union = set()
    for row, (shape, per_n) in E.GENERIC_FORM_SHAPES.items():
        hid, heads = shape[0], shape[1]
        assert hid % heads == 0 and shape[3] <= 32 and len(shape[4]) >= shape[3] - 1
        for n, forms in per_n.items():
            assert forms <= E.ALL_FORMS and len([f for f in forms if f.startswith("attention")]) == 1, (row, n)
            union |= forms
    for row, kinds in E.FORM_BM_ROWS.items():
        union |= {f"gemm<{bm},{v}>" for bm in (128, 64, 32) for v in kinds}
    assert union == E.ALL_FORMS, sorted(E.ALL_FORMS - union)
    assert len(E.ALL_FORMS) == 16


def test_create_refuses_gcndiff_below_hid_4_before_any_device_call():
    """hid_dim 2 and 3 divide by hid_dim // 2 - 1 == 0 in GCNdiff's timestep embedding: DPK_E_UNSUPPORTED from the
    shape check, which runs before any device call (as tests/test_cabi.py's refusals).  The hook rejects a
    null handle."""
    import ctypes

    from diffpose_amd import _lib

    L = _lib.lib()
    h = ctypes.c_void_p()
    for hid in (2, 3):
        c = _lib.DpkConfig(hid, 1, 1, 17, 5, 5, 0)
        assert L.dpk_create(ctypes.byref(c), ctypes.byref(h)) == -2 and not h.value, hid
    w = ctypes.c_uint(7)
    assert L.dpk_debug_generic_forms(None, ctypes.byref(w)) == -1 and w.value == 7


def test_pose_mask_words_of_the_32_joint_row():
    """bit j of word i = key j of pose i attends, as unsigned 32-bit words: bit 31 set on the even poses,
    pose 5 the word 0x80000000 alone.  torch's int32 sum of (bit << j) wraps through INT_MIN to the same
    32 bits, which is what the wrapper uploads (checked on the device by the GPU test)."""
    wide, per = E.form_masks_j32(7)
    want = np.array([0xFFFFFFF7, 0x7FFFFFFF, 0xFFFFFFF7, 0x7FFFFFFF, 0xFFFFFFF7, 0x80000000, 0xFFFFFFF7], dtype=np.uint32)
    got = E.pack_pose_bits(per.numpy())
    assert got.dtype == np.uint32 and np.array_equal(got, want), [hex(int(v)) for v in got]
    # the wrapper's packing (HipGCNdiff.set_mask), on the CPU: int32 words with the same bits
    words = (per.reshape(7, 32) != 0).to(torch.int32)
    bits = (words << torch.arange(32, dtype=torch.int32)).sum(dim=1, dtype=torch.int32)
    assert np.array_equal(bits.numpy().view(np.uint32), want)
    assert int(bits[5]) == -2**31
    assert E.pack_pose_bits(wide.numpy().reshape(1, 32))[0] == 0x7FFFFFFE
