"""CPU: what the train-mode gradient call (dpk_diff_loss_grad_train, dpk_dropout_mask) promises that needs no GPU: the
mask rule's numpy restatement against known answers, the train-mode oracle of tests/dropout_cases.py against the
oracle's own eval-mode forward and against the g17 fixture written by the reference's own train-mode backward
(tools/gen_goldens_dropout.py), the mask coverage of every GPU case, and the interface."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import counter_draws as C
import diff_grad_cases as GC
import dropout_cases as DC
from conftest import ROOT
from diffpose_amd import _lib
from diffpose_amd.weights import param_shapes
from oracle import gcndiff_oracle as O

NEW = ("dpk_diff_loss_grad_train", "dpk_dropout_mask")


# ---------------------------------------------------------------------------------------
# the restatement

def test_rate_zero_keeps_all_and_thresholds():
    assert DC.thr(0.0) == 0 and DC.scale(0.0) == 1.0
    assert DC.keep_mask(DC.SEED, 1, 2, 0.0, 0, 4097).all()
    for p in (0.1, 0.25):
        assert DC.thr(p) == int(np.ceil(float(np.float32(p)) * 2.0 ** 24))       # exact: a power-of-two scaling
        assert DC.scale(p) == float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    assert DC.thr(0.25) == 1 << 22 and DC.thr(0.1) == 1677722                   # float32(0.1) 2^24 = 1677721.625


def test_four_elements_share_one_call():
    q = np.arange(3, 40, dtype=np.uint64)
    words = np.stack(DC.group_words(DC.SEED, 1, 3, q), axis=1)                   # [groups, 4]
    seed = DC.SEED
    direct = np.stack(C.philox4x32_10(q, 0, 1 * 8 + 3, 0xD809, seed & 0xFFFFFFFF, seed >> 32), axis=1)
    assert np.array_equal(words, direct)
    for p in (0.1, 0.25):
        want = ((words >> np.uint32(8)) >= np.uint32(DC.thr(p))).reshape(-1)
        assert np.array_equal(DC.keep_mask(seed, 1, 3, p, 12, 4 * 37), want)
        # an unaligned window of the same elements
        assert np.array_equal(DC.keep_mask(seed, 1, 3, p, 13, 4 * 37 - 6), want[1:-5])
    # the group index's high word is counter word 1
    big = (1 << 34) + 5
    hi = C.philox4x32_10(big & 0xFFFFFFFF, big >> 32, 0, 0xD809, seed & 0xFFFFFFFF, seed >> 32)
    k = DC.keep_mask(seed, 0, 0, 0.25, 4 * big, 4)
    assert np.array_equal(k, np.array([(int(w) >> 8) >= DC.thr(0.25) for w in hi]))


def test_seed_layer_and_site_change_the_mask():
    base = DC.keep_mask(DC.SEED, 0, 1, 0.25, 0, 4096)
    for other in (DC.keep_mask(DC.SEED + 1, 0, 1, 0.25, 0, 4096), DC.keep_mask(DC.SEED + (1 << 32), 0, 1, 0.25, 0, 4096),
                  DC.keep_mask(DC.SEED, 1, 1, 0.25, 0, 4096), DC.keep_mask(DC.SEED, 0, 2, 0.25, 0, 4096)):
        assert 0.3 < float((other != base).mean()) < 0.45                       # independent: 2 p (1 - p) = 0.375


def test_masks_are_not_the_normal_draws():
    """counter word 3 is 0xD809, not the normal draws' 0x5EED: under one seed the mask is not the sign pattern of e"""
    n = 1 << 14
    for step in (-1, 0, 1):
        z, _ = C.normal_ref(DC.SEED, step, np.arange(n, dtype=np.int64))
        for layer, site in ((0, 0), (0, 1)):
            k = DC.keep_mask(DC.SEED, layer, site, 0.5, 0, n)
            agree = float((k == (z > 0)).mean())
            assert 0.45 < agree < 0.55, (step, layer, site, agree)


@pytest.mark.parametrize("p", [0.1, 0.25])
def test_kept_share(p):
    n = 1 << 20
    kept = float(DC.keep_mask(DC.SEED, 0, 1, p, 0, n).mean())
    q = 1.0 - DC.thr(p) / 2.0 ** 24
    assert abs(kept - q) <= 5.0 * np.sqrt(q * (1.0 - q) / n), (kept, q)
    assert abs(q - (1.0 - p)) < 2.0 ** -24


# ---------------------------------------------------------------------------------------
# the train-mode oracle

def test_forward_train_without_masks_is_the_oracle():
    i = GC.inputs("odd")
    shape, n = GC.CASES["odd"]
    P, g = O.params_to_torch(i["sd"]), torch.from_numpy(np.asarray(i["adj"]))
    kw = dict(n_layers=i["layers"], heads=i["heads"])
    with torch.no_grad():
        want = O.gcndiff_forward(P, g, i["x_t"], i["mask"], i["t"], **kw)
        ones = {(l, s): (torch.ones(DC.site_shape(s, n, shape[1], shape[3], shape[0]), dtype=torch.bool), 1.0)
                for l in range(shape[2]) for s in range(5)}
        for masks in ({}, None, ones):
            assert torch.equal(DC.forward_train(P, g, i["x_t"], i["mask"], i["t"], masks, **kw), want)
        some = DC.forward_train(P, g, i["x_t"], i["mask"], i["t"], DC.case_masks("odd"), **kw)
    assert not torch.equal(some, want)


def test_float32_train_oracle_is_the_reference_train_backward(golden):
    """as tests/test_diff_grad_cpu.py holds g16: bitwise"""
    z = DC.golden_g17(golden)
    i, masks, rates, seed = DC.g17_inputs(golden)
    assert rates == DC.REF_RATES and seed == DC.SEED and len(masks) == 10
    assert torch.equal(i["x_t"], z["x_t"])
    sums, _, g32 = DC.autograd(i, masks, torch.float32)
    assert torch.equal(sums, z["sums"]) and torch.equal(sums.mean(dim=0), z["loss_diff"])
    names = [k[5:] for k in z if k.startswith("grad.")]
    assert sorted(names) == sorted(g32) == sorted(param_shapes(hid=32, n_layers=2))
    for k in names:
        assert torch.equal(g32[k], z["grad." + k]), k
    with torch.no_grad():
        eps = DC.forward_train(O.params_to_torch(i["sd"]), torch.from_numpy(i["adj"]), i["x_t"], i["mask"], i["t"], masks,
                               n_layers=2, heads=2)
    assert torch.equal(eps, z["eps"])
    # and it is not the eval-mode step: g16 has the same inputs
    z16 = GC.golden_g16(golden)
    assert torch.equal(z16["x_t"], z["x_t"]) and not torch.equal(z16["eps"], z["eps"])


def test_g17_meta(golden):
    import hashlib
    import json

    meta = json.load(open(os.path.join(ROOT, "tests", "golden", "meta_g17.json")))
    blob = open(os.path.join(ROOT, "tests", "golden", "g17_train_dropout.npz"), "rb").read()
    assert meta["sha256"]["g17_train_dropout.npz"] == hashlib.sha256(blob).hexdigest()
    assert len(meta["kept"]) == 10 and tuple(meta["rates"]) == DC.REF_RATES


# ---------------------------------------------------------------------------------------
# mask coverage of the GPU cases

def test_every_gpu_case_keeps_and_drops_at_every_site(golden):
    for name, rates in DC.GPU_CASES:
        shape = GC.CASES[name][0]
        masks = DC.case_masks(name, rates)
        want = {(l, s) for l in range(shape[2]) for s in range(5) if DC.site_rate(s, rates) != 0}
        assert set(masks) == want and DC.coverage(masks), (name, rates)
    _, masks, _, _ = DC.g17_inputs(golden)
    assert DC.coverage(masks)
    for lo, hi in DC.G17_SHARDS:
        assert DC.coverage(DC.masks_for(DC.G17_SHAPE, hi - lo, DC.REF_RATES, DC.SEED, pose0=lo))
    assert DC.coverage(DC.masks_for(DC.G17_SHAPE, 5, DC.REF_RATES, DC.SEED + 1))


# ---------------------------------------------------------------------------------------
# the interface

def test_new_symbols_in_header_exports_and_library():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "diffpose_kernels.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = set(re.findall(r"\bT (dpk_\w+)", out))
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.EXPORTS and name in syms, name
    assert re.search(r"typedef\s+struct\s*\{\s*float\s+sublayer\s*,\s*attn\s*,\s*gconv\s*;\s*\}\s*dpk_dropout\s*;", src)
    assert _lib.lib().dpk_version() >= 103
    assert [f for f, _ in _lib.DpkDropout._fields_] == ["sublayer", "attn", "gconv"]


def test_refusals_before_any_device_call():
    L = _lib.lib()
    ok = _lib.DpkDropout(0.25, 0.1, 0.1)
    # no handle: DPK_E_INVALID
    assert L.dpk_diff_loss_grad_train(None, None, None, None, 0, None, 0, 0.0, ctypes.byref(ok), 0, 0, None, None, 0,
                                      None) == -1
    assert L.dpk_diff_loss_grad_train(None, None, None, None, 0, None, 0, 0.0, None, 0, 0, None, None, 0, None) == -1
    # the mask exporter has no handle: its refusals, and n = 0, return before a device call
    u64 = ctypes.c_uint64
    for p in (-0.1, 1.0, float("nan")):
        assert L.dpk_dropout_mask(u64(1), 0, 1, ctypes.c_float(p), 0, 0, None, None) == -1, p
    assert L.dpk_dropout_mask(u64(1), -1, 1, ctypes.c_float(0.1), 0, 0, None, None) == -1
    assert L.dpk_dropout_mask(u64(1), 0, 5, ctypes.c_float(0.1), 0, 0, None, None) == -1
    assert L.dpk_dropout_mask(u64(1), 0, 1, ctypes.c_float(0.1), -1, 0, None, None) == -1
    assert L.dpk_dropout_mask(u64(1), 0, 1, ctypes.c_float(0.1), 0, 4, None, None) == -1
    assert L.dpk_dropout_mask(u64(1), 0, 1, ctypes.c_float(0.1), 0, 0, None, None) == 0


def test_python_surface_is_opt_in():
    import inspect

    from diffpose_amd.gcndiff import HipGCNdiff

    sig = inspect.signature(HipGCNdiff.diffusion_loss_grad).parameters
    assert sig["dropout"].default is None and sig["dropout_seed"].default == 0 and sig["pose0"].default == 0
    assert HipGCNdiff.GRAD_FORMS[11:14] == ("attention<train>", "drop_add", "relu_drop")
    assert HipGCNdiff.DROP_SITES == DC.SITES
    assert list(inspect.signature(HipGCNdiff.dropout_mask).parameters)[1:] == ["layer", "site", "p", "seed", "n", "first"]
