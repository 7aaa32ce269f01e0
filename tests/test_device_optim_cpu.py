"""CPU: what the device-side optimiser (dpk_train_*) promises that needs no GPU: the host description of the refresh
(csrc/dpk_train_layout.inc as a stand-alone program under the host sanitizers, tests/c/dpk_train_layout_check.cpp), the
float64 model of the step against torch.optim.Adam itself, DeviceAdam's state_dict format, and the refusals that return
before a device is touched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import diff_grad_cases as GC
import optim_cases as OC
from conftest import ROOT
from diffpose_amd import _lib, optim

SRC = os.path.join(ROOT, "tests", "c", "dpk_train_layout_check.cpp")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
NEW = ("dpk_train_begin", "dpk_train_apply", "dpk_train_sync", "dpk_train_get", "dpk_train_set", "dpk_train_end")


def _dims(case):
    hid, heads, layers, npts = GC.CASES[case][0][:4]
    return (hid, heads, npts, layers, 5)


# (hid, heads, joints, layers, coords): the cases' shapes, then 32 joints and the shipped width on one layer
LAYOUT_SHAPES = {"g16": _dims("g16"), "odd": _dims("odd"), "perop": _dims("perop"), "h96": _dims("h96"),
                 "j32": (36, 4, 32, 1, 5), "l1": (96, 4, 17, 1, 5)}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no ROCm clang++")
    path = str(tmp_path_factory.mktemp("trainlayout") / "dpk_train_layout_check")
    subprocess.run([CLANG, "-std=c++17", "-ffp-contract=off", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", SRC, "-o", path], check=True, capture_output=True, text=True)
    return path


@pytest.mark.parametrize("shape", list(LAYOUT_SHAPES.values()), ids=list(LAYOUT_SHAPES))
def test_refresh_description_builds_the_four_arenas_bitwise(exe, shape):
    """every float of the four arenas from the flat parameters through the description == the arenas a weight load
    builds; what the description leaves alone is zero padding or a Chebyshev term; the Laplacian restated is
    stage_load's; host code only, under ASan and UBSan (a report ends the program with an error)"""
    hid, _heads, joints, layers, _coords = shape
    p = subprocess.run([exe] + [str(v) for v in shape], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    rows = {}
    for ln in p.stdout.splitlines():
        w = ln.split()
        rows.setdefault(w[0], []).append(w[1:])
    cheb = int(rows["cheb_nonzero"][0][0])
    assert cheb > 0
    for arena in ("forward", "forward_packed", "transposed", "transposed_packed"):
        floats, mism = next((int(r[1]), int(r[3])) for r in rows[arena] if r[0] == "floats")
        sourced, lg, kept = next((int(r[1]), int(r[3]), int(r[5])) for r in rows[arena] if r[0] == "sourced")
        assert mism == 0 and 0 <= sourced <= floats
        # the unchanged floats that are not zero: the Chebyshev terms, in the two arenas that hold them
        assert kept == (0 if arena.endswith("packed") else cheb), (arena, kept)
        if not arena.endswith("packed"):
            assert lg == layers * joints * joints and sourced > 0.9 * floats
    if hid % 4 == 0:
        assert int(rows["forward_packed"][0][1]) > 0          # the gemm_sk copies exist at this width
    assert rows["unused_params"][0][0] == "0" and rows["laplacian"][0][1] == "0" and rows["decimal"][0][0] == "ok"


@pytest.mark.parametrize("amsgrad", (False, True), ids=("adam", "amsgrad"))
@pytest.mark.parametrize("clip", sorted(OC.CLIPS), ids=sorted(OC.CLIPS))
def test_float64_model_is_torch_adam_in_float64(amsgrad, clip):
    """model64 against clip_grad_norm_ + torch.optim.Adam + EMAHelper's formula in float64: rtol 1e-12 on every array of
    every step"""
    i = OC.inputs("g16")
    c = OC.CLIPS[clip]
    mine = OC.model64(i["params"], i["grads"], amsgrad=amsgrad, clip=c, mu=OC.MU)
    ref, _, _ = OC.torch_adam(i["layout"], i["shapes"], i["params"], i["grads"], torch.float64, amsgrad=amsgrad, clip=c,
                              mu=OC.MU)
    assert mine[0]["gnorm"] > 100.0                            # the active clip (1.0) is active
    assert (mine[0]["coef"] < 1e-2) == (clip == "active")
    # exp_avg is a sum of gradients of either sign: where five of them cancel, the element keeps the rounding of its
    # largest term (torch sums the norm in another order, so its coefficient differs in the last float64 bit), and
    # rtol is taken of that term, max_k |coef_k g_k|, not of what is left (3 of 60,080 elements of g16 cancel below
    # 1e-4 of it).  The moments of second order and the shadow have no cancellation and are held to rtol of the element itself.
    seen = np.zeros(i["F"])
    for n, (a, b, g) in enumerate(zip(mine, ref, i["grads"]), start=1):
        if b["gnorm"] is not None:
            assert a["gnorm"] == pytest.approx(b["gnorm"], rel=1e-12)
        seen = np.maximum(seen, np.abs(a["coef"] * g.astype(np.float64)))
        assert np.all(np.abs(a["exp_avg"] - b["exp_avg"]) <= 1e-12 * np.maximum(np.abs(b["exp_avg"]), seen))
        # likewise a parameter that its updates (each up to about lr) carry through zero: rtol of |p0| + k lr
        k_lr = n * OC.LR
        assert np.all(np.abs(a["params"] - b["params"]) <= 1e-12 * np.maximum(np.abs(b["params"]), np.abs(i["params"]) + k_lr))
        for k in ("exp_avg_sq", "ema") + (("max_exp_avg_sq",) if amsgrad else ()):
            np.testing.assert_allclose(a[k], b[k], rtol=1e-12, atol=0, err_msg=k)
    # twelve decades of exp_avg_sq, and every parameter moved well past one ulp
    v = mine[0]["exp_avg_sq"]
    live = v > 0
    assert v[live].max() / v[live].min() > 1e12
    moved = np.abs(mine[0]["params"] - i["params"].astype(np.float64))[live]
    assert np.median(moved) > 100 * np.spacing(np.float32(np.abs(i["params"]).max()))


def test_bars_are_measured_and_floored():
    ref = OC.bars("g16", amsgrad=True, clip=1.0)
    assert len(ref["bar"]) == 2 * 4 * len(OC.inputs("g16")["layout"])
    for key, bar in ref["bar"].items():
        assert bar >= OC.GAP_FACTOR * ref["gap"][key] and bar > 0
    # the float32 reference itself passes its own yardstick
    i = OC.inputs("g16")
    t32, _, _ = OC.torch_adam(i["layout"], i["shapes"], i["params"], i["grads"], torch.float32, amsgrad=True, clip=1.0)
    for step in (1, OC.STEPS):
        for arr in OC.ARRAYS:
            assert not OC.within(t32[step - 1][arr], "g16", step, arr, ref)


@pytest.mark.parametrize("amsgrad", (False, True), ids=("adam", "amsgrad"))
def test_state_dict_format_interchanges_with_torch_adam(amsgrad):
    """adam_state_dict from flat arrays loads into torch.optim.Adam, which then steps as the optimiser it came from; a
    torch state_dict reads back into the same flat arrays"""
    i = OC.inputs("g16")
    layout, F, shapes = i["layout"], i["F"], i["shapes"]
    steps, opt, ps = OC.torch_adam(layout, shapes, i["params"], i["grads"][:2], torch.float32, amsgrad=amsgrad)
    arrays = {k: torch.from_numpy(steps[-1][k]).float() for k in ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if amsgrad else ())}
    sd = optim.adam_state_dict(layout, shapes, 2, arrays, OC.LR, OC.BETAS, OC.EPS, amsgrad)
    theirs = opt.state_dict()
    assert sorted(sd["state"]) == sorted(theirs["state"]) == list(range(len(layout)))
    for n, st in theirs["state"].items():
        assert sorted(st) == sorted(sd["state"][n])
        for k, v in st.items():
            assert torch.equal(v, sd["state"][n][k]) and v.shape == sd["state"][n][k].shape, (n, k)
    assert sd["param_groups"][0]["params"] == theirs["param_groups"][0]["params"]
    # torch accepts ours and continues exactly as its own optimiser does
    twin = [torch.nn.Parameter(q.detach().clone()) for q in ps]
    opt2 = torch.optim.Adam(twin, lr=OC.LR, betas=OC.BETAS, eps=OC.EPS, amsgrad=amsgrad)
    opt2.load_state_dict(sd)
    g = i["grads"][2]
    for (k, off, n), a, b in zip(layout, ps, twin):
        a.grad = torch.from_numpy(g[off:off + n]).reshape(shapes[k]).clone()
        b.grad = a.grad.clone()
    opt.step(), opt2.step()
    for a, b in zip(ps, twin):
        assert torch.equal(a, b)
    # and the reverse: torch's state dict back into flat arrays, the padding zero
    step, back, group = optim.adam_arrays(opt.state_dict(), layout, F, amsgrad)
    assert step == 3 and group["lr"] == OC.LR
    flat = np.zeros(F, dtype=np.float32)
    for (k, off, n), q in zip(layout, ps):
        flat[off:off + n] = opt.state[q]["exp_avg_sq"].reshape(-1).numpy()
    assert np.array_equal(back["exp_avg_sq"].numpy(), flat)
    # before the first step both are empty
    empty = optim.adam_state_dict(layout, shapes, 0, {}, OC.LR, OC.BETAS, OC.EPS, amsgrad)
    assert empty["state"] == {} and optim.adam_arrays(empty, layout, F, amsgrad)[0] == 0
    with pytest.raises(ValueError):
        optim.adam_arrays(sd, layout, F, not amsgrad)


def test_new_symbols_and_refusals_without_a_device():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "diffpose_kernels.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = set(re.findall(r"\bT (dpk_\w+)", out))
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.EXPORTS and name in syms, name
    assert "dpk_optim_config" in src
    L = _lib.lib()
    assert L.dpk_version() >= 104
    cfg = _lib.DpkOptimConfig(0.9, 0.999, 1e-8, 0, 1.0, 0.999)
    assert ctypes.sizeof(cfg) == 24
    step = ctypes.c_int64(0)
    assert L.dpk_train_begin(None, ctypes.byref(cfg)) == -1
    assert L.dpk_train_apply(None, None, ctypes.c_float(1e-3), None, None) == -1
    assert L.dpk_train_sync(None) == -1
    assert L.dpk_train_get(None, 0, None, ctypes.byref(step), None) == -1
    assert L.dpk_train_set(None, 0, None, -1, None) == -1
    assert L.dpk_train_end(None) == -1


def test_device_optimizer_reads_the_reference_config():
    """config.optim.optimizer other than Adam: NotImplementedError that points at the torch path, before any handle call"""
    from types import SimpleNamespace as ns

    from diffpose_amd.gcndiff import HipGCNdiff

    m = object.__new__(HipGCNdiff)
    m._trainer = None
    for name in ("RMSProp", "SGD"):
        cfg = ns(optim=ns(optimizer=name, lr=1e-3, eps=1e-8, amsgrad=False, grad_clip=1.0), model=ns(ema=True, ema_rate=0.999))
        with pytest.raises(NotImplementedError, match="torch"):
            m.device_optimizer(cfg)
    m._h = None          # nothing for __del__ to destroy
