"""GPU: the gradient of the denoising objective, dpk_diff_loss_grad / HipGCNdiff.diffusion_loss_grad /
runner.Diffpose.train_step, against the references and bars of tests/diff_grad_cases.py (whose yardstick
tests/test_diff_grad_cpu.py pins to the reference's own loss_diff.backward()): every parameter tensor of every case
within 8 x the oracle's own gap to the float64 gradient, the per-pose loss within diff_loss_cases' bar."""
import ctypes
import functools
from types import SimpleNamespace as ns

import numpy as np
import pytest
import torch

import caller_memory as CM
import counter_draws as C
import diff_grad_cases as GC
from conftest import record_delta
from diffpose_amd import _lib
from diffpose_amd._lib import DpkError
from diffpose_amd.gcndiff import HipGCNdiff, adj_mx_from_edges
from diffpose_amd.schedule import make_seq, training_timesteps

pytestmark = pytest.mark.gpu

BWD_FORMS, BWD_FORMS_W320, GEMM_FORMS = GC.BWD_FORMS, GC.BWD_FORMS_W320, GC.GEMM_FORMS


def ends_session(fn):
    """A library / HIP error is no parity miss: run nothing more on the device."""
    @functools.wraps(fn)
    def run(*a, **k):
        try:
            return fn(*a, **k)
        except DpkError as e:
            pytest.exit(f"diff_grad/{fn.__name__}: {e}", returncode=3)
        except RuntimeError as e:
            if "HIP error" in str(e) or "hipError" in str(e):
                pytest.exit(f"diff_grad/{fn.__name__}: {e}", returncode=3)
            raise
    return run


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _config(shape, dropout=0.25):
    hid, heads, layers, npts = shape[:4]
    coords = 5 if len(shape) == 5 else shape[5]
    return ns(model=ns(hid_dim=hid, emd_dim=hid, coords_dim=[coords, coords], num_layer=layers, n_head=heads,
                       dropout=dropout, n_pts=npts))


def _model(shape, sd, dev):
    m = HipGCNdiff(adj_mx_from_edges(shape[3], shape[4]), _config(shape), device=dev)
    m.load_state_dict(sd)
    return m


@pytest.fixture(scope="module")
def models(dev):
    """One model per case shape for the whole module"""
    made = {}

    def get(name):
        shape = GC.CASES[name][0]
        if shape not in made:
            made[shape] = _model(shape, GC.inputs(name)["sd"], dev)
        return made[shape]

    yield get
    for m in made.values():
        m.close()


@pytest.fixture(scope="module")
def g16(golden):
    """(inputs, references) of the g16 fixture, computed once; do not modify"""
    i = GC.g16_inputs(golden)
    return i, GC.references(i)


def _grad(m, i, dev, **kw):
    args = dict(noise_scale=i["scale"].to(dev), noise=i["e"].to(dev), mask=i["mask"].to(dev))
    args.update(kw)
    return m.diffusion_loss_grad(i["x0"].to(dev), i["t"], i["betas"], **args)


def _check(tag, loss, grads, ref, scale=1.0):
    """every tensor within its bar of the float64 gradient (``scale``: the factor the gradients carry over the
    reference's), the loss within its bar per pose; every delta recorded"""
    ok = True
    assert list(grads) == list(ref["g64"])
    for k, g64 in ref["g64"].items():
        got = grads[k].detach().cpu().double() / scale
        assert got.shape == g64.shape, k
        ok = record_delta(float((got - g64).abs().max()), ref["bar"][k], f"{tag}/{k}") and ok
    ratio = np.abs(loss.cpu().double().numpy() - ref["loss64"]) / ref["loss_bar"]
    ok = record_delta(float(ratio.max()), 1.0, f"{tag}/loss") and ok
    assert ok, tag


# ---------------------------------------------------------------------------------------
# 1. g16: the fixture's inputs

@ends_session
def test_g16_fixture(dev, golden, g16):
    z, (i, ref) = GC.golden_g16(golden), g16
    m = _model(GC.G16_SHAPE, i["sd"], dev)
    try:
        assert m.fused == 0
        dx = {k: i[k].to(dev) for k in ("x0", "scale", "e")}
        t = i["t"].to(dev)
        keep = {k: v.clone() for k, v in dx.items()}
        m.debug_grad_forms()
        loss, grads = m.diffusion_loss_grad(dx["x0"], t, i["betas"], noise_scale=dx["scale"], noise=dx["e"])
        fwd, bwd = m.debug_grad_forms()
        _check("diff_grad/g16", loss, grads, ref)
        assert fwd == GEMM_FORMS["g16"] and bwd == BWD_FORMS, (fwd, bwd)
        # the reference's own p.grad: the float64 gradient is the yardstick, the fixture within the same bars of it
        for k, g in grads.items():
            assert float((z["grad." + k].double() - ref["g64"][k]).abs().max()) <= ref["bar"][k], k
            assert tuple(g.shape) == tuple(z["grad." + k].shape)
        # twice: bitwise; inputs unchanged
        loss2, grads2 = m.diffusion_loss_grad(dx["x0"], t, i["betas"], noise_scale=dx["scale"], noise=dx["e"])
        assert torch.equal(grads.flat, grads2.flat) and torch.equal(loss, loss2)
        for k in dx:
            assert torch.equal(dx[k], keep[k]), k
        assert torch.equal(t.cpu(), i["t"])
        # weight 0.37: 0.37 N times the default's gradients
        loss3, grads3 = m.diffusion_loss_grad(dx["x0"], t, i["betas"], noise_scale=dx["scale"], noise=dx["e"], weight=0.37)
        assert torch.equal(loss3, loss)
        _check("diff_grad/g16/w0.37", loss3, grads3, ref, scale=0.37 * 5)
    finally:
        m.close()


# ---------------------------------------------------------------------------------------
# 2., 3. shapes that reach the other kernel forms

@pytest.mark.parametrize("name", ["odd", "perop", "j32", "w320"])
@ends_session
def test_per_op_shapes(dev, models, name):
    m, i, ref = models(name), GC.inputs(name), GC.case_references(name)
    assert m.fused == 0
    m.debug_grad_forms()
    loss, grads = _grad(m, i, dev)
    fwd, bwd = m.debug_grad_forms()
    _check(f"diff_grad/{name}", loss, grads, ref)
    assert bwd == (BWD_FORMS_W320 if name == "w320" else BWD_FORMS), bwd
    if name in GEMM_FORMS:
        assert fwd == GEMM_FORMS[name], fwd


# ---------------------------------------------------------------------------------------
# 4. handles with a persistent-sampler instance

@pytest.mark.parametrize("name", ["h96", "pad15"])
@ends_session
def test_persistent_sampler_handles(dev, models, name):
    m, i, ref = models(name), GC.inputs(name), GC.case_references(name)
    assert m.fused == 1
    x, seq = i["x0"].to(dev), make_seq("uniform", 51, 3)
    kw = dict(noise_scale=i["scale"].to(dev), noise=i["e"].to(dev), mask=i["mask"].to(dev))
    sample0 = m.sample(x, seq, i["betas"], mask=kw["mask"])
    dl0 = m.diffusion_loss(x, i["t"], i["betas"], **kw)
    loss, grads = _grad(m, i, dev)
    _check(f"diff_grad/{name}", loss, grads, ref)
    assert m.fused == 1 and m.debug_grad_forms()[1] == BWD_FORMS
    assert torch.equal(m.sample(x, seq, i["betas"], mask=kw["mask"]), sample0)
    assert torch.equal(m.diffusion_loss(x, i["t"], i["betas"], **kw), dl0)
    _, again = _grad(m, i, dev)
    assert torch.equal(again.flat, grads.flat)


# ---------------------------------------------------------------------------------------
# 5. masks

@ends_session
def test_masks(dev, models):
    m, i = models("g16"), GC.inputs("g16")
    n = i["x0"].shape[0]
    one_off = torch.ones(1, 1, 17, dtype=torch.bool)
    one_off[0, 0, 5] = False
    per = torch.from_numpy(CM.pose_masks(n, 17))
    try:
        for tag, mk in (("handle", one_off), ("per_pose", per)):
            loss, grads = _grad(m, i, dev, mask=mk.to(dev))
            _check(f"diff_grad/mask/{tag}", loss, grads, GC.references(i, mask=mk))
    finally:
        m.set_mask(None)


# ---------------------------------------------------------------------------------------
# 6. row partitions, NULL scale, counter-based draws

@pytest.mark.parametrize("name", ["g16_n40", "g16_n1"])
@ends_session
def test_row_partitions(dev, models, name):
    m, i = models(name), GC.inputs(name)
    loss, grads = _grad(m, i, dev)
    _check(f"diff_grad/{name}", loss, grads, GC.case_references(name))
    _, again = _grad(m, i, dev)
    assert torch.equal(again.flat, grads.flat)


@ends_session
def test_grad_honours_gemm_switches(dev, g16, monkeypatch):
    """DPK_GEN_GEMM=lds and DPK_GEN_BM=64 reach every per-op GEMM of the gradient call (the training forward's and
    the dX GEMMs go through the launch layer gen_forward uses), are read per call, and leave nothing behind."""
    i, ref = g16
    m = _model(GC.G16_SHAPE, i["sd"], dev)
    try:
        plain_loss, plain = _grad(m, i, dev)
        monkeypatch.setenv("DPK_GEN_GEMM", "lds")
        monkeypatch.setenv("DPK_GEN_BM", "64")
        m.debug_grad_forms()
        loss, grads = _grad(m, i, dev)
        fwd, _ = m.debug_grad_forms()
        assert not {f for f in fwd if f.startswith("gemm_sk<")}, fwd
        assert {f for f in fwd if f.startswith("gemm<")} == {"gemm<64,vec>", "gemm<64,scalar>"}, fwd
        _check("diff_grad/g16/lds64", loss, grads, ref)
        loss2, grads2 = _grad(m, i, dev)
        assert torch.equal(grads2.flat, grads.flat) and torch.equal(loss2, loss)
        monkeypatch.delenv("DPK_GEN_GEMM")
        monkeypatch.delenv("DPK_GEN_BM")
        loss3, grads3 = _grad(m, i, dev)
        assert torch.equal(grads3.flat, plain.flat) and torch.equal(loss3, plain_loss)
    finally:
        m.close()


@ends_session
def test_null_scale_and_one_row(dev, models):
    m, i = models("g16"), dict(GC.inputs("g16"))
    for tag, scale in (("null", None), ("one_row", i["scale"][:1].contiguous())):
        j = dict(i, scale=scale)
        j["target"] = GC.LC.target_ref(i["e"], scale)
        j["x_t"] = GC.LC.x_t_ref(i["x0"], i["e"], scale, i["t"], i["betas"])
        loss, grads = m.diffusion_loss_grad(i["x0"].to(dev), i["t"], i["betas"],
                                            noise_scale=None if scale is None else scale.to(dev), noise=i["e"].to(dev))
        _check(f"diff_grad/scale_{tag}", loss, grads, GC.references(j))


@ends_session
def test_counter_based_draws(dev, models):
    """noise_dev NULL: the draws normal_noise(seed, -1, global element).  Read back exactly under the one-step schedule
    betas = [0.25] (sb = 0.5: x_t = e / 2 from x0 = 0), they stand within counter_draws' bar of its host model; the
    gradients of the NULL call are bitwise those of a call given these draws, which the oracle is given too."""
    m, i = models("g16"), dict(GC.inputs("g16"))
    n, seed = i["x0"].shape[0], C.SEED_C + 5
    _, x_t, _ = m.diffusion_loss(torch.zeros_like(i["x0"]).to(dev), [0] * n, torch.tensor([0.25]), noise=None, seed=seed,
                                 return_parts=True)
    e = (2.0 * x_t).cpu()
    zr, r = C.normal_ref(seed, -1, np.arange(e.numel(), dtype=np.int64))
    z = e.double().numpy().reshape(-1)
    bar = C.draw_bar(r, 2.0 ** -23 * np.abs(z))
    assert record_delta(float((np.abs(z - zr) / bar).max()), 1.0, "diff_grad/counter/draws")
    i["e"] = e
    i["target"] = GC.LC.target_ref(e, i["scale"])
    i["x_t"] = GC.LC.x_t_ref(i["x0"], e, i["scale"], i["t"], i["betas"])
    loss, grads = _grad(m, i, dev, noise=None, seed=seed)
    loss_e, grads_e = _grad(m, i, dev)
    assert torch.equal(grads.flat, grads_e.flat) and torch.equal(loss, loss_e)
    _check("diff_grad/counter", loss, grads, GC.references(i))


# ---------------------------------------------------------------------------------------
# 7. caller memory

def _raw(m, x0, t, scale, rows, e, seed, weight, loss, flat, n, stream=None):
    return _lib.lib().dpk_diff_loss_grad(m._h, x0, t, scale, rows, e, ctypes.c_uint64(seed), ctypes.c_float(weight), loss,
                                         flat, n, stream)


@ends_session
def test_caller_memory(dev, models):
    m, i = models("g16"), GC.inputs("g16")
    n, rows = i["x0"].shape[0], i["scale"].shape[0]
    layout, total = m.param_layout()
    assert total == layout[-1][1] + layout[-1][2] and all(o % 4 == 0 for _, o, _ in layout)
    assert sum((k + 3) // 4 * 4 for _, _, k in layout[:-1]) + layout[-1][2] == total
    m.set_mask(None)
    loss0, grads0 = _grad(m, i, dev)
    w = 1.0 / n

    def arrays(role_out="out", null_loss=False):
        ins = [CM.Guarded(k, v.shape, device=dev, role="in" if role_out == "out" else "untouched",
                          data=v if role_out == "out" else None, misaligned=True)
               for k, v in (("x0", i["x0"]), ("t", i["t"]), ("scale", i["scale"]), ("noise", i["e"]))]
        outs = [CM.Guarded("loss", (n,), device=dev, role=role_out, misaligned=True, null=null_loss),
                CM.Guarded("grads", (total,), device=dev, role=role_out, misaligned=True)]
        assert all(a.alignment() == 4 for a in ins + outs if not a.null)
        return ins, outs

    for tag, null_loss in (("full", False), ("null_loss", True)):
        ins, outs = arrays(null_loss=null_loss)
        rc = _raw(m, ins[0].ptr, ins[1].ptr, ins[2].ptr, rows, ins[3].ptr, 0, w, outs[0].ptr, outs[1].ptr, n)
        _lib.check(m._h, "dpk_diff_loss_grad", rc)
        CM.check(ins + outs, {"loss": loss0, "grads": grads0.flat}, tag=f"diff_grad/memory/{tag}")
    ins, outs = arrays(role_out="untouched")
    rc = _raw(m, ins[0].ptr, ins[1].ptr, ins[2].ptr, rows, ins[3].ptr, 0, w, outs[0].ptr, outs[1].ptr, 0)
    assert rc == 0
    CM.check(ins + outs, tag="diff_grad/memory/n0")


# ---------------------------------------------------------------------------------------
# 8. train_step

@ends_session
def test_train_step(dev):
    from diffpose_amd.runner import Diffpose, default_args, default_config

    i = GC.inputs("g16")
    cfg = default_config()
    cfg.model = _config(GC.G16_SHAPE).model
    with pytest.raises(NotImplementedError, match="dropout"):
        Diffpose(default_args(), cfg, device=dev).train_step(i["x0"], torch.ones_like(i["x0"]), None, {})
    r = Diffpose(default_args(train_without_dropout=True), cfg, device=dev)
    r.create_diffusion_model(state_dict=i["sd"])
    m = r.model_diff
    try:
        with pytest.raises(NotImplementedError, match="train_step"):
            m.train(True)
        params = {k: torch.nn.Parameter(torch.from_numpy(v).to(dev)) for k, v in i["sd"].items()}
        before = {k: p.detach().clone() for k, p in params.items()}
        lr = 1e-3
        opt = torch.optim.SGD(list(params.values()), lr=lr)
        B = i["x0"].shape[0]
        scale = i["scale"].repeat(B // i["scale"].shape[0], 1, 1)
        # the step's own draws, and the GPU's own gradients at them
        g = torch.Generator().manual_seed(8)
        e = torch.randn((B, 17, 5), generator=g)
        t = training_timesteps(B, r.num_timesteps, generator=g)
        _, grads = m.diffusion_loss_grad(i["x0"].to(dev), t, r.betas, noise_scale=scale.to(dev), noise=e.to(dev),
                                         mask=r.src_mask)
        loss_diff = r.train_step(i["x0"], scale, opt, params, generator=torch.Generator().manual_seed(8))
        for k, p in params.items():
            assert torch.equal(p.grad, grads[k]), k
            assert torch.equal(p.detach(), before[k].add(grads[k], alpha=-lr)), k
        # the handle now computes with w - lr g: its loss on the fixed batch against the float64 model at those weights
        new_sd = {k: p.detach().cpu().numpy() for k, p in params.items()}
        lo = GC.LC.loss_oracle(new_sd, i["adj"], i["layers"], i["heads"], i["x_t"], i["target"], i["mask"], i["t"])
        loss = m.diffusion_loss(i["x0"].to(dev), i["t"], i["betas"], noise_scale=i["scale"].to(dev), noise=i["e"].to(dev))
        ratio = np.abs(loss.cpu().double().numpy() - lo["loss64"]) / lo["bar"]
        assert record_delta(float(ratio.max()), 1.0, "diff_grad/train_step/loss_after")
        old = GC.LC.loss_oracle(i["sd"], i["adj"], i["layers"], i["heads"], i["x_t"], i["target"], i["mask"], i["t"])
        assert float(np.abs(lo["loss64"] - old["loss64"]).max()) > 10 * float(lo["bar"].max())    # the step is visible
        j = dict(i, e=e, scale=scale, t=t.float(), target=GC.LC.target_ref(e, scale),
                 x_t=GC.LC.x_t_ref(i["x0"], e, scale, t.float(), i["betas"]))
        l64, _ = GC.autograd(j, torch.float64)
        assert abs(loss_diff - float(l64.mean())) <= 1e-5 * float(l64.mean()) + 1e-5
    finally:
        m.close()


# ---------------------------------------------------------------------------------------
# 9. refusals

@ends_session
def test_refusals(dev, models):
    from diffpose_amd.gcnpose import HipGCNpose
    from diffpose_amd.weights import synthetic_state_dict

    L = _lib.lib()
    m, i = models("h96"), GC.inputs("h96")
    n, rows = i["x0"].shape[0], i["scale"].shape[0]
    _, total = m.param_layout()
    x0, t, sc, e = (i[k].to(dev).contiguous() for k in ("x0", "t", "scale", "e"))
    loss, flat = torch.empty(n, device=dev), torch.empty(total, device=dev)
    call = lambda mm=m, stream=None: _raw(mm, x0.data_ptr(), t.data_ptr(), sc.data_ptr(), rows, e.data_ptr(), 0, 1.0 / n,  # noqa: E731
                                          loss.data_ptr(), flat.data_ptr(), n, stream)
    m.set_schedule([0], i["betas"], 0.0)
    m.set_mask(None)
    assert call() == 0
    torch.cuda.synchronize(dev)
    first = flat.clone()
    # a GCNpose handle
    pm = HipGCNpose(adj_mx_from_edges(), None, device=dev)
    pm.load_state_dict(synthetic_state_dict(kind="pose"))
    try:
        assert call(pm) == -2 and b"GCNpose" in L.dpk_last_error(pm._h)
        assert L.dpk_param_count(pm._h) == 0
    finally:
        pm.close()
    # a gemm mode other than fp32
    m.set_gemm_mode("f16x3")
    try:
        assert call() == -2 and b"fp32" in L.dpk_last_error(m._h)
    finally:
        m.set_gemm_mode("fp32")
    # under capture
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = call(stream=torch.cuda.current_stream(dev).cuda_stream)
        msg = L.dpk_last_error(m._h)
    assert rc == -4 and b"captured" in msg, (rc, msg)
    del g
    # the handle works afterwards
    flat.zero_()
    assert call() == 0
    torch.cuda.synchronize(dev)
    assert torch.equal(flat, first)
