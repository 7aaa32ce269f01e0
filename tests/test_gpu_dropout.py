"""GPU: the train-mode gradient of the denoising objective, dpk_diff_loss_grad_train / dpk_dropout_mask /
HipGCNdiff.diffusion_loss_grad(dropout=) / runner.Diffpose.train_step under args.train_dropout, against the masks,
references and bars of tests/dropout_cases.py (whose train-mode oracle tests/test_dropout_cpu.py pins to the reference's
own train-mode backward, fixture g17): the exported masks bitwise the numpy restatement, every parameter tensor of
every case within 8 x the oracle's own gap to the float64 train-mode gradient, the per-pose loss within
diff_loss_cases' bar."""
import ctypes
import functools
from types import SimpleNamespace as ns

import numpy as np
import pytest
import torch

import caller_memory as CM
import diff_grad_cases as GC
import dropout_cases as DC
from conftest import record_delta
from diffpose_amd import _lib
from diffpose_amd._lib import DpkError
from diffpose_amd.gcndiff import HipGCNdiff, adj_mx_from_edges
from diffpose_amd.schedule import training_timesteps

pytestmark = pytest.mark.gpu

TRAIN_FORMS = {"attention<train>", "drop_add", "relu_drop"}
FORMS_OF = {"sublayer": {"drop_add"}, "attn": {"attention<train>"}, "gconv": {"relu_drop"}}


def ends_session(fn):
    """A library / HIP error is no parity miss: run nothing more on the device."""
    @functools.wraps(fn)
    def run(*a, **k):
        try:
            return fn(*a, **k)
        except DpkError as e:
            pytest.exit(f"dropout/{fn.__name__}: {e}", returncode=3)
        except RuntimeError as e:
            if "HIP error" in str(e) or "hipError" in str(e):
                pytest.exit(f"dropout/{fn.__name__}: {e}", returncode=3)
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
def g17(golden):
    """(inputs, masks, references) of the g17 fixture, computed once; do not modify"""
    i, masks, rates, seed = DC.g17_inputs(golden)
    assert rates == DC.REF_RATES and seed == DC.SEED
    return i, masks, DC.references(i, masks)


def _grad(m, i, dev, rates=DC.REF_RATES, seed=DC.SEED, **kw):
    args = dict(noise_scale=i["scale"].to(dev), noise=i["e"].to(dev), mask=i["mask"].to(dev), dropout=rates,
                dropout_seed=seed)
    args.update(kw)
    return m.diffusion_loss_grad(i["x0"].to(dev), i["t"], i["betas"], **args)


def _check(tag, loss, grads, ref, scale=1.0):
    """every tensor within its bar of the float64 train-mode gradient, the loss within its bar per pose; every delta
    recorded before the assertion"""
    ok = True
    assert list(grads) == list(ref["g64"])
    for k, g64 in ref["g64"].items():
        got = grads[k].detach().cpu().double() / scale
        assert got.shape == g64.shape, k
        ok = record_delta(float((got - g64).abs().max()), ref["bar"][k], f"{tag}/{k}") and ok
    if loss is not None:
        ratio = np.abs(loss.cpu().double().numpy() - ref["loss64"]) / ref["loss_bar"]
        ok = record_delta(float(ratio.max()), 1.0, f"{tag}/loss") and ok
    assert ok, tag


# ---------------------------------------------------------------------------------------
# 1. the exported mask

@ends_session
def test_mask_export_is_the_restatement(dev, models):
    m = models("g16")
    pad, fill = 64, 0xA5
    for layer, site, p in ((0, 0, 0.1), (1, 2, 0.25), (1, 4, 0.1)):
        for n in (1, 3, 4, 5, 1023, 5 * 17 * 32):
            for first in (0, 1, 255 * 3):
                buf = torch.full((pad + n + pad,), fill, dtype=torch.uint8, device=dev)
                rc = _lib.lib().dpk_dropout_mask(ctypes.c_uint64(DC.SEED), layer, site, ctypes.c_float(p), first, n,
                                                 buf.data_ptr() + pad, None)
                assert rc == 0
                got = buf.cpu().numpy()
                assert (got[:pad] == fill).all() and (got[pad + n:] == fill).all(), (n, first)
                want = DC.keep_mask(DC.SEED, layer, site, p, first, n).astype(np.uint8)
                assert np.array_equal(got[pad:pad + n], want), (layer, site, p, n, first)
    # the wrapper, a site by name, rate 0, and an index past 2^34
    assert np.array_equal(m.dropout_mask(1, "sub1", 0.25, DC.SEED, 1023, first=1).cpu().numpy(),
                          DC.keep_mask(DC.SEED, 1, 2, 0.25, 1, 1023).astype(np.uint8))
    assert bool(m.dropout_mask(0, 3, 0.0, DC.SEED, 4099).all())
    big = (1 << 36) + 3
    assert np.array_equal(m.dropout_mask(0, 0, 0.1, DC.SEED, 9, first=big).cpu().numpy(),
                          DC.keep_mask(DC.SEED, 0, 0, 0.1, big, 9).astype(np.uint8))
    # n = 0 touches nothing
    buf = torch.full((pad,), fill, dtype=torch.uint8, device=dev)
    assert _lib.lib().dpk_dropout_mask(ctypes.c_uint64(DC.SEED), 0, 1, ctypes.c_float(0.25), 0, 0, buf.data_ptr() + 8,
                                       None) == 0
    assert bool((buf == fill).all())
    assert m.dropout_mask(0, 1, 0.25, DC.SEED, 0).numel() == 0


# ---------------------------------------------------------------------------------------
# 2. g17: the fixture

@ends_session
def test_g17_fixture(dev, golden, g17, models):
    z, (i, masks, ref) = DC.golden_g17(golden), g17
    m = models("g16")
    assert m.fused == 0
    m.debug_grad_forms()
    loss, grads = _grad(m, i, dev, rates=True)              # True: (config.model.dropout, 0.1, 0.1)
    fwd, bwd = m.debug_grad_forms()
    _check("dropout/g17", loss, grads, ref)
    assert fwd == GC.GEMM_FORMS["g16"] and bwd == GC.BWD_FORMS | TRAIN_FORMS, (fwd, bwd)
    # the reference's own train-mode p.grad stands within the same bars of the float64 gradient
    for k, g in grads.items():
        assert float((z["grad." + k].double() - ref["g64"][k]).abs().max()) <= ref["bar"][k], k
        assert tuple(g.shape) == tuple(z["grad." + k].shape)
    # and the eval-mode gradient does not: the masks are in the numbers
    _, plain = m.diffusion_loss_grad(i["x0"].to(dev), i["t"], i["betas"], noise_scale=i["scale"].to(dev),
                                     noise=i["e"].to(dev))
    miss = [k for k in ref["g64"] if float((plain[k].cpu().double() - ref["g64"][k]).abs().max()) > ref["bar"][k]]
    assert len(miss) > len(ref["g64"]) // 2, miss


# ---------------------------------------------------------------------------------------
# 3. one site at a time

@pytest.mark.parametrize("which", list(DC.ISOLATION))
@ends_session
def test_site_isolation(dev, models, which):
    rates = DC.ISOLATION[which]
    m, i = models("odd"), GC.inputs("odd")
    m.debug_grad_forms()
    loss, grads = _grad(m, i, dev, rates=rates)
    fwd, bwd = m.debug_grad_forms()
    _check(f"dropout/odd/{which}", loss, grads, DC.case_references("odd", rates))
    assert bwd == GC.BWD_FORMS | FORMS_OF[which] and fwd == GC.GEMM_FORMS["odd"], (fwd, bwd)


# ---------------------------------------------------------------------------------------
# 4. the reference's rates across shapes

@pytest.mark.parametrize("name", list(DC.SHAPE_CASES))
@ends_session
def test_reference_rates_across_shapes(dev, models, name):
    m, i, ref = models(name), GC.inputs(name), DC.case_references(name)
    fused = m.fused
    assert fused == (1 if name in ("h96", "pad15") else 0)
    m.debug_grad_forms()
    loss, grads = _grad(m, i, dev)
    _, bwd = m.debug_grad_forms()
    _check(f"dropout/{name}", loss, grads, ref)
    assert bwd == (GC.BWD_FORMS_W320 if name == "w320" else GC.BWD_FORMS) | TRAIN_FORMS, bwd
    assert m.fused == fused


# ---------------------------------------------------------------------------------------
# 5. key masks

@ends_session
def test_key_masks(dev, models):
    m, i = models("perop"), GC.inputs("perop")
    n, npts = i["x0"].shape[0], GC.CASES["perop"][0][3]
    one_off = torch.ones(1, 1, npts, dtype=torch.bool)
    one_off[0, 0, 5] = False
    per = torch.from_numpy(CM.pose_masks(n, npts))
    masks = DC.case_masks("perop")
    try:
        for tag, mk in (("handle", one_off), ("per_pose", per)):
            loss, grads = _grad(m, i, dev, mask=mk.to(dev))
            _check(f"dropout/mask/{tag}", loss, grads, DC.references(i, masks, mask=mk))
    finally:
        m.set_mask(None)


# ---------------------------------------------------------------------------------------
# 6. bitwise properties

@ends_session
def test_bitwise_properties(dev, models):
    m, i = models("g16"), GC.inputs("g16")
    loss0, plain = m.diffusion_loss_grad(i["x0"].to(dev), i["t"], i["betas"], noise_scale=i["scale"].to(dev),
                                         noise=i["e"].to(dev), mask=i["mask"].to(dev))
    m.debug_grad_forms()
    loss_z, zero = _grad(m, i, dev, rates=(0.0, 0.0, 0.0))
    assert torch.equal(zero.flat, plain.flat) and torch.equal(loss_z, loss0)
    assert m.debug_grad_forms()[1] == GC.BWD_FORMS             # no train form at rate 0
    loss1, g1 = _grad(m, i, dev)
    loss2, g2 = _grad(m, i, dev)
    assert torch.equal(g1.flat, g2.flat) and torch.equal(loss1, loss2)
    assert not torch.equal(g1.flat, plain.flat)
    loss3, g3 = _grad(m, i, dev, seed=DC.SEED + 1)
    assert not torch.equal(g3.flat, g1.flat) and not torch.equal(loss3, loss1)
    # pose0 keys the masks, and only them: at rate 0 it changes nothing
    _, zero3 = _grad(m, i, dev, rates=(0.0, 0.0, 0.0), pose0=3)
    assert torch.equal(zero3.flat, plain.flat)
    _, g4 = _grad(m, i, dev, pose0=3)
    assert not torch.equal(g4.flat, g1.flat)


# ---------------------------------------------------------------------------------------
# 7. sharding

@ends_session
def test_shards_add_up(dev, g17, models):
    i, masks, ref = g17
    m = models("g16")
    n = i["x0"].shape[0]
    total, losses = None, []
    for lo, hi in DC.G17_SHARDS:
        loss, grads = m.diffusion_loss_grad(i["x0"][lo:hi].to(dev), i["t"][lo:hi], i["betas"],
                                            noise_scale=i["scale"][lo:hi].to(dev), noise=i["e"][lo:hi].to(dev),
                                            weight=1.0 / n, dropout=DC.REF_RATES, dropout_seed=DC.SEED, pose0=lo)
        losses.append(loss)
        total = grads.flat.clone() if total is None else total + grads.flat
    layout, _ = m.param_layout()
    shapes = {k: v.shape for k, v in ref["g64"].items()}
    summed = {name: total[off:off + num].view(shapes[name]) for name, off, num in layout}
    _check("dropout/g17/shards", torch.cat(losses), summed, ref)


# ---------------------------------------------------------------------------------------
# 8. caller memory and refusals

def _raw(m, x0, t, scale, rows, e, seed, weight, drop, drop_seed, pose0, loss, flat, n, stream=None):
    return _lib.lib().dpk_diff_loss_grad_train(m._h, x0, t, scale, rows, e, ctypes.c_uint64(seed), ctypes.c_float(weight),
                                               drop, ctypes.c_uint64(drop_seed), pose0, loss, flat, n, stream)


@ends_session
def test_caller_memory(dev, models):
    m, i = models("g16"), GC.inputs("g16")
    n, rows = i["x0"].shape[0], i["scale"].shape[0]
    _, total = m.param_layout()
    m.set_mask(None)
    loss0, grads0 = _grad(m, i, dev, pose0=2)
    w = 1.0 / n
    drop = ctypes.byref(_lib.DpkDropout(*DC.REF_RATES))

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
        rc = _raw(m, ins[0].ptr, ins[1].ptr, ins[2].ptr, rows, ins[3].ptr, 0, w, drop, DC.SEED, 2, outs[0].ptr,
                  outs[1].ptr, n)
        _lib.check(m._h, "dpk_diff_loss_grad_train", rc)
        CM.check(ins + outs, {"loss": loss0, "grads": grads0.flat}, tag=f"dropout/memory/{tag}")
    ins, outs = arrays(role_out="untouched")
    rc = _raw(m, ins[0].ptr, ins[1].ptr, ins[2].ptr, rows, ins[3].ptr, 0, w, drop, DC.SEED, 2, outs[0].ptr, outs[1].ptr, 0)
    assert rc == 0
    CM.check(ins + outs, tag="dropout/memory/n0")


@ends_session
def test_refusals(dev, models):
    L = _lib.lib()
    m, i = models("g16"), GC.inputs("g16")
    n, rows = i["x0"].shape[0], i["scale"].shape[0]
    _, total = m.param_layout()
    x0, t, sc, e = (i[k].to(dev).contiguous() for k in ("x0", "t", "scale", "e"))
    loss, flat = torch.empty(n, device=dev), torch.empty(total, device=dev)
    ok = _lib.DpkDropout(*DC.REF_RATES)

    def call(drop=ok, pose0=0, stream=None):
        return _raw(m, x0.data_ptr(), t.data_ptr(), sc.data_ptr(), rows, e.data_ptr(), 0, 1.0 / n,
                    None if drop is None else ctypes.byref(drop), DC.SEED, pose0, loss.data_ptr(), flat.data_ptr(), n, stream)

    m.set_schedule([0], i["betas"], 0.0)
    m.set_mask(None)
    assert call() == 0
    torch.cuda.synchronize(dev)
    first = flat.clone()
    flat.fill_(7.0)
    assert call(drop=None) == -1 and b"NULL" in L.dpk_last_error(m._h)
    for bad, text in ((-0.1, b"-0.1"), (1.0, b"1.0"), (float("nan"), b"nan")):
        for field in ("sublayer", "attn", "gconv"):
            d = _lib.DpkDropout(*DC.REF_RATES)
            setattr(d, field, bad)
            msg = L.dpk_last_error(m._h) if call(drop=d) == -1 else b""
            assert field.encode() in msg and text in msg.lower(), (field, bad, msg)
    assert call(pose0=-1) == -1 and b"-1" in L.dpk_last_error(m._h)
    torch.cuda.synchronize(dev)
    assert bool((flat == 7.0).all())                     # a refused call writes nothing
    assert call() == 0
    torch.cuda.synchronize(dev)
    assert torch.equal(flat, first)


@ends_session
def test_refusals_mode_and_capture(dev, models):
    """gemm mode 1 and a capturing stream, on a handle that has the mode (as tests/test_gpu_diff_grad.py's refusals)"""
    L = _lib.lib()
    m, i = models("h96"), GC.inputs("h96")
    n, rows = i["x0"].shape[0], i["scale"].shape[0]
    _, total = m.param_layout()
    x0, t, sc, e = (i[k].to(dev).contiguous() for k in ("x0", "t", "scale", "e"))
    loss, flat = torch.empty(n, device=dev), torch.empty(total, device=dev)
    ok = _lib.DpkDropout(*DC.REF_RATES)
    call = lambda stream=None: _raw(m, x0.data_ptr(), t.data_ptr(), sc.data_ptr(), rows, e.data_ptr(), 0, 1.0 / n,  # noqa: E731
                                    ctypes.byref(ok), DC.SEED, 0, loss.data_ptr(), flat.data_ptr(), n, stream)
    m.set_schedule([0], i["betas"], 0.0)
    m.set_mask(None)
    assert call() == 0
    torch.cuda.synchronize(dev)
    first = flat.clone()
    m.set_gemm_mode("f16x3")
    try:
        assert call() == -2 and b"fp32" in L.dpk_last_error(m._h)
    finally:
        m.set_gemm_mode("fp32")
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = call(stream=torch.cuda.current_stream(dev).cuda_stream)
        msg = L.dpk_last_error(m._h)
    assert rc == -4 and b"captured" in msg, (rc, msg)
    del g
    flat.zero_()
    assert call() == 0
    torch.cuda.synchronize(dev)
    assert torch.equal(flat, first)


# ---------------------------------------------------------------------------------------
# 9. train_step

@ends_session
def test_train_step_with_dropout(dev):
    from diffpose_amd.runner import Diffpose, default_args, default_config

    i = GC.inputs("g16")
    cfg = default_config()
    cfg.model = _config(GC.G16_SHAPE).model
    with pytest.raises(NotImplementedError, match="dropout") as ei:
        Diffpose(default_args(), cfg, device=dev).train_step(i["x0"], torch.ones_like(i["x0"]), None, {})
    assert "train_dropout" in str(ei.value)
    r = Diffpose(default_args(train_dropout=True), cfg, device=dev)
    r.create_diffusion_model(state_dict=i["sd"])
    m = r.model_diff
    try:
        with pytest.raises(NotImplementedError, match="dropout="):
            m.train(True)
        params = {k: torch.nn.Parameter(torch.from_numpy(v).to(dev)) for k, v in i["sd"].items()}
        before = {k: p.detach().clone() for k, p in params.items()}
        lr = 1e-3
        opt = torch.optim.SGD(list(params.values()), lr=lr)
        B = i["x0"].shape[0]
        scale = i["scale"].repeat(B // i["scale"].shape[0], 1, 1)
        # the step's own draws, then its seed; and the GPU's own train-mode gradients at them
        g = torch.Generator().manual_seed(8)
        e = torch.randn((B, 17, 5), generator=g)
        t = training_timesteps(B, r.num_timesteps, generator=g)
        seed = int(torch.randint(0, 2 ** 63 - 1, (1,), generator=g))
        loss, grads = m.diffusion_loss_grad(i["x0"].to(dev), t, r.betas, noise_scale=scale.to(dev), noise=e.to(dev),
                                            mask=r.src_mask, dropout=True, dropout_seed=seed)
        _, plain = m.diffusion_loss_grad(i["x0"].to(dev), t, r.betas, noise_scale=scale.to(dev), noise=e.to(dev),
                                         mask=r.src_mask)
        assert not torch.equal(plain.flat, grads.flat)
        # a clip that binds (half the gradient's norm): the step is -lr x the clipped train-mode gradient.  The
        # expected .grad are views of one flat tensor at the layout's offsets, as train_step's are
        flat2 = grads.flat.clone()
        layout, _ = m.param_layout()
        want = {k: torch.nn.Parameter(before[k].clone()) for k in params}
        for name, off, num in layout:
            want[name].grad = flat2[off:off + num].view(want[name].shape)
        cfg.optim = ns(grad_clip=0.5 * float(torch.linalg.vector_norm(grads.flat)))
        norm = torch.nn.utils.clip_grad_norm_(list(want.values()), cfg.optim.grad_clip)
        assert float(norm) > cfg.optim.grad_clip
        loss_diff = r.train_step(i["x0"], scale, opt, params, generator=torch.Generator().manual_seed(8))
        for k, p in params.items():
            assert torch.equal(p.grad, want[k].grad), k
            assert torch.equal(p.detach(), before[k].add(want[k].grad, alpha=-lr)), k
        assert loss_diff == float(loss.mean())
        # the same e and t as a step without the flag: the float64 train-mode loss at those draws and that seed
        j = dict(i, e=e, scale=scale, t=t.float(), target=GC.LC.target_ref(e, scale),
                 x_t=GC.LC.x_t_ref(i["x0"], e, scale, t.float(), i["betas"]))
        l64, _, _ = DC.autograd(j, DC.masks_for(GC.G16_SHAPE, B, DC.REF_RATES, seed), torch.float64)
        assert abs(loss_diff - float(l64.mean())) <= 1e-5 * float(l64.mean()) + 1e-5
    finally:
        m.close()
