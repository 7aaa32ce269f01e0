"""GPU: the optimiser step on the device, dpk_train_* / HipGCNdiff.device_optimizer / runner.Diffpose.train_step with a
DeviceAdam, against the float64 model and the measured bars of tests/optim_cases.py (which tests/test_device_optim_cpu.py
pins to torch.optim.Adam): parameters and moments within 8 x torch's own float32 gap, the norm within one ulp, the EMA
shadow and the refreshed weights bit for bit."""
import ctypes
import functools
from types import SimpleNamespace as ns

import numpy as np
import pytest
import torch

import caller_memory as CM
import diff_grad_cases as GC
import optim_cases as OC
from conftest import record_delta
from diffpose_amd import _lib
from diffpose_amd._lib import DpkError
from diffpose_amd.gcndiff import HipGCNdiff, adj_mx_from_edges
from diffpose_amd.schedule import training_timesteps

pytestmark = pytest.mark.gpu
E_INVALID, E_UNSUPPORTED, E_STATE = -1, -2, -4


def ends_session(fn):
    """A library / HIP error is no parity miss: run nothing more on the device."""
    @functools.wraps(fn)
    def run(*a, **k):
        try:
            return fn(*a, **k)
        except DpkError as e:
            pytest.exit(f"device_optim/{fn.__name__}: {e}", returncode=3)
        except RuntimeError as e:
            if "HIP error" in str(e) or "hipError" in str(e):
                pytest.exit(f"device_optim/{fn.__name__}: {e}", returncode=3)
            raise
    return run


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _config(shape, dropout=0.25):
    hid, heads, layers, npts = shape[:4]
    return ns(model=ns(hid_dim=hid, emd_dim=hid, coords_dim=[5, 5], num_layer=layers, n_head=heads, dropout=dropout,
                       n_pts=npts))


def _model(name, dev, sd=None):
    shape = GC.CASES[name][0]
    m = HipGCNdiff(adj_mx_from_edges(shape[3], shape[4]), _config(shape), device=dev)
    m.load_state_dict(GC.inputs(name)["sd"] if sd is None else sd)
    return m


def _text(m):
    return _lib.lib().dpk_last_error(m._h).decode()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _raw_eps(m, i, dev):
    x, t = i["x0"].to(dev).contiguous(), i["t"].to(dev).contiguous()
    eps = torch.empty_like(x)
    rc = _lib.lib().dpk_eps(m._h, x.data_ptr(), t.data_ptr(), eps.data_ptr(), x.shape[0], _stream(dev))
    return rc, eps


def _raw_load(m, sd):
    names = list(sd)
    arrs = [np.ascontiguousarray(sd[k], dtype=np.float32) for k in names]
    fp = ctypes.POINTER(ctypes.c_float)
    return _lib.lib().dpk_load_weights(m._h, (ctypes.c_char_p * len(names))(*[k.encode() for k in names]),
                                       (fp * len(arrs))(*[a.ctypes.data_as(fp) for a in arrs]),
                                       (ctypes.c_int64 * len(arrs))(*[a.size for a in arrs]), len(arrs))


def _grad(m, i, dev):
    return m.diffusion_loss_grad(i["x0"].to(dev), i["t"], i["betas"], noise_scale=i["scale"].to(dev), noise=i["e"].to(dev),
                                 mask=i["mask"].to(dev))


def _arrays(opt, names=("params", "exp_avg", "exp_avg_sq")):
    return {k: opt._get(k)[0].cpu() for k in names}


# ---------------------------------------------------------------------------------------
# 1. a zero gradient changes nothing

@pytest.mark.parametrize("name", ["g16", "h96"])
@ends_session
def test_zero_gradient(dev, name):
    m, i = _model(name, dev), GC.inputs(name)
    try:
        assert m.fused == (1 if name == "h96" else 0)
        eps0 = m(i["x0"].to(dev), i["mask"].to(dev), i["t"].to(dev))
        opt = m.device_optimizer(lr=OC.LR, grad_clip=1.0, ema_rate=OC.MU)
        want = torch.from_numpy(OC.inputs(name)["params"])
        p0 = opt._get("params")[0]
        assert torch.equal(p0.cpu(), want)                      # the seed: the loaded weights in their torch layouts
        gn = opt.step(torch.zeros(opt.total, dtype=torch.float32, device=dev))
        p1, step = opt._get("params")
        assert step == 1 and float(gn) == 0.0 and torch.equal(p1, p0)
        assert torch.equal(opt._get("ema")[0].cpu(), OC.ema_by_torch(p0.cpu(), p0.cpu()))    # (1 - mu) p + mu p, rounded
        eps1 = m(i["x0"].to(dev), i["mask"].to(dev), i["t"].to(dev))       # (after the model's own sync on h96)
        assert torch.equal(eps1, eps0)
        assert list(m.state_dict()) == [k for k, _, _ in opt.layout]
        with pytest.raises(RuntimeError, match="DeviceAdam"):
            m.load_state_dict(i["sd"])
        opt.close()
        assert torch.equal(m(i["x0"].to(dev), i["mask"].to(dev), i["t"].to(dev)), eps0)
    finally:
        m.close()


# ---------------------------------------------------------------------------------------
# 2. one step and five steps from synthetic gradients

@pytest.mark.parametrize("clip", sorted(OC.CLIPS))
@pytest.mark.parametrize("name", ["g16", "odd", "h96"])
@ends_session
def test_steps_inside_the_bars(dev, name, clip):
    amsgrad = name == "g16"
    c = OC.CLIPS[clip]
    i, ref = OC.inputs(name), OC.bars(name, amsgrad=amsgrad, clip=c)
    m = _model(name, dev)
    try:
        opt = m.device_optimizer(lr=OC.LR, betas=OC.BETAS, eps=OC.EPS, amsgrad=amsgrad, grad_clip=c if c > 0 else None,
                                 ema_rate=OC.MU)
        names = OC.ARRAYS[:4 if amsgrad else 3]
        shadow = opt._get("ema")[0].cpu()
        ok = True
        for step in range(1, OC.STEPS + 1):
            g = torch.from_numpy(i["grads"][step - 1]).to(dev)
            keep = g.clone()
            gn = float(opt.step(g))
            assert torch.equal(g, keep)                          # grads_dev is an input
            g64 = ref["m64"][step - 1]["gnorm"]
            ok = record_delta(abs(gn - g64), OC.ulp32(g64), f"device_optim/{name}/{clip}/gnorm{step}") and ok
            p = opt._get("params")[0].cpu()
            new_shadow = opt._get("ema")[0].cpu()
            assert torch.equal(new_shadow, OC.ema_by_torch(p, shadow)), f"EMA shadow, step {step}"
            shadow = new_shadow
            if step in (1, OC.STEPS):
                for arr in names:
                    got, count = opt._get(arr)
                    assert count == step
                    got = got.cpu().numpy()
                    pad = np.ones(i["F"], dtype=bool)
                    for _k, off, n in i["layout"]:
                        pad[off:off + n] = False
                    assert not got[pad].any()                    # the padding stays zero
                    miss = OC.within(got, name, step, arr, ref)
                    worst = max((d / b for _k, d, b in miss), default=0.0)
                    ok = record_delta(worst, 1.0, f"device_optim/{name}/{clip}/{arr}{step}") and ok
                    assert not miss, (arr, step, miss[:3])
        assert ok
    finally:
        m.close()


# ---------------------------------------------------------------------------------------
# 3. the refresh is exact; 6. the sequence repeats bit for bit

def _three_applies(m, i, dev):
    """three steps on the case's own gradients; (optimiser, the three norms)"""
    opt = m.device_optimizer(lr=OC.LR, grad_clip=1.0, ema_rate=OC.MU)
    norms = []
    for _ in range(3):
        _loss, grads = _grad(m, i, dev)
        norms.append(opt.step(grads))
    return opt, torch.stack(norms).cpu()


@pytest.mark.parametrize("name", ["g16", "odd", "perop", "pad15", "h96"])
@ends_session
def test_refresh_is_exact(dev, name):
    i = GC.inputs(name)
    m = _model(name, dev)
    fresh = None
    try:
        opt, norms = _three_applies(m, i, dev)
        assert bool((norms > 0).all())
        trained = {k: v.cpu().numpy() for k, v in m.state_dict().items()}
        assert any(not np.array_equal(trained[k], np.asarray(i["sd"][k], dtype=np.float32).reshape(trained[k].shape)) for k in trained)
        fresh = _model(name, dev, sd=trained)
        # the gradient call first, with no sync: it runs the per-op model, which the refresh rewrote
        la, ga = _grad(m, i, dev)
        lb, gb = _grad(fresh, i, dev)
        assert torch.equal(la, lb), "loss of the gradient call"
        for k in ga:
            assert torch.equal(ga[k], gb[k]), k
        if m.fused:
            rc, _ = _raw_eps(m, i, dev)
            assert rc == E_STATE and "dpk_train_sync" in _text(m)
            opt.sync()
        x, mask, t = i["x0"].to(dev), i["mask"].to(dev), i["t"].to(dev)
        assert torch.equal(m(x, mask, t), fresh(x, mask, t)), "dpk_eps"
        args = dict(noise_scale=i["scale"].to(dev), noise=i["e"].to(dev), mask=mask)
        assert torch.equal(m.diffusion_loss(x, i["t"], i["betas"], **args), fresh.diffusion_loss(x, i["t"], i["betas"], **args))
        if name in ("g16", "h96"):
            seq = [10, 40]
            assert torch.equal(m.sample(x, seq, i["betas"], eta=0.0, mask=mask), fresh.sample(x, seq, i["betas"], eta=0.0, mask=mask))
    finally:
        m.close()
        if fresh is not None:
            fresh.close()


@pytest.mark.parametrize("name", ["g16", "h96"])
@ends_session
def test_the_sequence_repeats_bitwise(dev, name):
    i = GC.inputs(name)
    runs = []
    for _ in range(2):
        m = _model(name, dev)
        try:
            opt, norms = _three_applies(m, i, dev)
            runs.append((_arrays(opt), norms))
        finally:
            m.close()
    for k in runs[0][0]:
        assert torch.equal(runs[0][0][k], runs[1][0][k]), k
    assert torch.equal(runs[0][1], runs[1][1])


# ---------------------------------------------------------------------------------------
# 4. the stale rule

@ends_session
def test_stale_rule(dev):
    L = _lib.lib()
    for name in ("h96", "g16"):
        i = GC.inputs(name)
        m = _model(name, dev)
        fresh = None
        try:
            opt = m.device_optimizer(lr=OC.LR)
            rc, _ = _raw_eps(m, i, dev)
            assert rc == 0                                        # begun, no step yet: nothing is stale
            opt.step(_grad(m, i, dev)[1])
            rc, eps = _raw_eps(m, i, dev)
            if name == "h96":
                assert rc == E_STATE and "dpk_train_sync" in _text(m)
                _loss, _g = _grad(m, i, dev)                      # the gradient call is not refused
                assert L.dpk_train_sync(m._h) == 0
                rc, eps = _raw_eps(m, i, dev)
            assert rc == 0
            assert _raw_load(m, i["sd"]) == E_STATE and "training" in _text(m)
            assert L.dpk_set_graph(m._h, m.adj.ctypes.data_as(ctypes.POINTER(ctypes.c_float))) == E_STATE and "training" in _text(m)
            assert L.dpk_train_begin(m._h, ctypes.byref(_lib.DpkOptimConfig(0.9, 0.999, 1e-8, 0, 0.0, -1.0))) == E_STATE
            trained = {k: v.cpu().numpy() for k, v in m.state_dict().items()}
            opt.close()
            # an ordinary handle again, sampling from the trained weights
            fresh = _model(name, dev, sd=trained)
            x, mask = i["x0"].to(dev), i["mask"].to(dev)
            assert torch.equal(m.sample(x, [10, 40], i["betas"], mask=mask), fresh.sample(x, [10, 40], i["betas"], mask=mask))
            assert torch.equal(_raw_eps(m, i, dev)[1], eps)
            assert L.dpk_set_graph(m._h, m.adj.ctypes.data_as(ctypes.POINTER(ctypes.c_float))) == 0
            assert _raw_load(m, i["sd"]) == 0
            assert L.dpk_train_sync(m._h) == E_STATE
        finally:
            m.close()
            if fresh is not None:
                fresh.close()


# ---------------------------------------------------------------------------------------
# 5. against the torch path

@pytest.mark.parametrize("dropout", [False, True], ids=["eval", "train_dropout"])
@ends_session
def test_against_the_torch_path(dev, dropout):
    """five train_steps with a DeviceAdam against five with torch.optim.Adam on the existing path, the same draws.
    After step 1 both paths have seen the same gradient bit for bit, and the device's parameters are held to the torch
    path's own 1-step gap to the float64 model.  From step 2 on the two paths' gradients differ in their last bits
    (their weights do), and Adam turns a gradient that is rounding residue alone into a full +-lr step: the key biases
    (self_attn.linears.1.bias, whose gradient is exactly zero) moved 5e-5 apart in five steps on an MI355X, torch
    against torch would too.  So after five steps each path is held to the float64 model of its OWN gradient sequence:
    gap = |torch path - model64(its gradients)| per tensor, the device inside max(8 x gap, one ulp) of
    model64(the device path's gradients)."""
    from diffpose_amd.runner import Diffpose, default_args, default_config

    i = GC.inputs("g16")
    cfg = default_config()
    cfg.model = _config(GC.G16_SHAPE).model
    cfg.optim = ns(optimizer="Adam", lr=OC.LR, eps=OC.EPS, amsgrad=False, grad_clip=1.0, weight_decay=0.0)
    args = default_args(train_dropout=True) if dropout else default_args(train_without_dropout=True)
    B = i["x0"].shape[0]
    scale = i["scale"].repeat(B // i["scale"].shape[0], 1, 1)
    o = OC.inputs("g16")
    layout, F = o["layout"], o["F"]
    ra, rb = Diffpose(args, cfg, device=dev), Diffpose(args, cfg, device=dev)
    ra.create_diffusion_model(state_dict=i["sd"]), rb.create_diffusion_model(state_dict=i["sd"])
    try:
        params = {k: torch.nn.Parameter(torch.from_numpy(np.array(v)).to(dev)) for k, v in i["sd"].items()}
        topt = torch.optim.Adam(list(params.values()), lr=OC.LR, betas=OC.BETAS, eps=OC.EPS)
        dopt = rb.model_diff.device_optimizer(cfg)
        assert dopt.grad_clip == 1.0 and dopt.ema_rate is None
        grads, dgrads, la, lb, bars, first = [], [], [], [], [], None
        for s in range(5):
            # the torch path's gradient at its own weights, unclipped: the step's own draws repeated
            g = torch.Generator().manual_seed(500 + s)
            e = torch.randn((B, 17, 5), generator=g)
            t = training_timesteps(B, ra.num_timesteps, generator=g)
            kw = dict(dropout=True, dropout_seed=int(torch.randint(0, 2 ** 63 - 1, (1,), generator=g))) if dropout else {}
            _, gr = ra.model_diff.diffusion_loss_grad(i["x0"].to(dev), t, ra.betas, noise_scale=scale.to(dev),
                                                      noise=e.to(dev), mask=ra.src_mask, **kw)
            grads.append(gr.flat.cpu().numpy())
            _, gd = rb.model_diff.diffusion_loss_grad(i["x0"].to(dev), t, rb.betas, noise_scale=scale.to(dev),
                                                      noise=e.to(dev), mask=rb.src_mask, **kw)
            dgrads.append(gd.flat.cpu().numpy())
            sd_now = {k: p.detach().cpu().numpy() for k, p in params.items()}
            lo = GC.LC.loss_oracle(sd_now, i["adj"], i["layers"], i["heads"], GC.LC.x_t_ref(i["x0"], e, scale, t.float(), i["betas"]),
                                   GC.LC.target_ref(e, scale), i["mask"], t.float())
            bars.append((float(lo["loss64"].mean()), float(lo["bar"].mean())))
            la.append(ra.train_step(i["x0"], scale, topt, params, generator=torch.Generator().manual_seed(500 + s)))
            lb.append(rb.train_step(i["x0"], scale, dopt, generator=torch.Generator().manual_seed(500 + s)))
            if s == 0:
                first = ({k: p.detach().cpu().double().reshape(-1).numpy() for k, p in params.items()},
                         dopt._get("params")[0].cpu().double().numpy())
        assert np.array_equal(grads[0], dgrads[0])
        a64, d64 = OC.model64(o["params"], grads, clip=1.0), OC.model64(o["params"], dgrads, clip=1.0)
        last = ({k: p.detach().cpu().double().reshape(-1).numpy() for k, p in params.items()},
                dopt._get("params")[0].cpu().double().numpy())
        ok = True
        for step, (ta, got) in ((1, first), (5, last)):
            for k, off, n in layout:
                ma, md = a64[step - 1]["params"][off:off + n], d64[step - 1]["params"][off:off + n]
                gap = float(np.abs(ta[k] - ma).max())
                bar = max(OC.GAP_FACTOR * gap, OC.ulp32(float(np.abs(md).max())))
                ok = record_delta(float(np.abs(got[off:off + n] - md).max()), bar,
                                  f"device_optim/torch_path/{dropout}/step{step}/{k}") and ok
        for s, (l64, bar) in enumerate(bars):
            # eval mode: both losses against the float64 oracle at the step's weights; with dropout (no oracle for the
            # masks) against each other, at the same bar
            ok = record_delta(abs(lb[s] - (la[s] if dropout else l64)), bar, f"device_optim/torch_path/{dropout}/loss{s}") and ok
            if not dropout:
                ok = record_delta(abs(la[s] - l64), bar, f"device_optim/torch_path/{dropout}/loss{s}_torch") and ok
        assert ok
        assert dopt.step_count == 5
    finally:
        ra.model_diff.close()
        rb.model_diff.close()


def test_train_epoch(dev):
    from diffpose_amd.runner import Diffpose, default_args, default_config

    i = GC.inputs("g16")
    cfg = default_config()
    cfg.model = _config(GC.G16_SHAPE, dropout=0.0).model
    cfg.optim = ns(optimizer="Adam", lr=OC.LR, eps=OC.EPS, amsgrad=False, grad_clip=1.0)
    r = Diffpose(default_args(), cfg, device=dev)
    r.create_diffusion_model(state_dict=i["sd"])
    try:
        opt = r.model_diff.device_optimizer(cfg)
        B = i["x0"].shape[0]
        scale = i["scale"].repeat(B // i["scale"].shape[0], 1, 1)
        batches = [(i["x0"], scale), (i["x0"][:3], scale[:3])]
        avg = r.train_epoch(batches, opt, generator=torch.Generator().manual_seed(3))
        # the same two steps one at a time on a second model: AverageMeter's weighting
        r2 = Diffpose(default_args(), cfg, device=dev)
        r2.create_diffusion_model(state_dict=i["sd"])
        try:
            opt2 = r2.model_diff.device_optimizer(cfg)
            g = torch.Generator().manual_seed(3)
            l0 = r2.train_step(batches[0][0], batches[0][1], opt2, generator=g)
            l1 = r2.train_step(batches[1][0], batches[1][1], opt2, generator=g)
            assert avg == pytest.approx((l0 * B + l1 * 3) / (B + 3), rel=1e-6) and opt.step_count == 2
            assert torch.equal(opt._get("params")[0], opt2._get("params")[0])
        finally:
            r2.model_diff.close()
        with pytest.raises(TypeError):
            r.train_epoch(batches, torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1))
    finally:
        r.model_diff.close()


# ---------------------------------------------------------------------------------------
# 7. checkpoint round trip

@ends_session
def test_checkpoint_round_trip(dev):
    o = OC.inputs("g16")
    a, b = _model("g16", dev), _model("g16", dev)
    try:
        kw = dict(lr=OC.LR, amsgrad=True, grad_clip=1.0, ema_rate=OC.MU)
        oa, ob = a.device_optimizer(**kw), b.device_optimizer(**kw)
        for s in range(2):
            oa.step(torch.from_numpy(o["grads"][s]).to(dev))
        names = ("params", "exp_avg", "exp_avg_sq", "max_exp_avg_sq", "ema")
        saved = {}
        for k in names:
            saved[k], step = oa._get(k)
            assert step == 2
            ob._set(k, saved[k], step)
        sd = oa.state_dict()
        g3 = torch.from_numpy(o["grads"][2]).to(dev)
        na, nb = oa.step(g3), ob.step(g3)
        assert torch.equal(na, nb) and ob.step_count == 3
        after = _arrays(oa, names)
        for k, v in _arrays(ob, names).items():
            assert torch.equal(v, after[k]), k
        # the device's state in torch.optim.Adam on the CPU: its third step against the float64 model's third step from
        # the same state, the device's third step held to 8 x that gap
        layout, shapes = o["layout"], o["shapes"]
        p2 = saved["params"].cpu()
        ps = [torch.nn.Parameter(p2[off:off + n].reshape(shapes[k]).clone()) for k, off, n in layout]
        topt = torch.optim.Adam(ps, lr=OC.LR, betas=OC.BETAS, eps=OC.EPS, amsgrad=True)
        topt.load_state_dict(sd)
        for (k, off, n), q in zip(layout, ps):
            q.grad = torch.from_numpy(o["grads"][2][off:off + n]).reshape(shapes[k]).clone()
        torch.nn.utils.clip_grad_norm_(ps, 1.0)
        topt.step()
        init = dict(step=2, **{k: saved[k].cpu().numpy() for k in names[1:4]})
        m64 = OC.model64(p2.numpy(), [o["grads"][2]], amsgrad=True, clip=1.0, init=init)[0]["params"]
        ok = True
        for (k, off, n), q in zip(layout, ps):
            gap = float(np.abs(q.detach().double().reshape(-1).numpy() - m64[off:off + n]).max())
            bar = max(OC.GAP_FACTOR * gap, OC.ulp32(float(np.abs(m64[off:off + n]).max())))
            d = float(np.abs(after["params"][off:off + n].double().numpy() - m64[off:off + n]).max())
            ok = record_delta(d, bar, f"device_optim/checkpoint/{k}") and ok
        assert ok
        # and torch's state back into the device
        ob.load_state_dict(topt.state_dict())
        assert ob.step_count == 3
        v = ob._get("exp_avg_sq")[0].cpu()
        for (k, off, n), q in zip(layout, ps):
            assert torch.equal(v[off:off + n], topt.state[q]["exp_avg_sq"].reshape(-1)), k
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------------------------------
# 8. caller memory

@ends_session
def test_caller_memory(dev):
    L = _lib.lib()
    o = OC.inputs("g16")
    F = o["F"]
    m, twin = _model("g16", dev), _model("g16", dev)
    try:
        m.device_optimizer(lr=OC.LR, grad_clip=1.0)
        ref = twin.device_optimizer(lr=OC.LR, grad_clip=1.0)
        g = torch.from_numpy(o["grads"][0])
        want_norm = ref.step(g.to(dev)).reshape(1)
        want_p = ref._get("params")[0]
        st = _stream(dev)
        # between guard words at 4-byte-only alignment
        gin = CM.Guarded("grads_dev", (F,), device=dev, role="in", data=g, misaligned=True)
        gn = CM.Guarded("gnorm_dev", (1,), device=dev, role="out", misaligned=True)
        pout = CM.Guarded("out_dev", (F,), device=dev, role="out", misaligned=True)
        assert gin.alignment() == 4 and gn.alignment() == 4 and pout.alignment() == 4
        assert L.dpk_train_apply(m._h, gin.ptr, ctypes.c_float(OC.LR), gn.ptr, st) == 0
        assert L.dpk_train_get(m._h, 0, pout.ptr, None, st) == 0
        CM.check([gin, gn, pout], {"gnorm_dev": want_norm, "out_dev": want_p}, tag="device_optim/apply")
        sin = CM.Guarded("in_dev", (F,), device=dev, role="in", data=want_p.cpu(), misaligned=True)
        back = CM.Guarded("out_dev", (F,), device=dev, role="out", misaligned=True)
        assert L.dpk_train_set(m._h, 1, sin.ptr, -1, st) == 0 and L.dpk_train_get(m._h, 1, back.ptr, None, st) == 0
        CM.check([sin, back], {"out_dev": want_p}, tag="device_optim/set_get")
        assert L.dpk_train_set(m._h, 1, ref._get("exp_avg")[0].data_ptr(), -1, st) == 0
        # ending at the buffer's last byte, 4-byte aligned and no more: the tail of a buffer one float longer
        buf = torch.empty(F + 1, dtype=torch.float32, device=dev)
        buf[1:].copy_(torch.from_numpy(o["grads"][1]))
        one = torch.empty(2, dtype=torch.float32, device=dev)
        out = torch.empty(F + 1, dtype=torch.float32, device=dev)
        assert L.dpk_train_apply(m._h, buf.data_ptr() + 4, ctypes.c_float(OC.LR), one.data_ptr() + 4, st) == 0
        assert L.dpk_train_get(m._h, 0, out.data_ptr() + 4, None, st) == 0
        n2 = ref.step(torch.from_numpy(o["grads"][1]).to(dev))
        assert torch.equal(one[1], n2) and torch.equal(out[1:], ref._get("params")[0])
    finally:
        m.close()
        twin.close()


# ---------------------------------------------------------------------------------------
# 9. refusals

@ends_session
def test_refusals(dev):
    L = _lib.lib()
    m = _model("g16", dev)
    bare = HipGCNdiff(adj_mx_from_edges(17, GC.G16_SHAPE[4]), _config(GC.G16_SHAPE), device=dev)     # no weights
    try:
        cfg = lambda **k: ctypes.byref(_lib.DpkOptimConfig(**{**dict(beta1=0.9, beta2=0.999, eps=1e-8, amsgrad=0,   # noqa: E731
                                                                       grad_clip=1.0, ema_mu=-1.0), **k}))
        g = torch.zeros(OC.inputs("g16")["F"], dtype=torch.float32, device=dev)
        st = _stream(dev)
        assert L.dpk_train_apply(m._h, g.data_ptr(), ctypes.c_float(1e-3), None, st) == E_STATE and "dpk_train_begin" in _text(m)
        assert L.dpk_train_get(m._h, 0, g.data_ptr(), None, st) == E_STATE
        assert L.dpk_train_end(m._h) == E_STATE
        assert L.dpk_train_begin(bare._h, cfg()) == E_STATE and "weights" in _text(bare)
        assert L.dpk_train_begin(m._h, None) == E_INVALID and "NULL" in _text(m)
        for bad, word in ((dict(beta1=1.0), "beta1"), (dict(beta2=-0.1), "beta2"), (dict(beta1=float("nan")), "beta1"),
                          (dict(eps=-1e-8), "eps"), (dict(eps=float("nan")), "eps"), (dict(ema_mu=1.5), "ema_mu"),
                          (dict(ema_mu=float("nan")), "ema_mu")):
            assert L.dpk_train_begin(m._h, cfg(**bad)) == E_INVALID and word in _text(m), bad
        assert L.dpk_train_begin(m._h, cfg()) == 0
        assert L.dpk_train_begin(m._h, cfg()) == E_STATE and "already" in _text(m)
        assert L.dpk_train_apply(m._h, None, ctypes.c_float(1e-3), None, st) == E_INVALID
        assert L.dpk_train_apply(m._h, g.data_ptr(), ctypes.c_float(-1e-3), None, st) == E_INVALID and "lr" in _text(m)
        assert L.dpk_train_apply(m._h, g.data_ptr(), ctypes.c_float(float("nan")), None, st) == E_INVALID
        for which in (-1, 5):
            assert L.dpk_train_get(m._h, which, g.data_ptr(), None, st) == E_INVALID and "0..4" in _text(m)
        assert L.dpk_train_get(m._h, 3, g.data_ptr(), None, st) == E_INVALID and "amsgrad" in _text(m)
        assert L.dpk_train_get(m._h, 4, g.data_ptr(), None, st) == E_INVALID and "ema_mu" in _text(m)
        assert L.dpk_train_set(m._h, 3, g.data_ptr(), -1, st) == E_INVALID
        # on a capturing stream
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rc = L.dpk_train_apply(m._h, g.data_ptr(), ctypes.c_float(1e-3), None, _stream(dev))
            text = _text(m)
        assert rc == E_STATE and "captured" in text, (rc, text)
        del graph
        step = ctypes.c_int64(-1)
        assert L.dpk_train_get(m._h, 0, g.data_ptr(), ctypes.byref(step), st) == 0 and step.value == 0
        assert L.dpk_train_end(m._h) == 0
        # a GCNpose handle
        from diffpose_amd.gcnpose import HipGCNpose
        pose = HipGCNpose(adj_mx_from_edges(), None, device=dev)
        try:
            assert L.dpk_train_begin(pose._h, cfg()) == E_UNSUPPORTED and "GCNpose" in _text(pose)
        finally:
            pose.close()
    finally:
        m.close()
        bare.close()
