"""GPU: the denoising loss dpk_diff_loss / HipGCNdiff.diffusion_loss — per-pose-t noising, eps and the per-pose
ordered sums of (e * scale - eps)^2 — on every kind of GCNdiff handle, against the references and bars of
tests/diff_loss_cases.py (whose precondition tests/test_diff_loss_cpu.py checks on the same inputs):

  (a) x_t against the torch CPU expression ................................ bitwise
  (b) the returned eps against model(x_t, mask, t) on the same handle ..... bitwise
  (c) eps against the float64 oracle ...................................... max(5e-6, 8 g)
  (d) loss against the ordered fp32 sum restated on the host from the
      returned eps and fl(e * scale) ...................................... bitwise
  (e) loss against the float64 oracle, per pose ........................... 1e-5 * (sum |d64| + loss64)
"""
import ctypes
import functools
from types import SimpleNamespace as ns

import numpy as np
import pytest
import torch

import counter_draws as C
import diff_loss_cases as D
import edge_inputs as E
from conftest import record_delta
from diffpose_amd import _lib
from diffpose_amd._lib import DpkError
from diffpose_amd.gcndiff import HipGCNdiff, adj_mx_from_edges
from diffpose_amd.weights import synthetic_state_dict
from helpers import maxdiff as _maxdiff

pytestmark = pytest.mark.gpu


def ends_session(fn):
    """A library / HIP error is no parity miss: run nothing more on the device."""
    @functools.wraps(fn)
    def run(*a, **k):
        try:
            return fn(*a, **k)
        except DpkError as e:
            pytest.exit(f"diff_loss/{fn.__name__}: {e}", returncode=3)
    return run


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def models(dev):
    """One model per shape of diff_loss_cases.SHAPES (and "shipped", the 5-layer default) for the whole module"""
    made = {}

    def get(name):
        if name not in made:
            if name == "shipped":
                m = HipGCNdiff(adj_mx_from_edges(), None, device=dev)
                m.load_state_dict(synthetic_state_dict())
            else:
                hid, heads, layers, npts, edges = D.SHAPES[name]
                cfg = ns(model=ns(hid_dim=hid, emd_dim=hid, coords_dim=[5, 5], num_layer=layers, n_head=heads,
                                  dropout=0.25, n_pts=npts))
                m = HipGCNdiff(adj_mx_from_edges(npts, edges), cfg, device=dev)
                m.load_state_dict(D.inputs(name)["sd"])
            made[name] = m
        return made[name]

    yield get
    for m in made.values():
        m.close()


def _call(m, i, dev, **kw):
    """diffusion_loss(return_parts) on the case's inputs; (loss, x_t, eps) on the device"""
    args = dict(noise_scale=i["scale"].to(dev), noise=i["e"].to(dev), mask=i["mask"].to(dev), return_parts=True)
    args.update(kw)
    return m.diffusion_loss(i["x0"].to(dev), i["t"], i["betas"], **args)


def _check(tag, m, i, o, got, dev, oracle=True, mask=None):
    loss, x_t, eps = got
    mask = i["mask"].to(dev) if mask is None else mask
    for v in got:
        assert bool(torch.isfinite(v).all()), tag
    # (a)
    assert torch.equal(x_t.cpu(), i["x_t"]), (tag, _maxdiff(x_t, i["x_t"]))
    # (b)
    again = m(x_t, mask, i["t"].to(dev))
    assert torch.equal(eps, again), (tag, _maxdiff(eps, again))
    # (d)
    want = D.ordered_sum32(i["target"], eps)
    assert np.array_equal(loss.cpu().numpy(), want), (tag, loss.cpu().numpy(), want)
    if not oracle:
        return
    # (c)
    _, e64, g = o["eps"]
    assert g <= E.G_CEILING
    assert record_delta(_maxdiff(eps, e64), E.bar(g), tag + "/eps")
    # (e)
    ratio = np.abs(loss.cpu().double().numpy() - o["loss64"]) / o["bar"]
    print(f"{tag}: loss {loss.cpu().numpy()} |loss - loss64| / bar {ratio}")
    assert record_delta(float(ratio.max()), 1.0, tag + "/loss")


# ---------------------------------------------------------------------------------------
# 1. every kind of handle, fp32

HANDLES = [("h96", "four", "dpk/eps/sparse/fp32/z0"), ("h96", "two_pose", "dpk2/eps/sparse/fp32/z0"),
           ("dense", "four", "dpk/eps/dense/fp32/z0"), ("h128n8", None, "dpkw/eps/sparse/fp32/z0"),
           ("h64n2", None, "dpkn/eps/sparse/fp32/z0"), ("pad15", None, "dpk/eps/dense/fp32/z0/pad"), ("perop", None, None)]


@pytest.mark.parametrize("name,plan,kernel", HANDLES)
@ends_session
def test_fp32_on_every_handle(dev, models, name, plan, kernel):
    """N = 9: two full 4-pose tiles and a 1-pose tail (2-pose tiles: four and a tail); t hits both ends of the table;
    the 3-row scale.  The launch census says which eps kernel ran."""
    m = models(name)
    i, o = D.inputs(name), D.oracles(name)
    assert m.fused == (0 if kernel is None else 1)
    if plan:
        m.set_tail_plan(plan)
    try:
        m.debug_sampler_kernels()
        got = _call(m, i, dev)
        ran = m.debug_sampler_kernels()
        _check(f"diff_loss/{name}/{plan or 'default'}/fp32", m, i, o, got, dev)
    finally:
        if plan:
            m.set_tail_plan("step_split")
    assert ran == (set() if kernel is None else {kernel}), ran


@ends_session
def test_full_scale_rows(dev, models):
    """an N-row scale (rows == N), and None is ones"""
    m = models("h96")
    i, o = D.inputs("h96", True), D.oracles("h96", True)
    assert i["scale"].shape[0] == D.N
    _check("diff_loss/h96/full_scale/fp32", m, i, o, _call(m, i, dev), dev)
    i3 = D.inputs("h96")
    a = _call(m, i3, dev, noise_scale=None)
    b = _call(m, i3, dev, noise_scale=torch.ones(1, 17, 5, device=dev))
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert torch.equal(a[1].cpu(), D.x_t_ref(i3["x0"], i3["e"], None, i3["t"], i3["betas"]))
    assert np.array_equal(a[0].cpu().numpy(), D.ordered_sum32(i3["e"], a[2]))


@pytest.mark.parametrize("name", ["h96", "h128n8", "pad15"])
@ends_session
def test_fused_launch_is_the_three_launch_form_bitwise(dev, models, name, monkeypatch):
    """On a persistent handle the call is dpk_eps's one launch (noising in the tile load, the sum in the epilogue);
    DPK_LOSS_FUSED=0 runs the noising kernel, dpk_eps and the sum kernel instead.  Same bits, with the caller's e and
    with the counter-based draws, with every output and with loss alone.  Which form ran shows in the scratch: the
    fused call takes the 64-pose projection rows of a dpk_eps call alone, the three-launch form x_t and eps besides."""
    i = D.inputs(name)
    hid, heads, layers, npts, edges = D.SHAPES[name]
    cfg = ns(model=ns(hid_dim=hid, emd_dim=hid, coords_dim=[5, 5], num_layer=layers, n_head=heads, dropout=0.25,
                      n_pts=npts))
    m = HipGCNdiff(adj_mx_from_edges(npts, edges), cfg, device=dev)      # a fresh handle: its scratch is this test's
    def run():
        both = [_call(m, i, dev), _call(m, i, dev, noise=None, seed=11)]
        alone = _call(m, i, dev, return_parts=False)
        r = m.debug_resources()
        return both, alone, (r["eps_spare_poses"] if tps else r["generic_spare_kib"])

    # the spare only grows.  hid 96 counts it in poses of dpk_eps projection rows, at least 64 per dpk_eps-sized
    # request: the three-launch form first (it asks for its floats: under 64 poses' worth at N = 9), then the fused
    # call.  The other widths count KiB: the fused call first, then the larger three-launch request.
    tps = name != "h128n8"
    try:
        m.load_state_dict(i["sd"])
        if tps:
            monkeypatch.setenv("DPK_LOSS_FUSED", "0")
            three, alone3, spare_three = run()
            monkeypatch.delenv("DPK_LOSS_FUSED")
            fused, alone, spare_fused = run()
        else:
            fused, alone, spare_fused = run()
            monkeypatch.setenv("DPK_LOSS_FUSED", "0")
            three, alone3, spare_three = run()
    finally:
        m.close()
    for f, t3 in zip(fused, three):
        for u, v in zip(f, t3):
            assert torch.equal(u, v)
    assert torch.equal(alone, fused[0][0]) and torch.equal(alone3, alone)
    print(f"{name}: spare after the fused calls {spare_fused}, after the three-launch calls {spare_three}")
    if tps:
        assert spare_three < 64 and spare_fused == 64
    else:
        assert spare_three > spare_fused


# ---------------------------------------------------------------------------------------
# 2. the other gemm modes

@pytest.mark.parametrize("name,mode", [("h96", "f16x3"), ("h64n2", "f16x3"), ("h96", "bf16")])
@ends_session
def test_gemm_modes(dev, models, name, mode):
    """f16x3 at the fp32 bars; bf16 has no oracle bar: (a), (b) and (d) only"""
    m = models(name)
    i, o = D.inputs(name), D.oracles(name)
    m.set_gemm_mode(mode)
    try:
        got = _call(m, i, dev)
        _check(f"diff_loss/{name}/{mode}", m, i, o, got, dev, oracle=mode != "bf16")
    finally:
        m.set_gemm_mode("fp32")
    fp32 = _call(m, i, dev)
    assert torch.equal(fp32[1], got[1]) and not torch.equal(fp32[2], got[2])


# ---------------------------------------------------------------------------------------
# 3. per-pose masks

@pytest.mark.parametrize("name", ["h96", "pad15", "perop"])
@ends_session
def test_per_pose_masks(dev, models, name):
    """one all-masked pose and one single-key pose in the batch: (a), (b), (d); the masked poses' eps differ from the
    unmasked call's, the others' do not"""
    m = models(name)
    i = D.inputs(name)
    npts = i["x0"].shape[1]
    per = torch.ones(D.N, 1, npts, dtype=torch.bool)
    per[2] = False
    per[5] = False
    per[5, 0, 3] = True
    per = per.to(dev)
    plain = _call(m, i, dev)
    got = _call(m, i, dev, mask=per)
    _check(f"diff_loss/{name}/pose_masks", m, i, None, got, dev, oracle=False, mask=per)
    same = [p for p in range(D.N) if p not in (2, 5)]
    assert torch.equal(got[2][same], plain[2][same]) and torch.equal(got[0][same], plain[0][same])
    for p in (2, 5):
        assert not torch.equal(got[2][p], plain[2][p])
    _call(m, i, dev)          # back to the handle-wide mask


# ---------------------------------------------------------------------------------------
# 4. optional outputs and guards

def _raw(m, dev, x0, t, scale, rows, noise, seed, loss, xt, eps, n):
    p = lambda v: None if v is None else (v if isinstance(v, int) else v.data_ptr())   # noqa: E731
    return _lib.lib().dpk_diff_loss(m._h, p(x0), p(t), p(scale), rows, p(noise), ctypes.c_uint64(seed), p(loss), p(xt),
                                    p(eps), n, torch.cuda.current_stream(dev).cuda_stream)


@pytest.mark.parametrize("name", ["h96", "h128n8", "perop"])
@ends_session
def test_optional_outputs_and_guards(dev, models, name):
    """Each subset of the three outputs gives the bits of the full call, and nothing is written outside them: NaN
    guards of 64 floats before and after loss, x_t and eps stay NaN."""
    m = models(name)
    i = D.inputs(name)
    full = _call(m, i, dev)                      # binds the schedule and the mask
    x0, e, sc, t = i["x0"].to(dev), i["e"].to(dev), i["scale"].to(dev), i["t"].to(dev)
    n, G = D.N, 64
    sizes = (n, x0.numel(), x0.numel())
    for keep in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
        bufs = [torch.full((G + s + G,), float("nan"), device=dev) for s in sizes]
        ptrs = [b.data_ptr() + 4 * G if k else None for b, k in zip(bufs, keep)]
        rc = _raw(m, dev, x0, t, sc, sc.shape[0], e, 0, ptrs[0], ptrs[1], ptrs[2], n)
        _lib.check(m._h, "dpk_diff_loss", rc)
        torch.cuda.synchronize(dev)
        for b, k, s, want in zip(bufs, keep, sizes, full):
            assert bool(torch.isnan(b[:G]).all()) and bool(torch.isnan(b[G + s:]).all()), keep
            if k:
                assert torch.equal(b[G:G + s], want.reshape(-1)), keep
            else:
                assert bool(torch.isnan(b).all()), keep


# ---------------------------------------------------------------------------------------
# 5. uniform t is dpk_q_sample; the counter-based draws

@pytest.mark.parametrize("name", ["h96", "pad15", "perop"])
@ends_session
def test_uniform_t_is_q_sample_bitwise(dev, models, name):
    m = models(name)
    i = D.inputs(name)
    x0, e, sc = i["x0"].to(dev), i["e"].to(dev), i["scale"].to(dev)
    for ts in (0, 34, 50):
        t = [ts] * D.N
        _, x_t, _ = m.diffusion_loss(x0, t, i["betas"], noise_scale=sc, noise=e, return_parts=True)
        assert torch.equal(x_t, m.q_sample(x0, ts, sc, e)), ts
        assert torch.equal(x_t.cpu(), E.start_xT(i["x0"], i["e"], i["scale"], ts, i["betas"])), ts
        _, x_c, _ = m.diffusion_loss(x0, t, i["betas"], noise_scale=sc, noise=None, seed=C.SEED_C, return_parts=True)
        assert torch.equal(x_c, m.q_sample(x0, ts, sc, None, seed=C.SEED_C)), ts
        assert not torch.equal(x_c, x_t)


def _check_draws(tag, z, recover, seed):
    """z (float64, the draws read back, global elements 0..) against counter_draws.normal_ref at step -1 under the
    derived per-element bar, as tests/test_gpu_counter_draws.py checks the start"""
    ref, r = C.normal_ref(seed, -1, np.arange(z.size, dtype=np.int64))
    recover = np.broadcast_to(np.asarray(recover, np.float64), z.shape)
    assert np.isfinite(z).all() and float(recover.max()) <= C.RECOVER_MAX, tag
    bar = C.draw_bar(r, recover)
    d = np.abs(z - ref)
    ratio = np.where(bar > 0, d / np.where(bar > 0, bar, 1.0), np.where(d == 0, 0.0, np.inf))
    assert record_delta(float(ratio.max()), 1.0, tag), int((ratio > 1).sum())


@pytest.mark.parametrize("name", ["h96", "perop"])
@ends_session
def test_counter_based_site(dev, models, name):
    """noise=None draws normal_noise(seed, -1, global element), in the noising and in the loss alike.  Read without
    amplification: from x0 = 0 under counter_draws' schedule x_t = fl(fl(e scale) sb); and under the one-step
    schedule betas = [0.25] (abar = 0.75, sb = sqrtf(0.25) = 0.5 exactly) x_t = target / 2 exactly, so the target
    the loss used is 2 x_t and the host's ordered sum from it and the returned eps must be the loss, bitwise."""
    m = models(name)
    npts = D.SHAPES[name][3]
    n = 37                                        # ten tiles, the last with one pose
    zero = torch.zeros(n, npts, 5, device=dev)
    g = torch.Generator().manual_seed(19)
    rows = (0.25 + 2.0 * torch.rand((1, npts, 5), generator=g)).to(dev)
    den = rows.cpu().double().numpy().reshape(-1)
    seed = C.SEED_C + 3
    betas = torch.from_numpy(C.betas())
    _, x_t, _ = m.diffusion_loss(zero, [C.T_START] * n, betas, noise_scale=rows, noise=None, seed=seed,
                                 return_parts=True)
    assert torch.equal(x_t, m.q_sample(zero, C.T_START, rows, None, seed=seed))
    v = x_t.cpu().double().numpy().reshape(n, -1) / (den * C.start_sb())
    _check_draws(f"diff_loss/counter/{name}/x_t", v.reshape(-1), 2.0 ** -23 * np.abs(v.reshape(-1)), seed)
    # the loss's own read of the same draws
    half = torch.tensor([0.25])
    for sc in (None, rows):
        loss, x_t, eps = m.diffusion_loss(zero, [0] * n, half, noise_scale=sc, noise=None, seed=seed,
                                          return_parts=True)
        target = 2.0 * x_t.cpu()
        assert np.array_equal(loss.cpu().numpy(), D.ordered_sum32(target, eps)), sc is None
        assert torch.equal(eps, m(x_t, None, torch.zeros(n, device=dev)))
        z = target.double().numpy().reshape(n, -1) / (1.0 if sc is None else den)
        rec = 0.0 if sc is None else 2.0 ** -24 * np.abs(z.reshape(-1))
        _check_draws(f"diff_loss/counter/{name}/target/{'ones' if sc is None else 'scaled'}", z.reshape(-1), rec, seed)
    # another seed, other draws; a part of the batch, the same draws
    a = m.diffusion_loss(zero, [0] * n, half, seed=seed)
    assert torch.equal(a, loss) is False and torch.equal(m.diffusion_loss(zero, [0] * n, half, seed=seed), a)
    assert not torch.equal(m.diffusion_loss(zero, [0] * n, half, seed=seed + 1), a)
    assert torch.equal(m.diffusion_loss(zero[:5].contiguous(), [0] * 5, half, seed=seed), a[:5])


# ---------------------------------------------------------------------------------------
# 6. graph capture

@pytest.mark.parametrize("name", ["h96", "h128n8", "perop"])
@ends_session
def test_capture_replays_bitwise_and_keeps_its_schedule(dev, models, name):
    m = models(name)
    i = D.inputs(name)
    x0, e, sc, t = i["x0"].to(dev), i["e"].to(dev), i["scale"].to(dev), i["t"].to(dev)
    mask = i["mask"].to(dev)
    kw = dict(noise_scale=sc, noise=e, mask=mask, return_parts=True)
    eager = [v.clone() for v in m.diffusion_loss(x0, t, i["betas"], **kw)]
    other = torch.randn(e.shape, generator=torch.Generator().manual_seed(4)).to(dev)
    eager_other = [v.clone() for v in m.diffusion_loss(x0, t, i["betas"], noise_scale=sc, noise=other, mask=mask,
                                                       return_parts=True)]
    assert not torch.equal(eager[0], eager_other[0])
    # the eager calls above were the uncaptured warm-up: they left the pool a spare of this call's size
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = m.diffusion_loss(x0, t, i["betas"], **kw)
    try:
        for want, src in ((eager, None), (eager_other, other), (eager, i["e"].to(dev))):
            if src is not None:
                e.copy_(src)
            for v in out:
                v.zero_()
            g.replay()
            torch.cuda.synchronize(dev)
            for a, b in zip(out, want):
                assert torch.equal(a, b)
        # another schedule bound after the capture: the graph keeps the table it was captured with
        m.set_schedule([0, 10], torch.linspace(0.01, 0.2, 30), 0.0)
        for v in out:
            v.zero_()
        g.replay()
        torch.cuda.synchronize(dev)
        for a, b in zip(out, eager):
            assert torch.equal(a, b)
    finally:
        del g
    # and an eager call afterwards binds the betas again
    for a, b in zip(m.diffusion_loss(x0, t, i["betas"], **kw), eager):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------
# 7. refusals (no bad t reaches the device)

@ends_session
def test_refusals(dev, models):
    from diffpose_amd.gcnpose import HipGCNpose

    for name in ("h96", "perop"):
        m = models(name)
        i = D.inputs(name)
        x0, e, sc, t = i["x0"].to(dev), i["e"].to(dev), i["scale"].to(dev), i["t"].to(dev)
        _call(m, i, dev)
        loss = torch.empty(D.N, device=dev)
        # all outputs null
        rc = _raw(m, dev, x0, t, sc, 3, e, 0, None, None, None, D.N)
        assert rc == -1 and b"all null" in _lib.lib().dpk_last_error(m._h)
        # scale rows that do not divide N, in start_spec's wording
        with pytest.raises(DpkError, match="scale_rows 4 must be at least 1 and divide N = 9") as ei:
            _call(m, i, dev, noise_scale=torch.ones(4, x0.shape[1], 5, device=dev))
        assert ei.value.code == -1
        rc = _raw(m, dev, x0, t, sc, 0, e, 0, loss, None, None, D.N)
        assert rc == -1
        # a CPU t is checked: out of range, negative, non-integer, NaN, the wrong count; as list, numpy and tensor
        T = i["betas"].numel()
        for bad in ([0] * 8 + [T], [-1] + [0] * 8, [0.5] + [0] * 8, np.array([0] * 8 + [T]), torch.tensor([0.0] * 8 + [float("nan")]),
                    [0] * 8, [0] * 10):
            with pytest.raises(ValueError):
                m.diffusion_loss(x0, bad, i["betas"], noise_scale=sc, noise=e)
        m.diffusion_loss(x0, [T - 1] * D.N, i["betas"], noise_scale=sc, noise=e)
        with pytest.raises(ValueError):
            m.diffusion_loss(x0, i["t"], i["betas"], noise_scale=sc, noise=e[:5])
        with pytest.raises((ValueError, TypeError)):
            m.diffusion_loss(i["x0"], i["t"], i["betas"])            # x0 on the CPU
    # no schedule bound: start_spec's refusal
    x0 = torch.zeros(2, 17, 5, device=dev)
    tz, loss = torch.zeros(2, device=dev), torch.empty(2, device=dev)
    fresh = HipGCNdiff(adj_mx_from_edges(), None, device=dev)
    try:
        fresh.load_state_dict(synthetic_state_dict())
        rc = _raw(fresh, dev, x0, tz, None, 0, None, 0, loss, None, None, 2)
        assert rc == -1 and b"dpk_diff_loss: no schedule set (dpk_set_schedule)" in _lib.lib().dpk_last_error(fresh._h)
    finally:
        fresh.close()
    # a GCNpose handle
    pose = HipGCNpose(adj_mx_from_edges(), None, device=dev)
    try:
        pose.load_state_dict(synthetic_state_dict(kind="pose"))
        rc = _raw(pose, dev, x0, tz, None, 0, None, 0, loss, None, None, 2)
        assert rc == -2 and _lib.ERRORS[rc] == "DPK_E_UNSUPPORTED"
    finally:
        pose.close()


# ---------------------------------------------------------------------------------------
# 8. the reference's own training forward (fixture g15), and the runner

@ends_session
def test_golden_g15(dev, models, golden):
    z = D.golden_g15(golden)
    m = models("shipped")
    target = D.target_ref(z["e"], z["noise_scale"])
    loss, x_t, eps = m.diffusion_loss(z["x"].to(dev), z["t"], z["betas"], noise_scale=z["noise_scale"].to(dev),
                                      noise=z["e"].to(dev), mask=torch.ones(1, 1, 17, dtype=torch.bool, device=dev),
                                      return_parts=True)
    assert torch.equal(x_t.cpu(), z["x_t"])
    assert record_delta(_maxdiff(eps, z["eps"]), 5e-6, "diff_loss/g15/eps")
    o = D.loss_oracle(synthetic_state_dict(), adj_mx_from_edges(), 5, 4, z["x_t"], target,
                      torch.ones(1, 1, 17, dtype=torch.bool), z["t"].float())
    ratio = np.abs(loss.cpu().double().numpy() - o["loss64"]) / o["bar"]
    assert record_delta(float(ratio.max()), 1.0, "diff_loss/g15/loss")
    # the reference's own float32 sums sit inside the same bar, and the batch mean is its loss_diff to that bar
    assert float((np.abs(z["sums"].double().numpy() - o["loss64"]) / o["bar"]).max()) <= 1.0
    assert abs(float(loss.mean()) - float(z["loss_diff"])) <= 2.0 * float(o["bar"].mean())
    # through utils_diff, the same call
    from diffpose_amd.utils_diff import diffusion_loss

    again = diffusion_loss(m, z["x"].to(dev), z["t"], z["betas"], noise_scale=z["noise_scale"].to(dev),
                           noise=z["e"].to(dev), mask=torch.ones(1, 1, 17, dtype=torch.bool, device=dev))
    assert torch.equal(again, loss)


@ends_session
def test_runner_diffusion_loss_vs_oracle(dev):
    """Diffpose.diffusion_loss on two synthetic batches (6 and 5 poses) against the same pipeline built from the
    float64 oracle: e and t from one CPU generator seeded with args.seed, drawn batch by batch.  The bar is the
    mean of the per-pose loss bars (the epoch value is a mean of per-pose losses) plus 1e-6 of the value for the
    two fp32 means (at most 6 terms, 6 * 2^-24 each, rounded up)."""
    from diffpose_amd import runner
    from diffpose_amd.schedule import training_timesteps

    cfg = runner.default_config()
    dp = runner.Diffpose(runner.default_args(seed=4243), cfg, device=dev)
    dp.create_diffusion_model()
    rng = np.random.Generator(np.random.PCG64(808))
    batches = []
    for n in (6, 5):
        x = rng.normal(0, 0.3, size=(n, 17, 5)).astype(np.float32)
        sc = np.ones((n, 17, 5), np.float32)
        sc[:, :, :2] = 0.25 + 2.0 * rng.random(size=(n, 17, 2))
        batches.append((x, sc))
    got = dp.diffusion_loss(batches=batches)
    gen = torch.Generator().manual_seed(4243)
    tot = bar = 0.0
    for x, sc in batches:
        n = x.shape[0]
        e = torch.randn((n, 17, 5), generator=gen)
        t = training_timesteps(n, 51, generator=gen)
        x, sc = torch.from_numpy(x), torch.from_numpy(sc)
        o = D.loss_oracle(synthetic_state_dict(), adj_mx_from_edges(), 5, 4, D.x_t_ref(x, e, sc, t, dp.betas.cpu()),
                          D.target_ref(e, sc), torch.ones(1, 1, 17, dtype=torch.bool), t.float())
        tot += float(o["loss64"].mean()) * n
        bar += float(o["bar"].mean()) * n
    want, bar = tot / 11, bar / 11 + 1e-6 * tot / 11
    print(f"runner: epoch loss {got!r}, oracle {want!r}, bar {bar:.3e}")
    assert record_delta(abs(got - want), bar, "diff_loss/runner/epoch")
    assert dp.epoch_loss_diff == got and got > 1.0
    with pytest.raises(NotImplementedError):
        dp.model_diff.train()
