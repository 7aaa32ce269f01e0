"""GPU: the noised hypothesis start x_T = x*sqrt(a) + (e*noise_scale)*sqrt(1 - a), a = alpha_bar[t_start + 1],
inside the sampler (dpk_sample_start), alone (dpk_q_sample) and through generalized_steps and the runner.

The reference never executes this line (runners/diffpose_frame.py:363 is commented out), so no fixture of
its can pin it.  The yardstick is the reference's own expression evaluated by torch on the CPU from
schedule.alpha_bar_table, which the kernel must match bitwise on valid rows (four fp32 roundings, no FMA),
and the bit-exact oracle's DDIM loop started from that x_T, at the project's 5e-6 elementwise.

The statistical bounds on the counter-based draws are derived, not measured: over n independent standard
normals the sample mean has standard deviation 1/sqrt(n) and the sample variance sqrt(2/n); five of each
(a 6e-7 two-sided event) is the bar, and 5/sqrt(n) likewise for the correlation of two independent streams.
Recovering e = (x_T - x*sa)/sb from fp32 values perturbs it by about 2^-23 |x| sa / sb <= 1e-6, far below
5/sqrt(n) = 1.7e-2.
"""
import ctypes
import functools
import math
from types import SimpleNamespace as ns

import numpy as np
import pytest
import torch

from conftest import record_delta
from diffpose_amd import _lib
from diffpose_amd._lib import DpkError
from diffpose_amd.data import synthetic_batch
from diffpose_amd.gcndiff import H36M_EDGES, HipGCNdiff, adj_mx_from_edges
from diffpose_amd.schedule import alpha_bar_table, make_seq
from diffpose_amd.weights import synthetic_state_dict
from helpers import betas as _betas, maxdiff as _maxdiff

pytestmark = pytest.mark.gpu

TOL = 5e-6
T_START = 50                    # the reference's t = test_num_diffusion_timesteps (:355) under a 51-step beta
CHAIN16 = tuple((i, i + 1) for i in range(15))
SEQ10 = make_seq("uniform", 50, 10)
# name: hid, heads, layers, joints, edges — the five persistent-sampler instance shapes and a per-op shape
SHAPES = {
    "h96n4": (96, 4, 5, 17, H36M_EDGES),
    "h128n8": (128, 8, 3, 17, H36M_EDGES),
    "h128n4": (128, 4, 3, 17, H36M_EDGES),
    "h64n2": (64, 2, 2, 17, H36M_EDGES),
    "h64n4": (64, 4, 2, 17, H36M_EDGES),
    "perop": (48, 4, 1, 16, CHAIN16),
}


def ends_session(fn):
    """A library / HIP error is no parity miss: run nothing more on the device."""
    @functools.wraps(fn)
    def run(*a, **k):
        try:
            return fn(*a, **k)
        except DpkError as e:
            pytest.exit(f"hypothesis_start/{fn.__name__}: {e}", returncode=3)
    return run


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _sd(name):
    hid, _, layers, npts, _ = SHAPES[name]
    return synthetic_state_dict(hid=hid, n_layers=layers, n_pts=npts)


@pytest.fixture(scope="module")
def models(dev):
    """One model per shape for the whole module, closed at its end."""
    made = {}

    def get(name):
        if name not in made:
            hid, heads, layers, npts, edges = SHAPES[name]
            cfg = ns(model=ns(hid_dim=hid, emd_dim=hid, coords_dim=[5, 5], num_layer=layers, n_head=heads,
                              dropout=0.25, n_pts=npts))
            m = HipGCNdiff(adj_mx_from_edges(npts, edges), cfg, device=dev)
            m.load_state_dict(_sd(name))
            made[name] = m
        return made[name]

    yield get
    for m in made.values():
        m.close()


@functools.lru_cache(maxsize=None)
def _oracle(name):
    from oracle import gcndiff_oracle as O

    _, heads, layers, npts, edges = SHAPES[name]
    P = O.params_to_torch(_sd(name))
    g = O.adjacency(npts, edges)
    return O, lambda a, mk, t: O.gcndiff_forward(P, g, a, mk, t, n_layers=layers, heads=heads)


def _inputs(n, npts=17, seed=1):
    """x, e and a noise_scale with u, v entries != 1 ([var_u, var_v, 1, 1, 1] per joint), on the CPU"""
    x = torch.from_numpy(synthetic_batch(n, seed=seed)[0])[:, :npts].contiguous()
    g = torch.Generator().manual_seed(1000 + seed)
    e = torch.randn(x.shape, generator=g)
    scale = torch.ones(x.shape)
    scale[:, :, :2] = 0.25 + 2.0 * torch.rand((n, npts, 2), generator=g)
    return x, e, scale


def _sqrt32(v: torch.Tensor) -> torch.Tensor:
    """sqrtf of a one-element float32 tensor, correctly rounded: the float64 square root (libm, correctly rounded)
    rounded once more to float32, which is the correctly rounded float32 root (53 >= 2 * 24 + 2 bits).  torch's own
    float32 ``.sqrt()`` is not that on every CPU: on some AVX-512 hosts it returns 0x1.f8ddf2p-1 for
    a = 0x1.f1d552p-1 (the alpha-bar of t = 50 here), 0.67 ulp from the root 0.98606826833926..., where sqrtf,
    numpy and torch on other hosts give 0x1.f8ddf0p-1.  The product takes sqrtf on the host (diffpose_kernels.h)."""
    assert v.dtype == torch.float32 and v.numel() == 1
    return torch.tensor(math.sqrt(float(v)), dtype=torch.float32).view(1, 1, 1)


def x_T(x, e, scale, t_start=T_START, b=None):
    """runners/diffpose_frame.py:355-363 in torch on the CPU, a from the host's alpha-bar table: torch's float32
    subtraction, products and sum in the reference's order, the two square roots through _sqrt32"""
    a = torch.from_numpy(alpha_bar_table((_betas() if b is None else b).numpy()))[t_start + 1].view(1, 1, 1)
    e = e * scale
    return x * _sqrt32(a) + e * _sqrt32(1.0 - a)


def _ones(npts, dev=None):
    m = torch.ones(1, 1, npts, dtype=torch.bool)
    return m if dev is None else m.to(dev)


# ---------------------------------------------------------------------------------------
# 1. xs[0] is the torch expression, bitwise

@pytest.mark.parametrize("name,n", [("h96n4", 11), ("h128n8", 7), ("perop", 11)])
@ends_session
def test_xs0_is_the_torch_expression_bitwise(dev, models, name, n):
    """h96n4 under plan "four": 11 poses = two full 4-pose tiles and a 3-pose tail; h128n8: 2-pose tiles, the last
    half empty; the per-op handle: dpkg::qsample on a 16-joint chain."""
    m = models(name)
    npts = SHAPES[name][3]
    x, e, scale = _inputs(n, npts, seed=3)
    m.set_tail_plan("four")
    try:
        xs, _ = m.sample(x.to(dev), SEQ10, _betas(), mask=_ones(npts, dev), trajectory=True, t_start=T_START,
                         start_scale=scale.to(dev), start_noise=e.to(dev))
    finally:
        m.set_tail_plan("step_split")
    ref = x_T(x, e, scale)
    assert not torch.equal(ref, x)
    assert torch.equal(xs[0].cpu(), ref), _maxdiff(xs[0], ref)
    # the stand-alone form gives the same bits
    assert torch.equal(m.q_sample(x.to(dev), T_START, scale.to(dev), e.to(dev)).cpu(), ref)


# ---------------------------------------------------------------------------------------
# 2. trajectory and final against the oracle started from x_T

@pytest.mark.parametrize("eta", [0.0, 0.5])
@pytest.mark.parametrize("name,mode", [(k, "fp32") for k in SHAPES] + [("h64n2", "f16x3")])
@ends_session
def test_trajectory_vs_oracle(dev, models, name, mode, eta):
    O, fwd = _oracle(name)
    m = models(name)
    npts = SHAPES[name][3]
    n = 11
    x, e, scale = _inputs(n, npts, seed=5)
    z = None
    if eta != 0.0:
        z = torch.randn((len(SEQ10),) + tuple(x.shape), generator=torch.Generator().manual_seed(77))
    m.set_gemm_mode(mode)
    try:
        xs, x0s = m.sample(x.to(dev), SEQ10, _betas(), eta=eta, mask=_ones(npts, dev), trajectory=True,
                           noise=None if z is None else z.to(dev), t_start=T_START, start_scale=scale.to(dev),
                           start_noise=e.to(dev))
        out = m.sample(x.to(dev), SEQ10, _betas(), eta=eta, mask=_ones(npts, dev),
                       noise=None if z is None else z.to(dev), t_start=T_START, start_scale=scale.to(dev),
                       start_noise=e.to(dev))
    finally:
        m.set_gemm_mode("fp32")
    rxs, rx0s = O.generalized_steps(x_T(x, e, scale), _ones(npts), SEQ10, fwd, _betas(), eta=eta, noise=z)
    tag = f"hypothesis_start/{name}/{mode}/eta{eta}"
    assert torch.equal(xs[0].cpu(), rxs[0])
    assert record_delta(_maxdiff(xs, torch.stack(rxs)), TOL, tag + "/xs")
    assert record_delta(_maxdiff(x0s, torch.stack(rx0s)), TOL, tag + "/x0s")
    assert torch.equal(out, xs[-1])


# ---------------------------------------------------------------------------------------
# 3. scale rows broadcast hypothesis-major; None is ones

@pytest.mark.parametrize("name", ["h96n4", "perop"])
@ends_session
def test_scale_broadcast(dev, models, name):
    m = models(name)
    npts = SHAPES[name][3]
    F = 5
    x, e, scale = _inputs(3 * F, npts, seed=7)
    kw = dict(mask=_ones(npts, dev), trajectory=True, t_start=T_START, start_noise=e.to(dev))
    rows = scale[:F].contiguous()
    a, _ = m.sample(x.to(dev), SEQ10[:3], _betas(), start_scale=rows.to(dev), **kw)
    b, _ = m.sample(x.to(dev), SEQ10[:3], _betas(), start_scale=rows.repeat(3, 1, 1).to(dev), **kw)
    assert torch.equal(a, b)
    assert torch.equal(a[0].cpu(), x_T(x, e, rows.repeat(3, 1, 1)))
    a, _ = m.sample(x.to(dev), SEQ10[:3], _betas(), start_scale=None, **kw)
    b, _ = m.sample(x.to(dev), SEQ10[:3], _betas(), start_scale=torch.ones_like(x).to(dev), **kw)
    assert torch.equal(a, b)
    assert torch.equal(a[0].cpu(), x_T(x, e, torch.ones_like(x)))


# ---------------------------------------------------------------------------------------
# 4. the start off is today's path

@pytest.mark.parametrize("name", ["h96n4", "h64n2", "perop"])
@ends_session
def test_start_off_is_the_plain_sampler(dev, models, name):
    m = models(name)
    npts = SHAPES[name][3]
    x, e, scale = _inputs(13, npts, seed=9)
    xd = x.to(dev)

    def plain():       # dpk_sample through its own entry point
        out = torch.empty_like(xd)
        m.set_schedule(SEQ10, _betas(), 0.0)
        rc = _lib.lib().dpk_sample(m._h, xd.data_ptr(), out.data_ptr(), None, None, xd.shape[0],
                                   ctypes.c_uint64(0), torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(m._h, "dpk_sample", rc)
        return out

    first = plain()
    xs, _ = m.sample(xd, SEQ10, _betas(), mask=_ones(npts, dev), trajectory=True, t_start=None)
    assert xs[0].data_ptr() != xd.data_ptr() and torch.equal(xs[0], xd) and torch.equal(xs[-1], first)
    assert torch.equal(m.sample(xd, SEQ10, _betas(), mask=_ones(npts, dev), t_start=None), first)
    on = m.sample(xd, SEQ10, _betas(), mask=_ones(npts, dev), t_start=T_START, start_scale=scale.to(dev),
                  start_noise=e.to(dev))
    assert not torch.equal(on, first)
    # after a start-on call on the same handle
    assert torch.equal(m.sample(xd, SEQ10, _betas(), mask=_ones(npts, dev), t_start=None), first)
    assert torch.equal(plain(), first)
    # t_start < 0 through the new entry point is the same call
    out = torch.empty_like(xd)
    rc = _lib.lib().dpk_sample_start(m._h, xd.data_ptr(), out.data_ptr(), None, None, xd.shape[0], ctypes.c_uint64(0),
                                     None, -1, scale.to(dev).data_ptr(), 13, e.to(dev).data_ptr(),
                                     torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(m._h, "dpk_sample_start", rc)
    assert torch.equal(out, first)


# ---------------------------------------------------------------------------------------
# 5. counter-based draws

def _sa_sb(t_start=T_START):
    a = torch.from_numpy(alpha_bar_table(_betas().numpy()))[t_start + 1]
    return float(_sqrt32(a)), float(_sqrt32(1.0 - a))


@pytest.mark.parametrize("name", ["h96n4", "perop"])
@ends_session
def test_counter_based_draws_repeat_and_do_not_depend_on_the_batch(dev, models, name):
    m = models(name)
    npts = SHAPES[name][3]
    x = _inputs(23, npts, seed=11)[0].to(dev)
    kw = dict(mask=_ones(npts, dev), trajectory=True, t_start=T_START)
    a, _ = m.sample(x, SEQ10[:2], _betas(), seed=5, **kw)
    b, _ = m.sample(x, SEQ10[:2], _betas(), seed=5, **kw)
    c, _ = m.sample(x, SEQ10[:2], _betas(), seed=6, **kw)
    assert torch.equal(a, b)
    assert _maxdiff(a[0], c[0]) > 1e-2
    part, _ = m.sample(x[:5].contiguous(), SEQ10[:2], _betas(), seed=5, **kw)
    assert torch.equal(part, a[:, :5])
    assert torch.equal(m.q_sample(x, T_START, seed=5), a[0])


@ends_session
def test_counter_based_draws_are_standard_normal_and_apart_from_the_step_draws(dev, models):
    m = models("h96n4")
    N = 1024
    x = torch.from_numpy(synthetic_batch(N, seed=13)[0]).to(dev)
    seq = SEQ10[:3]
    xs, _ = m.sample(x, seq, _betas(), eta=0.5, seed=21, mask=_ones(17, dev), trajectory=True, noise=None,
                     t_start=T_START)
    sa, sb = _sa_sb()
    e = ((xs[0].double() - x.double() * sa) / sb).cpu().reshape(-1)
    n = e.numel()
    assert n == 87040
    mean, var = float(e.mean()), float(e.var(unbiased=True))
    print(f"start draws: n {n} mean {mean:.3e} (bar {5 / np.sqrt(n):.3e}) var-1 {var - 1:.3e} (bar {5 * np.sqrt(2 / n):.3e})")
    assert abs(mean) <= 5.0 / np.sqrt(n)
    assert abs(var - 1.0) <= 5.0 * np.sqrt(2.0 / n)
    # eta's draws of the same seed at steps 0..K-1: x' = c1 * z from x_t = eps = 0
    zero = torch.zeros_like(x)
    m.set_schedule(seq, _betas(), 0.5)
    for step in range(len(seq) - 1):         # the last step's c1 is 0 (alpha-bar of t = -1 is 1): its draw enters nothing
        xn, _ = m.ddim_update(zero, zero, step, seed=21)
        z = xn.double().cpu().reshape(-1)
        z = z / z.std()
        assert float(z.abs().max()) > 0
        corr = float((e * z).mean())
        print(f"step {step}: corr {corr:.3e}")
        assert abs(corr) <= 5.0 / np.sqrt(n)


# ---------------------------------------------------------------------------------------
# 6. tail plans and tile instances

@ends_session
def test_plans_and_tiles_bitwise(dev, models):
    """1,100 poses = 275 tiles: on a 256-CU device one full round and 19 tiles, which plan "step_split" runs as
    two halves each; debug_split(1) makes every second half recompute from x_in (and so apply the start itself)."""
    m = models("h96n4")
    N = 1100
    x, e, scale = _inputs(N, seed=15)
    rows = scale[:N // 4].contiguous().to(dev)          # four hypothesis blocks share 275 scale rows
    xd, ed = x.to(dev), e.to(dev)

    def run():
        xs, x0s = m.sample(xd, SEQ10, _betas(), mask=_ones(17, dev), trajectory=True, t_start=T_START,
                           start_scale=rows, start_noise=ed)
        return torch.cat([xs, x0s])

    try:
        m.set_tail_plan("four")
        m.set_tile_waves(4)
        four = run()
        assert torch.equal(four[0].cpu(), x_T(x, e, scale[:N // 4].repeat(4, 1, 1)))
        m.set_tile_waves(8)
        assert torch.equal(run(), four)
        m.set_tile_waves(4)
        m.set_tail_plan("step_split")
        assert torch.equal(run(), four)
        m.debug_split(1)
        assert torch.equal(run(), four)
        fallbacks = m.debug_split(0, read=True)
        print("second halves that recomputed:", fallbacks)
        m.set_tail_plan("two_pose")
        two = run()
        assert torch.equal(two[:, :1024], four[:, :1024])
        assert torch.equal(two[0], four[0])
        assert _maxdiff(two, four) <= TOL
    finally:
        m.debug_split(0)
        m.set_tail_plan("step_split")
        m.set_tile_waves(0)


# ---------------------------------------------------------------------------------------
# 7. graph capture

@pytest.mark.parametrize("name", ["h96n4", "h128n4"])
@ends_session
def test_start_under_capture(dev, models, name):
    m = models(name)
    x, e, scale = _inputs(24, seed=17)
    other = torch.randn(e.shape, generator=torch.Generator().manual_seed(4))
    xd, ed, sd = x.to(dev), e.to(dev), scale.to(dev)
    kw = dict(mask=_ones(17, dev), t_start=T_START, start_scale=sd)
    seq = SEQ10[:4]
    eager = m.sample(xd, seq, _betas(), start_noise=ed, **kw).clone()
    eager_other = m.sample(xd, seq, _betas(), start_noise=other.to(dev), **kw).clone()
    assert not torch.equal(eager, eager_other)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):                 # uncaptured warm-up on the capture's side stream
        m.sample(xd, seq, _betas(), start_noise=ed, **kw)
    torch.cuda.current_stream(dev).wait_stream(s)
    out = torch.empty_like(xd)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        m.sample(xd, seq, _betas(), start_noise=ed, out=out, **kw)
    for want, src in ((eager, None), (eager_other, other), (eager, e)):
        if src is not None:
            ed.copy_(src.to(dev))
        out.zero_()
        g.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(out, want)
    del g


# ---------------------------------------------------------------------------------------
# 8. a generic model callable through generalized_steps

@ends_session
def test_generic_callable_matches_the_fused_call(dev, models):
    from diffpose_amd.utils_diff import generalized_steps

    m = models("h96n4")
    x, e, scale = _inputs(9, seed=19)
    xd = x.to(dev)
    kw = dict(t_start=T_START, start_scale=scale.to(dev), start_noise=e.to(dev))
    fxs, fx0s = generalized_steps(xd, _ones(17, dev), SEQ10, m, _betas(), **kw)
    gxs, gx0s = generalized_steps(xd, _ones(17, dev), SEQ10, lambda a, mk, t, c: m(a, mk, t, c), _betas(), **kw)
    assert fxs[0] is not xd and gxs[0] is not xd
    assert torch.equal(fxs[0].cpu(), x_T(x, e, scale)) and torch.equal(gxs[0], fxs[0])
    assert len(gxs) == len(fxs) == 11 and len(gx0s) == len(fx0s) == 10
    assert record_delta(_maxdiff(torch.stack(gxs), torch.stack(fxs)), TOL)
    assert record_delta(_maxdiff(torch.stack(gx0s), torch.stack(fx0s)), TOL)
    # without a start xs[0] is the input object, as before
    assert generalized_steps(xd, _ones(17, dev), SEQ10[:2], m, _betas())[0][0] is xd
    # the "torch" source is the reference's randn_like draw on x's device
    torch.manual_seed(31)
    want = torch.randn_like(xd)
    torch.manual_seed(31)
    txs, _ = generalized_steps(xd, _ones(17, dev), SEQ10[:2], m, _betas(), t_start=T_START)
    assert torch.equal(txs[0].cpu(), x_T(x, want.cpu(), torch.ones_like(x)))


# ---------------------------------------------------------------------------------------
# 9. the runner

@ends_session
def test_runner_noise_start_vs_oracle(dev):
    """test_hyber with noise_start, H = 4, 32 frames in two batches, K = 10, against the same pipeline built from
    the oracle with :363 switched on: e = randn for the whole batch from the CPU generator, times the batch's
    noise_scale repeated hypothesis-major."""
    from oracle import gcndiff_oracle as O
    from oracle import metrics_oracle as M
    from diffpose_amd import metrics, runner
    from diffpose_amd.data import synthetic_eval_batches

    H = 4
    cfg = runner.default_config(test_times=H, test_timesteps=10, test_num_diffusion_timesteps=50, batch_size=16)
    args = runner.default_args(noise_start=True, noise="torch-cpu")
    dp = runner.Diffpose(args, cfg, device=dev)
    dp.create_diffusion_model()
    dp.create_pose_model()
    g = torch.Generator().manual_seed(8)
    batches = []
    for x2d, tgt, acts in synthetic_eval_batches(32, 16, seed=4243):
        sc = np.ones((len(x2d), 17, 5), np.float32)
        sc[:, :, :2] = (0.25 + 2.0 * torch.rand((len(x2d), 17, 2), generator=g)).numpy()
        batches.append((x2d, tgt, acts, sc))
    outs = []
    plain = dp.model_diff.sample

    def recording(*a, **k):
        o = plain(*a, **k)
        outs.append(o.cpu())
        return o

    dp.model_diff.sample = recording
    torch.manual_seed(123)
    p1, p2 = dp.test_hyber(batches=batches, is_train=1)

    Pd, Pp = O.params_to_torch(synthetic_state_dict()), O.params_to_torch(synthetic_state_dict(kind="pose"))
    adj = O.adjacency()
    mask = _ones(17)
    err = metrics.define_error_list(metrics.TEST_ACTIONS)
    torch.manual_seed(123)
    # at eta = 0 the runner draws nothing per step, so its e of batch after batch are consecutive draws (the
    # oracle's loop below would draw its unused z from the same generator in between)
    es = [torch.randn(H * len(b[0]), 17, 5) for b in batches]
    best, mean, frames = 0.0, 0.0, 0
    for (x2d, tgt, acts, sc), got, e in zip(batches, outs, es):
        x2d = torch.from_numpy(x2d)
        xyz = O.gcnpose_forward(Pp, adj, x2d, mask)
        x = O.build_uvxyz(x2d, xyz, H, "quirk")
        xT = x_T(x, e, torch.from_numpy(sc).repeat(H, 1, 1), t_start=50)
        out = O.generalized_steps(xT, mask, SEQ10, lambda a, m, t: O.gcndiff_forward(Pd, adj, a, m, t), _betas())[0][-1]
        assert record_delta(_maxdiff(got, out), TOL, "hypothesis_start/runner/out")
        # the four hypotheses of every frame differ
        hyp = got.reshape(H, -1, 17, 5)
        for i in range(H):
            for j in range(i + 1, H):
                assert float((hyp[i] - hyp[j]).abs().amax(dim=(1, 2)).min()) > 1e-4
        o = O.root_subtract_inplace_quirk(torch.mean(out.reshape(H, -1, 17, 5), 0)[:, :, 2:])
        t = O.root_subtract_inplace_quirk(torch.from_numpy(tgt))
        r1 = M.mpjpe_per_pose(o, t).double().numpy()
        r2 = M.p_mpjpe_per_pose(o.numpy().copy(), t.numpy().copy()).astype(np.float64)
        metrics.test_calculation(r1, r2, acts, err)
        oh = O.root_subtract_inplace_quirk(out[:, :, 2:]).reshape(H, -1, 17, 3)
        per = torch.stack([M.mpjpe_per_pose(oh[i], t).double() for i in range(H)])
        best += float(per.min(0).values.sum())
        mean += float(per.mean(0).sum())
        frames += per.shape[1]
    q1, q2 = metrics.print_error(None, err, 1)
    assert abs(p1 - q1) <= 1e-4 and abs(p2 - q2) <= 1e-4, (p1, q1, p2, q2)
    hl = dp.hypothesis_loss
    assert hl["frames"] == frames == 32
    assert abs(hl["best"][0] - best * 1000.0 / frames) <= 1e-4 and abs(hl["mean"][0] - mean * 1000.0 / frames) <= 1e-4
    assert hl["best"][0] <= hl["mean"][0] and hl["best"][1] <= hl["mean"][1]
    assert hl["best"][0] < hl["mean"][0]
    # the mean-aggregate is what test_hyber returns, not the best of H
    assert abs(p1 - hl["best"][0]) > 1e-6
    # and with the start off nothing of it is computed
    dp2 = runner.Diffpose(runner.default_args(noise="torch-cpu"), cfg, device=dev)
    dp2.model_diff, dp2.model_pose = dp.model_diff, dp.model_pose
    dp.model_diff.sample = plain
    dp2.test_hyber(batches=[b[:3] for b in batches], is_train=1)
    assert dp2.hypothesis_loss is None


@ends_session
def test_hypothesis_errors_is_pose_errors_per_row(dev):
    from diffpose_amd import metrics

    rng = np.random.Generator(np.random.PCG64(3))
    H, F = 3, 9
    out = torch.from_numpy(rng.normal(0, 0.3, size=(H * F, 17, 5)).astype(np.float32)).to(dev)
    tgt = torch.from_numpy(rng.normal(0, 0.3, size=(F, 17, 3)).astype(np.float32)).to(dev)
    h1, h2 = metrics.hypothesis_errors(out, tgt, H, "relative")
    assert h1.shape == h2.shape == (H, F)
    for i in range(H):
        p1, p2 = metrics.pose_errors(out[i * F:(i + 1) * F].contiguous(), tgt, 1, "relative")
        assert torch.equal(h1[i], p1) and torch.equal(h2[i], p2)


# ---------------------------------------------------------------------------------------
# 10. refusals

@ends_session
def test_refusals(dev, models):
    for name in ("h96n4", "perop"):
        m = models(name)
        npts = SHAPES[name][3]
        x, e, scale = _inputs(6, npts, seed=23)
        xd = x.to(dev)
        T = _betas().numel()
        # alpha_bar has T + 1 entries: t_start = T - 1 is the last timestep, T is outside (index_select raises)
        m.sample(xd, SEQ10[:2], _betas(), t_start=T - 1)
        with pytest.raises(DpkError, match="t_start"):
            m.sample(xd, SEQ10[:2], _betas(), t_start=T)
        with pytest.raises(DpkError, match="t_start"):
            m.q_sample(xd, T)
        with pytest.raises(DpkError, match="scale_rows"):
            m.sample(xd, SEQ10[:2], _betas(), t_start=T_START, start_scale=scale[:4].contiguous().to(dev))
        with pytest.raises(DpkError, match="scale_rows"):
            m.q_sample(xd, T_START, start_scale=scale[:5].contiguous().to(dev))
        with pytest.raises(ValueError):
            m.sample(xd, SEQ10[:2], _betas(), t_start=-3)
        with pytest.raises(ValueError):
            m.sample(xd, SEQ10[:2], _betas(), t_start=T_START, start_noise=e[:5].to(dev))
    # no schedule set: DPK_E_INVALID with text
    fresh = HipGCNdiff(adj_mx_from_edges(), None, device=dev)
    try:
        with pytest.raises(DpkError, match="no schedule") as ei:
            fresh.q_sample(torch.zeros(2, 17, 5, device=dev), T_START)
        assert ei.value.code == -1
    finally:
        fresh.close()
