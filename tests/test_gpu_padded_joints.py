"""GPU: GCNdiff on skeletons of 2..16 joints on the persistent sampler, as padded tiles: an n-joint pose rides in
the 17-row pose block of its width's instance (csrc/dpk_sampler.inc, the PAD kernels), the graph terms
zero-embedded by the packer (tests/test_pack_padded_cpu.py), rows and attention keys n..16 dead.

Every comparison is against the CPU oracle (bit-exact on the reference's own 15- and 16-joint fixtures g14,
tests/test_padded_goldens_cpu.py) at the project's 5e-6 bar for eps and trajectories (fp32 sums in another order),
recorded with record_delta; where two paths promise the same bits (the final output and xs[-1], a replayed graph
and the eager call, the hypothesis start and its torch expression, draws keyed by the global element index) the
comparison is bitwise.

Shapes: hid 96 / 4 heads and hid 64 / 2 heads at n = 16 (the dead rows are exactly the tiles' special 17th row), at
n = 15 (they reach into the last 16-row MFMA tile) and at n = 2 (forced with DPK_PAD_MIN_JOINTS=2); hid 128 / 8
heads at n = 16; hid 128 / 4 and hid 64 / 4 once each.  N = 7 on the 4-pose tiles is a full tile and a 3-pose
one, N = 3 on the 2-pose tiles (hid 128) a full tile and a half-empty one.
"""
import ctypes
import functools
import os
from types import SimpleNamespace as ns

import numpy as np
import pytest
import torch

from conftest import record_delta
from diffpose_amd import _lib
from diffpose_amd._lib import DpkError
from diffpose_amd.data import synthetic_batch
from diffpose_amd.gcndiff import HipGCNdiff, adj_mx_from_edges
from diffpose_amd.schedule import alpha_bar_table, make_seq
from diffpose_amd.weights import synthetic_state_dict
from helpers import betas as _betas, maxdiff as _maxdiff

pytestmark = pytest.mark.gpu

TOL = 5e-6
TREE16 = ((0, 1), (1, 2), (2, 3), (0, 4), (4, 5), (5, 6), (0, 7), (7, 8), (8, 9), (9, 10), (8, 11), (11, 12),
          (12, 13), (8, 14), (14, 15))
TREE15 = ((0, 1), (1, 2), (2, 3), (3, 4), (1, 5), (5, 6), (6, 7), (0, 8), (8, 9), (9, 10), (0, 11), (11, 12),
          (12, 13), (1, 14))
RING16 = tuple((i, (i + 1) % 16) for i in range(16)) + ((0, 8), (3, 12))     # no sub-graph of the H36M tree
# name: hid, heads, layers, joints, edges, poses per tile
SHAPES = {
    "h96j16": (96, 4, 2, 16, TREE16, 4),
    "h64j16": (64, 2, 1, 16, RING16, 4),
    "h96j15": (96, 4, 1, 15, TREE15, 4),
    "h64j15": (64, 2, 2, 15, TREE15, 4),
    "h96j2": (96, 4, 1, 2, ((0, 1),), 4),
    "h64j2": (64, 2, 1, 2, ((0, 1),), 4),
    "h128n8j16": (128, 8, 1, 16, TREE16, 2),
    "h128n4j16": (128, 4, 1, 16, TREE16, 2),
    "h64n4j16": (64, 4, 1, 16, TREE16, 4),
}
SEQ10 = make_seq("uniform", 50, 10)
T_START = 30


def ends_session(fn):
    """A library / HIP error is no parity miss: run nothing more on the device."""
    @functools.wraps(fn)
    def run(*a, **k):
        try:
            return fn(*a, **k)
        except DpkError as e:
            if e.code == -3:
                pytest.exit(f"padded_joints/{fn.__name__}: {e}", returncode=3)
            raise
    return run


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _N(name):
    return 7 if SHAPES[name][5] == 4 else 3


def _sd(name, zero_out=False):
    hid, _, layers, npts, _, _ = SHAPES[name]
    sd = dict(synthetic_state_dict(hid=hid, n_layers=layers, n_pts=npts))
    if zero_out:
        for k in ("gconv_output.weight", "gconv_output.bias"):
            sd[k] = np.zeros_like(np.asarray(sd[k]))
    return sd


@pytest.fixture(scope="module")
def models(dev):
    """One handle per (shape, per-op?, zero output layer?) for the whole module.  The environment is read by
    dpk_create alone: DPK_PAD_MIN_JOINTS=2 for the 2-joint shapes, DPK_FORCE_GENERIC=1 for the per-op handles."""
    made = {}

    def get(name, perop=False, zero_out=False):
        key = (name, perop, zero_out)
        if key not in made:
            hid, heads, layers, npts, edges, _ = SHAPES[name]
            cfg = ns(model=ns(hid_dim=hid, emd_dim=hid, coords_dim=[5, 5], num_layer=layers, n_head=heads,
                              dropout=0.25, n_pts=npts))
            env = {"DPK_FORCE_GENERIC": "1"} if perop else ({"DPK_PAD_MIN_JOINTS": "2"} if npts == 2 else {})
            old = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                m = HipGCNdiff(adj_mx_from_edges(npts, edges), cfg, device=dev)
            finally:
                for k, v in old.items():
                    if v is None:
                        del os.environ[k]
                    else:
                        os.environ[k] = v
            made[key] = m
            m.load_state_dict(_sd(name, zero_out))
        return made[key]

    yield get
    for m in made.values():
        m.close()


@functools.lru_cache(maxsize=None)
def _oracle(name):
    from oracle import gcndiff_oracle as O

    _, heads, layers, npts, edges, _ = SHAPES[name]
    P = O.params_to_torch(_sd(name))
    g = torch.from_numpy(adj_mx_from_edges(npts, edges))
    return O, lambda a, mk, t: O.gcndiff_forward(P, g, a, mk, t, n_layers=layers, heads=heads)


def _x(name, n=None, seed=1):
    npts = SHAPES[name][3]
    x = torch.from_numpy(synthetic_batch(_N(name) if n is None else n, seed=seed)[0])
    return x[:, :npts].contiguous()


def _ones(npts, dev=None):
    m = torch.ones(1, 1, npts, dtype=torch.bool)
    return m if dev is None else m.to(dev)


@functools.lru_cache(maxsize=None)
def _ref_traj(name):
    """the oracle's K=10 trajectory at eta 0 from _x(name), computed once and shared (never written to)"""
    O, fwd = _oracle(name)
    npts = SHAPES[name][3]
    xs, x0s = O.generalized_steps(_x(name), _ones(npts), SEQ10, fwd, _betas())
    return torch.stack(xs), torch.stack(x0s)


# ---------------------------------------------------------------------------------------
# 1. a persistent instance serves the handle

@pytest.mark.parametrize("name", list(SHAPES))
@ends_session
def test_fused_flag(dev, models, name):
    m = models(name)
    npts = SHAPES[name][3]
    assert m.fused == 1
    assert m.gemm_modes() == 0b011
    out = m.sample(_x(name).to(dev), SEQ10[:2], _betas(), mask=_ones(npts, dev))
    assert torch.isfinite(out).all()
    assert m.debug_resources()["generic_loop_graphs"] == 0      # the per-op sampler records its K-step loop
    assert m.debug_generic_forms() == set()


@ends_session
def test_per_op_handles_say_so(dev, models):
    m = models("h96j16", perop=True)
    assert m.fused == 0 and m.gemm_modes() == 0b001
    shipped = HipGCNdiff(adj_mx_from_edges(), None, device=dev)
    try:
        assert shipped.fused == 1 and shipped.gemm_modes() == 0b111
    finally:
        shipped.close()


# ---------------------------------------------------------------------------------------
# 2. eps under three masks

@pytest.mark.parametrize("name", list(SHAPES))
@ends_session
def test_eps_vs_oracle_under_masks(dev, models, name):
    """All-ones; a handle-wide mask without keys 0 and n - 1 (at n = 2: no key left); per-pose masks with one pose
    that has no key set and one with a single key.  A row whose keys are all masked is uniform over its n keys in
    the reference (masked_fill(-1e9) is soft): the dead keys n..16 must carry probability exactly 0, not 1/17."""
    _, fwd = _oracle(name)
    m = models(name)
    npts, N = SHAPES[name][3], _N(name)
    x = _x(name, seed=2)
    t = torch.tensor([49.0, 0.0, 12.0, 31.0, 7.0, 49.0, 25.0][:N])
    xd, td = x.to(dev), t.to(dev)
    ones = _ones(npts)
    tag = f"padded_joints/eps/{name}"
    eps = m(xd, ones.to(dev), td, 0)
    assert eps.shape == x.shape
    assert record_delta(_maxdiff(eps, fwd(x, ones, t)), TOL, tag + "/ones")
    mk = ones.clone()
    mk[0, 0, [0, npts - 1]] = False
    assert record_delta(_maxdiff(m(xd, mk.to(dev), td, 0), fwd(x, mk, t)), TOL, tag + "/handle_mask")
    per = torch.ones(N, 1, npts, dtype=torch.bool)
    per[0, 0, :] = False                       # no key set
    per[1, 0, :] = False
    per[1, 0, npts - 1] = True                 # a single key, the last live one
    per[2, 0, 0] = False
    assert record_delta(_maxdiff(m(xd, per.to(dev), td, 0), fwd(x, per, t)), TOL, tag + "/pose_masks")
    m.set_mask(None)


# ---------------------------------------------------------------------------------------
# 3. the K=10 trajectory

@pytest.mark.parametrize("name", list(SHAPES))
@ends_session
def test_trajectory_vs_oracle(dev, models, name):
    m = models(name)
    npts = SHAPES[name][3]
    xd = _x(name).to(dev)
    xs, x0s = m.sample(xd, SEQ10, _betas(), mask=_ones(npts, dev), trajectory=True)
    rxs, rx0s = _ref_traj(name)
    assert torch.equal(xs[0], xd)
    assert record_delta(_maxdiff(xs, rxs), TOL, f"padded_joints/traj/{name}/xs")
    assert record_delta(_maxdiff(x0s, rx0s), TOL, f"padded_joints/traj/{name}/x0s")
    out = m.sample(xd, SEQ10, _betas(), mask=_ones(npts, dev))
    assert torch.equal(out, xs[-1])


# ---------------------------------------------------------------------------------------
# 4. eta = 0.5

@pytest.mark.parametrize("name", ["h96j16", "h64j15", "h96j2", "h128n8j16"])
@ends_session
def test_eta_with_the_callers_draws(dev, models, name):
    O, fwd = _oracle(name)
    m = models(name)
    npts = SHAPES[name][3]
    x = _x(name, seed=3)
    z = torch.randn((len(SEQ10),) + tuple(x.shape), generator=torch.Generator().manual_seed(77))
    xs, x0s = m.sample(x.to(dev), SEQ10, _betas(), eta=0.5, mask=_ones(npts, dev), trajectory=True, noise=z.to(dev))
    rxs, rx0s = O.generalized_steps(x, _ones(npts), SEQ10, fwd, _betas(), eta=0.5, noise=z)
    assert record_delta(_maxdiff(xs, torch.stack(rxs)), TOL, f"padded_joints/eta/{name}/xs")
    assert record_delta(_maxdiff(x0s, torch.stack(rx0s)), TOL, f"padded_joints/eta/{name}/x0s")
    assert _maxdiff(torch.stack(rxs), torch.stack(O.generalized_steps(x, _ones(npts), SEQ10, fwd, _betas())[0])) > 1e-3


@pytest.mark.parametrize("name", ["h96j16", "h64j15", "h128n8j16"])
@ends_session
def test_counter_based_draws_are_the_per_op_handles(dev, models, name):
    """Both paths key a draw by (seed, step, global element index ((pose * n + j) * 5 + c)).  With the output layer
    zero eps is exactly 0 on both, so the trajectories are the draws through the same update arithmetic: bitwise
    (tests/test_gpu_counter_draws.py reads its draws back the same way at 17 joints).  With the real weights the
    two paths agree at the bar, as tests/test_gpu_generic_shapes.py holds the two paths at 17 joints."""
    npts = SHAPES[name][3]
    x = _x(name, seed=4).to(dev)
    kw = dict(eta=0.5, seed=(1 << 33) + 11, mask=_ones(npts, dev), trajectory=True)
    a = models(name, zero_out=True).sample(x, SEQ10[:3], _betas(), **kw)
    b = models(name, perop=True, zero_out=True).sample(x, SEQ10[:3], _betas(), **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0][1], a[0][0])
    a = models(name).sample(x, SEQ10, _betas(), **kw)
    b = models(name, perop=True).sample(x, SEQ10, _betas(), **kw)
    assert record_delta(_maxdiff(a[0], b[0]), TOL, f"padded_joints/counter/{name}/xs")
    assert record_delta(_maxdiff(a[1], b[1]), TOL, f"padded_joints/counter/{name}/x0s")


# ---------------------------------------------------------------------------------------
# 5. the hypothesis start

def _sqrt32(v):
    """sqrtf, correctly rounded (tests/test_gpu_hypothesis_start.py: torch's float32 sqrt is not on every host)"""
    import math
    return torch.tensor(math.sqrt(float(v)), dtype=torch.float32).view(1, 1, 1)


def _x_T(x, e, scale):
    a = torch.from_numpy(alpha_bar_table(_betas().numpy()))[T_START + 1].view(1, 1, 1)
    return x * _sqrt32(a) + (e * scale) * _sqrt32(1.0 - a)


@pytest.mark.parametrize("name", ["h96j16", "h64j15", "h128n8j16"])
@ends_session
def test_hypothesis_start(dev, models, name):
    """N = 6 poses under a scale of S = 3 rows (pose p reads row p % 3) and the caller's e: xs[0] is the torch
    expression bitwise, the trajectory the oracle's from that x_T; without e the draw is dpk_q_sample's."""
    O, fwd = _oracle(name)
    m = models(name)
    npts = SHAPES[name][3]
    x = _x(name, n=6, seed=5)
    g = torch.Generator().manual_seed(1005)
    e = torch.randn(x.shape, generator=g)
    rows = torch.ones(3, npts, 5)
    rows[:, :, :2] = 0.25 + 2.0 * torch.rand((3, npts, 2), generator=g)
    kw = dict(mask=_ones(npts, dev), trajectory=True, t_start=T_START, start_scale=rows.to(dev))
    xs, x0s = m.sample(x.to(dev), SEQ10, _betas(), start_noise=e.to(dev), **kw)
    ref0 = _x_T(x, e, rows.repeat(2, 1, 1))
    assert not torch.equal(ref0, x)
    assert torch.equal(xs[0].cpu(), ref0), _maxdiff(xs[0], ref0)
    rxs, rx0s = O.generalized_steps(ref0, _ones(npts), SEQ10, fwd, _betas())
    assert record_delta(_maxdiff(xs, torch.stack(rxs)), TOL, f"padded_joints/start/{name}/xs")
    assert record_delta(_maxdiff(x0s, torch.stack(rx0s)), TOL, f"padded_joints/start/{name}/x0s")
    cs, _ = m.sample(x.to(dev), SEQ10[:2], _betas(), seed=9, **kw)
    assert torch.equal(cs[0], m.q_sample(x.to(dev), T_START, rows.to(dev), seed=9))
    assert not torch.equal(cs[0], xs[0])


# ---------------------------------------------------------------------------------------
# 6. f16x3

@pytest.mark.parametrize("name", ["h96j16", "h64j16"])
@ends_session
def test_f16x3(dev, models, name):
    _, fwd = _oracle(name)
    m = models(name)
    npts, N = SHAPES[name][3], _N(name)
    x = _x(name)
    t = torch.tensor([49.0, 0.0, 12.0, 31.0, 7.0, 49.0, 25.0][:N])
    m.set_gemm_mode("f16x3")
    try:
        eps = m(x.to(dev), _ones(npts, dev), t.to(dev), 0)
        xs, x0s = m.sample(x.to(dev), SEQ10, _betas(), mask=_ones(npts, dev), trajectory=True)
    finally:
        m.set_gemm_mode("fp32")
    rxs, rx0s = _ref_traj(name)
    assert record_delta(_maxdiff(eps, fwd(x, _ones(npts), t)), TOL, f"padded_joints/f16x3/{name}/eps")
    assert record_delta(_maxdiff(xs, rxs), TOL, f"padded_joints/f16x3/{name}/xs")
    assert record_delta(_maxdiff(x0s, rx0s), TOL, f"padded_joints/f16x3/{name}/x0s")


# ---------------------------------------------------------------------------------------
# 7. what a padded handle refuses

@pytest.mark.parametrize("name", ["h96j16", "h64j15"])
def test_refusals(dev, models, name):
    m = models(name)
    npts = SHAPES[name][3]
    with pytest.raises(DpkError, match=rf"DPK_E_UNSUPPORTED.*{npts} joints") as ei:
        m.set_gemm_mode("bf16")
    assert ei.value.code == -2
    with pytest.raises(DpkError, match=rf"DPK_E_UNSUPPORTED.*{npts} joints") as ei:
        m.set_tile_waves(8)
    assert ei.value.code == -2
    m.set_tile_waves(4)
    m.set_tile_waves(0)
    # both left the handle as it was
    x = _x(name)
    out = m.sample(x.to(dev), SEQ10, _betas(), mask=_ones(npts, dev))
    assert record_delta(_maxdiff(out, _ref_traj(name)[0][-1]), TOL, f"padded_joints/refusals/{name}")


# ---------------------------------------------------------------------------------------
# 8. the reference's own 15- and 16-joint fixtures

@pytest.mark.parametrize("perop", [False, True])
@pytest.mark.parametrize("fixture", ["g14_shape_h96_n4_l2_j16.npz", "g14_shape_h64_n2_l1_j15.npz"])
@ends_session
def test_g14_fixtures(dev, golden, fixture, perop, monkeypatch):
    g = golden(fixture)
    hid, nh, nl, npts = int(g["hid"]), int(g["n_head"]), int(g["num_layer"]), int(g["n_pts"])
    if perop:
        monkeypatch.setenv("DPK_FORCE_GENERIC", "1")
    cfg = ns(model=ns(hid_dim=hid, emd_dim=hid, coords_dim=[5, 5], num_layer=nl, n_head=nh, dropout=0.25, n_pts=npts))
    m = HipGCNdiff(g["adj"], cfg, device=dev)
    try:
        m.load_state_dict(synthetic_state_dict(hid=hid, n_layers=nl, n_pts=npts))
        assert m.fused == (0 if perop else 1)
        x, t = torch.from_numpy(g["x"]).to(dev), torch.from_numpy(g["t8"]).to(dev)
        tag = f"padded_joints/g14/{fixture[10:-4]}/{'perop' if perop else 'padded'}"
        assert record_delta(_maxdiff(m(x, _ones(npts, dev), t, 0), g["eps"]), TOL, tag + "/eps")
        mask2 = torch.from_numpy(g["mask2"]).to(dev)
        assert record_delta(_maxdiff(m(x, mask2, t, 0), g["eps_masked"]), TOL, tag + "/eps_masked")
        xs, x0s = m.sample(x, [int(s) for s in g["seq"]], _betas(int(g["T"])), mask=_ones(npts, dev), trajectory=True)
        assert record_delta(_maxdiff(xs, g["xs"]), TOL, tag + "/xs")
        assert record_delta(_maxdiff(x0s, g["x0s"]), TOL, tag + "/x0s")
    finally:
        m.close()


# ---------------------------------------------------------------------------------------
# 9. graph capture

@ends_session
def test_capture_replays_the_eager_call(dev, models):
    name = "h96j16"
    m = models(name)
    npts = SHAPES[name][3]
    x = _x(name, seed=6)
    other = _x(name, seed=7)
    xd = x.to(dev)
    kw = dict(mask=_ones(npts, dev))
    seq = SEQ10[:4]
    eager = m.sample(xd, seq, _betas(), **kw).clone()
    eager_other = m.sample(other.to(dev), seq, _betas(), **kw).clone()
    assert not torch.equal(eager, eager_other)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):                 # uncaptured warm-up on the capture's side stream
        m.sample(xd, seq, _betas(), **kw)
    torch.cuda.current_stream(dev).wait_stream(s)
    out = torch.empty_like(xd)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        m.sample(xd, seq, _betas(), out=out, **kw)
    for want, src in ((eager, None), (eager_other, other), (eager, x)):
        if src is not None:
            xd.copy_(src.to(dev))
        out.zero_()
        g.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(out, want)
    del g


# ---------------------------------------------------------------------------------------
# 10. nothing beyond the [N][n][5] extents is read or written

@pytest.mark.parametrize("name", ["h96j16", "h64j15", "h96j2", "h128n8j16"])
@ends_session
def test_buffers_inside_nan_guards(dev, models, name):
    """x, out, xs, x0s (and dpk_eps's output) each sit inside a larger buffer pre-filled with NaN, 64 floats of
    guard before and as many floats after as a 17-joint layout of the same batch would overrun.  A read past the
    extents would bring a NaN into the results, a write would replace one: the results are bitwise those of the
    plain call and every guard float is still NaN."""
    m = models(name)
    npts, N = SHAPES[name][3], _N(name)
    K = len(SEQ10)
    x = _x(name, seed=8).to(dev)
    mask = _ones(npts, dev)
    want_xs, want_x0s = m.sample(x, SEQ10, _betas(), mask=mask, trajectory=True)
    t = torch.full((N,), 12.0, device=dev)
    want_eps = m(x, mask, t, 0)
    pre, post = 64, 2 * (K + 1) * N * 17 * 5

    def guarded(numel):
        buf = torch.full((pre + numel + post,), float("nan"), device=dev)
        return buf, buf[pre:pre + numel]

    bx, vx = guarded(N * npts * 5)
    vx.copy_(x.reshape(-1))
    bo, vo = guarded(N * npts * 5)
    bs, vs = guarded((K + 1) * N * npts * 5)
    b0, v0 = guarded(K * N * npts * 5)
    be, ve = guarded(N * npts * 5)
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(m._h, "dpk_sample", L.dpk_sample(m._h, vx.data_ptr(), vo.data_ptr(), vs.data_ptr(), v0.data_ptr(), N,
                                                ctypes.c_uint64(0), stream))
    _lib.check(m._h, "dpk_eps", L.dpk_eps(m._h, vx.data_ptr(), t.data_ptr(), ve.data_ptr(), N, stream))
    torch.cuda.synchronize(dev)
    assert torch.equal(vs.view_as(want_xs), want_xs) and torch.equal(v0.view_as(want_x0s), want_x0s)
    assert torch.equal(vo.view_as(x), want_xs[-1]) and torch.equal(ve.view_as(x), want_eps)
    assert torch.equal(vx.view_as(x), x)
    for buf, view in ((bx, vx), (bo, vo), (bs, vs), (b0, v0), (be, ve)):
        assert bool(torch.isnan(buf[:pre]).all()) and bool(torch.isnan(buf[pre + view.numel():]).all())
