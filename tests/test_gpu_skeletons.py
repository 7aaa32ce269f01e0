"""GPU: skeletons other than 17 joints around the sampler (dpk_pose_metrics_n, dpk_gmm_sample_n,
dpk_gmm_sample_f64_n, and metrics / gmm / runner on top of them).

* at 17 joints the ``_n`` calls give the bits of the 17-joint calls (g7's and g8's inputs);
* the metrics kernel against the reference's own per-frame values at 16 and 21 joints (golden g13) with the
  bars of tests/test_gpu_pose_metrics.py::test_pose_metrics_vs_golden, and against the float64 SVD oracle
  at 2, 3, 4, 16, 21 and 32 joints;
* the GMM sampler against g13 and the oracle's ``gmm_item``, bit for bit;
* ``runner.Diffpose`` end to end on a 16-joint chain and a 21-joint hand against the oracle pipeline.

Bars.  P-MPJPE: 1e-12 m of the float64 oracle (a float64 numpy emulation of the kernel's algorithm, Horn's
quaternion form with a 4x4 Jacobi eigensolver, stays within 2.1e-16 m of it on these inputs) and, from 3
joints up, 1e-7 m of the reference's float32 numpy (whose own rounding is at most 3.5e-8 m there; at 2
joints its float32 SVD is 1.07e-7 m from its float64 self, so only the float64 oracle is used).  MPJPE:
rtol 1e-9 of float64.  xyz: 1e-7 of torch's fp32 hypothesis mean.  End to end: 1e-4 mm, the bar of
test_runner_test_hyber_vs_oracle.
"""
import ctypes
import functools
import math
from types import SimpleNamespace as ns

import numpy as np
import pytest
import torch

from conftest import record_delta
from helpers import betas as _betas, maxdiff as _maxdiff

from diffpose_amd import _lib, metrics
from diffpose_amd._lib import DpkError
from diffpose_amd.gmm import PoseGeneratorGMM, numpy_atol

pytestmark = pytest.mark.gpu

MODES = ["quirk", "relative", "raw"]                 # root_mode 0, 1, 2
CHAIN16 = [(i, i + 1) for i in range(15)]
# a hand: the wrist (joint 0) and five fingers of 4 joints, finger f holding joints 1 + 4 f .. 4 + 4 f
HAND21 = [e for f in range(5) for e in ((0, 1 + 4 * f), (1 + 4 * f, 2 + 4 * f), (2 + 4 * f, 3 + 4 * f),
                                        (3 + 4 * f, 4 + 4 * f))]


def ends_session(fn):
    """A library / HIP error is no parity miss: run nothing more on the device."""
    @functools.wraps(fn)
    def run(*a, **k):
        try:
            return fn(*a, **k)
        except DpkError as e:
            pytest.exit(f"skeletons/{fn.__name__}: {e}", returncode=3)
    return run


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _rc(name, rc):
    _lib.check(None, name, rc)


# ---------------------------------------------------------------------------------------
# 1. n_pts = 17 is the 17-joint call, bit for bit

@ends_session
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_metrics_n_at_17_is_the_old_call_bitwise(dev, golden, H, mode):
    g = golden("g7_metrics.npz")
    F = len(g["pred"]) // H
    out = np.zeros((H * F, 17, 5), np.float32)
    out[:, :, 2:] = g["pred"][:H * F]
    out[:, :, :2] = 7.0                               # uv is not read
    o = torch.from_numpy(out).to(dev)
    t = torch.from_numpy(g["tgt"][:F].copy()).to(dev)
    L = _lib.lib()
    res = []
    for new in (False, True):
        p1 = torch.full((F,), -1.0, dtype=torch.float64, device=dev)
        p2 = torch.full((F,), -1.0, dtype=torch.float64, device=dev)
        xyz = torch.full((F, 17, 3), -1.0, dtype=torch.float32, device=dev)
        tail = (mode, p1.data_ptr(), p2.data_ptr(), xyz.data_ptr(), _stream(dev))
        if new:
            _rc("dpk_pose_metrics_n", L.dpk_pose_metrics_n(o.data_ptr(), t.data_ptr(), F, H, 17, *tail))
        else:
            _rc("dpk_pose_metrics", L.dpk_pose_metrics(o.data_ptr(), t.data_ptr(), F, H, *tail))
        res.append((p1.cpu(), p2.cpu(), xyz.cpu()))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert float(res[0][0].min()) > 0 and float(res[0][1].min()) > 0


@ends_session
@pytest.mark.parametrize("f64", [False, True])
def test_gmm_n_at_17_is_the_old_call_bitwise(dev, golden, f64):
    g = golden("g8_gmm.npz")
    dt = torch.float64 if f64 else torch.float32
    gmm = torch.from_numpy(g["gmm"]).to(dt).to(dev)
    p3 = torch.from_numpy(g["poses_3d"]).to(dt).to(dev)
    idx = torch.from_numpy(g["indices"].astype(np.int64)).to(dev)
    u = torch.from_numpy(g["u"]).to(dev)
    F, n_src, kn = len(g["indices"]), gmm.shape[0], gmm.shape[2]
    L = _lib.lib()
    old, new = (L.dpk_gmm_sample_f64, L.dpk_gmm_sample_f64_n) if f64 else (L.dpk_gmm_sample, L.dpk_gmm_sample_n)
    for u_ptr, seed in ((u.data_ptr(), 0), (None, 99)):
        res = []
        for fn, jn in ((old, ()), (new, (17,))):
            uv = torch.full((F, 17, 5), -1.0, dtype=torch.float32, device=dev)
            sc = torch.full((F, 17, 5), -1.0, dtype=torch.float32, device=dev)
            status = torch.full((1,), 5, dtype=torch.int32, device=dev)
            _rc("dpk_gmm_sample", fn(gmm.data_ptr(), p3.data_ptr(), n_src, *jn, kn, idx.data_ptr(), F, u_ptr, seed,
                                     numpy_atol(np.float32), uv.data_ptr(), sc.data_ptr(), status.data_ptr(),
                                     ctypes.c_void_p(_stream(dev))))
            res.append((uv.cpu(), sc.cpu(), status.cpu()))
        for a, b in zip(*res):
            assert torch.equal(a, b)
        assert int(res[0][2]) == 0
        if u_ptr is not None and not f64:
            assert np.array_equal(res[1][0].numpy(), g["uvxyz"]) and np.array_equal(res[1][1].numpy(), g["noise_scale"])


# ---------------------------------------------------------------------------------------
# 2. the metrics kernel

@ends_session
@pytest.mark.parametrize("J", [16, 21])
def test_pose_metrics_vs_g13(dev, golden, J):
    """tests/test_gpu_pose_metrics.py::test_pose_metrics_vs_golden on the reference's values at J joints"""
    from oracle import metrics_oracle as M

    g = golden(f"g13_metrics_j{J}.npz")
    pred, tgt = g["pred"], g["tgt"]
    out = np.zeros((len(pred), J, 5), np.float32)
    out[:, :, 2:] = pred
    p1, p2, xyz = metrics.pose_errors(torch.from_numpy(out).to(dev), torch.from_numpy(tgt).to(dev), 1, "raw",
                                      return_xyz=True)
    p1, p2 = p1.cpu().numpy(), p2.cpu().numpy()
    assert np.array_equal(xyz.cpu().numpy(), pred)
    assert record_delta(float(np.abs(p2 - g["per_pose_p2"]).max()), 1e-7, f"skeletons/g13/j{J}/p2_vs_reference_f32")
    ref_p1 = np.linalg.norm(pred.astype(np.float64) - tgt.astype(np.float64), axis=-1).mean(-1)
    record_delta(float(np.abs(p1 / ref_p1 - 1).max()), 1e-9, f"skeletons/g13/j{J}/p1_rel")
    assert np.allclose(p1, ref_p1, rtol=1e-9, atol=0)
    ref_p2 = M.p_mpjpe_per_pose(pred.astype(np.float64), tgt.astype(np.float64))
    assert record_delta(float(np.abs(p2 - ref_p2).max()), 1e-12, f"skeletons/g13/j{J}/p2_vs_oracle_f64")


def _hyp_mean(out, H):
    """The kernel's hypothesis mean restated in float32: the sum over h in sequence, then / H"""
    o = out.reshape(H, -1, *out.shape[1:])
    s = np.zeros_like(o[0])
    for h in range(H):
        s = s + o[h]
    assert s.dtype == np.float32
    return s if H == 1 else s / np.float32(H)


def _root(a, mode):
    """test_hyber's root handling on a float32 [F,J,3] array, in float32"""
    a = a.copy()
    if mode == "relative":
        a = a - a[:, :1]
    elif mode == "quirk":
        a[:, 0] = 0.0
    assert a.dtype == np.float32
    return a


@functools.lru_cache(maxsize=None)
def _oracle_case(J, H):
    """Inputs (F = 70: one full 64-thread block and a partial one) and, per root mode, the float64 references"""
    from oracle import metrics_oracle as M

    rng = np.random.Generator(np.random.PCG64(1000 * J + H))
    F = 70
    tgt = rng.normal(0.0, 0.25, size=(F, J, 3))
    tgt[:, 0] = 0.0
    xyz = tgt[None] + rng.normal(0.0, 0.05, size=(H, F, J, 3))
    out = rng.normal(0.0, 0.3, size=(H * F, J, 5)).astype(np.float32)
    out[:, :, 2:] = xyz.reshape(H * F, J, 3).astype(np.float32)
    tgt = tgt.astype(np.float32)
    mean = _hyp_mean(out, H)[:, :, 2:]
    tmean = torch.mean(torch.from_numpy(out).reshape(H, F, J, 5), 0)[:, :, 2:].numpy()
    refs = {}
    for mode in MODES:
        o, t = _root(mean, mode), _root(tgt, mode)
        o64, t64 = o.astype(np.float64), t.astype(np.float64)
        refs[mode] = (o, _root(tmean, mode), np.linalg.norm(o64 - t64, axis=-1).mean(-1),
                      M.p_mpjpe_per_pose(o64.copy(), t64.copy()), M.p_mpjpe_per_pose(o.copy(), t.copy()))
    return out, tgt, refs


@ends_session
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("J", [2, 3, 4, 16, 21, 32])
def test_pose_metrics_vs_fp64_oracle(dev, J, H):
    out, tgt, refs = _oracle_case(J, H)
    od, td = torch.from_numpy(out).to(dev), torch.from_numpy(tgt).to(dev)
    for mode in MODES:
        p1, p2, xyz = metrics.pose_errors(od, td, H, mode, return_xyz=True)
        p1, p2, xyz = p1.cpu().numpy(), p2.cpu().numpy(), xyz.cpu().numpy()
        o, o_torch, r1, r2, r2_f32 = refs[mode]
        tag = f"skeletons/oracle/j{J}/h{H}/{mode}"
        assert p1.shape == p2.shape == (70,) and xyz.shape == (70, J, 3)
        assert np.isfinite(p1).all() and np.isfinite(p2).all()
        assert record_delta(float(np.abs(xyz - o_torch).max()), 1e-7, tag + "/xyz_vs_torch_mean")
        assert record_delta(float(np.abs(xyz - o).max()), 1e-7, tag + "/xyz_vs_sequential_mean")
        assert record_delta(float(np.abs(p2 - r2).max()), 1e-12, tag + "/p2_vs_oracle_f64")
        record_delta(float(np.abs(p1 / r1 - 1).max()), 1e-9, tag + "/p1_rel")
        assert np.allclose(p1, r1, rtol=1e-9, atol=0)
        if J >= 3:
            assert record_delta(float(np.abs(p2 - r2_f32).max()), 1e-7, tag + "/p2_vs_reference_f32")


@ends_session
def test_hypothesis_errors_16_joints_is_pose_errors_per_row(dev):
    out, tgt, _ = _oracle_case(16, 3)
    od, td = torch.from_numpy(out).to(dev), torch.from_numpy(tgt).to(dev)
    h1, h2 = metrics.hypothesis_errors(od, td, 3, "relative")
    assert h1.shape == h2.shape == (3, 70)
    for i in range(3):
        p1, p2 = metrics.pose_errors(od[i * 70:(i + 1) * 70].contiguous(), td, 1, "relative")
        assert torch.equal(h1[i], p1) and torch.equal(h2[i], p2)
    assert not torch.equal(h1[0], h1[1])


def test_pose_errors_shape_refusals(dev):
    """A joint count outside 2..32 or a mismatch raises a ValueError that names both shapes."""
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    for o, t in ((z(4, 1, 5), z(4, 1, 3)), (z(4, 33, 5), z(4, 33, 3)), (z(4, 16, 5), z(4, 17, 3)),
                 (z(4, 17, 5), z(4, 16, 3)), (z(6, 16, 5), z(4, 16, 3))):
        with pytest.raises(ValueError) as ei:
            metrics.pose_errors(o, t)
        assert str(tuple(o.shape)) in str(ei.value) and str(tuple(t.shape)) in str(ei.value)
    e = metrics.pose_errors(z(0, 16, 5), z(0, 16, 3))
    assert e[0].shape == (0,)


# ---------------------------------------------------------------------------------------
# 3. the GMM sampler

def _split(a, lens):
    out, o = [], 0
    for n in lens:
        out.append(a[o:o + n])
        o += n
    return out


@ends_session
@pytest.mark.parametrize("tag", ["", "_f64"])
def test_gmm_vs_g13(dev, golden, tag):
    g = golden("g13_gmm_j16.npz")
    lens = [int(x) for x in g["lens"]]
    acts = [[f"Jog {si}"] * n for si, n in enumerate(lens)]
    cams = _split(np.zeros((sum(lens), 9), np.float32), lens)
    ds = PoseGeneratorGMM(_split(g["poses_3d" + tag], lens), _split(g["gmm" + tag], lens), acts, cams, device=dev)
    assert ds.n_pts == 16 and ds._f64 == bool(tag) and len(ds) == 6

    def check(uv, s, p2, p3):
        assert np.array_equal(uv.cpu().numpy(), g["uvxyz" + tag])
        assert np.array_equal(s.cpu().numpy(), g["noise_scale" + tag])
        assert np.array_equal(p2.cpu().numpy(), g["pose_2d" + tag])
        assert np.array_equal(p3.cpu().numpy(), g["pose_3d" + tag])

    uv, s, p2, p3, a, _ = ds.batch(g["indices"], u=g["u"])
    check(uv, s, p2, p3)
    assert a == [str(x) for x in g["actions"]]
    np.random.seed(1316)                                          # the global numpy stream, per item
    items = [ds[int(i)] for i in g["indices"]]
    check(*(torch.stack([it[k] for it in items]) for k in range(4)))
    with pytest.raises(ValueError, match=r"\(7,16\)"):
        ds.batch(g["indices"], u=np.zeros((7, 17)))


@ends_session
@pytest.mark.parametrize("kn", [1, 5])
@pytest.mark.parametrize("J", [2, 16, 32])
def test_gmm_vs_oracle_item(dev, J, kn):
    from oracle.gmm_oracle import gmm_item

    rng = np.random.Generator(np.random.PCG64(100 * J + kn))
    n_src, idx = 3, [0, 4, -1, 7, 2]                                 # indices that wrap and a negative one
    w = rng.dirichlet(np.ones(kn), size=(n_src, J)).astype(np.float32)
    g = np.concatenate([w[..., None], rng.uniform(-1, 1, size=(n_src, J, kn, 4))], axis=-1).astype(np.float32)
    p3 = rng.normal(0.0, 0.4, size=(n_src, J, 3)).astype(np.float32)
    u = rng.random((len(idx), J))
    ds = PoseGeneratorGMM([p3], [g], [["a", "b", "c"]], [np.zeros((n_src, 1), np.float32)], device=dev)
    uv, s, _, _, acts, _ = ds.batch(idx, u=u)
    assert uv.shape == s.shape == (5, J, 5) and acts == ["a", "b", "c", "b", "c"]
    p3rel = p3 - p3[:, :1]
    for n, i in enumerate(idx):
        ruv, rs = gmm_item(p3rel, g, i, u[n], numpy_atol(np.float32))
        assert np.array_equal(uv[n].cpu().numpy(), ruv), (n, i)
        assert np.array_equal(s[n].cpu().numpy(), rs), (n, i)
    # seeded mode (u = None): repeatable, and another seed gives other draws (kernel_n 1 has one component)
    big = (np.arange(200) % 7) - 3
    a = ds.batch(big, seed=7)[0]
    assert torch.equal(a, ds.batch(big, seed=7)[0])
    assert torch.equal(a, ds.batch(big, seed=8)[0]) == (kn == 1)


@ends_session
def test_gmm_argument_errors_16_joints(dev):
    g = np.zeros((2, 16, 3, 5), np.float32)
    g[..., 0] = [0.5, 0.25, 0.25]
    bad = g.copy()
    bad[1, 15, :, 0] = [0.6, -0.1, 0.5]
    mk = lambda a: PoseGeneratorGMM([np.zeros((2, 16, 3), np.float32)], [a], [["a", "b"]],  # noqa: E731
                                    [np.zeros((2, 1), np.float32)], device=dev)
    ds = mk(bad)
    ds.batch([0])
    with pytest.raises(ValueError, match="non-negative"):
        ds.batch([1])
    bad[1, 15, :, 0] = [0.6, 0.3, 0.2]
    with pytest.raises(ValueError, match="sum to 1"):
        mk(bad).batch([0, 1])
    with pytest.raises(ValueError, match="2..32"):
        mk(np.zeros((2, 33, 3, 5), np.float32))
    with pytest.raises(ValueError, match=r"\(2,16,3\)"):
        PoseGeneratorGMM([np.zeros((2, 17, 3), np.float32)], [g], [["a", "b"]], [np.zeros((2, 1), np.float32)], device=dev)


# ---------------------------------------------------------------------------------------
# 4. the runner, end to end

ACT = ["Walking", "Jog", "Gestures", "Box"]
H, K, T_START = 2, 5, 50


def _config(J, edges):
    from diffpose_amd import runner

    cfg = runner.default_config(test_times=H, test_timesteps=K, test_num_diffusion_timesteps=50, batch_size=12)
    cfg.model = ns(hid_dim=48, emd_dim=48, coords_dim=[5, 5], num_layer=1, n_head=4, dropout=0.25, n_pts=J)
    cfg.data = ns(dataset="other", num_joints=J, edges=edges, actions=ACT)
    return cfg


def _x_T(x, e, scale):
    """runners/diffpose_frame.py:355-363 in float32 on the CPU; the square roots as sqrtf gives them"""
    from diffpose_amd.schedule import alpha_bar_table

    a = float(alpha_bar_table(_betas().numpy())[T_START + 1])
    sa = torch.tensor(math.sqrt(a), dtype=torch.float32)
    sb = torch.tensor(math.sqrt(float(np.float32(1.0) - np.float32(a))), dtype=torch.float32)
    return x * sa + (e * scale) * sb


def _end_to_end(dev, J, edges, noise_start):
    from oracle import gcndiff_oracle as O
    from oracle import metrics_oracle as M
    from diffpose_amd import runner
    from diffpose_amd.data import synthetic_eval_batches
    from diffpose_amd.schedule import make_seq
    from diffpose_amd.weights import synthetic_state_dict

    cfg = _config(J, edges)
    args = runner.default_args(root_mode="relative", noise="torch-cpu", noise_start=noise_start)
    dp = runner.Diffpose(args, cfg, device=dev)
    dp.create_diffusion_model()
    dp.create_pose_model()
    assert dp.model_diff.n_pts == dp.model_pose.n_pts == J
    batches = list(synthetic_eval_batches(24, 12, seed=4300 + J, num_pts=J, actions=ACT))
    if noise_start:
        gen = torch.Generator().manual_seed(8)
        scaled = []
        for x2d, tgt, acts in batches:
            sc = np.ones((len(x2d), J, 5), np.float32)
            sc[:, :, :2] = (0.25 + 2.0 * torch.rand((len(x2d), J, 2), generator=gen)).numpy()
            scaled.append((x2d, tgt, acts, sc))
        batches = scaled
    torch.manual_seed(123)
    p1, p2 = dp.test_hyber(batches=batches, is_train=1)
    hl = dp.hypothesis_loss
    dp.model_diff.close()
    dp.model_pose.close()

    kw = dict(hid=48, n_layers=1, n_pts=J)
    Pd = O.params_to_torch(synthetic_state_dict(**kw))
    Pp = O.params_to_torch(synthetic_state_dict(kind="pose", **kw))
    adj = O.adjacency(J, edges)
    mask = torch.ones(1, 1, J, dtype=torch.bool)
    seq = make_seq("uniform", 50, K)
    err = metrics.define_error_list(ACT)
    torch.manual_seed(123)
    es = [torch.randn(H * len(b[0]), J, 5) for b in batches] if noise_start else [None] * len(batches)
    for b, e in zip(batches, es):
        x2d, tgt, acts = b[:3]
        x2d = torch.from_numpy(x2d)
        xyz = O.gcnpose_forward(Pp, adj, x2d, mask, n_layers=1, heads=4)
        x = O.build_uvxyz(x2d, xyz, H, "relative")
        if noise_start:
            x = _x_T(x, e, torch.from_numpy(b[3]).repeat(H, 1, 1))
        out = O.generalized_steps(x, mask, seq, lambda a, m, t: O.gcndiff_forward(Pd, adj, a, m, t, n_layers=1, heads=4),
                                  _betas())[0][-1]
        o = torch.mean(out.reshape(H, -1, J, 5), 0)[:, :, 2:]
        o, t = o - o[:, :1].clone(), torch.from_numpy(tgt)
        t = t - t[:, :1].clone()
        r1 = M.mpjpe_per_pose(o, t).double().numpy()
        r2 = M.p_mpjpe_per_pose(o.numpy().copy(), t.numpy().copy()).astype(np.float64)
        metrics.test_calculation(r1, r2, acts, err, n_joints=J)
    q1, q2 = metrics.print_error(None, err, 1)
    tag = f"skeletons/runner/j{J}" + ("/noise_start" if noise_start else "")
    ok1 = record_delta(abs(p1 - q1), 1e-4, tag + "/p1_mm")
    ok2 = record_delta(abs(p2 - q2), 1e-4, tag + "/p2_mm")
    assert ok1 and ok2, (p1, q1, p2, q2)
    assert p1 > 1.0 and p2 > 1.0 and list(dp.action_error_sum) == ACT
    return hl


@ends_session
@pytest.mark.parametrize("J,edges", [(16, CHAIN16), (21, HAND21)], ids=["chain16", "hand21"])
def test_runner_other_skeletons_vs_oracle(dev, J, edges):
    assert len(edges) == J - 1 and {j for e in edges for j in e} == set(range(J))        # a tree over all joints
    assert _end_to_end(dev, J, edges, noise_start=False) is None


@ends_session
def test_runner_16_joints_noise_start_vs_oracle(dev):
    hl = _end_to_end(dev, 16, CHAIN16, noise_start=True)
    assert hl["frames"] == 24
    assert hl["best"][0] <= hl["mean"][0] and hl["best"][1] <= hl["mean"][1]


@ends_session
def test_generic_callable_with_start_at_16_joints(dev):
    """utils_diff.generalized_steps with a model callable and the hypothesis start: the schedule-only handle
    behind it takes the joint count of x (it was a 17-joint handle, whose q_sample refused 16-joint poses)."""
    from diffpose_amd.data import synthetic_batch
    from diffpose_amd.gcndiff import HipGCNdiff, adj_mx_from_edges
    from diffpose_amd.schedule import make_seq
    from diffpose_amd.utils_diff import generalized_steps
    from diffpose_amd.weights import synthetic_state_dict

    m = HipGCNdiff(adj_mx_from_edges(16, CHAIN16), _config(16, CHAIN16), device=dev)
    m.load_state_dict(synthetic_state_dict(hid=48, n_layers=1, n_pts=16))
    x = torch.from_numpy(synthetic_batch(9, seed=19, num_pts=16)[0])
    gen = torch.Generator().manual_seed(3)
    e = torch.randn(x.shape, generator=gen)
    scale = torch.ones(x.shape)
    scale[:, :, :2] = 0.25 + 2.0 * torch.rand((9, 16, 2), generator=gen)
    ones = torch.ones(1, 1, 16, dtype=torch.bool, device=dev)
    seq = make_seq("uniform", 50, K)
    kw = dict(t_start=T_START, start_scale=scale.to(dev), start_noise=e.to(dev))
    fxs, fx0s = generalized_steps(x.to(dev), ones, seq, m, _betas(), **kw)
    gxs, gx0s = generalized_steps(x.to(dev), ones, seq, lambda a, mk, t, c: m(a, mk, t, c), _betas(), **kw)
    assert torch.equal(fxs[0].cpu(), _x_T(x, e, scale)) and torch.equal(gxs[0], fxs[0])
    assert record_delta(_maxdiff(torch.stack(gxs), torch.stack(fxs)), 5e-6)
    assert record_delta(_maxdiff(torch.stack(gx0s), torch.stack(fx0s)), 5e-6)
    m.close()
