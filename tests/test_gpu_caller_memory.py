"""GPU: the caller-memory contract of include/diffpose_kernels.h on every path: a call touches exactly the
documented extents of each array, needs no more than natural alignment, never writes an input, writes every element
of a non-NULL output, leaves a NULL output's memory alone, and may run in place where the header says so.

Every caller array sits inside a larger buffer filled with a recognisable NaN (tests/caller_memory.py: Guarded, the
checker, the case table; tests/test_caller_memory_cpu.py shows the checker finds each violation).  The calls go
through _lib.lib() with raw pointers, because the Python wrappers allocate their own outputs.  Expected values are
the same call made the ordinary way on the same handle, with torch-allocated tensors through the wrapper (the
other GPU files pin that call to the oracle); dpk_gmm_sample's come from oracle/gmm_oracle.py.

Bars: persistent-sampler handles and the handle-free kernels bitwise in both alignment variants (pre = 64 elements,
or 65: a float pointer 4-byte aligned and no more).  Per-op handles bitwise in the aligned variant; in the
misaligned one the host may pick other kernel forms, and the bar is the project's standing 5e-6 against the plain
call, reported with record_delta (profiles/caller_memory_deltas.jsonl keeps a run).

Every row asserts what it ran: the launch census names (dpk/..., dpk8/..., dpk2/..., dpkw/...) on a persistent
handle, a non-empty set of kernel forms on a per-op one.  CU below is the device's compute-unit count: one 4-pose
tile per CU is a round, so N = 4 CU + 3 is a full round and a 3-pose tail.
"""
import contextlib
import ctypes
import functools
from types import SimpleNamespace as ns

import numpy as np
import pytest
import torch

import caller_memory as CM
import edge_inputs as E
from conftest import record_delta
from diffpose_amd import _lib
from diffpose_amd._lib import DpkError
from diffpose_amd.gcndiff import H36M_EDGES, HipGCNdiff, adj_mx_from_edges
from diffpose_amd.gcnpose import HipGCNpose
from diffpose_amd.gmm import numpy_atol
from diffpose_amd.metrics import pose_errors
from diffpose_amd.weights import synthetic_state_dict
from helpers import betas as _betas

pytestmark = pytest.mark.gpu

DENSE_EDGES = tuple(H36M_EDGES) + ((3, 16), (6, 13))      # outside the compiled Chebyshev pattern
GRAPHS = {"h36m": H36M_EDGES, "dense": DENSE_EDGES, "chain": E.CHAIN16}
ALIGN = pytest.mark.parametrize("mis", [False, True], ids=["aligned", "misaligned"])
# kind of a sampler call -> (eta, the caller's step draws, hypothesis start, xs given, x0s given)
KINDS = {"traj": (0.0, False, False, True, True), "plain": (0.0, False, False, False, False),
         "noise": (CM.ETA_NOISE, True, False, True, True), "start": (0.0, False, True, True, False),
         "start_plain": (0.0, False, True, False, False)}


def ends_session(fn):
    """A library / HIP error is no contract miss: run nothing more on the device."""
    @functools.wraps(fn)
    def run(*a, **k):
        try:
            return fn(*a, **k)
        except DpkError as e:
            if e.code == -3:
                pytest.exit(f"caller_memory/{fn.__name__}: {e}", returncode=3)
            raise
        except RuntimeError as e:                 # torch's own report of a HIP error (at a synchronise, a copy)
            if "HIP error" in str(e):
                pytest.exit(f"caller_memory/{fn.__name__}: {e}", returncode=3)
            raise
    return run


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def default_paths(monkeypatch):
    """the per-op path's recorded loop and kernel choices at their defaults"""
    for k in ("DPK_GEN_GRAPH", "DPK_GEN_GEMM", "DPK_GEN_BM", "DPK_LOSS_FUSED"):
        monkeypatch.delenv(k, raising=False)


def _cfg(hid, heads, layers, joints, coords=(5, 5)):
    return ns(model=ns(hid_dim=hid, emd_dim=hid, coords_dim=list(coords), num_layer=layers, n_head=heads,
                       dropout=0.25, n_pts=joints))


@pytest.fixture(scope="module")
def models(dev):
    """one GCNdiff handle per (shape, graph) of the case table for the whole module"""
    made = {}

    def get(row):
        key = (row.hid, row.heads, row.layers, row.joints, row.graph)
        if key not in made:
            m = HipGCNdiff(adj_mx_from_edges(row.joints, GRAPHS[row.graph]),
                           _cfg(row.hid, row.heads, row.layers, row.joints), device=dev)
            made[key] = m
            m.load_state_dict(synthetic_state_dict(hid=row.hid, n_layers=row.layers, n_pts=row.joints))
        return made[key]

    yield get
    for m in made.values():
        m.close()


def _cu(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


@contextlib.contextmanager
def _knobs(m, row):
    """the row's tail plan, tile waves and gemm mode; the handle's defaults and key mask afterwards"""
    if row.plan:
        m.set_tail_plan(row.plan)
    if row.waves is not None:
        m.set_tile_waves(row.waves)
    m.set_gemm_mode(row.gemm)
    try:
        yield
    finally:
        if row.split_dbg:
            m.debug_split(0)
        if row.plan:
            m.set_tail_plan("step_split")
        if row.waves is not None:
            m.set_tile_waves(0)
        m.set_gemm_mode("fp32")
        m._mask_key = None
        m.set_mask(None)


class Frame:
    """the Guarded arrays of one call"""

    def __init__(self, dev, mis, joints, ch=5):
        self.dev, self.mis, self.tile, self.arrays = dev, mis, 4 * joints * ch, []

    def arr(self, name, shape=None, data=None, role=None, **kw):
        shape = tuple(data.shape) if shape is None else shape
        role = role or ("in" if data is not None else "out")
        kw.setdefault("tile", self.tile)
        return self.add(CM.Guarded(name, shape, device=self.dev, role=role, data=data, misaligned=self.mis, **kw))

    def add(self, g):
        self.arrays.append(g)
        return g

    def check(self, expected, tag, bar=None):
        if bar is not None:
            expected = {k: (v, bar) for k, v in expected.items()}
        CM.check(self.arrays, expected, tag=tag, record=record_delta)
        for g in self.arrays:
            assert g.alignment() == g.itemsize if self.mis else g.alignment() >= 64, (tag, g.name, g.alignment())


def _case(dev, n, joints, k):
    """the device inputs of one (N, K): CM.sampler_inputs, the schedule, the per-pose key masks and their words"""
    c = ns(N=n, J=joints, K=k, seq=CM.SEQS[k], b=_betas(),
           **{key: v.to(dev) for key, v in CM.sampler_inputs(n, joints, k).items()})
    per = CM.pose_masks(n, joints)
    c.mask = torch.from_numpy(per).to(dev)
    c.words = torch.from_numpy(E.pack_pose_bits(per).view(np.int32).copy())
    return c


def _want(m, c, kind, mask):
    """the call made the ordinary way: torch-allocated tensors through the wrapper"""
    if kind == "eps":
        return dict(eps=m(c.x, mask, c.t))
    eta, zm, start, xs, x0s = KINDS[kind]
    kw = dict(eta=eta, mask=mask)
    if zm:
        kw["noise"] = c.z
    if start:
        kw.update(t_start=c.seq[-1], start_scale=c.scale, start_noise=c.e)
    if xs or x0s:
        wxs, wx0s = m.sample(c.x, c.seq, c.b, trajectory=True, **kw)
        return dict(out=wxs[-1].clone(), xs=wxs, x0s=wx0s)
    return dict(out=m.sample(c.x, c.seq, c.b, **kw))


def _raw(m, fr, c, kind, inplace=False):
    """the same call through raw pointers into the frame's guarded arrays; in place: out_dev (eps_dev) == x_dev"""
    L, h, st = _lib.lib(), m._h, _stream(fr.dev)
    N, J, K = c.N, c.J, c.K
    if inplace:
        x = fr.arr("eps" if kind == "eps" else "out", data=c.x, role="inout")
    else:
        x = fr.arr("x", data=c.x)
    if kind == "eps":
        t = fr.arr("t", data=c.t, tile=4)
        eps = x if inplace else fr.arr("eps", c.x.shape)
        _lib.check(h, "dpk_eps", L.dpk_eps(h, x.ptr, t.ptr, eps.ptr, N, st))
        return
    eta, zm, start, xs, x0s = KINDS[kind]
    m.set_schedule(c.seq, c.b, eta)
    out = x if inplace else fr.arr("out", c.x.shape)
    gxs = fr.arr("xs", (K + 1, N, J, 5), slices=K + 1, null=not xs)
    gx0 = fr.arr("x0s", (K, N, J, 5), slices=K, null=not x0s)
    seed = ctypes.c_uint64(0)
    if start:
        sc, e = fr.arr("scale", data=c.scale), fr.arr("start_noise", data=c.e)
        rc = L.dpk_sample_start(h, x.ptr, out.ptr, gxs.ptr, gx0.ptr, N, seed, None, c.seq[-1], sc.ptr,
                                c.scale.shape[0], e.ptr, st)
    elif zm:
        z = fr.arr("noise", data=c.z, slices=K)
        rc = L.dpk_sample_noise(h, x.ptr, out.ptr, gxs.ptr, gx0.ptr, N, seed, z.ptr, st)
    else:
        rc = L.dpk_sample(h, x.ptr, out.ptr, gxs.ptr, gx0.ptr, N, seed, st)
    _lib.check(h, "dpk_sample", rc)


def _names(row, kind):
    """the launch census of the call on the row's handle"""
    mode = "eps" if kind == "eps" else "sample"
    graph = "dense" if row.graph == "dense" else "sparse"
    tail = f"z{1 if kind == 'noise' else 0}" + ("/start" if kind.startswith("start") else "")
    return {f"{t}/{mode}/{graph}/{row.gemm}/{tail}" for t in (row.eps if kind == "eps" else row.sample)}


def _run(m, row, c, kind, fr, tag, inplace=False):
    """one guarded call: the contract, the expected values (in fr's caller), the path it ran"""
    perop = not row.sample
    m.debug_sampler_kernels()
    m.debug_generic_forms()
    if row.split_dbg:
        m.debug_split(row.split_dbg, read=True)           # late first halves from here on; clears the counter
    _raw(m, fr, c, kind, inplace)
    ran, forms = m.debug_sampler_kernels(), m.debug_generic_forms()
    if row.split_dbg:
        fallbacks = m.debug_split(0, read=True)
        assert fallbacks == (0 if kind == "eps" else 2), (tag, fallbacks)    # both split tiles recomputed
    assert ran == _names(row, kind), (tag, ran)
    if perop and kind in ("plain", "start_plain"):
        # the recorded K-step loop: its forms were counted when it was recorded (by this call, or by the wrapper's)
        assert m.debug_resources()["generic_loop_graphs"] >= 1, tag
    else:
        assert bool(forms) == perop, (tag, forms)


# ---------------------------------------------------------------------------------------
# 1. GCNdiff: dpk_eps, dpk_sample, dpk_sample_noise, dpk_sample_start on every row of the table

@ALIGN
@pytest.mark.parametrize("name", list(CM.ROWS))
@ends_session
def test_gcndiff_rows(dev, models, name, mis):
    """Each call of the row with every array guarded, then once more under per-pose key masks whose [N] word array
    sits between guard words all zero, and all ones: a valid pose never reads a neighbour's word, so both match
    the wrapper's call bitwise."""
    row = CM.ROWS[name]
    m = models(row)
    perop = not row.sample
    assert m.fused == (0 if perop else 1)
    N = CM.n_poses(row, _cu(dev))
    bar = CM.PEROP_BAR if perop and mis else None
    L = _lib.lib()
    with _knobs(m, row):
        for K in row.ks:
            c = _case(dev, N, row.joints, K)
            wants = {}
            for guard in (None, 0, -1):
                mask = None if guard is None else c.mask
                if (mask is None) not in wants:
                    m._mask_key = None
                    wants[mask is None] = {kind: _want(m, c, kind, mask) for kind in row.calls}
                want = wants[mask is None]
                if guard is None and not mis and "start" in want:
                    x_T = E.start_xT(c.x.cpu(), c.e.cpu(), c.scale.cpu(), c.seq[-1], c.b)
                    assert torch.equal(want["start"]["xs"][0].cpu(), x_T), name          # xs[0] is x_T
                gm = None
                if guard is not None:
                    gm = CM.Guarded("pose_masks", (N,), dtype=torch.int32, device=dev, role="in", data=c.words,
                                    tile=4, misaligned=mis, pattern=guard)
                    _lib.check(m._h, "dpk_set_pose_masks", L.dpk_set_pose_masks(m._h, gm.ptr, N))
                for kind in row.calls:
                    tag = (f"caller_memory/{name}/{'misaligned' if mis else 'aligned'}/K{K}/"
                           f"{'nomask' if guard is None else 'guard%d' % guard}/{kind}")
                    fr = Frame(dev, mis, row.joints)
                    if gm is not None:
                        fr.add(gm)
                    _run(m, row, c, kind, fr, tag)
                    fr.check(want[kind], tag, bar)


# ---------------------------------------------------------------------------------------
# 2. dpk_q_sample and dpk_ddim_update(_noise)

@ALIGN
@pytest.mark.parametrize("name", CM.UPDATE_ROWS)
@ends_session
def test_q_sample_and_ddim_update(dev, models, name, mis):
    """dpk_q_sample at N = 1 and 7, with and without scale and draws; dpk_ddim_update_noise at eta 0.5 with the
    caller's step draws over 1, 255, 257 and 7 x 85 elements (one thread, a block less one, a block and one, and
    three blocks the last partial), x0_dev given and NULL, at the first and the last step; dpk_ddim_update with the
    counter-based draws."""
    row = CM.ROWS[name]
    m = models(row)
    perop = not row.sample
    bar = CM.PEROP_BAR if perop and mis else None
    L, h, st = _lib.lib(), m._h, _stream(dev)
    K, J = 3, row.joints
    seq, b = CM.SEQS[K], _betas()
    side = "misaligned" if mis else "aligned"
    m.set_schedule(seq, b, 0.0)
    for N in (1, 7):
        c = _case(dev, N, J, K)
        for use_scale in (False, True):
            for use_e in (False, True):
                tag = f"caller_memory/{name}/{side}/q_sample/n{N}/scale{int(use_scale)}/draws{int(use_e)}"
                want = m.q_sample(c.x, seq[-1], c.scale if use_scale else None, c.e if use_e else None, seed=11)
                fr = Frame(dev, mis, J)
                x, xT = fr.arr("x", data=c.x), fr.arr("xT", c.x.shape)
                sc = fr.arr("scale", data=c.scale) if use_scale else None
                e = fr.arr("start_noise", data=c.e) if use_e else None
                rc = L.dpk_q_sample(h, x.ptr, xT.ptr, N, seq[-1], sc.ptr if sc else None, c.scale.shape[0],
                                    e.ptr if e else None, ctypes.c_uint64(11), st)
                _lib.check(h, "dpk_q_sample", rc)
                fr.check(dict(xT=want), tag, bar)
    m.set_schedule(seq, b, CM.ETA_NOISE)
    g = torch.Generator().manual_seed(77)
    for n in CM.DDIM_ELEMS:
        xt, et, z = (torch.randn(n, generator=g).to(dev) for _ in range(3))
        for step in (0, K - 1):
            with_z = m.ddim_update(xt, et, step, noise=z)
            seeded = m.ddim_update(xt, et, step, seed=13)
            for fn, want, give_x0 in (("noise", with_z, True), ("noise", with_z, False), ("seed", seeded, True)):
                tag = f"caller_memory/{name}/{side}/ddim_update/{fn}/n{n}/step{step}/x0{int(give_x0)}"
                fr = Frame(dev, mis, J)
                kw = dict(tile=256)
                gxt, get = fr.arr("xt", data=xt, **kw), fr.arr("eps", data=et, **kw)
                gxn, gx0 = fr.arr("xnext", (n,), **kw), fr.arr("x0", (n,), null=not give_x0, **kw)
                if fn == "noise":
                    gz = fr.arr("noise", data=z, **kw)
                    rc = L.dpk_ddim_update_noise(h, gxt.ptr, get.ptr, gxn.ptr, gx0.ptr, n, step, ctypes.c_uint64(13),
                                                 gz.ptr, st)
                else:
                    rc = L.dpk_ddim_update(h, gxt.ptr, get.ptr, gxn.ptr, gx0.ptr, n, step, ctypes.c_uint64(13), st)
                _lib.check(h, "dpk_ddim_update", rc)
                fr.check(dict(xnext=want[0], x0=want[1]), tag, bar)


# ---------------------------------------------------------------------------------------
# 3. GCNpose: xyz and uvxyz [H,N,J,5]

POSE = {"pose96": ((96, 4, 2, 17, H36M_EDGES), 5, 3, (("four", "dpk"), ("two_pose", "dpk2"))),
        "pose_perop": (E.FORM_POSE_SHAPE, E.FORM_POSE_N, 2, ((None, None),))}


@ALIGN
@pytest.mark.parametrize("name", list(POSE))
@ends_session
def test_gcnpose(dev, name, mis):
    """dpk_pose on the persistent shape (N = 5, H = 3: a full tile and a 1-pose one on the 4-pose tile, three
    2-pose tiles on the tail tile) and per op on 21 joints (N = 7, H = 2), root modes 0..2, with xyz only, uvxyz
    only and both: every one of the H repeats is written, and they are equal."""
    (hid, heads, layers, J, edges), N, H, plans = POSE[name]
    pm = HipGCNpose(adj_mx_from_edges(J, edges), _cfg(hid, heads, layers, J, (2, 3)), device=dev)
    try:
        pm.load_state_dict(synthetic_state_dict(kind="pose", hid=hid, n_layers=layers, n_pts=J))
        perop = name == "pose_perop"
        assert pm.fused == (0 if perop else 1)
        bar = CM.PEROP_BAR if perop and mis else None
        x2d = (0.3 * torch.randn(N, J, 2, generator=torch.Generator().manual_seed(21 + J))).to(dev)
        L, st = _lib.lib(), _stream(dev)
        for plan, tile in plans:
            if plan:
                pm.set_tail_plan(plan)
            for mode in (0, 1, 2):
                wuv, wxyz = pm.uvxyz(x2d, None, H, mode, return_xyz=True)
                for give_xyz, give_uv in ((True, False), (False, True), (True, True)):
                    tag = (f"caller_memory/{name}/{'misaligned' if mis else 'aligned'}/{plan}/root{mode}/"
                           f"xyz{int(give_xyz)}/uvxyz{int(give_uv)}")
                    fr = Frame(dev, mis, J)
                    gx = fr.arr("x2d", data=x2d, tile=4 * J * 2)
                    gxyz = fr.arr("xyz", (N, J, 3), tile=4 * J * 3, null=not give_xyz)
                    guv = fr.arr("uvxyz", (H, N, J, 5), slices=H, null=not give_uv)
                    pm.debug_sampler_kernels()
                    pm.debug_generic_forms()
                    _lib.check(pm._h, "dpk_pose", L.dpk_pose(pm._h, gx.ptr, gxyz.ptr, guv.ptr, N, H, mode, st))
                    ran, forms = pm.debug_sampler_kernels(), pm.debug_generic_forms()
                    fr.check(dict(xyz=wxyz, uvxyz=wuv), tag, bar)
                    assert ran == (set() if perop else {f"{tile}/pose/sparse/fp32/z0"}), (tag, ran)
                    assert bool(forms) == perop, (tag, forms)
                    if give_uv:
                        rep = guv.view().view(torch.int32)
                        assert all(torch.equal(rep[0], rep[hh]) for hh in range(1, H)), tag
    finally:
        pm.close()


# ---------------------------------------------------------------------------------------
# 4. the handle-free kernels

@ALIGN
@pytest.mark.parametrize("joints", [2, 17, 32])
@ends_session
def test_pose_metrics_n(dev, joints, mis):
    """F = 70 frames (a full and a partial 64-thread workgroup), H = 3, p1 / p2 as guarded double arrays, xyz given
    and NULL"""
    F, H, J = 70, 3, joints
    g = torch.Generator().manual_seed(400 + J)
    out = (0.3 * torch.randn(H * F, J, 5, generator=g)).to(dev)
    tgt = (0.3 * torch.randn(F, J, 3, generator=g)).to(dev)
    L, st = _lib.lib(), _stream(dev)
    for mode in (0, 1, 2):
        p1, p2, xyz = pose_errors(out, tgt, H, mode, return_xyz=True)
        for give in (True, False):
            tag = f"caller_memory/metrics/j{J}/{'misaligned' if mis else 'aligned'}/root{mode}/xyz{int(give)}"
            fr = Frame(dev, mis, J)
            go = fr.arr("out_uvxyz", data=out, slices=H, tile=64 * J * 5)
            gt = fr.arr("targets", data=tgt, tile=64 * J * 3)
            g1 = fr.arr("p1", (F,), dtype=torch.float64, tile=64)
            g2 = fr.arr("p2", (F,), dtype=torch.float64, tile=64)
            gx = fr.arr("xyz", (F, J, 3), tile=64 * J * 3, null=not give)
            rc = L.dpk_pose_metrics_n(go.ptr, gt.ptr, F, H, J, mode, g1.ptr, g2.ptr, gx.ptr, st)
            if rc == -3:
                pytest.exit(f"{tag}: DPK_E_HIP", returncode=3)
            _lib.check(None, "dpk_pose_metrics_n", rc)
            fr.check(dict(p1=p1, p2=p2, xyz=xyz), tag)


@functools.lru_cache(maxsize=None)
def _gmm(joints, kernel_n):
    inp = CM.gmm_inputs(joints, kernel_n)
    return inp, {f64: CM.gmm_expected(inp, np.float64 if f64 else np.float32) for f64 in (False, True)}


@pytest.mark.parametrize("kernel_n", CM.GMM_KERNELS)
@pytest.mark.parametrize("joints", CM.GMM_JOINTS)
@ends_session
def test_gmm_sample_n(dev, joints, kernel_n):
    """dpk_gmm_sample_n and dpk_gmm_sample_f64_n, both alignment variants, against oracle/gmm_oracle.py: F = 31
    frames (F x J never a multiple of the 256-thread block), kernel_n up to the documented bound of 64, a guarded
    int64 index that wraps and has negative entries, a guarded u, and the one status int between guard ints."""
    inp, wants = _gmm(joints, kernel_n)
    F, J, S = CM.GMM_F, joints, CM.GMM_SRC
    L, st = _lib.lib(), _stream(dev)
    for f64 in (False, True):
        dt = torch.float64 if f64 else torch.float32
        wuv, wns = (torch.from_numpy(a) for a in wants[f64])
        for mis in (False, True):
            tag = f"caller_memory/gmm/j{J}/k{kernel_n}/{'f64' if f64 else 'f32'}/{'misaligned' if mis else 'aligned'}"
            fr = Frame(dev, mis, J)
            gg = fr.arr("gmm", data=torch.from_numpy(inp["gmm"]), dtype=dt, tile=J * kernel_n * 5)
            gp = fr.arr("poses3d", data=torch.from_numpy(inp["poses3d"]), dtype=dt, tile=J * 3)
            gi = fr.arr("index", data=torch.from_numpy(inp["index"]), dtype=torch.int64, tile=256)
            gu = fr.arr("u", data=torch.from_numpy(inp["u"]), dtype=torch.float64, tile=256)
            guv = fr.arr("uvxyz", (F, J, 5), tile=256 * 5)
            gns = fr.arr("noise_scale", (F, J, 5), tile=256 * 5)
            gs = fr.arr("status", (1,), dtype=torch.int32, tile=0)
            fn = L.dpk_gmm_sample_f64_n if f64 else L.dpk_gmm_sample_n
            rc = fn(gg.ptr, gp.ptr, S, J, kernel_n, gi.ptr, F, gu.ptr, 0, numpy_atol(np.float64 if f64 else np.float32),
                    guv.ptr, gns.ptr, gs.ptr, st)
            if rc == -3:
                pytest.exit(f"{tag}: DPK_E_HIP", returncode=3)
            _lib.check(None, "dpk_gmm_sample_n", rc)
            fr.check(dict(uvxyz=wuv, noise_scale=wns, status=torch.zeros(1, dtype=torch.int32)), tag)


# ---------------------------------------------------------------------------------------
# 5. N = 0: every entry point returns OK and touches nothing

@ends_session
def test_no_poses_touch_nothing(dev, models):
    L, st = _lib.lib(), _stream(dev)
    seed = ctypes.c_uint64(0)
    for name in ("four", "perop48"):
        row = CM.ROWS[name]
        m, J = models(row), row.joints
        m.set_schedule(CM.SEQS[3], _betas(), CM.ETA_NOISE)
        fr = Frame(dev, False, J)
        a = {k: fr.arr(k, shape, role="untouched") for k, shape in
             dict(x=(1, J, 5), t=(1,), out=(1, J, 5), xs=(4, 1, J, 5), x0s=(3, 1, J, 5), noise=(3, 1, J, 5),
                  scale=(1, J, 5), e=(1, J, 5), loss=(1,)).items()}
        p = {k: g.ptr for k, g in a.items()}
        h = m._h
        calls = dict(
            dpk_eps=lambda: L.dpk_eps(h, p["x"], p["t"], p["out"], 0, st),
            dpk_sample=lambda: L.dpk_sample(h, p["x"], p["out"], p["xs"], p["x0s"], 0, seed, st),
            dpk_sample_noise=lambda: L.dpk_sample_noise(h, p["x"], p["out"], p["xs"], p["x0s"], 0, seed, p["noise"], st),
            dpk_sample_start=lambda: L.dpk_sample_start(h, p["x"], p["out"], p["xs"], p["x0s"], 0, seed, p["noise"], 34,
                                                        p["scale"], 1, p["e"], st),
            dpk_q_sample=lambda: L.dpk_q_sample(h, p["x"], p["out"], 0, 34, p["scale"], 1, p["e"], seed, st),
            dpk_diff_loss=lambda: L.dpk_diff_loss(h, p["x"], p["t"], p["scale"], 1, p["e"], seed, p["loss"], p["out"],
                                                  p["xs"], 0, st),
            dpk_ddim_update=lambda: L.dpk_ddim_update(h, p["x"], p["e"], p["out"], p["x0s"], 0, 0, seed, st),
            dpk_ddim_update_noise=lambda: L.dpk_ddim_update_noise(h, p["x"], p["e"], p["out"], p["x0s"], 0, 0, seed,
                                                                  p["noise"], st))
        for fn, call in calls.items():
            _lib.check(h, fn, call())
            fr.check({}, f"caller_memory/{name}/n0/{fn}")
    # dpk_pose, and the handle-free kernels with no frames
    pm = HipGCNpose(adj_mx_from_edges(), _cfg(96, 4, 2, 17, (2, 3)), device=dev)
    try:
        pm.load_state_dict(synthetic_state_dict(kind="pose", hid=96, n_layers=2, n_pts=17))
        fr = Frame(dev, False, 17)
        a = [fr.arr(k, shape, role="untouched") for k, shape in
             dict(x2d=(1, 17, 2), xyz=(1, 17, 3), uvxyz=(2, 1, 17, 5)).items()]
        _lib.check(pm._h, "dpk_pose", L.dpk_pose(pm._h, a[0].ptr, a[1].ptr, a[2].ptr, 0, 2, 1, st))
        fr.check({}, "caller_memory/pose/n0")
    finally:
        pm.close()
    fr = Frame(dev, False, 17)
    f32 = [fr.arr(f"f{i}", (1, 17, 5), role="untouched") for i in range(4)]
    f64 = [fr.arr(f"d{i}", (17,), dtype=torch.float64, role="untouched") for i in range(3)]
    idx = fr.arr("index", (1,), dtype=torch.int64, role="untouched")
    status = fr.arr("status", (1,), dtype=torch.int32, role="untouched")
    rcs = [L.dpk_pose_metrics_n(f32[0].ptr, f32[1].ptr, 0, 2, 17, 1, f64[0].ptr, f64[1].ptr, f32[2].ptr, st),
           L.dpk_gmm_sample_n(f32[0].ptr, f32[1].ptr, 9, 17, 5, idx.ptr, 0, f64[0].ptr, 0, 3.4526698e-4, f32[2].ptr,
                              f32[3].ptr, status.ptr, st),
           L.dpk_gmm_sample_f64_n(f64[1].ptr, f64[2].ptr, 9, 17, 5, idx.ptr, 0, f64[0].ptr, 0, 1.5e-8, f32[2].ptr,
                                  f32[3].ptr, status.ptr, st),
           # the 17-joint names of the same three
           L.dpk_pose_metrics(f32[0].ptr, f32[1].ptr, 0, 2, 1, f64[0].ptr, f64[1].ptr, f32[2].ptr, st),
           L.dpk_gmm_sample(f32[0].ptr, f32[1].ptr, 9, 5, idx.ptr, 0, f64[0].ptr, 0, 3.4526698e-4, f32[2].ptr,
                            f32[3].ptr, status.ptr, st),
           L.dpk_gmm_sample_f64(f64[1].ptr, f64[2].ptr, 9, 5, idx.ptr, 0, f64[0].ptr, 0, 1.5e-8, f32[2].ptr,
                                f32[3].ptr, status.ptr, st)]
    assert rcs == [0] * 6, rcs
    fr.check({}, "caller_memory/handle_free/n0")


# ---------------------------------------------------------------------------------------
# 6. in place: x = sample(x), x = eps(x), x = q_sample(x), x = update(x)

@pytest.mark.parametrize("name", CM.INPLACE_ROWS)
@ends_session
def test_in_place(dev, models, name):
    """xT_dev == x_dev in dpk_q_sample, out_dev == x_dev in dpk_sample and dpk_sample_start (xs / x0s given and
    NULL), eps_dev == x_dev in dpk_eps and xnext_dev == xt_dev in dpk_ddim_update_noise, aligned, guarded: each is
    bitwise the out-of-place call.  A tile loads its poses before it stores them; the halves of a step-split tile
    are serialised by their claim / publish words (and on the recompute path the late first half never writes); the
    per-op forward reads x in its first kernel only."""
    row = CM.ROWS[name]
    m = models(row)
    N, J = CM.n_poses(row, _cu(dev)), row.joints
    L, h, st = _lib.lib(), m._h, _stream(dev)
    with _knobs(m, row):
        for K in row.ks:
            c = _case(dev, N, J, K)
            base = f"caller_memory/{name}/in_place/K{K}"
            m.set_schedule(c.seq, c.b, 0.0)
            want = m.q_sample(c.x, c.seq[-1], c.scale, c.e)
            fr = Frame(dev, False, J)
            io = fr.arr("xT", data=c.x, role="inout")
            sc, e = fr.arr("scale", data=c.scale), fr.arr("start_noise", data=c.e)
            rc = L.dpk_q_sample(h, io.ptr, io.ptr, N, c.seq[-1], sc.ptr, c.scale.shape[0], e.ptr, ctypes.c_uint64(0), st)
            _lib.check(h, "dpk_q_sample", rc)
            fr.check(dict(xT=want), base + "/q_sample")
            for kind in ("eps", "traj", "plain", "start", "start_plain"):
                m._mask_key = None
                want = _want(m, c, kind, None)
                fr = Frame(dev, False, J)
                _run(m, row, c, kind, fr, f"{base}/{kind}", inplace=True)
                fr.check(want, f"{base}/{kind}")
            m.set_schedule(c.seq, c.b, CM.ETA_NOISE)
            xt, et, z = c.x.reshape(-1), c.e.reshape(-1), c.z[0].reshape(-1)
            for step in (0, K - 1):
                wn, w0 = m.ddim_update(xt, et, step, noise=z)
                fr = Frame(dev, False, J)
                kw = dict(tile=256)
                io = fr.arr("xnext", data=xt, role="inout", **kw)
                get, gz, gx0 = fr.arr("eps", data=et, **kw), fr.arr("noise", data=z, **kw), fr.arr("x0", xt.shape, **kw)
                rc = L.dpk_ddim_update_noise(h, io.ptr, get.ptr, io.ptr, gx0.ptr, xt.numel(), step, ctypes.c_uint64(0),
                                             gz.ptr, st)
                _lib.check(h, "dpk_ddim_update_noise", rc)
                fr.check(dict(xnext=wn, x0=w0), f"{base}/ddim_update/step{step}")
