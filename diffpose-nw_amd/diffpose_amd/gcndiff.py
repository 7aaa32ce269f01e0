"""HipGCNdiff — the GCNdiff denoiser as a handle on the HIP library.

Mirrors the reference model's construction and call surface
(``GCNdiff(adj, config)``, ``load_state_dict(states[0])``, ``model(x, mask, t, cemd)``;
reference ``models/gcndiff.py:55-113``, ``runners/diffpose_frame.py:118-132``) so a
caller can swap it in for the DataParallel-wrapped torch module at inference.
All compute runs in libdpk.so on the GPU; torch is used only for device memory
and the current stream.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from .schedule import alpha_bar_table
from .weights import HID, N_HEAD, N_LAYERS, N_PTS, COORDS, normalize_state_dict

# 16 skeleton edges of the runner (runners/diffpose_frame.py:120-124)
H36M_EDGES = ((0, 1), (1, 2), (2, 3), (0, 4), (4, 5), (5, 6), (0, 7), (7, 8), (8, 9), (9, 10),
              (8, 11), (11, 12), (12, 13), (8, 14), (14, 15), (15, 16))


def adj_mx_from_edges(num_pts: int = N_PTS, edges=H36M_EDGES) -> np.ndarray:
    """Row-normalised D^-1 (A_sym + I) as float32 (reference models/GraFormer.py:32-44, sparse=False)."""
    a = np.zeros((num_pts, num_pts), dtype=np.float32)
    for i, j in np.asarray(edges, dtype=np.int64).reshape(-1, 2):
        a[i, j] = 1.0
        a[j, i] = 1.0
    a += np.eye(num_pts, dtype=np.float32)
    inv = np.power(a.sum(1, dtype=np.float32), -1).astype(np.float32)
    inv[np.isinf(inv)] = 0.0
    return (inv[:, None] * a).astype(np.float32)


def _f32p(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _dev_index(device) -> int:
    if device is None:
        return torch.cuda.current_device()
    d = torch.device(device)
    if d.type != "cuda":
        raise ValueError(f"HipGCNdiff runs on a HIP device, got {d}")
    return torch.cuda.current_device() if d.index is None else d.index


def _model_dims(config, default_coords=COORDS):
    if config is None:
        return HID, N_LAYERS, N_HEAD, N_PTS, tuple(default_coords)
    m = getattr(config, "model", config)
    return (int(m.hid_dim), int(m.num_layer), int(m.n_head), int(m.n_pts), tuple(int(c) for c in m.coords_dim))


class _HipModel:
    """A libdpk handle for one model (graph, weights, key mask) on one HIP device."""

    KIND = "diff"
    DEFAULT_COORDS = COORDS

    def __init__(self, adj, config=None, device=None):
        hid, nl, nh, npts, coords = _model_dims(config, self.DEFAULT_COORDS)
        self.device = torch.device("cuda", _dev_index(device))
        L = _lib.lib()
        cfg = _lib.DpkConfig(hid, nl, nh, npts, coords[0], coords[1], self.device.index)
        h = ctypes.c_void_p()
        rc = L.dpk_create(ctypes.byref(cfg), ctypes.byref(h))
        if rc == -2 and self.KIND == "diff" and hid < 4:      # no handle holds the text of a refused create
            raise _lib.DpkError("dpk_create", rc, f"GCNdiff needs hid_dim >= 4, got {hid}: its timestep embedding "
                                                  "divides by hid_dim // 2 - 1 (models/gcndiff.py:15-33)")
        _lib.check(None, "dpk_create", rc)
        self._h = h
        self.n_pts = npts
        self.num_layer = nl
        self.hid_dim = hid
        self.n_head = nh
        self.coords_dim = tuple(coords)
        # config.model.dropout: only a train-mode gradient call reads it (diffusion_loss_grad(dropout=True))
        self.dropout = float(getattr(getattr(config, "model", None), "dropout", 0.0) or 0.0)
        adj = adj.detach().cpu().numpy() if torch.is_tensor(adj) else np.asarray(adj)
        self.adj = np.ascontiguousarray(adj, dtype=np.float32)
        if self.adj.shape != (npts, npts):
            raise ValueError(f"adj must be ({npts},{npts}), got {self.adj.shape}")
        _lib.check(h, "dpk_set_graph", L.dpk_set_graph(h, _f32p(self.adj)))
        self._mask_key = None
        self._mask_ref = None
        self._pose_bits = None       # per-pose key masks (device int32 words), kept alive while bound
        self._mask_hold = []         # per-pose mask arrays a captured graph reads (kept until close)
        self._sched_key = None
        self._trainer = None         # an open DeviceAdam (diffpose_amd/optim.py): the device holds the weights
        self.training = False

    # -- nn.Module-like surface -------------------------------------------------------
    def load_state_dict(self, state_dict, strict: bool = True):
        """Accept the reference's states[0] (with/without 'module.'), torch tensors or numpy."""
        if getattr(self, "_trainer", None) is not None:
            raise RuntimeError("load_state_dict while a DeviceAdam is open on this model: the device holds the weights of "
                               "the run (DeviceAdam.load_params writes them; close() ends the run)")
        sd = normalize_state_dict(state_dict, kind=self.KIND, n_layers=self.num_layer, hid=self.hid_dim,
                                  n_pts=self.n_pts, coords=self.coords_dim)
        names = list(sd.keys())
        arrs = [np.ascontiguousarray(sd[k], dtype=np.float32) for k in names]
        c_names = (ctypes.c_char_p * len(names))(*[k.encode() for k in names])
        c_ptrs = (ctypes.POINTER(ctypes.c_float) * len(arrs))(*[_f32p(a) for a in arrs])
        c_num = (ctypes.c_int64 * len(arrs))(*[a.size for a in arrs])
        L = _lib.lib()
        _lib.check(self._h, "dpk_load_weights", L.dpk_load_weights(self._h, c_names, c_ptrs, c_num, len(arrs)))
        self._state = sd
        return self

    def state_dict(self):
        """name -> tensor of the loaded weights; while a ``DeviceAdam`` is open on the model, the parameters on the
        device (a fresh copy, on the model's device)."""
        from collections import OrderedDict

        tr = getattr(self, "_trainer", None)
        if tr is not None:
            return tr.params_state_dict()
        return OrderedDict((k, torch.from_numpy(np.array(v, dtype=np.float32))) for k, v in self._state.items())

    def _train_sync(self) -> None:
        """Before a sampler-path call: while a ``DeviceAdam`` is open on a persistent-sampler model and a step has run
        since the last sync, ``dpk_train_sync`` (a device-wide wait and a host repack); never under a capture, where the
        call itself then refuses with the reason."""
        tr = getattr(self, "_trainer", None)
        if tr is not None and tr._stale and self.fused and not torch.cuda.is_current_stream_capturing():
            tr.sync()

    def eval(self):
        self.training = False
        return self

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError(f"{type(self).__name__} has no train mode (forward, sample and diffusion_loss "
                                      "run without dropout on the device): take gradient steps with "
                                      "HipGCNdiff.diffusion_loss_grad (dropout= for the reference's train-mode "
                                      "masks) or runner.Diffpose.train_step (SURVEY §8f f4)")
        return self.eval()

    def to(self, *a, **k):
        return self

    def cuda(self, *a, **k):
        return self

    def parameters(self):
        return iter(())

    # -- mask -----------------------------------------------------------------------
    def set_mask(self, mask) -> None:
        """Key mask as the reference's ``masked_fill(mask == 0, -1e9)`` (models/GraFormer.py:107-108):
        one mask for every pose ((1,1,17) as runners/diffpose_frame.py:39-40 builds it, or any 17
        entries), or one per pose ((N,1,17), broadcast over heads and queries like the reference's
        ``mask.unsqueeze(1)``; the next call's batch must then have N poses)."""
        L = _lib.lib()
        if torch.is_tensor(mask) or isinstance(mask, np.ndarray):
            shape = tuple(mask.shape)
            if len(shape) == 3 and shape[0] != 1:
                if shape[1:] != (1, self.n_pts):
                    raise ValueError(f"a per-pose mask must be (N, 1, {self.n_pts}), got {shape}")
                mt = torch.as_tensor(mask).to(self.device)
                words = (mt.reshape(shape[0], self.n_pts) != 0).to(torch.int32)
                shifts = torch.arange(self.n_pts, device=self.device, dtype=torch.int32)
                bits = (words << shifts).sum(dim=1, dtype=torch.int32).contiguous()
                _lib.check(self._h, "dpk_set_pose_masks", L.dpk_set_pose_masks(self._h, bits.data_ptr(), shape[0]))
                self._pose_bits = bits
                return
        if mask is None:
            m = np.ones(self.n_pts, dtype=np.uint8)
        else:
            mt = mask.detach().cpu() if torch.is_tensor(mask) else torch.as_tensor(np.asarray(mask))
            m = mt.reshape(-1).numpy().astype(np.uint8)
            if m.size != self.n_pts:
                raise ValueError(f"mask must have {self.n_pts} key entries, got {m.size}")
        m = np.ascontiguousarray(m)
        _lib.check(self._h, "dpk_set_mask", L.dpk_set_mask(self._h, m.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
        if self._pose_bits is not None:
            _lib.check(self._h, "dpk_set_pose_masks", L.dpk_set_pose_masks(self._h, None, 0))
            self._pose_bits = None

    def _check_mask_batch(self, n: int) -> None:
        """A per-pose mask broadcasts only against a batch of its own size (torch broadcasting)."""
        if self._pose_bits is not None and self._pose_bits.numel() != n:
            raise ValueError(f"per-pose mask has {self._pose_bits.numel()} poses, the batch {n}")

    def _note_mask_use(self) -> None:
        """Before a launch that reads the per-pose mask array by address (dpk_set_pose_masks):
        a captured launch keeps that address for the graph's life, so the array is held until
        close(); an eager launch on another stream than the one that allocated it must not see
        the caching allocator hand the memory out again while it runs (record_stream)."""
        bits = self._pose_bits
        if bits is None:
            return
        if torch.cuda.is_current_stream_capturing():
            if not any(b is bits for b in self._mask_hold):
                self._mask_hold.append(bits)
        else:
            bits.record_stream(torch.cuda.current_stream(self.device))

    def _sync_mask(self, mask) -> None:
        """Upload the key mask when it changed.  Cached by object identity + in-place version;
        the cached object is kept alive so its id cannot be recycled by a new tensor."""
        key = None if mask is None else (id(mask), getattr(mask, "_version", 0))
        if key is None or key != self._mask_key or mask is not self._mask_ref:
            self.set_mask(mask)
            self._mask_key = key
            self._mask_ref = mask

    def _check_x(self, x, channels: int | None = None):
        channels = self.coords_dim[0] if channels is None else channels
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32):
            raise TypeError("x must be a float32 CUDA(HIP) tensor")
        if x.dim() != 3 or x.shape[1] != self.n_pts or x.shape[2] != channels:
            raise ValueError(f"x must be (N, {self.n_pts}, {channels}), got {tuple(x.shape)}")
        if x.device != self.device:
            raise ValueError(f"x on {x.device}, model on {self.device}")
        return x.contiguous()

    GEMM_MODES = {"fp32": 0, "f16x3": 1, "bf16": 2}

    def set_gemm_mode(self, mode: str = "fp32") -> None:
        """Arithmetic of the per-layer GEMMs (see dpk_set_gemm_mode): "fp32" (default, fp32 MFMA)
        "f16x3" (3-term fp16-split MFMA, fp32 accumulate) or "bf16" (bf16 operands, fp32
        accumulate: reduced precision, for the tolerance study).  Not a reference option: the
        reference runs fp32 throughout, and "fp32" is what its parity is pinned on."""
        if mode not in self.GEMM_MODES:
            raise ValueError(f"gemm mode must be one of {sorted(self.GEMM_MODES)}, got {mode!r}")
        _lib.check(self._h, "dpk_set_gemm_mode", _lib.lib().dpk_set_gemm_mode(self._h, self.GEMM_MODES[mode]))
        self.gemm_mode = mode

    def gemm_modes(self) -> int:
        """The GEMM modes this model's calls run (see dpk_gemm_modes): bit m set for mode m of GEMM_MODES,
        so 0b111 at hid 96 / 4 heads on 17 joints, 0b011 at the other persistent-sampler shapes and on padded tiles
        (fewer than 17 joints at any of them), and 0b001 per op."""
        return int(_lib.lib().dpk_gemm_modes(self._h))

    @property
    def fused(self) -> int:
        """1 when a persistent sampler instance serves this model (17 joints, or fewer as padded tiles), 0 when
        its calls run per op (see dpk_fused)."""
        return int(_lib.lib().dpk_fused(self._h))

    TAIL_PLANS = {"four": 0, "two_pose": 1, "step_split": 2}

    def set_tail_plan(self, plan: str = "step_split") -> None:
        """How a partial last round of 4-pose tiles runs (see dpk_set_tail_plan): "step_split"
        (default: its tiles' K steps split over two CUs, bitwise equal to "four"), "two_pose"
        (a round of 2-pose tiles) or "four" (a round of 4-pose tiles).  Scheduling only: the
        reference has no tiles."""
        if plan not in self.TAIL_PLANS:
            raise ValueError(f"tail plan must be one of {sorted(self.TAIL_PLANS)}, got {plan!r}")
        _lib.check(self._h, "dpk_set_tail_plan", _lib.lib().dpk_set_tail_plan(self._h, self.TAIL_PLANS[plan]))

    def set_tile_waves(self, waves: int = 0) -> None:
        """Waves of the workgroup that runs a 4-pose tile of ``sample`` (see dpk_set_tile_waves): 4 (one per
        SIMD), 8 (two per SIMD) or 0 (default: what was measured faster for the GEMM mode).  Scheduling only:
        both instances compute bitwise the same outputs."""
        if waves not in (0, 4, 8):
            raise ValueError(f"tile waves must be 0, 4 or 8, got {waves!r}")
        _lib.check(self._h, "dpk_set_tile_waves", _lib.lib().dpk_set_tile_waves(self._h, int(waves)))

    def debug_split(self, mode: int = 0, read: bool = False):
        """Test hook (dpk_debug_split): set the step-split handoff mode; with ``read``, wait for the
        device and return the number of second halves that recomputed their first half's steps."""
        n = ctypes.c_int(0)
        _lib.check(self._h, "dpk_debug_split",
                   _lib.lib().dpk_debug_split(self._h, int(mode), ctypes.byref(n) if read else None))
        return n.value if read else None

    def debug_resources(self) -> dict:
        """Test hook (dpk_debug_resources): capture-owned resources and free flag slots."""
        buf = (ctypes.c_int * 8)()
        _lib.check(self._h, "dpk_debug_resources", _lib.lib().dpk_debug_resources(self._h, buf, 8))
        keys = ("captures", "tracked", "released", "free_slots", "retired_schedules", "eps_spare_poses",
                "generic_loop_graphs", "generic_spare_kib")
        return dict(zip(keys, list(buf)))

    # bit i of dpk_debug_generic_forms (csrc/dpk_generic.inc, dpkg::GenForm)
    GENERIC_FORMS = ("gemm_narrow", "gemm_sk<4>", "gemm_sk<2>", "gemm<128,vec>", "gemm<128,scalar>", "gemm<64,vec>",
                     "gemm<64,scalar>", "gemm<32,vec>", "gemm<32,scalar>", "attention<TT>", "attention<TF>",
                     "attention<FF>", "graph<T>", "graph<F>", "cheb_basis<T>", "cheb_basis<F>")

    def debug_generic_forms(self) -> set:
        """Test hook (dpk_debug_generic_forms): the names of the per-op kernel forms this model's calls have
        launched (or recorded into a loop graph) since the last read; empty on a persistent-sampler handle."""
        w = ctypes.c_uint(0)
        _lib.check(self._h, "dpk_debug_generic_forms", _lib.lib().dpk_debug_generic_forms(self._h, ctypes.byref(w)))
        return {name for i, name in enumerate(self.GENERIC_FORMS) if (w.value >> i) & 1}

    # bit i of dpk_debug_grad_forms' second word (csrc/dpk_generic_bwd.inc, dpkg::BwdForm)
    GRAD_FORMS = ("dw_partial<vec>", "dw_partial<scalar>", "attention_bwd<T>", "ln_bwd", "graph_t<T>", "graph_t<F>",
                  "cheb_t", "dlg<T>", "temb_bwd", "attention_bwd<F>", "dlg<F>", "attention<train>", "drop_add",
                  "relu_drop")

    def debug_grad_forms(self):
        """Test hook (dpk_debug_grad_forms): (GENERIC_FORMS names of the training forward's and the dX GEMMs'
        launches, GRAD_FORMS names of the backward's own kernels) of the ``diffusion_loss_grad`` calls since the
        last read."""
        a, b = ctypes.c_uint(0), ctypes.c_uint(0)
        _lib.check(self._h, "dpk_debug_grad_forms",
                   _lib.lib().dpk_debug_grad_forms(self._h, ctypes.byref(a), ctypes.byref(b)))
        return ({n for i, n in enumerate(self.GENERIC_FORMS) if (a.value >> i) & 1},
                {n for i, n in enumerate(self.GRAD_FORMS) if (b.value >> i) & 1})

    def debug_sampler_kernels(self) -> set:
        """Test hook (dpk_debug_sampler_kernels): the names (_lib.sampler_kernel_name, e.g.
        dpk8/sample/sparse/bf16/z1/start) of the persistent sampler's kernels this model's calls have launched, or
        recorded into a capture, since the last read; empty on a per-op handle."""
        return set(_lib.sampler_kernels(self._h))

    def profile(self, enable: bool = True) -> None:
        """Bracket each model-kernel launch with HIP events (see dpk_profile)."""
        _lib.check(self._h, "dpk_profile", _lib.lib().dpk_profile(self._h, 1 if enable else 0))

    def kernel_times_ms(self):
        """Wait for and return the recorded kernel durations (ms), oldest first."""
        L = _lib.lib()
        cap = 4096
        buf = (ctypes.c_float * cap)()
        n = ctypes.c_int()
        _lib.check(self._h, "dpk_profile_read", L.dpk_profile_read(self._h, buf, cap, ctypes.byref(n)))
        return [buf[i] for i in range(min(n.value, cap))]

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        tr, self._trainer = getattr(self, "_trainer", None), None
        if tr is not None:
            tr._open = False         # dpk_destroy frees the trainer's arrays
        if h:
            _lib.lib().dpk_destroy(h)
        self._mask_hold = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HipGCNdiff(_HipModel):
    """GCNdiff(adj, config) on MI355X.  ``model(x, mask, t, cemd) -> eps`` like the reference."""

    # -- schedule -------------------------------------------------------------------
    def set_schedule(self, seq, betas, eta: float = 0.0) -> None:
        """Bind seq / betas / eta (cached: re-uploaded only when they change)."""
        b = betas.detach().cpu().numpy() if torch.is_tensor(betas) else np.asarray(betas)
        b = np.ascontiguousarray(b, dtype=np.float32)
        seq = [int(s) for s in seq]
        key = (tuple(seq), b.tobytes(), float(eta))
        if key == self._sched_key:
            return
        abar = np.ascontiguousarray(alpha_bar_table(b))
        cseq = (ctypes.c_int * len(seq))(*seq)
        L = _lib.lib()
        _lib.check(self._h, "dpk_set_schedule",
                   L.dpk_set_schedule(self._h, _f32p(abar), abar.size, cseq, len(seq), ctypes.c_float(eta)))
        self._sched_key = key
        self.K = len(seq)

    # -- compute --------------------------------------------------------------------
    def forward(self, x, mask, t, cemd=0):
        """eps = GCNdiff(x, mask, t) (models/gcndiff.py:101-113); ``cemd`` is unused there too."""
        x = self._check_x(x)
        n = x.shape[0]
        t = torch.as_tensor(t, device=self.device).to(torch.float32).reshape(-1).contiguous()
        if t.numel() == 1 and n != 1:
            t = t.expand(n).contiguous()
        if t.numel() != n:
            raise ValueError(f"t must have {n} entries, got {t.numel()}")
        self._sync_mask(mask)
        self._check_mask_batch(n)
        self._note_mask_use()
        self._train_sync()
        eps = torch.empty_like(x)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        L = _lib.lib()
        _lib.check(self._h, "dpk_eps", L.dpk_eps(self._h, x.data_ptr(), t.data_ptr(), eps.data_ptr(), n, stream))
        return eps

    __call__ = forward

    def _check_start(self, x, t_start, start_scale, start_noise, names=("start_scale", "start_noise")):
        """The hypothesis-start arguments of ``sample`` / ``q_sample`` for the batch x: (t_start, scale,
        scale rows, draws) with the tensors contiguous float32 on x's device, or None for no scale / draws."""
        t_start = int(t_start)
        if t_start < 0:
            raise ValueError(f"t_start must be a timestep >= 0, got {t_start}")
        pose = tuple(x.shape[1:])
        rows = 0
        if start_scale is not None:
            if not (torch.is_tensor(start_scale) and start_scale.dtype == torch.float32 and start_scale.dim() == 3
                    and tuple(start_scale.shape[1:]) == pose and start_scale.device == x.device):
                raise ValueError(f"{names[0]} must be a float32 tensor of shape (S,) + {pose} on {x.device}")
            start_scale = start_scale.contiguous()
            rows = start_scale.shape[0]
        if start_noise is not None:
            if not (torch.is_tensor(start_noise) and start_noise.dtype == torch.float32
                    and start_noise.shape == x.shape and start_noise.device == x.device):
                raise ValueError(f"{names[1]} must be a float32 tensor of shape {tuple(x.shape)} on {x.device}")
            start_noise = start_noise.contiguous()
        return t_start, start_scale, rows, start_noise

    def sample(self, x, seq, betas, eta: float = 0.0, mask=None, seed: int = 0, trajectory: bool = False,
               out=None, noise=None, t_start=None, start_scale=None, start_noise=None):
        """Run the whole DDIM loop on device.  Returns the final x, or (xs, x0s) stacks
        ([K+1,N,17,5], [K,N,17,5]) when ``trajectory`` is set.  ``noise``: None (counter-based
        draws from ``seed`` when eta > 0) or a [K,N,17,5] float32 device tensor whose slice k is the
        z of the k-th executed step (the reference's per-step ``torch.randn_like(x)``,
        common/utils_diff.py:65; see ``utils_diff.draw_noise``).

        ``t_start`` (default None: start from x as given) turns the noised hypothesis start on: the loop
        starts from ``x_T = x * a.sqrt() + (e * start_scale) * (1 - a).sqrt()`` with ``a`` the alpha-bar of
        timestep ``t_start`` (runners/diffpose_frame.py:355-363), computed where the kernel loads x, and
        ``xs[0]`` is x_T.  ``start_scale``: [S,17,5] with S dividing N (pose n reads row n % S: the GMM
        sampler's un-repeated noise_scale serves hypothesis-major rows) or None (ones); ``start_noise``:
        the draws e, [N,17,5], or None (counter-based from ``seed``, independent of batch size)."""
        x = self._check_x(x)
        self.set_schedule(seq, betas, eta)
        start = None if t_start is None else self._check_start(x, t_start, start_scale, start_noise)
        if noise is not None:
            shape = (self.K,) + tuple(x.shape)
            if not (torch.is_tensor(noise) and noise.is_cuda and noise.dtype == torch.float32
                    and tuple(noise.shape) == shape and noise.device == x.device):
                raise ValueError(f"noise must be a float32 tensor of shape {shape} on {x.device}")
            noise = noise.contiguous()
        self._sync_mask(mask)
        n = x.shape[0]
        self._check_mask_batch(n)
        self._note_mask_use()
        self._train_sync()
        out = torch.empty_like(x) if out is None else out
        xs = x0s = None
        if trajectory:
            xs = torch.empty((self.K + 1,) + tuple(x.shape), dtype=x.dtype, device=x.device)
            x0s = torch.empty((self.K,) + tuple(x.shape), dtype=x.dtype, device=x.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        L = _lib.lib()
        xs_p = xs.data_ptr() if xs is not None else None
        x0s_p = x0s.data_ptr() if x0s is not None else None
        seed_c = ctypes.c_uint64(seed & (2**64 - 1))
        if start is not None:
            t0, sc, rows, e = start
            rc = L.dpk_sample_start(self._h, x.data_ptr(), out.data_ptr(), xs_p, x0s_p, n, seed_c,
                                    noise.data_ptr() if noise is not None else None, t0,
                                    sc.data_ptr() if sc is not None else None, rows,
                                    e.data_ptr() if e is not None else None, stream)
        elif noise is None:
            rc = L.dpk_sample(self._h, x.data_ptr(), out.data_ptr(), xs_p, x0s_p, n, seed_c, stream)
        else:
            rc = L.dpk_sample_noise(self._h, x.data_ptr(), out.data_ptr(), xs_p, x0s_p, n, seed_c,
                                    noise.data_ptr(), stream)
        _lib.check(self._h, "dpk_sample", rc)
        if trajectory:
            return xs, x0s
        return out

    def q_sample(self, x, t_start: int, start_scale=None, start_noise=None, seed: int = 0, out=None):
        """The noised hypothesis start alone (dpk_q_sample): ``x * a.sqrt() + (e * start_scale) * (1 - a).sqrt()``
        for the bound schedule's alpha-bar at ``t_start``, arguments as in ``sample``.  For model callables
        whose loop runs on the host (``utils_diff.generalized_steps``)."""
        pose = (self.n_pts, getattr(self, "coords_dim", COORDS)[0])     # a pose of this handle's shape
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3
                and tuple(x.shape[1:]) == pose):
            raise ValueError(f"x must be a float32 CUDA(HIP) tensor of shape (N,) + {pose}")
        x = x.contiguous()
        t0, sc, rows, e = self._check_start(x, t_start, start_scale, start_noise)
        out = torch.empty_like(x) if out is None else out
        stream = torch.cuda.current_stream(x.device).cuda_stream
        rc = _lib.lib().dpk_q_sample(self._h, x.data_ptr(), out.data_ptr(), x.shape[0], t0,
                                     sc.data_ptr() if sc is not None else None, rows,
                                     e.data_ptr() if e is not None else None,
                                     ctypes.c_uint64(seed & (2**64 - 1)), stream)
        _lib.check(self._h, "dpk_q_sample", rc)
        return out

    def _loss_timesteps(self, t, n: int, T: int):
        """``t`` of ``diffusion_loss`` as the [n] float32 device array dpk_diff_loss takes.  Given on the CPU (a
        list, numpy or a CPU tensor) it is checked: integer values in 0..T-1, else ValueError.  A device tensor is
        passed on unchecked (no sync): integer values in that range are the caller's precondition, and the kernel
        clamps the table index, so a bad value reads a wrong row, never outside the table."""
        if torch.is_tensor(t) and t.is_cuda:
            tt = t.to(device=self.device, dtype=torch.float32).reshape(-1)
        else:
            tc = torch.as_tensor(np.asarray(t.detach().numpy() if torch.is_tensor(t) else t)).reshape(-1)
            tf = tc.to(torch.float64)
            if tc.numel() and not bool(((tf == tf.round()) & (tf >= 0) & (tf <= T - 1)).all()):
                raise ValueError(f"t must hold integer timesteps in 0..{T - 1}, got {tc.tolist()}")
            tt = tf.to(torch.float32).to(self.device)
        if tt.numel() == 1 and n != 1:
            tt = tt.expand(n)
        if tt.numel() != n:
            raise ValueError(f"t must have {n} entries, got {tt.numel()}")
        return tt.contiguous()

    def diffusion_loss(self, x0, t, betas, noise_scale=None, noise=None, seed: int = 0, mask=None,
                       return_parts: bool = False):
        """The denoising loss per pose, the forward of the reference's training objective in eval mode
        (runners/diffpose_frame.py:211-226, dropout off): ``x_t = x0 * a.sqrt() + (e * noise_scale) * (1 - a).sqrt()``
        with ``a`` the alpha-bar of each pose's own timestep ``t[n]``, ``eps = model(x_t, mask, t)`` and
        ``loss[n] = (e * noise_scale - eps).square().sum(dim=(1, 2))``, summed in ascending element order in fp32.
        ``loss.mean()`` is the reference's ``loss_diff``.  Returns ``loss [N]``, or ``(loss, x_t, eps)`` with
        ``return_parts``.

        ``t``: [N] integer timesteps in 0..len(betas)-1 (``schedule.training_timesteps`` draws them as the
        reference does); see ``_loss_timesteps`` for the check.  ``noise_scale``: [S,n_pts,5] with S dividing N (pose
        n reads row n % S) or None (ones); ``noise``: the draws e, [N,n_pts,5], or None (counter-based from
        ``seed``, the draws of ``q_sample``).  The bound schedule is kept, whatever its seq, when its betas are
        ``betas``; otherwise ``([0], betas, 0.0)`` is bound.  At a uniform ``t`` the returned x_t is bitwise
        ``q_sample(x0, t)``, and eps is bitwise ``model(x_t, mask, t)``."""
        x0 = self._check_x(x0)
        b = betas.detach().cpu().numpy() if torch.is_tensor(betas) else np.asarray(betas)
        b = np.ascontiguousarray(b, dtype=np.float32)
        if self._sched_key is None or self._sched_key[1] != b.tobytes():
            self.set_schedule([0], b, 0.0)
        n = x0.shape[0]
        tt = self._loss_timesteps(t, n, b.shape[0])
        _t0, sc, rows, e = self._check_start(x0, 0, noise_scale, noise, names=("noise_scale", "noise"))
        self._sync_mask(mask)
        self._check_mask_batch(n)
        self._note_mask_use()
        self._train_sync()
        loss = torch.empty(n, dtype=torch.float32, device=self.device)
        xt = torch.empty_like(x0) if return_parts else None
        eps = torch.empty_like(x0) if return_parts else None
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = _lib.lib().dpk_diff_loss(self._h, x0.data_ptr(), tt.data_ptr(), sc.data_ptr() if sc is not None else None,
                                      rows, e.data_ptr() if e is not None else None,
                                      ctypes.c_uint64(seed & (2**64 - 1)), loss.data_ptr(),
                                      xt.data_ptr() if xt is not None else None,
                                      eps.data_ptr() if eps is not None else None, n, stream)
        _lib.check(self._h, "dpk_diff_loss", rc)
        return (loss, xt, eps) if return_parts else loss

    def param_layout(self):
        """dpk_param_layout as a list of (name, offset, numel) in state_dict order, and the flat array's extent in
        floats (the last entry's offset + numel)."""
        L = _lib.lib()
        out = []
        name, off, num = ctypes.c_char_p(), ctypes.c_int64(), ctypes.c_int64()
        for i in range(int(L.dpk_param_count(self._h))):
            _lib.check(self._h, "dpk_param_layout",
                       L.dpk_param_layout(self._h, i, ctypes.byref(name), ctypes.byref(off), ctypes.byref(num)))
            out.append((name.value.decode(), int(off.value), int(num.value)))
        return out, (out[-1][1] + out[-1][2] if out else 0)

    DROP_SITES = ("attn", "sub0", "sub1", "gc1", "gc2")      # site ids 0..4 of the dropout masks

    def dropout_rates(self, dropout):
        """``diffusion_loss_grad``'s ``dropout`` as (sublayer, attn, gconv): ``True`` is the reference's
        ``(config.model.dropout, 0.1, 0.1)`` (models/gcndiff.py:79-85), a 3-tuple explicit rates"""
        if dropout is True:
            return (float(self.dropout), 0.1, 0.1)
        rates = tuple(float(v) for v in dropout)
        if len(rates) != 3:
            raise ValueError(f"dropout must be None, True or (sublayer, attn, gconv), got {dropout!r}")
        return rates

    def dropout_mask(self, layer: int, site, p: float, seed: int, n: int, first: int = 0):
        """``dpk_dropout_mask``: the uint8 keep mask (1 kept, 0 dropped) of elements ``first .. first + n - 1`` of
        ``(layer, site)`` under ``seed`` at rate ``p``; ``site`` an id 0..4 or a name of ``DROP_SITES``.  Element i is
        the flat index in the site's tensor over the whole batch ([N, heads, J, J] for attn, else [N, J, hid])."""
        site = self.DROP_SITES.index(site) if isinstance(site, str) else int(site)
        keep = torch.empty(int(n), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            rc = _lib.lib().dpk_dropout_mask(ctypes.c_uint64(seed & (2**64 - 1)), int(layer), site, ctypes.c_float(p),
                                             int(first), int(n), keep.data_ptr() if n else None, stream)
        if rc:
            raise _lib.DpkError("dpk_dropout_mask", rc, f"layer {layer} site {site} p {p} first {first} n {n}")
        return keep

    def diffusion_loss_grad(self, x0, t, betas, noise_scale=None, noise=None, seed: int = 0, mask=None, weight=None,
                            dropout=None, dropout_seed: int = 0, pose0: int = 0):
        """``diffusion_loss`` and its gradient: ``(loss [N], grads)`` with ``grads`` an OrderedDict name -> view of one
        flat device tensor (``grads.flat``), every parameter of the state_dict under its name and with the reference's
        shape: d(sum_n weight * loss[n]) / d parameter, what ``loss_diff.backward()`` leaves in ``p.grad``
        (runners/diffpose_frame.py:226-229) for the default ``weight`` = 1 / N.  Eval mode (dropout off), fp32, the
        per-op kernels on every handle; the same arguments give bitwise the same gradients.  Arguments and their
        checks as in ``diffusion_loss``; a rank holding a shard of a batch of B poses passes ``weight=1 / B``.

        ``dropout`` (None: the call above) asks for the train-mode gradient, ``dpk_diff_loss_grad_train``: ``True`` for
        the reference's rates ``(config.model.dropout, 0.1, 0.1)`` or a tuple (sublayer, attn, gconv), with
        counter-based masks under ``dropout_seed`` (include/diffpose_kernels.h has the rule, ``dropout_mask`` the
        masks); ``loss`` is then the train-mode loss.  ``pose0``: the global index of this shard's first pose, so that
        the shards of a batch draw the batch's masks."""
        from collections import OrderedDict

        from .weights import param_shapes

        x0 = self._check_x(x0)
        b = betas.detach().cpu().numpy() if torch.is_tensor(betas) else np.asarray(betas)
        b = np.ascontiguousarray(b, dtype=np.float32)
        if self._sched_key is None or self._sched_key[1] != b.tobytes():
            self.set_schedule([0], b, 0.0)
        n = x0.shape[0]
        tt = self._loss_timesteps(t, n, b.shape[0])
        _t0, sc, rows, e = self._check_start(x0, 0, noise_scale, noise, names=("noise_scale", "noise"))
        self._sync_mask(mask)
        self._check_mask_batch(n)
        self._note_mask_use()
        weight = (1.0 / n if n else 0.0) if weight is None else float(weight)
        layout, total = self.param_layout()
        loss = torch.empty(n, dtype=torch.float32, device=self.device)
        flat = torch.zeros(total, dtype=torch.float32, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        head = (self._h, x0.data_ptr(), tt.data_ptr(), sc.data_ptr() if sc is not None else None, rows,
                e.data_ptr() if e is not None else None, ctypes.c_uint64(seed & (2**64 - 1)), ctypes.c_float(weight))
        tail = (loss.data_ptr(), flat.data_ptr(), n, stream)
        if dropout is None:
            rc = _lib.lib().dpk_diff_loss_grad(*head, *tail)
            _lib.check(self._h, "dpk_diff_loss_grad", rc)
        else:
            rates = _lib.DpkDropout(*self.dropout_rates(dropout))
            rc = _lib.lib().dpk_diff_loss_grad_train(*head, ctypes.byref(rates),
                                                     ctypes.c_uint64(dropout_seed & (2**64 - 1)), int(pose0), *tail)
            _lib.check(self._h, "dpk_diff_loss_grad_train", rc)
        shapes = param_shapes(hid=self.hid_dim, n_layers=self.num_layer, n_pts=self.n_pts, coords=self.coords_dim)

        class _Grads(OrderedDict):
            pass

        grads = _Grads()
        for name, off, num in layout:
            grads[name] = flat[off:off + num].view(shapes[name])
        grads.flat = flat
        return loss, grads

    def device_optimizer(self, config=None, *, lr=None, betas=(0.9, 0.999), eps: float = 1e-8, amsgrad: bool = False,
                         grad_clip=None, ema_rate=None):
        """A ``DeviceAdam`` (diffpose_amd/optim.py) on this model: the parameters move to the device for the run, and
        ``optimizer.step(grads)`` is clip + Adam + EMA + the refresh of the weights in a few launches.  With ``config``
        (the reference's): ``config.optim.{lr, eps, amsgrad, grad_clip}`` (the betas are the reference's
        fixed (0.9, 0.999), common/utils.py:41-43), ``config.model.ema_rate`` when ``config.model.ema`` is set; keyword arguments given
        explicitly win.  RMSProp and SGD stay on the torch path (``runner.Diffpose.train_step`` with a torch
        optimiser)."""
        from .optim import DeviceAdam

        if config is not None:
            o = config.optim
            name = getattr(o, "optimizer", "Adam")
            if name != "Adam":
                raise NotImplementedError(f"config.optim.optimizer = {name!r}: the device-side optimiser is Adam; train "
                                          "with a torch optimiser through runner.Diffpose.train_step(..., params=...)")
            if getattr(o, "weight_decay", 0):
                raise NotImplementedError(f"config.optim.weight_decay = {o.weight_decay}: the device-side Adam has none; "
                                          "use the torch path")
            lr = o.lr if lr is None else lr
            eps = getattr(o, "eps", eps)
            amsgrad = getattr(o, "amsgrad", amsgrad)
            grad_clip = getattr(o, "grad_clip", None) if grad_clip is None else grad_clip
            m = getattr(config, "model", None)
            if ema_rate is None and getattr(m, "ema", False):
                ema_rate = m.ema_rate
        if lr is None:
            raise TypeError("device_optimizer needs lr= (or a config with optim.lr)")
        if getattr(self, "_trainer", None) is not None:
            raise RuntimeError("a DeviceAdam is already open on this model")
        return DeviceAdam(self, lr=lr, betas=betas, eps=eps, amsgrad=amsgrad, grad_clip=grad_clip, ema_rate=ema_rate)

    def ddim_update(self, xt, et, step: int, seed: int = 0, want_x0: bool = True, noise=None):
        """x_{t-1} (and x0) from an external eps for schedule step ``step``; ``noise``: this step's
        draw z (shaped like xt, on its device) or None (counter-based from ``seed``)."""
        xt, et = xt.contiguous(), et.contiguous()
        if noise is not None:
            if not (torch.is_tensor(noise) and noise.dtype == torch.float32 and noise.shape == xt.shape
                    and noise.device == xt.device):
                raise ValueError(f"noise must be a float32 tensor shaped like xt {tuple(xt.shape)} on {xt.device}")
            noise = noise.contiguous()
        xn = torch.empty_like(xt)
        x0 = torch.empty_like(xt) if want_x0 else None
        stream = torch.cuda.current_stream(xt.device).cuda_stream
        L = _lib.lib()
        rc = L.dpk_ddim_update_noise(self._h, xt.data_ptr(), et.data_ptr(), xn.data_ptr(),
                                     x0.data_ptr() if x0 is not None else None, xt.numel(), step,
                                     ctypes.c_uint64(seed & (2**64 - 1)),
                                     noise.data_ptr() if noise is not None else None, stream)
        _lib.check(self._h, "dpk_ddim_update", rc)
        return xn, x0



def GCNdiff(adj, config, device=None) -> HipGCNdiff:   # noqa: N802  (reference constructor name)
    return HipGCNdiff(adj, config, device=device)
