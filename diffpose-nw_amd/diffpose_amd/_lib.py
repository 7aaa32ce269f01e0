"""ctypes binding of libdpk.so (the C ABI declared in include/diffpose_kernels.h).

The library is built in-tree (``python __graft_entry__.py`` → ``build()``, or
``make -C diffpose-nw_amd``).  There is no fallback: if it is missing or fails to
load, ``lib()`` raises, and every product entry point fails loudly.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DPK_LIB", os.path.join(_HERE, "libdpk.so"))

DPK_OK = 0
ERRORS = {-1: "DPK_E_INVALID", -2: "DPK_E_UNSUPPORTED", -3: "DPK_E_HIP", -4: "DPK_E_STATE", -5: "DPK_E_WEIGHTS"}

# every symbol include/diffpose_kernels.h declares
EXPORTS = ("dpk_version", "dpk_create", "dpk_set_graph", "dpk_load_weights", "dpk_set_mask", "dpk_set_pose_masks",
           "dpk_set_schedule", "dpk_eps", "dpk_sample", "dpk_sample_noise", "dpk_sample_start", "dpk_q_sample", "dpk_diff_loss", "dpk_diff_loss_grad", "dpk_diff_loss_grad_train", "dpk_dropout_mask", "dpk_train_draws",
           "dpk_param_count", "dpk_param_layout", "dpk_train_begin", "dpk_train_apply", "dpk_train_sync", "dpk_train_get",
           "dpk_train_set", "dpk_train_end", "dpk_ddim_update", "dpk_ddim_update_noise",
           "dpk_pose", "dpk_pose_metrics", "dpk_pose_metrics_n", "dpk_gmm_sample", "dpk_gmm_sample_f64", "dpk_gmm_sample_n",
           "dpk_gmm_sample_f64_n", "dpk_set_gemm_mode", "dpk_gemm_modes", "dpk_fused",
           "dpk_set_tail_plan", "dpk_set_tile_waves", "dpk_debug_split", "dpk_debug_resources", "dpk_debug_generic_forms", "dpk_debug_grad_forms", "dpk_debug_sampler_kernels",
           "dpk_profile",
           "dpk_profile_read", "dpk_kernel_geometry", "dpk_last_error", "dpk_destroy")


class DpkConfig(ctypes.Structure):
    _fields_ = [("hid_dim", ctypes.c_int), ("num_layers", ctypes.c_int), ("n_head", ctypes.c_int),
                ("n_pts", ctypes.c_int), ("coords_in", ctypes.c_int), ("coords_out", ctypes.c_int),
                ("device", ctypes.c_int)]


class DpkDropout(ctypes.Structure):
    """dpk_dropout: the rates of a train-mode gradient call (the reference: config.model.dropout, 0.1, 0.1)"""
    _fields_ = [("sublayer", ctypes.c_float), ("attn", ctypes.c_float), ("gconv", ctypes.c_float)]


class DpkOptimConfig(ctypes.Structure):
    """dpk_optim_config: torch.optim.Adam's constants, the clip and the EMA rate of a device-side training run"""
    _fields_ = [("beta1", ctypes.c_float), ("beta2", ctypes.c_float), ("eps", ctypes.c_float), ("amsgrad", ctypes.c_int),
                ("grad_clip", ctypes.c_float), ("ema_mu", ctypes.c_float)]


class DpkError(RuntimeError):
    def __init__(self, fn: str, code: int, msg: str = ""):
        super().__init__(f"{fn} failed: {ERRORS.get(code, code)} {msg}".strip())
        self.code = code


_LIB = None


def lib() -> ctypes.CDLL:
    """Load libdpk.so once.  Imports torch first so the HIP runtime is shared with it."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"libdpk.so not found at {LIB_PATH}: build it with `python __graft_entry__.py` "
                          "(build()) or `make -C diffpose-nw_amd`; there is no CPU fallback")
    import torch  # noqa: F401  (binds libamdhip64.so.7 before our library resolves it)

    L = ctypes.CDLL(LIB_PATH)
    if "DPK_LIB" in os.environ:
        # an A/B build of another version (tools/ab_bench.sh): bind what it exports
        class _Partial:
            def __init__(self, lib):
                self._lib = lib

            def __getattr__(self, name):
                try:
                    return getattr(self._lib, name)
                except AttributeError:
                    return lambda *a: -2          # DPK_E_UNSUPPORTED: not in that build
        L = _Partial(L)
    vp, i32, i64, u64, fp = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_float)
    L.dpk_version.restype = i32
    L.dpk_create.argtypes = [ctypes.POINTER(DpkConfig), ctypes.POINTER(vp)]
    L.dpk_set_graph.argtypes = [vp, fp]
    L.dpk_load_weights.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(fp), ctypes.POINTER(i64), i32]
    L.dpk_set_mask.argtypes = [vp, ctypes.POINTER(ctypes.c_uint8)]
    L.dpk_set_pose_masks.argtypes = [vp, vp, i32]
    L.dpk_set_schedule.argtypes = [vp, fp, i32, ctypes.POINTER(i32), i32, ctypes.c_float]
    L.dpk_eps.argtypes = [vp, vp, vp, vp, i32, vp]
    L.dpk_sample.argtypes = [vp, vp, vp, vp, vp, i32, u64, vp]
    L.dpk_sample_noise.argtypes = [vp, vp, vp, vp, vp, i32, u64, vp, vp]
    L.dpk_sample_start.argtypes = [vp, vp, vp, vp, vp, i32, u64, vp, i32, vp, i32, vp, vp]
    L.dpk_q_sample.argtypes = [vp, vp, vp, i32, i32, vp, i32, vp, u64, vp]
    L.dpk_diff_loss.argtypes = [vp, vp, vp, vp, i32, vp, u64, vp, vp, vp, i32, vp]
    L.dpk_diff_loss_grad.argtypes = [vp, vp, vp, vp, i32, vp, u64, ctypes.c_float, vp, vp, i32, vp]
    L.dpk_diff_loss_grad_train.argtypes = [vp, vp, vp, vp, i32, vp, u64, ctypes.c_float, ctypes.POINTER(DpkDropout), u64, i64,
                                           vp, vp, i32, vp]
    L.dpk_dropout_mask.argtypes = [u64, i32, i32, ctypes.c_float, i64, i64, vp, vp]
    L.dpk_train_draws.argtypes = [u64, u64, i32, i64, i64, i32, i32, vp, vp, vp]
    L.dpk_param_count.argtypes = [vp]
    L.dpk_param_layout.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(i64), ctypes.POINTER(i64)]
    L.dpk_train_begin.argtypes = [vp, ctypes.POINTER(DpkOptimConfig)]
    L.dpk_train_apply.argtypes = [vp, vp, ctypes.c_float, vp, vp]
    L.dpk_train_sync.argtypes = [vp]
    L.dpk_train_get.argtypes = [vp, i32, vp, ctypes.POINTER(i64), vp]
    L.dpk_train_set.argtypes = [vp, i32, vp, i64, vp]
    L.dpk_train_end.argtypes = [vp]
    L.dpk_debug_grad_forms.argtypes = [vp, ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint)]
    L.dpk_ddim_update.argtypes = [vp, vp, vp, vp, vp, i64, i32, u64, vp]
    L.dpk_ddim_update_noise.argtypes = [vp, vp, vp, vp, vp, i64, i32, u64, vp, vp]
    L.dpk_debug_split.argtypes = [vp, i32, ctypes.POINTER(i32)]
    L.dpk_debug_resources.argtypes = [vp, ctypes.POINTER(i32), i32]
    L.dpk_debug_generic_forms.argtypes = [vp, ctypes.POINTER(ctypes.c_uint)]
    L.dpk_debug_sampler_kernels.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32), i32, ctypes.POINTER(i32)]
    L.dpk_pose.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp]
    L.dpk_pose_metrics.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp]
    L.dpk_gmm_sample.argtypes = [vp, vp, i32, i32, vp, i32, vp, u64, ctypes.c_double, vp, vp, vp, vp]
    L.dpk_gmm_sample_f64.argtypes = [vp, vp, i32, i32, vp, i32, vp, u64, ctypes.c_double, vp, vp, vp, vp]
    L.dpk_pose_metrics_n.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]
    L.dpk_gmm_sample_n.argtypes = [vp, vp, i32, i32, i32, vp, i32, vp, u64, ctypes.c_double, vp, vp, vp, vp]
    L.dpk_gmm_sample_f64_n.argtypes = [vp, vp, i32, i32, i32, vp, i32, vp, u64, ctypes.c_double, vp, vp, vp, vp]
    L.dpk_set_gemm_mode.argtypes = [vp, i32]
    L.dpk_gemm_modes.argtypes = [vp]
    L.dpk_fused.argtypes = [vp]
    L.dpk_set_tail_plan.argtypes = [vp, i32]
    L.dpk_set_tile_waves.argtypes = [vp, i32]
    L.dpk_profile.argtypes = [vp, i32]
    L.dpk_profile_read.argtypes = [vp, fp, i32, ctypes.POINTER(i32)]
    L.dpk_kernel_geometry.argtypes = [ctypes.POINTER(i32)] * 3
    L.dpk_last_error.argtypes = [vp]
    L.dpk_last_error.restype = ctypes.c_char_p
    L.dpk_destroy.argtypes = [vp]
    L.dpk_destroy.restype = None
    for name in EXPORTS:
        if name in ("dpk_last_error", "dpk_destroy"):
            continue
        getattr(L, name).restype = i32
    _LIB = L
    return L


def check(handle, fn: str, rc: int) -> None:
    if rc != DPK_OK:
        msg = ""
        if handle:
            raw = lib().dpk_last_error(handle)
            msg = raw.decode() if raw else ""
        raise DpkError(fn, rc, msg)


def kernel_geometry():
    L = lib()
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    L.dpk_kernel_geometry(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    return {"poses_per_workgroup": a.value, "threads_per_workgroup": b.value, "lds_bytes": c.value}


# dpk_debug_sampler_kernels: the fields of a kernel id (include/diffpose_kernels.h)
SAMPLER_TILES = ("dpk", "dpk8", "dpk2", "dpkw", "dpkw4", "dpkn", "dpkn4")
SAMPLER_MODES = ("sample", "eps", "pose")
SAMPLER_GEMMS = ("fp32", "f16x3", "bf16")


def sampler_kernel_id(tile: str, mode: str, sparse: bool, gemm: str, zm: int = 0, start: bool = False,
                      pad: bool = False) -> int:
    """The id word of sample_kernel<mode, sparse, gemm, zm, start, pad> of ``tile``."""
    return (SAMPLER_TILES.index(tile) | SAMPLER_MODES.index(mode) << 4 | int(bool(sparse)) << 6 |
            SAMPLER_GEMMS.index(gemm) << 7 | int(zm) << 9 | int(bool(start)) << 10 | int(bool(pad)) << 11)


def sampler_kernel_name(kid: int) -> str:
    """A kernel id as text: tile/mode/graph/gemm/z<ZM>, then /start and /pad where set, e.g.
    dpk8/sample/sparse/bf16/z1/start."""
    name = "/".join((SAMPLER_TILES[kid & 15], SAMPLER_MODES[kid >> 4 & 3], "sparse" if kid >> 6 & 1 else "dense",
                     SAMPLER_GEMMS[kid >> 7 & 3], f"z{kid >> 9 & 1}"))
    return name + ("/start" if kid >> 10 & 1 else "") + ("/pad" if kid >> 11 & 1 else "")


def sampler_kernels(handle) -> list:
    """dpk_debug_sampler_kernels as names: what ``handle``'s calls launched since the last read, or with None
    every sample_kernel compiled into the library."""
    L = lib()
    n = ctypes.c_int(0)
    check(handle, "dpk_debug_sampler_kernels", L.dpk_debug_sampler_kernels(None, None, 0, ctypes.byref(n)))
    buf = (ctypes.c_uint32 * max(n.value, 1))()       # a handle cannot have launched more than are compiled
    check(handle, "dpk_debug_sampler_kernels", L.dpk_debug_sampler_kernels(handle, buf, len(buf), ctypes.byref(n)))
    return [sampler_kernel_name(buf[i]) for i in range(min(n.value, len(buf)))]


def compiled_sampler_kernels() -> list:
    """The name of every sample_kernel instantiation compiled into the library, in the library's order."""
    return sampler_kernels(None)
