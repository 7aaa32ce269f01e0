"""Shared rules, shapes and stand-ins of the training-run tests (tests/test_train_run_cpu.py and
tests/test_train_run_gloo.py on the CPU, tests/test_gpu_train_draws.py and tests/test_gpu_train_run.py on the GPU).
Everything comes from fixed seeds; nothing here touches a GPU.

1. The draw rules of dpk_train_draws (include/diffpose_kernels.h), restated in numpy on tests/counter_draws.py:
   ``t_rule`` (integers only, compared exactly) and ``e_ref`` (counter_draws.normal_ref at step -1 and the global
   element index, held to counter_draws.draw_bar(r, 0): the kernel stores the draw itself, nothing is recovered).
2. The run of the tests: a synthetic resident dataset of 23 frames with kernel_n = 3, batches of 8 (an epoch is
   8 + 8 + 7), 3 epochs with decay = 2, evaluation on 6 frames with test_timesteps = 2 and test_times = 1.
3. Stand-ins for the CPU tests of ``runner.Diffpose.train``: ``StubAdam`` (the DeviceAdam methods the run uses, on flat
   CPU tensors in a restated layout), ``StubData`` and ``stub_step_grads`` (a gradient and a loss that depend on the
   global frame index alone, small integers in float32, so every sum is exact in any order).
"""
from __future__ import annotations

from types import SimpleNamespace as ns

import numpy as np
import torch

import counter_draws as C

FRAMES, KERNEL_N, BATCH, EPOCHS, DECAY = 23, 3, 8, 3, 2
LR, GAMMA, MU = 1e-3, 0.9, 0.999
EVAL_FRAMES = 6
STEPS_PER_EPOCH = 3                                  # 8 + 8 + 7
RUN_SEED = 19960903
T_EDGES = ((1, 5), (2, 2), (51, 1), (51, 37))         # (T, batch)


# ---------------------------------------------------------------------------------------
# 1. the draw rules

def t_rule(t_seed, T: int, batch: int, pose0: int = 0, n=None) -> np.ndarray:
    """t of poses pose0 .. pose0 + n - 1 of a batch of ``batch``: int64, integer arithmetic only"""
    n = batch - pose0 if n is None else n
    p = np.arange(pose0, pose0 + n, dtype=np.int64)
    h = batch // 2 + 1
    first = p < h
    q = np.where(first, p, p - h)
    assert np.all(q < h) and np.all(q >= 0)
    w = C.counter_word(t_seed, q)
    r = (((w >> np.uint64(32)) * np.uint64(T)) >> np.uint64(32)).astype(np.int64)
    return np.where(first, r, T - 1 - r)


def e_ref(e_seed, pose0: int, n: int, pose_floats: int):
    """(z, r) float64 [n * pose_floats]: normal_ref(e_seed, -1, global element index) and the draws' radii"""
    idx = np.arange(n * pose_floats, dtype=np.uint64) + np.uint64(pose0 * pose_floats)
    return C.normal_ref(e_seed, -1, idx)


# ---------------------------------------------------------------------------------------
# 2. the run

def dataset_arrays(joints: int = 17, dtype=np.float32, frames: int = FRAMES, seed: int = 31):
    """PoseGenerator_gmm's constructor arguments for two sequences of ``frames`` frames in all: poses_3d [F,J,3],
    poses_2d_gmm [F,J,kernel_n,5] = (weight, mu_u, mu_v, var_u, var_v) with Dirichlet weights, actions, camerapara"""
    rng = np.random.Generator(np.random.PCG64(seed + joints))
    w = rng.dirichlet(np.ones(KERNEL_N), size=(frames, joints))
    mu = rng.normal(0.0, 0.3, size=(frames, joints, KERNEL_N, 2))
    var = rng.uniform(0.25, 2.25, size=(frames, joints, KERNEL_N, 2))
    gmm = np.concatenate([w[..., None], mu, var], axis=-1).astype(dtype)
    if dtype == np.float32:                                          # float32 weights that still sum to 1 within atol
        assert np.abs(gmm[..., 0].astype(np.float64).sum(-1) - 1).max() < 1e-6
    p3 = rng.normal(0.0, 0.25, size=(frames, joints, 3)).astype(dtype)
    cam = rng.normal(size=(frames, 9)).astype(np.float32)
    cut = frames // 2
    acts = [["Walking 1"] * cut, ["Eating 1"] * (frames - cut)]
    return [p3[:cut], p3[cut:]], [gmm[:cut], gmm[cut:]], acts, [cam[:cut], cam[cut:]]


def run_config(shape, ema: bool = True, dropout: float = 0.25, n_epochs: int = EPOCHS):
    """The config of the tests' run for a model ``shape`` = (hid, heads, layers, joints, edges)"""
    hid, heads, layers, joints, edges = shape[:5]
    return ns(model=ns(hid_dim=hid, emd_dim=hid, coords_dim=[5, 5], num_layer=layers, n_head=heads, dropout=dropout,
                       n_pts=joints, ema=ema, ema_rate=MU),
              diffusion=ns(beta_schedule="linear", beta_start=0.0001, beta_end=0.001, num_diffusion_timesteps=51),
              training=ns(batch_size=BATCH, num_workers=0, n_epochs=n_epochs),
              testing=ns(test_times=1, test_timesteps=2, test_num_diffusion_timesteps=50),
              optim=ns(optimizer="Adam", lr=LR, eps=1e-8, amsgrad=False, grad_clip=1.0, decay=DECAY, lr_gamma=GAMMA,
                       weight_decay=0.0),
              data=ns(dataset="human36m", num_joints=joints, edges=edges))


def lr_after(epoch: int) -> float:
    """the learning rate in force after ``epoch`` (common/utils.py:26-30 at every epoch % decay == 0)"""
    last = epoch - epoch % DECAY
    return LR * GAMMA ** (last / DECAY)


def eval_batches(joints: int = 17):
    from diffpose_amd.data import synthetic_eval_batches

    other = {} if joints == 17 else {"num_pts": joints}
    return list(synthetic_eval_batches(EVAL_FRAMES, BATCH, seed=5, **other))


# ---------------------------------------------------------------------------------------
# 3. stand-ins (CPU)

def stub_layout():
    """(layout, F, shapes) of the h96 shape (hid 96, 2 layers: weights.load_checkpoint's hid), dpk_param_layout
    restated (tests/optim_cases.py)"""
    import optim_cases as OC

    return OC.layout_of("h96")


class StubAdam:
    """The methods of DeviceAdam that ``train`` uses, on flat CPU float32 tensors.  The step is not Adam: it is a
    deterministic rule in which every array matters (exp_avg carries momentum, exp_avg_sq accumulates), so a resume
    that drops one of them shows."""

    def __init__(self, lr: float = LR, ema: bool = True):
        from diffpose_amd import optim as OP

        self.OP = OP
        self.layout, self.total, self.shapes = stub_layout()
        self.param_groups = [{"lr": float(lr), "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0, "amsgrad": False}]
        self.params = torch.zeros(self.total)
        for k, off, n in self.layout:
            self.params[off:off + n] = 1.0
        self.exp_avg, self.exp_avg_sq = torch.zeros(self.total), torch.zeros(self.total)
        self.ema = self.params.clone() if ema else None
        self.step_count = 0
        self.lrs = []

    def step(self, flat):
        lr = float(self.param_groups[0]["lr"])
        self.lrs.append(lr)
        self.step_count += 1
        self.exp_avg = 0.5 * self.exp_avg + flat
        self.exp_avg_sq = self.exp_avg_sq + flat * flat
        self.params = self.params - lr * self.exp_avg
        if self.ema is not None:
            self.ema = (1.0 - MU) * self.params + MU * self.ema

    def params_state_dict(self):
        return self.OP.split_flat(self.params.clone(), self.layout, self.shapes)

    def load_params(self, sd):
        sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
        self.params = self.OP.join_flat(sd, self.layout, self.total)

    def state_dict(self):
        arrays = {"exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone()}
        return self.OP.adam_state_dict(self.layout, self.shapes, self.step_count, arrays, self.param_groups[0]["lr"],
                                       (0.9, 0.999), 1e-8, False)

    def load_state_dict(self, sd):
        step, arrays, group = self.OP.adam_arrays(sd, self.layout, self.total, False)
        self.step_count, self.exp_avg, self.exp_avg_sq = step, arrays["exp_avg"], arrays["exp_avg_sq"]
        self.param_groups[0]["lr"] = float(group["lr"])

    def ema_state_dict(self):
        return self.OP.split_flat(self.ema.clone(), self.layout, self.shapes)

    def load_ema_state_dict(self, sd):
        self.ema = self.OP.join_flat(sd, self.layout, self.total)


class StubData:
    """What ``train`` asks of its dataset when the device part of a step is replaced"""

    def __init__(self, frames: int = FRAMES):
        self.frames, self.checks = frames, 0

    def __len__(self):
        return self.frames

    def check_status(self):
        self.checks += 1


def stub_step_grads(total: int, calls=None):
    """``step_grads`` for ``train``: the rank's poses lo .. hi - 1 of the batch ``rows`` give the flat gradient
    sum over them of (1 + frame % 5) at position (7 frame + k) % total for k = 0..2, and the loss sum
    sum of (3 + frame % 4): small integers in float32 / float64, exact in any order and any split.  The step's seeds
    enter through their low bits (seed % 3 added to one position), so a wrong step counter shows."""
    def fn(rows, lo, hi, B, seeds):
        assert rows.dtype == torch.int64 and rows.numel() == B and len(seeds) == 4
        flat = torch.zeros(total, dtype=torch.float32)
        loss = 0.0
        for f in rows[lo:hi].tolist():
            for k in range(3):
                flat[(7 * f + k) % total] += float(1 + f % 5)
            flat[f % total] += float(sum(s % 3 for s in seeds))
            loss += float(3 + f % 4)
        if calls is not None:
            calls.append((rows.tolist(), lo, hi, B, tuple(seeds)))
        return loss, flat
    return fn


def stub_frame_errors(input_2d, targets_3d, H, seq, i, noise, root_mode):
    """test_hyber's per-shard compute replaced: per-frame values of the frame alone, float64"""
    x = torch.from_numpy(np.asarray(input_2d)).double()
    t = torch.from_numpy(np.asarray(targets_3d)).double()
    p1 = (t.abs().mean(dim=(1, 2)) + x.abs().mean(dim=(1, 2))) * 1e-3
    return p1, 0.5 * p1


def states_equal(a, b) -> bool:
    """two checkpoint lists hold the same bits"""
    if len(a) != len(b) or a[2:4] != b[2:4]:
        return False
    dicts = [(a[0], b[0])] + ([(a[4], b[4])] if len(a) > 4 else [])
    for x, y in dicts:
        if list(x) != list(y) or not all(torch.equal(x[k], y[k]) for k in x):
            return False
    sa, sb = a[1], b[1]
    if sa["param_groups"] != sb["param_groups"] or sorted(sa["state"]) != sorted(sb["state"]):
        return False
    return all(torch.equal(sa["state"][i][k], sb["state"][i][k]) for i in sa["state"] for k in sa["state"][i])
