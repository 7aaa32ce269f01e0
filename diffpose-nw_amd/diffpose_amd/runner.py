"""Diffpose — the reference runner's evaluation path on the HIP library.

Mirrors ``Diffpose`` in ``runners/diffpose_frame.py``:

| Method | Reference lines | What it does here |
|---|---|---|
| ``__init__`` | 26-58 | src_mask and betas from the config |
| ``create_diffusion_model`` | 118-132 | ``HipGCNdiff`` handle, optional checkpoint |
| ``create_pose_model`` | 134-154 | ``HipGCNpose`` handle, optional checkpoint |
| ``test_hyber`` | 270-420 | pose front-end plus uvxyz assembly (one launch); the K-step DDIM sampler (one launch); per-frame MPJPE / P-MPJPE (one launch); the reference's per-action accounting on the host. Returns (p1, p2) in mm |
| ``train_step`` | 211-233 for one batch | draws, the per-pose losses and every parameter's gradient in one ``dpk_diff_loss_grad`` call (eval mode), ``.grad`` on the caller's torch parameters, clipping, ``optimizer.step()``, the weights loaded back. Returns ``loss_diff`` |
| ``train`` | 156-268 | the run on a ``DeviceAdam``: per epoch the shuffle, one wait-free step per batch (``PoseGeneratorGMM.batch_device``, ``dpk_train_draws``, the gradient call, ``optimizer.step``), ``lr_decay``, the reference's checkpoint list, ``test_hyber(is_train=True)``; ``resume=``; data-parallel under torch.distributed. Returns (best_epoch, best_p1) |
| ``diffusion_loss`` | 203-233, forward only | the training objective in eval mode: per-pose-t noising, eps and the per-pose sums in one ``dpk_diff_loss`` call per batch; the reference's ``update(loss_diff, n)`` on the host. Returns the epoch average |

Several ranks (``torch.distributed`` initialised with world size > 1, one process per GPU): every
rank reads the same batches, takes the contiguous frame range ``shard_frames(B, world, rank)`` of
each with all ``test_times`` hypothesis rows of those frames, and runs pose, sampler and per-frame
metrics on it alone.  The one collective per batch is the final MPJPE reduction: an all-gather of
the per-frame (MPJPE, P-MPJPE) pairs (16 B per frame, fp64) back into frame order, after which
every rank runs the reference's unchanged accounting over the whole batch and returns the same
(p1, p2) as one process would.  A gather of per-frame values, not per-rank sums: the reference
books a mixed-action batch's P-MPJPE as the whole batch's mean once per frame
(``common/utils.py:136-150``), which per-shard sums cannot reproduce.  With eta > 0 the default
noise source ("torch") draws the reference's randn_like sequence for the whole batch
(``runners/diffpose_frame.py:359``, then one draw per step at ``common/utils_diff.py:65``) and each
rank keeps its rows, so the samples do not depend on the world size either.

``args.noise_start`` (default False, the reference as it stands) switches the reference's commented-out
line back on (``runners/diffpose_frame.py:355-363``): the sampler starts every hypothesis row from
``x * a.sqrt() + (e * noise_scale) * (1 - a).sqrt()`` with ``a`` the alpha-bar of ``args.t_start`` (default
``config.testing.test_num_diffusion_timesteps``, as ``:355``), inside the sampler launch.  A batch may then
be a 4-tuple whose last element is the GMM sampler's ``noise_scale [B,17,5]`` (absent: ones), the ``:359``
draw ``e`` is kept instead of dropped (drawn for the whole batch first, at eta = 0 too), and the best-of-H
and per-hypothesis-mean MPJPE / P-MPJPE are kept in ``hypothesis_loss`` beside the reference's
mean-aggregate (p1, p2), which stays what ``test_hyber`` returns.

The H36M ``.npz`` datasets are absent offline. ``test_hyber`` therefore takes an iterable of
``(input_2d [B,17,2], targets_3d [B,17,3], actions [B])`` batches, the shape the reference's
``PoseGenerator_gmm`` loader delivers after its GMM draw. If none is given, it uses seeded
synthetic batches (``data.synthetic_eval_batches``).

Other skeletons: ``config.model.n_pts`` (2..32, joint 0 the root) with ``config.data.edges``, a list of
``(i, j)`` joint pairs (required when ``n_pts`` is not 17; the default is the runner's 16 H36M edges),
sets the graph of both models, the key mask, the noise draws and every batch shape (17 above reads
``n_pts``).  ``config.data.actions``, if present, replaces the H36M action names of the per-action
accounting.  Such models run the per-op path of the sampler.

Checkpoints load with ``torch.load(weights_only=True)``.
"""
from __future__ import annotations

import logging
import os
import time
import types

import numpy as np
import torch

import torch.distributed as dist

from . import metrics
from .data import shard_frames, synthetic_batch, synthetic_eval_batches
from .dist import gather_frames, shard_rows
from .gcndiff import H36M_EDGES, HipGCNdiff, adj_mx_from_edges
from .gcnpose import HipGCNpose
from .schedule import get_beta_schedule, make_seq
from .weights import load_checkpoint, synthetic_state_dict


def default_config(test_times: int = 1, test_timesteps: int = 50, test_num_diffusion_timesteps: int = 50,
                   num_diffusion_timesteps: int = 51, batch_size: int = 1024):
    """The model / diffusion / testing values of configs/human36m_diffpose_uvxyz_cpn.yml, with the
    testing section set to the BASELINE K=50 configuration by default."""
    ns = types.SimpleNamespace
    return ns(
        model=ns(hid_dim=96, emd_dim=96, coords_dim=[5, 5], num_layer=5, n_head=4, dropout=0.25, n_pts=17),
        diffusion=ns(beta_schedule="linear", beta_start=0.0001, beta_end=0.001,
                     num_diffusion_timesteps=num_diffusion_timesteps),
        training=ns(batch_size=batch_size, num_workers=0),
        testing=ns(test_times=test_times, test_timesteps=test_timesteps,
                   test_num_diffusion_timesteps=test_num_diffusion_timesteps),
        data=ns(dataset="human36m", num_joints=17))


def default_args(**kw):
    a = types.SimpleNamespace(skip_type="uniform", eta=0.0, downsample=1, track_metrics=False, seed=19960903,
                              root_mode="quirk", noise="torch")
    for k, v in kw.items():
        setattr(a, k, v)
    return a


class Diffpose:
    def __init__(self, args, config, device=None):
        self.args = args
        self.config = config
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.n_pts = int(getattr(config.model, "n_pts", 17))
        data = getattr(config, "data", None)
        self.edges = getattr(data, "edges", None)
        if self.edges is None:
            if self.n_pts != 17:
                raise ValueError(f"config.data.edges is required for n_pts = {self.n_pts}: the default graph is "
                                 "the 17-joint H36M skeleton")
            self.edges = H36M_EDGES
        self.edges = tuple((int(i), int(j)) for i, j in self.edges)
        if any(not (0 <= i < self.n_pts and 0 <= j < self.n_pts) for i, j in self.edges):
            raise ValueError(f"config.data.edges names a joint outside 0..{self.n_pts - 1}: {self.edges}")
        actions = getattr(data, "actions", None)
        self.actions = list(metrics.TEST_ACTIONS if actions is None else actions)
        self.src_mask = torch.ones(1, 1, self.n_pts, dtype=torch.bool, device=self.device)
        d = config.diffusion
        betas = get_beta_schedule(beta_schedule=d.beta_schedule, beta_start=d.beta_start, beta_end=d.beta_end,
                                  num_diffusion_timesteps=d.num_diffusion_timesteps)
        self.betas = torch.from_numpy(betas).float().to(self.device)
        self.num_timesteps = self.betas.shape[0]
        self.track_metrics = getattr(args, "track_metrics", False)
        self.inference_times, self.memory_usage = [], []
        self.diffusion_step_count = []
        self.model_diff = self.model_pose = None
        self.noise_start = bool(getattr(args, "noise_start", False))
        self.t_start = int(getattr(args, "t_start", config.testing.test_num_diffusion_timesteps))
        self.hypothesis_loss = None

    def _adj(self):
        # by default the runner's 16 H36M edges (diffpose_frame.py:120-125)
        return adj_mx_from_edges(self.n_pts, self.edges)

    def create_diffusion_model(self, model_path=None, state_dict=None):
        self.model_diff = HipGCNdiff(self._adj(), self.config, device=self.device)
        if model_path:
            self.model_diff.load_state_dict(load_checkpoint(model_path, kind="diff"))
        else:
            self.model_diff.load_state_dict(state_dict if state_dict is not None else self._synthetic("diff"))

    def create_pose_model(self, model_path=None, state_dict=None):
        cfg = types.SimpleNamespace(**vars(self.config))
        cfg.model = types.SimpleNamespace(**vars(self.config.model))
        cfg.model.coords_dim = [2, 3]        # diffpose_frame.py:138 (on a copy: no aliasing of config)
        self.model_pose = HipGCNpose(self._adj(), cfg, device=self.device)
        if model_path:
            logging.info("initialize model by:" + model_path)
            self.model_pose.load_state_dict(load_checkpoint(model_path, kind="pose"))
        else:
            logging.info("initialize model randomly")
            self.model_pose.load_state_dict(state_dict if state_dict is not None else self._synthetic("pose"))

    def _synthetic(self, kind):
        m = self.config.model
        return synthetic_state_dict(kind=kind, hid=int(m.hid_dim), n_layers=int(m.num_layer), n_pts=self.n_pts)

    def _seq(self):
        te = self.config.testing
        return make_seq(self.args.skip_type, te.test_num_diffusion_timesteps, te.test_timesteps)

    @staticmethod
    def _world():
        """(world size, rank, distributed): an initialised torch.distributed job (world size 1
        included: the gather then runs over one rank), else (1, 0, False)."""
        if dist.is_available() and dist.is_initialized():
            return dist.get_world_size(), dist.get_rank(), True
        return 1, 0, False

    def _batch_noise(self, n_frames: int, H: int, K: int, world: int, rank: int):
        """This rank's rows of the reference's noise draws for one batch, or None (eta = 0, or the
        in-kernel "philox" source).  The reference draws e = randn_like(input_uvxyz) before the
        sampler (runners/diffpose_frame.py:359, unused) and then one randn_like per step
        (common/utils_diff.py:65); all are drawn for the whole batch so every world size sees the
        same numbers, and each rank keeps the rows of its frames (``shard_rows``)."""
        from .utils_diff import draw_noise

        src = getattr(self.args, "noise", "torch")
        if float(self.args.eta) == 0.0 or src in (None, "philox"):
            return None
        full = torch.empty((H * n_frames, self.n_pts, 5), dtype=torch.float32, device=self.device)
        draw_noise(full, 1, src)                        # :359's e, consumed and dropped like the reference's
        z = draw_noise(full, K, src)
        if world == 1:
            return z
        return z[:, shard_rows(n_frames, H, world, rank).to(z.device)].contiguous()

    def _batch_noise_start(self, n_frames: int, H: int, K: int, world: int, rank: int):
        """``_batch_noise`` with the hypothesis start on: (z rows or None, e rows or None).  The ``:359``
        draw e is kept, and is drawn first for the whole batch whatever eta is (the reference draws it at
        eta = 0 too); None for the "philox" source (the kernel's counter-based draws, keyed by the rank's
        own row index)."""
        from .utils_diff import draw_noise

        src = getattr(self.args, "noise", "torch")
        if src in (None, "philox"):
            return None, None
        full = torch.empty((H * n_frames, self.n_pts, 5), dtype=torch.float32, device=self.device)
        e = draw_noise(full, 1, src)[0]
        z = draw_noise(full, K, src) if float(self.args.eta) != 0.0 else None
        if world > 1:
            rows = shard_rows(n_frames, H, world, rank).to(e.device)
            e = e[rows].contiguous()
            z = None if z is None else z[:, rows].contiguous()
        return z, e

    def _frame_errors(self, input_2d, targets_3d, H, seq, i, noise, root_mode, start=None):
        """Pose model, sampler and per-frame metrics for one (shard of a) batch: float64 device
        tensors (MPJPE, P-MPJPE) in metres, one per frame.  Also records the reference's per-batch
        timing window under ``track_metrics``.  ``start``: (e rows or None, noise_scale rows [F,n_pts,5] or
        None) of the hypothesis start, which then runs inside the sampler launch."""
        F = input_2d.shape[0]
        if F == 0:
            e = torch.empty(0, dtype=torch.float64, device=self.device)
            return e, e.clone()
        input_2d = torch.as_tensor(input_2d).to(self.device)
        targets_3d = torch.as_tensor(targets_3d).to(self.device)
        track = self.track_metrics
        if track:
            torch.cuda.synchronize(self.device)
            tp = time.time()
        # GCNpose + root handling + cat + repeat(test_times): one launch
        x = self.model_pose.uvxyz(input_2d, self.src_mask, H, root_mode)
        if track:
            # the reference's window (runners/diffpose_frame.py:345-370): memory baseline and
            # start time after the pose model, stop after the sampler and a device sync
            torch.cuda.synchronize(self.device)
            self.pose_times.append(time.time() - tp)
            torch.cuda.reset_peak_memory_stats(self.device)
            mem0 = torch.cuda.memory_allocated(self.device)
            t0 = time.time()
        # generalized_steps(...)[0][-1]: the final sample only (no trajectory stacks)
        kw = {}
        if start is not None:
            e, scale = start
            if scale is not None:
                scale = torch.as_tensor(scale, dtype=torch.float32).to(self.device)
            kw = dict(t_start=self.t_start, start_scale=scale, start_noise=e)
        out = self.model_diff.sample(x, seq, self.betas, eta=self.args.eta, mask=self.src_mask,
                                     seed=self.args.seed + i, noise=noise, **kw)
        if track:
            torch.cuda.synchronize(self.device)
            self.inference_times.append(time.time() - t0)
            self.memory_usage.append((torch.cuda.max_memory_allocated(self.device) - mem0) / 2 ** 20)
            tm = time.time()
        p1, p2 = metrics.pose_errors(out, targets_3d, H, root_mode)
        if track:
            torch.cuda.synchronize(self.device)
            self.metrics_times.append(time.time() - tm)
        if start is not None:
            # per hypothesis, beside the mean-aggregate: sums of the best of H and of the H-average per frame
            h1, h2 = metrics.hypothesis_errors(out, targets_3d, H, root_mode)
            self._hyp_sums += torch.stack([h1.min(0).values.sum(), h2.min(0).values.sum(),
                                           h1.mean(0).sum(), h2.mean(0).sum()]).cpu()
            self._hyp_frames += F
        return p1, p2

    def test_hyber(self, batches=None, is_train=False, n_frames: int = 4096, frame_errors=None):
        """Evaluate; returns (p1, p2) = per-action-averaged MPJPE / P-MPJPE in mm.  Under a
        multi-rank torch.distributed job every rank returns the whole evaluation's (p1, p2)
        (module docstring).  ``frame_errors`` replaces the per-shard compute (tests of the
        distributed accounting on CPU): ``fn(input_2d, targets_3d, H, seq, batch_index, noise,
        root_mode) -> (p1, p2)`` for the rank's frames; with ``args.noise_start`` it is also passed
        ``start=(e rows, noise_scale rows)`` as a keyword."""
        te = self.config.testing
        H = int(te.test_times)
        seq = self._seq()
        self.diffusion_step_count = len(seq)        # runners/diffpose_frame.py:321
        if batches is None:
            other = {} if self.n_pts == 17 else {"num_pts": self.n_pts}
            if self.actions != metrics.TEST_ACTIONS:
                other["actions"] = self.actions
            batches = synthetic_eval_batches(n_frames, self.config.training.batch_size, seed=self.args.seed, **other)
        root_mode = getattr(self.args, "root_mode", "quirk")
        world, rank, distributed = self._world()
        if frame_errors is None:
            frame_errors = self._frame_errors
            self.model_diff.eval()
            self.model_pose.eval()
            self.model_diff.set_schedule(seq, self.betas, self.args.eta)
        epoch_p1, epoch_p2 = metrics.AverageMeter(), metrics.AverageMeter()
        err = metrics.define_error_list(self.actions)
        self.inference_times, self.memory_usage = [], []
        self.pose_times, self.metrics_times = [], []
        i = -1
        self._hyp_sums, self._hyp_frames = torch.zeros(4, dtype=torch.float64), 0
        with torch.no_grad():
            for i, batch in enumerate(batches):
                input_2d, targets_3d, actions = batch[:3]
                noise_scale = batch[3] if self.noise_start and len(batch) > 3 else None
                actions = list(actions)
                input_2d = np.asarray(input_2d, dtype=np.float32)
                targets_3d = np.asarray(targets_3d, dtype=np.float32)
                B = input_2d.shape[0]
                if targets_3d.shape[0] != B or len(actions) != B:
                    raise ValueError(f"batch {i}: {B} inputs, {targets_3d.shape[0]} targets, {len(actions)} actions")
                lo, hi = shard_frames(B, world, rank)
                kw = {}
                if self.noise_start:
                    noise, e = self._batch_noise_start(B, H, len(seq), world, rank)
                    if noise_scale is not None:
                        noise_scale = np.asarray(noise_scale, dtype=np.float32)
                        if noise_scale.shape != (B, self.n_pts, 5):
                            raise ValueError(f"batch {i}: noise_scale must be ({B}, {self.n_pts}, 5), "
                                             f"got {noise_scale.shape}")
                        noise_scale = np.ascontiguousarray(noise_scale[lo:hi])
                    kw["start"] = (e, noise_scale)
                else:
                    noise = self._batch_noise(B, H, len(seq), world, rank)
                p1, p2 = frame_errors(np.ascontiguousarray(input_2d[lo:hi]), np.ascontiguousarray(targets_3d[lo:hi]),
                                      H, seq, i, noise, root_mode, **kw)
                if distributed:
                    # the final MPJPE reduction: per-frame (p1, p2) of every rank, in frame order
                    both = gather_frames(torch.stack([p1, p2], dim=1).to(torch.float64), B, 1)
                    p1, p2 = both[:, 0], both[:, 1]
                p1h, p2h = p1.cpu().numpy(), p2.cpu().numpy()     # 16 B per frame to the host
                epoch_p1.update(float(np.mean(p1h)) * 1000.0, B)
                epoch_p2.update(float(np.mean(p2h)) * 1000.0, B)
                metrics.test_calculation(p1h, p2h, actions, err, n_joints=self.n_pts)
        if self.track_metrics and self.inference_times:
            # Final computational metrics (runners/diffpose_frame.py:407-409)
            log_dir = getattr(self.args, "log_path", None)
            path = os.path.join(log_dir, "performance_metrics.txt" if world == 1 else
                                f"performance_metrics_rank{rank}.txt") if log_dir else None
            self.log_performance_metrics(path)
        logging.info("sum (%d) | MPJPE: %.4f | P-MPJPE: %.4f", i + 1, epoch_p1.avg, epoch_p2.avg)
        self.epoch_loss = (epoch_p1.avg, epoch_p2.avg)
        # this rank's frames: best-of-H and per-hypothesis-average MPJPE / P-MPJPE in mm (noise_start only)
        self.hypothesis_loss = None
        if self._hyp_frames:
            b1, b2, m1, m2 = (self._hyp_sums * 1000.0 / self._hyp_frames).tolist()
            self.hypothesis_loss = {"best": (b1, b2), "mean": (m1, m2), "frames": self._hyp_frames}
        self.action_error_sum = err
        return metrics.print_error(None, err, is_train if rank == 0 else True)   # one table per job

    def _pose_losses(self, x0, noise_scale, t, e, i):
        """Per-pose denoising losses of one (shard of a) batch: one ``dpk_diff_loss`` call, float32 [F] on the device."""
        if x0.shape[0] == 0:
            return torch.empty(0, dtype=torch.float32, device=self.device)
        dev = lambda a: torch.as_tensor(a, dtype=torch.float32).to(self.device)   # noqa: E731
        return self.model_diff.diffusion_loss(dev(x0), t, self.betas, noise_scale=dev(noise_scale), noise=dev(e),
                                              mask=self.src_mask)

    def diffusion_loss(self, batches=None, n_frames: int = 4096, pose_losses=None):
        """The validation value of the reference's training objective (runners/diffpose_frame.py:203-233 with the
        model in eval mode: dropout off, no backward): for every batch ``(targets_uvxyz [B,n_pts,5], noise_scale
        [B,n_pts,5], ...)`` — the leading two of what ``PoseGeneratorGMM.batch`` yields — draw ``t`` as ``:216-218``
        (``schedule.training_timesteps``) and ``e`` as ``:214``, take ``loss_diff`` = the mean of the per-pose
        losses (``HipGCNdiff.diffusion_loss``) and book ``update(loss_diff, B)`` as ``:233``; returns the epoch
        average.  ``t`` and ``e`` come from one CPU generator seeded with ``args.seed``, drawn for the whole batch,
        so the value does not depend on the world size: under a multi-rank torch.distributed job each rank runs
        the poses ``shard_frames(B, world, rank)`` and one all-gather of the per-pose losses (4 B per pose) puts
        them back in batch order, after which every rank books the same mean as one process would.  Without
        ``batches``: seeded synthetic poses with noise scales in [0.5, 1.5).  ``pose_losses`` replaces the per-shard
        compute (tests of the distributed accounting on CPU): ``fn(x0, noise_scale, t, e, batch_index) -> [F]``
        float32 losses for the rank's F poses, ``t`` an int64 CPU tensor and ``e`` a float32 CPU tensor."""
        from .schedule import training_timesteps

        if batches is None:
            x, _ = synthetic_batch(n_frames, seed=self.args.seed, num_pts=self.n_pts)
            rng = np.random.Generator(np.random.PCG64(self.args.seed + 1))
            scale = (0.5 + rng.random(size=x.shape)).astype(np.float32)
            bs = int(self.config.training.batch_size)
            batches = [(x[lo:lo + bs], scale[lo:lo + bs]) for lo in range(0, n_frames, bs)]
        world, rank, distributed = self._world()
        if pose_losses is None:
            pose_losses = self._pose_losses
            self.model_diff.eval()
        gen = torch.Generator().manual_seed(int(self.args.seed))
        epoch = metrics.AverageMeter()
        with torch.no_grad():
            for i, batch in enumerate(batches):
                x0, noise_scale = batch[0], batch[1]
                x0 = torch.as_tensor(x0).detach().to(torch.float32)
                noise_scale = torch.as_tensor(noise_scale).detach().to(torch.float32)
                B = x0.shape[0]
                if tuple(x0.shape) != (B, self.n_pts, 5) or noise_scale.shape != x0.shape:
                    raise ValueError(f"batch {i}: targets_uvxyz and noise_scale must be ({B}, {self.n_pts}, 5), got "
                                     f"{tuple(x0.shape)} and {tuple(noise_scale.shape)}")
                if B == 0:
                    continue
                e = torch.randn((B, self.n_pts, 5), generator=gen)             # :214, for the whole batch
                t = training_timesteps(B, self.num_timesteps, generator=gen)   # :216-218
                lo, hi = shard_frames(B, world, rank)
                loss = pose_losses(x0[lo:hi], noise_scale[lo:hi], t[lo:hi], e[lo:hi], i).to(torch.float32)
                if distributed:
                    loss = gather_frames(loss.reshape(-1, 1), B, 1).reshape(-1)
                epoch.update(float(loss.cpu().mean()), B)                      # :226's batch mean, :233
        self.epoch_loss_diff = epoch.avg
        return epoch.avg

    def train_step(self, targets_uvxyz, noise_scale, optimizer, params=None, generator=None, return_losses: bool = False):
        """One gradient step on one batch: the body of the reference's training loop (runners/diffpose_frame.py:211-233)
        with the model in eval mode (dropout off).  Draws ``e`` (:214) and the antithetic ``t`` (:216-218) as
        ``diffusion_loss`` does (torch's default generator, or ``generator``), takes the per-pose losses and every
        parameter's gradient in one ``HipGCNdiff.diffusion_loss_grad`` call, assigns them as ``.grad`` of ``params``
        (the caller's dict name -> torch parameter on the model's device, the state_dict's names), clips with
        ``config.optim.grad_clip`` when the config has one (:229), calls ``optimizer.step()`` (:230) and loads the
        updated ``params`` back into the handle.  Returns ``loss_diff`` (a float, :226).

        The reference trains with dropout ``config.model.dropout`` (:195 ``model_diff.train()``).  With
        ``args.train_dropout`` set the step is the reference's train-mode step: the gradient call runs with dropout at
        the reference's rates (``diffusion_loss_grad(dropout=True)``) under counter-based masks whose seed is one
        63-bit ``torch.randint`` from ``generator``, drawn after ``e`` and ``t``, so the same generator gives the same
        ``e`` and ``t`` with or without the flag.  Without it a config whose dropout is not 0 raises
        NotImplementedError unless ``args.train_without_dropout`` is set (eval-mode gradients).

        With a ``DeviceAdam`` (``model_diff.device_optimizer(config)``) as ``optimizer`` the step stays on the device: the
        gradient call, then ``optimizer.step(grads)`` (clip, Adam, EMA and the refresh of the weights the kernels read);
        no ``.grad`` assignments, no ``load_state_dict``, ``params`` unused.  ``return_losses`` returns the per-pose
        losses (float32 [B] on the device) instead of their mean as a float, which costs a wait for the device."""
        from .schedule import training_timesteps

        train_dropout = self._dropout_mode()
        x0 = torch.as_tensor(targets_uvxyz).detach().to(torch.float32)
        noise_scale = torch.as_tensor(noise_scale).detach().to(torch.float32)
        B = x0.shape[0]
        if tuple(x0.shape) != (B, self.n_pts, 5) or noise_scale.shape != x0.shape or B == 0:
            raise ValueError(f"targets_uvxyz and noise_scale must be (B, {self.n_pts}, 5) with B > 0, got "
                             f"{tuple(x0.shape)} and {tuple(noise_scale.shape)}")
        e = torch.randn((B, self.n_pts, 5), generator=generator)                   # :214
        t = training_timesteps(B, self.num_timesteps, generator=generator)        # :216-218
        dev = lambda a: a.to(self.device)   # noqa: E731
        drop = {}
        if train_dropout:
            drop = dict(dropout=True, dropout_seed=int(torch.randint(0, 2 ** 63 - 1, (1,), generator=generator)))
        loss, grads = self.model_diff.diffusion_loss_grad(dev(x0), t, self.betas, noise_scale=dev(noise_scale),
                                                          noise=dev(e), mask=self.src_mask, **drop)
        from .optim import DeviceAdam

        if isinstance(optimizer, DeviceAdam):
            optimizer.step(grads)
            return loss if return_losses else float(loss.mean())
        if params is None:
            raise TypeError("train_step with a torch optimiser needs params (name -> torch parameter)")
        for name, g in grads.items():
            params[name].grad = g.to(params[name].dtype)
        clip = getattr(getattr(self.config, "optim", None), "grad_clip", None)
        if clip is not None:
            torch.nn.utils.clip_grad_norm_(list(params.values()), clip)
        optimizer.step()
        self.model_diff.load_state_dict({k: v.detach() for k, v in params.items()})
        return loss if return_losses else float(loss.mean())

    def train_epoch(self, batches, optimizer, generator=None):
        """The inner loop of the reference's training epoch (runners/diffpose_frame.py:203-236) over ``batches`` of
        ``(targets_uvxyz [B,n_pts,5], noise_scale [B,n_pts,5], ...)`` with a ``DeviceAdam``: one ``train_step`` per
        batch.  Every step's per-pose losses stay on the device and are read once, after the last step, so the loop
        itself never waits for the device; returns the epoch's ``AverageMeter`` value (:233, ``update(loss_diff, B)``),
        also kept as ``epoch_loss_diff``."""
        from .optim import DeviceAdam

        if not isinstance(optimizer, DeviceAdam):
            raise TypeError("train_epoch runs the device-side step: pass model_diff.device_optimizer(...); a torch "
                            "optimiser takes train_step(..., params=...) per batch")
        kept = []
        for batch in batches:
            losses = self.train_step(batch[0], batch[1], optimizer, generator=generator, return_losses=True)
            kept.append(losses)
        epoch = metrics.AverageMeter()
        for losses in kept:
            epoch.update(float(losses.cpu().mean()), losses.numel())
        self.epoch_loss_diff = epoch.avg
        return epoch.avg

    def _dropout_mode(self) -> bool:
        """``train_step``'s rule: True for the train-mode step (``args.train_dropout``), False for eval-mode gradients;
        a config with dropout and neither flag raises."""
        p_drop = float(getattr(self.config.model, "dropout", 0.0) or 0.0)
        train_dropout = bool(getattr(self.args, "train_dropout", False))
        if p_drop != 0.0 and not train_dropout and not getattr(self.args, "train_without_dropout", False):
            raise NotImplementedError(f"config.model.dropout = {p_drop}: the device backward runs without dropout masks "
                                      "by default; set args.train_dropout to train with dropout as the reference does, "
                                      "args.train_without_dropout to train in eval mode, or dropout to 0")
        return train_dropout

    def train_draws(self, e_seed: int, t_seed: int, B: int, lo: int = 0, hi=None, stream=None):
        """``dpk_train_draws`` for poses ``lo .. hi - 1`` of a batch of ``B``: ``(e [hi - lo, n_pts, 5], t [hi - lo])``
        float32 device tensors, each value a function of its seed and its global index alone (a shard's rows are
        bitwise the whole batch's rows).  ``e`` is what the loss calls draw for ``noise=None`` under ``seed=e_seed``;
        ``t`` the reference's antithetic pair draw (runners/diffpose_frame.py:216-218)."""
        import ctypes

        from . import _lib

        hi = B if hi is None else hi
        n = hi - lo
        e = torch.empty((n, self.n_pts, 5), dtype=torch.float32, device=self.device)
        t = torch.empty(n, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream(self.device) if stream is None else stream
            rc = _lib.lib().dpk_train_draws(ctypes.c_uint64(e_seed & (2 ** 64 - 1)), ctypes.c_uint64(t_seed & (2 ** 64 - 1)),
                                            int(self.num_timesteps), int(B), int(lo), int(n), self.n_pts * 5,
                                            e.data_ptr() if n else None, t.data_ptr() if n else None, st.cuda_stream)
        if rc:
            raise _lib.DpkError("dpk_train_draws", rc, f"T {self.num_timesteps} batch {B} pose0 {lo} n {n}")
        return e, t

    def _host_betas(self):
        """``self.betas`` as a host array, read back once: a gradient call given it does not wait for the device"""
        if getattr(self, "_betas_host", None) is None:
            self._betas_host = np.ascontiguousarray(self.betas.cpu().numpy(), dtype=np.float32)
        return self._betas_host

    def _step_grads(self, train_data, rows, lo, hi, B, seeds, dropout):
        """The device part of one step of ``train`` for this rank's poses ``lo .. hi - 1`` of the batch ``rows``: the
        whole batch's GMM draw (its uniforms are keyed by the output position) and its rows, this shard's e and t,
        the gradient call with weight 1 / B.  Returns (the shard's loss sum, a float64 0-d device tensor; the flat
        gradient).  Nothing here waits for the device."""
        gmm_seed, e_seed, t_seed, drop_seed = seeds
        uvxyz, scale = train_data.batch_device(rows, gmm_seed)
        e, t = self.train_draws(e_seed, t_seed, B, lo, hi)
        drop = dict(dropout=True, dropout_seed=drop_seed) if dropout else {}
        loss, grads = self.model_diff.diffusion_loss_grad(uvxyz[lo:hi], t, self._host_betas(), noise_scale=scale[lo:hi],
                                                          noise=e, mask=self.src_mask, weight=1.0 / B, pose0=lo, **drop)
        return loss.sum(dtype=torch.float64), grads.flat

    def _train_inner(self, train_data, optimizer, epoch: int, step: int, step_grads=None, dropout: bool = False):
        """The inner loop of epoch ``epoch`` of ``train`` from global step ``step``: the epoch's permutation (one upload),
        then per batch the device part of the step, the all-reduce of the gradient where there are several ranks and
        ``optimizer.step``.  Returns (the global step after the epoch, this rank's loss sum per batch as a float64
        device tensor, the batch sizes).  Waits for the device only at the reference's ``i % 100`` log line."""
        from .schedule import train_epoch_permutation, train_step_seeds

        world, rank, distributed = self._world()
        bs, n_data = int(self.config.training.batch_size), len(train_data)
        perm = train_epoch_permutation(self.args.seed, epoch, n_data).to(self.device)     # one upload per epoch
        n_batches = (n_data + bs - 1) // bs
        slots = torch.zeros(n_batches, dtype=torch.float64, device=self.device)
        sizes, seen = [], 0
        for i in range(n_batches):
            step += 1
            rows = perm[i * bs:(i + 1) * bs]
            B = int(rows.numel())
            lo, hi = shard_frames(B, world, rank)
            seeds = train_step_seeds(self.args.seed, step)
            if step_grads is not None:
                loss_sum, flat = step_grads(rows, lo, hi, B, seeds)
            else:
                loss_sum, flat = self._step_grads(train_data, rows, lo, hi, B, seeds, dropout)
            if distributed:
                dist.all_reduce(flat, op=dist.ReduceOp.SUM)
            optimizer.step(flat)
            slots[i] = loss_sum
            sizes.append(B)
            seen += hi - lo
            if i % 100 == 0 and i != 0:
                logging.info("| Epoch%04d: %04d/%04d | Step %06d | Loss: %.6f |", epoch, i + 1, n_batches, step,
                             float(slots[:i + 1].sum()) / max(seen, 1))
        return step, slots, sizes

    def train(self, train_data, eval_batches=None, resume=None, *, optimizer=None, step_grads=None, frame_errors=None):
        """The reference's training run (runners/diffpose_frame.py:156-268) on the device-side step: for
        ``config.training.n_epochs`` epochs, shuffle ``train_data`` (a ``PoseGeneratorGMM`` on this runner's device),
        take one clip + Adam + EMA step per batch of ``config.training.batch_size`` frames (the last, partial batch
        kept), then decay the learning rate (``config.optim.{lr, decay, lr_gamma}``, common/utils.py:26-30), write the
        reference's checkpoint to ``ckpt_{epoch}.pth`` and ``ckpt.pth`` under ``args.log_path`` and evaluate with
        ``test_hyber(batches=eval_batches, is_train=True)`` (``eval_batches``: an iterable, a callable that returns
        a fresh one per epoch, or None for ``test_hyber``'s own default).  Returns ``(best_epoch, best_p1)``, kept as
        ``self.best_epoch``, ``self.best_p1``; every epoch's loss average (the reference's ``AverageMeter`` over
        ``update(loss_diff, B)``) is ``self.epoch_loss_diff``, all of them ``self.train_log``.

        The optimiser is ``model_diff.device_optimizer(config)`` (Adam; RMSProp and SGD raise there), opened here unless
        one is already open on the model or given as ``optimizer``, and left open on return.  Dropout follows
        ``train_step``'s rule (``args.train_dropout`` / ``args.train_without_dropout``).

        Every draw is a function of ``(args.seed, epoch, step)`` (``schedule.word``): the 1-based global step s uses
        words 4 s .. 4 s + 3 as the GMM seed, e's seed, t's seed and the dropout seed; epoch ep shuffles with
        ``schedule.train_epoch_permutation``.  No generator state lives elsewhere, so ``resume=path`` (a checkpoint
        written here or by the reference: parameters, Adam state, epoch, step and the EMA shadow when present)
        continues the uninterrupted run exactly, except that ``best_p1`` is not in the reference's format and
        restarts at 1000.

        Several ranks (an initialised torch.distributed job): every rank draws the whole batch's GMM sample and runs
        the poses ``shard_frames(B, world, rank)`` with weight 1 / B and the batch's own rows of e, t and the dropout
        masks (``dpk_train_draws``, ``pose0``); one all-reduce of the flat gradient per step, and every rank applies
        the same bits with the deterministic ``dpk_train_apply``, so the parameters stay bitwise equal without a
        broadcast.  One more all-reduce per epoch sums the per-batch loss slots.  Rank 0 writes the files.

        The inner loop does not wait for the device except at the reference's ``i % 100`` log line, which reads this
        rank's losses so far.  ``step_grads`` replaces the device part of a step (tests of the loop, the sharding, the
        collectives, the schedule and the checkpoints on the CPU): ``fn(rows, lo, hi, B, seeds) -> (loss sum of the
        rank's poses, flat gradient)`` with ``rows`` the batch's int64 frame indices on the runner's device and
        ``seeds`` the step's four; ``frame_errors`` is passed on to ``test_hyber``."""
        cfg, args = self.config, self.args
        if optimizer is None:
            optimizer = getattr(self.model_diff, "_trainer", None) or self.model_diff.device_optimizer(cfg)
        dropout = self._dropout_mode() if step_grads is None else False
        world, rank, distributed = self._world()
        lr_init, decay, gamma = cfg.optim.lr, cfg.optim.decay, cfg.optim.lr_gamma
        ema = bool(getattr(cfg.model, "ema", False))
        log_path = getattr(args, "log_path", None)
        best_p1, best_epoch = 1000, 0
        start_epoch, step = 0, 0
        if resume is not None:
            states = torch.load(resume, map_location="cpu", weights_only=True)
            optimizer.load_params(states[0])
            optimizer.load_state_dict(states[1])
            if len(states) > 4:
                optimizer.load_ema_state_dict(states[4])
            start_epoch, step = int(states[2]) + 1, int(states[3])
        self.train_log = []
        for epoch in range(start_epoch, int(cfg.training.n_epochs)):
            step, slots, sizes = self._train_inner(train_data, optimizer, epoch, step, step_grads, dropout)
            if distributed:
                dist.all_reduce(slots, op=dist.ReduceOp.SUM)
            meter = metrics.AverageMeter()
            for total, B in zip(slots.cpu().tolist(), sizes):
                meter.update(total / B, B)                                    # :233 with loss_diff = the batch mean
            self.epoch_loss_diff = meter.avg
            if epoch % decay == 0:
                lr_now = lr_init * gamma ** (epoch / decay)                   # common/utils.py:26-30
                for group in optimizer.param_groups:
                    group["lr"] = lr_now
            train_data.check_status()
            if rank == 0 and log_path:
                from collections import OrderedDict

                states = [OrderedDict(("module." + k, v.detach().cpu().clone())
                                      for k, v in optimizer.params_state_dict().items()),
                          optimizer.state_dict(), epoch, step]
                if ema:
                    states.append(OrderedDict((k, v.detach().cpu().clone())
                                              for k, v in optimizer.ema_state_dict().items()))
                os.makedirs(log_path, exist_ok=True)
                torch.save(states, os.path.join(log_path, f"ckpt_{epoch}.pth"))
                torch.save(states, os.path.join(log_path, "ckpt.pth"))
            logging.info("test the performance of current model")
            kw = {} if frame_errors is None else {"frame_errors": frame_errors}
            p1, p2 = self.test_hyber(batches=eval_batches() if callable(eval_batches) else eval_batches, is_train=True,
                                     **kw)
            if p1 < best_p1:
                best_p1, best_epoch = p1, epoch
            logging.info("| Best Epoch: %04d MPJPE: %.2f | Epoch: %04d MPJEPE: %.2f PA-MPJPE: %.2f |", best_epoch,
                         best_p1, epoch, p1, p2)
            self.train_log.append(dict(epoch=epoch, step=step, loss_diff=self.epoch_loss_diff, p1=p1, p2=p2,
                                       lr=float(optimizer.param_groups[0]["lr"])))
        self.best_p1, self.best_epoch = best_p1, best_epoch
        return best_epoch, best_p1

    def log_performance_metrics(self, output_path=None):
        """Summary of the per-batch inference times and peak-memory deltas collected under
        ``args.track_metrics``, logged and (with a path) written in the reference's file format
        (runners/diffpose_frame.py:422-461).  ``inference_times`` cover the sampler call alone,
        between device syncs, as the reference's cover its generalized_steps call (:352-370);
        the pose-model and metrics times of each batch are kept beside them (``pose_times``,
        ``metrics_times``) and appended to the raw data."""
        if not self.track_metrics or not self.inference_times:
            return
        times, mem = self.inference_times, self.memory_usage
        avg_time, max_time, min_time = sum(times) / len(times), max(times), min(times)
        steps_data = f"Diffusion steps: {self.diffusion_step_count}"
        if mem:
            mem_data = f"Memory (MB): avg={sum(mem) / len(mem):.2f}, min={min(mem):.2f}, max={max(mem):.2f}"
        else:
            mem_data = "Memory: not tracked"
        logging.info("=== Performance Summary ===")
        logging.info(f"Time (s): avg={avg_time:.4f}, min={min_time:.4f}, max={max_time:.4f}")
        logging.info(steps_data)
        logging.info(mem_data)
        if output_path:
            with open(output_path, "w") as f:
                f.write("=== Performance Metrics ===\n")
                f.write(f"Time (s): avg={avg_time:.4f}, min={min_time:.4f}, max={max_time:.4f}\n")
                f.write(f"{steps_data}\n")
                f.write(f"{mem_data}\n")
                f.write("\n=== Raw Data ===\n")
                f.write(f"Times: {times}\n")
                f.write(f"Memory: {mem}\n")
                # not in the reference's file: the rest of each batch, outside its timing window
                f.write(f"Pose model times: {getattr(self, 'pose_times', [])}\n")
                f.write(f"Metrics times: {getattr(self, 'metrics_times', [])}\n")
