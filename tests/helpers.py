"""Helpers that several test files share (imported like tests/edge_inputs.py; no fixtures in here)."""
import socket

import numpy as np
import torch

from diffpose_amd.schedule import get_beta_schedule


def betas(T=51):
    """the linear beta schedule of the reference's configs over T timesteps"""
    return torch.from_numpy(get_beta_schedule("linear", beta_start=1e-4, beta_end=1e-3,
                                              num_diffusion_timesteps=T)).float()


def maxdiff(a, b):
    """max |a - b| in float64 of two tensors or arrays of one shape"""
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, np.float64)
    assert a.shape == b.shape
    return float(np.abs(a - b).max())


def mpjpe_mm(out, targets):
    """MPJPE in mm of the root-relative xyz of out (N, 17, 5; tensor or array) against targets (N, 17, 3)"""
    o = out.detach().cpu().double() if torch.is_tensor(out) else torch.from_numpy(np.asarray(out)).double()
    xyz = o[:, :, 2:]
    xyz = xyz - xyz[:, :1, :]
    t = torch.from_numpy(np.asarray(targets)).double()
    return float(torch.mean(torch.norm(xyz - t, dim=-1)) * 1000.0)


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port
