"""CPU: the g14 fixtures (tools/gen_goldens_padded.py: the reference's GCNdiff at hid 96 / 4 heads / 2 layers on a
16-joint tree and hid 64 / 2 heads / 1 layer on a 15-joint tree, widths whose persistent sampler runs such
skeletons as padded tiles) are the recorded files, and the oracle reproduces them bit for bit, so the GPU tests
of tests/test_gpu_padded_joints.py may take the oracle as their yardstick at these joint counts."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from diffpose_amd.weights import synthetic_state_dict
from helpers import betas as _betas
from oracle import gcndiff_oracle as O

G14 = ["g14_shape_h96_n4_l2_j16.npz", "g14_shape_h64_n2_l1_j15.npz"]


def test_g14_files_are_the_recorded_ones():
    meta = json.load(open(os.path.join(GOLDEN, "meta_g14.json")))
    assert sorted(meta["sha256"]) == sorted(G14)
    for name, sha in meta["sha256"].items():
        assert hashlib.sha256(open(os.path.join(GOLDEN, name), "rb").read()).hexdigest() == sha, name


@pytest.mark.parametrize("name", G14)
def test_oracle_reproduces_g14(golden, name):
    g = golden(name)
    hid, nh, nl, npts = int(g["hid"]), int(g["n_head"]), int(g["num_layer"]), int(g["n_pts"])
    assert g["x"].shape == (8, npts, 5)
    sd = synthetic_state_dict(hid=hid, n_layers=nl, n_pts=npts)
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v, dtype="<f4").tobytes())
    meta = json.load(open(os.path.join(GOLDEN, "meta_g14.json")))
    assert meta["weights_sha256"][name] == h.hexdigest()
    P = O.params_to_torch(sd)
    graph = O.adjacency(npts, [tuple(e) for e in g["edges"].tolist()])
    assert np.array_equal(graph.numpy(), g["adj"])
    ones = torch.ones(1, 1, npts, dtype=torch.bool)
    x, t = torch.from_numpy(g["x"]), torch.from_numpy(g["t8"])
    fn = lambda xt, m, tt: O.gcndiff_forward(P, graph, xt, m, tt, n_layers=nl, heads=nh)  # noqa: E731
    assert np.array_equal(fn(x, ones, t).numpy(), g["eps"])
    mask2 = torch.from_numpy(g["mask2"])
    assert int(mask2.sum()) == npts - 2
    assert np.array_equal(fn(x, mask2, t).numpy(), g["eps_masked"])
    xs, x0s = O.generalized_steps(x, ones, [int(s) for s in g["seq"]], fn, _betas(int(g["T"])))
    assert g["xs"].shape == (11, 8, npts, 5) and g["x0s"].shape == (10, 8, npts, 5)
    assert np.array_equal(torch.stack(xs).numpy(), g["xs"])
    assert np.array_equal(torch.stack(x0s).numpy(), g["x0s"])
