"""CPU: what dpk_diff_loss_grad promises that needs no GPU: the new symbols, the gradient layout table and the
transposed weight arena (csrc/dpk_grad_layout.inc as a stand-alone program under the host sanitizers,
tests/c/dpk_grad_layout_check.cpp), and the yardstick itself: autograd through the float32 oracle against the g16
fixture written by the reference's own loss_diff.backward() (tools/gen_goldens_grad.py)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import diff_grad_cases as GC
from conftest import ROOT
from diffpose_amd import _lib
from diffpose_amd.weights import param_shapes

SRC = os.path.join(ROOT, "tests", "c", "dpk_grad_layout_check.cpp")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
NEW = ("dpk_diff_loss_grad", "dpk_param_count", "dpk_param_layout", "dpk_debug_grad_forms")
# (hid, heads, joints, layers, coords): the g16 shape, the shipped one, nothing a multiple of 4, 32 joints, coords 12
LAYOUT_SHAPES = ((32, 2, 17, 2, 5), (96, 4, 17, 5, 5), (15, 3, 17, 2, 5), (36, 4, 32, 1, 5), (36, 2, 17, 2, 12))


def test_new_symbols_in_header_exports_and_library():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "diffpose_kernels.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = set(re.findall(r"\bT (dpk_\w+)", out))
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.EXPORTS and name in syms, name
    L = _lib.lib()
    assert L.dpk_version() >= 102
    assert L.dpk_param_count(None) == 0
    assert L.dpk_diff_loss_grad(None, None, None, None, 0, None, 0, 0.0, None, None, 0, None) == -1


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no ROCm clang++")
    path = str(tmp_path_factory.mktemp("gradlayout") / "dpk_grad_layout_check")
    subprocess.run([CLANG, "-std=c++17", "-ffp-contract=off", "-O0", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", SRC, "-o", path], check=True, capture_output=True, text=True)
    return path


@pytest.mark.parametrize("shape", LAYOUT_SHAPES, ids=lambda s: "h%d_n%d_j%d_l%d_c%d" % s)
def test_layout_table_and_transposed_arena(exe, shape, tmp_path):
    hid, heads, joints, layers, coords = shape
    p = subprocess.run([exe] + [str(v) for v in shape] + [str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr      # a sanitizer report ends the program with an error
    lines = [ln.split() for ln in p.stdout.splitlines()]
    table = [(ln[2], int(ln[3]), int(ln[4])) for ln in lines if ln[0] == "entry"]
    shapes = param_shapes(hid=hid, n_layers=layers, n_pts=joints, coords=(coords, coords))
    # names, order and numels of the state_dict; offsets multiples of 4, entries packed in order
    assert [t[0] for t in table] == list(shapes)
    assert [t[2] for t in table] == [int(np.prod(s)) for s in shapes.values()]
    off = 0
    for _, o, n in table:
        assert o == off and o % 4 == 0
        off += (n + 3) // 4 * 4
    floats = int(next(ln[1] for ln in lines if ln[0] == "floats"))
    assert floats == table[-1][1] + table[-1][2]
    # the transposed arena: every block the numpy transpose of the staged block, everything else as staged
    stage = np.fromfile(tmp_path / "stage.bin", dtype=np.float32)
    trans = np.fromfile(tmp_path / "trans.bin", dtype=np.float32)
    sd = np.fromfile(tmp_path / "sd.bin", dtype=np.float32)
    n_stage, zero, zero_n, ahat, jj4, total = (int(v) for v in next(ln[1:] for ln in lines if ln[0] == "arena"))
    assert stage.size == n_stage == zero and trans.size == total == ahat + layers * jj4 and ahat == zero + zero_n
    blocks = [(int(ln[1]), int(ln[2]), int(ln[3])) for ln in lines if ln[0] == "block"]
    assert len(blocks) == 7 * layers + 4 + layers
    same = np.ones(n_stage, dtype=bool)
    for w, K, N in blocks:
        assert same[w:w + K * N].all(), "blocks overlap"
        same[w:w + K * N] = False
        assert np.array_equal(trans[w:w + K * N].reshape(N, K), stage[w:w + K * N].reshape(K, N).T), (w, K, N)
    assert np.array_equal(trans[:n_stage][same], stage[same])
    assert not trans[zero:ahat].any() and zero_n >= max(3 * hid, 3 * coords, 4 * hid, layers * hid)
    # A_hat as loaded, one layer per jj4 floats; the staged Laplacian is c_i^-1/2 A_ij c_j^-1/2 of it
    pos, by_name = 0, {}
    for name, _, n in table:
        by_name[name] = sd[pos:pos + n]
        pos += n
    for l in range(layers):
        a = by_name[f"atten_layers.{l}.feed_forward.A_hat"]
        assert np.array_equal(trans[ahat + l * jj4: ahat + l * jj4 + joints * joints], a)
    # the QKV block of the staging is [in][q | k | v]: the split the reduce pass undoes
    wqkv = blocks[0]
    q = by_name["atten_layers.0.self_attn.linears.0.weight"].reshape(hid, hid)
    assert np.array_equal(stage[wqkv[0]:wqkv[0] + 3 * hid * hid].reshape(hid, 3 * hid)[:, :hid], q.T)


def test_float32_oracle_autograd_is_the_reference_backward(golden):
    z = GC.golden_g16(golden)
    i = GC.g16_inputs(golden)
    assert torch.equal(i["x_t"], z["x_t"])                  # the float32 noising in the reference's order
    sums, g32 = GC.autograd(i, torch.float32)
    assert torch.equal(sums, z["sums"]) and torch.equal(sums.mean(dim=0), z["loss_diff"])
    names = [k[5:] for k in z if k.startswith("grad.")]
    assert sorted(names) == sorted(g32) == sorted(param_shapes(hid=32, n_layers=2))
    for k in names:
        assert torch.equal(g32[k], z["grad." + k]), k
    # the float32 forward is the oracle's
    from oracle import gcndiff_oracle as O
    with torch.no_grad():
        eps = O.gcndiff_forward(O.params_to_torch(i["sd"]), torch.from_numpy(i["adj"]), i["x_t"], i["mask"], i["t"],
                                n_layers=2, heads=2)
    assert torch.equal(eps, z["eps"])


def test_bars_are_the_oracles_own_gaps(golden):
    """gap_p is 1e-7 .. 1e-5 of each tensor's largest entry at the g16 shape; the key biases' gradient is zero"""
    ref = GC.references(GC.g16_inputs(golden))
    for k, g in ref["g64"].items():
        scale = float(g.abs().max())
        if k.endswith("linears.1.bias"):
            assert scale < 1e-12 and ref["bar"][k] >= GC.GAP_FACTOR * ref["gap"][k.replace("linears.1", "linears.0")]
            continue
        assert 0 < ref["gap"][k] <= 2e-5 * scale, (k, ref["gap"][k], scale)
        assert ref["bar"][k] == GC.GAP_FACTOR * ref["gap"][k]
