"""CPU: the split-fp16 (gemm mode 1) weight arena of the four persistent-sampler instances other than the
shipped shape (dpkw hid 128 / 8 heads, dpkw4 128 / 4, dpkn 64 / 2, dpkn4 64 / 4), packed by the host packer
(csrc/dpk_pack.inc) and read back by the documented layout in a stand-alone program
(tests/c/dpk_pack16_check.cpp) under the host sanitizers.

The bound on (hi + lo) / 64 against the staged weight is derived in the program from the fp16 format
(split_bound): max(2^-22 |w|, 2^-31).  A packer that leaves these instances without the arena (as before
gemm mode 1 existed at these widths) fails the program's size check, so every test here fails with it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "dpk_pack16_check.cpp")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"     # the system g++ may predate _Float16

INSTANCES = {"dpkw": (128, 3), "dpkw4": (128, 5), "dpkn": (64, 2), "dpkn4": (64, 5)}     # hid, layers packed


def _fields(line):
    return dict(kv.split("=", 1) for kv in line.split())


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no ROCm clang++")
    exe = str(tmp_path_factory.mktemp("pack16") / "dpk_pack16_check")
    subprocess.run([CLANG, "-std=c++17", "-ffp-contract=off", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True, capture_output=True, text=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr      # a sanitizer report or a missing arena ends it with an error
    return {k: _fields(v) for k, v in (line.split(" ", 1) for line in p.stdout.splitlines())}


@pytest.mark.parametrize("inst", sorted(INSTANCES))
def test_arena_sizes(lines, inst):
    """The split-fp16 arena has the layout's size (5 layers x the six GEMMs' 2 KiB blocks) and there is no
    bf16 arena: gemm mode 2 stays with the shipped shape."""
    f = lines[inst]
    hid = INSTANCES[inst][0]
    # per layer: (3 + 1 + 2) D x D + D x 2D + 2 (D x 3D) = 14 D^2 weights, two halves (hi, lo) each
    assert int(f["expected"]) == 5 * 14 * hid * hid * 4
    assert f["a16_bytes"] == f["expected"] and f["sized"] == "1"
    assert f["abf_empty"] == "1" and f["abf_bytes"] == "0"
    assert f["w16_ok"] == "1"


@pytest.mark.parametrize("inst", sorted(INSTANCES))
def test_every_weight_once_within_the_split_rounding(lines, inst):
    f = lines[inst + "-values"]
    hid, layers = INSTANCES[inst]
    assert int(f["layers"]) == layers and int(f["checked"]) == layers * 14 * hid * hid
    assert f["bad"] == "0", f
    assert f["missing"] == "0" and f["dup"] == "0" and f["tiled"] == "1"
    assert f["past"] == "0"                       # layers the model does not have stay zero
    assert float(f["worst_over_bound"]) <= 1.0
    assert f["sub_lo"] == "1" and f["zero_lo"] == "1"     # the inputs reached the subnormal and the exact cases


@pytest.mark.parametrize("inst", sorted(INSTANCES))
def test_out_of_range_weight_turns_w16_ok_off(lines, inst):
    f = lines[inst + "-range"]
    assert f["w16_ok"] == "0"
    assert f["plain_a16_empty"] == "1" and f["plain_abf_empty"] == "1"     # pack(s, p, false): no half-width arenas
