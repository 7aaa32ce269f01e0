"""CPU: the host packer for padded tiles (a GCNdiff model of fewer than 17 joints in a sampler instance's
17-joint arena) as a stand-alone program (tests/c/dpk_pack_padded_check.cpp) under the host sanitizers: the
instance table accepts 2..17 joints for GCNdiff, each shape by its own entry alone, and the arena packed from an
n-joint staging is, float for float, the arena of a 17-joint staging holding the zero-embedded n-joint graph terms."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "dpk_pack_padded_check.cpp")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"     # the system g++ may predate _Float16

EMBED = ("embed-h96-n16", "embed-h96-n2", "embed-h128-n16", "embed-h64-n2")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no ROCm clang++")
    exe = str(tmp_path_factory.mktemp("packpad") / "dpk_pack_padded_check")
    subprocess.run([CLANG, "-std=c++17", "-ffp-contract=off", "-O0", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True, capture_output=True, text=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = dict(line.split(" ", 1) for line in p.stdout.splitlines())
    out["returncode"] = p.returncode
    out["stderr"] = p.stderr
    return out


def test_program_ends_clean(lines):
    assert lines["returncode"] == 0, lines      # a sanitizer report or a failed check ends it with an error


def test_table_accepts_2_to_17_joints_by_their_own_entry(lines):
    assert lines["table"] == "ok=1"


@pytest.mark.parametrize("case", EMBED)
def test_padded_arena_is_the_zero_embedded_17_joint_arena(lines, case):
    assert lines[case] == "same_weights=1 arena_equal=1 others_equal=1 sparse=0 ok=1"


def test_h36m_subtree_of_16_joints_is_packed_dense(lines):
    assert lines["subtree-n16"] == "sparse=0"
