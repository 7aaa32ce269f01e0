"""CPU: the host weight packer (csrc/dpk_stage.inc, dpk_layout.inc, dpk_pack.inc) as a stand-alone program
(tests/c/dpk_pack_check.cpp) under the host sanitizers.  Every packed buffer must match, bit for bit, the
digest recorded from the two loaders this packer replaced, run on the same LCG-built state dicts."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "dpk_pack_check.cpp")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"     # the system g++ may predate _Float16

# FNV-1a-64 digests of the host buffers packed at commit dd74c60 (before the loaders were merged): cases
# a-d by its dpk_set_graph + dpk_load_weights (shipped shape: hid 96 / 4 heads), e-f by its gen_set_graph +
# gen_load + its fused-width packer (dpkw: hid 128 / 8 heads; dpkn: hid 64 / 2 heads), on these inputs
EXPECTED = {
    # kind 0, 5 layers, H36M adjacency
    "a": "arena=868a614cfd64be86 temb=d837e1b2fd8a32d5 a16=c1a8b470f4a3ef27 abf=136d6b1554c65041 sparse=1 w16_ok=1",
    # kind 0, 3 layers, H36M plus the edge 3-6 (outside the compiled pattern)
    "b": "arena=c43216830e2f2c74 temb=c1e68062f23078b5 a16=12f5a9ebca9d1357 abf=1f5350ce5d70a061 sparse=0 w16_ok=1",
    # kind 1 (GCNpose, coords 2 -> 3), 4 layers
    "c": "arena=41d8080fd1292320 temb=a0a2c0baf3dce925 a16=05acc223b24001b7 abf=ddd2564828373e7e sparse=1 w16_ok=1",
    # as (a) with one GEMM weight at 1016.0: 64 w = 65024 is past the split-fp16 range
    "d": "arena=ff160630ca1d7caf temb=d837e1b2fd8a32d5 a16=c5919f734839866b abf=595033da42801107 sparse=1 w16_ok=0",
    # dpkw, 3 layers; dpkn, 5 layers: no half-width arenas (w16_ok stays at its default)
    "e": "arena=5125fe362b7a9b3a temb=40340e06c54754eb sparse=1 w16_ok=1",
    "f": "arena=d632cc0b47997f0a temb=d257d030c3574ac5 sparse=1 w16_ok=1",
}


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no ROCm clang++")
    exe = str(tmp_path_factory.mktemp("pack") / "dpk_pack_check")
    subprocess.run([CLANG, "-std=c++17", "-ffp-contract=off", "-O0", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True, capture_output=True, text=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr      # a sanitizer report ends the program with an error
    return dict(line.split(" ", 1) for line in p.stdout.splitlines())


@pytest.mark.parametrize("case", sorted(EXPECTED))
def test_packed_buffers_match_the_former_loaders(lines, case):
    assert lines[case] == EXPECTED[case]


def test_failed_load_names_the_key_and_leaves_the_staging(lines):
    assert lines["g-missing"] == "ok=0 unchanged=1 err=missing key gconv_layers.3.gconv2.gconv.bias"
    assert lines["g-wrong"] == "ok=0 unchanged=1 err=size mismatch for atten_layers.4.feed_forward.gconv2.fc.weight"
    assert lines["g-full"] == "ok=1 unchanged=0"        # the complete dict of the same values does load
