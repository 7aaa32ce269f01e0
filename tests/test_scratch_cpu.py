"""CPU: the scratch pool every launch path takes its device buffers from (csrc/dpk_scratch.inc) as a
stand-alone program over a fake runtime (tests/c/dpk_scratch_check.cpp) under the host sanitizers: which
buffer a call may write, what a capture takes and gives back, and that nothing leaks or is freed twice."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "dpk_scratch_check.cpp")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

# buffers are named b1, b2, ... in order of allocation, streams 1 and 2
EXPECTED = {
    # two streams, two buffers; growing stream 1's (b1 -> b4) syncs stream 1 only, then hook, then free; the
    # spare grows alongside, the new one (b5) allocated before the old one (b2) is freed
    "a": "different=1 same=1 grown=1 events=sync:1,hook:b1,free:b1,free:b2",
    "b": "spare_cap=100 spare_same=1",
    "c": "first=ok took_spare=1 spare_cap=0 second=ok same=1 larger=shared-too-small(100) other_stream=no-spare(0) "
         "held=1",
    # live buffers: stream + capture + spare of 50; the capture's 100 replace the spare; again with a spare of
    # 200, and the capture's 100 are freed
    "d": "live=3 larger_becomes_spare=1 live=2 live=3 smaller_freed=1 live=2",
    # the spare's allocation fails (the one permitted failure: only a later capture needs it)
    "e": "request=ok spare_kept=1 error_cleared=1 captured=ok from_old_spare=1",
    # the stream's own allocation fails: the call's failure, error 2 (out of memory) left for the caller
    "e2": "request=failed error=2 stream_cap=0",
    "f": "after_pool=1 after_held=0",
}


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no ROCm clang++")
    exe = str(tmp_path_factory.mktemp("scratch") / "dpk_scratch_check")
    subprocess.run([CLANG, "-std=c++17", "-O0", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True, capture_output=True, text=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr      # a sanitizer report (a leak included) ends it with an error
    return dict(line.split(" ", 1) for line in p.stdout.splitlines())


@pytest.mark.parametrize("case", sorted(EXPECTED))
def test_scratch_pool_case(lines, case):
    assert lines[case] == EXPECTED[case]
