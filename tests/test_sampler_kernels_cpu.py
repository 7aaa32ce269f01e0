"""CPU: the table of tests/sampler_cells.py against what is compiled.

tests/test_gpu_sampler_kernels.py runs one cell per kernel of the persistent sampler and asserts that their union
is _lib.compiled_sampler_kernels().  That list is enumerated by the library beside its launchers
(csrc/dpk_genfused.inc, list_mode), so three things are closed here, without a GPU:
  * the list equals the sample_kernel symbols of the gfx950 code object inside the built libdpk.so (names only:
    the namespace and the six template arguments parsed from the mangled names), so nothing compiled is unlisted
    and nothing listed is uncompiled, and their number is the one the rules give, 226, with the per-namespace
    split of sampler_cells.COUNTS;
  * every compiled kernel is claimed by a cell and no cell claims a kernel that is not compiled;
  * on every fp32 / f16x3 cell's inputs the oracle's own gap g = max|o32 - o64| stays under
    edge_inputs.G_CEILING, so 8 g never loosens the 5e-6 bar unnoticed.
The first two need the built library and skip without it, like tests/test_asm_hazards.py.
"""
import collections
import os
import re
import subprocess
import sys
import tempfile

import pytest

import edge_inputs as E
import sampler_cells as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import asm_hazard_check as H  # noqa: E402

from diffpose_amd import _lib  # noqa: E402

LIB = os.path.join(ROOT, "diffpose-nw_amd", "diffpose_amd", "libdpk.so")
needs_lib = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(H.OBJDUMP)),
                               reason="needs the built libdpk.so and llvm-objdump")
# <ns>::sample_kernel<(int)MODE, (bool)SPARSE, (int)G16, (int)ZM, (bool)START, (bool)PAD>(SampleArgs, ...)
SYMBOL = re.compile(r"_ZN(\d+)([a-z0-9]+?)13sample_kernelILi(\d)ELb([01])ELi(\d)ELi(\d)ELb([01])ELb([01])EEEv[A-Za-z0-9_]*")


def _code_object_kernels():
    """The names (_lib.sampler_kernel_name) of the sample_kernel functions in the code object's symbol table."""
    with tempfile.TemporaryDirectory() as t:
        co = os.path.join(t, "co.elf")
        with open(co, "wb") as f:
            f.write(H.code_object(LIB))
        table = subprocess.run([H.OBJDUMP, "-t", co], check=True, capture_output=True, text=True).stdout
    names = []
    for line in table.splitlines():
        sym = line.split()[-1] if line.split() else ""
        if "sample_kernel" not in sym or "." in sym:      # .kd descriptors and the .num_vgpr ... resource symbols
            continue
        m = SYMBOL.fullmatch(sym)
        assert m and int(m.group(1)) == len(m.group(2)), sym
        ns, mode, sparse, g16, zm, start, pad = m.group(2), *(int(v) for v in m.groups()[2:])
        names.append(_lib.sampler_kernel_name(_lib.sampler_kernel_id(
            ns, _lib.SAMPLER_MODES[mode], sparse, _lib.SAMPLER_GEMMS[g16], zm, start, pad)))
    return names


def test_kernel_names_round_trip():
    for c in C.CELLS:
        kid = _lib.sampler_kernel_id(c.tile, c.mode, c.sparse, c.gemm, c.zm, c.start, c.pad)
        assert _lib.sampler_kernel_name(kid) == c.name and kid < 1 << 12
    assert _lib.sampler_kernel_name(_lib.sampler_kernel_id("dpk8", "sample", True, "bf16", 1, True)) == \
        "dpk8/sample/sparse/bf16/z1/start"
    assert len(C.BY_NAME) == len(C.CELLS)


@needs_lib
def test_library_list_is_the_code_objects_symbols():
    compiled = _lib.compiled_sampler_kernels()
    symbols = _code_object_kernels()
    assert len(set(compiled)) == len(compiled) and len(set(symbols)) == len(symbols)
    assert set(symbols) == set(compiled), sorted(set(symbols) ^ set(compiled))
    per_ns = collections.Counter(n.split("/")[0] for n in symbols)
    assert dict(per_ns) == C.COUNTS and len(symbols) == C.TOTAL == sum(C.COUNTS.values()), per_ns


@needs_lib
def test_library_list_reports_its_full_count():
    """*count always gets the full number, whatever the buffer holds; a null count is refused."""
    import ctypes

    L = _lib.lib()
    n = ctypes.c_int(-1)
    assert L.dpk_debug_sampler_kernels(None, None, 0, ctypes.byref(n)) == 0 and n.value == C.TOTAL
    buf = (ctypes.c_uint32 * 4)()
    assert L.dpk_debug_sampler_kernels(None, buf, 4, ctypes.byref(n)) == 0 and n.value == C.TOTAL
    assert [_lib.sampler_kernel_name(v) for v in buf] == _lib.compiled_sampler_kernels()[:4]
    assert L.dpk_debug_sampler_kernels(None, buf, 4, None) == -1
    assert L.dpk_debug_sampler_kernels(None, None, 4, ctypes.byref(n)) == -1


@needs_lib
def test_cells_claim_exactly_the_compiled_kernels():
    compiled = set(_lib.compiled_sampler_kernels())
    assert not compiled - set(C.BY_NAME), f"compiled, no cell: {sorted(compiled - set(C.BY_NAME))}"
    assert not set(C.BY_NAME) - compiled, f"a cell for a kernel that is not compiled: {sorted(set(C.BY_NAME) - compiled)}"


def test_cell_table_follows_the_rules():
    per_ns = collections.Counter(c.tile for c in C.CELLS)
    assert dict(per_ns) == C.COUNTS and len(C.CELLS) == C.TOTAL
    assert sum(c.gemm == "bf16" for c in C.CELLS) == 32
    # the never-run families come last
    flags = [c.never_run for c in C.CELLS]
    assert flags == sorted(flags) and any(flags) and not all(flags)
    # every bf16 cell's case exists and has a bar or a recorded reason for none
    import bf16_scheme as B
    from test_gpu_bf16_scheme import BARS

    for c in C.CELLS:
        if c.gemm == "bf16":
            name = C.bf16_case(c)
            assert name in B.ALL_CASES + B.KERNEL_CASES
            assert (name in BARS) + (name in C.BF16_BARS) + (name in C.BF16_DROPPED) == 1, name
    assert set(C.BF16_BARS) | set(C.BF16_DROPPED) == set(B.KERNEL_CASES)


_ORACLE_KEYS = sorted({(C.shape_of(c), c.mode == "pose", bool(c.zm), c.start) for c in C.CELLS if c.gemm != "bf16"},
                      key=repr)


def _key_id(key):
    (hid, heads, _, npts, edges), pose, noise, start = key
    graph = "chain" if npts != 17 else "dense" if edges == C.DENSE_EDGES else "h36m"
    return f"h{hid}n{heads}-j{npts}{graph}" + "-pose" * pose + "-noise" * noise + "-start" * start


@pytest.mark.parametrize("shape,pose,noise,start", _ORACLE_KEYS, ids=[_key_id(k) for k in _ORACLE_KEYS])
def test_oracle_gap_stays_under_the_ceiling(shape, pose, noise, start):
    if pose:
        o = E.pose_oracles("baseline", shape, E.N, 2, "relative")
    else:
        o = E.diff_oracles("baseline", shape, E.N, noise, start)
    for k, (o32, o64, g) in o.items():
        print(f"{k}: g {g:.3e}")
        assert g <= E.G_CEILING, (k, g)
        assert bool(o32.isfinite().all()) and bool(o64.isfinite().all())
    if start:
        r = E.regime("baseline", shape, start=True)
        assert not (r["x_T"] == r["x"]).all() and r["start_scale"].shape[0] < r["x"].shape[0]
