"""CPU: the per-op path's host-side launch rule (csrc/dpk_genplan.inc) as a stand-alone program
(tests/c/dpk_genplan_check.cpp) under the host sanitizers: which GEMM kernel, tile height, grid and LDS size each
side of every predicate gets, the gemm_sk pack plan and packer, the staged-or-global choices and the gradient
call's scratch plan.  The forward, the training forward and the backward's dX GEMMs all launch through this one
rule; the expected lines below are worked out by hand from the rule as DESIGN.md states it (the per-op path's
kernel forms), never read off a run."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "dpk_genplan_check.cpp")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

# the base GEMM: 119 rows (7 poses x 17 joints), K = N = ldc = 32, every operand 16-byte aligned, a packed copy with
# NJ 2, 256 CUs: 4 32-row tiles beat 2 64-row and 1 128-row tile (cost 32 < 64 < 128); gemm_sk's grid is
# ceil(119 / 16) x ceil(2 column tiles / NJ)
SCALAR32 = "gemm<32,scalar> bm=32 vec=0 grid=4x1 lds=0"
VEC32 = "gemm<32,vec> bm=32 vec=1 grid=4x1 lds=0"
SK2 = "gemm_sk<2> bm=32 vec=1 grid=8x1 lds=0"
EXPECTED = {
    "gemm_base": SK2,
    # N <= 8 with K N 4 <= 65536: one wave per row, W in LDS
    "gemm_n8": "gemm_narrow bm=32 vec=1 grid=30x1 lds=3072",
    "gemm_n9": SCALAR32,
    "gemm_narrow_lds_at": "gemm_narrow bm=32 vec=1 grid=30x1 lds=65536",
    "gemm_narrow_lds_past": SCALAR32,                    # K 3277, N 5
    # vec: K % 4, N % 4, A and W
    "gemm_k_off": SCALAR32, "gemm_n_off": SCALAR32, "gemm_a_off": SCALAR32, "gemm_w_off": SCALAR32,
    # gemm_sk only: C, bias, tproj, tp_stride % 4, ldc % 4, a packed copy
    "gemm_c_off": VEC32, "gemm_bias_off": VEC32, "gemm_tp": SK2, "gemm_tp_off": VEC32, "gemm_tps_off": VEC32,
    "gemm_ldc_off": VEC32, "gemm_unpacked": VEC32,
    "gemm_nj4": "gemm_sk<4> bm=32 vec=1 grid=8x2 lds=0",  # 8 column tiles, 4 per workgroup
    # M K 4 + K 4 = 2^31 - 16384 and 2^31 (K 4096); at 1024 / 2048 / 4096 tiles on 256 CUs every height costs 512
    # rows: the taller tile wins the tie
    "gemm_oor_below": "gemm_sk<2> bm=128 vec=1 grid=8192x1 lds=0",
    "gemm_oor_at": "gemm<128,vec> bm=128 vec=1 grid=1024x1 lds=0",
    "gemm_switch_lds": VEC32,
    # 153 rows under a forced height: a partial second 128-row tile, a partial third 64-row tile
    "gemm_bm128": "gemm<128,vec> bm=128 vec=1 grid=2x1 lds=0",
    "gemm_bm64": "gemm<64,vec> bm=64 vec=1 grid=3x1 lds=0",
    "gemm_bm32": "gemm<32,vec> bm=32 vec=1 grid=5x1 lds=0",
    "gemm_bm48": "gemm<32,vec> bm=32 vec=1 grid=5x1 lds=0",      # ignored: the rule's own 32
    "gemm_bm64_sk": "gemm_sk<2> bm=64 vec=1 grid=8x1 lds=0",
    "switch_unset": "sk=1 bm=0", "switch_lds_64": "sk=0 bm=64", "switch_other": "sk=1 bm=0",
    "tile_119_200cu": VEC32, "tile_119_256cu": VEC32,
    "tile_tie": "gemm<128,vec> bm=128 vec=1 grid=1x1 lds=0",     # one CU: 1 x 128 = 2 x 64 = 4 x 32
    "tile_129_1cu": "gemm<32,vec> bm=32 vec=1 grid=5x1 lds=0",   # 256 > 192 > 160
    # (K 15, N 32) has no copy; 36 x 32: 3 chunks x 2 tiles x 256; 516 x 1548: 33 chunks x 98 (97 padded) x 256;
    # 128 x 384: 8 x 24 x 256, 24 column tiles in fours
    "pack_36x32": "off=0 NJ=2", "pack_516x1548": "off=1536 NJ=2", "pack_128x384": "off=829440 NJ=4",
    "pack_48x20": "off=878592 NJ=2",
    "pack_total": "packs=4 floats=880128 match=1 skipped=1 found=1",
    # hid 32, 2 layers: 6 blocks a layer, 3072 + 1024 + 2048 + 2048 + 3072 + 3072 floats; the input ChebConv (K 15) none
    "pack_g16": "packs=12 floats=28672 same=1",
    # hid 320 / 8 heads / 17 joints: 17 x 964 x 4 = 65552 bytes
    "attn_w320": "attention<FF> ppb=1 blocks=5 lds=0",
    "attn_tt": "attention<TT> ppb=7 blocks=1 lds=36176",         # 17 x 76 x 4 a pose, 256 / 34 poses
    "attn_tf": "attention<TF> ppb=3 blocks=3 lds=22236",         # d_k 9: 17 x 109 x 4 a pose, 256 / 68 poses
    "attn_out_off": "attention<TF> ppb=7 blocks=1 lds=34748",    # 17 x 73 x 4
    "attn_bwd_w320": "hb=8 stage=0 lds=18496",                   # 2 x 8 x 289 floats; + 17 x 1281 floats is past 64 KB
    "attn_bwd_g16": "hb=2 stage=1 lds=13396",
    "attn_bwd_j32": "hb=4 stage=1 lds=51328",                    # 4096 / 1024 heads a pass
    "dlg_w320_2hid": "stage=0 lds=0 blocks=1",                   # 2 x 17 x 641 floats
    "dlg_w320_hid": "stage=1 lds=43656 blocks=1",                # 2 x 17 x 321
    "dlg_n9": "stage=1 lds=4488 blocks=2",
    "graph_w260_2hid": "stage=0 lds=0 blocks=325",               # (32 x 520 + 1024) x 4 = 70656
    "graph_w260_hid": "stage=1 lds=37376 blocks=5",
    "cheb_w516_hid": "stage=0 lds=0 blocks=323",                 # (32 x 516 + 2048) x 4 = 74240
    "cheb_w516_input": "stage=1 lds=8832 blocks=5",
    "dw_vec": "vec=1 grid=1x1 ps=3104",                          # 2 x 1 tiles of 64 x 64
    "dw_g_off": "vec=0 grid=1x2 ps=3104",                        # 6 x 1 tiles of 16 x 32
    "dw_k15": "vec=0 grid=6x1 ps=512",                           # 680 rows: six slabs
    # N = 1: 256 + 2 (9 x 576 + 3 x 1664 + 2 x 1088) + 576 + 1664 + 64 + 64 + 4 x 128
    "plan_g16_n1": "stash=27840 floats=51840 aligned=1 ordered=1 stash_ok=1 floats_ok=1 formula=1 null_same=1",
    "plan_g16_n40": "stash=1079040 floats=1363520 aligned=1 ordered=1 stash_ok=1 floats_ok=1 formula=1 null_same=1",
    "plan_odd": "stash=89984 floats=117120 aligned=1 ordered=1 stash_ok=1 floats_ok=1 formula=1 null_same=1",
}


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no ROCm clang++")
    exe = str(tmp_path_factory.mktemp("genplan") / "dpk_genplan_check")
    subprocess.run([CLANG, "-std=c++17", "-O0", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True, capture_output=True, text=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr      # a sanitizer report ends it with an error
    return dict(line.split(" ", 1) for line in p.stdout.splitlines())


def test_every_line_expected(lines):
    assert sorted(lines) == sorted(EXPECTED)


@pytest.mark.parametrize("case", sorted(EXPECTED))
def test_genplan_case(lines, case):
    assert lines[case] == EXPECTED[case]


def test_pinned_form_sets_importable_without_gpu():
    """the whole-shape sets the GPU tests observe (tests/test_gpu_diff_grad.py) live beside the cases"""
    import diff_grad_cases as GC
    assert GC.BWD_FORMS_W320 == (GC.BWD_FORMS - {"attention_bwd<T>"}) | {"attention_bwd<F>", "dlg<F>"}
    assert set(GC.GEMM_FORMS) == {"g16", "odd"}
