# One iteration on a GPU box, from the repository root: the GPU tests, the full bench line, the phase traces.
# Output under build/iter/; stops at the first step that fails.
O=build/iter; mkdir -p $O
timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $O/gpu_tests.log 2>&1; rc=$?
tail -3 $O/gpu_tests.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 200 python bench.py --full --cpu-frames 256 > $O/b.json 2>&1 && timeout -k 10 120 python tools/phase_trace.py --run > $O/trace_fp32.txt 2>&1 && timeout -k 10 120 python tools/phase_trace.py --run --gemm f16x3 > $O/trace_f16.txt 2>&1
