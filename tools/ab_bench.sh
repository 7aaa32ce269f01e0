# A/B timing of alternative builds of libdpk on the GPU box: bash tools/ab_bench.sh lib1.so lib2.so ...
# (each run: bench.py --no-cpu --no-variants --steps 20; the in-tree library is "default")
# AB_REPS: interleaved rounds (default 2).  AB_ARGS: further bench.py arguments, e.g. "--gemm f16x3" or
# "--config 3".  A library written NAME=VALUE@lib (lib: a path or "default") runs with that environment
# variable set, e.g. DPK_TILE_WAVES=8@default.
O=$GRAFT_REPO_ROOT/gpurun_out; mkdir -p $O
for rep in $(seq 1 ${AB_REPS:-2}); do
  for arm in default "$@"; do
    lib=${arm#*@}; env=
    if [ "$lib" != "$arm" ]; then env=${arm%%@*}; fi
    if [ "$lib" = default ]; then unset DPK_LIB; else export DPK_LIB=$lib; fi
    env $env timeout -k 10 120 python3 bench.py --no-cpu --no-variants --steps 20 $AB_ARGS > $O/ab.json 2>/dev/null || exit 1
    python3 -c "import json,sys; d=json.loads(open('$O/ab.json').read().strip().splitlines()[-1]); print('$arm', d['value'], d['roofline']['avg_launch_ms'])"
  done
done
