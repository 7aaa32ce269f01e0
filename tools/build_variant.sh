#!/bin/bash
# Build an alternative libdpk for A/B timing (tools/ab_bench.sh): tools/build_variant.sh NAME [-DFLAG=V ...]
# -> build/ab/NAME.so (the `variant` target of diffpose-nw_amd/Makefile: its flags plus the given defines).
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; shift
make -s -C "$ROOT/diffpose-nw_amd" variant NAME="$NAME" DEFS="$*" 2>&1 | grep -v "hip-link" || true
test -f "$ROOT/build/ab/$NAME.so" && echo "built build/ab/$NAME.so $*"
