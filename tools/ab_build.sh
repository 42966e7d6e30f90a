#!/bin/bash
# Build a kernel variant of libpow_gpu.so from a copy of csrc/ for tools/ab_sweep.
#   tools/ab_build.sh <csrc-dir> <out-dir>
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
src=$1; out=$2
mkdir -p "$out"
# the shipped library's source list (build.py), taken from the copy in <csrc-dir>
srcs=$(cd "$R" && python3 -m mpi_blockchain_amd.build --sources | sed "s|.*/|$src/|")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -shared -std=c++17 -mcode-object-version=5 \
  -I "$R/include" -I "$src" $srcs ${AB_FLAGS:-} -o "$out/libpow_gpu.so"
