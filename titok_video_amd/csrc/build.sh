#!/bin/bash
# Build libtitok_hip.so for gfx950 in-tree (the .so travels to the GPU box with the snapshot).
set -e
cd "$(dirname "$0")"
OUT=../libtitok_hip.so
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=on -fno-slp-vectorize -Wall -Wno-unused-function"
# host-only C++ (no HIP call, no kernel): the float64 rotary table must round as written, so no contraction
HOST_FLAGS="-O2 -std=c++17 -fPIC -ffp-contract=off -Wall"
# every object of the library, named once: compiled by the two loops, linked in this order
HIP_SRCS="ttv_elem ttv_gemm ttv_patch_embed ttv_attn ttv_attn_swp ttv_attn64 ttv_mlp ttv_bwd ttv_train ttv_optim ttv_vq ttv_vq_train ttv_metrics ttv_lpips ttv_i3d ttv_vjepa ttv_resample ttv_crops ttv_disc ttv_panels ttv_plan ttv_api"
HOST_SRCS="ttv_plan_host"
mkdir -p build
pids=()
for f in $HIP_SRCS; do
  if [ ! -f build/$f.o ] || [ $f.hip -nt build/$f.o ] || [ ttv_common.h -nt build/$f.o ] || [ ttv_kernels.h -nt build/$f.o ] || { [ $f = ttv_gemm ] && { [ ttv_qkv256.inc -nt build/$f.o ] || [ ttv_qkv256ws.inc -nt build/$f.o ]; }; } || [ ../../include/titok_hip.h -nt build/$f.o ]; then
    if [ $f = ttv_attn64 ]; then bash build_attn64.sh build/$f.o &       # two-step build: see build_attn64.sh
    else hipcc $FLAGS -c $f.hip -o build/$f.o &
    fi
    pids+=($!)
  fi
done
for f in $HOST_SRCS; do
  if [ ! -f build/$f.o ] || [ $f.cpp -nt build/$f.o ] || [ ../../include/titok_hip.h -nt build/$f.o ]; then
    hipcc $HOST_FLAGS -c $f.cpp -o build/$f.o &
    pids+=($!)
  fi
done
for p in "${pids[@]}"; do wait $p || exit 1; done
hipcc --offload-arch=gfx950 -shared -fPIC $(printf 'build/%s.o ' $HIP_SRCS $HOST_SRCS) -o $OUT
echo "built $(realpath $OUT)"
