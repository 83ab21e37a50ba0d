#!/bin/bash
# Build libtitok_hip.so for gfx950 in-tree (the .so travels to the GPU box with the snapshot).  The only place that compiles and links it:
#   build.sh                                                  the product library -> ../libtitok_hip.so
#   build.sh --variant NAME UNIT[=SOURCE] ... [FLAGS ...]     an instrumented library -> variants/libtitok_hip_NAME.so (tools/README.md)
# A variant is the product's objects with the named units (names of HIP_SRCS) recompiled with the extra FLAGS into build/UNIT__NAME.o;
# UNIT=SOURCE compiles another source file in the unit's place (path relative to this directory).  Variants of different names may be
# built at the same time once the product objects are up to date (run build.sh once first).
set -e
cd "$(dirname "$0")"
OUT=../libtitok_hip.so
export FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=on -fno-slp-vectorize -Wall -Wno-unused-function"   # build_attn64.sh reads it
# host-only C++ (no HIP call, no kernel): the float64 rotary table must round as written, so no contraction
HOST_FLAGS="-O2 -std=c++17 -fPIC -ffp-contract=off -Wall"
# every object of the library, named once: compiled by the two loops, linked in this order
HIP_SRCS="ttv_elem ttv_gemm ttv_patch_embed ttv_attn ttv_attn_swp ttv_attn64 ttv_attn_pv8 ttv_mlp ttv_bwd ttv_train ttv_optim ttv_vq ttv_vq_train ttv_metrics ttv_lpips ttv_i3d ttv_inception ttv_vjepa ttv_resample ttv_crops ttv_disc ttv_panels ttv_video ttv_video_quality ttv_plan ttv_api"
HOST_SRCS="ttv_plan_host"
VARIANT=; UNITS=
if [ "$1" = --variant ]; then
  VARIANT=$2; shift 2 || true
  while [ $# -gt 0 ] && [ "${1#-}" = "$1" ]; do UNITS="$UNITS $1"; shift; done       # what follows the units: extra compiler flags
  [ -n "$VARIANT" ] && [ -n "$UNITS" ] || { echo "usage: build.sh --variant NAME UNIT[=SOURCE] ... [FLAGS ...]"; exit 2; }
  for u in $UNITS; do case " $HIP_SRCS " in *" ${u%%=*} "*) ;; *) echo "build.sh: ${u%%=*} is not one of HIP_SRCS"; exit 2;; esac; done
elif [ $# -gt 0 ]; then echo "usage: build.sh [--variant NAME UNIT[=SOURCE] ... [FLAGS ...]]"; exit 2
fi
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
OBJS=$(printf 'build/%s.o ' $HIP_SRCS $HOST_SRCS)
if [ -n "$VARIANT" ]; then
  pids=()
  for u in $UNITS; do
    f=${u%%=*}; src=${u#*=}; [ $u != $f ] || src=$f.hip
    o=build/${f}__$VARIANT.o
    if [ $f != ttv_attn64 ]; then hipcc $FLAGS "$@" -c $src -o $o &
    elif [ $u = $f ]; then bash build_attn64.sh $o "$@" &
    else echo "build.sh: ttv_attn64 takes no other source"; exit 2
    fi
    pids+=($!)
    OBJS=${OBJS/build\/$f.o /$o }
  done
  for p in "${pids[@]}"; do wait $p || exit 1; done
  mkdir -p variants
  OUT=variants/libtitok_hip_$VARIANT.so
fi
# --no-undefined: an object missing from the list is a link error here, not a load error on the GPU box
hipcc --offload-arch=gfx950 -shared -fPIC -Wl,--no-undefined $OBJS -o $OUT
echo "built $(realpath $OUT)"
