#!/bin/bash
# Diagnostic build of the to_qkv kernel with -DQKV_STAMPS (ttv_qkv256.inc) -> csrc/variants/libtitok_hip_qkvstamps.so, then tools/qkv256_stamps.py.
#   tools/qkv256_stamps.sh build   (cross-compile only; the library travels to the GPU box)
#   tools/qkv256_stamps.sh run     (GPU box: the reader under the library built before)         no argument: both
set -e
R="$(cd "$(dirname "$0")/.." && pwd)"
[ "$1" = run ] || bash $R/titok_video_amd/csrc/build.sh --variant qkvstamps ttv_gemm -DQKV_STAMPS -Wno-unused-variable $QKV_EXTRA
cd "$R"
[ "$1" = build ] || TTV_LIB_PATH=$R/titok_video_amd/csrc/variants/libtitok_hip_qkvstamps.so python3 tools/qkv256_stamps.py
