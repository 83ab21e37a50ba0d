#!/bin/bash
# Knock-out builds of the weight-stationary to_qkv kernel (ttv_qkv256ws.inc: -DQW_KO_LDS / _EPI / _MFMA / _X) -> titok_video_amd/csrc/variants/libtitok_hip_qw_<name>.so
#   tools/qkv256_knockout.sh build   (cross-compile only; the .so files travel to the GPU box)
#   tools/qkv256_knockout.sh run     (GPU box: tools/qkv256_bench.py under every variant)
set -e
R="$(cd "$(dirname "$0")/.." && pwd)"
V=$R/titok_video_amd/csrc/variants
NAMES=${NAMES:-"base lds epi mfma x lds_epi lds_epi_x rows"}
flags() { case $1 in base) echo "";; lds) echo "-DQW_KO_LDS=1";; epi) echo "-DQW_KO_EPI=1";; mfma) echo "-DQW_KO_MFMA=1";; x) echo "-DQW_KO_X=1";; lds_epi) echo "-DQW_KO_LDS=1 -DQW_KO_EPI=1";; lds_epi_x) echo "-DQW_KO_LDS=1 -DQW_KO_EPI=1 -DQW_KO_X=1";; rows) echo "-DQW_KO_ROWS=1";; st_base) echo "-DQKV_STAMPS";; st_mfmaonly) echo "-DQKV_STAMPS -DQW_KO_LDS=1 -DQW_KO_EPI=1 -DQW_KO_X=1";; esac; }
if [ "$1" = build ]; then
  mkdir -p $V
  bash $R/titok_video_amd/csrc/build.sh > /dev/null      # product objects up to date before the parallel variant builds
  for n in $NAMES; do
    bash $R/titok_video_amd/csrc/build.sh --variant qw_$n ttv_gemm -Wno-unused-variable $(flags $n) > $V/gemm_$n.log 2>&1 &
    [ $(jobs -r | wc -l) -ge 4 ] && wait -n
  done
  wait; ls -la $V/*.so
else
  for n in $NAMES; do
    echo "== variant $n"
    case $n in st_*) TTV_LIB_PATH=$R/titok_video_amd/csrc/variants/libtitok_hip_qw_$n.so python3 $R/tools/qkv256ws_clock.py 2>&1 | grep -v amdgpu.ids;;
      *) TTV_LIB_PATH=$R/titok_video_amd/csrc/variants/libtitok_hip_qw_$n.so ONLY_WS=1 python3 $R/tools/qkv256_bench.py 2>&1 | grep -v amdgpu.ids | grep "k_qkv256ws" | tail -4;; esac
  done
fi
