#!/bin/bash
# Diagnostic builds of the pipelined attention kernel with one ingredient knocked out each (results are garbage, the launch time
# tells what the ingredient costs): csrc/variants/libtitok_hip_ko_{dma,barrier,valu,lds,all}.so;  run with
#   TTV_LIB_PATH=titok_video_amd/csrc/variants/libtitok_hip_ko_dma.so FP32=0 python tools/attn_bench.py 1.5
set -e
for v in dma barrier valu lds all; do
  case $v in
    dma) D="-DPP_KO_DMA=1";; barrier) D="-DPP_KO_BARRIER=1";; valu) D="-DPP_KO_VALU=1";; lds) D="-DPP_KO_LDS=1";; all) D="-DPP_KO_DMA=1 -DPP_KO_BARRIER=1 -DPP_KO_VALU=1 -DPP_KO_LDS=1";;
  esac
  bash "$(dirname "$0")/../titok_video_amd/csrc/build.sh" --variant ko_$v ttv_attn $D
done
