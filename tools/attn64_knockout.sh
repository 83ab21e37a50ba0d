#!/bin/bash
# Diagnostic builds of the 64-rows-per-wave attention kernel with single ingredients knocked out (garbage results, same launch):
# csrc/variants/libtitok_hip_ko64_<name>.so for name in dma lds max exp all.  Run tools/attn_bench.py with TTV_LIB_PATH on each
# (tools/attn64_knockout_run.sh).
set -e
for v in "dma:-DW64_KO_DMA=1" "lds:-DW64_KO_LDS=1" "max:-DW64_KO_MAX=1" "exp:-DW64_KO_EXP=1" "all:-DW64_KO_DMA=1 -DW64_KO_LDS=1 -DW64_KO_MAX=1 -DW64_KO_EXP=1"; do
  name=${v%%:*}; defs=${v#*:}
  bash "$(dirname "$0")/../titok_video_amd/csrc/build.sh" --variant ko64_$name ttv_attn64 $defs
done
