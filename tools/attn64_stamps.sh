#!/bin/bash
# Diagnostic build of the 64-rows-per-wave attention kernel with -DATTN64_STAMPS (extra defines: $1) -> csrc/variants/libtitok_hip_stamps64.so
exec bash "$(dirname "$0")/../titok_video_amd/csrc/build.sh" --variant stamps64 ttv_attn64 -DATTN64_STAMPS $1
