#!/bin/bash
# Diagnostic build: ttv_attn_swp.hip with -DSWP_STAMPS (+ extra -D flags) -> csrc/variants/libtitok_hip_swpstamps.so
exec bash "$(dirname "$0")/../titok_video_amd/csrc/build.sh" --variant swpstamps ttv_attn_swp -DSWP_STAMPS "$@"
