#!/bin/bash
# Diagnostic build: ttv_bwd.hip with -DWG_STAMPS (extra -D flags pass through) -> csrc/variants/libtitok_hip_wgstamps.so
exec bash "$(dirname "$0")/../titok_video_amd/csrc/build.sh" --variant wgstamps ttv_bwd -DWG_STAMPS "$@"
