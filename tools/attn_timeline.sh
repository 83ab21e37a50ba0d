#!/bin/bash
# Diagnostic build: ttv_attn.hip with -DATTN_TIMELINE -> csrc/variants/libtitok_hip_timeline.so (tools/attn_timeline.py)
exec bash "$(dirname "$0")/../titok_video_amd/csrc/build.sh" --variant timeline ttv_attn -DATTN_TIMELINE
