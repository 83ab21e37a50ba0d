#!/bin/bash
# Diagnostic build: the attention and layer-tail sources with -DATTN_STAMPS / -DMLP_STAMPS -> csrc/variants/libtitok_hip_stamps.so
exec bash "$(dirname "$0")/../titok_video_amd/csrc/build.sh" --variant stamps ttv_attn ttv_mlp -DATTN_STAMPS -DMLP_STAMPS
