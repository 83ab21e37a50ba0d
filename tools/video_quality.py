#!/usr/bin/env python3
"""The per-frame quality kernels (titok_video_amd/video.py: frame_sse, frame_ssim) on one GPU, at the 64 x 256 x 256 video of
tools/video_roundtrip.py and with its measurement: HIP events over launches that rotate over working sets which together exceed
twice the 256 MiB Infinity Cache (an HBM rate), and over one set (cache-warm).

  frame_sse, frame_ssim   one call each over the whole video, packed RGB against packed RGB and NV12 against NV12: us and GB/s over
                          the bytes compared (both sides, every sample once: 2 x 3 bytes per RGB pixel, 2 x 1.5 per 4:2:0 pixel);
  the yardstick           a device-to-device copy_ of the same byte count (half read, half written), same run, same rotation;
  one round trip          encode_video + quality of the seeded tiny / tiny tokenizer in bf16, and the VideoQuality it gives.

Reported, not gated.  GPU box only; writes what it prints to the file given as the first argument, if any
(profiles/video_quality.txt)."""
import ctypes as C
import os
import sys
import time
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from video_roundtrip import DEV, ITERS, LINES, OVERLAP, PATCH, SEQ, TILE, TOKENS, VIDEO, WARMUP, copy_yardstick, events, rotating, say  # noqa: E402

from titok_video_amd import _lib  # noqa: E402
from titok_video_amd import video as V  # noqa: E402
from titok_video_amd.model.titok import TiTok  # noqa: E402
from titok_video_amd.synthetic import seeded_titok_state  # noqa: E402


def rgb_frames():
    return torch.randint(0, 256, VIDEO + (3,), dtype=torch.uint8, device=DEV)


def nv12_frames():
    y = torch.randint(0, 256, VIDEO, dtype=torch.uint8, device=DEV)
    uv = torch.randint(0, 256, (VIDEO[0], VIDEO[1] // 2, VIDEO[2] // 2, 2), dtype=torch.uint8, device=DEV)
    return V.YUV420Frames(y, uv=uv)


def bench_kernels():
    lib, stream = _lib.lib(), _lib.stream_ptr(torch.device(DEV))
    n, H, W = VIDEO
    px = n * H * W

    def sse(kind):
        def make(_k):
            out = torch.empty((n, 3), dtype=torch.int64, device=DEV)
            if kind == "rgb":
                a, b = rgb_frames(), rgb_frames()
                return lambda: _lib.check(lib.ttv_video_frame_sse_u8(a.data_ptr(), b.data_ptr(), n, 1, H, W, out.data_ptr(), stream), "frame_sse")
            a, b = nv12_frames(), nv12_frames()
            ca, cb = a.c_frames(), b.c_frames()
            return lambda: (a, b, _lib.check(lib.ttv_video_frame_sse_yuv420(C.byref(ca), C.byref(cb), n, 1, H, W, out.data_ptr(), stream), "frame_sse_yuv"))
        return make

    def ssim(kind):
        def make(_k):
            out = torch.empty((n, 3), dtype=torch.float64, device=DEV)
            need = lib.ttv_video_frame_ssim_workspace_bytes(n, H, W, int(kind != "rgb"))
            work = torch.empty((need // 8,), dtype=torch.float64, device=DEV)
            if kind == "rgb":
                a, b = rgb_frames(), rgb_frames()
                return lambda: _lib.check(lib.ttv_video_frame_ssim_u8(a.data_ptr(), b.data_ptr(), n, 1, H, W, out.data_ptr(), work.data_ptr(), need,
                                                                      stream), "frame_ssim")
            a, b = nv12_frames(), nv12_frames()
            ca, cb = a.c_frames(), b.c_frames()
            return lambda: (a, b, _lib.check(lib.ttv_video_frame_ssim_yuv420(C.byref(ca), C.byref(cb), n, 1, H, W, out.data_ptr(), work.data_ptr(),
                                                                             need, stream), "frame_ssim_yuv"))
        return make

    for kind, nbytes in (("rgb", 2 * 3 * px), ("nv12", 2 * 3 * px // 2)):
        sets = max(2, -(-(2 * 256 * 2 ** 20) // nbytes))
        rows = []
        for what, maker in (("frame_sse", sse), ("frame_ssim", ssim)):
            fn = rotating(maker(kind), sets)
            rows.append((what, events(lambda: fn(True)), events(lambda: fn(False))))
            del fn
            torch.cuda.empty_cache()
        c_hbm, c_warm = copy_yardstick(nbytes, sets)
        torch.cuda.empty_cache()
        for what, hbm, warm in rows:
            say(f"  {what:10s} {kind:5s} {nbytes / 1e6:6.1f} MB compared: {hbm:7.1f} us = {nbytes / hbm / 1e3:6.0f} GB/s over {sets} sets, {warm:7.1f} us = "
                f"{nbytes / warm / 1e3:6.0f} GB/s on one   (copy / kernel: {c_hbm / hbm:.2f}, {c_warm / warm:.2f})")
        say(f"  {'copy_':10s} {kind:5s} {nbytes / 1e6:6.1f} MB moved:    {c_hbm:7.1f} us = {nbytes / c_hbm / 1e3:6.0f} GB/s over {sets} sets, {c_warm:7.1f} us = "
            f"{nbytes / c_warm / 1e3:6.0f} GB/s on one")


def round_trip():
    cfg = SimpleNamespace(tokenizer=SimpleNamespace(model=SimpleNamespace(patch_size=list(PATCH), fsq_levels=[7, 5, 5, 5, 5], encoder_size="tiny",
                                                                          decoder_size="tiny")))
    model = TiTok(cfg)
    model.load_state_dict(seeded_titok_state(0), strict=True)
    model = model.to(DEV, torch.bfloat16).eval()
    vt = V.VideoTokenizer(model, tile=TILE, overlap=OVERLAP, tokens_per_tile=TOKENS, seq_len=SEQ, dtype=torch.bfloat16, depth=2)
    g = torch.Generator(device=DEV).manual_seed(0)
    for kind in ("rgb", "nv12"):
        if kind == "rgb":
            frames = torch.randint(0, 256, VIDEO + (3,), dtype=torch.uint8, device=DEV, generator=g)
        else:
            frames = V.YUV420Frames(torch.randint(0, 256, VIDEO, dtype=torch.uint8, device=DEV, generator=g),
                                    uv=torch.randint(0, 256, (VIDEO[0], VIDEO[1] // 2, VIDEO[2] // 2, 2), dtype=torch.uint8, device=DEV, generator=g))
        tok = vt.encode_video(frames, fps=24.0)
        q = vt.quality(frames, tok)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        q = vt.quality(frames, tok)
        ms = (time.perf_counter() - t0) * 1e3
        fmt = lambda row: ", ".join(f"{c} {v:.3f}" for c, v in zip(q.components, row))      # noqa: E731
        say(f"  round trip {kind}: {tok.bits_per_pixel:.4f} bits per pixel of seeded noise; quality() {ms:.1f} ms for {len(q.sse)} frames; PSNR overall "
            f"{fmt(q.psnr_overall())} dB, pooled {q.psnr_pooled():.3f} dB; SSIM mean {fmt(q.ssim_mean())}; worst frame {q.worst_frame()} "
            f"({fmt(q.psnr()[q.worst_frame()])} dB)")


if __name__ == "__main__":
    say(f"device: {torch.cuda.get_device_name(0)}; video {VIDEO}; kernel times by HIP events over {ITERS} launches after {WARMUP}")
    bench_kernels()
    round_trip()
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(LINES) + "\n")
