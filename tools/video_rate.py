#!/usr/bin/env python3
"""Measured distortion on the whole-video path (titok_video_amd/video.py) on one GPU: tools/video_roundtrip.py's video, tiles and
seeded tiny / tiny tokenizer in bf16.

  tile_sse        ttv_video_tile_sse_u8 over all tiles, one launch (and the clearing of its sums), by HIP events: us and GB/s over the
                  bytes the kernel asks for (3 bytes and 3 elements read per tile pixel, 8 bytes written per tile), rotating over
                  working sets that together exceed twice the 256 MiB Infinity Cache (an HBM rate) and on one set (cache-warm), in
                  both dtypes;
  the yardstick   a device-to-device copy_ that moves the same byte count (half read, half written), in the same run, same rotation;
  the probe       rate_distortion over the default ladder of 128 tokens per tile (16, 32, 64, 128), host clock around work that ends
                  in a synchronise, beside one encode_video + decode_video at 128 tokens per tile in the same run, and encode_video
                  with a budget (the probe plus the allocator).

Reported, not gated.  GPU box only; writes what it prints to the file given as the first argument, if any."""
import ctypes as C
import os
import sys
import time
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_roundtrip import DEV, ITERS, LINES, OVERLAP, PATCH, SEQ, TILE, TOKENS, TRIPS, VIDEO, WARMUP, copy_yardstick, events, rotating, say  # noqa: E402

from titok_video_amd import _lib  # noqa: E402
from titok_video_amd import video as V  # noqa: E402
from titok_video_amd.model.titok import TiTok  # noqa: E402
from titok_video_amd.synthetic import seeded_titok_state  # noqa: E402


def bench_kernel(dtype):
    plan = V.TilePlan(VIDEO, TILE, OVERLAP, PATCH)
    esz = torch.empty(0, dtype=dtype).element_size()
    tile_px = plan.n_tiles * plan.tile[0] * plan.tile[1] * plan.tile[2]
    video_px = VIDEO[0] * VIDEO[1] * VIDEO[2]
    lib, stream, code, cp = _lib.lib(), _lib.stream_ptr(torch.device(DEV)), _lib.dtype_code(dtype), plan.c_plan()
    name = "bf16" if dtype == torch.bfloat16 else "fp32"
    say(f"{plan!r}: {plan.n_tiles} tiles, cover ratio {tile_px / video_px:.2f}, {name}")
    nbytes = tile_px * 3 * (1 + esz) + 8 * plan.n_tiles
    sets = max(2, -(-(2 * 256 * 2 ** 20) // (video_px * 3 + tile_px * 3 * esz)))

    def make(k):
        frames = torch.randint(0, 256, VIDEO + (3,), dtype=torch.uint8, device=DEV)
        tiles = (torch.rand((plan.n_tiles, 3) + plan.tile, device=DEV) * 2.4 - 1.2).to(dtype)
        ptrs = [t.data_ptr() for t in tiles.unbind(0)]
        host, table = (C.c_void_p * len(ptrs))(*ptrs), torch.tensor(ptrs, dtype=torch.int64).to(DEV)
        out = torch.empty(plan.n_tiles, dtype=torch.int64, device=DEV)
        return lambda: (tiles, _lib.check(lib.ttv_video_tile_sse_u8(frames.data_ptr(), C.byref(cp), 0, plan.n_tiles, host, table.data_ptr(), code,
                                                                    out.data_ptr(), stream), "tile_sse"))
    fn = rotating(make, sets)
    hbm, warm = events(lambda: fn(True)), events(lambda: fn(False))
    c_hbm, c_warm = copy_yardstick(nbytes, sets)
    say(f"  tile_sse {nbytes / 1e6:6.1f} MB asked for ({video_px * 3 / 1e6:.1f} MB of video, each byte read {tile_px / video_px:.2f}x; {tile_px * 3 * esz / 1e6:.1f} MB "
        f"of tiles read): {hbm:7.1f} us = {nbytes / hbm / 1e3:6.0f} GB/s over {sets} sets, {warm:7.1f} us = {nbytes / warm / 1e3:6.0f} GB/s on one")
    say(f"          copy_ of the same byte count:{'':47s} {c_hbm:7.1f} us = {nbytes / c_hbm / 1e3:6.0f} GB/s over {sets} sets, {c_warm:7.1f} us = "
        f"{nbytes / c_warm / 1e3:6.0f} GB/s on one   (tile_sse / copy: {c_hbm / hbm:.2f}, {c_warm / warm:.2f})")
    sums = torch.empty(plan.n_tiles, dtype=torch.int64, device=DEV)
    fill = events(lambda: sums.zero_())
    say(f"          a call is two launches, the clearing of its {8 * plan.n_tiles} bytes of sums and the kernel; a fill of as many bytes alone "
        f"(torch's zero_), launch after launch: {fill:5.1f} us")
    del fn
    torch.cuda.empty_cache()
    return warm


def clock(fn, trips=TRIPS):
    for _ in range(2):
        out = fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(trips):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / trips, out


def bench_probe(sse_us):
    cfg = SimpleNamespace(tokenizer=SimpleNamespace(model=SimpleNamespace(patch_size=list(PATCH), fsq_levels=[7, 5, 5, 5, 5], encoder_size="tiny",
                                                                          decoder_size="tiny")))
    model = TiTok(cfg)
    model.load_state_dict(seeded_titok_state(0), strict=True)
    model = model.to(DEV, torch.bfloat16).eval()
    frames = torch.randint(0, 256, VIDEO + (3,), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(DEV)
    ladder = V.default_ladder(TOKENS)
    for depth in (1, 2):
        vt = V.VideoTokenizer(model, tile=TILE, overlap=OVERLAP, tokens_per_tile=TOKENS, seq_len=SEQ, dtype=torch.bfloat16, depth=depth)
        enc, tok = clock(lambda: vt.encode_video(frames, fps=24.0))
        dec, _ = clock(lambda: vt.decode_video(tok))
        probe, table = clock(lambda: vt.rate_distortion(frames, ladder))
        budget = table.n_tiles * ladder[-1] // 2
        alloc, picked = clock(lambda: vt.encode_video(frames, fps=24.0, total_tokens=budget))
        say(f"  depth {depth}: rate_distortion over {ladder} {probe / 1e3:7.2f} ms ({len(ladder)} forward passes of {table.n_tiles} tiles); encode_video "
            f"{enc / 1e3:7.2f} ms + decode_video {dec / 1e3:7.2f} ms = {(enc + dec) / 1e3:7.2f} ms at {TOKENS} tokens per tile (probe / round trip "
            f"{probe / (enc + dec):.2f}); its {len(ladder)} x {sse_us:.0f} us of tile_sse (cache-warm) are {100 * len(ladder) * sse_us / probe:.2f} % of the probe")
        say(f"           encode_video(total_tokens={budget}) {alloc / 1e3:7.2f} ms: {sum(picked.counts)} tokens over counts "
            f"{sorted(set(picked.counts))}, {picked.bits_per_pixel:.4f} bits per pixel (uniform {TOKENS}: {tok.bits_per_pixel:.4f})")


if __name__ == "__main__":
    say(f"device: {torch.cuda.get_device_name(0)}; kernel times by HIP events over {ITERS} launches after {WARMUP}; host-clocked runs over {TRIPS} after 2")
    bench_kernel(torch.float32)
    bench_probe(bench_kernel(torch.bfloat16))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(LINES) + "\n")
