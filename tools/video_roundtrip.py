#!/usr/bin/env python3
"""The whole-video path (titok_video_amd/video.py) on one GPU: a 64 x 256 x 256 video, tile 16 x 128 x 128, overlap 4 x 16 x 16,
seeded tiny / tiny tokenizer in bf16, 128 tokens per tile.

  gather, blend   ttv_video_tiles_u8 over all tiles and ttv_video_blend_u8 over the whole timeline, one launch each, by HIP events:
                  us and GB/s over the bytes the kernel asks for (gather: 3 bytes read and 3 elements written per tile pixel; blend:
                  3 elements read per tile pixel and 3 bytes written per pixel of the timeline), rotating over working sets that
                  together exceed twice the 256 MiB Infinity Cache (an HBM rate) and on one set (cache-warm);
  the yardstick   a device-to-device copy_ that moves the same byte count (half read, half written), in the same run, same rotation;
  the round trip  encode_video + decode_video, host clock around work that ends in a synchronise, and the two kernels' share of it.

With --yuv as the first argument: the three Y'CbCr 4:2:0 entry points (ttv_video_tiles_yuv420, ttv_video_blend_yuv420,
ttv_video_tile_sse_yuv420; NV12, BT.709 limited range, left-sited and centred chroma) beside their three RGB siblings and a copy_ of the
YUV kernel's byte count, all in the same run, from HBM and cache-warm (profiles/video_yuv.txt).

Reported, not gated.  GPU box only; writes what it prints to the file given as the first argument (after --yuv), if any."""
import ctypes as C
import os
import sys
import time
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from titok_video_amd import _lib  # noqa: E402
from titok_video_amd import video as V  # noqa: E402
from titok_video_amd.model.titok import TiTok  # noqa: E402
from titok_video_amd.synthetic import seeded_titok_state  # noqa: E402

DEV = "cuda:0"
VIDEO, TILE, OVERLAP, PATCH, TOKENS, SEQ = (64, 256, 256), (16, 128, 128), (4, 16, 16), (4, 8, 8), 128, 6144
WARMUP, ITERS, TRIPS = 3, 40, 5
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def events(fn, iters=ITERS):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def rotating(make, sets):
    """fn(rotate) over `sets` independent working sets built by make(k)."""
    work, turn = [make(k) for k in range(sets)], [0]

    def fn(rotate):
        w = work[turn[0] % sets if rotate else 0]
        turn[0] += 1
        w()
    return fn


def copy_yardstick(nbytes, sets):
    def make(_k):
        src = torch.randint(0, 256, (nbytes // 2,), dtype=torch.uint8, device=DEV)
        dst = torch.empty_like(src)
        return lambda: dst.copy_(src)
    fn = rotating(make, sets)
    return events(lambda: fn(True)), events(lambda: fn(False))


def bench_kernels(dtype):
    plan = V.TilePlan(VIDEO, TILE, OVERLAP, PATCH)
    esz = torch.empty(0, dtype=dtype).element_size()
    tile_px = plan.n_tiles * plan.tile[0] * plan.tile[1] * plan.tile[2]
    video_px = VIDEO[0] * VIDEO[1] * VIDEO[2]
    lib, stream, code, cp = _lib.lib(), _lib.stream_ptr(torch.device(DEV)), _lib.dtype_code(dtype), plan.c_plan()
    name = "bf16" if dtype == torch.bfloat16 else "fp32"
    say(f"{plan!r}: {plan.n_tiles} tiles, cover ratio {tile_px / video_px:.2f}, {name}")

    g_bytes = tile_px * 3 * (1 + esz)
    sets = max(2, -(-(2 * 256 * 2 ** 20) // (video_px * 3 + tile_px * 3 * esz)))

    def make_gather(k):
        frames = torch.randint(0, 256, VIDEO + (3,), dtype=torch.uint8, device=DEV)
        out = torch.empty((plan.n_tiles, 3) + plan.tile, dtype=dtype, device=DEV)
        return lambda: _lib.check(lib.ttv_video_tiles_u8(frames.data_ptr(), C.byref(cp), 0, plan.n_tiles, out.data_ptr(), code, stream), "tiles")
    fn = rotating(make_gather, sets)
    hbm, warm = events(lambda: fn(True)), events(lambda: fn(False))
    c_hbm, c_warm = copy_yardstick(g_bytes, sets)
    say(f"  gather  {g_bytes / 1e6:7.1f} MB asked for ({video_px * 3 / 1e6:.1f} MB of video, each byte read {tile_px / video_px:.2f}x; {tile_px * 3 * esz / 1e6:.1f} MB "
        f"written): {hbm:7.1f} us = {g_bytes / hbm / 1e3:6.0f} GB/s over {sets} sets, {warm:7.1f} us = {g_bytes / warm / 1e3:6.0f} GB/s on one")
    say(f"          copy_ of the same byte count:{'':47s} {c_hbm:7.1f} us = {g_bytes / c_hbm / 1e3:6.0f} GB/s over {sets} sets, {c_warm:7.1f} us = "
        f"{g_bytes / c_warm / 1e3:6.0f} GB/s on one   (gather / copy: {c_hbm / hbm:.2f}, {c_warm / warm:.2f})")
    del fn
    torch.cuda.empty_cache()

    b_bytes = tile_px * 3 * esz + video_px * 3

    def make_blend(k):
        tiles = (torch.rand((plan.n_tiles, 3) + plan.tile, device=DEV) * 2.4 - 1.2).to(dtype)
        ptrs = [t.data_ptr() for t in tiles.unbind(0)]
        host, table = (C.c_void_p * len(ptrs))(*ptrs), torch.tensor(ptrs, dtype=torch.int64).to(DEV)
        out = torch.empty(VIDEO + (3,), dtype=torch.uint8, device=DEV)
        return lambda: (tiles, _lib.check(lib.ttv_video_blend_u8(host, table.data_ptr(), C.byref(cp), 0, VIDEO[0], code, out.data_ptr(), stream), "blend"))
    fn = rotating(make_blend, sets)
    hbm_b, warm_b = events(lambda: fn(True)), events(lambda: fn(False))
    c_hbm, c_warm = copy_yardstick(b_bytes, sets)
    say(f"  blend   {b_bytes / 1e6:7.1f} MB asked for ({tile_px * 3 * esz / 1e6:.1f} MB of tiles read, {video_px * 3 / 1e6:.1f} MB of frames written): "
        f"{hbm_b:7.1f} us = {b_bytes / hbm_b / 1e3:6.0f} GB/s over {sets} sets, {warm_b:7.1f} us = {b_bytes / warm_b / 1e3:6.0f} GB/s on one")
    say(f"          copy_ of the same byte count:{'':47s} {c_hbm:7.1f} us = {b_bytes / c_hbm / 1e3:6.0f} GB/s over {sets} sets, {c_warm:7.1f} us = "
        f"{b_bytes / c_warm / 1e3:6.0f} GB/s on one   (blend / copy: {c_hbm / hbm_b:.2f}, {c_warm / warm_b:.2f})")
    del fn
    torch.cuda.empty_cache()
    return warm, warm_b


def bench_round_trip(gather_us, blend_us):
    cfg = SimpleNamespace(tokenizer=SimpleNamespace(model=SimpleNamespace(patch_size=list(PATCH), fsq_levels=[7, 5, 5, 5, 5], encoder_size="tiny",
                                                                          decoder_size="tiny")))
    model = TiTok(cfg)
    model.load_state_dict(seeded_titok_state(0), strict=True)
    model = model.to(DEV, torch.bfloat16).eval()
    frames = torch.randint(0, 256, VIDEO + (3,), dtype=torch.uint8, device=DEV)
    for depth in (1, 2):
        vt = V.VideoTokenizer(model, tile=TILE, overlap=OVERLAP, tokens_per_tile=TOKENS, seq_len=SEQ, dtype=torch.bfloat16, depth=depth)
        times = {}
        for what, fn in (("encode_video", lambda: vt.encode_video(frames, fps=24.0)), ("decode_video", lambda: vt.decode_video(tok))):
            for _ in range(2):
                out = fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(TRIPS):
                out = fn()
            torch.cuda.synchronize()
            times[what] = (time.perf_counter() - t0) * 1e6 / TRIPS
            if what == "encode_video":
                tok = out
        total = times["encode_video"] + times["decode_video"]
        say(f"  round trip, depth {depth}: encode_video {times['encode_video'] / 1e3:7.2f} ms, decode_video {times['decode_video'] / 1e3:7.2f} ms "
            f"({VIDEO[0] * 1e6 / total:.0f} frames/s, {tok.bits_per_pixel:.4f} bits per pixel); the two kernels' {gather_us + blend_us:.0f} us "
            f"(one launch each, cache-warm) are {100 * (gather_us + blend_us) / total:.2f} % of it")


def bench_yuv(dtype):
    """gather, blend and tile_sse: YUV (both sitings) and RGB, and a copy_ of the YUV kernel's byte count, same run and rotation."""
    plan = V.TilePlan(VIDEO, TILE, OVERLAP, PATCH)
    esz = torch.empty(0, dtype=dtype).element_size()
    tile_px = plan.n_tiles * plan.tile[0] * plan.tile[1] * plan.tile[2]
    video_px = VIDEO[0] * VIDEO[1] * VIDEO[2]
    lib, stream, code, cp = _lib.lib(), _lib.stream_ptr(torch.device(DEV)), _lib.dtype_code(dtype), plan.c_plan()
    name = "bf16" if dtype == torch.bfloat16 else "fp32"
    sets = max(2, -(-(2 * 256 * 2 ** 20) // (video_px * 3 // 2 + tile_px * 3 * esz)))
    say(f"{plan!r}: {plan.n_tiles} tiles, cover ratio {tile_px / video_px:.2f}, {name}, {sets} working sets")

    def yuv_frames(siting, _fill):
        y = torch.randint(0, 256, VIDEO, dtype=torch.uint8, device=DEV)
        uv = torch.randint(0, 256, (VIDEO[0], VIDEO[1] // 2, VIDEO[2] // 2, 2), dtype=torch.uint8, device=DEV)
        return V.YUV420Frames(y, uv=uv, siting=siting)

    def tiles_and_table():
        tiles = (torch.rand((plan.n_tiles, 3) + plan.tile, device=DEV) * 2.4 - 1.2).to(dtype)
        ptrs = [t.data_ptr() for t in tiles.unbind(0)]
        return tiles, (C.c_void_p * len(ptrs))(*ptrs), torch.tensor(ptrs, dtype=torch.int64).to(DEV)

    def gather(siting):
        def make(_k):
            out = torch.empty((plan.n_tiles, 3) + plan.tile, dtype=dtype, device=DEV)
            if siting is None:
                frames = torch.randint(0, 256, VIDEO + (3,), dtype=torch.uint8, device=DEV)
                return lambda: _lib.check(lib.ttv_video_tiles_u8(frames.data_ptr(), C.byref(cp), 0, plan.n_tiles, out.data_ptr(), code, stream), "tiles")
            f = yuv_frames(siting, True)
            cf = f.c_frames()
            return lambda: (f, _lib.check(lib.ttv_video_tiles_yuv420(C.byref(cf), C.byref(cp), 0, plan.n_tiles, out.data_ptr(), code, stream), "tiles_yuv"))
        return make

    def blend(siting):
        def make(_k):
            tiles, host, table = tiles_and_table()
            if siting is None:
                out = torch.empty(VIDEO + (3,), dtype=torch.uint8, device=DEV)
                return lambda: (tiles, _lib.check(lib.ttv_video_blend_u8(host, table.data_ptr(), C.byref(cp), 0, VIDEO[0], code, out.data_ptr(), stream), "blend"))
            f = yuv_frames(siting, False)
            cf = f.c_frames()
            return lambda: (tiles, f, _lib.check(lib.ttv_video_blend_yuv420(host, table.data_ptr(), C.byref(cp), 0, VIDEO[0], code, C.byref(cf), stream), "blend_yuv"))
        return make

    def sse(siting):
        def make(_k):
            tiles, host, table = tiles_and_table()
            out = torch.empty((plan.n_tiles,), dtype=torch.int64, device=DEV)
            if siting is None:
                frames = torch.randint(0, 256, VIDEO + (3,), dtype=torch.uint8, device=DEV)
                return lambda: (tiles, _lib.check(lib.ttv_video_tile_sse_u8(frames.data_ptr(), C.byref(cp), 0, plan.n_tiles, host, table.data_ptr(), code,
                                                                            out.data_ptr(), stream), "sse"))
            f = yuv_frames(siting, True)
            cf = f.c_frames()
            return lambda: (tiles, f, _lib.check(lib.ttv_video_tile_sse_yuv420(C.byref(cf), C.byref(cp), 0, plan.n_tiles, host, table.data_ptr(), code,
                                                                               out.data_ptr(), stream), "sse_yuv"))
        return make

    tile_bytes = tile_px * 3 * esz
    for what, maker, yuv_bytes, rgb_bytes in (("gather", gather, tile_px * 3 // 2 + tile_bytes, tile_px * 3 + tile_bytes),
                                              ("blend", blend, tile_bytes + video_px * 3 // 2, tile_bytes + video_px * 3),
                                              ("tile_sse", sse, tile_px * 3 // 2 + tile_bytes, tile_px * 3 + tile_bytes)):
        rows = []
        for label, siting, nbytes in (("yuv420 left", "left", yuv_bytes), ("yuv420 center", "center", yuv_bytes), ("rgb", None, rgb_bytes)):
            fn = rotating(maker(siting), sets)
            rows.append((label, nbytes, events(lambda: fn(True)), events(lambda: fn(False))))
            del fn
            torch.cuda.empty_cache()
        c_hbm, c_warm = copy_yardstick(yuv_bytes, sets)
        for label, nbytes, hbm, warm in rows:
            say(f"  {what:8s} {label:13s} {nbytes / 1e6:7.1f} MB asked for: {hbm:7.1f} us = {nbytes / hbm / 1e3:6.0f} GB/s from HBM, {warm:7.1f} us = "
                f"{nbytes / warm / 1e3:6.0f} GB/s cache-warm")
        say(f"  {what:8s} {'copy_':13s} {yuv_bytes / 1e6:7.1f} MB moved:     {c_hbm:7.1f} us = {yuv_bytes / c_hbm / 1e3:6.0f} GB/s from HBM, {c_warm:7.1f} us = "
            f"{yuv_bytes / c_warm / 1e3:6.0f} GB/s cache-warm")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--yuv":
        say(f"device: {torch.cuda.get_device_name(0)}; kernel times by HIP events over {ITERS} launches after {WARMUP}")
        bench_yuv(torch.float32)
        bench_yuv(torch.bfloat16)
        if len(sys.argv) > 2:
            os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
            with open(sys.argv[2], "w") as f:
                f.write("\n".join(LINES) + "\n")
        sys.exit(0)
    say(f"device: {torch.cuda.get_device_name(0)}; kernel times by HIP events over {ITERS} launches after {WARMUP}; round trips over {TRIPS} after 2")
    bench_kernels(torch.float32)
    g, b = bench_kernels(torch.bfloat16)
    bench_round_trip(g, b)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(LINES) + "\n")
