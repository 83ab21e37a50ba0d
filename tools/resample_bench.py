#!/usr/bin/env python3
"""ttv_clip_resample_u8 timed: one config-#3-like batch (bf16, training geometry, clips drawn by data.sample_chunks until the 6144-row
budget is full) and 64 clips in one call, against the per-clip ttv_clip_from_u8 loop of the loader without `sampling=` on the same
OUTPUT shapes (which reads a third of the bytes: it resizes nothing).  Five warm-up calls, median of N (default 100) device-event
timings per figure.  GPU box only.    python tools/resample_bench.py"""
import os
import random
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from titok_video_amd import _lib  # noqa: E402
from titok_video_amd.data import ClipSampling, resample_geoms, sample_chunks  # noqa: E402

N = int(os.environ.get("N", "100"))
DEV = torch.device("cuda:0")
HBM_TBS = 6.3            # achievable HBM bandwidth of the part, the figure DESIGN.md uses


def draw_geoms(n_clips=None, seq_len=6144, seed=1):
    """Training geometries of decoded 160..288 x 200..384 sources at 24 fps, as the loader's workers draw them."""
    rng, s, out, rows = random.Random(seed), ClipSampling(), [], 0
    while True:
        src = (rng.randrange(96, 192), rng.randrange(160, 289), rng.randrange(200, 385))
        for ch in sample_chunks(rng, src, 24, s):
            t, ho, wo = ch["out"]
            rows += (t // 4) * (ho // 8) * (wo // 8) + 64
            if (n_clips is None and rows > seq_len) or (n_clips is not None and len(out) == n_clips):
                return out
            out.append(ch["geom"])


def median_ms(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(N):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench.py measures on the GPU; there is no CPU path")
    lib, stream = _lib.lib(), _lib.stream_ptr(DEV)
    for label, geoms in (("config-#3-like batch", draw_geoms()), ("64 clips", draw_geoms(64))):
        g = torch.Generator().manual_seed(0)
        srcs = [torch.randint(0, 256, (x[0], x[1], x[2], 3), generator=g, dtype=torch.uint8).to(DEV) for x in geoms]
        bytes_in = sum(s.numel() for s in srcs)
        bytes_out = sum(3 * x[0] * x[7] * x[8] * 2 for x in geoms)
        clips = resample_geoms(srcs, geoms, torch.bfloat16, stream)            # destinations allocated once, outside the timing
        flat = [int(v) for x in geoms for v in x]
        arr, sp, dp = (_lib.i32 * len(flat))(*flat), _lib.ptr_array(srcs), _lib.ptr_array(clips)

        def call():
            _lib.check(lib.ttv_clip_resample_u8(sp, dp, arr, len(geoms), _lib.TTV_BF16, stream), "ttv_clip_resample_u8")

        med, best = median_ms(call)
        print(f"{label}: {len(geoms)} clips, {bytes_in / 1e6:.2f} MB uint8 in, {bytes_out / 1e6:.2f} MB bf16 out")
        print(f"  ttv_clip_resample_u8, one call: median {1e3 * med:.1f} us (min {1e3 * best:.1f}) of {N}; "
              f"{(bytes_in + bytes_out) / med / 1e9:.3f} TB/s implied ({100 * (bytes_in + bytes_out) / med / 1e9 / HBM_TBS:.1f} % of {HBM_TBS} TB/s)")
        # the parent's path on the same output shapes: frames already on the lattice, one ttv_clip_from_u8 launch per clip
        flat8 = [torch.randint(0, 256, (x[0], x[7], x[8], 3), generator=g, dtype=torch.uint8).to(DEV) for x in geoms]
        b8 = sum(f.numel() for f in flat8)

        def loop():
            for f, c, x in zip(flat8, clips, geoms):
                _lib.check(lib.ttv_clip_from_u8(f.data_ptr(), x[0], x[7], x[8], c.data_ptr(), _lib.TTV_BF16, stream), "ttv_clip_from_u8")

        med8, best8 = median_ms(loop)
        print(f"  ttv_clip_from_u8, {len(geoms)} calls on the same outputs ({b8 / 1e6:.2f} MB in): median {1e3 * med8:.1f} us (min {1e3 * best8:.1f}); "
              f"{(b8 + bytes_out) / med8 / 1e9:.3f} TB/s implied")


if __name__ == "__main__":
    main()
