#!/usr/bin/env python3
"""EvalMetrics(['ssim']).update on 32 clips of 3 x 16 x 128 x 128 (the benchmark batch): µs per update (HIP events around a
window of updates, after a warm-up), and the bytes of both inputs over that time as a fraction of the HBM peak; the same for the
two launches of ttv_ssim_accumulate alone (host arrays built once), which leaves out the per-clip host work of update().  The
index costs about 130 FLOP per output element, so the update is bound by memory and latency, not by arithmetic.  GPU box only."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from titok_video_amd import _lib  # noqa: E402
from titok_video_amd.model.metrics.eval_metrics import EvalMetrics  # noqa: E402

DEV = "cuda:0"
HBM_PEAK = 8.0e12      # bytes/s, spec (MI355X); a float4 copy reaches about 6.3e12
SHAPE, CLIPS, WARMUP, ITERS = (3, 16, 128, 128), 32, 5, 50


def timed(fn):
    """µs per call of fn over ITERS calls after WARMUP, HIP events on the current stream."""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / ITERS


for dtype in (torch.bfloat16, torch.float32):
    g = torch.Generator(device=DEV).manual_seed(0)
    target = [(torch.rand(SHAPE, generator=g, device=DEV) * 2 - 1).to(dtype) for _ in range(CLIPS)]
    recon = [(t.float() + 0.1 * torch.randn(SHAPE, generator=g, device=DEV)).to(dtype) for t in target]
    m = EvalMetrics(SimpleNamespace(training=SimpleNamespace(eval=SimpleNamespace(log_metrics=["ssim"]))))
    us_update = timed(lambda: m.update(recon, target))
    rp, tp = _lib.ptr_array(recon), _lib.ptr_array(target)
    dims = (C.c_int32 * (4 * CLIPS))(*(list(SHAPE) * CLIPS))
    ws = torch.empty(_lib.lib().ttv_ssim_workspace_bytes(dims, CLIPS), dtype=torch.uint8, device=DEV)
    acc = torch.zeros(2, dtype=torch.float64, device=DEV)
    stream = _lib.stream_ptr(torch.device(DEV))
    us_launch = timed(lambda: _lib.check(_lib.lib().ttv_ssim_accumulate(rp, tp, dims, CLIPS, _lib.dtype_code(dtype), 1, acc.data_ptr(),
                                                                         ws.data_ptr(), ws.numel(), stream), "ttv_ssim_accumulate"))
    nbytes = 2 * sum(t.numel() * t.element_size() for t in target)
    m.reset()
    m.update(recon, target)
    val = m.compute()["eval/ssim"]
    for what, us in (("update()", us_update), ("launches", us_launch)):
        print(f"ssim {what:9s} {CLIPS} x {SHAPE} {str(dtype):15s} {us:8.1f} us  {nbytes / 1e6:6.1f} MB  {nbytes / us / 1e6:6.2f} TB/s = "
              f"{nbytes / us / 1e6 / (HBM_PEAK / 1e12):.3f} of HBM peak  (ssim {val:.6f})", flush=True)
