#!/usr/bin/env python3
"""The L2 quantiser's training forward + backward with the commitment term and the EMA codebook (commitment_weight 0.25,
codebook_update "ema", dead_code_threshold 1) against the same call with the defaults (the straight-through lookup and `_LookupFn`'s
scatter-add backward), and each new C entry on its own: microseconds per call, the bytes it has to move and the rate that implies.

Device events on one stream; every shape is warmed up; the two module variants alternate in windows of REPS calls and the median
window is reported with the spread; the shader clock the driver reports is printed before and after.  The launches are
latency-bound (tens of MB at most): the rates say how far from a memory bound they are, not how good the kernels are.  GPU box only.

    python tools/bench_vq_train.py            # REPS=200 WINDOWS=7"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from titok_video_amd import _lib  # noqa: E402
from titok_video_amd.model.quantizer.vq_l2 import L2Quantizer  # noqa: E402

DEV = "cuda:0"
REPS, WINDOWS = int(os.environ.get("REPS", "200")), int(os.environ.get("WINDOWS", "7"))
SHAPES = [(4096, 8192, 32), (32768, 16384, 64)]          # rows, N, C (bf16)
DT = torch.bfloat16


def clock():
    try:
        return f"{torch.cuda.clock_rate()} MHz"
    except Exception as e:      # the driver query is optional
        return f"unavailable ({type(e).__name__})"


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def timed(fns, reps=REPS, windows=WINDOWS):
    """{name: (median us, min, max)} with the variants alternating window by window."""
    for fn in fns.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            got[k].append(window(fn, reps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}


def step_of(vq, z, g):
    def step():
        zz = z.detach().requires_grad_(True)
        codes, _ = vq(zz)
        codes.backward(g)
    return step


def main():
    print(f"device {torch.cuda.get_device_name(0)}; shader clock before: {clock()}; REPS {REPS}, WINDOWS {WINDOWS} (median [min .. max] us per call)")
    lib = _lib.lib()
    for rows, n, c in SHAPES:
        gen = torch.Generator().manual_seed(0)
        cb = torch.randn(n, c, generator=gen)
        z = torch.randn(rows, c, generator=gen).to(DEV, DT)
        g = torch.randn(rows, c, generator=gen).to(DEV, DT)
        new = L2Quantizer(cb, commitment_weight=0.25, codebook_update="ema", dead_code_threshold=1.0).to(DEV).train()
        old = L2Quantizer(cb).to(DEV).train()
        res = timed({"defaults": step_of(old, z, g), "commit + ema": step_of(new, z, g), "argmin alone": lambda: old.indices(z)})
        print(f"\nrows {rows} x codebook {n} x {c} bf16: quantiser training forward + backward")
        for k, (med, lo, hi) in res.items():
            print(f"  {k:14s} {med:9.1f} [{lo:8.1f} .. {hi:8.1f}]")
        d = res["commit + ema"][0] - res["defaults"][0]
        print(f"  commit + ema over defaults: {d:+.1f} us per step")
        # ---- the C entries one by one, on this shape's own indices and with every row on one entry (the longest chain)
        # and on the 32 entries of one block (that block's waves walk its list once per entry)
        esz = 2
        idx = old.indices(z)
        one = torch.full_like(idx, n // 3)
        blk = (n // 3 // 32 * 32 + torch.arange(rows, device=DEV) % 32).to(torch.int32)     # every row on the 32 entries of ONE block, spread over them
        cbd, norms = new._cb(DT)
        ws, nbytes = new._workspace(rows, n, DEV)
        loss = torch.zeros(1, device=DEV)
        stats = torch.empty(n * (2 * c + 1), device=DEV)
        e, dz = old.lookup(idx, DT), torch.empty_like(z)
        s, code = _lib.stream_ptr(DEV), _lib.dtype_code(DT)
        mod = new

        def stats_call(ix):
            return lambda: _lib.check(lib.ttv_vq_ema_stats(z.data_ptr(), code, c, ix.data_ptr(), rows, n, c, mod.cluster_size.data_ptr(), 1.0, 0,
                                                           mod.ema_step.data_ptr(), 0, 1, stats.data_ptr(), ws.data_ptr(), nbytes, s), "stats")
        calls = {
            "commit_forward": lambda: _lib.check(lib.ttv_vq_commit_forward(z.data_ptr(), code, c, cbd.data_ptr(), c, idx.data_ptr(), rows, n, c,
                                                                          loss.data_ptr(), ws.data_ptr(), nbytes, s), "commit_forward"),
            "commit_backward": lambda: _lib.check(lib.ttv_vq_commit_backward(g.data_ptr(), c, z.data_ptr(), c, e.data_ptr(), c, code, rows, c, 1e-6,
                                                                            dz.data_ptr(), c, s), "commit_backward"),
            "ema_stats": stats_call(idx),
            "ema_stats one": stats_call(one),
            "ema_stats block": stats_call(blk),
            "ema_update": lambda: _lib.check(lib.ttv_vq_ema_update(stats.data_ptr(), mod.cluster_size.data_ptr(), mod.embed_avg.data_ptr(),
                                                                  mod.codebook.data_ptr(), cbd.data_ptr(), code, norms.data_ptr(), mod.ema_step.data_ptr(),
                                                                  n, c, 0.99, 0.01, 1e-5, 1.0, ws.data_ptr(), nbytes, s), "ema_update"),
        }
        nb = -(-n // 32)
        moved = {       # bytes the call has to move through memory once (the statistics' index scans are listed apart: they stay in L2)
            "commit_forward": 2 * rows * c * esz + rows * 4,
            "commit_backward": 4 * rows * c * esz,
            "ema_stats": rows * 4 + rows * c * esz + n * (2 * c + 1) * 4 + 2 * 3 * rows * 4,
            "ema_stats one": rows * 4 + rows * c * esz + n * (2 * c + 1) * 4 + 2 * 3 * rows * 4,
            "ema_stats block": rows * 4 + rows * c * esz + n * (2 * c + 1) * 4 + 2 * 3 * rows * 4,
            "ema_update": n * (2 * c + 1) * 4 + n * 4 + n * c * 4 + 2 * n * c * 4 + n * c * esz + 2 * n * 4,
        }
        res = timed(calls)
        print("  per C entry (launches: commit_forward 2, commit_backward 1, ema_stats 1, ema_update 2)")
        for k, (med, lo, hi) in res.items():
            print(f"  {k:16s} {med:9.1f} [{lo:8.1f} .. {hi:8.1f}]  {moved[k] / 1e6:7.2f} MB  {moved[k] / med / 1e6:7.3f} TB/s")
        print(f"  ema_stats also scans the index vector twice per block: {nb} blocks x {2 * rows * 4 / 1e3:.0f} KB = {nb * 2 * rows * 4 / 1e6:.1f} MB from L2")
    print(f"\nshader clock after: {clock()}")


if __name__ == "__main__":
    main()
