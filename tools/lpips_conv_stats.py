#!/usr/bin/env python3
"""Per-layer times of the LPIPS convolutions from a rocprofv3 --kernel-trace result (rocpd SQLite) of tools/lpips_bench.py:

    REPS=1 ITERS=5 rocprofv3 --kernel-trace --stats -d prof -o lpips -- python tools/lpips_bench.py
    python tools/lpips_conv_stats.py prof/lpips_results.db

Each step issues 24 k_conv_mfma dispatches (conv 2 .. 13 forward on 50 images, then their dgrads on 25, last layer first); the
median of each slot over the steps, its algorithmic GFLOP and the fraction of the 2.5 PFLOP/s bf16 peak are printed, then the
per-step totals of the other HIP kernels of the path."""
import sqlite3
import statistics
import sys
from collections import defaultdict

CIN = [3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512]
COUT = [64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512]
STAGE = [0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4]
SIZE, N_FWD, N_BWD, PEAK = 128, 50, 25, 2.5e15


def main():
    rows = list(sqlite3.connect(sys.argv[1]).execute("select name, duration from kernels order by start"))
    conv = [d for n, d in rows if "k_conv_mfma" in n]
    steps = len(conv) // 24
    tot_t = tot_f = 0.0
    for s in range(24):
        us = statistics.median(conv[s::24][:steps]) / 1e3
        if s < 12:
            l, n, kind, ci, co = s + 1, N_FWD, "fwd", CIN[s + 1], COUT[s + 1]
        else:
            l = 12 - (s - 12)
            n, kind, ci, co = N_BWD, "dgrad", COUT[l], CIN[l]
        f = 2 * 9 * ci * co * (SIZE >> STAGE[l]) ** 2 * n
        tot_t, tot_f = tot_t + us, tot_f + f
        print(f"{kind:5s} conv{l + 1:<2d} {ci:3d}->{co:3d} {SIZE >> STAGE[l]:3d}^2  {us:7.1f} us  {f / 1e9:5.1f} GFLOP  {f / (us * 1e-6) / PEAK:.3f} of peak")
    print(f"all k_conv_mfma: {tot_t:.1f} us, {tot_f / 1e9:.1f} GFLOP, {tot_f / (tot_t * 1e-6) / PEAK:.3f} of peak")
    other = defaultdict(float)
    for n, d in rows:
        for k in ("k_conv_first", "k_conv_last", "k_conv_splitk", "k_head_fwd", "k_head_bwd", "k_route", "k_pool", "k_head_finish"):
            if k in n:
                other[k] += d / 1e3 / steps
    for k, v in sorted(other.items(), key=lambda kv: -kv[1]):
        print(f"{k:14s} {v:7.1f} us per step")


if __name__ == "__main__":
    main()
