"""Host time of one batch plan + its ttv_batch, by both builders in one process on the same batches: BatchPlan (numpy) and the
library's plan (TTV_NATIVE_PLAN=1: NativeBatchPlan).  The batches are the seeded ragged ones of tests/probes/plan_host_probe.py
(4-7 clips of its six shapes, K in {32, 64, 128}); every plan is new, as for a loader that never repeats a batch shape.

DEVICE=cuda:0 (default): the whole call, uploads and launches included (host time: nothing waits for the GPU except BatchPlan's own
copy-stream wait).  DEVICE=cpu: BatchPlan on the host, and of the library the host-only calls (ttv_plan_rows_sizes / _fill,
ttv_plan_attn_sizes / _fill) - what runs on a machine without a GPU.  REPEAT=n passes over the 200 batches (default 3, best pass)."""
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from titok_video_amd import plan as P  # noqa: E402

PATCH = (4, 8, 8)
random.seed(0)
shapes = [(16, 128, 128), (8, 64, 96), (16, 64, 64), (4, 128, 96), (12, 96, 128), (16, 96, 96)]


def make():
    n = random.randint(4, 7)
    return [random.choice(shapes) for _ in range(n)], [random.choice([32, 64, 128]) for _ in range(n)]


batches = [make() for _ in range(200)]
dev = torch.device(os.environ.get("DEVICE", "cuda:0"))
repeat = int(os.environ.get("REPEAT", "3"))


def python_plan(g, c):
    P.BatchPlan(g, c, PATCH, dev).batch_for(4, 2)


def native_plan(g, c):
    if dev.type == "cuda":
        P.NativeBatchPlan(g, c, PATCH, dev).batch_for(4, 2)
    else:
        P.native_host_tables(g, c, PATCH, 4, 2)


def ms_per_plan(fn):
    best = float("inf")
    for _ in range(repeat):
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for g, c in batches:
            fn(g, c)
        best = min(best, (time.perf_counter() - t0) / len(batches) * 1e3)
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
    return best


for g, c in batches[:8]:        # warm-up: library load, rotary base tables, pinned staging
    python_plan(g, c)
    native_plan(g, c)
py, nat = ms_per_plan(python_plan), ms_per_plan(native_plan)
what = "plan + batch_for" if dev.type == "cuda" else "plan + batch_for (BatchPlan on the host; library: host-only calls)"
print(f"{dev}: per {what}: BatchPlan {py:.3f} ms | library {nat:.3f} ms | ratio {py / nat:.1f}x")
