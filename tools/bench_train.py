#!/usr/bin/env python3
"""Training-step timing at the benchmark shape (32 x 16x128x128 clips, K=128, bf16): forward (tape) + L1 + backward + AdamW.
B= batch (5 = the reference's 6144-token budget), GRAPH=1: the whole step captured once in a HIP graph (torch.cuda.CUDAGraph) and
replayed - the step is a fixed launch sequence for a fixed batch shape, and at small batches the host cannot issue ~280 launches
as fast as the GPU runs them.  EMA=1: an ema.WeightEMA of the model (decay 0.9999) updated after every step (not with GRAPH=1: the update
takes its weight from the host).  OPT_DEVICE=1: optim.HipAdamW's device path (step count, bias corrections and rate formed by
ttv_opt_prepare; three launches per bucket instead of two) - with GRAPH=1 it is the HIP optimizer that is captured, not torch's.
--recompute: both towers on the recompute tape (TiTok.set_activation_recompute).  --ab: stored and recompute tape alternating in this
one process (ROUNDS= rounds of STEPS= timed steps per mode behind one untimed step, default 3; not with GRAPH=1), one JSON line with every round's time per mode
and torch.cuda.max_memory_allocated() per mode.  SIZE= tower size (default tiny), CLIP=TxHxW (default 16x128x128), K= tokens per clip
(default 128); --det-ab: deterministic mode (titok_video_amd.set_deterministic) off and on alternating in this one process, ROUNDS= rounds of
STEPS= timed steps per setting, one JSON line with every round's time per setting (profiles/deterministic_train_ab.txt); B=fit: the largest batch whose STORED tapes and backward workspace (the library's size functions) fill at most 3/4 of
the free device memory."""
import json, os, sys, time
from types import SimpleNamespace
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from titok_video_amd.model.titok import TiTok
from titok_video_amd.synthetic import seeded_titok_state, synthetic_clips
from titok_video_amd.train import freeze_python_gc, limit_host_threads, make_optimizer, training_step
RECOMPUTE, AB = "--recompute" in sys.argv[1:], "--ab" in sys.argv[1:]
DET_AB = "--det-ab" in sys.argv[1:]
SIZE = os.environ.get("SIZE", "tiny")
CLIP = tuple(int(v) for v in os.environ.get("CLIP", "16x128x128").split("x"))
K = int(os.environ.get("K", "128"))
if os.environ.get("TTV_DEBUG"):   # an OR of ttv_debug_set bits by value (the _lib.DBG_* table in tools/README.md; A/B runs on one box)
    from titok_video_amd import _lib
    _lib.lib().ttv_debug_set(int(os.environ["TTV_DEBUG"]))
cfg = SimpleNamespace(tokenizer=SimpleNamespace(model=SimpleNamespace(patch_size=[4, 8, 8], fsq_levels=[7, 5, 5, 5, 5], encoder_size=SIZE, decoder_size=SIZE)))
m = TiTok(cfg); m.load_state_dict(seeded_titok_state(0, encoder_size=SIZE, decoder_size=SIZE)); m = m.to("cuda:0", torch.bfloat16).train()
m.set_activation_recompute(RECOMPUTE)


def tape_and_workspace_bytes(n_clips, mode):
    """Both towers' tapes plus the larger backward workspace for n_clips clips, from the library's size functions."""
    import ctypes as C
    from titok_video_amd import _lib
    p = (CLIP[0] // 4) * (CLIP[1] // 8) * (CLIP[2] // 8)
    batch = _lib.Batch(n_clips=n_clips, total_rows=n_clips * (p + K), sum_tokens=n_clips * K, sum_patches=n_clips * p)
    tapes, ws = 0, 0
    for tower in (m.encoder, m.decoder):
        dims = tower._dims(_lib.TTV_BF16)
        tapes += _lib.lib().ttv_tower_tape_bytes_ex(C.byref(dims), C.byref(batch), mode)
        ws = max(ws, _lib.lib().ttv_tower_bwd_workspace_bytes_ex(C.byref(dims), C.byref(batch), mode))
    return tapes + ws


if os.environ.get("B", "32") == "fit":
    free = torch.cuda.mem_get_info("cuda:0")[0]
    B = 1
    while tape_and_workspace_bytes(B + 1, 0) <= 0.75 * free:
        B += 1
else:
    B = int(os.environ.get("B", "32"))
clips = synthetic_clips([CLIP] * B, seed=1, dtype=torch.bfloat16, device="cuda:0")
counts = [K] * B
GRAPH = os.environ.get("GRAPH", "0") == "1"
OPT_DEVICE = os.environ.get("OPT_DEVICE", "0") == "1"
opt = make_optimizer(m, hip_capturable=True) if OPT_DEVICE else make_optimizer(m, capturable=True) if GRAPH else make_optimizer(m)
if os.environ.get("GC_FREEZE", "1") == "1":
    freeze_python_gc()
    limit_host_threads()
n = int(os.environ.get("STEPS", "10"))
EMA = os.environ.get("EMA", "0") == "1" and not GRAPH
if EMA:
    from titok_video_amd.ema import WeightEMA
    ema = WeightEMA(m, decay=0.9999)
if DET_AB:
    assert not GRAPH, "--det-ab times eager steps"
    import titok_video_amd
    rounds = int(os.environ.get("ROUNDS", "3"))
    times, loss = {False: [], True: []}, {}
    for r in range(rounds + 1):                # round 0 warms both settings up (the larger workspace is allocated) and is not reported
        for mode in (False, True):
            titok_video_amd.set_deterministic(mode)
            training_step(m, clips, counts, opt)          # not timed
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                loss[mode], gn, _ = training_step(m, clips, counts, opt)
            torch.cuda.synchronize()
            if r > 0:
                times[mode].append(1e3 * (time.perf_counter() - t0) / n)
    titok_video_amd.set_deterministic(False)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    print(json.dumps({"size": SIZE, "clip": CLIP, "tokens": K, "batch": B, "steps_per_round": n, "off_ms_per_step": times[False],
                      "deterministic_ms_per_step": times[True], "off_ms_median": med[False], "deterministic_ms_median": med[True],
                      "deterministic_over_off": med[True] / med[False], "loss_off": float(loss[False]), "loss_deterministic": float(loss[True])}))
    sys.exit(0)
if AB:
    assert not GRAPH, "--ab times eager steps"
    rounds = int(os.environ.get("ROUNDS", "3"))
    times, peak, loss = {False: [], True: []}, {False: 0, True: 0}, {}
    # one clip first: the optimizer's state and the weight packs are allocated for good by the first step, and the caching allocator
    # would cut them out of the first full-size step's freed tape blocks - two stored base tapes then no longer find 100 GiB in one piece
    training_step(m, clips[:1], counts[:1], opt)
    for r in range(rounds + 1):                # round 0 warms both modes up and is not reported
        for mode in (False, True):
            m.set_activation_recompute(mode)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()           # the other mode's tape blocks go back first: two stored base tapes do not fit beside them
            training_step(m, clips, counts, opt)          # not timed: takes this mode's blocks from the device again
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            for _ in range(n):
                loss[mode], gn, _ = training_step(m, clips, counts, opt)
            torch.cuda.synchronize()
            if r > 0:
                times[mode].append(1e3 * (time.perf_counter() - t0) / n)
                peak[mode] = max(peak[mode], torch.cuda.max_memory_allocated())
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    print(json.dumps({"size": SIZE, "clip": CLIP, "tokens": K, "batch": B, "steps_per_round": n,
                      "stored_ms_per_step": times[False], "recompute_ms_per_step": times[True],
                      "stored_ms_median": med[False], "recompute_ms_median": med[True], "recompute_over_stored": med[True] / med[False],
                      "stored_peak_bytes": peak[False], "recompute_peak_bytes": peak[True],
                      "stored_tape_and_workspace_bytes": tape_and_workspace_bytes(B, 0),
                      "recompute_tape_and_workspace_bytes": tape_and_workspace_bytes(B, 1),
                      "loss": float(loss[True])}))
    sys.exit(0)
if GRAPH:
    from titok_video_amd.train import GraphedTrainingStep
    step = GraphedTrainingStep(m, opt, clips, counts)
    for _ in range(3):
        loss, gn, _ = step(clips)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        loss, gn, _ = step(clips)
    torch.cuda.synchronize()
else:
    for _ in range(3):
        training_step(m, clips, counts, opt)
        if EMA:
            ema.update()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        loss, gn, _ = training_step(m, clips, counts, opt)
        if EMA:
            ema.update()
    torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / n
print(json.dumps({"train_ms_per_step": 1e3 * dt, "clips_per_s": B / dt, "batch": B, "loss": float(loss), "graph": GRAPH, "ema": EMA, "opt_device": OPT_DEVICE,
                  "recompute": RECOMPUTE, "peak_bytes": torch.cuda.max_memory_allocated()}))
