#!/usr/bin/env python3
"""Tower-level A/B of the opt-in e4m3 P.V attention (TiTok.set_attention_pv): whole forwards (encode -> FSQ -> decode) with the mode off
and on, alternated ROUNDS times in ONE process on one box, for
  tiny    tiny towers at the benchmark batch (32 clips of 16x128x128, K = 128)
  base4   base towers, B clips of 32x256x256, K = 1024, bf16 linears            (BASELINE config #4's shape)
  base5   the same with fp8_linears = "mx" (all four linears block-scaled e4m3)  (BASELINE config #5's shape, FSQ in place of the L2 codebook)
Prints clips/s of every leg and, against the bf16 / mode-off forward of the SAME weights and clips: the relative error of the
pre-quantisation tokens z and the fraction of FSQ indices kept.  (README's 0.111 / 82 % for config #5 are against the fp32 oracle with
the L2 codebook on one clip - a different yardstick; the `mx linears, pv off` row here is that mode on this tool's yardstick.)
GPU box only.    [ROUNDS=3] [STEPS=5] [B=4] python tools/pv8_ab.py [tiny base4 base5]"""
import os
import sys
import time
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from titok_video_amd.model.titok import TiTok  # noqa: E402
from titok_video_amd.synthetic import seeded_titok_state, synthetic_clips  # noqa: E402

DEV = "cuda:0"
ROUNDS, STEPS, B_BASE = int(os.environ.get("ROUNDS", "3")), int(os.environ.get("STEPS", "5")), int(os.environ.get("B", "4"))
CONFIGS = {
    "tiny": dict(size="tiny", clip=(16, 128, 128), k=128, batch=32, gain=6.0, fp8=False, steps=10),      # (x STEPS: ~1 ms forwards)
    "base4": dict(size="base", clip=(32, 256, 256), k=1024, batch=B_BASE, gain=2.0, fp8=False),
    "base5": dict(size="base", clip=(32, 256, 256), k=1024, batch=B_BASE, gain=2.0, fp8="mx"),
}


def leg(m, clips, counts, fp8, pv, steps):
    m.encoder.fp8_linears = m.decoder.fp8_linears = fp8
    m.set_attention_pv(pv)
    with torch.no_grad():
        for _ in range(2):
            m(clips, counts)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            m(clips, counts)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        res = m.encoder.run(clips, counts, None, m.quantize.params, want_z=True)
    return len(clips) / dt, res["z"].float().cpu(), res["indices"].cpu()


for name in sys.argv[1:] or list(CONFIGS):
    c = CONFIGS[name]
    cfg = SimpleNamespace(tokenizer=SimpleNamespace(model=SimpleNamespace(patch_size=[4, 8, 8], fsq_levels=[8, 8, 8, 6, 5], encoder_size=c["size"],
                                                                            decoder_size=c["size"])))
    m = TiTok(cfg)
    m.load_state_dict(seeded_titok_state(0, c["size"], c["size"], gain=c["gain"]))
    m = m.to(DEV, torch.bfloat16).eval()
    clips = synthetic_clips([c["clip"]] * c["batch"], seed=1, dtype=torch.bfloat16, device=DEV)
    counts = [c["k"]] * c["batch"]
    _, z0, i0 = leg(m, clips, counts, False, None, 1)          # the yardstick: bf16 linears, bf16 P.V
    legs = [("pv off", c["fp8"], None), ("pv fp8", c["fp8"], "fp8")]
    print(f"== {name}: {c['size']} towers, {c['batch']} x {c['clip']} K = {c['k']}, fp8_linears = {c['fp8']}; {ROUNDS} alternations, {STEPS * c.get('steps', 1)} timed forwards per leg")
    for r in range(ROUNDS):
        for label, fp8, pv in legs:
            cps, z, idx = leg(m, clips, counts, fp8, pv, STEPS * c.get("steps", 1))
            print(f"{name} round {r} {label:7s}: {cps:9.1f} clips/s   z rel err vs bf16 {float((z - z0).norm() / z0.norm()):.4f}   "
                  f"FSQ indices kept {100.0 * float((idx == i0).float().mean()):.1f} %", flush=True)
    del m, clips
    torch.cuda.empty_cache()
