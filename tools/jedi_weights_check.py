#!/usr/bin/env python3
"""For whoever has upstream's real V-JEPA files: check that they map onto ours and compare our JEDi features with a plain torch
restatement of the same files.  No `jepa/` checkout is needed.

    python tools/jedi_weights_check.py path/to/vitl16.pth.tar path/to/ssv2-probe.pth.tar [--clips 2]

Prints the key / shape map each loader found (jedi.vjepa_state_dict / probe_state_dict), then runs a few seeded clips of
3 x 16 x 128 x 128 through the HIP path and through the restatement (F.interpolate bicubic, the ViT-L/16 blocks and the attentive
pooler written out in torch, float64 with the bf16-autocast rounding points; tests/vjepa_ref.py) on the same GPU, and prints the
relative L2 difference per feature vector, finetuned and not.  GPU box only."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import vjepa_ref as R  # noqa: E402
from titok_video_amd.model.metrics import jedi as J  # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("encoder")
    ap.add_argument("probe")
    ap.add_argument("--clips", type=int, default=2)
    args = ap.parse_args()
    enc, probe = J.vjepa_state_dict(args.encoder), J.probe_state_dict(args.probe)
    for name, sd in (("encoder", enc), ("probe", probe)):
        print(f"{name}: {len(sd)} tensors")
        for k, v in sd.items():
            if not k.startswith("blocks.") or k.startswith("blocks.0."):
                print(f"  {k:60s} {tuple(v.shape)}")
    model = J.VJEPA(enc, probe).to(DEV)
    g = torch.Generator().manual_seed(0)
    clips = [(torch.rand(3, 16, 128, 128, generator=g) * 2 - 1).to(DEV, torch.bfloat16) for _ in range(args.clips)]
    worst = 0.0
    for finetuned in (True, False):
        ours = model.features([clips], finetuned)
        for i, c in enumerate(clips):
            theirs = R.features(c, enc, probe, finetuned)
            rel = float((ours[i].double() - theirs).norm() / theirs.norm())
            worst = max(worst, rel)
            print(f"finetuned={finetuned} clip {i}: |ours - restatement| / |restatement| = {rel:.3e}")
    print(f"worst {worst:.3e}: " + ("features agree" if worst < 2e-2 else "FEATURES DISAGREE"))
    sys.exit(0 if worst < 2e-2 else 1)


if __name__ == "__main__":
    main()
