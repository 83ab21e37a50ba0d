#!/usr/bin/env python3
"""For whoever has the reference's real detector file: compare our I3D features with the TorchScript detector's own.

    python tools/fvd_detector_check.py path/to/i3d_torchscript.pt [--clips 4]

Loads the file twice: through fvd.i3d_state_dict (which proves the parameter layout maps onto ours) and with torch.jit.load, then
runs both on a few seeded clips of 3 x 16 x 128 x 128 preprocessed as the reference does (F.interpolate to (3, 224, 224), last
frame repeated to 10): ours through the HIP path, theirs as `detector(x, rescale=False, resize=False, return_features=True)` in
fp32 on the same GPU.  Prints the max |difference| per clip relative to the largest feature.  GPU box only."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from titok_video_amd.model.metrics import fvd  # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("path")
    ap.add_argument("--clips", type=int, default=4)
    args = ap.parse_args()
    det = fvd.I3D.from_file(args.path)
    print(f"{args.path}: parameter layout maps onto the canonical I3D state dict")
    ref = torch.jit.load(args.path, map_location="cpu").eval().to(DEV, torch.float32)
    g = torch.Generator().manual_seed(0)
    clips = [(torch.rand(3, 16, 128, 128, generator=g) * 2 - 1).to(DEV) for _ in range(args.clips)]
    ours = det.features([(clips, False)])
    worst = 0.0
    with torch.no_grad():
        for i, c in enumerate(clips):
            x = F.interpolate(c[None], size=(3, 224, 224), mode="trilinear", align_corners=False)
            x = torch.cat([x, x[:, :, -1:].repeat(1, 1, 7, 1, 1)], dim=2)
            theirs = ref(x, rescale=False, resize=False, return_features=True).reshape(-1).float()
            rel = float((ours[i] - theirs).abs().max() / theirs.abs().max())
            worst = max(worst, rel)
            print(f"clip {i}: max |ours - detector| / max |detector| = {rel:.3e}")
    print(f"worst {worst:.3e}: " + ("features agree" if worst < 1e-4 else "FEATURES DISAGREE"))
    sys.exit(0 if worst < 1e-4 else 1)


if __name__ == "__main__":
    main()
