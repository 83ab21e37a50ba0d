"""Golden fixture for the evaluation LPIPS (EvalMetrics 'lpips'): runs the REFERENCE's own LPIPS.forward
(model/metrics/lpips_gram.py:184-200) on the CPU in fp32, one frame pair at a time, at frame sizes that are not multiples of 16.

Run in the build container only (needs the reference checkout):   python tests/golden/make_golden_lpips_eval.py

The torchvision stand-ins, the bypass of the network download and the seeded weights are those of make_golden_lpips.py.  The
reconstruction is clamped to [-1, 1] here, as EvalMetrics.update does before the image metrics (eval_metrics.py:33-37); the target
is not.  Inputs are not stored: tests/lpips_eval_ref.py re-draws them from the seeds (a fingerprint of each clip is stored).
Recorded: the seeds, the clip shapes (T, H, W), the fingerprints and the per-frame LPIPS values (fp32).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (sets sys.path for the reference and this repo)
import make_golden_lpips as ML  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
import lpips_eval_ref as E  # noqa: E402


def main():
    torch.set_num_threads(16)
    MG.install_standins()
    ML.install_lpips_standins()
    from titok_video_amd.synthetic import seeded_lpips_state
    import model.metrics.lpips_gram as RL
    RL.LPIPS.load_from_pretrained = lambda self, name="vgg_lpips": None
    lp = RL.LPIPS().eval()
    lp.load_state_dict(seeded_lpips_state(E.WEIGHT_SEED), strict=True)
    out = {"weight_seed": np.int64(E.WEIGHT_SEED), "clip_seed": np.int64(E.CLIP_SEED), "shapes": np.array(E.SHAPES, np.int32)}
    with torch.no_grad():
        for i, (recon, target) in enumerate(E.fixture_pairs()):
            out[f"clip{i}_fp"] = np.array(E.fingerprint(recon, target))
            x = recon.clamp(-1, 1)
            vals = [lp(x[:, t][None], target[:, t][None])[0] for t in range(recon.shape[1])]
            out[f"clip{i}_lpips"] = MG.np32(torch.cat(vals))
    MG.save("lpips_eval_kat.npz", **out)


if __name__ == "__main__":
    main()
