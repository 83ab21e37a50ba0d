"""Golden fixture for the loader's resampling stage: torch-CPU `F.interpolate(x.float(), mode='bicubic', antialias=True)` (aten's
`_upsample_bicubic2d_aa`, the kernel torchvision's `resize(..., BICUBIC, antialias=True)` calls on its float path) on four small
uint8 clips, stored in fp32.  It pins tests/resample_ref.py to aten; the reference checkout is not needed.

    python tests/golden/make_golden_resample.py

Stored per case k: `frames_k` uint8 [2][Hs][Ws][3] (seeded noise: overshoot everywhere), `geom_k` = (T, Hs, Ws, Hr, Wr, oy, ox, Ho, Wo,
flip) and `out_k` fp32 [3][2][Ho][Wo] on the 0 .. 255 scale, unrounded.  Prints the largest |restatement - fixture| per case; the bound
of tests/test_resample_cpu.py::test_restatement_matches_aten_fixture is four times the largest of them.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import resample_ref as R  # noqa: E402

# name, geometry
CASES = [
    ("down_2x", R.train_geom(2, 16, 20, 8, 10)),
    ("down_1.37x_by_1.61x", R.train_geom(2, 26, 29, 19, 18)),
    ("up_1.25x", R.train_geom(2, 8, 12, 10, 15)),
    ("eval_window", R.eval_geom(2, 15, 22, 8, 12)),
]


def main():
    out, worst = {"names": np.array([c[0] for c in CASES])}, 0.0
    for k, (name, geom) in enumerate(CASES):
        frames = R.noise_frames(100 + k, *geom[:3])
        ref = R.torch_float_path(frames, geom)
        d = float(np.abs(R.prerounding(frames, geom) - ref.astype(np.float64)).max())
        worst = max(worst, d)
        print(f"{name}: geom {geom}  max |float64 restatement - aten fp32| = {d:.3e}")
        out[f"frames_{k}"], out[f"geom_{k}"], out[f"out_{k}"] = frames, np.array(geom, dtype=np.int32), ref
    path = os.path.join(HERE, "resample_kat.npz")
    np.savez_compressed(path, **out)
    print(f"largest difference {worst:.3e}; wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
