"""Golden fixture for FVD: runs the REFERENCE's own code (model/metrics/fvd.py FVDCalculator.update / compute and
frechet_distance) on the CPU.

Run in the build container only (needs the reference checkout):   python tests/golden/make_golden_fvd.py

FVDCalculator.__init__ downloads the I3D TorchScript file; it is bypassed (the object is built with __new__ and the attributes
__init__ would set), and `self.detector` is a stand-in callable that records a fingerprint of every detector input (shape, sum,
sum of squares, a strided pixel sample) and returns a fixed seeded projection of it as the features.  So the fixture pins the
reference's preprocessing (F.interpolate to size (C, 224, 224), then the last frame repeated to 10 frames) and its Fréchet
distance, not the detector.

Inputs are not stored: they are re-drawn from the seeds below.  Recorded:
  * for ragged clip pairs (T in {1, 2, 3, 8, 16, 17}; 128 x 128, 168 x 136, 96 x 160, 300 x 260), recon clamped to [-1, 1] as
    EvalMetrics does before the call: the fingerprints of both detector inputs, and compute() on the stand-in's features;
  * frechet_distance(fake, real) of seeded float64 feature sets with N = 1, 2, 37 and 450 (full-rank covariance at d = 400),
    including identical sets.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402,F401  (sets sys.path for the reference and this repo)

CLIP_SEED = 17
CLIP_SHAPES = [(1, 128, 128), (2, 168, 136), (3, 96, 160), (8, 300, 260), (16, 128, 128), (17, 168, 136)]
SAMPLE_STRIDE = 9973
PROJ_SEED, PROJ_DIM, PROJ_STRIDE = 23, 16, 101
FEAT_SEED = 29
FEAT_SETS = [(1, False), (2, False), (37, False), (450, False), (37, True), (450, True)]


def clip_pair(i: int):
    """Seeded (recon, target) [3, T, H, W] fp32; recon spreads past [-1, 1] so the clamp matters."""
    g = torch.Generator().manual_seed(CLIP_SEED + i)
    shape = (3,) + CLIP_SHAPES[i]
    recon = (torch.rand(shape, generator=g) * 2 - 1) * 1.2
    target = torch.rand(shape, generator=g) * 2 - 1
    return recon, target


def fingerprint(x: torch.Tensor):
    x64 = x.double()
    return (np.array(x.shape, dtype=np.int64), float(x64.sum()), float((x64 * x64).sum()),
            x.reshape(-1)[::SAMPLE_STRIDE].double().numpy())


def feature_sets(i: int):
    n, same = FEAT_SETS[i]
    g = np.random.default_rng(FEAT_SEED + i)
    fake = g.standard_normal((n, 400)) * (1.0 + 0.5 * g.random(400)) + 0.3
    real = fake.copy() if same else g.standard_normal((n, 400)) * (1.0 + 0.5 * g.random(400))
    return fake, real


class StandIn:
    def __init__(self):
        g = torch.Generator().manual_seed(PROJ_SEED)
        self.proj = None
        self.g = g
        self.records = []

    def __call__(self, x, rescale=None, resize=None, return_features=None):
        assert rescale is False and resize is False and return_features is True
        self.records.append(fingerprint(x[0]))
        flat = x.reshape(x.shape[0], -1)[:, ::PROJ_STRIDE].double()
        if self.proj is None:
            self.proj = torch.randn(flat.shape[1], PROJ_DIM, generator=self.g, dtype=torch.float64)
        return (flat @ self.proj).float()


def main():
    import torch.nn as nn
    from model.metrics import fvd as ref

    calc = ref.FVDCalculator.__new__(ref.FVDCalculator)
    nn.Module.__init__(calc)
    calc.detector = StandIn()
    calc.detector_kwargs = dict(rescale=False, resize=False, return_features=True)
    calc.metric_name = "fvd"
    calc.reset()
    for i in range(len(CLIP_SHAPES)):
        recon, target = clip_pair(i)
        calc.update(recon.clamp(-1, 1).unsqueeze(0), target.unsqueeze(0))
    out = {"clip_seed": CLIP_SEED, "clip_shapes": np.array(CLIP_SHAPES, dtype=np.int64), "sample_stride": SAMPLE_STRIDE,
           "feat_seed": FEAT_SEED, "feat_sets": np.array([(n, int(s)) for n, s in FEAT_SETS], dtype=np.int64),
           "update_compute": float(calc.compute())}
    # update() calls the detector on the target first, then on the reconstruction
    for i in range(len(CLIP_SHAPES)):
        for which, rec in (("real", calc.detector.records[2 * i]), ("fake", calc.detector.records[2 * i + 1])):
            shape, s, ss, sample = rec
            out[f"{which}{i}_shape"], out[f"{which}{i}_sum"], out[f"{which}{i}_sumsq"], out[f"{which}{i}_sample"] = shape, s, ss, sample
    out["fvd"] = np.array([ref.frechet_distance(*feature_sets(i)) for i in range(len(FEAT_SETS))])
    np.savez_compressed(os.path.join(HERE, "fvd_kat.npz"), **out)
    print("fvd:", out["fvd"], "update compute:", out["update_compute"])


if __name__ == "__main__":
    main()
