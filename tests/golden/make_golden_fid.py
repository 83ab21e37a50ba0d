"""Golden fixture for the frame statistics: runs the REFERENCE's own calculate_fid, compute_inception_score and mmd_poly
(model/metrics/metrics.py) with the installed numpy, scipy and sklearn.

Run in the build container only (needs the reference checkout):   python tests/golden/make_golden_fid.py

The reference's metrics.py cannot be imported (it imports torchvision and torchmetrics), so the function definitions of
calculate_fid, calculate_frechet_distance, calculate_activation_statistics, compute_inception_score and mmd_poly are taken out of
the file with `ast` and executed on their own, with `np`, `linalg` and `metrics` bound as the file binds them.  Nothing of it is
stored here: the fixture holds results only.

Inputs are not stored: they are re-drawn from the seeds below (`feature_sets`, `prob_sets`; tests/test_fid_cpu.py repeats the two
recipes).  Recorded, all on float64 inputs: calculate_fid(real, fake) and mmd_poly(real, fake, degree=2, coef0=0) (the call of
MetricCalculator.gather, without its factor 100) of seeded feature sets of dimension 48 with n = 2, 37, 300 and one identical
pair; compute_inception_score of seeded softmax rows over 10 classes.
"""
from __future__ import annotations

import ast
import os
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_FILE = "/root/reference/model/metrics/metrics.py"
SEED, DIM, CLASSES = 73, 48, 10
FEAT_CASES = [(2, False), (37, False), (300, False), (37, True)]          # (n, identical pair)
PROB_CASES = [(1, 1.0), (37, 1.0), (300, 3.0)]                             # (n, logit spread)
NAMES = ("calculate_fid", "calculate_frechet_distance", "calculate_activation_statistics", "compute_inception_score", "mmd_poly")


def feature_sets(i: int, n: int, same: bool):
    """Seeded (real, fake) [n, DIM] float64: real ~ N(0, 1) scaled per dimension, fake = 0.8 N(0, 1) + 0.3 (or fake = real)."""
    rng = np.random.default_rng(SEED + i)
    real = rng.standard_normal((n, DIM)) * (1.0 + 0.5 * rng.random(DIM))
    fake = real.copy() if same else 0.8 * rng.standard_normal((n, DIM)) + 0.3
    return real, fake


def prob_sets(i: int, n: int, spread: float):
    """Seeded softmax rows [n, CLASSES] float64 of logits N(0, spread^2)."""
    rng = np.random.default_rng(SEED + 100 + i)
    z = spread * rng.standard_normal((n, CLASSES))
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def reference_functions():
    from scipy import linalg
    from sklearn import metrics

    tree = ast.parse(open(REF_FILE).read())
    fns = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in NAMES]
    assert sorted(f.name for f in fns) == sorted(NAMES)
    scope = {"np": np, "linalg": linalg, "metrics": metrics}
    exec(compile(ast.Module(body=fns, type_ignores=[]), REF_FILE, "exec"), scope)
    return scope


def main():
    ref = reference_functions()
    fid, mmd = [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i, (n, same) in enumerate(FEAT_CASES):
            real, fake = feature_sets(i, n, same)
            fid.append(float(ref["calculate_fid"](real, fake)))
            mmd.append(float(ref["mmd_poly"](real, fake, degree=2, coef0=0)))
    iscore = [float(ref["compute_inception_score"](prob_sets(i, n, s))) for i, (n, s) in enumerate(PROB_CASES)]
    np.savez(os.path.join(HERE, "fid_kat.npz"), seed=SEED, dim=DIM, classes=CLASSES,
             feat_cases=np.array(FEAT_CASES, dtype=np.int64), fid=np.array(fid), mmd=np.array(mmd),
             prob_cases=np.array(PROB_CASES, dtype=np.float64), inception_score=np.array(iscore))
    print("wrote fid_kat.npz", fid, mmd, iscore)


if __name__ == "__main__":
    main()
