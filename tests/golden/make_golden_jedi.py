"""Golden fixture for JEDi's statistic: runs the REFERENCE's own mmd_poly (model/metrics/jedi.py) with the installed sklearn.

Run in the build container only (needs the reference checkout):   python tests/golden/make_golden_jedi.py

The reference's jedi.py cannot be imported (it imports the `jepa/` checkout and torchvision), so the function definition of
mmd_poly is taken out of the file with `ast` and executed on its own, with `metrics` bound to sklearn.metrics as the file binds it.
Nothing of it is stored here: the fixture holds results only.

Inputs are not stored: they are re-drawn from the seeds below.  Recorded: mmd_poly(X, Y, degree=2, coef0=0) (the call of
JEDiMetric.compute, without its factor 100) of seeded feature sets with n = m = 1, 2, 37, 300, in float32 and float64, and for
identical sets; plus degree 3 / coef0 1 and degree 2 / coef0 1 for the direct path.
"""
from __future__ import annotations

import ast
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_FILE = "/root/reference/model/metrics/jedi.py"
SEED, DIM = 41, 48
CASES = [(1, "float32", False), (2, "float32", False), (37, "float32", False), (300, "float32", False),
         (1, "float64", False), (2, "float64", False), (37, "float64", False), (300, "float64", False),
         (37, "float64", True), (300, "float32", True)]
EXTRA = [(37, 3, 1.0), (37, 2, 1.0)]    # (n, degree, coef0) for the direct path, float64


def feature_sets(i: int, n: int, dtype: str, same: bool):
    """Seeded (X, Y) [n, DIM]: X ~ N(0, 1), Y = 0.8 X' + 0.3 with X' an independent draw (or Y = X)."""
    rng = np.random.default_rng(SEED + i)
    X = rng.standard_normal((n, DIM)).astype(dtype)
    Y = X.copy() if same else (0.8 * rng.standard_normal((n, DIM)) + 0.3).astype(dtype)
    return X, Y


def reference_mmd_poly():
    from sklearn import metrics

    tree = ast.parse(open(REF_FILE).read())
    fn = next(node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name == "mmd_poly")
    scope = {"metrics": metrics}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), REF_FILE, "exec"), scope)
    return scope["mmd_poly"]


def main():
    mmd = reference_mmd_poly()
    vals = [float(mmd(*feature_sets(i, n, dt, same), degree=2, coef0=0)) for i, (n, dt, same) in enumerate(CASES)]
    extra = []
    for j, (n, deg, c0) in enumerate(EXTRA):
        X, Y = feature_sets(100 + j, n, "float64", False)
        extra.append(float(mmd(X, Y, degree=deg, coef0=c0)))
    np.savez(os.path.join(HERE, "jedi_kat.npz"), seed=SEED, dim=DIM,
             n=np.array([c[0] for c in CASES]), dtype=np.array([c[1] for c in CASES]), same=np.array([c[2] for c in CASES]),
             mmd=np.array(vals), extra_cases=np.array(EXTRA, dtype=np.float64), extra_mmd=np.array(extra))
    print("wrote jedi_kat.npz", vals, extra)


if __name__ == "__main__":
    main()
