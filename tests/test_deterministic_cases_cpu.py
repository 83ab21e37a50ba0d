"""What tests/test_hip_deterministic.py rests on, checked without a GPU on the inputs of tests/deterministic_cases.py:

  * a plain float32 sum of a destination's terms, one after the other, stays inside the bound n * 2^-24 * sum |term| around the float64
    sum - so the bound is one a correct fp32 summation meets (the kernels sum in another, also fixed, order: the bound holds for any);
  * the terms of a destination really span about 2^20 in magnitude (at least 2^16 between the largest and the smallest non-zero term of
    every destination whose terms walk the range - all but the codebook entries with a few rows: the inputs walk 2^20 exactly, the derived factors near one take at most
    2^4 of it) and have both signs;
  * no destination's float64 sum is so close to zero that the bound exceeds the sum itself: a wrong value would then pass.
"""
import numpy as np
import pytest

from tests import deterministic_cases as DC


def _cases():
    out = []
    for rows, width in DC.RMS_SHAPES:
        for maps in (False, True):
            out.append((f"rmsnorm {rows}x{width} maps={maps}", lambda r=rows, w=width, m=maps: DC.rmsnorm_case(r, w, m), True))
        out.append((f"chain {rows}x{width}", lambda r=rows, w=width: DC.chain_case(r, w), True))
    out += [("colsum", DC.colsum_case, True), ("sumall", DC.sumall_case, True), ("outer_small", DC.outer_small_case, True),
            ("vq", DC.vq_case, True), ("wgrad 65", lambda: DC.wgrad_case(65), True), ("wgrad 1025", lambda: DC.wgrad_case(1025), True)]
    c = DC.clips_case()
    out.append(("l1", lambda: {"terms": c["l1_terms"], "count": np.array([len(c["l1_terms"])])}, False))      # |r - t|: one sign only
    out.append(("sq_err", lambda: {"terms": c["sq_terms"], "count": np.array([len(c["sq_terms"])])}, False))  # squares
    return out


CASES = _cases()


@pytest.mark.parametrize("name,build,signed", CASES, ids=[c[0] for c in CASES])
def test_terms_are_what_the_gpu_test_assumes(name, build, signed):
    case = build()
    terms, count = case["terms"], np.asarray(case["count"])
    assert terms.dtype == np.float64 and terms.ndim == 2 and count.shape == (terms.shape[1],)
    total, bound = DC.f64_sum_and_bound(terms, count)
    live = count > 0
    assert live.sum() >= 1 and (not name.startswith("vq") or (~live).sum() == 5), "vq: exactly one entry (5 columns) takes no row"
    # 1. the float32 sequential sum meets the bound
    seq = DC.sequential_f32(terms).astype(np.float64)
    assert np.all(np.abs(seq - total)[live] <= bound[live]), name
    # 2. the range and the signs: every destination with at least 9 terms
    mag = np.abs(terms)
    big = mag.max(0)
    small = np.where(mag > 0, mag, np.inf).min(0)
    walked = live & (count >= case.get("walk_min", 9))
    assert walked.any()
    span = np.log2(big[walked] / small[walked])
    assert span.min() >= 16, (name, float(span.min()))
    if signed:
        mixed = ((terms > 0).any(0) & (terms < 0).any(0))[walked]
        # the chain's terms carry the sign of a second random factor: nine rows of three-to-one signs leave 0.75^9 + 0.25^9 = 7.5 % of the
        # columns one-signed (expected), so 85 % mixed is asked of those; every other case has both signs in every destination
        assert mixed.mean() >= 0.85 if name.startswith("chain 9x") else mixed.all(), (name, float(mixed.mean()))
    # 3. the bound is not vacuous
    assert np.all(bound[live] < np.abs(total[live])), (name, float((bound[live] / np.abs(total[live])).max()))


def test_fold_is_the_sequential_sum_in_block_order():
    """fold_f32, the second stage restated: block 0's partial first, the destination last."""
    p = np.array([[1.0], [2.0 ** -24], [2.0 ** -24], [-1.0]], dtype=np.float32)
    assert DC.fold_f32(np.array([0.0], dtype=np.float32), p)[0] == 0.0                   # 1 + 2^-24 rounds back to 1, twice
    assert DC.fold_f32(np.array([0.0], dtype=np.float32), p[::-1].copy())[0] == np.float32(2.0 ** -23)   # -1 + 2^-24 is exact
    q = np.array([[2.0 ** -24], [2.0 ** -24], [1.0], [-1.0]], dtype=np.float32)
    assert DC.fold_f32(np.array([0.0], dtype=np.float32), q)[0] == np.float32(2.0 ** -23)   # the small ones first: they survive
    assert DC.fold_f32(np.array([4.0], dtype=np.float32), q)[0] == np.float32(4.0)          # ... and are lost against the destination
