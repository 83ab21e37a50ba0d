"""The R1 / R2 noise generator's restatement (tests/gp_noise_ref.py) on the CPU: the integer part against the Philox4x32-10 known
answers (Random123's kat_vectors), restated once more in pure Python; the uniform map's ends; the block layout over clips whose
numel is no multiple of 4; disjoint streams per draw; and the float32 evaluation of the same formulas against the float64 one,
which the GPU test's bf16 cap (at most 0.5 % of the elements differ from the bf16 chain) relies on."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gp_noise_ref as GR  # noqa: E402

KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def philox_python(counter, key):
    c, (k0, k1) = list(counter), key
    for _ in range(10):
        p0, p1 = GR.M0 * c[0], GR.M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k1, p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + GR.W0) & 0xFFFFFFFF, (k1 + GR.W1) & 0xFFFFFFFF
    return tuple(c)


def test_philox_known_answers():
    for counter, key, want in KAT:
        assert philox_python(counter, key) == want
        got = GR.philox4x32_10([np.array([v]) for v in counter], key)
        assert tuple(int(v[0]) for v in got) == want
    rng = np.random.default_rng(0)                              # the vectorised form on arbitrary counters
    ctr = rng.integers(0, 2 ** 32, size=(4, 64), dtype=np.uint64)
    got = GR.philox4x32_10(list(ctr), (0x01234567, 0x89ABCDEF))
    for j in range(64):
        assert tuple(int(v[j]) for v in got) == philox_python([int(v) for v in ctr[:, j]], (0x01234567, 0x89ABCDEF))


def test_uniform_stays_strictly_inside_the_unit_interval_and_is_exact_in_float32():
    for ftype in (np.float64, np.float32):
        lo, hi = GR.unit_open(np.array([0, 2 ** 32 - 1], dtype=np.uint32), ftype)
        assert lo == 2.0 ** -24 and hi == 1.0 - 2.0 ** -24 and 0.0 < lo < hi < 1.0
    x = np.random.default_rng(1).integers(0, 2 ** 32, size=4096, dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(GR.unit_open(x, np.float32).astype(np.float64), GR.unit_open(x, np.float64))
    assert np.isfinite(np.sqrt(-2.0 * np.log(GR.unit_open(np.array([0, 2 ** 32 - 1], dtype=np.uint32))))).all()


def test_block_layout_over_clips_whose_numel_is_no_multiple_of_four():
    numels = [105, 6, 768, 1]
    offs, total = GR.clip_offsets(numels)
    assert offs == [0, 108, 116, 884] and total == 888 and all(o % 4 == 0 for o in offs)
    whole = GR.normals(0, total, seed=7, draw=3)
    for o, n in zip(offs, numels):                              # a clip reads its own blocks: lane = element % 4 of the padded line
        assert np.array_equal(GR.normals(o, n, seed=7, draw=3), whole[o:o + n])
    blocks = [set(range(o // 4, (o + n + 3) // 4)) for o, n in zip(offs, numels)]
    for i in range(len(blocks)):
        for j in range(i + 1, len(blocks)):
            assert not blocks[i] & blocks[j]                    # no block straddles two clips
    w = GR.philox4x32_10([np.array([27]), np.array([0]), np.array([3]), np.array([0])], (7, 0))       # block 27 = elements 108 .. 111
    ua, ub = GR.unit_open(w[0]), GR.unit_open(w[1])
    r = np.sqrt(-2.0 * np.log(ua))
    assert whole[108] == (r * np.cos(2.0 * np.pi * ub))[0] and whole[109] == (r * np.sin(2.0 * np.pi * ub))[0]


def test_draws_and_seeds_give_disjoint_streams():
    n = 1 << 14
    a, b = GR.normals(0, n, seed=11, draw=0), GR.normals(0, n, seed=11, draw=1)
    c, d = GR.normals(0, n, seed=12, draw=0), GR.normals(0, n, seed=11 + (1 << 32), draw=0)
    e = GR.normals(0, n, seed=11, draw=1 << 32)
    streams = [a, b, c, d, e]
    assert np.array_equal(a, GR.normals(0, n, seed=11, draw=0))
    for i in range(5):
        for j in range(i + 1, 5):
            assert not np.intersect1d(streams[i], streams[j]).size       # no value in common, let alone a shifted copy
            assert abs(np.corrcoef(streams[i], streams[j])[0, 1]) < 5 / np.sqrt(n)


def test_float32_evaluation_stays_far_under_the_bf16_cap():
    """The GPU test caps the elements that differ from the restatement's bf16 chain at 0.5 %.  A float32 evaluation of the same
    formulas (numpy's log, sqrt, cos, sin in float32) must stay under that cap against the float64 one by a wide margin.  Estimate: an
    element differs when the float64 normal lies within the float32 evaluation's error of a bf16 rounding boundary.  The angle 2 pi u
    is rounded to float32 (up to 2^-22 absolute at 6.28), log, sqrt and the product add a few 2^-24 relative, so the error is a few
    2^-23 |n| against boundaries 2^-8 |n| to 2^-7 |n| apart: a fraction of about 2 * 4 * 2^-23 / 2^-8 = 2.4e-4 at the most, a twentieth
    of the cap.  Held here to a tenth of the cap."""
    n = 1 << 20
    n64, n32 = GR.normals(0, n, seed=5, draw=0), GR.normals(0, n, seed=5, draw=0, ftype=np.float32).astype(np.float64)
    assert np.abs(n32 - n64).max() < 64 * 2.0 ** -24 * 6.0
    gp = float(np.float32(0.01))
    chain = lambda v: GR.round_bf16(GR.round_f32(GR.round_bf16(v) * gp))
    differ = float(np.mean(chain(n32) != chain(n64)))
    print(f"float32 vs float64 evaluation: {differ:.2e} of the bf16 s values differ")
    assert differ < 0.005 / 10


def test_round_bf16_matches_torch():
    import torch
    x = np.random.default_rng(2).standard_normal(1 << 14) * np.exp(np.random.default_rng(3).uniform(-20, 20, 1 << 14))
    x = np.concatenate([x, [0.0, 1.0, 1.00390625, 1.01171875, -3.0e-39]])      # ties to even at 1 + 2^-8 and 1 + 3 2^-8
    want = torch.from_numpy(x).to(torch.bfloat16).double().numpy()
    assert np.array_equal(GR.round_bf16(x)[:-1], want[:-1])
