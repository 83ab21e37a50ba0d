"""The allocator of the whole-video path without a GPU: `video.allocate_tokens`, `RateTable`, `TilePlan.tile_elements` and the default
ladder against the restatement of tests/rate_ref.py, against exhaustive search where that is possible, and by hand."""
import itertools
import math
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rate_ref as RR  # noqa: E402
import video_ref as VR  # noqa: E402

from titok_video_amd import video as V  # noqa: E402
from titok_video_amd.video import RateTable, allocate_tokens, default_ladder  # noqa: E402


def random_table(rng, kind):
    """(ladder, sse, elements).  'any': independent sums, so rows rise and fall, with zeros and repeats planted; 'falling': rows that
    fall but are not convex; 'convex': an equal-step ladder and strictly decreasing, strictly convex rows."""
    n, m = rng.randint(1, 5), rng.randint(1, 4)
    if kind == "convex":
        step = rng.randint(1, 6)
        first = rng.randint(1, 8)
        ladder = [first + step * l for l in range(m)]
    else:
        ladder = sorted(rng.sample(range(1, 40), m))
    elements = [3 * rng.randint(1, 4000) for _ in range(n)]
    sse = []
    for _ in range(n):
        if kind == "any":
            row = [rng.choice((0, 0, rng.randint(0, 50), rng.randint(0, 10 ** 7))) if rng.random() < 0.4 else rng.randint(1, 10 ** 9)
                   for _ in range(m)]
            if m > 1 and rng.random() < 0.3:
                row[rng.randrange(1, m)] = row[0]                       # a repeat: ties
        elif kind == "falling":
            row = sorted((rng.randint(0, 10 ** 8) for _ in range(m)), reverse=True)
        else:
            drops = sorted(rng.sample(range(1, 10 ** 6), m - 1), reverse=True) if m > 1 else []
            row = [rng.randint(1, 1000) + sum(drops)]
            for d in drops:
                row.append(row[-1] - d)
        sse.append(row)
    return ladder, sse, elements


def tables(kind, count, seed):
    rng = random.Random(seed)
    return [random_table(rng, kind) for _ in range(count)]


def budgets(rng, ladder, n):
    lo, hi = n * ladder[0], n * ladder[-1]
    return sorted({lo, hi, hi + 7, (lo + hi) // 2} | {rng.randint(lo, hi + 3) for _ in range(4)})


# ---- against the restatement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["any", "falling", "convex"])
def test_budget_mode_equals_the_restatement_and_keeps_its_promises(kind):
    rng = random.Random(11)
    seen_ragged = 0
    for ladder, sse, elements in tables(kind, 150, seed={"any": 1, "falling": 2, "convex": 3}[kind]):
        table = RateTable(ladder, sse, elements)
        n = len(sse)
        for budget in budgets(rng, ladder, n):
            got = allocate_tokens(table, total_tokens=budget)
            assert got == RR.allocate_budget(ladder, sse, budget), (ladder, sse, budget)
            assert len(got) == n and all(k in ladder for k in got) and sum(got) <= budget
            total = RR.total_sse(ladder, sse, got)
            for k in ladder:
                if n * k <= budget:
                    assert total <= RR.total_sse(ladder, sse, [k] * n), (ladder, sse, budget, got, k)
            seen_ragged += len(set(got)) > 1
    assert seen_ragged > 20                                             # not only uniform answers


def test_target_mode_equals_the_restatement():
    rng = random.Random(5)
    unreachable = 0
    for ladder, sse, elements in tables("any", 200, seed=4):
        table = RateTable(ladder, sse, elements)
        quality = table.psnr()
        for j, row in enumerate(sse):
            for l, v in enumerate(row):
                assert quality[j][l] == RR.psnr(v, elements[j]) and (quality[j][l] == math.inf) == (v == 0)
        for target in (0.0, 200.0, rng.uniform(-20, 60), rng.uniform(-20, 60)):
            got = allocate_tokens(table, target_psnr=target)
            assert got == RR.allocate_target(ladder, sse, elements, target), (ladder, sse, elements, target)
            unreachable += any(max(q) < target for q in quality)
    assert unreachable > 50


# ---- budget mode against exhaustive search ----------------------------------------------------------------------------------------------
def test_budget_mode_is_optimal_on_convex_tables():
    """With equal steps and strictly decreasing, strictly convex rows the greedy rule is optimal: no allocation within the budget has
    a lower total than the one returned.  Every one of len(ladder)^n_tiles allocations is tried."""
    rng = random.Random(21)
    tried = 0
    for ladder, sse, elements in tables("convex", 120, seed=6):
        n, m = len(sse), len(ladder)
        assert n <= 5 and m <= 4
        assert len({b - a for a, b in zip(ladder, ladder[1:])}) <= 1, "the ladder has equal steps"
        for row in sse:
            drops = [a - b for a, b in zip(row, row[1:])]
            assert all(d > 0 for d in drops), "rows are strictly decreasing"
            assert all(a > b for a, b in zip(drops, drops[1:])), "rows are strictly convex"
        table = RateTable(ladder, sse, elements)
        for budget in budgets(rng, ladder, n):
            best = min(sum(sse[j][l] for j, l in enumerate(levels)) for levels in itertools.product(range(m), repeat=n)
                       if sum(ladder[l] for l in levels) <= budget)
            got = allocate_tokens(table, total_tokens=budget)
            assert sum(got) <= budget and RR.total_sse(ladder, sse, got) == best, (ladder, sse, budget, got)
            tried += 1
    assert tried > 500


# ---- target mode by hand ----------------------------------------------------------------------------------------------------------------
def test_target_mode_by_hand():
    """3000 elements per tile: PSNR = 10 log10(65025 * 3000 / sse).  195075000 / sse: 1e3 -> 52.90 dB, 1e4 -> 42.90, 1e5 -> 32.90,
    1e6 -> 22.90, 1e7 -> 12.90."""
    ladder = (2, 4, 8, 16)
    sse = [[10 ** 7, 10 ** 6, 10 ** 5, 10 ** 4],          # falls: 12.9, 22.9, 32.9, 42.9
           [10 ** 5, 10 ** 7, 10 ** 4, 10 ** 6],          # not monotone: 32.9, 12.9, 42.9, 22.9
           [10 ** 6, 10 ** 7, 10 ** 6, 10 ** 7],          # never better than 22.9, the least sum twice
           [0, 10 ** 3, 0, 10 ** 3],                      # exact at 2 tokens
           [10 ** 3, 10 ** 3, 10 ** 3, 10 ** 3]]          # flat at 52.9
    table = RateTable(ladder, sse, [3000] * 5)
    quality = table.psnr()
    assert quality[3][0] == math.inf and abs(quality[0][2] - 32.90) < 0.01
    for target, want in ((30.0, [8, 2, 2, 2, 2]), (40.0, [16, 8, 2, 2, 2]), (50.0, [16, 8, 2, 2, 2]), (20.0, [4, 2, 2, 2, 2]),
                         (60.0, [16, 8, 2, 2, 2]), (-5.0, [2, 2, 2, 2, 2])):
        assert min(abs(q - target) for row in quality for q in row) > 1e-6, "a tile's PSNR lies on the target: the test would hang on a rounding"
        assert allocate_tokens(table, target_psnr=target) == want, target
        assert RR.allocate_target(ladder, sse, [3000] * 5, target) == want, target


def test_budget_mode_by_hand():
    ladder = (1, 2, 4)
    # tile 0: drops 90 then 6 (3 per token); tile 1: the middle point lies above the chord (10 then 60 -> one step of 70 / 3);
    # tile 2: rises, no step at all
    sse = [[100, 10, 4], [100, 90, 30], [50, 60, 70]]
    table = RateTable(ladder, sse, [300] * 3)
    assert allocate_tokens(table, total_tokens=3) == [1, 1, 1]
    assert allocate_tokens(table, total_tokens=4) == [2, 1, 1]                 # 90 per token
    assert allocate_tokens(table, total_tokens=6) == [4, 1, 1]                 # tile 1's one hull step takes 3 tokens, 2 are left
    assert allocate_tokens(table, total_tokens=7) == [2, 4, 1]                 # 70 / 3 per token beats 6 / 2
    assert allocate_tokens(table, total_tokens=9) == [4, 4, 1]
    assert allocate_tokens(table, total_tokens=100) == [4, 4, 1]               # tile 2 never leaves its best count
    # the guard: the hulls skip the middle count (30 then 70: the chord is steeper), their one step of 3 tokens does not fit what is
    # left of 4, and the uniform middle count does
    lad, rows = (1, 2, 4), [[100, 70, 0], [100, 70, 0]]
    t2 = RateTable(lad, rows, [3, 3])
    assert allocate_tokens(t2, total_tokens=4) == [2, 2] == RR.allocate_budget(lad, rows, 4)
    assert allocate_tokens(t2, total_tokens=5) == [4, 1] == RR.allocate_budget(lad, rows, 5)       # 100 in all, uniform 140


# ---- smaller checks ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    table = RateTable((2, 4), [[5, 3], [9, 1]], [30, 30])
    with pytest.raises(ValueError):
        allocate_tokens(table)
    with pytest.raises(ValueError):
        allocate_tokens(table, target_psnr=30.0, total_tokens=8)
    with pytest.raises(ValueError):
        allocate_tokens(table, total_tokens=3)                                 # below 2 tiles x 2 tokens
    assert allocate_tokens(table, total_tokens=4) == [2, 2]
    for ladder in ((4, 2), (2, 2), (0, 2), ()):
        with pytest.raises(ValueError):
            RateTable(ladder, [[1] * len(ladder)], [3])
    with pytest.raises(ValueError):
        RateTable((2, 4), [[1, 2, 3]], [3])                                    # a row longer than the ladder
    with pytest.raises(ValueError):
        RateTable((2, 4), [[1, 2]], [3, 3])                                    # an element count too many


def test_elements_for_short_axes():
    for video, tile, overlap, patch, stride in (((11, 37, 45), (8, 16, 24), (4, 8, 8), (4, 8, 8), 2),       # T' = 6 < 8
                                                ((5, 9, 13), (8, 16, 24), (4, 8, 8), (4, 8, 8), 1),         # every axis short
                                                ((9, 21, 27), (8, 16, 12), (4, 8, 4), (4, 8, 4), 1),
                                                ((20, 40, 56), (8, 32, 32), (4, 8, 8), (4, 8, 8), 1)):       # no short axis
        plan, ref = V.TilePlan(video, tile, overlap, patch, stride), VR.Plan(video, tile, overlap, patch, stride)
        assert plan.tile == ref.tile
        got = [plan.tile_elements(j) for j in range(plan.n_tiles)]
        assert got == [RR.elements(ref, j) for j in range(ref.n_tiles)]
        full = 3 * math.prod(plan.tile)
        short = any(n < t for n, t in zip(plan.timeline, plan.tile))
        assert all(g < full for g in got) if short else all(g == full for g in got)
    plan = V.TilePlan((5, 9, 13), (8, 16, 24), (4, 8, 8), (4, 8, 8))
    assert plan.n_tiles == 1 and plan.tile_elements(0) == 3 * 5 * 9 * 13


def test_default_ladder():
    assert default_ladder(128) == (16, 32, 64, 128)
    assert default_ladder(100) == (13, 25, 50, 100)
    assert default_ladder(8) == (1, 2, 4, 8)
    assert default_ladder(3) == (1, 2, 3)
    assert default_ladder(2) == (1, 2)
    assert default_ladder(1) == (1,)
    with pytest.raises(ValueError):
        default_ladder(0)


def test_level_of_the_restatement_on_every_bf16_value():
    """All bf16 values in [-1.5, 1.5], both zeros included, and the specials: the element-wise restatement, its array form and
    video_ref's blend rule agree."""
    bits = np.arange(0x10000, dtype=np.uint32) << 16
    vals = bits.view(np.float32)
    with np.errstate(invalid="ignore"):
        vals = vals[np.abs(vals) <= 1.5]
    assert vals.size > 32000 and (vals == 0).sum() == 2
    want = VR.levels_of(VR.clamp(vals)).astype(np.int64)
    assert (RR.level(vals) == want).all() and (RR.level_fast(vals) == want).all()
    assert want.min() == 0 and want.max() == 255 and len(np.unique(want)) == 256
    special = np.array([np.nan, np.inf, -np.inf, 0.0, 1.0, -1.0, 1.3, -1.3], dtype=np.float32)
    assert RR.level(special).tolist() == RR.level_fast(special).tolist() == [0, 255, 0, 128, 255, 0, 255, 0]
