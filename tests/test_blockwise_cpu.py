"""tests/blockwise.py, the per-(sequence, head, 64-row block) checker of the attention tests and the per-128x128-tile checker of the
weight gradients: each must catch one wrong block or tile that the global relative error lets through.  Second half: the helpers
of the inference-forward tests (tests/test_hip_forward_shapes.py) - what the global check of tests/test_hip_ops.py accepts and the
per-block, per-tile and per-row checks reject, the chunked float64 forward reference, and the no-floored-block condition on the
inputs those tests launch."""
import pytest
import torch

from tests.blockwise import block_errors, check_blockwise, check_tiles, global_error, row_blocks, tile_errors

# 16 benchmark-size clips (1152 rows each, 18 blocks) and a ragged tail; 8 heads of width 64: 2 328 (block, head) cells
CU = [0] + [1152 * (i + 1) for i in range(16)] + [1152 * 16 + 317, 1152 * 16 + 317 + 53, 1152 * 16 + 317 + 53 + 1]
HEADS = 8
BLOCK_TOL = 2e-2           # the per-block bf16 bound of tests/test_hip_backward_shapes.py
GLOBAL_TOL = 2.5e-2         # the global bf16 bound of tests/test_hip_backward.py test_attention_backward


def _pair():
    g = torch.Generator().manual_seed(0)
    ref = torch.randn(CU[-1], HEADS * 64, generator=g)
    out = ref * (1 + 1e-3 * torch.randn(ref.shape, generator=g))      # a close result: ~1e-3 everywhere
    return out, ref


def test_row_blocks_restart_at_every_sequence():
    ids, n = row_blocks([0, 130, 131, 195], 64)
    assert n == 3 + 1 + 1
    assert ids[:130].tolist() == [0] * 64 + [1] * 64 + [2] * 2
    assert ids[130:].tolist() == [3] + [4] * 64


def test_close_result_passes():
    out, ref = _pair()
    worst, glob = check_blockwise(out, ref, CU, HEADS, BLOCK_TOL, GLOBAL_TOL)
    assert worst < 2e-3 and glob < 2e-3


@pytest.mark.parametrize("factor", [1.05, 0.0])
@pytest.mark.parametrize("where", [(3, 37, 5), (17, 0, 7), (18, 0, 0)])   # (sequence, first row in it, head); 18: the one-row sequence
def test_one_wrong_block_is_rejected_where_the_global_bound_passes(factor, where):
    out, ref = _pair()
    seq, row, head = where
    r0 = CU[seq] + row // 64 * 64
    r1 = min(r0 + 64, CU[seq + 1])
    bad = ref.clone()
    bad[r0:r1, head * 64:(head + 1) * 64] *= factor
    assert global_error(out, bad) < GLOBAL_TOL                        # the global bound alone lets it through
    with pytest.raises(AssertionError, match="block"):
        check_blockwise(out, bad, CU, HEADS, BLOCK_TOL, GLOBAL_TOL)
    err = block_errors(out, bad, CU, HEADS)
    blk = int(row_blocks(CU)[0][r0])
    assert float(err[blk, head]) > BLOCK_TOL
    err[blk, head] = 0
    assert float(err.max()) < 2e-3                                    # and only that cell


def test_non_finite_result_is_rejected():
    out, ref = _pair()
    out[5, 3] = float("nan")
    with pytest.raises(AssertionError, match="non-finite"):
        check_blockwise(out, ref, CU, HEADS, BLOCK_TOL, GLOBAL_TOL)


def test_attention_reference_matches_the_oracle_and_autograd():
    """The float64 reference of the attention tests against the oracle's attention_varlen (float32 arithmetic) and torch autograd through
    it: ragged lengths, GQA 3:1."""
    from oracle import titok_oracle as O
    from tests.blockwise import attention_reference
    cu, hq, hkv = [0, 70, 71, 200], 6, 2
    d, gq = hq * 64, hkv * 64
    g = torch.Generator().manual_seed(5)
    x = torch.randn(cu[-1], 2 * d + 2 * gq, generator=g)
    dout = torch.randn(cu[-1], d, generator=g)
    out, gated, lse, grad = attention_reference(x, dout, cu, hq, hkv)
    f = x.clone().requires_grad_(True)
    q, gt, k, v = f.split([d, d, gq, gq], dim=-1)
    ref = O.attention_varlen(q.unflatten(-1, (hq, 64)), k.unflatten(-1, (hkv, 64)), v.unflatten(-1, (hkv, 64)), cu).flatten(-2)
    ref.backward(dout)
    assert global_error(out, ref) < 1e-5
    assert global_error(gated, ref * torch.sigmoid(gt)) < 1e-5
    assert global_error(grad, f.grad) < 1e-4 and float(grad[:, d:2 * d].abs().max()) == 0.0
    for b in range(3):
        qq, kk = x[cu[b]:cu[b + 1], :d].double().view(-1, hq, 64), x[cu[b]:cu[b + 1], 2 * d:2 * d + gq].double().view(-1, hkv, 64)
        sc = torch.einsum("qhd,khd->hqk", qq, kk.repeat_interleave(hq // hkv, 1)) * 0.125
        assert float((lse[cu[b]:cu[b + 1]] - torch.logsumexp(sc, -1).T).abs().max()) < 1e-12


# the per-tile checker of the weight gradients (tests/test_hip_backward_bf16.py): the tiny tower's w12 gradient, 1408 x 256 = 11 x 2 tiles
TILE_TOL, W_GLOBAL_TOL = 1e-2, 1e-2


def _matrix(n=1408, k=256):
    g = torch.Generator().manual_seed(1)
    ref = torch.randn(n, k, generator=g)
    return ref * (1 + 1e-3 * torch.randn(ref.shape, generator=g)), ref


def test_tile_errors_cover_every_tile_with_short_edges():
    out, ref = _matrix(300, 136)                                      # 3 x 2 tiles, the last row / column of tiles short
    err = tile_errors(out, ref)
    assert err.shape == (3, 2) and float(err.max()) < 2e-3 and float(err.min()) > 5e-4
    bad = out.clone()
    bad[256:, 128:] *= 1.05                                           # the 44 x 8 corner tile alone
    err = tile_errors(bad, ref)
    assert float(err[2, 1]) > 0.04 and float(err[:2].max()) < 2e-3 and float(err[2, 0]) < 2e-3


@pytest.mark.parametrize("factor", [1.02, 0.0])
@pytest.mark.parametrize("where", [(0, 0), (5, 1), (10, 1)])             # (tile row, tile column); row 10: the short last row of tiles
def test_one_wrong_tile_is_rejected_where_the_global_bound_passes(factor, where):
    out, ref = _matrix()
    tn, tk = where
    bad = out.clone()
    bad[tn * 128:(tn + 1) * 128, tk * 128:(tk + 1) * 128] *= factor
    worst, glob = check_tiles(out, ref, TILE_TOL, W_GLOBAL_TOL)
    assert worst < 2e-3 and glob < 2e-3
    if factor:
        assert global_error(bad, ref) < W_GLOBAL_TOL                  # 2 % of one of 22 tiles: 0.4 % globally
    with pytest.raises(AssertionError, match="tile"):
        check_tiles(bad, ref, TILE_TOL, W_GLOBAL_TOL if factor else 1.0)
    err = tile_errors(bad, ref)
    assert float(err[tn, tk]) > TILE_TOL
    err[tn, tk] = 0
    assert float(err.max()) < 2e-3


def test_non_finite_matrix_is_rejected():
    out, ref = _matrix(256, 256)
    out[3, 200] = float("inf")
    with pytest.raises(AssertionError, match="non-finite"):
        check_tiles(out, ref, TILE_TOL, W_GLOBAL_TOL)


# ---------------------------------------------------------------------------------------------- the inference-forward helpers
def _ops_assert_close_figures(out, ref):
    """The two figures of tests/test_hip_ops.py assert_close (copied, not imported: that module needs the GPU library): relative
    Frobenius error over the whole output, and max-abs error as a fraction of max|ref|; bf16 bounds 3e-3 and 2e-2."""
    out, ref = out.double(), ref.double()
    return float((out - ref).norm() / (ref.norm() + 1e-30)), float((out - ref).abs().max()) / float(ref.abs().max() + 1e-30)


def _ops_assert_close_accepts(out, ref):
    r, m = _ops_assert_close_figures(out, ref)
    return bool(torch.isfinite(out.double()).all()) and r < 3e-3 and m <= 2e-2


F_CU = [1152 * i for i in range(33)]            # the benchmark batch: 32 sequences of 1152 rows, width 256 = 4 heads
F_BLOCK_TOL, F_GLOBAL_TOL = 6e-3, 4e-3          # FWD_TOL["bf16"] of tests/test_hip_backward_shapes.py


@pytest.fixture(scope="module")
def forward_pair():
    from tests.blockwise import bf16_store
    g = torch.Generator().manual_seed(2)
    ref = torch.randn(36864, 256, generator=g, dtype=torch.float64)
    ref[20000] *= 1e-3                                                # a row of 1/1000 of its neighbours' norm
    return bf16_store(ref), ref                                       # the best a bf16 kernel can do: the reference rounded once


def test_forward_pair_passes_every_check(forward_pair):
    from tests.blockwise import check_row_tiles, check_rows
    out, ref = forward_pair
    assert _ops_assert_close_accepts(out, ref)
    worst, glob = check_blockwise(out, ref, F_CU, 4, F_BLOCK_TOL, F_GLOBAL_TOL)
    assert worst < 2.5e-3 and glob < 2.5e-3
    worst, glob = check_row_tiles(out, ref, 16, 64, F_BLOCK_TOL, F_GLOBAL_TOL)
    assert worst < 2.5e-3
    assert check_rows(out, ref, [0, 20000, 36863], F_BLOCK_TOL) < 2.5e-3


def test_one_block_of_one_head_off_by_3_percent_passes_the_global_check_only(forward_pair):
    out, ref = forward_pair
    bad = out.clone()
    r0 = 1152 * 7 + 64 * 12                                           # sequence 7, block 12, head 0: block 7 * 18 + 12 = 138
    # (3 % of the output's very largest elements is what the max-abs figure does see; this block's largest is 0.61 of the global one)
    assert float(ref[r0:r0 + 64, :64].abs().max()) < 0.65 * float(ref.abs().max())
    bad[r0:r0 + 64, :64] *= 1.03
    assert _ops_assert_close_accepts(bad, ref)
    with pytest.raises(AssertionError, match="block 138 head 0"):
        check_blockwise(bad, ref, F_CU, 4, F_BLOCK_TOL, F_GLOBAL_TOL)


def test_one_16x64_tile_off_by_3_percent_passes_the_global_and_the_block_check(forward_pair):
    from tests.blockwise import check_row_tiles
    out, ref = forward_pair
    bad = out.clone()
    assert float(ref[36848:36864, 64:128].abs().max()) < 0.6 * float(ref.abs().max())      # (see the block test above)
    bad[36848:36864, 64:128] *= 1.03                                  # the last wave's 16 rows, second 64 columns
    assert _ops_assert_close_accepts(bad, ref)
    check_blockwise(bad, ref, F_CU, 4, 2e-2, F_GLOBAL_TOL)            # a quarter of a 64-row block: 1.5 % of it
    with pytest.raises(AssertionError, match="tile rows 36848..36863 columns 64..127"):
        check_row_tiles(bad, ref, 16, 64, F_BLOCK_TOL, F_GLOBAL_TOL)


def test_a_negated_row_of_small_norm_passes_everything_but_the_row_check(forward_pair):
    from tests.blockwise import check_row_tiles, check_rows
    out, ref = forward_pair
    bad = out.clone()
    bad[20000] = -bad[20000]
    assert _ops_assert_close_accepts(bad, ref)
    check_blockwise(bad, ref, F_CU, 4, F_BLOCK_TOL, F_GLOBAL_TOL)     # 200 % of 1e-3 of one row in 64: 2.5e-4 of the block
    check_row_tiles(bad, ref, 16, 64, F_BLOCK_TOL, F_GLOBAL_TOL)
    with pytest.raises(AssertionError, match="row 20000"):
        check_rows(bad, ref, [0, 20000, 36863], F_BLOCK_TOL)


def test_row_tiles_leave_out_rows_and_measure_a_ragged_last_tile():
    from tests.blockwise import check_row_tiles, row_tile_errors
    g = torch.Generator().manual_seed(3)
    ref = torch.randn(145, 128, generator=g, dtype=torch.float64)
    ref[20] *= 100.0
    out = ref * (1 + 1e-3 * torch.randn(ref.shape, generator=g, dtype=torch.float64))
    assert row_tile_errors(out, ref).shape == (10, 2)
    bad = out.clone()
    bad[21, :64] *= 1.5                                               # the neighbour of the x100 row: 0.5 % of its tile with that row in
    check_row_tiles(bad, ref, 16, 64, 6e-3, 4e-3)
    with pytest.raises(AssertionError, match="tile rows 16..31 columns 0..63"):
        check_row_tiles(bad, ref, 16, 64, 6e-3, 1.0, leave_out=[20])
    bad = out.clone()
    bad[144, 64:] *= 1.05                                             # the one-row last tile
    with pytest.raises(AssertionError, match="tile rows 144..144 columns 64..127"):
        check_row_tiles(bad, ref, 16, 64, 6e-3, 4e-3)


def test_check_rows_takes_one_bound_per_row_and_heads():
    from tests.blockwise import check_rows, row_errors
    g = torch.Generator().manual_seed(4)
    ref = torch.randn(10, 128, generator=g, dtype=torch.float64)
    ref[3] = 0.0
    out = ref.clone()
    out[7, 64:] *= 1.01
    assert row_errors(out, ref, [3, 7], heads=2).tolist() == [[0.0, 0.0], [0.0, pytest.approx(0.01)]]
    check_rows(out, ref, [3, 7], torch.tensor([1e-9, 2e-2]), heads=2)
    with pytest.raises(AssertionError, match="row 7 head 1"):
        check_rows(out, ref, [3, 7], torch.tensor([2e-2, 5e-3]), heads=2)
    out[3, 5] = 1e-30                                                 # anything but zero where the reference row is zero
    with pytest.raises(AssertionError, match="row 3"):
        check_rows(out, ref, [3], 1.0)


def test_attention_forward_reference_matches_attention_reference():
    """The chunked no-autograd forward against the autograd reference (ragged lengths, GQA 3:1, chunks smaller than a sequence), and
    its pre-scaled form: q carrying head_dim^-0.5 * log2(e) exactly (in float64) gives the same softmax through 2^x."""
    from tests import blockwise
    from tests.blockwise import attention_forward_reference, attention_reference
    from tests.forward_cases import C_EXP
    cu, hq, hkv = [0, 70, 71, 400], 6, 2
    d, gq = hq * 64, hkv * 64
    g = torch.Generator().manual_seed(6)
    x = torch.randn(cu[-1], 2 * d + 2 * gq, generator=g, dtype=torch.float64)
    out, gated, _, _ = attention_reference(x, torch.zeros(cu[-1], d), cu, hq, hkv)
    o1, g1 = attention_forward_reference(x, cu, hq, hkv)
    assert float((o1 - out).abs().max()) < 1e-13 and float((g1 - gated).abs().max()) < 1e-13
    xs = x.clone()
    xs[:, :d] *= C_EXP
    o2, g2 = attention_forward_reference(xs, cu, hq, hkv, c_exp=C_EXP)
    assert float((o2 - out).abs().max()) < 1e-13 and float((g2 - gated).abs().max()) < 1e-13
    assert (1 << 24) // (3 * 329) < 329 * 64                          # the 329-row sequence above was one chunk: force several
    old = blockwise.CHUNK_ELEMENTS
    blockwise.CHUNK_ELEMENTS = 3 * 329 * 100
    try:
        o3, _ = attention_forward_reference(x, cu, hq, hkv)
    finally:
        blockwise.CHUNK_ELEMENTS = old
    assert float((o3 - out).abs().max()) < 1e-13


_FLOOR_CASES = [(b, h) for b in ("bench", "five", "ragged", "far", "spikes6", "spikes30", "ragged_k") for h in ((4, 2), (8, 2), (12, 4))
                if h == (4, 2) or b not in ("bench", "five")]


@pytest.mark.parametrize("batch,heads", _FLOOR_CASES, ids=[f"{b}-{h[0]}_{h[1]}" for b, h in _FLOOR_CASES])
def test_no_forward_reference_block_is_under_the_floor(batch, heads):
    """The condition tests/test_hip_forward_shapes.py asserts before every launch, here on every attention batch but `base` (the
    benchmark-size ones at 4 / 2 heads only, for the suite's time; every head count is evaluated before the GPU launch), both operand sets, gated and ungated: block_errors would measure a floored block
    against the floor, not against itself."""
    from tests import forward_cases as FC
    from tests.blockwise import attention_forward_reference, floored_blocks
    hq, hkv = heads
    x, rows = FC.attention_inputs(batch, hq, hkv)
    cu = FC.cu_seqlens(batch)
    assert all(0 <= r < cu[-1] for r in rows)
    plain, scaled = FC.attention_operands(x, hq)
    for ops, c in ((plain, None), (scaled, FC.C_EXP)):
        for ref in attention_forward_reference(ops, cu, hq, hkv, c_exp=c):
            assert bool(torch.isfinite(ref).all())
            assert not bool(floored_blocks(ref, cu, hq).any())


def test_floored_blocks_names_what_block_errors_floors():
    from tests.blockwise import floored_blocks
    out, ref = _pair()
    ref = ref.clone()
    ref[CU[3] + 64:CU[3] + 128, 128:192] *= 1e-3
    mask = floored_blocks(ref, CU, HEADS)
    assert int(mask.sum()) == 1 and bool(mask[int(row_blocks(CU)[0][CU[3] + 64]), 2])


def test_dense_cases_have_the_rows_they_name():
    from tests import forward_cases as FC
    from titok_video_amd.plan import BatchPlan
    for M in FC.DENSE_M:
        assert BatchPlan(*FC.DENSE_PLANS[M], FC.PATCH, "cpu").total_rows == M
        rows = FC.planted_rows(M)
        assert len(rows) == 12 and min(rows) == 0 and max(rows) == M - 1 and 15 in rows
        assert sorted(rows.values()) == [0.0] * 4 + [1e-3] * 4 + [100.0] * 4
        assert len({rows[0], rows[15], rows[M - 1]}) == 3
