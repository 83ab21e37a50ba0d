"""tests/blockwise.py, the per-(sequence, head, 64-row block) checker of the attention tests and the per-128x128-tile checker of the
weight gradients: each must catch one wrong block or tile that the global relative error lets through."""
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
