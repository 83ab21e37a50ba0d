"""CPU checks of tests/wide_cases.py: the conditions the GPU tests of tests/test_hip_wide_layer.py rest on, evaluated on the same
inputs they launch - no reference tile under the floor of blockwise.block_errors, the planted rows where the tile edges are, the two
definitions of the post-norm's statistic far enough apart to be told apart, and the restated layer against the oracle's towers."""
import pytest
import torch

from oracle import titok_oracle as O
from tests import mx_cases as MC
from tests import wide_cases as WC
from tests.blockwise import bf16_store, global_error
from titok_video_amd.model.base.utils import geglu_inner_dim


@pytest.mark.parametrize("case", WC.GEMM_CASES, ids=WC.case_id)
def test_no_reference_tile_is_under_the_floor(case):
    ref = WC.reference(case)
    o = WC.operands(case)
    assert ref.shape == (case.M, WC.out_features(case)) and ref.dtype == torch.float64 and bool(torch.isfinite(ref).all())
    assert MC.floored_tiles(WC.pad64(ref), o["planted"]) == []
    zero = [r for r, k in o["planted"].items() if k == 0.0]
    assert bool((ref[zero] == 0).all()) and bool((o["x"][zero] == 0).all())
    assert bool((o["row_scale"][zero] == torch.tensor(WC.EPS ** -0.5, dtype=torch.float32)).all())
    if case.epi == "qkv":      # the four column blocks are whole 64-column tiles, so each is measured by tiles of its own
        assert all(a % 64 == 0 and b % 64 == 0 for a, b in WC.qkv_blocks(case.width).values())


def test_shapes_reach_every_tile_edge():
    assert [WC.out_features(WC.Case("qkv", w, 1)) for w in WC.WIDTHS] == [1280, 2048, 2560]
    assert [WC.out_features(WC.Case("geglu", w, 1)) for w in WC.WIDTHS] == [1376, 2048, 2752]
    for w in WC.WIDTHS:
        size = WC.SIZE[w]
        width, _layers, (hq, hkv) = O.model_dims(size)
        assert width == w and WC.GQA[w] == 64 * hkv
        assert WC.INNER[w] == geglu_inner_dim(w)
    # a one-row last tile under a full one for each token-tile height, several tiles, the smallest launch
    assert all(t + 1 in WC.MS for t in WC.TILES) and 1 in WC.MS and max(WC.MS) > 4 * max(WC.TILES)
    assert WC.INNER[512] % 64 and not WC.t256_takes(WC.Case("geglu", 512, 129)) and not WC.t256_takes(WC.Case("geglu", 1024, 129))
    assert WC.t256_takes(WC.Case("geglu", 768, 129)) and all(WC.t256_takes(WC.Case(e, w, 129)) for e in ("store", "qkv") for w in WC.WIDTHS)
    assert len(set(WC.GEMM_CASES)) == len(WC.GEMM_CASES) == 54 and WC.PADDED_LDY <= set(WC.GEMM_CASES)
    assert {c.epi for c in WC.PADDED_LDY} == {"store", "qkv", "geglu"}
    for M in WC.MS:
        assert WC.qkv_rope_table(M)[0].shape == (M, 30)


@pytest.mark.parametrize("M", WC.MS)
def test_planted_rows_sit_at_the_tile_edges(M):
    pl = WC.planted(M)
    if M == 1:
        assert pl == {}
        return
    assert all(0 <= r < M for r in pl)
    assert {0, 1, 2, M - 1, M - 2, M - 3, M // 2} <= set(pl)
    for t in WC.TILES:
        if M > t:
            assert t - 1 in pl, f"the last row of the first {t}-token tile is not planted"
            assert M - 1 in pl and (M - 1) // t >= 1
    assert {pl[r] for r in (0, 1, 2)} == {pl[r] for r in (M - 3, M - 2, M - 1)} == set(WC.KINDS)
    # the launch carries what it says: x 100, x 1e-3 and zero rows over rows a factor of two apart
    x = WC.operands(WC.Case("store", 512, M))["x"].double()
    rs = WC.rstd64(x)
    plain = [r for r in range(M - 1) if r not in pl and r + 1 not in pl and r % 7 != 6]
    ratio = rs[plain] / rs[[r + 1 for r in plain]]
    assert bool(((ratio > 1.6) & (ratio < 2.5)).all()), "neighbouring rows' statistics are not a factor of two apart"


@pytest.mark.parametrize("width", WC.WIDTHS)
@pytest.mark.parametrize("rows", WC.STAT_ROWS)
def test_the_two_definitions_of_the_post_norm_statistic_can_be_told_apart(rows, width):
    x, gain = WC.norm_inputs(rows, width)
    o = WC.norm_unrounded(x, gain)
    stored, unrounded = WC.rstd64(bf16_store(o)), WC.rstd64(o)
    apart = ((stored - unrounded).abs() / stored)
    assert float(apart.max()) >= 10 * WC.rstd_bound(width), (float(apart.max()), WC.rstd_bound(width))
    assert float(apart[0]) >= 10 * WC.rstd_bound(width) and bool((bf16_store(o)[0].abs() == 1).all())
    if rows > WC.ZERO_ROW:
        assert bool((o[WC.ZERO_ROW] == 0).all()) and abs(float(stored[WC.ZERO_ROW]) * WC.EPS ** 0.5 - 1) < 1e-12
    s = WC.stat_inputs(rows, width)
    assert s.shape == (rows, width) and (rows <= WC.ZERO_ROW or bool((s[WC.ZERO_ROW] == 0).all()))


def test_residual_cases_keep_both_terms():
    for N, K in WC.RESID_NK:
        assert K % 64 == 0 or K == 1376          # 1376: the register-staged kernel (no LDS-DMA, no 256 x 256 tiles)
        for alpha in WC.resid_alphas(N):
            x, w, r, ref = WC.resid_operands(N, K, 129, alpha)
            prod = x.double() @ w.double().T
            assert 0.5 < float(prod.norm() / (alpha * r.double()).norm()) < 2.0
    assert [WC.resid_alphas(n)[1] for n in (512, 768, 1024)] == [16.0, 24.0, 48.0]


@pytest.mark.parametrize("fold", [True, False], ids=["fold", "nofold"])
@pytest.mark.parametrize("size", ["small", "base"])
def test_the_wide_layer_restatement_without_rounding_is_the_oracle_s_encoder(size, fold):
    """encoder_stack at full depth with exact weights and no rounding re-associates the oracle's stack (fold: gain and q factor inside
    the weight, the statistic after the product; no fold: the q factor inside the weight, the norm in front) and nothing else: the
    oracle's z to 1e-4 (its norms, rotary and attention compute in float32), as tests/test_mx_cases_cpu.py does for the MX layer."""
    sd = {WC.PREFIX + k: v for k, v in WC.tower_state(size).items()}
    full = O.model_dims(size)[1]
    clips = [c.double() for c in WC.layer_clips("ragged")]
    counts = WC.LAYER_BATCHES["ragged"][1]
    with torch.no_grad():
        z_ref = O.encoder_forward(clips, counts, sd, size, prefix=WC.PREFIX)
        x, mask = WC.encoder_stack(size, "ragged", full, MC.identity, fold=fold, bf16_weights=False, sd=sd, clips=clips)
        z = WC.encoder_z(x, mask, sd)
    assert x.shape == (331, O.model_dims(size)[0]) and int(mask.sum()) == sum(counts) == z.shape[0]
    assert global_error(z, z_ref) < 1e-4
    if size == "small" and fold:
        # the truncated stacks the GPU test compares with: they run, the rounding model differs from the unrounded one, alpha is the
        # full depth's whatever depth runs (a two-layer stack under alpha = 4 is another function)
        a, _ = WC.encoder_stack(size, "ragged", 2)
        b, _ = WC.encoder_stack(size, "ragged", 2, MC.bf16_round)
        assert bool(torch.isfinite(a).all()) and 1e-4 < global_error(b, a) < 5e-2
        width, _, heads = O.model_dims(size)
        hs = WC.held_state(size)
        x0, cos, sin, cu, _m = MC.encoder_front(clips, counts, hs, size, MC.identity, prefix=WC.PREFIX)
        w = MC.mx_layer_weights(hs, WC.PREFIX + "model_layers.", 2, width, quant=False, last_plain=False, bf16_all=True)
        shallow = MC.mx_stack(x0, w, hs, WC.PREFIX + "model_layers.", 2, heads, cos, sin, cu, MC.identity)
        assert global_error(shallow, a) > 1e-2
