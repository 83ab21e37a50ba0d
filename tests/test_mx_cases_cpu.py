"""CPU checks of tests/mx_cases.py: the conditions the GPU tests of tests/test_hip_fp8_blocks.py rest on, evaluated on the same inputs
they launch - no reference tile under the floor of blockwise.block_errors, the tile height every shape is chosen for, the
power-of-two row of the post-norm cases, and the helpers against the oracle."""
import pytest
import torch

from oracle import fp8_oracle as F
from oracle import titok_oracle as O
from tests import mx_cases as MC


@pytest.mark.parametrize("case", MC.GEMM_CASES + MC.GEGLU_Q_CASES[2:], ids=MC.case_id)
def test_no_reference_tile_is_under_the_floor(case):
    ref = MC.reference(case)
    assert ref.shape == (case.M, case.N) and ref.dtype == torch.float64 and bool(torch.isfinite(ref).all())
    assert MC.floored_tiles(ref, MC.operands(case)["planted"]) == []


def test_every_case_is_unique_and_reaches_the_tile_height_it_names():
    cases = MC.GEMM_CASES + MC.GEGLU_Q_CASES
    assert len(set(MC.GEMM_CASES)) == len(MC.GEMM_CASES)
    for c in cases:
        assert MC.token_tile(c.M, c.N, c.epi) == c.tile, c
    # both heights for every flavour and epilogue, a ragged last tile under a full one, and the two k depths the scale prefetch has
    for f, e in {(c.flavour, c.epi) for c in cases}:
        assert {c.tile for c in cases if (c.flavour, c.epi) == (f, e)} == {128, 160}, (f, e)
    assert all(c.M % c.tile for c in cases) and any(c.M > c.tile for c in cases)
    assert {c.K // 128 for c in MC.GEMM_CASES if c.flavour == "mx"} == {6, 16}
    for M, (shapes, counts) in MC.QKV_PLANS.items():
        assert MC.qkv_rope_table(M)[0].shape == (M, 30)


def test_planted_rows_are_planted_before_quantisation():
    c = MC.Case("mx", "store", 300, 2048, 768, 128)
    o = MC.operands(c)
    zero = [r for r, k in o["planted"].items() if k == 0.0]
    assert len(o["planted"]) == 12 and len(zero) == 4
    assert bool((o["x"][zero] == 0).all()) and bool((o["xq"][zero] & 0x7F == 0).all()) and bool((o["xe"][zero] == 127).all())
    assert bool((MC.reference(c)[zero] == 0).all())
    assert MC.planted(1) == {}


def test_rows_quantize_is_the_row_scaled_format():
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(37, 256, generator=g) * torch.rand(37, 1, generator=g) * 5).to(torch.bfloat16)
    x[4] = 0
    q, sc = MC.rows_quantize(x)
    assert float(sc[4]) == 1.0 and bool((q[4] == 0).all())
    xf = x.double()
    deq = MC.rows_dequantize(q, sc)
    assert float(((deq - xf).abs() / (xf.abs() + sc.double()[:, None] * 2.0 ** -6)).max()) <= 2 ** -4 + 1e-6      # half an e4m3 ulp
    assert float(deq.abs().amax(1).div(xf.abs().amax(1).clamp_min(1e-30))[torch.arange(37) != 4].sub(1).abs().max()) < 1e-6


def test_rotary64_is_the_oracle_s_rotary():
    g = torch.Generator().manual_seed(1)
    cos, sin = MC.qkv_rope_table(300)
    x = torch.randn(300, 4 * 64, generator=g)
    want = O.apply_rotary(x.reshape(300, 4, 64), cos, sin).reshape(300, -1)          # float32 math inside
    got = MC.rotary64(x, cos, sin)
    assert got.dtype == torch.float64 and float((got - want.double()).abs().max()) < 1e-5
    assert torch.equal(got.reshape(300, 4, 64)[..., 60:], x.double().reshape(300, 4, 64)[..., 60:])      # the last two pairs stay


@pytest.mark.parametrize("width", MC.NORM_WIDTHS)
def test_the_power_of_two_row_yields_exact_powers_of_two(width):
    x, gain = MC.norm_inputs(131, width, "pow2")
    assert bool((x[MC.POW2_ROW].abs() == 2.0 ** MC.POW2_A).all())
    y = MC.norm_stored(x, gain)[MC.POW2_ROW].float()
    assert torch.equal(y.abs(), gain), "the stored row is not exactly +-448 * 2^k"
    t = (y.abs().view(-1, 32).amax(1) * torch.tensor(1.0 / 448.0)).float()           # the fp32 product of the scale rule
    m, e = torch.frexp(t)
    assert bool((m == 0.5).all()), "a block maximum / 448 is not an exact power of two"
    k = torch.log2(gain.view(-1, 32)[:, 0] / 448.0).round().int()
    q, e8, _ = F.mx_quantize(y.to(torch.bfloat16)[None])
    assert torch.equal(e8[0].int() - 127, k), "the exponent was not kept"
    assert bool(((q & 0x7F) == 0x7E).all()), "every element is +-448 of its block"
    assert k.min() >= -6 and k.max() <= 5 and (width < 256 or len(set(k.tolist())) > 1)
    # the other special rows are there
    assert bool((x[3] == 0).all()) and bool((x[5, 32:64] == 0).all()) and bool((x[5, :32] != 0).any())


@pytest.mark.parametrize("size", ["tiny", "base"])
def test_the_mx_layer_restatement_without_quantisation_is_the_oracle_s_towers(size):
    """mx_encoder_forward / mx_decoder_forward with quantisation and rounding switched off re-associate the oracle's stack (gain and q
    factor inside the weight, rstd after the product, softmax 2^(q . k)) and nothing else.  The oracle's norms, rotary and attention
    compute in float32 whatever they are given, so the two agree to float32 accuracy through the layers, not to float64's: 1e-4
    relative (a mis-composed layer - a gain applied twice, a missing q factor, alpha on layer 0 - is off by tens of per cent)."""
    from titok_video_amd.synthetic import seeded_titok_state, synthetic_clips
    from tests.blockwise import global_error
    levels = [8, 8, 8, 6, 5]
    sd = seeded_titok_state(3, size, size, gain=3.0)
    shapes, counts = [(4, 16, 16), (8, 16, 24), (4, 32, 16)], [16, 24, 20]
    clips = [c.double() for c in synthetic_clips(shapes, seed=13)]
    with torch.no_grad():
        z_ref = O.encoder_forward(clips, counts, sd, size, prefix="encoder.")
        z = MC.mx_encoder_forward(clips, counts, sd, size, quant=False)
        assert z.dtype == torch.float64 and z.shape == z_ref.shape == (60, 5)
        assert global_error(z, z_ref) < 1e-4
        codes = O.fsq_forward(z_ref.float(), levels)[0].double()
        rec_ref = O.decoder_forward(codes, counts, shapes, sd, size, prefix="decoder.")
        rows, sizes = MC.mx_decoder_forward(codes, counts, shapes, sd, size, quant=False)
        assert sizes == [(t // 4) * (h // 8) * (w // 8) for t, h, w in shapes]
        for chunk, shape, ref in zip(torch.split(rows, sizes), shapes, rec_ref):
            got = O.unpatchify(chunk, [v // p for v, p in zip(shape, (4, 8, 8))], (4, 8, 8), 3)
            assert global_error(got, ref) < 1e-4
        # with quantisation on the same call takes the other branch of every linear (images, mx(operand)): it must run and differ
        if size == "tiny":
            zq = MC.mx_encoder_forward(clips, counts, sd, size, quant=True)
            assert bool(torch.isfinite(zq).all()) and not torch.equal(zq, z)
