"""Mixed bf16 / fp8 linears (BASELINE config #5: "mixed bf16/fp8 MFMA"; not a reference feature - the reference runs bf16 autocast).
`-m gpu`.  Stated tolerance: OCP e4m3 keeps 3 mantissa bits (relative rounding error <= 2^-4 per element); with one scale per token /
per weight row and K >= 768 the fp8 projections differ from the bf16 ones by a few per cent (relative Frobenius error < 5e-2, asserted
below); the kernel itself is exact arithmetic on the quantised operands (fp32 accumulation) and is checked tightly against float64."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import titok_oracle as O
from titok_video_amd import _lib
from titok_video_amd.model.titok import TiTok
from titok_video_amd.synthetic import seeded_titok_state, synthetic_clips

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def quant(x, gain=None, eps=1e-5):
    lib, S = _lib.lib(), _lib.stream_ptr(torch.device(DEV))
    q = torch.empty(x.shape, dtype=torch.uint8, device=DEV)
    sc = torch.empty(x.shape[0], dtype=torch.float32, device=DEV)
    _lib.check(lib.ttv_quant_rows_fp8(x.data_ptr(), _lib.dtype_code(x.dtype), x.shape[1], _lib.ptr(gain), eps, q.data_ptr(), x.shape[1], sc.data_ptr(),
                                      x.shape[0], x.shape[1], S), "quant")
    return q, sc


def dequant(q, sc):
    return q.view(torch.float8_e4m3fn).float() * sc[:, None]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_quant_rows_fp8(dtype):
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(333, 768, generator=g) * torch.rand(333, 1, generator=g) * 5).to(dtype).to(DEV)
    x[7] = 0
    q, sc = quant(x)
    xf = x.float()
    ref_sc = xf.abs().amax(1) / 448.0
    ref_sc[7] = 1.0
    assert torch.allclose(sc, ref_sc, rtol=1e-6, atol=0)
    ref_q = (xf / sc[:, None]).to(torch.float8_e4m3fn)                      # round-to-nearest-even, OCP e4m3
    assert torch.equal(q, ref_q.view(torch.uint8))
    err = (dequant(q, sc) - xf).abs()
    assert float((err / (xf.abs() + sc[:, None] * 2 ** -6)).max()) <= 2 ** -4 + 1e-6    # <= half an e4m3 ulp relative (subnormals: absolute)
    # with the RMSNorm in front (what the tower does): quantises round_to_dtype(x * rstd * gain)
    gain = (1 + 0.1 * torch.randn(768, generator=g)).to(DEV)
    q2, sc2 = quant(x[:64], gain)
    y = (x[:64].float() * torch.rsqrt(x[:64].float().pow(2).mean(1, keepdim=True) + 1e-5) * gain).to(dtype).float()
    y_sc = y.abs().amax(1) / 448.0
    y_sc[7] = 1.0
    assert torch.allclose(sc2, y_sc, rtol=2e-2 if dtype == torch.bfloat16 else 1e-5)
    assert float((dequant(q2, sc2) - y).norm() / y.norm()) < 4e-2


@pytest.mark.parametrize("M,N,K", [(1000, 2048, 768), (36864, 768, 768), (333, 256, 128)])
def test_linear_fp8_is_exact_on_the_quantised_operands(M, N, K):
    lib, S = _lib.lib(), _lib.stream_ptr(torch.device(DEV))
    g = torch.Generator().manual_seed(M + N)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16).to(DEV)
    xq, xs = quant(x)
    wq, wsc = quant(w)
    y = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    _lib.check(lib.ttv_linear_fp8(xq.data_ptr(), K, xs.data_ptr(), wq.data_ptr(), K, wsc.data_ptr(), y.data_ptr(), N, M, N, K, 0, None, 0, 0, S), "fp8")
    rows = torch.arange(0, M, max(1, M // 512), device=DEV)
    ref = dequant(xq[rows], xs[rows]).double() @ dequant(wq, wsc).double().t()
    got = y[rows].double()
    assert float((got - ref).norm() / ref.norm()) < 3e-3                     # bf16 output rounding only
    bf = (x[rows].double() @ w.double().t())
    rel = float((got - bf).norm() / bf.norm())
    print(f"fp8 linear {M}x{N}x{K}: rel. error vs the unquantised product {rel:.4f}")
    assert rel < 5e-2                                                        # the stated fp8 tolerance


def test_linear_fp8_geglu_and_qkv_epilogues():
    lib, S = _lib.lib(), _lib.stream_ptr(torch.device(DEV))
    from titok_video_amd.plan import BatchPlan
    g = torch.Generator().manual_seed(5)
    plan = BatchPlan([(8, 32, 48), (4, 16, 16)], [40, 24], (4, 8, 8), DEV)
    M, d, gq, I = plan.total_rows, 768, 256, 2048
    x = torch.randn(M, d, generator=g).to(torch.bfloat16).to(DEV)
    xq, xs = quant(x)
    xd = dequant(xq, xs).double()
    # GEGLU: w [2I, d]
    w12 = (torch.randn(2 * I, d, generator=g) * d ** -0.5).to(torch.bfloat16).to(DEV)
    wq, wsc = quant(w12)
    h = torch.empty(M, I, dtype=torch.bfloat16, device=DEV)
    _lib.check(lib.ttv_linear_fp8(xq.data_ptr(), d, xs.data_ptr(), wq.data_ptr(), d, wsc.data_ptr(), h.data_ptr(), I, M, I, d, 2, None, 0, 0, S), "geglu")
    u = xd @ dequant(wq, wsc).double().t()
    ref = torch.nn.functional.gelu(u[:, I:]) * u[:, :I]
    assert float((h.double() - ref).norm() / ref.norm()) < 4e-3
    # to_qkv + rotary
    nq = 2 * d + 2 * gq
    wqkv = (torch.randn(nq, d, generator=g) * d ** -0.5).to(torch.bfloat16).to(DEV)
    wq2, ws2 = quant(wqkv)
    y = torch.empty(M, nq, dtype=torch.bfloat16, device=DEV)
    _lib.check(lib.ttv_linear_fp8(xq.data_ptr(), d, xs.data_ptr(), wq2.data_ptr(), d, ws2.data_ptr(), y.data_ptr(), nq, M, nq, d, 1,
                                  plan.rope_cs.data_ptr(), d, gq, S), "qkv")
    acc = (xd @ dequant(wq2, ws2).double().t()).float()
    cs = plan.rope_cs.cpu()
    ref = acc.cpu().clone()
    for lo, hi in ((0, d), (2 * d, 2 * d + gq)):
        blk = ref[:, lo:hi].reshape(M, -1, 64)
        blk = O.apply_rotary(blk, cs[:, :32], cs[:, 32:])
        ref[:, lo:hi] = blk.reshape(M, -1)
    assert float((y.float().cpu() - ref).norm() / ref.norm()) < 4e-3


def test_base_towers_with_fp8_linears_stay_within_the_stated_tolerance():
    """Whole base-size towers with the QKV and W12 projections on the fp8 MFMA, against the same towers in bf16 and against the fp32
    oracle.  Stated end-to-end tolerance (measured 0.18 / 0.09 on these seeded weights): mean |pre-rounding FSQ value error| < 0.25 -
    five times the bf16 path's, i.e. an fp8 ENCODER does not preserve token indices (3 of 4 tokens change on this model; twelve KEEL
    layers scale the residual stream by alpha = 24 before every post-norm) - and decoder reconstructions within 12 % relative.  The option
    is therefore off by default and meant for throughput runs (config #5) and decoders."""
    levels = [8, 8, 8, 6, 5]
    cfg = SimpleNamespace(tokenizer=SimpleNamespace(model=SimpleNamespace(patch_size=[4, 8, 8], fsq_levels=levels, encoder_size="base", decoder_size="base")))
    sd = seeded_titok_state(3, "base", "base", gain=3.0)
    shapes, counts = [(4, 16, 16), (8, 16, 24), (4, 32, 16)], [16, 24, 20]
    clips_cpu = synthetic_clips(shapes, seed=13)
    with torch.no_grad():
        ref_recon, ref_idx, _z, ref_b = O.titok_forward(clips_cpu, counts, sd, levels, "base", "base")
    res = {}
    for f8 in (False, True):
        m = TiTok(cfg)
        m.load_state_dict(sd, strict=True)
        m = m.to(DEV, torch.bfloat16).eval()
        m.encoder.fp8_linears = m.decoder.fp8_linears = f8
        clips = [c.to(DEV, torch.bfloat16) for c in clips_cpu]
        with torch.no_grad():
            codes, od = m.encode(clips, counts, want_bounded=True)
            recon = m.decode(O.fsq_indices_to_codes(ref_idx, levels).to(DEV, torch.bfloat16), counts, shapes)
        res[f8] = (m.last_bounded.cpu(), od["indices"].cpu(), torch.cat([r.float().cpu().flatten() for r in recon]))
    ref_flat = torch.cat([r.flatten() for r in ref_recon])
    e16 = float((res[False][0] - ref_b).abs().mean())
    e8 = float((res[True][0] - ref_b).abs().mean())
    r16 = float((res[False][2] - ref_flat).norm() / ref_flat.norm())
    r8 = float((res[True][2] - ref_flat).norm() / ref_flat.norm())
    print(f"base towers: mean |bounded err| bf16 {e16:.4f} | bf16+fp8 {e8:.4f}; index mismatches vs fp32 bf16 {int((res[False][1] != ref_idx).sum())} | "
          f"bf16+fp8 {int((res[True][1] != ref_idx).sum())} of {ref_idx.numel()}; decoder rel. error bf16 {r16:.4f} | bf16+fp8 {r8:.4f}")
    assert not torch.equal(res[False][0], res[True][0])          # the fp8 path really ran
    assert e8 < 0.25 and r8 < 0.12


# ---- block-scaled (MX) e4m3: round 4 ----------------------------------------------------------------------------------------------
def quant_mx(x, row_scaled=False):
    lib, S = _lib.lib(), _lib.stream_ptr(torch.device(DEV))
    rows, K = x.shape
    q = torch.empty((rows, K), dtype=torch.uint8, device=DEV)
    mx = torch.zeros((rows, int(lib.ttv_mx_scale_bytes_per_row(K))), dtype=torch.uint8, device=DEV)
    rs = torch.empty(rows, dtype=torch.float32, device=DEV) if row_scaled else None
    _lib.check(lib.ttv_quant_mx_fp8(x.data_ptr(), _lib.dtype_code(x.dtype), x.stride(0), q.data_ptr(), K, mx.data_ptr(), _lib.ptr(rs), rows, K, S), "quant_mx")
    return q, mx, rs


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("K", [128, 768, 2048])
@pytest.mark.parametrize("row_scaled", [False, True])
def test_quant_mx_fp8_matches_the_oracle_bit_for_bit(dtype, K, row_scaled):
    """Elements, E8M0 bytes (in the library's lane-major layout) and row factors of k_quant_mx_fp8 against oracle/fp8_oracle.py: rows
    with blocks 1e-4 .. 1e4 apart (the case block scales exist for), an all-zero row, an all-zero block, exact powers of two."""
    from oracle import fp8_oracle as F
    g = torch.Generator().manual_seed(K + int(row_scaled))
    rows = 131
    x = torch.randn(rows, K, generator=g) * torch.exp(4 * torch.randn(rows, K // 32, generator=g)).repeat_interleave(32, 1)
    x[3] = 0
    x[5, 32:64] = 0
    x[6] = 448.0 * 2.0 ** torch.randint(-6, 6, (K,), generator=g).float()
    x = x.to(dtype)
    q, mx, rs = quant_mx(x.to(DEV), row_scaled)
    rq, re, rrs = F.mx_quantize(x, row_scaled)
    if row_scaled:
        assert torch.equal(rs.cpu(), rrs)
    assert torch.equal(mx.cpu(), F.mx_scale_layout(re))
    assert torch.equal(q.cpu(), rq)
    # and the format's accuracy, wherever a block's scale leaves the element in e4m3's normal range: half an ulp = 2^-4 relative
    deq = F.mx_dequantize(rq, re, rrs)
    xf = x.double()
    blk_floor = (2.0 ** (re.double() - 127 - 6)).repeat_interleave(32, 1) * (rrs.double()[:, None] if row_scaled else 1.0)
    assert float(((deq - xf).abs() / (xf.abs() + blk_floor)).max()) <= 2 ** -4 + 1e-6


@pytest.mark.parametrize("M,N,K", [(1000, 1024, 768), (300, 768, 2048), (36864, 256, 128), (129, 640, 1664)])
def test_linear_fp8_mx_is_exact_on_the_quantised_operands(M, N, K):
    """k_gemm_fp8_dma<.., MX>: the block scales reach the right lanes of v_mfma_scale_f32_16x16x128_f8f6f4 (data with block maxima
    spread over 2^±6, so a scale applied to the wrong block is an error of orders of magnitude) - against the float64 product of the
    dequantised operands; row factors on both sides / on neither."""
    from oracle import fp8_oracle as F
    lib, S = _lib.lib(), _lib.stream_ptr(torch.device(DEV))
    g = torch.Generator().manual_seed(M + N + K)
    spread = lambda r: torch.exp2(torch.randint(-6, 7, (r, K // 32), generator=g).float()).repeat_interleave(32, 1)
    x = (torch.randn(M, K, generator=g) * spread(M)).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) * spread(N) * K ** -0.5).to(torch.bfloat16)
    xq, xmx, _ = quant_mx(x.to(DEV))
    wq, wmx, wrs = quant_mx(w.to(DEV), True)
    xrs = (0.5 + torch.rand(M, generator=g)).to(DEV)
    rq, re, _ = F.mx_quantize(x)
    wq_o, we_o, wrs_o = F.mx_quantize(w, True)
    assert torch.equal(xq.cpu(), rq) and torch.equal(wq.cpu(), wq_o)
    rows = torch.arange(0, M, max(1, M // 256))
    xd = F.mx_dequantize(rq[rows], re[rows])
    wd = F.mx_dequantize(wq_o, we_o, wrs_o)
    for use_rows in (True, False):
        y = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
        wq2, wmx2, _ = (wq, wmx, None) if use_rows else quant_mx(w.to(DEV), False)
        _lib.check(lib.ttv_linear_fp8_mx(xq.data_ptr(), K, xmx.data_ptr(), xrs.data_ptr() if use_rows else None, wq2.data_ptr(), K, wmx2.data_ptr(),
                                         wrs.data_ptr() if use_rows else None, y.data_ptr(), N, M, N, K, 0, None, 0, 0, None, 0, 0.0, S), "fp8_mx")
        if use_rows:
            ref = (xd * xrs.cpu().double()[rows, None]) @ wd.t()
        else:
            w2q, w2e, _ = F.mx_quantize(w)
            ref = xd @ F.mx_dequantize(w2q, w2e).t()
        got = y.cpu()[rows].double()
        assert float((got - ref).norm() / ref.norm()) < 3e-3, use_rows       # the bf16 rounding of the output only
        assert float(((got - ref).abs() / (ref.abs() + 1e-2 * ref.abs().mean())).max()) < 2e-2


def test_linear_fp8_mx_epilogues():
    """GEGLU, to_qkv + rotary and the residual epilogue (alpha * resid + acc, in place) on block-scaled operands."""
    from oracle import fp8_oracle as F
    from titok_video_amd.plan import BatchPlan
    lib, S = _lib.lib(), _lib.stream_ptr(torch.device(DEV))
    g = torch.Generator().manual_seed(9)
    plan = BatchPlan([(8, 32, 48), (4, 16, 16)], [40, 24], (4, 8, 8), DEV)
    M, d, gq, I = plan.total_rows, 768, 256, 2048
    x = torch.randn(M, d, generator=g).to(torch.bfloat16)
    xq, xmx, _ = quant_mx(x.to(DEV))
    rq, re, _ = F.mx_quantize(x)
    xd = F.mx_dequantize(rq, re)

    def weight(n, k):
        w = (torch.randn(n, k, generator=g) * k ** -0.5).to(torch.bfloat16)
        q, mx, rs = quant_mx(w.to(DEV), True)
        return (q, mx, rs), F.mx_dequantize(*F.mx_quantize(w, True))
    (wq, wmx, wrs), wd = weight(2 * I, d)
    h = torch.empty(M, I, dtype=torch.bfloat16, device=DEV)
    _lib.check(lib.ttv_linear_fp8_mx(xq.data_ptr(), d, xmx.data_ptr(), None, wq.data_ptr(), d, wmx.data_ptr(), wrs.data_ptr(), h.data_ptr(), I, M, I, d, 2,
                                     None, 0, 0, None, 0, 0.0, S), "geglu")
    u = xd @ wd.t()
    ref = torch.nn.functional.gelu(u[:, I:]) * u[:, :I]
    assert float((h.cpu().double() - ref).norm() / ref.norm()) < 4e-3
    # to_qkv + rotary
    nq = 2 * d + 2 * gq
    (wq, wmx, wrs), wd = weight(nq, d)
    y = torch.empty(M, nq, dtype=torch.bfloat16, device=DEV)
    _lib.check(lib.ttv_linear_fp8_mx(xq.data_ptr(), d, xmx.data_ptr(), None, wq.data_ptr(), d, wmx.data_ptr(), wrs.data_ptr(), y.data_ptr(), nq, M, nq, d, 1,
                                     plan.rope_cs.data_ptr(), d, gq, None, 0, 0.0, S), "qkv")
    ref = (xd @ wd.t()).float()
    cs = plan.rope_cs.cpu()
    for lo, hi in ((0, d), (2 * d, 2 * d + gq)):
        ref[:, lo:hi] = O.apply_rotary(ref[:, lo:hi].reshape(M, -1, 64), cs[:, :32], cs[:, 32:]).reshape(M, -1)
    assert float((y.float().cpu() - ref).norm() / ref.norm()) < 4e-3
    # w3-shaped: K = 2048 -> d, y = 24 * resid + acc written over resid
    hq_in = torch.randn(M, I, generator=g).to(torch.bfloat16)
    hq, hmx, _ = quant_mx(hq_in.to(DEV))
    hd = F.mx_dequantize(*F.mx_quantize(hq_in)[:2])
    (wq, wmx, wrs), wd = weight(d, I)
    resid = torch.randn(M, d, generator=g).to(torch.bfloat16)
    yr = resid.clone().to(DEV)
    _lib.check(lib.ttv_linear_fp8_mx(hq.data_ptr(), I, hmx.data_ptr(), None, wq.data_ptr(), I, wmx.data_ptr(), wrs.data_ptr(), yr.data_ptr(), d, M, d, I, 3,
                                     None, 0, 0, yr.data_ptr(), d, 24.0, S), "resid")
    ref = 24.0 * resid.double() + hd @ wd.t()
    assert float((yr.cpu().double() - ref).norm() / ref.norm()) < 4e-3


def _base_cfg(levels):
    return SimpleNamespace(tokenizer=SimpleNamespace(model=SimpleNamespace(patch_size=[4, 8, 8], fsq_levels=levels, encoder_size="base", decoder_size="base")))


def test_base_towers_with_mx_fp8_linears_stay_within_the_stated_tolerance():
    """Whole base-size towers with ALL FOUR linears of every layer on the block-scaled fp8 MFMA (`fp8_linears = "mx"`), against the bf16
    towers and the fp32 oracle.  Stated tolerance: e4m3 keeps 3 mantissa bits whatever the scale granularity, so the error is that of
    round 2's row-scaled pair plus the two added linears': mean |pre-rounding FSQ value error| < 0.30, decoder reconstructions within
    15 % relative - token indices are NOT preserved (printed)."""
    levels = [8, 8, 8, 6, 5]
    cfg = _base_cfg(levels)
    sd = seeded_titok_state(3, "base", "base", gain=3.0)
    shapes, counts = [(4, 16, 16), (8, 16, 24), (4, 32, 16)], [16, 24, 20]
    clips_cpu = synthetic_clips(shapes, seed=13)
    with torch.no_grad():
        ref_recon, ref_idx, _z, ref_b = O.titok_forward(clips_cpu, counts, sd, levels, "base", "base")
    res = {}
    for mode in (False, True, "mx"):
        m = TiTok(cfg)
        m.load_state_dict(sd, strict=True)
        m = m.to(DEV, torch.bfloat16).eval()
        m.encoder.fp8_linears = m.decoder.fp8_linears = mode
        clips = [c.to(DEV, torch.bfloat16) for c in clips_cpu]
        with torch.no_grad():
            codes, od = m.encode(clips, counts, want_bounded=True)
            recon = m.decode(O.fsq_indices_to_codes(ref_idx, levels).to(DEV, torch.bfloat16), counts, shapes)
        res[mode] = (m.last_bounded.cpu(), od["indices"].cpu(), torch.cat([r.float().cpu().flatten() for r in recon]))
    ref_flat = torch.cat([r.flatten() for r in ref_recon])
    for mode in res:
        e = float((res[mode][0] - ref_b).abs().mean())
        r = float((res[mode][2] - ref_flat).norm() / ref_flat.norm())
        print(f"base towers, fp8_linears={mode!s:5}: mean |bounded err| {e:.4f}; index mismatches vs fp32 {int((res[mode][1] != ref_idx).sum())} of "
              f"{ref_idx.numel()}; decoder rel. error {r:.4f}")
    assert not torch.equal(res[False][0], res["mx"][0]) and not torch.equal(res[True][0], res["mx"][0])      # the MX path really ran
    assert float((res["mx"][0] - ref_b).abs().mean()) < 0.30
    assert float((res["mx"][2] - ref_flat).norm() / ref_flat.norm()) < 0.15


# 84 rows: one partial token tile per GEMM, one query block and one key tile per sequence.  4 112 rows: to_qkv and w12 take the 160-token
# tile of k_gemm_fp8_dma, out_proj and w3 the 128-token tile; the sequences span nine query blocks and eighteen key tiles.  2 120 rows:
# only w12 takes the 160-token tile; a sequence of 968 rows ends inside a query block.
FUSED_BATCHES = {
    "84rows": ([(4, 16, 16), (8, 16, 24), (4, 32, 16)], [16, 24, 20]),
    "4112rows": ([(16, 128, 128)] * 3 + [(16, 64, 64)], [128] * 3 + [400]),
    "2120rows": ([(16, 128, 128), (16, 128, 96)], [128, 200]),
}


@pytest.mark.parametrize("batch", list(FUSED_BATCHES))
def test_mx_quantisation_fused_into_the_producers_is_bit_identical(batch):
    """run_layer_mx writes the block-scaled image of x from the KEEL post-norm kernel, of the attention output from the attention
    epilogue and of h from the w12 GEMM's GEGLU epilogue; with ttv_debug_set bit 11 every operand is quantised by a pass of its own.
    Same values, same blocks, same rounding: the towers' outputs must be equal bit for bit - z, indices and reconstructions, and the
    encoder's z with its last layer on the MX path as well (DBG_ENC_ALL_ROWS)."""
    levels = [8, 8, 8, 6, 5]
    sd = seeded_titok_state(3, "base", "base", gain=3.0)
    shapes, counts = FUSED_BATCHES[batch]
    assert sum(k + (t // 4) * (h // 8) * (w // 8) for (t, h, w), k in zip(shapes, counts)) == int(batch[:-4])
    clips = [c.to(DEV, torch.bfloat16) for c in synthetic_clips(shapes, seed=13)]
    m = TiTok(_base_cfg(levels))
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV, torch.bfloat16).eval()
    m.encoder.fp8_linears = m.decoder.fp8_linears = "mx"
    outs = []
    for bit in (0, _lib.DBG_MX_UNFUSED_QUANT):
        _lib.lib().ttv_debug_set(bit)
        try:
            with torch.no_grad():
                z = m.encoder.run(clips, counts, None, None, want_z=True)["z"].clone()
                recon, info = m(clips, counts)
                _lib.lib().ttv_debug_set(bit | _lib.DBG_ENC_ALL_ROWS)
                z_all = m.encoder.run(clips, counts, None, None, want_z=True)["z"].clone()
            torch.cuda.synchronize()
        finally:
            _lib.lib().ttv_debug_set(0)
        outs.append((z, [r.clone() for r in recon], info["indices"].clone(), z_all))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][2], outs[1][2])
    assert all(torch.equal(a, b) for a, b in zip(outs[0][1], outs[1][1]))
    assert torch.equal(outs[0][3], outs[1][3])
    assert not torch.equal(outs[0][0], outs[0][3])      # the all-rows forward really took the MX kernels in the last layer


def test_mx_tower_layer_off_the_mx_path_reads_the_folded_bf16_weights_not_the_mx_images():
    """A layer of an MX tower that does not run run_layer_mx - the encoder's last layer, which works on the latent rows only
    (ttv_batch.qblocks_latent) - must take its projections from the folded bf16 weights: the e4m3 pointers of an MX tower hold the
    BLOCK-scaled image of W * gain, which the row-scaled GEMM of the generic path would read with the pre-norm gain applied twice and the
    E8M0 block scales dropped (round-4 advisor finding).  Synthetic weights hide that (gains 1 +- 0.1, blocks of equal magnitude), so this
    test gives the last encoder layer pre-norm gains around 2 and outlier input channels (a 32-column block 8x larger than its
    neighbours: block exponents differ by 3) and compares the latent-rows forward with the all-rows, all-MX forward (ttv_debug_set
    bit 19) and with the fp32 oracle.  The two differ by one layer's e4m3 noise; the misuse would be a factor ~2."""
    levels = [8, 8, 8, 6, 5]
    sd = seeded_titok_state(3, "base", "base", gain=3.0)
    last = 11
    g = torch.Generator().manual_seed(5)
    for name in (f"encoder.model_layers.attn_layer.{last}.pre_ln.weight", f"encoder.model_layers.ffd_layer.{last}.norm.weight"):
        sd[name] = sd[name] * (2.0 + 0.5 * torch.rand(sd[name].shape, generator=g))
    for name in (f"encoder.model_layers.attn_layer.{last}.to_qkv.weight", f"encoder.model_layers.ffd_layer.{last}.w12.weight"):
        w = sd[name].clone()
        w[:, 64:96] *= 8.0            # one 32-column block of every row: its E8M0 scale sits 3 above the row's other blocks
        w[:, 400:432] *= 0.125
        sd[name] = w
    shapes, counts = [(4, 16, 16), (8, 16, 24), (4, 32, 16)], [16, 24, 20]
    clips_cpu = synthetic_clips(shapes, seed=13)
    with torch.no_grad():
        _recon, _idx, _zq, ref_b = O.titok_forward(clips_cpu, counts, sd, levels, "base", "base")
    m = TiTok(_base_cfg(levels))
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV, torch.bfloat16).eval()
    m.encoder.fp8_linears = m.decoder.fp8_linears = "mx"
    clips = [c.to(DEV, torch.bfloat16) for c in clips_cpu]
    outs = {}
    for bits in (0, 1 << 19):      # _lib.DBG_ENC_ALL_ROWS (the results below are keyed by the value)
        _lib.lib().ttv_debug_set(bits)
        try:
            with torch.no_grad():
                m.encode(clips, counts, want_bounded=True)
            torch.cuda.synchronize()
        finally:
            _lib.lib().ttv_debug_set(0)
        outs[bits] = m.last_bounded.float().cpu()
    e_lat = float((outs[0] - ref_b).abs().mean())
    e_all = float((outs[1 << 19] - ref_b).abs().mean())
    d = float((outs[0] - outs[1 << 19]).abs().mean())
    print(f"MX encoder, last layer on latent rows (bf16 kernels): mean |bounded err| {e_lat:.4f}; all rows on the MX kernels: {e_all:.4f}; "
          f"between the two: {d:.4f}")
    assert not torch.equal(outs[0], outs[1 << 19])      # the shortcut really took the other kernels
    # doubled gains and outlier channels make this model harsher on e4m3 than the synthetic towers (sharper softmax), so the yardstick is
    # the all-MX forward of the SAME weights: with its last layer in bf16 the forward can only be closer to the oracle, not further
    assert e_lat < 1.25 * e_all + 0.02, (e_lat, e_all)
    assert d < 2.0 * e_all + 0.02, (d, e_all)
