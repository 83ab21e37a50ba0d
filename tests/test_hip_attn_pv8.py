"""The opt-in e4m3 P.V attention (csrc/ttv_attn_pv8.hip: k_quant_v_pv8 + k_attn_pv8) against its restatement
tests/pv8_ref.py, and the towers that run it (ttv_tower_weights.attn_pv8, TiTok.set_attention_pv).

The element bound (test 3, reused by 4 and 7b).  The reference is EXACT float64 softmax attention on the bf16 q, k and on the
DEQUANTISED V image - V's rounding is taken out by construction - so what is left of the kernel's error is, per output element (q, d),
with p_t = 2^(s_t - max_t s_t), l = sum p_t, A = (1/l) sum p_t |V_td|:
  1. P's rounding to e4m3 at p * 2^6: relative 2^-4 for a normal (three mantissa bits, round to nearest even: half an ulp of the binade's
     low end), absolute 2^-10 for a subnormal (e4m3's smallest step is 2^-9), i.e. 2^-(10 + 6) in units of p; never saturated (p * 2^6 <= 256):
         (1/l) sum_t max(2^-4 p_t, 2^-16) |V_td|
     taken against the row maximum: the kernel's reference is never above it, so its p are never smaller and its floor never coarser;
  2. p itself: the fp32 score accumulates 64 products (64 roundings of at most 2^-24 max_t sum_i |q_i k_ti| each = 2^-18 of it), the
     subtraction of the reference rounds once (2^-24 * 160 covers every exponent that does not flush to zero), v_exp_f32 is good to 2^-21:
         eps_p = ln 2 (2^-18 max_t sum_i |q_i k_ti| + 2^-24 * 160) + 2^-21,   in numerator and row sum: 2 eps_p A
  3. fp32 accumulation: 64 products per MFMA, one accumulate per key tile, a few rescales of O (8 counted), the row sum's S additions, v_rcp_f32 and
     the final multiply (1 + 1): (64 + S / 64 + 8 + S + 2) 2^-24 A
  4. the gate (sigmoid from v_exp_f32 and v_rcp_f32, one multiply): a factor 1 + 2^-20 on the above, times the gate;
  5. the bf16 store: 2^-9 of the value stored, itself at most |reference| + (1 .. 4).
Nothing in it comes from the kernel's output.  tests/test_attn_pv8_cpu.py shows on the CPU that a float64 model whose only inexact step
is (1) stays inside term (1) alone.

Measured on MI355X (the figures the tests print; DESIGN.md section 4z has them next to the timings):
  3. worst |error| / bound per case: s128 0.35 / 0.57 (spread 1.5 / 6), s200_gqa_gate 0.33 / 0.75, packed 0.33 / 0.79, packed_mode1 0.36 / 0.76.
  4. spikes: 0.25 over all rows; the aligned rows reproduce their one surviving V row exactly.
  5. relative RMS error against float64 attention, packed case: ttv_attention_pv8 3.5e-2 / 2.9e-2, ttv_attention (bf16) 2.2e-3 / 2.1e-3.
  7. tower layers 0.25 - 0.31 of the bound (tiny, small, base with MX linears); FSQ indices of these two small clips all kept, z moves by
     1e-3 (tiny, 2 layers) and 2.3e-3 (small, 1 layer) - tools/pv8_ab.py has the figures of full-size batches.
  The whole file: 4 s on the GPU machine (22 tests).
Without the feature every test here fails at its first call: the library has no ttv_quant_v_pv8 / ttv_attention_pv8, TiTok no set_attention_pv.
"""
import contextlib
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import pv8_ref as R
from titok_video_amd import _lib
from titok_video_amd.plan import get_plan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
GATE, QSCALED = 1, 4
INVALID = 1          # TTV_ERR_INVALID


def L():
    return _lib.lib()


def S():
    return _lib.stream_ptr(torch.device(DEV))


def report(*parts):
    print("MEASURED", *parts, flush=True)


def err():
    return L().ttv_error_string().decode()


def quant_image(xd, cu_d, n_seqs, hq, hkv, fill=0xAB):
    Lr, ld = xd.shape
    nbytes = L().ttv_attention_pv8_bytes(Lr, n_seqs, hkv)
    assert nbytes == R.image_bytes(Lr, n_seqs, hkv)
    img = torch.full((nbytes + 64,), fill, dtype=torch.uint8, device=DEV)        # 64 guard bytes behind the image
    _lib.check(L().ttv_quant_v_pv8(xd.data_ptr(), ld, cu_d.data_ptr(), n_seqs, Lr, hq, hkv, img.data_ptr(), S()), "ttv_quant_v_pv8")
    return img


def run_pv8(x, cu, hq, hkv, gate, tab, img=None):
    """(output [L, d] bf16 on the CPU, image on the device); rows no entry covers keep the NaN the output starts from."""
    xd = x.to(DEV)
    cu_d = torch.from_numpy(np.asarray(cu, dtype=np.int32)).to(DEV)
    if img is None:
        img = quant_image(xd, cu_d, len(cu) - 1, hq, hkv)
    out = torch.full((x.shape[0] + 1, hq * 64), float("nan"), dtype=BF, device=DEV)
    td = tab.to(DEV)
    _lib.check(L().ttv_attention_pv8(xd.data_ptr(), x.shape[1], out.data_ptr(), hq * 64, cu_d.data_ptr(), td.data_ptr(), td.shape[0], hq, hkv, 64,
                                     QSCALED | (GATE if gate else 0), img.data_ptr(), S()), "ttv_attention_pv8")
    torch.cuda.synchronize()
    o = out.cpu()
    assert bool(torch.isnan(o[-1]).all()), "written past the last row"
    return o[:-1], img


@functools.lru_cache(maxsize=None)
def case(shape, spread):
    """Inputs, restated image, reference and bound of one case: computed once, shared by the tests, never modified."""
    lens, hq, hkv, gate, half = R.SHAPES[shape]
    x, cu = R.rows(shape, spread)
    d, g = hq * 64, hkv * 64
    img, deq = R.v_image(x[:, 2 * d + g:2 * d + 2 * g], cu, hkv, fill=0xAB)
    ref, terms = R.pv8_attention(x, cu, hq, hkv, deq, gate)
    return SimpleNamespace(x=x, cu=cu, hq=hq, hkv=hkv, gate=gate, tab=R.table(cu, hq, half), img=img, deq=deq, ref=ref, terms=terms,
                           bound=R.element_bound(ref, terms, cu, hq))


def hold(o, ref, bound, what):
    assert bool(torch.isfinite(o.float()).all()), f"{what}: non-finite output"
    e = (o.double() - ref).abs()
    ratio = e / bound
    worst = int(ratio.argmax())
    r, c = divmod(worst, o.shape[1])
    report(f"{what}: max |err| / bound {float(ratio.max()):.3f} at (row {r}, col {c}); max |err| {float(e.max()):.3e}, rms err {float(e.pow(2).mean().sqrt()):.3e}, "
           f"rms ref {float(ref.pow(2).mean().sqrt()):.3e}")
    assert bool((e <= bound).all()), f"{what}: element (row {r}, col {c}) off by {float(e[r, c]):.3e} > bound {float(bound[r, c]):.3e}"


# ---------------------------------------------------------------------------------------------- 1: the image
def test_image_bit_for_bit():
    """64 | 129 | 320 rows, 2 kv-heads: an all-zero block, a block whose amax is 448 * 2^-3 exactly (an exact power of two times 448: the
    scale must keep that exponent, elements reach 448), zero padding of the last tiles (129: one key in its third tile), unused slots and
    the guard bytes untouched."""
    lens, hq, hkv = [64, 129, 320], 4, 2
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    d, g = hq * 64, hkv * 64
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(int(cu[-1]), 2 * d + 2 * g, generator=gen)
    v0 = 2 * d + g
    x[64 + 32:64 + 64, v0 + 70] = 0.0                       # sequence 1, tile 0, block (t = 1, kv-head 1, d = 6): all zero
    x[193 + 64:193 + 96, v0 + 3] *= 0.01                    # sequence 2, tile 1, block (t = 0, kv-head 0, d = 3): amax = 56 = 448 / 8 exactly
    x[193 + 64 + 9, v0 + 3] = -56.0
    x = x.to(BF)
    want, _ = R.v_image(x[:, v0:v0 + g], cu, hkv, fill=0xAB)
    base = ((R.tile_slot(cu, 2) + 1) * hkv + 0) * R.TILE_BYTES
    assert want[base + R.scale_byte_positions()[0, 3]] == 127 - 3 and want[base + R.tile_byte_positions()[9, 3]] == 0xFE       # -448
    base = ((R.tile_slot(cu, 1) + 0) * hkv + 1) * R.TILE_BYTES
    assert want[base + R.scale_byte_positions()[1, 6]] == 127
    xd = x.to(DEV)
    img = quant_image(xd, torch.from_numpy(cu).to(DEV), 3, hq, hkv, fill=0xAB).cpu().numpy()
    assert (img[-64:] == 0xAB).all(), "bytes written behind the image"
    got = img[:-64]
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} image bytes differ; first at byte {bad[0]} = tile {bad[0] // R.TILE_BYTES} + {bad[0] % R.TILE_BYTES}: {got[bad[0]]:#x} != {want[bad[0]]:#x}"
    used = sum((n + 63) // 64 for n in lens) * hkv
    assert int((want.reshape(-1, R.TILE_BYTES) != 0xAB).any(1).sum()) == used       # the restatement itself: every tile of a sequence filled, no other


# ---------------------------------------------------------------------------------------------- 2: one-hot
def test_one_hot_rows_are_exact():
    """Twelve sequences of 250 rows in one buffer (2 q-heads on 1 kv-head), one per (tile in first / middle / last, quarter of the tile):
    the planted key's score is 64, every other score within +-4 of 0, so p of the others rounds to zero in e4m3 (2^-54 against a
    smallest step of 2^-9) and vanishes in the fp32 row sum: the output must be the planted key's V row, bit for bit.  V holds e4m3-exact
    values from an asymmetric set whose block maximum is 2 wherever 2 occurs (scale 2^-7: 0.25 .. 2 -> 32 .. 256, all representable)."""
    hq, hkv, Sq = 2, 1, 250
    combos = [(tile, quarter) for tile in (0, 1, 3) for quarter in range(4)]
    cu = (np.arange(len(combos) + 1) * Sq).astype(np.int32)
    d, g = hq * 64, hkv * 64
    gen = torch.Generator().manual_seed(11)
    x = torch.zeros(int(cu[-1]), 2 * d + 2 * g)
    x[:, :d] = 0.05 * torch.randn(x.shape[0], d, generator=gen)
    x[:, 2 * d:2 * d + g] = 0.5 * torch.randn(x.shape[0], g, generator=gen)
    values = torch.tensor([2.0, -1.5, 1.0, -0.75, 0.5, 0.25, -2.0, 1.75, -0.25, 1.25])
    x[:, 2 * d + g:] = values[torch.randint(0, len(values), (x.shape[0], g), generator=gen)]
    for hd in range(hq):
        x[:, hd * 64] = 8.0                                   # every query: 8 on feature 0
    x[:, 2 * d] = 0.0                                         # every key: 0 there ...
    keys = []
    for i, (tile, quarter) in enumerate(combos):
        key = 64 * tile + 16 * quarter + 3 + 2 * quarter      # ... except the planted one: 8 * 8 = 64
        keys.append(key)
        x[int(cu[i]) + key, 2 * d] = 8.0
    x = x.to(BF)
    o, _ = run_pv8(x, cu, hq, hkv, False, R.table(cu, hq))
    for i, key in enumerate(keys):
        want = x[int(cu[i]) + key, 2 * d + g:].repeat(hq)
        got = o[int(cu[i]):int(cu[i + 1])]
        rows_bad = (got.view(torch.int16) != want.view(torch.int16)[None, :]).any(1).nonzero().flatten()
        assert rows_bad.numel() == 0, f"tile / quarter {combos[i]} key {key}: {rows_bad.numel()} query rows differ from V[key], first {int(rows_bad[0])}"


# ---------------------------------------------------------------------------------------------- 3: the bound
@pytest.mark.parametrize("spread", [1.5, 6.0])
@pytest.mark.parametrize("shape", list(R.SHAPES))
def test_element_bound(shape, spread):
    c = case(shape, spread)
    o, img = run_pv8(c.x, c.cu, c.hq, c.hkv, c.gate, c.tab)
    assert (img.cpu().numpy()[:-64] == c.img).all(), "the image differs from its restatement"
    hold(o, c.ref, c.bound, f"pv8 {shape} spread {spread}")


# ---------------------------------------------------------------------------------------------- 4: spikes
def test_spikes_move_the_reference_and_stay_finite():
    """Keys that lift the row maximum by more than 140 log2 units at a time, after the first tile, in both lane halves and in the
    second half of a tile (pv8_ref.spiked_rows): the rescale factor underflows to zero, nothing may become inf or NaN, and the aligned
    rows - like all others - stay inside the bound of test 3."""
    x, cu, aligned = R.spiked_rows()
    hq, hkv = 2, 1
    _, deq = R.v_image(x[:, 2 * hq * 64 + 64:], cu, hkv)
    ref, terms = R.pv8_attention(x, cu, hq, hkv, deq, False)
    s = x[aligned, :64].double() @ x[:, 2 * hq * 64:2 * hq * 64 + 64].double().t()
    top = s.topk(2, dim=1).values
    assert float((top[:, 0] - top[:, 1]).min()) > 140.0 and float(s[:, :64].max()) < 20.0        # the construction
    o, _ = run_pv8(x, cu, hq, hkv, False, R.table(cu, hq))
    hold(o, ref, R.element_bound(ref, terms, cu, hq), "pv8 spikes")
    hold(o[aligned], ref[aligned], R.element_bound(ref, terms, cu, hq)[aligned], "pv8 spikes, aligned rows")


# ---------------------------------------------------------------------------------------------- 5: figures
@pytest.mark.parametrize("spread", [1.5, 6.0])
def test_error_figures_against_float64_attention(spread):
    """No bar beyond test 3: RMS and max error of ttv_attention_pv8 and of ttv_attention (k_attn_bf16) against float64 attention on the
    bf16 inputs as they are (V not quantised), same inputs."""
    c = case("packed", spread)
    exact = R.attention_f64(c.x, c.cu, c.hq, c.hkv, c.gate)
    o8, _ = run_pv8(c.x, c.cu, c.hq, c.hkv, c.gate, c.tab)
    xd, cu_d, td = c.x.to(DEV), torch.from_numpy(c.cu).to(DEV), c.tab.to(DEV)
    o16 = torch.zeros(c.x.shape[0], c.hq * 64, dtype=BF, device=DEV)
    _lib.check(L().ttv_attention(xd.data_ptr(), c.x.shape[1], o16.data_ptr(), c.hq * 64, cu_d.data_ptr(), td.data_ptr(), td.shape[0], c.hq, c.hkv, 64,
                                 QSCALED | GATE, _lib.TTV_BF16, S()), "ttv_attention")
    rms = float(exact.pow(2).mean().sqrt())
    for name, o in (("ttv_attention_pv8", o8), ("ttv_attention (bf16)", o16.cpu())):
        e = (o.double() - exact).abs()
        report(f"spread {spread} {name}: rms err {float(e.pow(2).mean().sqrt()):.3e} ({float(e.pow(2).mean().sqrt()) / rms:.3e} of rms {rms:.3e}), max err {float(e.max()):.3e}")
        assert bool(torch.isfinite(o.float()).all())


# ---------------------------------------------------------------------------------------------- 6: determinism, independence, refusals
def test_deterministic_and_independent_of_packing():
    c = case("packed", 6.0)
    a, img = run_pv8(c.x, c.cu, c.hq, c.hkv, c.gate, c.tab)
    b, _ = run_pv8(c.x, c.cu, c.hq, c.hkv, c.gate, c.tab)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), "two runs differ"
    for s in range(len(c.cu) - 1):
        r0, r1 = int(c.cu[s]), int(c.cu[s + 1])
        cu1 = np.array([0, r1 - r0], dtype=np.int32)
        alone, _ = run_pv8(c.x[r0:r1].contiguous(), cu1, c.hq, c.hkv, c.gate, R.table(cu1, c.hq))
        assert torch.equal(alone.view(torch.int16), a[r0:r1].view(torch.int16)), f"sequence {s} alone differs from the packed run"


def test_refused_arguments():
    c = case("s128", 1.5)
    xd, cu_d, td = c.x.to(DEV), torch.from_numpy(c.cu).to(DEV), c.tab.to(DEV)
    img = quant_image(xd, cu_d, 1, 1, 1)
    out = torch.zeros(129, 64, dtype=BF, device=DEV)
    ld = c.x.shape[1]

    def call(x_ptr=xd.data_ptr(), o_ptr=out.data_ptr(), i_ptr=img.data_ptr(), head_dim=64, flags=QSCALED):
        return L().ttv_attention_pv8(x_ptr, ld, o_ptr, 64, cu_d.data_ptr(), td.data_ptr(), td.shape[0], 1, 1, head_dim, flags, i_ptr, S())
    assert call() == 0
    for kw, word in ((dict(head_dim=128), "head_dim"), (dict(flags=0), "pre-scaled"), (dict(flags=GATE), "pre-scaled"), (dict(flags=QSCALED | 2), "flags"),
                     (dict(x_ptr=xd.data_ptr() + 2), "unaligned"), (dict(o_ptr=out.data_ptr() + 8), "unaligned"), (dict(i_ptr=img.data_ptr() + 4), "unaligned")):
        assert call(**kw) == INVALID and word in err(), (kw, err())
    assert L().ttv_quant_v_pv8(xd.data_ptr(), ld, cu_d.data_ptr(), 1, 128, 1, 1, img.data_ptr() + 4, S()) == INVALID and "unaligned" in err()
    assert L().ttv_attention_pv8_bytes(-1, 1, 1) == -1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 7: towers
LEVELS = [8, 8, 8, 6, 5]
CLIPS = ([(16, 64, 64), (8, 32, 48)], [61, 5])           # 317 and 53 packed rows (tests/forward_cases.py "ragged", its two middle clips)


@functools.lru_cache(maxsize=None)
def _model(size, layers):
    from titok_video_amd.model.titok import TiTok
    torch.manual_seed(7)
    cfg = SimpleNamespace(tokenizer=SimpleNamespace(model=SimpleNamespace(patch_size=[4, 8, 8], fsq_levels=LEVELS, encoder_size=size, decoder_size=size)))
    m = TiTok(cfg).to(DEV, BF).eval()
    for t in (m.encoder, m.decoder):        # `layers` layers of the tower (the device of tests/test_hip_wide_layer.py); alpha stays the full depth's
        t.num_layers = layers
        t.invalidate_packs()
    return m


@functools.lru_cache(maxsize=None)
def _clips():
    gen = torch.Generator().manual_seed(3)
    return tuple(torch.randn(3, *shape, generator=gen).to(DEV, BF) for shape in CLIPS[0])


def _forward(m, mode, fp8=False):
    m.set_attention_pv(mode)
    m.encoder.fp8_linears = m.decoder.fp8_linears = fp8
    try:
        with torch.no_grad():
            res = m.encoder.run(list(_clips()), CLIPS[1], None, m.quantize.params, want_z=True, want_bounded=True)
            rec = m.decode(res["codes"], CLIPS[1], [tuple(c.shape[1:]) for c in _clips()])
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in res.items()}, [r.cpu() for r in rec]
    finally:
        m.set_attention_pv(None)
        m.encoder.fp8_linears = m.decoder.fp8_linears = False


def _equal(a, b):
    return all(torch.equal(a[0][k].view(torch.uint8), b[0][k].view(torch.uint8)) for k in a[0]) and \
        all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a[1], b[1]))


@pytest.mark.parametrize("size,layers", [("tiny", 2), ("small", 1)])
def test_towers_mode_off_keeps_bits_and_workspace(size, layers):
    """(a) a model that never heard of the mode, the same model after the mode was on and off again: the same bits (the off state is the
    struct's zero, the pack key tells the two packs apart); the workspace size does not depend on the mode.  (c) figures, no bar."""
    m = _model(size, layers)
    dims = m.encoder._dims(_lib.TTV_BF16)
    plan = get_plan(CLIPS[0], CLIPS[1], m.encoder.patch, torch.device(DEV))
    batch = plan.batch_for(*m.encoder.heads)
    need = L().ttv_tower_workspace_bytes(C.byref(dims), C.byref(batch))
    off = _forward(m, None)
    on = _forward(m, "fp8")
    again = _forward(m, None)
    assert _equal(off, again), "mode off after mode on: other bits"
    assert not _equal(off, on), "mode on changed nothing: the towers did not run the pv8 kernels"
    assert L().ttv_tower_workspace_bytes(C.byref(dims), C.byref(batch)) == need
    ws_bytes = m.encoder._workspace(dims, plan, torch.device(DEV)).numel()
    assert ws_bytes == need
    keep = float((on[0]["indices"] == off[0]["indices"]).float().mean())
    zrel = float((on[0]["z"] - off[0]["z"]).norm() / off[0]["z"].norm())
    rrel = float(torch.cat([(a.float() - b.float()).flatten() for a, b in zip(on[1], off[1])]).norm() / torch.cat([b.float().flatten() for b in off[1]]).norm())
    report(f"towers {size} x {layers} layers, attention_pv fp8 vs off: FSQ index keep rate {keep:.3f}, relative z error {zrel:.4f}, relative reconstruction error {rrel:.4f}")
    assert all(bool(torch.isfinite(r.float()).all()) for r in on[1])


@contextlib.contextmanager
def forced(bits):
    L().ttv_debug_set(bits)
    try:
        yield
        torch.cuda.synchronize()
    finally:
        L().ttv_debug_set(0)


def _align256(n):
    return (n + 255) // 256 * 256


@pytest.mark.parametrize("size,layers,fp8", [("tiny", 1, False), ("tiny", 2, False), ("small", 1, False), ("base", 2, "mx")])
def test_tower_layers_stay_inside_the_bound(size, layers, fp8):
    """(b), (d): the encoder's LAST layer's attention output, replayed from that layer's own qkv (both read back from the workspace: carve()
    in ttv_api.hip puts x | xn | qkv | ao first), stays inside the bound of test 3; depths 1 and 2 make every layer of a two-layer tower
    the last one once.  Every row computed (debug bit ENC_ALL_ROWS: the latent-rows-only last layer would leave the patch rows of ao to
    the layer before).  With fp8_linears = "mx" (base: the size whose widths the block-scaled linears take) the same through
    run_layer_mx, whose fused MX epilogue gives way to the quantisation pass over the attention output: the modes compose."""
    m = _model(size, layers)
    enc = m.encoder
    hq, hkv = enc.heads
    plan = get_plan(CLIPS[0], CLIPS[1], enc.patch, torch.device(DEV))
    dims = enc._dims(_lib.TTV_BF16)
    Lr, d, g = plan.total_rows, enc.width, hkv * 64
    nq = 2 * d + 2 * g
    m.set_attention_pv("fp8")
    enc.fp8_linears = fp8
    try:
        ws = enc._workspace(dims, plan, torch.device(DEV))
        with forced(_lib.DBG_ENC_ALL_ROWS), torch.no_grad():
            res = enc.run(list(_clips()), CLIPS[1], None, None, want_z=True)
        assert bool(torch.isfinite(res["z"]).all())
    finally:
        m.set_attention_pv(None)
        enc.fp8_linears = False
    off_qkv = 2 * _align256(Lr * d * 2)
    off_ao = off_qkv + _align256(Lr * nq * 2)
    qkv = ws[off_qkv:off_qkv + Lr * nq * 2].view(BF).view(Lr, nq).cpu()
    ao = ws[off_ao:off_ao + Lr * d * 2].view(BF).view(Lr, d).cpu()
    cu = np.asarray(plan.cu_seqlens, dtype=np.int32)
    _, deq = R.v_image(qkv[:, 2 * d + g:], cu, hkv)
    ref, terms = R.pv8_attention(qkv, cu, hq, hkv, deq, True)
    hold(ao, ref, R.element_bound(ref, terms, cu, hq), f"tower {size} layer {layers - 1} of {layers} fp8_linears={fp8}")


def test_towers_refuse_what_the_kernels_cannot_run():
    """(e) the index-exact modes and fp32 clips raise ValueError, in either order; so does any other value."""
    m = _model("tiny", 2)
    with pytest.raises(ValueError):
        m.set_attention_pv("fp4")
    try:
        m.set_attention_pv("fp8")
        for mode in ("fp32", "split3"):
            with pytest.raises(ValueError):
                m.set_index_exact(mode)
        with pytest.raises(ValueError), torch.no_grad():
            m.encoder.run([c.float() for c in _clips()], CLIPS[1], None, m.quantize.params, want_z=False)
        m.set_attention_pv(None)
        m.set_index_exact("fp32")
        with pytest.raises(ValueError):
            m.set_attention_pv("fp8")
    finally:
        m.set_index_exact(None)
        m.set_attention_pv(None)
