"""The decoder's constant block (ttv_dec_l0_const, TTV_DEC_L0_CONST): the patch rows enter layer 0 as ln_pre_p(mask_token), so their
q | gate | k | v are built once per (weight pack, clip geometry); layer 0's to_qkv then computes the latent token tiles only and its
attention reads the patch rows from the block; a patch query block loops over the latent keys only and adds the block's cached sums
over the patch keys.  Against the switch-off run (ttv_debug_set bit 22, same process): bit for bit everywhere except the patch query
rows of layer 0's attention output, which differ by the place of one fp32 addition per accumulator and are held to
|delta| <= one bf16 ulp of the element + n_tiles * 2^-23 * max_j |v_jd| (n_tiles fp32 additions of p * v terms re-associated, after
normalisation, gate factor <= 1) and to the per-block float64 bound of tests/blockwise.py.  `-m gpu`.

Layer 0's intermediates are read out of the tower's workspace after a forward of ONE layer (`num_layers` set to 1 on the module: the
C side then stops behind layer 0, whose to_qkv output and attention output stay in the workspace).  Workspace layout (ttv_api.hip, carve):
x, xn [L, d], qkv [L, 2d+2g], ao [L, d], each rounded up to 256 bytes.

Shapes: the smallest at which each piece can go wrong - case A, 3 clips of 8x64x64 with K = 128 (one latent and one patch query block
per clip, the source changes once in a four-tile key loop); case B, 2 clips of 8x64x128 with K = 256 (two blocks of each kind: the
source changes in the middle of the table and of the ring); K = 32 and a batch of two geometries fall back to the plain sequence."""
from types import SimpleNamespace

import pytest
import torch

from oracle import titok_oracle as O
from tests import forward_cases as FC
from tests.blockwise import attention_forward_reference, check_blockwise
from tests.test_hip_backward_shapes import FWD_TOL
from titok_video_amd import _lib
from titok_video_amd.model.titok import TiTok
from titok_video_amd.plan import get_plan
from titok_video_amd.synthetic import seeded_titok_state, synthetic_clips

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
LEVELS = [7, 5, 5, 5, 5]
PIX_TOL_BF16 = 0.25           # the forward tests' bound on a bf16 reconstruction against the oracle's decode of the same indices
OFF = _lib.DBG_DEC_L0_NO_CONST
CASES = {"A": ([(8, 64, 64)] * 3, [128] * 3), "B": ([(8, 64, 128)] * 2, [256] * 2)}
FALLBACKS = {"k32": ([(8, 64, 64)] * 3, [32] * 3), "two_geometries": ([(8, 64, 64), (8, 64, 128)], [128, 128])}


@pytest.fixture(autouse=True)
def full_items(monkeypatch):
    monkeypatch.setenv("TTV_ATTN_SPLIT", "0")        # tables of full items at these small batches too (what the benchmark batch gets)
    yield
    _lib.lib().ttv_debug_set(0)


def build_model(seed=0):
    cfg = SimpleNamespace(tokenizer=SimpleNamespace(model=SimpleNamespace(patch_size=[4, 8, 8], fsq_levels=LEVELS, encoder_size="tiny",
                                                                          decoder_size="tiny")))
    m = TiTok(cfg)
    m.load_state_dict(seeded_titok_state(seed), strict=True)
    return m.to(DEV, BF).eval()


def decode(model, codes, counts, shapes, bits):
    _lib.lib().ttv_debug_set(bits)
    try:
        with torch.no_grad():
            recon = model.decode(codes, counts, shapes)
        torch.cuda.synchronize()
    finally:
        _lib.lib().ttv_debug_set(0)
    return [r.clone() for r in recon]


def layer0_views(dec, shapes, counts):
    """(workspace, qkv view [L, 2d+2g], ao view [L, d]) of the decoder's workspace on the current stream."""
    plan = get_plan(shapes, counts, dec.patch, torch.device(DEV))
    ws = dec._workspace(dec._dims(_lib.dtype_code(BF)), plan, torch.device(DEV))
    L, d, g = plan.total_rows, dec.width, dec.heads[1] * 64
    nq = 2 * d + 2 * g
    a256 = lambda v: (v + 255) // 256 * 256
    o_qkv = 2 * a256(L * d * 2)
    o_ao = o_qkv + a256(L * nq * 2)
    return ws, ws[o_qkv:o_qkv + L * nq * 2].view(BF).view(L, nq), ws[o_ao:o_ao + L * d * 2].view(BF).view(L, d), plan


def one_layer_runs(model, shapes, counts, seed):
    """Layer 0 alone, switch off and on, over a workspace pre-filled with a pattern: (qkv, ao, recon) of each, the plan, the block."""
    dec = model.decoder
    codes = torch.randn(sum(counts), len(LEVELS), generator=torch.Generator().manual_seed(seed)).to(DEV, BF)
    dec.num_layers = 1
    try:
        ws, qkv, ao, plan = layer0_views(dec, shapes, counts)
        out = {}
        for name, bits in (("off", OFF), ("on", 0)):
            ws.fill_(0x7f)
            recon = decode(model, codes, counts, shapes, bits)
            out[name] = (qkv.clone(), ao.clone(), recon)
        pack = dec._packed(BF, torch.device(DEV))
        l0 = pack.dec_l0_const(dec._dims(_lib.dtype_code(BF)), plan)
    finally:
        dec.num_layers = len(dec.model_layers.attn_layer)
        dec.invalidate_packs()           # (a pack built meanwhile carries one layer)
    return out, plan, l0, pack


def block_rows(pack, l0, nq):
    """The rows of the pack's only block, as the tensor that owns them."""
    (ent,) = pack._l0_const.values()
    block = ent["keep"][0]
    assert block.data_ptr() == l0.rows
    return block[:l0.patch_rows * nq * 2].view(BF).view(l0.patch_rows, nq)


def bf16_ulp(x):
    """One unit in the last place of the bf16 values in x (8 significant bits), as float64; the smallest normal's for zero."""
    a = x.double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


def reassociation_bound(qkv_off, ao_off, cu, hq, hkv):
    """[L, d] bound on |on - off| of the gated attention output: one bf16 ulp of the switch-off element + n_tiles * 2^-23 * max_j |v_jd|."""
    d, g, rep = hq * 64, hkv * 64, hq // hkv
    bound = bf16_ulp(ao_off)
    for b in range(len(cu) - 1):
        s, e = cu[b], cu[b + 1]
        n_tiles = -(-(e - s) // 64)
        vmax = qkv_off[s:e, 2 * d + g:].double().abs().amax(0)                     # [g]: per v column, over the sequence's keys
        per_col = torch.cat([vmax[(h // rep) * 64:(h // rep) * 64 + 64] for h in range(hq)])
        bound[s:e] += n_tiles * 2.0 ** -23 * per_col
    return bound


def check_patch_rows(ao_on, ao_off, qkv_off, plan, counts, hq, hkv, tag):
    """Latent query rows bit for bit; patch query rows inside the re-association bound.  Prints the worst ratio."""
    cu = plan.cu_seqlens
    on, off = ao_on.cpu(), ao_off.cpu()
    bound = reassociation_bound(qkv_off.cpu(), off, cu, hq, hkv)
    worst = 0.0
    for b, k in enumerate(counts):
        lat, pat = slice(cu[b], cu[b] + k), slice(cu[b] + k, cu[b + 1])
        assert torch.equal(on[lat].view(torch.int16), off[lat].view(torch.int16)), f"{tag} clip {b}: latent query rows differ"
        ratio = ((on[pat].double() - off[pat].double()).abs() / bound[pat]).max()
        worst = max(worst, float(ratio))
    print(f"MEASURED {tag}: worst |on - off| / bound over the patch query rows {worst:.3f}")
    assert worst <= 1.0, f"{tag}: a patch query row left the re-association bound ({worst:.3f} of it)"


@pytest.mark.parametrize("case", sorted(CASES))
def test_layer0_pieces_are_the_switch_off_bits(case):
    """to_qkv: the latent rows carry the switch-off bits and no patch row of ws.qkv is written (the pattern survives); the block's rows
    are the patch rows the switch-off to_qkv writes for every clip; the attention output's latent query rows are the switch-off bits
    (same keys, same order, whichever buffer they come from), its patch query rows inside the re-association bound, and all of it
    inside the per-block float64 bound of tests/blockwise.py."""
    shapes, counts = CASES[case]
    model = build_model()
    out, plan, l0, pack = one_layer_runs(model, shapes, counts, seed=5)
    assert l0 is not None and l0.latent_rows == counts[0] and l0.state, "no block, or its sums left the window on plain weights"
    (qkv_off, ao_off, rec_off), (qkv_on, ao_on, rec_on) = out["off"], out["on"]
    hq, hkv = model.decoder.heads
    nq = qkv_off.shape[1]
    pattern = torch.full((1,), 0x7f7f, dtype=torch.int16, device=DEV).view(BF)
    rows = block_rows(pack, l0, nq)
    cu = plan.cu_seqlens
    for b, k in enumerate(counts):
        lat, pat = slice(cu[b], cu[b] + k), slice(cu[b] + k, cu[b + 1])
        assert torch.equal(qkv_on[lat].view(torch.int16), qkv_off[lat].view(torch.int16)), f"clip {b}: latent rows of to_qkv differ"
        assert bool((qkv_on[pat].view(torch.int16) == pattern.view(torch.int16)).all()), f"clip {b}: the restricted to_qkv wrote a patch row"
        assert not bool((qkv_off[pat].view(torch.int16) == pattern.view(torch.int16)).all())
        assert torch.equal(rows.view(torch.int16), qkv_off[pat].view(torch.int16)), f"clip {b}: block rows differ from the forward's patch rows"
    check_patch_rows(ao_on, ao_off, qkv_off, plan, counts, hq, hkv, f"case {case}")
    _, gated = attention_forward_reference(qkv_off.cpu(), cu, hq, hkv, c_exp=FC.C_EXP)
    bt, gt = FWD_TOL["bf16"]
    wb, gl = check_blockwise(ao_on.cpu(), gated, cu, hq, bt, gt, f"layer-0 attention with the constant block, case {case}")
    print(f"MEASURED case {case}: worst block {wb:.2e} (bound {bt:.1e}) global {gl:.2e} (bound {gt:.1e})")


@pytest.mark.parametrize("case", sorted(CASES))
def test_whole_forward_same_indices_same_reconstruction_and_oracle(case):
    shapes, counts = CASES[case]
    model = build_model()
    sd = seeded_titok_state(0)
    clips = synthetic_clips(shapes, seed=21, dtype=BF, device=DEV)
    res = {}
    for name, bits in (("on", 0), ("off", OFF)):
        _lib.lib().ttv_debug_set(bits)
        with torch.no_grad():
            recon, info = model(clips, counts)
        torch.cuda.synchronize()
        _lib.lib().ttv_debug_set(0)
        res[name] = ([r.clone() for r in recon], info["indices"].clone())
    assert torch.equal(res["on"][1], res["off"][1]), "token indices differ"
    pack = model.decoder._packed(BF, torch.device(DEV))
    assert len(pack._l0_const) == 1 and next(iter(pack._l0_const.values()))["state"], "the forward did not build a usable block"
    with torch.no_grad():
        ref = O.titok_decode_indices(res["on"][1].cpu(), shapes, counts, sd, LEVELS)
    for name in ("on", "off"):
        perr = max(float((r.float().cpu() - x).abs().max()) for r, x in zip(res[name][0], ref))
        print(f"MEASURED case {case} switch {name}: decoder max pixel error against the oracle {perr:.3e}")
        assert perr < PIX_TOL_BF16


@pytest.mark.parametrize("case", sorted(FALLBACKS))
def test_fallback_geometries_build_no_block_and_change_no_bit(case):
    shapes, counts = FALLBACKS[case]
    model = build_model()
    codes = torch.randn(sum(counts), len(LEVELS), generator=torch.Generator().manual_seed(9)).to(DEV, BF)
    on, off = decode(model, codes, counts, shapes, 0), decode(model, codes, counts, shapes, OFF)
    assert all(torch.equal(a, b) for a, b in zip(on, off))
    pack = model.decoder._packed(BF, torch.device(DEV))
    assert all(v is None for v in pack._l0_const.values()), "a block was built for a geometry that cannot use it"


def exponents(qkv, plan, counts, width):
    """Largest softmax exponent of head 0 of clip 0: (patch query . patch key, patch query . latent key)."""
    k0, s0 = counts[0], plan.cu_seqlens[1]
    q, k = qkv[:s0, :64].float(), qkv[:s0, 2 * width:2 * width + 64].float()
    sc = q[k0:] @ k.T
    return float(sc[:, k0:].max()), float(sc[:, :k0].max())


def test_patch_patch_exponents_beyond_the_window_make_the_block_unusable():
    """q rows of layer 0's to_qkv scaled until a patch-patch exponent passes 60: the builder's row sums leave k_attn_swp's window, the
    block carries no state, and the forward - rows from the block, every key, the kernel's exact loop where a block needs it - is the
    switch-off run bit for bit."""
    shapes, counts = CASES["A"]
    model = build_model()
    dec = model.decoder
    with torch.no_grad():
        dec.model_layers.attn_layer[0].to_qkv.weight[:dec.width].mul_(40.0)
    out, plan, l0, _ = one_layer_runs(model, shapes, counts, seed=6)
    (qkv_off, ao_off, rec_off), (_, ao_on, rec_on) = out["off"], out["on"]
    pp, pl = exponents(qkv_off, plan, counts, dec.width)
    print(f"MEASURED largest exponents of clip 0, head 0: patch-patch {pp:.1f}, patch-latent {pl:.1f}")
    assert pp > 70.0, "the scaling did not push a patch-patch exponent out of the window"
    assert l0 is not None and not l0.state, "the builder did not flag its sums"
    assert torch.equal(ao_on.view(torch.int16), ao_off.view(torch.int16))
    assert bool(torch.isfinite(ao_on.float()).all())
    assert all(torch.equal(a, b) for a, b in zip(rec_on, rec_off))


def test_combined_sum_beyond_the_window_takes_the_exact_loop_over_both_sources():
    """A mask token so small that the patch rows stay ~1e-2 of the latent rows behind the two norms, and q rows scaled by 600: the
    patch-patch exponents stay near zero (the block's own sums are inside the window: state present) while a patch query's exponents
    on the latent keys pass 60, so only the COMBINED sum leaves the window and the block runs its exact loop over every key, latent
    tiles from ws.qkv and patch tiles from the block through the same staging macro.  Held to the float64 bound."""
    shapes, counts = CASES["A"]
    model = build_model()
    dec = model.decoder
    with torch.no_grad():
        dec.mask_token.fill_(1e-7)
        dec.model_layers.attn_layer[0].to_qkv.weight[:dec.width].mul_(600.0)
    out, plan, l0, _ = one_layer_runs(model, shapes, counts, seed=6)
    (qkv_off, ao_off, _), (_, ao_on, _) = out["off"], out["on"]
    hq, hkv = dec.heads
    pp, pl = exponents(qkv_off, plan, counts, dec.width)
    print(f"MEASURED largest exponents of clip 0, head 0: patch-patch {pp:.1f}, patch-latent {pl:.1f}")
    assert pp < 40.0 and pl > 70.0, "the inputs do not separate the block's own sums from the combined ones"
    assert l0 is not None and l0.state, "the block's own sums should be inside the window"
    assert bool(torch.isfinite(ao_on.float()).all())
    _, gated = attention_forward_reference(qkv_off.cpu(), plan.cu_seqlens, hq, hkv, c_exp=FC.C_EXP)
    bt, gt = FWD_TOL["bf16"]
    wb, gl = check_blockwise(ao_on.cpu(), gated, plan.cu_seqlens, hq, bt, gt, "layer-0 attention, exact loop with the constant block")
    print(f"MEASURED exact loop: worst block {wb:.2e} (bound {bt:.1e}) global {gl:.2e} (bound {gt:.1e})")
    # the exact loop sums every key from zero in the switch-off order: the switch-off bits wherever that run took its exact loop too
    check_patch_rows(ao_on, ao_off, qkv_off, plan, counts, hq, hkv, "exact loop")


def test_weight_changes_rebuild_the_block_and_geometries_get_their_own():
    shapes, counts = CASES["A"]
    shapes_b, counts_b = CASES["B"]
    model = build_model()
    dec = model.decoder
    codes = torch.randn(sum(counts), len(LEVELS), generator=torch.Generator().manual_seed(11)).to(DEV, BF)
    codes_b = torch.randn(sum(counts_b), len(LEVELS), generator=torch.Generator().manual_seed(12)).to(DEV, BF)
    first = decode(model, codes, counts, shapes, 0)
    pack0 = dec._packed(BF, torch.device(DEV))
    decode(model, codes_b, counts_b, shapes_b, 0)
    assert dec._packed(BF, torch.device(DEV)) is pack0 and len(pack0._l0_const) == 2, "one block per geometry"
    # an in-place update that bumps the parameter's version: new pack, new block, the output of a fresh model with those weights
    with torch.no_grad():
        dec.ln_pre_p.weight.mul_(1.5)
        dec.model_layers.attn_layer[0].to_qkv.weight.mul_(0.75)
    second = decode(model, codes, counts, shapes, 0)
    pack1 = dec._packed(BF, torch.device(DEV))
    assert pack1 is not pack0 and len(pack1._l0_const) == 1
    assert not all(torch.equal(a, b) for a, b in zip(first, second))
    fresh = build_model()
    fresh.load_state_dict(model.state_dict(), strict=True)
    assert all(torch.equal(a, b) for a, b in zip(second, decode(fresh, codes, counts, shapes, 0)))
    # load_state_dict: back to the seeded weights, the first output again
    model.load_state_dict(seeded_titok_state(0), strict=True)
    third = decode(model, codes, counts, shapes, 0)
    pack2 = dec._packed(BF, torch.device(DEV))
    assert pack2 is not pack1 and len(pack2._l0_const) == 1
    assert all(torch.equal(a, b) for a, b in zip(first, third))
