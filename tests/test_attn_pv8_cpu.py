"""CPU side of the opt-in e4m3 P.V attention: the C ABI surface (struct sizes, symbols), the Python switch and its refusals, and the
conditions the restatement tests/pv8_ref.py must meet itself before tests/test_hip_attn_pv8.py may hold a kernel to it."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import pv8_ref as R
from titok_video_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(shape, spread) for shape in R.SHAPES for spread in (1.5, 6.0)]


def _cfg(**extra):
    return SimpleNamespace(tokenizer=SimpleNamespace(model=SimpleNamespace(patch_size=[4, 8, 8], fsq_levels=[8, 8, 8, 6, 5], encoder_size="tiny",
                                                                            decoder_size="tiny", **extra)))


def test_struct_sizes_unchanged_and_symbols_declared():
    assert C.sizeof(_lib.TowerWeights) == 11 * 8                     # attn_pv8 sits in the tail padding behind f32_split3
    assert _lib.TowerWeights.attn_pv8.offset == _lib.TowerWeights.f32_split3.offset + 4
    assert C.sizeof(_lib.TowerDims) == 15 * 4 and C.sizeof(_lib.LayerWeights) == 25 * 8
    header = open(os.path.join(ROOT, "include", "titok_hip.h")).read()
    for name, nargs in (("ttv_attention_pv8_bytes", 3), ("ttv_quant_v_pv8", 9), ("ttv_attention_pv8", 13)):
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs
        decl = re.search(r"\b%s\(([^;]*?)\);" % name, header, re.S)
        assert decl and len(decl.group(1).split(",")) == nargs, name
    assert _lib.SYMBOLS["ttv_attention_pv8_bytes"][0] is C.c_int64
    assert re.search(r"int32_t f32_split3;\s*/\*.*?\*/\s*int32_t attn_pv8;\s*} ttv_tower_weights;", header, re.S)
    build = open(os.path.join(ROOT, "titok_video_amd", "csrc", "build.sh")).read()
    assert " ttv_attn_pv8 " in build


def test_set_attention_pv_surface_and_refusals():
    from titok_video_amd.model.titok import TiTok
    m = TiTok(_cfg())
    assert m.encoder.attention_pv is None and m.decoder.attention_pv is None
    assert m.set_attention_pv("fp8") is m and m.encoder.attention_pv == "fp8" and m.decoder.attention_pv == "fp8"
    for mode in ("fp32", "split3"):
        with pytest.raises(ValueError):
            m.set_index_exact(mode)
    m.set_attention_pv(None)
    assert m.encoder.attention_pv is None and m.decoder.attention_pv is None
    for bad in ("fp4", "bf16", True, 8):
        with pytest.raises(ValueError):
            m.set_attention_pv(bad)
    m.set_index_exact("split3")
    with pytest.raises(ValueError):
        m.set_attention_pv("fp8")
    m.set_index_exact(None)
    m2 = TiTok(_cfg(attention_pv="fp8"))
    assert m2.encoder.attention_pv == "fp8" and m2.decoder.attention_pv == "fp8"
    with pytest.raises(ValueError):
        TiTok(_cfg(attention_pv="int8"))


def test_attention_pv_is_part_of_the_pack_key_and_refused_for_fp32():
    """The weight pack is rebuilt when the mode changes (its struct carries attn_pv8), and a pack for fp32 compute refuses the mode."""
    from titok_video_amd.model.base import blocks
    from titok_video_amd.model.titok import TiTok
    m = TiTok(_cfg())
    built = []

    class FakePack:
        def __init__(self, tower, dtype, device):
            built.append(getattr(tower, "attention_pv", None))
            self._owned = None

        def use_on_current_stream(self):
            pass
    real = blocks._WeightPack
    blocks._WeightPack = FakePack
    try:
        m.encoder._packed(torch.bfloat16, "cpu")
        m.encoder._packed(torch.bfloat16, "cpu")
        m.set_attention_pv("fp8")
        m.encoder._packed(torch.bfloat16, "cpu")
        m.set_attention_pv(None)
        m.encoder._packed(torch.bfloat16, "cpu")
    finally:
        blocks._WeightPack = real
        m.encoder.invalidate_packs()
    assert built == [None, "fp8", None]
    src = open(os.path.join(ROOT, "titok_video_amd", "model", "base", "blocks.py")).read()
    assert "attention_pv='fp8' is a bf16 inference mode" in src and "attn_pv8=1 if self.attn_pv8 else 0" in src


def test_keys_by_block_is_a_permutation_per_tile():
    kb = R.keys_by_block()
    assert kb.shape == (2, 32) and sorted(kb.flatten().tolist()) == list(range(64))
    # the fragment order covers every (key, d) byte of a tile once, and a block's bytes are bytes 16 t .. 16 t + 15 of both lane halves
    pos = R.tile_byte_positions()
    assert sorted(pos.flatten().tolist()) == list(range(4096))
    for t in range(2):
        assert sorted(R.fragment_key(h, b) for h in range(2) for b in range(16 * t, 16 * t + 16)) == sorted(kb[t].tolist())
    assert sorted(R.scale_byte_positions().flatten().tolist()) == list(range(4096, 4224))


def test_tile_slots_never_overlap():
    rng = np.random.default_rng(0)
    for _ in range(200):
        lens = rng.integers(1, 400, size=rng.integers(1, 9))
        cu = np.concatenate([[0], np.cumsum(lens)])
        end = 0
        for s, n in enumerate(lens):
            assert R.tile_slot(cu, s) >= end
            end = R.tile_slot(cu, s) + (int(n) + 63) // 64
        assert end * R.TILE_BYTES <= R.image_bytes(int(cu[-1]), len(lens), 1)


def test_image_restatement_round_trips():
    """Dequantising the image gives V to MX precision (2^-4 of the block maximum), zero blocks give byte 127 and zero bytes."""
    x, cu = R.rows("packed", 1.5)
    hq, hkv = 4, 2
    v = x[:, 2 * hq * 64 + hkv * 64:].clone()
    v[64:96, 5] = 0
    img, deq = R.v_image(v, cu, hkv, fill=0xAB)
    assert img.size == R.image_bytes(int(cu[-1]), 3, hkv)
    err = (deq - v.double()).abs()
    assert float(err.max()) <= 2.0 ** -4 * float(v.double().abs().max())
    assert float(deq[64:96, 5].abs().max()) == 0.0
    base = (R.tile_slot(cu, 1) * hkv + 0) * R.TILE_BYTES
    assert img[base + R.scale_byte_positions()[0, 5]] == 127


@pytest.mark.parametrize("shape,spread", CASES)
def test_p_rounding_alone_stays_inside_its_term(shape, spread):
    """A float64 model whose ONLY inexact step is P's rounding to e4m3 at p * 2^6 - against the row maximum and against a reference the
    full 2 units below it - differs from the exact softmax on the dequantised V by no more than term 1 of the bound; and the bound exceeds
    that term."""
    lens, hq, hkv, gate, _ = R.SHAPES[shape]
    x, cu = R.rows(shape, spread)
    d, g = hq * 64, hkv * 64
    _, deq = R.v_image(x[:, 2 * d + g:], cu, hkv)
    ref, terms = R.pv8_attention(x, cu, hq, hkv, deq, gate)
    bound = R.element_bound(ref, terms, cu, hq)
    assert bool((bound > terms["quant"] * terms["g"]).all())
    for lag in (0.0, R.LAG):
        model = R.pv8_model(x, cu, hq, hkv, deq, gate, lag=lag)
        e = (model - ref).abs()
        assert bool((e <= terms["quant"] * terms["g"] * (1 + 1e-12)).all()), (lag, float((e / (terms["quant"] * terms["g"])).max()))


def test_spiked_rows_are_what_they_claim():
    x, cu, aligned = R.spiked_rows()
    s = x[aligned, :64].double() @ x[:, 256:320].double().t()
    top = s.topk(2, dim=1)
    assert float((top.values[:, 0] - top.values[:, 1]).min()) > 140.0 and set(top.indices[:, 0].tolist()) == {300}
    for key in (66, 133, 232):          # lower lane half, upper lane half, second half of the tile: pv8_ref.fragment_key's inverse
        assert key >= 64
    assert (66 % 64) & 4 == 0 and (133 % 64) & 4 == 4 and (232 % 64) >= 32
