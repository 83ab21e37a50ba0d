"""Activation recompute, the part that needs no GPU: the tape size functions (host code) and the Python switches.

The tape of a training tower (csrc/ttv_train.hip, carve_tape), every buffer rounded up to 256 bytes, e = bytes of the compute dtype,
ye = bytes of the KEEL sums (2 in a bf16 tower, 4 in an fp32 one), L rows, P patch rows, K latent rows, d width, g = kv_heads * 64,
I inner width:

  head / tail   encoder: patches [P, patch_dim], pe [P, d], agc [K, d], xc [K, d]       decoder: hpre [K, d], pn [P, d]
  boundaries    (layers + 1) x [L, d]
  one layer     xn1 [L, d], qkvg [L, 2d + 2g], lse [L, q_heads] fp32, a [L, d], ag [L, d], y1 [L, d] (ye), x1 [L, d], xn2 [L, d],
                u [L, 2I], h [L, I], y2 [L, d] (ye)          - layer 0 has no y1 / y2

  TTV_TAPE_STORED    : head / tail + boundaries + layers x layer, less the two y buffers layer 0 lacks
  TTV_TAPE_RECOMPUTE : head / tail + boundaries + min(2, layers) x slot, a slot being a layer WITH y1 / y2

so for layers >= 2:  stored - recompute == (layers - 2) * slot - 2 * align256(L * d * ye).
"""
import ctypes as C
from types import SimpleNamespace

import pytest

from titok_video_amd import _lib
from titok_video_amd.model.base.utils import geglu_inner_dim, get_model_dims

LEVELS = [7, 5, 5, 5, 5]
PATCH = (4, 8, 8)
# (clips, (T, H, W), K): a small ragged-free batch per size, and config #4's base batch (32 clips of 32x256x256, K = 1024)
BATCHES = {"tiny": (5, (16, 128, 128), 128), "small": (3, (8, 64, 64), 40), "base": (32, (32, 256, 256), 1024)}


@pytest.fixture(scope="module")
def handle():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


def a256(n):
    return (n + 255) // 256 * 256


def dims_for(size, kind, dtype):
    width, layers, heads, mlp_ratio = get_model_dims(size)
    return _lib.TowerDims(kind=kind, dtype=dtype, width=width, layers=layers, q_heads=heads[0], kv_heads=heads[1], head_dim=64,
                          inner=geglu_inner_dim(width, mlp_ratio), patch_t=PATCH[0], patch_h=PATCH[1], patch_w=PATCH[2], pix_channels=3,
                          token_size=5, eps=1e-5, alpha=float(2 * layers))


def batch_for(size):
    n, (t, h, w), k = BATCHES[size]
    p = (t // PATCH[0]) * (h // PATCH[1]) * (w // PATCH[2])
    return _lib.Batch(n_clips=n, total_rows=n * (p + k), sum_tokens=n * k, sum_patches=n * p)


def layer_bytes(d, b, with_y):
    """One layer's region, from the field list of the module docstring."""
    e = 2 if d.dtype == _lib.TTV_BF16 else 4
    ye = e                                              # (the suite runs without TTV_TAPE_Y_F32 / TTV_TRAIN_FUSED_NORMS, which make it 4)
    L, dm, g, I = b.total_rows, d.width, d.kv_heads * 64, d.inner
    fields = [L * dm * e, L * (2 * dm + 2 * g) * e, L * d.q_heads * 4, L * dm * e, L * dm * e, L * dm * ye if with_y else 0,
              L * dm * e, L * dm * e, L * 2 * I * e, L * I * e, L * dm * ye if with_y else 0]
    return sum(a256(f) for f in fields), a256(L * dm * ye)


def fixed_bytes(d, b):
    e = 2 if d.dtype == _lib.TTV_BF16 else 4
    L, P, K, dm = b.total_rows, b.sum_patches, b.sum_tokens, d.width
    pd = d.pix_channels * d.patch_t * d.patch_h * d.patch_w
    head = [P * pd * e, P * dm * e, K * dm * e, K * dm * e] if d.kind == _lib.TTV_ENCODER else [K * dm * e, P * dm * e]
    return sum(a256(f) for f in head) + (d.layers + 1) * a256(L * dm * e)


@pytest.mark.parametrize("size", ["tiny", "small", "base"])
@pytest.mark.parametrize("dtype", [_lib.TTV_BF16, _lib.TTV_F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("kind", [_lib.TTV_ENCODER, _lib.TTV_DECODER], ids=["encoder", "decoder"])
def test_tape_sizes_of_both_modes(handle, kind, dtype, size):
    d, b = dims_for(size, kind, dtype), batch_for(size)
    plain = handle.ttv_tower_tape_bytes(C.byref(d), C.byref(b))
    stored = handle.ttv_tower_tape_bytes_ex(C.byref(d), C.byref(b), _lib.TTV_TAPE_STORED)
    rec = handle.ttv_tower_tape_bytes_ex(C.byref(d), C.byref(b), _lib.TTV_TAPE_RECOMPUTE)
    assert stored == plain > 0
    slot, ybytes = layer_bytes(d, b, True)
    assert d.layers >= 2
    assert stored - rec == (d.layers - 2) * slot - 2 * ybytes
    # and each total on its own, so that the identity cannot hold by two equal mistakes
    assert stored == fixed_bytes(d, b) + d.layers * slot - 2 * ybytes
    assert rec == fixed_bytes(d, b) + 2 * slot
    # the backward workspace does not depend on the mode
    ws = handle.ttv_tower_bwd_workspace_bytes(C.byref(d), C.byref(b))
    assert ws > 0
    for mode in (_lib.TTV_TAPE_STORED, _lib.TTV_TAPE_RECOMPUTE):
        assert handle.ttv_tower_bwd_workspace_bytes_ex(C.byref(d), C.byref(b), mode) == ws


def test_a_single_layer_tower_has_one_slot(handle):
    d, b = dims_for("tiny", _lib.TTV_DECODER, _lib.TTV_BF16), batch_for("tiny")
    d.layers = 1
    slot, _ = layer_bytes(d, b, True)
    assert handle.ttv_tower_tape_bytes_ex(C.byref(d), C.byref(b), _lib.TTV_TAPE_RECOMPUTE) == fixed_bytes(d, b) + slot


def test_base_towers_at_the_batch_of_config_4(handle):
    """12 layers against 2 slots plus 13 boundaries: the recompute tape is under a third of the stored one."""
    b = batch_for("base")
    assert b.total_rows == 294912
    for kind, name in ((_lib.TTV_ENCODER, "encoder"), (_lib.TTV_DECODER, "decoder")):
        d = dims_for("base", kind, _lib.TTV_BF16)
        stored = handle.ttv_tower_tape_bytes_ex(C.byref(d), C.byref(b), _lib.TTV_TAPE_STORED)
        rec = handle.ttv_tower_tape_bytes_ex(C.byref(d), C.byref(b), _lib.TTV_TAPE_RECOMPUTE)
        print(f"base {name}, 32 clips of 32x256x256, K = 1024, bf16: stored tape {stored / 2**30:.1f} GiB, recompute tape {rec / 2**30:.1f} GiB")
        assert 0 < rec < stored / 3


def test_unknown_tape_mode_is_refused(handle):
    d, b = dims_for("tiny", _lib.TTV_ENCODER, _lib.TTV_BF16), batch_for("tiny")
    for mode in (2, -1, 7):
        assert handle.ttv_tower_tape_bytes_ex(C.byref(d), C.byref(b), mode) == -1
        assert handle.ttv_tower_bwd_workspace_bytes_ex(C.byref(d), C.byref(b), mode) == -1
        # the mode is judged before anything else: nothing here reaches the GPU
        rcs = [handle.ttv_encoder_forward_train_ex(C.byref(d), None, C.byref(b), None, None, None, 0, None, mode),
               handle.ttv_encoder_backward_ex(C.byref(d), None, None, C.byref(b), None, None, None, None, None, 0, None, mode),
               handle.ttv_decoder_forward_train_ex(C.byref(d), None, C.byref(b), None, None, None, 0, None, 0, None, mode),
               handle.ttv_decoder_backward_ex(C.byref(d), None, None, C.byref(b), None, None, None, None, None, None, 0, None, mode)]
        for rc in rcs:
            assert rc == 1                                              # TTV_ERR_INVALID
            assert b"tape mode" in handle.ttv_error_string()


# ---------------------------------------------------------------------------------------------- the Python surface
def _config(**model_keys):
    return SimpleNamespace(tokenizer=SimpleNamespace(model=SimpleNamespace(
        patch_size=list(PATCH), fsq_levels=LEVELS, encoder_size="tiny", decoder_size="tiny", **model_keys)))


def test_tower_attribute_and_the_tokenizer_switch():
    from titok_video_amd.model.base.blocks import TiTokDecoder, TiTokEncoder
    from titok_video_amd.model.titok import TiTok
    assert TiTokEncoder().activation_recompute is False and TiTokDecoder().activation_recompute is False
    m = TiTok(_config())
    assert m.encoder.activation_recompute is False and m.decoder.activation_recompute is False      # key absent: off
    assert m.set_activation_recompute(True) is m
    assert m.encoder.activation_recompute is True and m.decoder.activation_recompute is True
    m.set_activation_recompute(False)
    assert m.encoder.activation_recompute is False and m.decoder.activation_recompute is False
    on = TiTok(_config(activation_recompute=True))
    assert on.encoder.activation_recompute is True and on.decoder.activation_recompute is True
    assert set(on.state_dict()) == set(m.state_dict())                  # a switch, not a parameter


def _loss_config(**disc_keys):
    cfg = _config()
    cfg.tokenizer.losses = SimpleNamespace(perceptual_weight=0.0, gram_weight=0.0, disc_weight=0.1)
    cfg.discriminator = SimpleNamespace(losses=SimpleNamespace(gp_weight=0.0, gp_noise=0.01, centering_weight=0.0),
                                        model=SimpleNamespace(model_size="tiny", patch_size=list(PATCH), **disc_keys))
    cfg.training = SimpleNamespace(main=SimpleNamespace(max_steps=10))
    return cfg


def test_discriminator_config_key():
    from titok_video_amd.model.losses.loss_module import ReconstructionLoss
    assert ReconstructionLoss(_loss_config()).disc_model.activation_recompute is False              # key absent: off
    assert ReconstructionLoss(_loss_config(activation_recompute=True)).disc_model.activation_recompute is True
    assert ReconstructionLoss(_loss_config(activation_recompute=False)).disc_model.activation_recompute is False
