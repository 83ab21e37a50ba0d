"""Host side of the whole-video path (titok_video_amd/video.py): the tile plan, the numeric conditions the GPU identity test rests on,
and the token container, against the numpy restatement of tests/video_ref.py.  No GPU."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import video_ref as VR  # noqa: E402

from titok_video_amd import video as V  # noqa: E402

F32 = np.float32
AXES = [((30, 16, 4), 16, [0, 12, 14]), ((20, 8, 4), 8, [0, 4, 8, 12]), ((40, 32, 8), 32, [0, 8]), ((56, 32, 8), 32, [0, 24]),
        ((16, 16, 4), 16, [0]), ((17, 16, 4), 16, [0, 1]), ((5, 8, 2), 8, [0])]


# ---- plan -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,tile_eff,origins", AXES)
def test_axis_origins(case, tile_eff, origins):
    n, tile, o = case
    for axis in range(3):       # the same rule on every axis, the other two a single full tile
        video, tiles, overlap = [8, 8, 8], [8, 8, 8], [0, 0, 0]
        video[axis], tiles[axis], overlap[axis] = n, tile, o
        plan = V.TilePlan(video, tiles, overlap, (4, 4, 4))
        assert plan.origins[axis] == origins and plan.tile[axis] == tile_eff
        assert plan.counts[axis] == len(origins) and plan.n_tiles == len(origins)
        ref = VR.Plan(video, tiles, overlap, (4, 4, 4))
        assert ref.origins[axis] == origins and ref.tile == plan.tile
    assert VR.axis_plan(n, tile, o, 4) == (tile_eff, origins)


def test_short_axis_is_one_padded_tile_on_the_patch_lattice():
    plan = V.TilePlan((5, 30, 9), (8, 16, 16), (2, 4, 4), (4, 8, 8))
    assert plan.tile == (8, 16, 16) and plan.origins == ([0], [0, 12, 14], [0])
    assert V.TilePlan((3, 16, 16), (16, 16, 16), (4, 4, 4), (4, 8, 8)).tile == (4, 16, 16)


def test_tile_order_and_timeline():
    plan = V.TilePlan((11, 37, 45), (8, 16, 24), (4, 8, 8), (4, 8, 8), frame_stride=2)
    assert plan.timeline == (6, 37, 45) and plan.tile == (8, 16, 24)
    assert plan.origins == ([0], [0, 8, 16, 21], [0, 16, 21])
    ref = VR.Plan((11, 37, 45), (8, 16, 24), (4, 8, 8), (4, 8, 8), 2)
    seen = []
    for kt, kh, kw in itertools.product(*(range(c) for c in plan.counts)):
        index = (kt * plan.counts[1] + kh) * plan.counts[2] + kw
        assert plan.tile_origin(index) == (plan.origins[0][kt], plan.origins[1][kh], plan.origins[2][kw]) == ref.origin(index)
        seen.append(index)
    assert seen == list(range(plan.n_tiles))
    assert plan.patches_per_tile == 2 * 2 * 3
    c = plan.c_plan()
    assert (c.T, c.H, c.W, c.frame_stride) == (11, 37, 45, 2) and list(c.tile) == [8, 16, 24] and list(c.count) == [1, 4, 3]


@pytest.mark.parametrize("n,tile,o", [a[0] for a in AXES] + [(64, 16, 8), (33, 16, 8), (100, 8, 0), (31, 16, 7), (9, 8, 4), (1, 4, 0)])
def test_every_point_is_covered_one_to_three_times_with_positive_weights(n, tile, o):
    plan = V.TilePlan((n, 8, 8), (tile, 8, 8), (o, 0, 0), (4, 8, 8))
    cover = np.zeros(n, dtype=int)
    w = plan.axis_weights(0)
    assert len(w) == plan.tile[0] and min(w) >= 1 and max(w) <= o + 1 and w == w[::-1] and w == VR.Plan((n, 8, 8), (tile, 8, 8), (o, 0, 0), (4, 8, 8)).weights(0).tolist()
    for t0 in plan.origins[0]:
        assert t0 >= 0 and (t0 + plan.tile[0] <= n or len(plan.origins[0]) == 1)
        cover[t0:t0 + plan.tile[0]] += 1
    assert cover.min() >= 1 and cover.max() <= 3
    assert plan.origins[0] == sorted(set(plan.origins[0]))
    if (n, tile, o) == (30, 16, 4):
        assert cover[14] == cover[15] == 3


@pytest.mark.parametrize("kwargs", [
    dict(tile=(6, 16, 16)), dict(tile=(8, 16, 12)), dict(tile=(0, 16, 16)), dict(overlap=(-1, 4, 4)), dict(overlap=(5, 4, 4)),
    dict(overlap=(4, 9, 4)), dict(frame_stride=0), dict(tile=(512, 512, 512), overlap=(255, 255, 255), patch=(4, 8, 8)),
    dict(video=(0, 16, 16)), dict(tile=(8, 16))])
def test_refused_arguments(kwargs):
    args = dict(video=(20, 40, 56), tile=(8, 16, 16), overlap=(4, 4, 4), patch=(4, 8, 8), frame_stride=1)
    V.TilePlan(**args)
    args.update(kwargs)
    with pytest.raises(ValueError):
        V.TilePlan(**args)


def test_largest_weight_stays_below_2_to_24():
    V.TilePlan((8, 8, 8), (512, 512, 256), (255, 255, 127), (4, 8, 8))          # 256 * 256 * 128 = 2^23
    assert (255 + 1) * (255 + 1) * (255 + 1) == 1 << 24


# ---- the conditions the GPU identity test rests on ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_every_level_survives_the_round_trip(dtype):
    levels = np.arange(256)
    d = VR.unit_from_u8(levels, dtype)
    assert d.dtype == F32 and d[0] == -1 and d[255] == 1
    assert (VR.levels_of(d) == levels).all()
    err = np.abs((d.astype(np.float64) + 1.0) * 127.5 - levels).max()
    assert err <= (0.2461 if dtype == "bf16" else 1e-4), err
    if dtype == "bf16":
        assert err > 0.24                                   # the figure is the format's, not slack
        assert (d == torch.from_numpy(VR.unit_from_u8(levels, "f32")).to(torch.bfloat16).float().numpy()).all()      # torch's rounding


def test_a_weighted_mean_of_identical_values_stays_put():
    rng = np.random.default_rng(0)
    values = np.unique(np.concatenate([VR.unit_from_u8(np.arange(256), "f32"), VR.unit_from_u8(np.arange(256), "bf16")]))
    worst = 0.0
    for trial in range(400):
        n = int(rng.integers(2, 28))
        hi = [1, 5, 17 * 17 * 5, (1 << 24) - 1][trial % 4]
        w = rng.integers(1, hi + 1, size=n)
        num = np.zeros_like(values)
        for wk in w:
            num = num + F32(wk) * values
        q = num / F32(int(w.sum()))
        assert q.dtype == F32
        worst = max(worst, float(np.abs(q.astype(np.float64) - values).max()))
    assert worst < 1e-6, worst


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("stride", [1, 3])
def test_restatement_gather_then_blend_is_the_identity(dtype, stride):
    rng = np.random.default_rng(stride)
    frames = rng.integers(0, 256, size=(20, 24, 28, 3), dtype=np.uint8)
    frames[0, 0, 0], frames[-1, -1, -1] = 0, 255
    plan = VR.Plan(frames.shape[:3], (8, 16, 16), (4, 8, 8), (4, 8, 8), stride)
    tiles = VR.gather(frames, plan, 0, plan.n_tiles, dtype)
    assert (VR.blend(list(tiles), plan) == frames[::stride]).all()
    t0, t1 = 1, plan.timeline[0] - 1
    assert (VR.blend(list(tiles), plan, t0, t1) == frames[::stride][t0:t1]).all()


def test_restatement_blend_by_hand():
    # two tiles along W, overlap 2: weights (1, 2, 3, 3, ..., 3, 2, 1); tile (1, 1, 8) over n = 14 has origins 0, 6
    plan = VR.Plan((1, 1, 14), (1, 1, 8), (0, 0, 2), (1, 1, 1))
    assert plan.origins[2] == [0, 6] and plan.weights(2).tolist() == [1, 2, 3, 3, 3, 3, 2, 1]
    a = np.full((3, 1, 1, 8), F32(-1.0))
    b = np.full((3, 1, 1, 8), F32(1.0))
    a[0, 0, 0, 7], b[1, 0, 0, 0] = np.nan, 2.5
    out = VR.blend([a, b], plan)[0, 0]
    assert out[:6, 2].tolist() == [0] * 6 and out[8:, 2].tolist() == [255] * 6
    # x = 6: a's u = 6 (w 2) and b's u = 0 (w 1): (2 * -1 + 1 * 1) / 3 = -1/3 -> (2/3) * 127.5 = 85; x = 7: (1 * -1 + 2 * 1) / 3 -> 170
    assert out[6, 2] == 85 and out[7, 2] == 170
    assert out[7, 0] == 0                                    # a NaN in either tile is a NaN, level 0
    assert out[6, 1] == 85 and out[8, 1] == 255              # 2.5 clamps to 1


# ---- container --------------------------------------------------------------------------------------------------------------------------
def _tokens(codebook, seed, quantizer="fsq"):
    rng = np.random.default_rng(seed)
    plan = V.TilePlan((20, 40, 56), (8, 32, 32), (4, 8, 8), (4, 8, 8), 3)
    counts = [int(k) for k in rng.integers(1, 12, size=plan.n_tiles)]
    counts[0], counts[-1] = 1, 11                       # ragged whatever the draw
    idx = rng.integers(0, codebook, size=sum(counts))
    idx[0], idx[-1] = codebook - 1, 0
    return V.VideoTokens(torch.from_numpy(idx.astype(np.int32)), counts, (20, 40, 56), (8, 32, 32), (4, 8, 8), (4, 8, 8), 3, 8.0, codebook, quantizer)


@pytest.mark.parametrize("codebook,bits", [(2, 1), (4375, 13), (16384, 14), (16385, 15)])
def test_container_round_trip(codebook, bits, tmp_path):
    tok = _tokens(codebook, seed=bits)
    assert V.index_bits(codebook) == VR.index_bits(codebook) == bits
    data = tok.to_bytes()
    header, stored = VR.parse_container(data)
    assert stored == tok.indices.tolist() and header["bits"] == bits and header["counts"] == tok.counts
    n = len(stored)
    assert data.endswith(VR.pack(stored, bits)) and len(data) == 16 + len(data[16:]) and len(VR.pack(stored, bits)) == (n * bits + 7) // 8
    path = tmp_path / "clip.ttvtok"
    tok.save(path)
    back = V.VideoTokens.load(path)
    assert torch.equal(back.indices, tok.indices) and back.indices.dtype == torch.int32 and back.counts == tok.counts
    for name in ("video", "tile", "overlap", "patch", "frame_stride", "fps", "codebook_size", "quantizer"):
        assert getattr(back, name) == getattr(tok, name), name
    assert back.plan().origins == tok.plan().origins
    assert tok.bits_per_pixel == 8 * len(data) / (7 * 40 * 56)


def test_uniform_counts_are_stored_once_and_one_bit_indices_pack():
    tok = V.VideoTokens(torch.tensor([1, 0, 1, 1, 0, 1, 0, 0, 1], dtype=torch.int32), [3, 3, 3], (8, 8, 8), (8, 8, 8), (0, 0, 0), (4, 8, 8), 1, None, 2, "l2")
    data = tok.to_bytes()
    header, stored = VR.parse_container(data)
    assert header["counts"] == 3 and header["n_tiles"] == 3 and stored == tok.indices.tolist()
    assert data[-2:] == bytes([0b00101101, 0b1])
    back = V.VideoTokens.from_bytes(data)
    assert back.counts == [3, 3, 3] and back.fps is None and back.quantizer == "l2"


def test_truncated_or_foreign_streams_raise():
    data = _tokens(4375, seed=1).to_bytes()
    V.VideoTokens.from_bytes(data)
    for bad in (data[:-1], data[:40], data[:12], b"", b"RIFF" + data[4:], data + b"\0", data[:8] + (2).to_bytes(4, "little") + data[12:],
                data[:16] + b"{" * 10 + data[26:]):
        with pytest.raises(ValueError):
            V.VideoTokens.from_bytes(bad)
    with pytest.raises(ValueError):
        V.VideoTokens(torch.zeros(5, dtype=torch.int32), [2, 2], (8, 8, 8), (8, 8, 8), (0, 0, 0), (4, 8, 8), 1, None, 16, "fsq")
    with pytest.raises(ValueError):        # an index outside the codebook is not written
        V.VideoTokens(torch.tensor([16], dtype=torch.int32), [1], (8, 8, 8), (8, 8, 8), (0, 0, 0), (4, 8, 8), 1, None, 16, "fsq").to_bytes()


# ---- no CPU path ------------------------------------------------------------------------------------------------------------------------
def test_host_tensors_raise():
    plan = V.TilePlan((8, 16, 16), (8, 16, 16), (0, 0, 0), (4, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        V.gather_tiles(torch.zeros(8, 16, 16, 3, dtype=torch.uint8), plan)
    with pytest.raises(RuntimeError, match="no CPU path"):
        V.blend_tiles([torch.zeros(3, 8, 16, 16)], plan)
    from types import SimpleNamespace

    from titok_video_amd.model.titok import TiTok
    cfg = SimpleNamespace(tokenizer=SimpleNamespace(model=SimpleNamespace(patch_size=[4, 8, 8], fsq_levels=[7, 5, 5, 5, 5], encoder_size="tiny",
                                                                          decoder_size="tiny")))
    with pytest.raises(RuntimeError, match="no CPU path"):
        V.VideoTokenizer(TiTok(cfg), tile=(8, 32, 32))


def test_budget_ranges_follow_the_reference_rule():
    assert V._budget_ranges([40] * 16, 0, 16, 200) == [(0, 5), (5, 10), (10, 15), (15, 16)]
    assert V._budget_ranges([40] * 16, 4, 8, 6144) == [(4, 8)]
    assert V._budget_ranges([100, 150, 60, 10, 200], 0, 5, 200) == [(0, 1), (1, 2), (2, 4), (4, 5)]
