"""The whole-video path on the MI355X: `ttv_video_tiles_u8` and `ttv_video_blend_u8` (csrc/ttv_video.hip) through the C ABI, bit for
bit against the numpy restatement of tests/video_ref.py, and `video.VideoTokenizer` end to end against the same steps done by hand
around the public `TiTok.encode` / `decode_indices`.  Every value is defined bit for bit, so no byte may differ.  `-m gpu`.

Every output lies in a buffer filled with a canary and longer than the output on both sides."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import video_ref as VR  # noqa: E402

from titok_video_amd import _lib  # noqa: E402
from titok_video_amd import video as V  # noqa: E402
from titok_video_amd.model.titok import TiTok  # noqa: E402
from titok_video_amd.synthetic import seeded_titok_state  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
CANARY_U8, CANARY_F, GUARD = 0xA5, 77.0, 64


def S():
    return _lib.stream_ptr(torch.device(DEV))


def both(video, tile, overlap, patch, stride=1):
    """The package's plan and the restatement's, which must agree before anything is compared."""
    plan, ref = V.TilePlan(video, tile, overlap, patch, stride), VR.Plan(video, tile, overlap, patch, stride)
    assert plan.tile == ref.tile and list(plan.origins) == ref.origins
    return plan, ref


def random_frames(shape, seed):
    g = torch.Generator().manual_seed(seed)
    f = torch.randint(0, 256, tuple(shape) + (3,), generator=g, dtype=torch.uint8)
    f.view(-1)[0], f.view(-1)[-1] = 0, 255
    return f


def raw_gather(frames_dev, plan, begin, end, dt, cplan=None, out_shift=0, dtype_code=None):
    """The C entry point into a canary-filled buffer with GUARD elements on either side.  Returns (rc, tiles as float32 numpy)."""
    n = (end - begin) * 3 * plan.tile[0] * plan.tile[1] * plan.tile[2]
    buf = torch.full((max(n, 0) + 2 * GUARD,), CANARY_F, dtype=DTYPES[dt], device=DEV)
    cp = plan.c_plan() if cplan is None else cplan
    rc = _lib.lib().ttv_video_tiles_u8(frames_dev.data_ptr() if frames_dev is not None else None, C.byref(cp), begin, end,
                                       buf.data_ptr() + GUARD * buf.element_size() + out_shift,
                                       _lib.dtype_code(DTYPES[dt]) if dtype_code is None else dtype_code, S())
    torch.cuda.synchronize()
    h = buf.float().cpu().numpy()
    if rc != 0:
        assert (h == CANARY_F).all(), "a refused call wrote something"
        return rc, None
    assert (h[:GUARD] == CANARY_F).all() and (h[GUARD + n:] == CANARY_F).all(), "elements outside the tiles were written"
    return rc, h[GUARD:GUARD + n].reshape((end - begin, 3) + plan.tile)


def same_bits(got, want, what):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert bad == 0, f"{what}: {bad} of {want.size} elements differ"


# ---- gather -----------------------------------------------------------------------------------------------------------------------------
GATHER = {
    "stride 2, T shorter than the tile": ((11, 37, 45), (8, 16, 24), (4, 8, 8), (4, 8, 8), 2, None),
    "stride 1, a tile range": ((11, 37, 45), (8, 16, 24), (4, 8, 8), (4, 8, 8), 1, (5, 19)),
    "every axis shorter than the tile": ((5, 9, 13), (8, 16, 24), (4, 8, 8), (4, 8, 8), 1, None),
    "Wt no multiple of 8": ((9, 21, 27), (8, 16, 12), (4, 8, 4), (4, 8, 4), 1, None),
}


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("case", list(GATHER))
def test_gather_is_exact(case, dt):
    video, tile, overlap, patch, stride, rng = GATHER[case]
    plan, ref = both(video, tile, overlap, patch, stride)
    begin, end = rng if rng else (0, plan.n_tiles)
    assert 0 <= begin < end <= plan.n_tiles
    frames = random_frames(video, seed=sum(video))
    want = VR.gather(frames.numpy(), ref, begin, end, dt)
    rc, got = raw_gather(frames.to(DEV), plan, begin, end, dt)
    assert rc == 0
    same_bits(got, want, f"{case} {dt}")
    # the same frames one byte off the word grid: the first and the last words of the array are out of bounds for a 4-byte load
    shifted = torch.zeros(frames.numel() + 1, dtype=torch.uint8, device=DEV)
    shifted[1:] = frames.view(-1).to(DEV)
    view = shifted[1:].view(frames.shape)
    assert view.data_ptr() % 4 == 1
    rc, got = raw_gather(view, plan, begin, end, dt)
    assert rc == 0
    same_bits(got, want, f"{case} {dt}, frames one byte off the word grid")
    same_bits(V.gather_tiles(view, plan, begin, end, DTYPES[dt]).float().cpu().numpy(), want, f"gather_tiles, {case} {dt}")


def test_gather_matches_the_loader_bits():
    """A tile that is the whole clip holds what ttv_clip_from_u8 gives for it."""
    plan, _ = both((8, 16, 24), (8, 16, 24), (0, 0, 0), (4, 8, 8))
    frames = random_frames((8, 16, 24), seed=3).to(DEV)
    for dt in DTYPES.values():
        clip = torch.empty((3, 8, 16, 24), dtype=dt, device=DEV)
        _lib.check(_lib.lib().ttv_clip_from_u8(frames.data_ptr(), 8, 16, 24, clip.data_ptr(), _lib.dtype_code(dt), S()), "clip_from_u8")
        assert torch.equal(V.gather_tiles(frames, plan, dtype=dt)[0], clip)


def test_gather_refuses_bad_arguments():
    plan, _ = both((11, 37, 45), (8, 16, 24), (4, 8, 8), (4, 8, 8))
    frames = random_frames((11, 37, 45), seed=1).to(DEV)
    assert raw_gather(frames, plan, 0, 2, "bf16")[0] == 0
    assert raw_gather(frames, plan, 3, 3, "bf16")[0] == 0                           # an empty range is no error and no launch
    assert raw_gather(frames, plan, 0, 2, "bf16", dtype_code=7)[0] == 1
    assert raw_gather(None, plan, 0, 2, "bf16")[0] == 1
    assert raw_gather(frames, plan, 0, 2, "bf16", out_shift=2)[0] == 1             # a destination off the 16-byte grid
    assert raw_gather(frames, plan, 0, plan.n_tiles + 1, "bf16")[0] == 1 and raw_gather(frames, plan, -1, 2, "bf16")[0] == 1
    for field, value in (("count", (2, 5, 3)), ("count", (3, 4, 3)), ("overlap", (5, 8, 8)), ("overlap", (4, -1, 8)), ("tile", (8, 0, 24))):
        cp = plan.c_plan()
        setattr(cp, field, (_lib.i32 * 3)(*value))
        assert raw_gather(frames, plan, 0, 2, "bf16", cplan=cp)[0] == 1, (field, value)    # e.g. an origin outside the timeline
    cp = plan.c_plan()
    cp.frame_stride = 0
    assert raw_gather(frames, plan, 0, 2, "bf16", cplan=cp)[0] == 1
    assert b"video_tiles_u8" in _lib.lib().ttv_error_string()
    with pytest.raises(ValueError):
        V.gather_tiles(frames[:, :, :44], plan)


# ---- blend ------------------------------------------------------------------------------------------------------------------------------
def raw_blend(tiles, plan, t0, t1, lead=0, dtype_code=None, null_table=False):
    """The C entry point on device tiles (None = NULL) into a canary-filled byte buffer, `lead` bytes in.  Returns (rc, frames)."""
    Tn, H, W = plan.timeline
    n = max(t1 - t0, 0) * H * W * 3
    buf = torch.full((lead + n + GUARD,), CANARY_U8, dtype=torch.uint8, device=DEV)
    ptrs = [0 if t is None else t.data_ptr() for t in tiles]
    host = (C.c_void_p * len(ptrs))(*ptrs)
    table = torch.tensor(ptrs, dtype=torch.int64).to(DEV)
    dt = next(t.dtype for t in tiles if t is not None)
    cp = plan.c_plan()
    rc = _lib.lib().ttv_video_blend_u8(None if null_table else host, table.data_ptr(), C.byref(cp), t0, t1,
                                       _lib.dtype_code(dt) if dtype_code is None else dtype_code, buf.data_ptr() + lead, S())
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    if rc != 0:
        assert (h == CANARY_U8).all(), "a refused call wrote something"
        return rc, None
    assert (h[:lead] == CANARY_U8).all() and (h[lead + n:] == CANARY_U8).all(), "bytes outside the frames were written"
    return rc, h[lead:lead + n].reshape(max(t1 - t0, 0), H, W, 3)


def random_tiles(plan, dt, seed, nans=True):
    """Per tile U(-1.5, 1.5) with exact +-1, +-1.5 and NaNs planted; device tensors, one allocation each."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(plan.n_tiles):
        x = torch.rand((3,) + plan.tile, generator=g) * 3.0 - 1.5
        f = x.view(-1)
        for j, v in enumerate((1.0, -1.0, 1.5, -1.5, 0.0)):
            f[(j * 53 + 7 * k + 1) % f.numel()] = v
        if nans:
            f[(11 * k + 3) % f.numel()] = float("nan")
            f[(97 * k + 29) % f.numel()] = float("nan")
        out.append(x.to(DTYPES[dt]).to(DEV))
    return out


def host_tiles(tiles):
    return [None if t is None else t.float().cpu().numpy() for t in tiles]


def check_blend(tiles, plan, ref, t0, t1, what, leads=(0, 1)):
    want = VR.blend(host_tiles(tiles), ref, t0, t1)
    for lead in leads:
        rc, got = raw_blend(tiles, plan, t0, t1, lead)
        assert rc == 0, _lib.lib().ttv_error_string()
        bad = int((got != want).sum())
        assert got.shape == want.shape and bad == 0, f"{what}, output {lead} bytes off: {bad} of {want.size} bytes differ"
    return want


BLEND = {
    "odd sizes, every axis overlapped": ((11, 37, 45), (8, 16, 24), (4, 8, 8), (4, 8, 8)),
    "triple cover along T": ((30, 8, 8), (16, 8, 8), (4, 0, 0), (4, 8, 8)),
    "triple cover along H": ((4, 30, 8), (4, 16, 8), (0, 4, 0), (4, 8, 8)),
    "triple cover along W": ((4, 8, 30), (4, 8, 16), (0, 0, 4), (4, 8, 8)),
    "triple cover on all three": ((30, 30, 30), (16, 16, 16), (4, 4, 4), (4, 8, 8)),
    "overlap 0, pure stitching": ((16, 32, 48), (8, 16, 24), (0, 0, 0), (4, 8, 8)),
    "a single padded tile": ((5, 9, 13), (8, 16, 24), (4, 8, 8), (4, 8, 8)),
    "W a multiple of 4, Wt not of 8": ((9, 21, 28), (8, 16, 12), (4, 8, 4), (4, 8, 4)),
}


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("case", list(BLEND))
def test_blend_is_exact(case, dt):
    video, tile, overlap, patch = BLEND[case]
    plan, ref = both(video, tile, overlap, patch)
    tiles = random_tiles(plan, dt, seed=len(case))
    want = check_blend(tiles, plan, ref, 0, plan.timeline[0], f"{case} {dt}")
    assert want.min() == 0 and want.max() == 255
    got = V.blend_tiles(tiles, plan).cpu().numpy()
    assert (got == want).all(), f"blend_tiles, {case} {dt}"


@pytest.mark.parametrize("dt", list(DTYPES))
def test_blend_of_constant_tiles(dt):
    plan, ref = both((11, 37, 45), (8, 16, 24), (4, 8, 8), (4, 8, 8))
    vals = torch.linspace(-1.2, 1.2, plan.n_tiles)
    tiles = [torch.full((3,) + plan.tile, float(v), dtype=DTYPES[dt], device=DEV) for v in vals]
    want = check_blend(tiles, plan, ref, 0, plan.timeline[0], f"constant tiles {dt}")
    assert len(np.unique(want)) > plan.n_tiles                 # the overlaps hold mixtures, not only the tiles' own levels


@pytest.mark.parametrize("dt", list(DTYPES))
def test_blend_of_a_frame_range_with_null_tiles(dt):
    plan, ref = both((20, 40, 56), (8, 32, 32), (4, 8, 8), (4, 8, 8))
    assert plan.origins[0] == [0, 4, 8, 12] and plan.tiles_per_layer == 4
    tiles = random_tiles(plan, dt, seed=9)
    part = [None] * 4 + tiles[4:12] + [None] * 4              # frames [9, 12) lie in layers 1 and 2 only
    want = check_blend(part, plan, ref, 9, 12, f"frames [9, 12) {dt}")
    assert (want == VR.blend(host_tiles(tiles), ref)[9:12]).all()
    assert (V.blend_tiles(part, plan, 9, 12).cpu().numpy() == want).all()
    # a covering tile that is NULL: the error, and nothing launched
    for hole in (4, 11):
        broken = list(part)
        broken[hole] = None
        rc, _ = raw_blend(broken, plan, 9, 12)
        assert rc == 1 and b"NULL" in _lib.lib().ttv_error_string()
    assert raw_blend(part, plan, 8, 12)[0] == 0 and raw_blend(part, plan, 7, 12)[0] == 1 and raw_blend(part, plan, 9, 13)[0] == 1


def test_blend_refuses_bad_arguments():
    plan, _ = both((11, 37, 45), (8, 16, 24), (4, 8, 8), (4, 8, 8))
    tiles = random_tiles(plan, "f32", seed=2, nans=False)
    n = plan.timeline[0]
    assert raw_blend(tiles, plan, 0, n)[0] == 0
    assert raw_blend(tiles, plan, 4, 4)[0] == 0                                     # an empty range is no error and no launch
    for t0, t1 in ((-1, 3), (0, n + 1), (5, 4)):
        assert raw_blend(tiles, plan, t0, t1)[0] == 1, (t0, t1)
    assert raw_blend(tiles, plan, 0, n, dtype_code=5)[0] == 1
    assert raw_blend(tiles, plan, 0, n, null_table=True)[0] == 1
    assert b"video_blend_u8" in _lib.lib().ttv_error_string()
    with pytest.raises(ValueError):
        V.blend_tiles(tiles[:-1], plan)
    with pytest.raises(ValueError):
        V.blend_tiles(tiles[:-1] + [tiles[-1][:, :, :, :16]], plan)


# ---- identity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("stride", [1, 3])
def test_gather_then_blend_returns_the_video(stride, dt):
    plan, _ = both((20, 40, 56), (8, 32, 32), (4, 8, 8), (4, 8, 8), stride)
    frames = random_frames((20, 40, 56), seed=stride)
    tiles = V.gather_tiles(frames.to(DEV), plan, dtype=DTYPES[dt])
    out = V.blend_tiles(list(tiles.unbind(0)), plan)
    assert out.dtype == torch.uint8 and tuple(out.shape) == plan.timeline + (3,)
    assert torch.equal(out.cpu(), frames[::stride])


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
VIDEO, TILE, OVERLAP, PATCH, K, SEQ = (20, 40, 56), (8, 32, 32), (4, 8, 8), (4, 8, 8), 8, 200


def tiny_model(quantizer="fsq"):
    if quantizer == "fsq":
        m = SimpleNamespace(patch_size=list(PATCH), fsq_levels=[7, 5, 5, 5, 5], encoder_size="tiny", decoder_size="tiny")
        sd = seeded_titok_state(0)
    else:
        m = SimpleNamespace(patch_size=list(PATCH), fsq_levels=None, quantizer="l2", codebook_size=256, token_size=8, encoder_size="tiny",
                            decoder_size="tiny")
        sd = seeded_titok_state(0, token_size=8)
    model = TiTok(SimpleNamespace(tokenizer=SimpleNamespace(model=m)))
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("quantize.") for k in missing)
    return model.to(DEV, torch.bfloat16).eval()


def by_hand(model, frames):
    """The same round trip around the public model calls: restatement-cut tiles uploaded, encoded in the batches the token budget
    gives (5 tiles of 40 rows under 200), decoded layer by layer, blended by the restatement."""
    ref = VR.Plan(VIDEO, TILE, OVERLAP, PATCH)
    assert ref.n_tiles == 16 and ref.tile == TILE
    cut = VR.gather(frames.numpy(), ref, 0, 16, "bf16")
    idx = []
    with torch.no_grad():
        for a, b in ((0, 5), (5, 10), (10, 15), (15, 16)):
            clips = [torch.from_numpy(cut[k]).to(torch.bfloat16).to(DEV) for k in range(a, b)]
            idx.append(model.encode(clips, [K] * (b - a))[1]["indices"])
        idx = torch.cat(idx)
        recon = []
        for layer in range(4):
            recon += model.decode_indices(idx[layer * 4 * K:(layer + 1) * 4 * K], [TILE] * 4, [K] * 4)
    return idx.cpu(), VR.blend([r.float().cpu().numpy() for r in recon], ref)


@pytest.fixture(scope="module")
def fsq_round_trip():
    model = tiny_model()
    frames = random_frames(VIDEO, seed=77)
    vt = V.VideoTokenizer(model, tile=TILE, overlap=OVERLAP, tokens_per_tile=K, seq_len=SEQ, dtype=torch.bfloat16, depth=2)
    tok = vt.encode_video(frames.to(DEV), fps=24.0)
    out = vt.decode_video(tok)
    torch.cuda.synchronize()
    return model, frames, vt, tok, out


def test_round_trip_equals_the_steps_done_by_hand(fsq_round_trip):
    model, frames, vt, tok, out = fsq_round_trip
    idx, want = by_hand(model, frames)
    assert tok.indices.dtype == torch.int32 and tok.counts == [K] * 16 and tok.fps == 24.0 and tok.codebook_size == 4375
    assert (tok.video, tok.tile, tok.overlap, tok.patch, tok.frame_stride, tok.quantizer) == (VIDEO, TILE, OVERLAP, PATCH, 1, "fsq")
    assert torch.equal(tok.indices.cpu(), idx.to(torch.int32))
    assert out.dtype == torch.uint8 and out.is_cuda and tuple(out.shape) == VIDEO + (3,)
    bad = int((out.cpu().numpy() != want).sum())
    assert bad == 0, f"{bad} of {want.size} bytes differ from the round trip done by hand"
    assert len(np.unique(want)) > 32                            # a picture, not a constant


def test_iter_yields_gap_free_ranges(fsq_round_trip):
    _, _, vt, tok, out = fsq_round_trip
    at, parts = 0, []
    for t0, part in vt.decode_video_iter(tok):
        assert t0 == at and part.shape[0] >= 1 and part.dtype == torch.uint8 and tuple(part.shape[1:]) == VIDEO[1:] + (3,)
        at += part.shape[0]
        parts.append(part)
    assert at == VIDEO[0] and [p.shape[0] for p in parts] == [4, 4, 4, 8]
    assert torch.equal(torch.cat(parts), out)


def test_three_runs_and_both_depths_are_identical(fsq_round_trip):
    model, frames, vt, tok, out = fsq_round_trip
    dev_frames = frames.to(DEV)
    one = V.VideoTokenizer(model, tile=TILE, overlap=OVERLAP, tokens_per_tile=K, seq_len=SEQ, dtype=torch.bfloat16, depth=1)
    for who in (vt, vt, one):
        again = who.encode_video(dev_frames, fps=24.0)
        assert torch.equal(again.indices, tok.indices)
        assert torch.equal(who.decode_video(again), out)


def test_frame_stride_and_ragged_counts(fsq_round_trip):
    model, frames, _, _, _ = fsq_round_trip
    counts = [3, 8, 5, 8]                                      # T' = 7 is one padded layer of 2 x 2 tiles
    vt = V.VideoTokenizer(model, tile=TILE, overlap=OVERLAP, tokens_per_tile=counts, seq_len=SEQ, dtype=torch.bfloat16, depth=2)
    tok = vt.encode_video(frames.to(DEV), fps=24.0, frame_stride=3)
    assert tok.counts == counts and tok.indices.numel() == sum(counts) and tok.fps == 8.0 and tok.plan().timeline == (7, 40, 56)
    out = vt.decode_video(tok)
    assert tuple(out.shape) == (7, 40, 56, 3)
    with pytest.raises(ValueError):
        vt.encode_video(frames.to(DEV))                        # 16 tiles, 4 counts


def test_tokens_survive_save_and_load(fsq_round_trip, tmp_path):
    _, _, vt, tok, out = fsq_round_trip
    tok.save(tmp_path / "v.ttvtok")
    back = V.VideoTokens.load(tmp_path / "v.ttvtok")
    assert not back.indices.is_cuda and torch.equal(back.indices, tok.indices.cpu())
    assert torch.equal(vt.decode_video(back), out)
    assert tok.bits_per_pixel == 8 * os.path.getsize(tmp_path / "v.ttvtok") / (20 * 40 * 56)


def test_tokens_that_do_not_fit_the_model_raise(fsq_round_trip):
    _, _, vt, tok, _ = fsq_round_trip

    def variant(**kw):
        args = dict(indices=tok.indices, counts=tok.counts, video=tok.video, tile=tok.tile, overlap=tok.overlap, patch=tok.patch,
                    frame_stride=1, fps=None, codebook_size=tok.codebook_size, quantizer=tok.quantizer)
        args.update(kw)
        return V.VideoTokens(**args)
    assert torch.equal(vt.decode_video(variant()), fsq_round_trip[4])
    for kw in (dict(codebook_size=4096), dict(quantizer="l2"), dict(patch=(4, 8, 4)), dict(tile=(8, 32, 36)),
               dict(video=(20, 40, 90)), dict(tile=(8, 64, 64))):
        with pytest.raises(ValueError):
            next(vt.decode_video_iter(variant(**kw)))


def test_l2_quantiser_round_trip():
    model = tiny_model("l2")
    frames = random_frames(VIDEO, seed=78)
    vt = V.VideoTokenizer(model, tile=TILE, overlap=OVERLAP, tokens_per_tile=K, seq_len=SEQ, dtype=torch.bfloat16, depth=2)
    tok = vt.encode_video(frames.to(DEV))
    assert tok.quantizer == "l2" and tok.codebook_size == 256 and tok.fps is None and int(tok.indices.max()) < 256
    idx, want = by_hand(model, frames)
    assert torch.equal(tok.indices.cpu(), idx.to(torch.int32))
    assert (vt.decode_video(tok).cpu().numpy() == want).all()


def test_tile_defaults_to_the_config_max_grid():
    model = tiny_model()
    with pytest.raises(ValueError, match="tile is required"):
        V.VideoTokenizer(model)
    model.config.training = SimpleNamespace(sampling=SimpleNamespace(max_grid=[16, 168, 168]))
    assert V.VideoTokenizer(model).tile == (16, 168, 168)


# ---- memory -----------------------------------------------------------------------------------------------------------------------------
def test_iter_holds_a_few_layers_not_the_video():
    """80 frames, tile 8, overlap 4: 19 temporal layers.  The yardstick is the same decode with every reconstruction kept until one
    blend of the whole timeline; the frames that come out are kept in both runs."""
    model = tiny_model()
    frames = random_frames((80, 64, 64), seed=5).to(DEV)
    vt = V.VideoTokenizer(model, tile=(8, 64, 64), overlap=(4, 0, 0), tokens_per_tile=K, seq_len=6144, dtype=torch.bfloat16, depth=1)
    tok = vt.encode_video(frames)
    plan = tok.plan()
    assert plan.counts == (19, 1, 1)
    warm = vt.decode_video(tok)                                 # plans, workspaces and packed weights exist from here on
    del warm

    def peak_of(run):
        import gc
        gc.collect()             # cyclic garbage of earlier tests still holds device memory: freed inside `run` it would lower the peak below `base`
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        kept = run()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, kept

    def streamed():
        return [part for _, part in vt.decode_video_iter(tok)]

    def all_kept():
        with torch.no_grad():
            recon = []
            for k in range(19):
                recon += model.decode_indices(tok.indices[k * K:(k + 1) * K], [plan.tile], [K])
            return [V.blend_tiles(recon, plan)]

    peak_iter, parts = peak_of(streamed)
    peak_all, whole = peak_of(all_kept)
    assert torch.equal(torch.cat(parts), whole[0])
    one = 3 * 8 * 64 * 64 * 2
    print(f"peak while streaming {peak_iter} B, with every reconstruction kept {peak_all} B (one reconstruction {one} B)")
    assert peak_iter < peak_all
