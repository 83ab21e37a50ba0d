"""Per-tile token counts from measured distortion on the MI355X: `ttv_video_tile_sse_u8` (csrc/ttv_video.hip) through the C ABI, every
sum equal as an integer to the numpy restatement of tests/rate_ref.py, and `VideoTokenizer.rate_distortion` / `encode_video` with a
target or a budget against the same steps done by hand around the public model call.  `-m gpu`.

The sums lie in a buffer filled with a canary and longer than the output on both sides."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rate_ref as RR  # noqa: E402
import video_ref as VR  # noqa: E402

from tests import test_hip_video as HV  # noqa: E402  (its geometries, seeded frames and tiny model)
from titok_video_amd import _lib  # noqa: E402
from titok_video_amd import video as V  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = HV.DEV
DTYPES = HV.DTYPES
CANARY, GUARD = 0x5A5A5A5A5A5A5A5A, 8
PLANTED = (float("nan"), float("inf"), float("-inf"), 1.0, -1.0, 1.3, -1.3, 0.0)


def raw_sse(frames_dev, plan, begin, end, tiles, dt, cplan=None, dtype_code=None, null=(), ptrs=None, sse_shift=0, buf=None):
    """The C entry point on device tiles into a canary-filled buffer of sums with GUARD of them on either side.
    Returns (rc, sums as a list of Python ints, the buffer)."""
    n = max(end - begin, 0)
    if buf is None:
        buf = torch.full((n + 2 * GUARD,), CANARY, dtype=torch.int64, device=DEV)
    before = buf.cpu().numpy().copy()
    ptrs = [t.data_ptr() for t in tiles] if ptrs is None else ptrs
    host = (C.c_void_p * max(len(ptrs), 1))(*ptrs)
    table = torch.tensor(ptrs if ptrs else [0], dtype=torch.int64).to(DEV)
    cp = plan.c_plan() if cplan is None else cplan
    rc = _lib.lib().ttv_video_tile_sse_u8(None if "frames" in null else frames_dev.data_ptr(), C.byref(cp), begin, end,
                                          None if "host" in null else host, None if "dev" in null else table.data_ptr(),
                                          _lib.dtype_code(DTYPES[dt]) if dtype_code is None else dtype_code,
                                          None if "sse" in null else buf.data_ptr() + 8 * GUARD + sse_shift, HV.S())
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    if rc != 0:
        assert (h == before).all(), "a refused call wrote something"
        return rc, None, buf
    assert (h[:GUARD] == before[:GUARD]).all() and (h[GUARD + n:] == before[GUARD + n:]).all(), "sums outside the range were written"
    return rc, [int(v) for v in h[GUARD:GUARD + n]], buf


def seeded_recon(plan, ref, begin, end, dt, seed, shift=0):
    """Per tile of the range U(-1.3, 1.3) with PLANTED at the start of the first row (inside the video on every geometry here) and
    again at scattered places; device tensors, one allocation each, `shift` elements off their allocation's start.
    Returns (device tensors, float32 numpy of the values they hold)."""
    g = torch.Generator().manual_seed(seed)
    dev, host = [], []
    for k in range(begin, end):
        x = torch.rand((3,) + plan.tile, generator=g) * 2.6 - 1.3
        assert RR.counted(ref, k)[2] >= len(PLANTED)
        f = x.view(-1)
        for j, v in enumerate(PLANTED):
            x[k % 3, 0, 0, j] = v
            f[(j * 211 + 31 * k + 17) % f.numel()] = v
        store = torch.empty(x.numel() + shift, dtype=DTYPES[dt], device=DEV)
        store[shift:] = x.view(-1).to(DTYPES[dt])
        t = store[shift:].view(x.shape)
        dev.append(t)
        host.append(t.float().cpu().numpy())
    return dev, host


def want_sums(frames, ref, begin, end, host_tiles):
    return [RR.tile_sse(frames.numpy(), ref, k, host_tiles[k - begin]) for k in range(begin, end)]


# ---- the kernel -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("case", list(HV.GATHER))
def test_tile_sse_is_exact(case, dt):
    video, tile, overlap, patch, stride, rng = HV.GATHER[case]
    plan, ref = HV.both(video, tile, overlap, patch, stride)
    begin, end = rng if rng else (0, plan.n_tiles)
    frames = HV.random_frames(video, seed=sum(video))
    tiles, host = seeded_recon(plan, ref, begin, end, dt, seed=len(case))
    want = want_sums(frames, ref, begin, end, host)
    assert min(want) > 0 and [plan.tile_elements(k) for k in range(begin, end)] == [RR.elements(ref, k) for k in range(begin, end)]
    rc, got, _ = raw_sse(frames.to(DEV), plan, begin, end, tiles, dt)
    assert rc == 0, _lib.lib().ttv_error_string()
    assert got == want, f"{case} {dt}"
    # the same frames one byte off the word grid: the first and the last words of the array are out of bounds for a 4-byte load
    shifted = torch.zeros(frames.numel() + 1, dtype=torch.uint8, device=DEV)
    shifted[1:] = frames.view(-1).to(DEV)
    view = shifted[1:].view(frames.shape)
    assert view.data_ptr() % 4 == 1
    rc, got, _ = raw_sse(view, plan, begin, end, tiles, dt)
    assert rc == 0 and got == want, f"{case} {dt}, frames one byte off the word grid"
    assert V.tile_sse(view, plan, tiles, begin, end).tolist() == want, f"tile_sse, {case} {dt}"
    # tiles one element off the 16-byte grid: aligned to their element size only, so no vector load may touch them
    tiles1, host1 = seeded_recon(plan, ref, begin, end, dt, seed=len(case), shift=1)
    assert all(t.data_ptr() % 16 for t in tiles1) and all((a.view(np.uint32) == b.view(np.uint32)).all() for a, b in zip(host, host1))
    rc, got, _ = raw_sse(frames.to(DEV), plan, begin, end, tiles1, dt)
    assert rc == 0 and got == want, f"{case} {dt}, tiles one element off the vector grid"


@pytest.mark.parametrize("dt", list(DTYPES))
def test_identities(dt):
    """gather_tiles' own output costs nothing; a pre-filled sum is overwritten; three runs give the same bits."""
    plan, ref = HV.both((20, 40, 56), (8, 32, 32), (4, 8, 8), (4, 8, 8), 3)                  # T' = 7: one padded layer
    frames = HV.random_frames((20, 40, 56), seed=8).to(DEV)
    cut = list(V.gather_tiles(frames, plan, dtype=DTYPES[dt]).unbind(0))
    rc, got, _ = raw_sse(frames, plan, 0, plan.n_tiles, cut, dt)
    assert rc == 0 and got == [0] * plan.n_tiles
    assert V.tile_sse(frames, plan, cut).tolist() == [0] * plan.n_tiles
    tiles, host = seeded_recon(plan, ref, 0, plan.n_tiles, dt, seed=4)
    want = want_sums(frames.cpu(), ref, 0, plan.n_tiles, host)
    rc, first, buf = raw_sse(frames, plan, 0, plan.n_tiles, tiles, dt)
    assert rc == 0 and first == want and min(want) > 0
    for _ in range(2):                                       # on the sums of the last run: written, not accumulated
        rc, again, buf = raw_sse(frames, plan, 0, plan.n_tiles, tiles, dt, buf=buf)
        assert rc == 0 and again == first


@pytest.mark.parametrize("dt", list(DTYPES))
def test_a_sum_beyond_32_bits(dt):
    plan, _ = HV.both((8, 64, 64), (8, 64, 64), (0, 0, 0), (4, 8, 8))
    assert plan.n_tiles == 1
    frames = torch.full((8, 64, 64, 3), 255, dtype=torch.uint8, device=DEV)
    recon = torch.full((3, 8, 64, 64), -1.0, dtype=DTYPES[dt], device=DEV)
    rc, got, _ = raw_sse(frames, plan, 0, 1, [recon], dt)
    assert rc == 0 and got == [98304 * 65025] and got[0] == 6392217600 > 2 ** 32


@pytest.mark.parametrize("dt", list(DTYPES))
def test_every_bf16_pattern_has_its_level(dt):
    """One tile of (8, 64, 64) holds every bf16 bit pattern (as bf16, and widened in fp32): every NaN, quiet or signalling, is level
    0, the infinities are 0 and 255, and everything beyond +-1 is clamped."""
    plan, ref = HV.both((8, 64, 64), (8, 64, 64), (0, 0, 0), (4, 8, 8))
    bits = (np.arange(3 * 8 * 64 * 64) % 65536).astype(np.uint16)
    host = (bits.astype(np.uint32) << 16).view(np.float32).reshape(3, 8, 64, 64)
    assert np.isnan(host).sum() > 250 and np.isinf(host).sum() >= 2
    if dt == "bf16":
        recon = torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16).view(3, 8, 64, 64).to(DEV)
    else:
        recon = torch.from_numpy(host.copy()).to(DEV)
    frames = HV.random_frames((8, 64, 64), seed=12)
    rc, got, _ = raw_sse(frames.to(DEV), plan, 0, 1, [recon], dt)
    assert rc == 0 and got == [RR.tile_sse(frames.numpy(), ref, 0, host)]


def test_tile_sse_refuses_bad_arguments():
    plan, ref = HV.both((11, 37, 45), (8, 16, 24), (4, 8, 8), (4, 8, 8))
    frames = HV.random_frames((11, 37, 45), seed=1).to(DEV)
    tiles, _ = seeded_recon(plan, ref, 0, plan.n_tiles, "bf16", seed=2)
    n = plan.n_tiles

    def call(begin=0, end=3, **kw):
        kw.setdefault("ptrs", [t.data_ptr() for t in tiles[begin:max(end, begin)]])
        return raw_sse(frames, plan, begin, end, None, "bf16", **kw)[0]
    assert call() == 0
    assert call(4, 4) == 0 and call(n, n) == 0                                      # an empty range is no error and no launch
    assert call(4, 4, null=("frames", "host", "dev", "sse")) == 0
    assert call(dtype_code=7) == 1
    for what in ("frames", "host", "dev", "sse"):
        assert call(null=(what,)) == 1, what
    for begin, end in ((-1, 2), (0, n + 1), (5, 4), (n + 1, n + 1)):
        assert call(begin, end, ptrs=[tiles[0].data_ptr()] * 3) == 1, (begin, end)
    good = [t.data_ptr() for t in tiles[:3]]
    assert call(ptrs=[good[0], 0, good[2]]) == 1 and b"NULL" in _lib.lib().ttv_error_string()
    assert call(ptrs=[good[0], good[1], good[2] + 1]) == 1 and b"aligned" in _lib.lib().ttv_error_string()
    assert call(sse_shift=4) == 1
    for field, value in (("count", (2, 5, 3)), ("overlap", (5, 8, 8)), ("overlap", (4, -1, 8)), ("tile", (8, 0, 24))):
        cp = plan.c_plan()
        setattr(cp, field, (_lib.i32 * 3)(*value))
        assert call(cplan=cp) == 1, (field, value)
    cp = plan.c_plan()
    cp.frame_stride = 0
    assert call(cplan=cp) == 1
    assert b"video_tile_sse_u8" in _lib.lib().ttv_error_string()
    f32 = [t.float() for t in tiles[:3]]
    assert raw_sse(frames, plan, 0, 3, f32, "f32", ptrs=[f32[0].data_ptr(), f32[1].data_ptr() + 2, f32[2].data_ptr()])[0] == 1
    with pytest.raises(ValueError):
        V.tile_sse(frames, plan, tiles[:2], 0, 3)
    with pytest.raises(ValueError):
        V.tile_sse(frames, plan, tiles[:2] + [tiles[2].float()], 0, 3)
    with pytest.raises(RuntimeError):
        V.tile_sse(frames.cpu(), plan, tiles[:3], 0, 3)


# ---- rate_distortion end to end ---------------------------------------------------------------------------------------------------------
VIDEO, TILE, OVERLAP, PATCH, SEQ, LADDER = HV.VIDEO, HV.TILE, HV.OVERLAP, HV.PATCH, HV.SEQ, (2, 4, 8)
BATCHES = ((0, 5), (5, 10), (10, 15), (15, 16))


def table_by_hand(model, frames):
    """The same probe around the public model call: restatement-cut tiles uploaded, coded at every count of the ladder in the batches
    the token budget gives (a tile is 32 patch rows: 5 tiles under 200 rows at 2, 4 and 8 tokens), the downloaded reconstructions
    measured by the restatement.  Returns (sse [16][3], elements [16], indices [16][3] as int32 tensors on the host)."""
    ref = VR.Plan(VIDEO, TILE, OVERLAP, PATCH)
    assert ref.n_tiles == 16 and ref.tile == TILE and all(5 * (32 + k) <= SEQ < 6 * (32 + k) for k in LADDER)
    cut = VR.gather(frames.numpy(), ref, 0, 16, "bf16")
    sse, idx = [[] for _ in range(16)], [[] for _ in range(16)]
    with torch.no_grad():
        for k in LADDER:
            for a, b in BATCHES:
                clips = [torch.from_numpy(cut[j]).to(torch.bfloat16).to(DEV) for j in range(a, b)]
                recon, info = model(clips, [k] * (b - a))
                parts = info["indices"].to(torch.int32).cpu().view(b - a, k)
                for j in range(a, b):
                    sse[j].append(RR.tile_sse(frames.numpy(), ref, j, recon[j - a].float().cpu().numpy()))
                    idx[j].append(parts[j - a])
    return sse, [RR.elements(ref, j) for j in range(16)], idx


@pytest.fixture(scope="module")
def fsq_probe():
    model = HV.tiny_model()
    frames = HV.random_frames(VIDEO, seed=77)
    return model, frames, table_by_hand(model, frames)


def check_table(table, by_hand):
    sse, elements, idx = by_hand
    assert table.ladder == LADDER and table.elements == elements == [3 * 8 * 32 * 32] * 16
    assert table.sse == sse and all(isinstance(v, int) for row in table.sse for v in row)
    for j in range(16):
        for l, k in enumerate(LADDER):
            got = table.indices[j][l]
            assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == (k,)
            assert torch.equal(got.cpu(), idx[j][l]), (j, k)
    assert len({v for row in sse for v in row}) > 16                # measurements, not a constant


@pytest.mark.parametrize("depth", [1, 2])
def test_rate_distortion_equals_the_steps_done_by_hand(fsq_probe, depth):
    model, frames, by_hand = fsq_probe
    vt = V.VideoTokenizer(model, tile=TILE, overlap=OVERLAP, tokens_per_tile=8, seq_len=SEQ, dtype=torch.bfloat16, depth=depth)
    check_table(vt.rate_distortion(frames.to(DEV), LADDER), by_hand)
    with pytest.raises(ValueError):
        vt.rate_distortion(frames.to(DEV), (4, 2))
    with pytest.raises(RuntimeError):
        vt.rate_distortion(frames, LADDER)


def test_rate_distortion_with_the_l2_quantiser():
    model = HV.tiny_model("l2")
    frames = HV.random_frames(VIDEO, seed=78)
    vt = V.VideoTokenizer(model, tile=TILE, overlap=OVERLAP, tokens_per_tile=8, seq_len=SEQ, dtype=torch.bfloat16, depth=2)
    table = vt.rate_distortion(frames.to(DEV), LADDER)
    check_table(table, table_by_hand(model, frames))
    assert max(int(i.max()) for row in table.indices for i in row) < 256


def ragged_choice(by_hand):
    """A target and a budget, read off the by-hand table, whose allocations are not uniform (else ragged batches go untested)."""
    sse, elements, _ = by_hand
    quality = sorted({RR.psnr(v, e) for row, e in zip(sse, elements) for v in row})
    targets = [(a + b) / 2 for a, b in zip(quality, quality[1:]) if b - a > 1e-3]
    target = next((t for t in targets if len(set(RR.allocate_target(LADDER, sse, elements, t))) > 1), None)
    budget = next((b for b in range(16 * LADDER[0] + 1, 16 * LADDER[-1]) if len(set(RR.allocate_budget(LADDER, sse, b))) > 1), None)
    assert target is not None and budget is not None, "the table offers no ragged allocation"
    return target, budget


@pytest.mark.parametrize("mode", ["target", "budget"])
def test_encode_video_with_a_target_and_with_a_budget(fsq_probe, mode, tmp_path):
    model, frames, by_hand = fsq_probe
    sse, elements, idx = by_hand
    target, budget = ragged_choice(by_hand)
    vt = V.VideoTokenizer(model, tile=TILE, overlap=OVERLAP, tokens_per_tile=8, seq_len=SEQ, dtype=torch.bfloat16, depth=2)
    if mode == "target":
        want = RR.allocate_target(LADDER, sse, elements, target)
        tok = vt.encode_video(frames.to(DEV), fps=24.0, ladder=LADDER, target_psnr=target)
    else:
        want = RR.allocate_budget(LADDER, sse, budget)
        tok = vt.encode_video(frames.to(DEV), fps=24.0, ladder=LADDER, total_tokens=budget)
        assert sum(tok.counts) <= budget
    assert len(set(want)) > 1, "the chosen counts are all equal: no ragged batch is exercised"
    assert tok.counts == want and tok.indices.dtype == torch.int32 and tok.fps == 24.0
    assert torch.equal(tok.indices.cpu(), torch.cat([idx[j][LADDER.index(k)] for j, k in enumerate(want)]))
    out = vt.decode_video(tok)
    assert out.dtype == torch.uint8 and tuple(out.shape) == VIDEO + (3,)
    tok.save(tmp_path / "v.ttvtok")
    back = V.VideoTokens.load(tmp_path / "v.ttvtok")
    assert back.counts == want and torch.equal(back.indices, tok.indices.cpu())
    header, _ = VR.parse_container((tmp_path / "v.ttvtok").read_bytes())
    assert header["counts"] == want
    assert torch.equal(vt.decode_video(back), out)


def test_encode_video_defaults_and_refusals(fsq_probe):
    model, frames, by_hand = fsq_probe
    dev_frames = frames.to(DEV)
    vt = V.VideoTokenizer(model, tile=TILE, overlap=OVERLAP, tokens_per_tile=8, seq_len=SEQ, dtype=torch.bfloat16, depth=2)
    # the default ladder of 8 tokens per tile is (1, 2, 4, 8): a budget of 16 leaves every tile at 1
    tok = vt.encode_video(dev_frames, total_tokens=16)
    assert tok.counts == [1] * 16 and tok.indices.numel() == 16
    # without the new arguments: the tokens of before, after the probe as well
    plain = vt.encode_video(dev_frames, fps=24.0)
    idx, _ = HV.by_hand(model, frames)
    assert plain.counts == [8] * 16 and torch.equal(plain.indices.cpu(), idx.to(torch.int32))
    for kw in (dict(target_psnr=30.0, total_tokens=64), dict(ladder=LADDER), dict(total_tokens=15), dict(ladder=(4, 2), total_tokens=64)):
        with pytest.raises(ValueError):
            vt.encode_video(dev_frames, **kw)
    ragged = V.VideoTokenizer(model, tile=TILE, overlap=OVERLAP, tokens_per_tile=[8] * 16, seq_len=SEQ, dtype=torch.bfloat16, depth=1)
    with pytest.raises(ValueError):
        ragged.encode_video(dev_frames, total_tokens=64)
    assert ragged.encode_video(dev_frames, ladder=LADDER, total_tokens=32).counts == [2] * 16
