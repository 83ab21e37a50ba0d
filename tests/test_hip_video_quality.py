"""Per-frame quality of whole videos on the MI355X: `ttv_video_frame_sse_*` and `ttv_video_frame_ssim_*` (csrc/ttv_video_quality.hip)
through the C ABI against the numpy restatement of tests/quality_ref.py - the sums integer for integer, SSIM within the 5e-5 that
tests/test_hip_ssim.py holds the same fp32 filter arithmetic to (C1 and C2 scale with the square of the range, so the bound carries
over to levels 0 .. 255) - and `video.VideoTokenizer.quality` end to end.  `-m gpu`.

Every output lies in a buffer filled with a canary and longer than the output on both sides; a refused call writes nothing."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quality_ref as QR  # noqa: E402
from test_hip_video import K, SEQ, random_frames, tiny_model  # noqa: E402
from test_hip_video_yuv import Surface, random_planes  # noqa: E402

from titok_video_amd import _lib  # noqa: E402
from titok_video_amd import video as V  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 16
CANARY_I = 0x5A5A5A5A5A5A5A5A
CANARY_F = -777.25
SSIM_TOL = 5e-5
COLOUR = ("bt601", "full", "center")


def S():
    return _lib.stream_ptr(torch.device(DEV))


def shifted(t: torch.Tensor, shift: int) -> torch.Tensor:
    """The same bytes on the GPU, `shift` bytes off the allocation's (256-byte) grid: the first and the last words of the array are
    then out of bounds for a 4-byte load."""
    buf = torch.zeros(t.numel() + shift, dtype=torch.uint8, device=DEV)
    buf[shift:] = t.reshape(-1).to(DEV)
    view = buf[shift:].view(t.shape)
    assert view.data_ptr() % 4 == shift % 4
    return view


class Out:
    """n x 3 results inside a canary-filled buffer."""

    def __init__(self, n, dtype, prefill=None):
        self.n, self.canary = n, CANARY_I if dtype is torch.int64 else CANARY_F
        self.buf = torch.full((3 * n + 2 * GUARD,), self.canary, dtype=dtype, device=DEV)
        if prefill is not None:
            self.buf[GUARD:GUARD + 3 * n] = prefill
        self.ptr = self.buf.data_ptr() + GUARD * 8

    def read(self, rc):
        torch.cuda.synchronize()
        h = self.buf.cpu()
        if rc != 0:
            assert bool((h == self.canary).all()), "a refused call wrote something"
            return None
        assert bool((h[:GUARD] == self.canary).all()) and bool((h[GUARD + 3 * self.n:] == self.canary).all()), "written outside the output"
        return h[GUARD:GUARD + 3 * self.n].view(self.n, 3)


def raw_sse_rgb(a, b, n, stride, H, W, out=None):
    out = Out(n, torch.int64) if out is None else out
    rc = _lib.lib().ttv_video_frame_sse_u8(a.data_ptr(), b.data_ptr(), n, stride, H, W, out.ptr, S())
    got = out.read(rc)
    return rc, None if got is None else got.tolist()


def raw_sse_yuv(da, db, n, stride, H, W, out=None):
    out = Out(n, torch.int64) if out is None else out
    rc = _lib.lib().ttv_video_frame_sse_yuv420(C.byref(da), C.byref(db), n, stride, H, W, out.ptr, S())
    got = out.read(rc)
    return rc, None if got is None else got.tolist()


def raw_ssim(kind, a, b, n, stride, H, W, work_bytes=None):
    """(rc, float64 [n,3] numpy); `a`, `b` device tensors (kind 'rgb') or Yuv420 descriptions (kind 'yuv')."""
    h = _lib.lib()
    need = h.ttv_video_frame_ssim_workspace_bytes(n, H, W, int(kind == "yuv"))
    work = torch.full((max(need, 8) // 8 + 2 * GUARD,), CANARY_F, dtype=torch.float64, device=DEV)
    out = Out(n, torch.float64)
    wptr, nbytes = work.data_ptr() + GUARD * 8, (max(need, 0) if work_bytes is None else work_bytes)
    if kind == "rgb":
        rc = h.ttv_video_frame_ssim_u8(a.data_ptr(), b.data_ptr(), n, stride, H, W, out.ptr, wptr, nbytes, S())
    else:
        rc = h.ttv_video_frame_ssim_yuv420(C.byref(a), C.byref(b), n, stride, H, W, out.ptr, wptr, nbytes, S())
    got = out.read(rc)
    w = work.cpu()
    used = 0 if rc != 0 else max(need, 0) // 8
    assert bool((w[:GUARD] == CANARY_F).all()) and bool((w[GUARD + used:] == CANARY_F).all()), "written outside the workspace"
    return rc, None if got is None else got.numpy().copy()


# ---- squared error, RGB -------------------------------------------------------------------------------------------------------------
#            H,  W, n, b_stride, shift of a, shift of b
SSE_RGB = [(37, 45, 3, 1, 0, 0), (37, 45, 3, 2, 1, 3), (37, 45, 1, 3, 3, 1), (1, 45, 3, 3, 1, 0), (37, 1, 3, 2, 0, 3), (1, 1, 1, 1, 3, 3),
           (40, 64, 3, 1, 0, 0), (53, 200, 1, 1, 1, 1), (53, 200, 2, 2, 3, 2), (53, 200, 2, 1, 0, 0)]


@pytest.mark.parametrize("case", SSE_RGB, ids=lambda c: "x".join(map(str, c)))
def test_sse_rgb_is_exact(case):
    H, W, n, stride, sa, sb = case
    if H == 53:
        assert 3 * H * W > 12 * 256 * 4 * 2                      # more than two blocks a frame
    a = random_frames((n, H, W), seed=H + W + n)
    b = random_frames(((n - 1) * stride + 1, H, W), seed=H * W + stride)
    want = QR.sse_rgb(a.numpy(), b.numpy(), stride)
    da, db = shifted(a, sa), shifted(b, sb)
    rc, got = raw_sse_rgb(da, db, n, stride, H, W)
    assert rc == 0 and got == want
    if sa == sb == 0:
        assert V.frame_sse(da, db, stride).tolist() == want


def test_sse_beyond_32_bits_and_of_identical_frames():
    a = torch.zeros((2, 264, 256, 3), dtype=torch.uint8, device=DEV)
    b = torch.full((2, 264, 256, 3), 255, dtype=torch.uint8, device=DEV)
    b[1] = 0
    big = 67584 * 65025
    assert big > 1 << 32
    rc, got = raw_sse_rgb(a, b, 2, 1, 264, 256)
    assert rc == 0 and got == [[big] * 3, [0] * 3]
    f = random_frames((2, 37, 45), seed=4).to(DEV)
    assert raw_sse_rgb(f, f.clone(), 2, 1, 37, 45) == (0, [[0] * 3] * 2)


def test_sse_is_written_not_accumulated():
    a, b = random_frames((2, 20, 24), seed=1), random_frames((2, 20, 24), seed=2)
    want = QR.sse_rgb(a.numpy(), b.numpy())
    out = Out(2, torch.int64, prefill=12345)
    da, db = a.to(DEV), b.to(DEV)
    assert raw_sse_rgb(da, db, 2, 1, 20, 24, out) == (0, want)
    assert raw_sse_rgb(da, db, 2, 1, 20, 24, out) == (0, want)                    # a second call into the same buffer
    y, u, v = random_planes(2, 20, 24, 3)
    sa, sb = Surface(y, u, v, "i420"), Surface(*random_planes(2, 20, 24, 4), "nv12")
    want = QR.sse_planes((y, u, v), random_planes(2, 20, 24, 4))
    for _ in range(2):
        assert raw_sse_yuv(sa.desc(*COLOUR), sb.desc(*COLOUR), 2, 1, 20, 24, out) == (0, want)


# ---- squared error, 4:2:0 --------------------------------------------------------------------------------------------------------------
#            H,  W, n, b_stride, layout a, layout b, (y_pad, c_pad, lead) of a, of b
SSE_YUV = [(37, 45, 3, 1, "i420", "nv12", (0, 0, 0), (0, 0, 0)), (37, 45, 2, 2, "nv21", "i420", (0, 0, 0), (0, 0, 0)),
           (37, 45, 3, 1, "i420", "nv12", (3, 5, 1), (6, 1, 3)), (37, 45, 2, 3, "nv21", "i420", (1, 2, 2), (5, 3, 1)),
           (37, 45, 2, 1, "nv12", "nv21", (2, 3, 3), (0, 0, 1)), (1, 1, 2, 1, "i420", "nv12", (0, 0, 0), (3, 1, 1)),
           # more than one block per plane and frame, in luma and in chroma, and every pair of sample steps
           (140, 300, 1, 1, "nv12", "nv12", (4, 4, 0), (0, 2, 2)), (140, 300, 2, 2, "i420", "nv21", (1, 3, 3), (0, 0, 0)),
           (140, 300, 1, 1, "nv12", "i420", (0, 0, 1), (2, 1, 0)), (140, 300, 1, 1, "i420", "i420", (0, 0, 0), (3, 3, 3))]


@pytest.mark.parametrize("case", SSE_YUV, ids=lambda c: "-".join(map(str, c[:6])) + ("-pitched" if any(c[6] + c[7]) else ""))
def test_sse_yuv_is_exact(case):
    H, W, n, stride, la, lb, (ypa, cpa, leada), (ypb, cpb, leadb) = case
    if H == 140:
        assert (H // 2) * ((W // 2 + 7) // 8) > 256 * 4          # more than one chroma block a frame
    pa, pb = random_planes(n, H, W, seed=H + n), random_planes((n - 1) * stride + 1, H, W, seed=W + stride)
    want = QR.sse_planes(pa, pb, stride)
    for fill_a, fill_b in ((0, 255), (255, 0)):                 # what is no sample differs as much as it can and must not count
        sa, sb = Surface(*pa, la, ypa, cpa, leada, fill_a), Surface(*pb, lb, ypb, cpb, leadb, fill_b)
        rc, got = raw_sse_yuv(sa.desc(*COLOUR), sb.desc(*COLOUR), n, stride, H, W)
        assert rc == 0 and got == want, (fill_a, fill_b)
    assert V.frame_sse(sa.frames(*COLOUR), sb.frames(*COLOUR), stride).tolist() == want


def test_interleaved_bytes_of_the_other_component_do_not_count():
    """U and V of both sides equal except in V: the U sums are 0 although every second byte of the interleaved rows differs."""
    y, u, v = random_planes(2, 37, 45, seed=8)
    v2 = (255 - v).astype(np.uint8)
    for la, lb in (("nv12", "nv12"), ("nv12", "i420"), ("i420", "nv21")):
        sa, sb = Surface(y, u, v, la), Surface(y, u, v2, lb)       # named: a description does not keep its buffers alive
        rc, got = raw_sse_yuv(sa.desc(*COLOUR), sb.desc(*COLOUR), 2, 1, 37, 45)
        assert rc == 0 and got == QR.sse_planes((y, u, v), (y, u, v2)) and all(row[0] == 0 and row[1] == 0 and row[2] > 0 for row in got)


def test_sse_refuses_bad_arguments():
    f = random_frames((3, 20, 24), seed=1).to(DEV)
    assert raw_sse_rgb(f, f, 0, 1, 20, 24)[0] == 0                                  # nothing to do is no error
    assert raw_sse_rgb(f, f, -1, 1, 20, 24)[0] == 1 and raw_sse_rgb(f, f, 2, 0, 20, 24)[0] == 1 and raw_sse_rgb(f, f, 2, 1, 0, 24)[0] == 1
    out = Out(2, torch.int64)
    out.ptr += 4
    assert raw_sse_rgb(f, f, 2, 1, 20, 24, out)[0] == 1
    s = Surface(*random_planes(3, 20, 24, 1), "nv12", 2, 2)
    good = s.desc(*COLOUR)
    assert raw_sse_yuv(good, good, 3, 1, 20, 24)[0] == 0
    for bad in (dict(c_step=3), dict(y_pitch=23), dict(c_pitch=23), dict(y_frame=20 * 26 - 3), dict(c_frame=9 * 26 + 22), dict(u=None)):
        assert raw_sse_yuv(s.desc(*COLOUR, **bad), good, 3, 1, 20, 24)[0] == 1, bad
        assert raw_sse_yuv(good, s.desc(*COLOUR, **bad), 3, 1, 20, 24)[0] == 1, bad
    with pytest.raises(ValueError):
        V.frame_sse(s.frames(*COLOUR), s.frames("bt709", "full", "center"))
    with pytest.raises(ValueError):
        V.frame_sse(f, s.frames(*COLOUR))
    with pytest.raises(ValueError):
        V.frame_sse(f, f[:2], 2)


# ---- SSIM ------------------------------------------------------------------------------------------------------------------------------
def pattern(kind, shape, seed):
    """Planes [n,h,w] of a kind, and a second set to compare them with: independent noise; a smooth ramp and the same ramp a little
    brighter and steeper; the ramp under noise against the clean ramp."""
    r = np.random.default_rng(seed)
    n, h, w = shape
    ramp = (np.arange(h)[:, None] * 2.0 + np.arange(w)[None, :] * 3.0)[None] + 10.0 * np.arange(n)[:, None, None]
    if kind == "random":
        a, b = r.integers(0, 256, shape), r.integers(0, 256, shape)
    elif kind == "ramp":
        a, b = ramp, ramp * 1.07 + 3
    else:
        a, b = ramp + r.normal(0, 12, shape), ramp
    return tuple(np.clip(np.rint(p), 0, 255).astype(np.uint8) for p in (a, b))


KINDS = ("random", "ramp", "ramp+noise")
WORST = {}


def report(what, got, want):
    d = float(np.abs(got - want).max())
    WORST[what] = d
    print(f"ssim {what}: largest |kernel - float64 restatement| = {d:.3e} (bound {SSIM_TOL:g}); largest so far {max(WORST.values()):.3e}")
    return d


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", [(11, 11), (12, 43), (43, 44), (75, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_ssim_rgb_is_within_the_bound(size, kind):
    H, W = size
    n, stride = 2, 2
    pa = [pattern(kind, (n, H, W), seed=c + H) for c in range(3)]
    a = np.stack([p[0] for p in pa], axis=-1)
    b3 = np.stack([p[1] for p in pa], axis=-1)
    b = np.stack([b3[0], 255 - b3[0], b3[1]])                   # frame 1 of a meets frame 2 of b
    want = QR.ssim_rgb(a, b, stride)
    da, db = shifted(torch.from_numpy(a), 1), shifted(torch.from_numpy(b), 2)
    rc, got = raw_ssim("rgb", da, db, n, stride, H, W)
    assert rc == 0 and report(f"rgb {H}x{W} {kind}", got, want) < SSIM_TOL
    rc, again = raw_ssim("rgb", da, db, n, stride, H, W)
    assert rc == 0 and (got.view(np.uint64) == again.view(np.uint64)).all(), "two calls differ in bits"
    assert (V.frame_ssim(da, db, stride).cpu().numpy().view(np.uint64) == got.view(np.uint64)).all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", [(21, 22, "i420", "nv21", (0, 0, 0)), (45, 87, "nv12", "nv12", (3, 5, 1)), (45, 87, "i420", "nv12", (1, 2, 3))],
                         ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}-{c[3]}" + ("-pitched" if any(c[4]) else ""))
def test_ssim_yuv_is_within_the_bound(case, kind):
    H, W, la, lb, (yp, cp, lead) = case
    n, stride, Hc, Wc = 2, 1, (H + 1) // 2, (W + 1) // 2
    py, pu, pv = pattern(kind, (n, H, W), 1), pattern(kind, (n, Hc, Wc), 2), pattern(kind, (n, Hc, Wc), 3)
    pa, pb = (py[0], pu[0], pv[0]), (py[1], pu[1], pv[1])
    want = QR.ssim_planes(pa, pb, stride)
    sa, sb = Surface(*pa, la, yp, cp, lead, 0), Surface(*pb, lb, yp, cp, lead, 255)
    rc, got = raw_ssim("yuv", sa.desc(*COLOUR), sb.desc(*COLOUR), n, stride, H, W)
    assert rc == 0 and report(f"4:2:0 {H}x{W} {la}/{lb} {kind}", got, want) < SSIM_TOL
    rc, again = raw_ssim("yuv", sa.desc(*COLOUR), sb.desc(*COLOUR), n, stride, H, W)
    assert rc == 0 and (got.view(np.uint64) == again.view(np.uint64)).all(), "two calls differ in bits"
    assert (V.frame_ssim(sa.frames(*COLOUR), sb.frames(*COLOUR), stride).cpu().numpy().view(np.uint64) == got.view(np.uint64)).all()


def test_ssim_of_identical_and_of_constant_planes():
    f = random_frames((2, 43, 44), seed=6).to(DEV)
    rc, got = raw_ssim("rgb", f, f.clone(), 2, 1, 43, 44)
    assert rc == 0 and np.abs(got - 1).max() < 1e-6
    for la, lb in ((0, 255), (255, 255), (17, 200), (128, 127)):
        a = torch.full((1, 43, 44, 3), la, dtype=torch.uint8, device=DEV)
        b = torch.full((1, 43, 44, 3), lb, dtype=torch.uint8, device=DEV)
        rc, got = raw_ssim("rgb", a, b, 1, 1, 43, 44)
        assert rc == 0 and np.abs(got - (2 * la * lb + QR.C1) / (la * la + lb * lb + QR.C1)).max() < 1e-6, (la, lb, got)
    levels = ((90, 30), (30, 90), (250, 30))                     # (a, b) of Y, U, V
    shapes = ((1, 45, 87), (1, 23, 44), (1, 23, 44))
    pa, pb = ([np.full(s, lv[k], np.uint8) for s, lv in zip(shapes, levels)] for k in (0, 1))
    sa, sb = Surface(*pa, "nv12", 3, 5, 1, 7), Surface(*pb, "i420")
    rc, got = raw_ssim("yuv", sa.desc(*COLOUR), sb.desc(*COLOUR), 1, 1, 45, 87)
    want = [(2 * p * q + QR.C1) / (p * p + q * q + QR.C1) for p, q in levels]
    assert rc == 0 and np.abs(got[0] - np.array(want)).max() < 1e-6


def test_ssim_refuses_planes_without_a_whole_window():
    f = random_frames((1, 10, 32), seed=1).to(DEV)
    assert raw_ssim("rgb", f, f, 1, 1, 10, 32)[0] == 1 and b"at least 11" in _lib.lib().ttv_error_string()
    g = random_frames((1, 32, 10), seed=1).to(DEV)
    assert raw_ssim("rgb", g, g, 1, 1, 32, 10)[0] == 1
    s = Surface(*random_planes(1, 20, 32, 1), "nv12")
    assert raw_ssim("yuv", s.desc(*COLOUR), s.desc(*COLOUR), 1, 1, 20, 32)[0] == 1 and b"at least 21" in _lib.lib().ttv_error_string()
    ok = random_frames((1, 24, 32), seed=1).to(DEV)
    assert raw_ssim("rgb", ok, ok, 1, 1, 24, 32, work_bytes=16)[0] == 1 and b"workspace" in _lib.lib().ttv_error_string()
    assert raw_ssim("rgb", ok, ok, 1, 1, 24, 32)[0] == 0 and raw_ssim("rgb", ok, ok, 0, 1, 24, 32)[0] == 0
    with pytest.raises(ValueError):
        V.frame_ssim(f, f)


# ---- two independent kernels -------------------------------------------------------------------------------------------------------------
def test_frame_sums_equal_tile_sums_when_one_tile_covers_a_pixel():
    """Without overlap the blend's level of a pixel is tile_sse's level of the one element that covers it, so the two kernels - one
    summing tiles of float reconstructions, one summing frames of bytes - add up the same integers."""
    model = tiny_model()
    video, tile = (16, 64, 64), (8, 32, 32)
    frames = random_frames(video, seed=31).to(DEV)
    vt = V.VideoTokenizer(model, tile=tile, overlap=(0, 0, 0), tokens_per_tile=K, seq_len=SEQ, dtype=torch.bfloat16, depth=1)
    tok = vt.encode_video(frames)
    plan = tok.plan()
    assert plan.n_tiles == 8 and plan.tile == tile
    per_frame = V.frame_sse(vt.decode_video(tok), frames)
    with torch.no_grad():
        recon = []
        for layer in range(2):
            recon += model.decode_indices(tok.indices[layer * 4 * K:(layer + 1) * 4 * K].to(DEV), [tile] * 4, [K] * 4)
    per_tile = V.tile_sse(frames, plan, recon)
    total = int(per_frame.sum())
    assert total == int(per_tile.sum()) and total > 0
    # tile by tile as well: a tile's sum is the sum of its frames' pixels, which the restatement counts on the decoded bytes
    out, src = vt.decode_video(tok).cpu().numpy().astype(np.int64), frames.cpu().numpy().astype(np.int64)
    for j in range(8):
        t0, h0, w0 = plan.tile_origin(j)
        d = out[t0:t0 + 8, h0:h0 + 32, w0:w0 + 32] - src[t0:t0 + 8, h0:h0 + 32, w0:w0 + 32]
        assert int((d * d).sum()) == int(per_tile[j])


# ---- VideoTokenizer.quality ----------------------------------------------------------------------------------------------------------------
VIDEO, TILE, OVERLAP = (20, 40, 56), (8, 32, 32), (4, 8, 8)


@pytest.fixture(scope="module")
def tokenizer():
    return V.VideoTokenizer(tiny_model(), tile=TILE, overlap=OVERLAP, tokens_per_tile=K, seq_len=SEQ, dtype=torch.bfloat16, depth=2)


@pytest.mark.parametrize("stride", [1, 2])
def test_quality_of_an_rgb_round_trip(tokenizer, stride):
    frames = random_frames(VIDEO, seed=77)
    dev = frames.to(DEV)
    tok = tokenizer.encode_video(dev, frame_stride=stride)
    q = tokenizer.quality(dev, tok)
    out = tokenizer.decode_video(tok)
    n = -(-VIDEO[0] // stride)
    assert q.components == ("r", "g", "b") and q.elements == (40 * 56,) * 3 and q.t0 == 0 and len(q.sse) == n
    assert q.sse == QR.sse_rgb(out.cpu().numpy(), frames.numpy()[::stride])
    assert q.ssim == V.frame_ssim(out, dev, stride).cpu().tolist()                   # the same tensors in one call: bit for bit
    assert np.abs(np.array(q.ssim) - QR.ssim_rgb(out.cpu().numpy(), frames.numpy()[::stride])).max() < SSIM_TOL
    assert all(isinstance(v, int) for row in q.sse for v in row) and all(isinstance(v, float) for row in q.ssim for v in row)
    assert q.psnr()[0][0] == 10 * math.log10(65025 * 40 * 56 / q.sse[0][0]) and q.worst_frame() in range(n)
    none = tokenizer.quality(dev, tok, ssim=False)
    assert none.sse == q.sse and none.ssim is None and none.as_dict()["ssim_mean"] is None
    with pytest.raises(ValueError):
        tokenizer.quality(dev[:, :, :48].contiguous(), tok)
    with pytest.raises(ValueError):
        tokenizer.quality(dev[1:], tok)


@pytest.mark.parametrize("stride", [1, 2])
def test_quality_of_a_420_round_trip(tokenizer, stride):
    planes = random_planes(*VIDEO, seed=9)
    frames = Surface(*planes, "nv12", 3, 5, 1).frames(*COLOUR)
    tok = tokenizer.encode_video(frames, frame_stride=stride)
    q = tokenizer.quality(frames, tok)
    n = -(-VIDEO[0] // stride)
    out = tokenizer.decode_video(tok, output=frames.like(n))
    assert (out.layout, out.matrix, out.range, out.siting) == ("nv12",) + COLOUR
    assert q.components == ("y", "u", "v") and q.elements == (40 * 56, 20 * 28, 20 * 28) and len(q.sse) == n
    got = tuple(p.cpu().numpy() for p in (out.y, out.u, out.v))
    assert q.sse == QR.sse_planes(got, tuple(p[::stride] for p in planes))
    assert q.ssim == V.frame_ssim(out, frames, stride).cpu().tolist()
    assert np.abs(np.array(q.ssim) - QR.ssim_planes(got, tuple(p[::stride] for p in planes))).max() < SSIM_TOL
    with pytest.raises(ValueError):
        tokenizer.quality(random_frames(VIDEO, seed=1).to(DEV)[:, :39].contiguous(), tok)


# ---- memory ----------------------------------------------------------------------------------------------------------------------------
def test_quality_holds_a_few_layers_not_the_video():
    """The pattern of test_iter_holds_a_few_layers_not_the_video: a long, thin video (tile 8, overlap 4: 19 temporal layers at 80
    frames), the source resident before the peak is counted.  `quality` keeps per range two results of n x 3 numbers, which the
    allocator rounds up to 512 bytes each; nothing else may grow with the length."""
    model = tiny_model()
    vt = V.VideoTokenizer(model, tile=(8, 64, 64), overlap=(4, 0, 0), tokens_per_tile=K, seq_len=6144, dtype=torch.bfloat16, depth=1)

    def peak_of(run):
        import gc
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        kept = run()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, kept

    peaks = {}
    for T in (80, 160):
        frames = random_frames((T, 64, 64), seed=5).to(DEV)
        tok = vt.encode_video(frames)
        assert tok.plan().counts == (T // 4 - 1, 1, 1)
        warm = vt.quality(frames, tok)                           # plans, workspaces and packed weights exist from here on
        peaks[T], q = peak_of(lambda: vt.quality(frames, tok))
        assert q.sse == warm.sse and q.ssim == warm.ssim and len(q.sse) == T
        if T == 80:
            peak_decode, out = peak_of(lambda: vt.decode_video(tok))
            assert q.sse == QR.sse_rgb(out.cpu().numpy(), frames.cpu().numpy())
            del out
        del frames, tok, warm, q
    print(f"peak during quality(): {peaks[80]} B at 80 frames, {peaks[160]} B at 160; during decode_video at 80 frames {peak_decode} B "
          f"(the video is {80 * 64 * 64 * 3} B)")
    assert peaks[80] < peak_decode
    more_ranges = (160 - 80) // 4
    assert peaks[160] <= peaks[80] + more_ranges * 2 * 512
