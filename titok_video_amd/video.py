"""Whole videos in and out: overlapped 3-D tiles through the tokenizer, tokens back to uint8 frames.

    vt = VideoTokenizer(model, tile=(16, 128, 128), overlap=(4, 16, 16), tokens_per_tile=128, seq_len=6144,
                        dtype=torch.bfloat16, depth=2)
    tok = vt.encode_video(frames_u8, fps=24.0, frame_stride=3)      # frames_u8: uint8 [T,H,W,3] on the GPU -> VideoTokens
    out = vt.decode_video(tok)                                       # uint8 [T',H,W,3] on the GPU
    for t0, part in vt.decode_video_iter(tok): ...                   # frame ranges in timeline order, memory of a few tile layers
    tok.save(path); VideoTokens.load(path); tok.bits_per_pixel
    tok = vt.encode_video(frames_u8, fps=24.0, target_psnr=30.0)     # per-tile token counts from measured distortion: this quality ...
    tok = vt.encode_video(frames_u8, fps=24.0, total_tokens=4096)    # ... or this many tokens for the whole video
    table = vt.rate_distortion(frames_u8, (16, 32, 64, 128)); allocate_tokens(table, total_tokens=4096); table.psnr()

`TilePlan` is the geometry (pure Python, no GPU): where the tiles lie, their order and their blending weights.  The pixel work is
three HIP kernels (csrc/ttv_video.hip): `gather_tiles` cuts and normalises tiles (`ttv_video_tiles_u8`), `blend_tiles` turns
reconstructed tiles into frames (`ttv_video_blend_u8`), `tile_sse` measures reconstructed tiles against the source
(`ttv_video_tile_sse_u8`); include/titok_hip.h states all three element by element.  None has a CPU or eager path: host tensors raise.
The token container (`VideoTokens.to_bytes`) is host-side numpy and the allocator (`allocate_tokens`) plain Python on exact integers:
token streams and rate tables are tiny.

Decoders hand out Y'CbCr 4:2:0 and encoders take it: `YUV420Frames` wraps such planes (I420, NV12, NV21; pitched decoder surfaces as
views, no copy) and goes wherever the uint8 RGB frames go - `gather_tiles`, `tile_sse`, `encode_video`, `rate_distortion` - and
`blend_tiles(out=...)`, `decode_video(output=...)` and `decode_video_iter(output=...)` write planes instead of RGB
(`ttv_video_tiles_yuv420`, `ttv_video_blend_yuv420`, `ttv_video_tile_sse_yuv420`: the colour conversion is defined on integers in the
header and fused into the three kernels, there is no RGB frame in between).

What the frames that come back are worth: `vt.quality(frames, tok)` decodes range by range and measures every frame against the
source, per component (R, G, B or Y, U, V) - `VideoQuality` with per-frame `sse`, `psnr()`, `ssim` and their summaries.  The
measurements are `frame_sse` and `frame_ssim` on uint8 frames or `YUV420Frames` (csrc/ttv_video_quality.hip:
`ttv_video_frame_sse_u8 / _yuv420`, `ttv_video_frame_ssim_u8 / _yuv420`), GPU only like the rest.
"""
from __future__ import annotations

import ctypes as C
import json
import math
import struct
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

MAGIC = b"TTVTOK\r\n"
VERSION = 1
MAX_WEIGHT = 1 << 24          # tile weights are integers that fp32 holds exactly


def _triple(v, what) -> Tuple[int, int, int]:
    out = tuple(int(x) for x in v)
    if len(out) != 3:
        raise ValueError(f"{what} must have three entries (t, h, w), got {v!r}")
    return out


class TilePlan:
    """Tiles of a video (T, H, W) of nominal size `tile` overlapping by `overlap`, on the timeline of every `frame_stride`-th frame.

    Timeline: output frame j is source frame frame_stride * j, j < T' = ceil(T / frame_stride); `timeline` = (T', H, W).
    Per axis of length n: with n < tile there is one tile at 0 of ceil(n / patch) * patch samples (beyond n - 1 the edge repeats on the
    way in and is dropped on the way out); otherwise tiles of `tile` at k * (tile - overlap), the last one moved back to n - tile, so
    no padding is ever needed.  All tiles share the effective shape `tile`; index = (kt * n_h + kh) * n_w + kw.  A tile's weight at
    local coordinate u of an axis is min(u + 1, tile - u, overlap + 1); at an element the product over the axes."""

    def __init__(self, video, tile, overlap, patch, frame_stride: int = 1):
        self.video, self.nominal_tile = _triple(video, "video"), _triple(tile, "tile")
        self.overlap, self.patch, self.frame_stride = _triple(overlap, "overlap"), _triple(patch, "patch"), int(frame_stride)
        if min(self.video) < 1 or min(self.patch) < 1:
            raise ValueError(f"video {self.video} and patch {self.patch} must be at least 1 on every axis")
        if self.frame_stride < 1:
            raise ValueError(f"frame_stride must be at least 1, got {frame_stride}")
        for t, o, p in zip(self.nominal_tile, self.overlap, self.patch):
            if t < 1 or t % p:
                raise ValueError(f"tile {self.nominal_tile} must be a positive multiple of the patch {self.patch}")
            if o < 0 or 2 * o > t:
                raise ValueError(f"overlap {self.overlap} must lie in 0 .. tile / 2 of tile {self.nominal_tile}")
        if math.prod(o + 1 for o in self.overlap) >= MAX_WEIGHT:
            raise ValueError(f"overlap {self.overlap}: (ot + 1)(oh + 1)(ow + 1) must stay below 2^24")
        self.timeline = (-(-self.video[0] // self.frame_stride),) + self.video[1:]
        tiles, origins = [], []
        for n, t, o, p in zip(self.timeline, self.nominal_tile, self.overlap, self.patch):
            if n < t:
                tiles.append(-(-n // p) * p)
                origins.append([0])
            else:
                stride = t - o
                m = -(-(n - t) // stride) + 1
                tiles.append(t)
                origins.append([k * stride for k in range(m - 1)] + [n - t])
        self.tile: Tuple[int, int, int] = tuple(tiles)
        self.origins: Tuple[List[int], ...] = tuple(origins)
        self.counts: Tuple[int, int, int] = tuple(len(o) for o in origins)
        self.n_tiles = math.prod(self.counts)
        self.tiles_per_layer = self.counts[1] * self.counts[2]

    def tile_origin(self, index: int) -> Tuple[int, int, int]:
        if not 0 <= index < self.n_tiles:
            raise IndexError(f"tile {index} of {self.n_tiles}")
        kt, r = divmod(index, self.tiles_per_layer)
        kh, kw = divmod(r, self.counts[2])
        return self.origins[0][kt], self.origins[1][kh], self.origins[2][kw]

    def tile_elements(self, index: int) -> int:
        """Samples of tile `index` that lie inside the video, over the three channels: 3 * prod over the axes of
        min(tile, n - origin).  What a tile holds beyond a short axis is edge-clamped on the way in and counted nowhere."""
        return 3 * math.prod(min(t, n - o) for t, n, o in zip(self.tile, self.timeline, self.tile_origin(index)))

    def axis_weights(self, axis: int) -> List[int]:
        t, o = self.tile[axis], self.overlap[axis]
        return [min(u + 1, t - u, o + 1) for u in range(t)]

    @property
    def patches_per_tile(self) -> int:
        return math.prod(t // p for t, p in zip(self.tile, self.patch))

    def c_plan(self) -> "_lib.VideoPlan":
        i3 = _lib.i32 * 3
        return _lib.VideoPlan(T=self.video[0], H=self.video[1], W=self.video[2], frame_stride=self.frame_stride, tile=i3(*self.tile),
                              overlap=i3(*self.overlap), count=i3(*self.counts))

    def __repr__(self):
        return (f"TilePlan(video={self.video}, tile={self.nominal_tile}, overlap={self.overlap}, patch={self.patch}, "
                f"frame_stride={self.frame_stride}): {self.counts} tiles of {self.tile}")


# ---- Y'CbCr 4:2:0 frames -----------------------------------------------------------------------------------------------------------------
YUV_LAYOUTS = ("i420", "nv12", "nv21")


class YUV420Frames:
    """8-bit Y'CbCr 4:2:0 frames on the GPU, as decoders hand them out: `y` uint8 [T,H,W] and chroma of Hc = ceil(H / 2) by
    Wc = ceil(W / 2), either planar `u` and `v` [T,Hc,Wc] (I420) or interleaved `uv` [T,Hc,Wc,2] (NV12; `vu` for NV21).  The tensors may
    be views with row and frame strides - a pitched decoder surface wrapped without a copy - as long as samples of a row are adjacent
    (innermost stride 1; 2 between the pairs of an interleaved plane) and `u` and `v` share their strides.  `matrix` 'bt601' | 'bt709',
    `range` 'limited' | 'full', `siting` 'left' (chroma horizontally co-sited with even luma columns, the H.264 / HEVC default) |
    'center'.  include/titok_hip.h defines every value computed from or into such frames."""

    def __init__(self, y, u=None, v=None, uv=None, matrix: str = "bt709", range: str = "limited", siting: str = "left", vu=None):
        given = [k for k, t in (("u", u), ("v", v), ("uv", uv), ("vu", vu)) if t is not None]
        if given not in (["u", "v"], ["uv"], ["vu"]):
            raise ValueError(f"YUV420Frames: give u and v, or uv, or vu; got {given or 'no chroma'}")
        for name, table, value in (("matrix", _lib.YUV_MATRIX, matrix), ("range", _lib.YUV_RANGE, range), ("siting", _lib.YUV_SITING, siting)):
            if value not in table:
                raise ValueError(f"YUV420Frames: {name} must be one of {sorted(table)}, got {value!r}")
        if not isinstance(y, torch.Tensor) or y.dtype != torch.uint8 or y.dim() != 3 or min(y.shape) < 1:
            raise ValueError(f"YUV420Frames: y must be uint8 [T,H,W], got {getattr(y, 'dtype', type(y))} {tuple(getattr(y, 'shape', ()))}")
        T, H, W = (int(n) for n in y.shape)
        Hc, Wc = (H + 1) // 2, (W + 1) // 2
        pair = uv if uv is not None else vu
        if pair is not None:
            if not isinstance(pair, torch.Tensor) or pair.dtype != torch.uint8 or tuple(pair.shape) != (T, Hc, Wc, 2):
                raise ValueError(f"YUV420Frames: interleaved chroma must be uint8 {(T, Hc, Wc, 2)}, got {getattr(pair, 'dtype', type(pair))} "
                                 f"{tuple(getattr(pair, 'shape', ()))}")
            if pair.stride(3) != 1 or (Wc > 1 and pair.stride(2) != 2):
                raise ValueError(f"YUV420Frames: the pairs of interleaved chroma must be adjacent bytes (strides 2, 1), got {pair.stride()[2:]}")
            first, second = pair[..., 0], pair[..., 1]
            u, v = (first, second) if uv is not None else (second, first)
            self.layout, step = ("nv12" if uv is not None else "nv21"), 2
        else:
            for name, t in (("u", u), ("v", v)):
                if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or tuple(t.shape) != (T, Hc, Wc):
                    raise ValueError(f"YUV420Frames: {name} must be uint8 {(T, Hc, Wc)}, got {getattr(t, 'dtype', type(t))} "
                                     f"{tuple(getattr(t, 'shape', ()))}")
            if Wc > 1 and (u.stride(2) != 1 or v.stride(2) != 1):
                raise ValueError(f"YUV420Frames: the samples of a chroma row must be adjacent bytes, got strides {u.stride(2)} and {v.stride(2)}")
            if (Hc > 1 and u.stride(1) != v.stride(1)) or (T > 1 and u.stride(0) != v.stride(0)):
                raise ValueError(f"YUV420Frames: u and v must share their row and frame strides, got {u.stride()} and {v.stride()}")
            self.layout, step = "i420", 1
        if W > 1 and y.stride(2) != 1:
            raise ValueError(f"YUV420Frames: the samples of a luma row must be adjacent bytes, got stride {y.stride(2)}")
        c_row = step * (Wc - 1) + 1
        self.y_pitch = int(y.stride(1)) if H > 1 else W
        self.c_pitch = int(u.stride(1)) if Hc > 1 else step * Wc
        y_min, c_min = (H - 1) * self.y_pitch + W, (Hc - 1) * self.c_pitch + c_row
        self.y_frame = int(y.stride(0)) if T > 1 else y_min
        self.c_frame = int(u.stride(0)) if T > 1 else c_min
        if self.y_pitch < W or self.c_pitch < step * Wc or self.y_frame < y_min or self.c_frame < c_min:
            raise ValueError(f"YUV420Frames: rows or frames overlap: luma strides {y.stride()} for {(T, H, W)}, chroma strides {u.stride()} "
                             f"for {(T, Hc, Wc)} at {step} byte(s) per sample")
        if self.y_pitch >= 1 << 31 or self.c_pitch >= 1 << 31:
            raise ValueError("YUV420Frames: a row pitch of 2^31 bytes or more")
        if not (y.device == u.device == v.device):
            raise ValueError(f"YUV420Frames: planes on different devices: {y.device}, {u.device}, {v.device}")
        _lib.require_gpu(y, "YUV420Frames")
        self.y, self.u, self.v, self.c_step = y, u, v, step
        self.matrix, self.range, self.siting = matrix, range, siting
        self.shape: Tuple[int, int, int] = (T, H, W)
        self.device = y.device

    @classmethod
    def empty(cls, T: int, H: int, W: int, layout: str = "i420", device="cuda", matrix: str = "bt709", range: str = "limited",
              siting: str = "left") -> "YUV420Frames":
        """Uninitialised planes for T frames of H x W: 'i420' (planar u, v), 'nv12' (interleaved uv) or 'nv21' (interleaved vu)."""
        if layout not in YUV_LAYOUTS:
            raise ValueError(f"YUV420Frames.empty: layout must be one of {YUV_LAYOUTS}, got {layout!r}")
        T, H, W = int(T), int(H), int(W)
        if min(T, H, W) < 1:
            raise ValueError(f"YUV420Frames.empty: {(T, H, W)} must be at least 1 on every axis")
        Hc, Wc = (H + 1) // 2, (W + 1) // 2
        y = torch.empty((T, H, W), dtype=torch.uint8, device=device)
        kw = dict(matrix=matrix, range=range, siting=siting)
        if layout == "i420":
            return cls(y, u=torch.empty((T, Hc, Wc), dtype=torch.uint8, device=device), v=torch.empty((T, Hc, Wc), dtype=torch.uint8, device=device), **kw)
        pair = torch.empty((T, Hc, Wc, 2), dtype=torch.uint8, device=device)
        return cls(y, uv=pair, **kw) if layout == "nv12" else cls(y, vu=pair, **kw)

    def frames(self, t0: int, t1: int) -> "YUV420Frames":
        """Frames [t0, t1) as views of the same planes."""
        if not 0 <= t0 < t1 <= self.shape[0]:
            raise ValueError(f"frames [{t0}, {t1}) of {self.shape[0]}")
        out = object.__new__(YUV420Frames)
        out.__dict__.update(self.__dict__)
        out.y, out.u, out.v = self.y[t0:t1], self.u[t0:t1], self.v[t0:t1]
        out.shape = (t1 - t0,) + self.shape[1:]
        return out

    def like(self, T: int) -> "YUV420Frames":
        """New planes for T frames of this picture size, layout and colour description."""
        return YUV420Frames.empty(T, self.shape[1], self.shape[2], self.layout, self.device, self.matrix, self.range, self.siting)

    def c_frames(self) -> "_lib.Yuv420":
        return _lib.Yuv420(y=self.y.data_ptr(), u=self.u.data_ptr(), v=self.v.data_ptr(), y_frame=self.y_frame, c_frame=self.c_frame,
                           y_pitch=self.y_pitch, c_pitch=self.c_pitch, c_step=self.c_step, matrix=_lib.YUV_MATRIX[self.matrix],
                           range=_lib.YUV_RANGE[self.range], siting=_lib.YUV_SITING[self.siting])

    def __repr__(self):
        return f"YUV420Frames({self.shape}, {self.layout}, {self.matrix}, {self.range}, {self.siting})"


def _frames_shape(frames, what: str) -> Tuple[int, int, int]:
    """(T, H, W) of uint8 [T,H,W,3] frames or of a `YUV420Frames`, which is on the GPU."""
    if isinstance(frames, YUV420Frames):
        return frames.shape
    _lib.require_gpu(frames, what)
    if frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError(f"frames must be uint8 [T,H,W,3] or YUV420Frames, got {tuple(frames.shape)}")
    return tuple(frames.shape[:3])


# ---- the three kernels ----------------------------------------------------------------------------------------------------------------
def gather_tiles(frames_u8: torch.Tensor, plan: TilePlan, begin: int = 0, end: Optional[int] = None,
                 dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """Tiles [begin, end) of `plan` cut from decoded frames uint8 [T,H,W,3] on the GPU: one buffer [end - begin, 3, Tt, Ht, Wt] in
    `dtype`, values u8 / 127.5 - 1 (the loader's bits).  One launch on the current stream.  `frames_u8` may be a `YUV420Frames`: the
    values are then the header's N / 8355840 - 1 of the converted pixels, not rounded to 8 bits on the way (`ttv_video_tiles_yuv420`)."""
    if isinstance(frames_u8, YUV420Frames):
        if frames_u8.shape != plan.video:
            raise ValueError(f"frames must be YUV420Frames of {plan.video}, got {frames_u8.shape}")
        end = plan.n_tiles if end is None else int(end)
        if not 0 <= begin <= end <= plan.n_tiles:
            raise ValueError(f"tiles [{begin}, {end}) of {plan.n_tiles}")
        out = torch.empty((end - begin, 3) + plan.tile, dtype=dtype, device=frames_u8.device)
        cp, cf = plan.c_plan(), frames_u8.c_frames()
        _lib.check(_lib.lib().ttv_video_tiles_yuv420(C.byref(cf), C.byref(cp), int(begin), end, out.data_ptr(), _lib.dtype_code(dtype),
                                                     _lib.stream_ptr(frames_u8.device)), "ttv_video_tiles_yuv420")
        return out
    _lib.require_gpu(frames_u8, "gather_tiles")
    if frames_u8.dtype != torch.uint8 or tuple(frames_u8.shape) != plan.video + (3,) or not frames_u8.is_contiguous():
        raise ValueError(f"frames must be contiguous uint8 {plan.video + (3,)}, got {frames_u8.dtype} {tuple(frames_u8.shape)}")
    end = plan.n_tiles if end is None else int(end)
    if not 0 <= begin <= end <= plan.n_tiles:
        raise ValueError(f"tiles [{begin}, {end}) of {plan.n_tiles}")
    out = torch.empty((end - begin, 3) + plan.tile, dtype=dtype, device=frames_u8.device)
    cp = plan.c_plan()
    _lib.check(_lib.lib().ttv_video_tiles_u8(frames_u8.data_ptr(), C.byref(cp), int(begin), end, out.data_ptr(), _lib.dtype_code(dtype),
                                             _lib.stream_ptr(frames_u8.device)), "ttv_video_tiles_u8")
    return out


def blend_tiles(tiles: Sequence[Optional[torch.Tensor]], plan: TilePlan, t0: int = 0, t1: Optional[int] = None, out=None):
    """Frames [t0, t1) of the timeline, uint8 [t1 - t0, H, W, 3] on the GPU, from reconstructed tiles [3,Tt,Ht,Wt] in tile order; an
    entry may be None when its tile holds no frame of the range.  Overlaps are the weighted mean the header defines; bit-reproducible.
    One launch on the current stream.  `out`: None for RGB; 'i420' | 'nv12' | 'nv21' for new `YUV420Frames` (BT.709, limited range,
    left-sited); or a `YUV420Frames` of (t1 - t0, H, W) whose planes are written and which is returned (`ttv_video_blend_yuv420`: the
    same blended levels, converted in the same launch)."""
    t1 = plan.timeline[0] if t1 is None else int(t1)
    if len(tiles) != plan.n_tiles:
        raise ValueError(f"{len(tiles)} tiles for a plan of {plan.n_tiles}")
    given = [t for t in tiles if t is not None]
    if not given:
        raise ValueError("blend_tiles: no tile given")
    dtype, device = given[0].dtype, given[0].device
    for t in given:
        _lib.require_gpu(t, "blend_tiles")
        if t.dtype != dtype or t.device != device or tuple(t.shape) != (3,) + plan.tile or not t.is_contiguous():
            raise ValueError(f"tiles must be contiguous {(3,) + plan.tile} of one dtype on one device, got {t.dtype} {tuple(t.shape)}")
    ptrs = [0 if t is None else t.data_ptr() for t in tiles]
    host = (_lib.vp * len(ptrs))(*ptrs)
    table = torch.tensor(ptrs, dtype=torch.int64).to(device)
    cp = plan.c_plan()
    if out is not None:
        if isinstance(out, str):
            if t1 <= t0:
                raise ValueError(f"blend_tiles: no frame in [{t0}, {t1}) to make {out} planes for")
            out = YUV420Frames.empty(t1 - t0, plan.timeline[1], plan.timeline[2], out, device)
        if not isinstance(out, YUV420Frames) or out.shape != (t1 - t0,) + plan.timeline[1:] or out.device != device:
            raise ValueError(f"out must be a layout name or YUV420Frames of {(t1 - t0,) + plan.timeline[1:]} on {device}, got {out!r}")
        cf = out.c_frames()
        _lib.check(_lib.lib().ttv_video_blend_yuv420(host, table.data_ptr(), C.byref(cp), int(t0), t1, _lib.dtype_code(dtype), C.byref(cf),
                                                     _lib.stream_ptr(device)), "ttv_video_blend_yuv420")
        return out
    out = torch.empty((max(t1 - t0, 0),) + plan.timeline[1:] + (3,), dtype=torch.uint8, device=device)
    _lib.check(_lib.lib().ttv_video_blend_u8(host, table.data_ptr(), C.byref(cp), int(t0), t1, _lib.dtype_code(dtype), out.data_ptr(),
                                             _lib.stream_ptr(device)), "ttv_video_blend_u8")
    return out


def tile_sse(frames_u8: torch.Tensor, plan: TilePlan, recon_tiles: Sequence[torch.Tensor], begin: int = 0,
             end: Optional[int] = None) -> torch.Tensor:
    """Per tile of [begin, end) the sum of squared level differences between its reconstruction `recon_tiles[k - begin]`
    ([3,Tt,Ht,Wt], what the model returns for the tile `gather_tiles` cut) and the source pixels of `frames_u8`: int64 [end - begin] on
    the GPU, exact integers (`ttv_video_tile_sse_u8`; the header defines the level of an element and which samples count).  One launch
    on the current stream.  With `YUV420Frames` the source level is the header's (N + 32768) >> 16 (`ttv_video_tile_sse_yuv420`)."""
    yuv = isinstance(frames_u8, YUV420Frames)
    if yuv:
        if frames_u8.shape != plan.video:
            raise ValueError(f"frames must be YUV420Frames of {plan.video}, got {frames_u8.shape}")
    else:
        _lib.require_gpu(frames_u8, "tile_sse")
        if frames_u8.dtype != torch.uint8 or tuple(frames_u8.shape) != plan.video + (3,) or not frames_u8.is_contiguous():
            raise ValueError(f"frames must be contiguous uint8 {plan.video + (3,)}, got {frames_u8.dtype} {tuple(frames_u8.shape)}")
    end = plan.n_tiles if end is None else int(end)
    if not 0 <= begin <= end <= plan.n_tiles:
        raise ValueError(f"tiles [{begin}, {end}) of {plan.n_tiles}")
    if len(recon_tiles) != end - begin:
        raise ValueError(f"{len(recon_tiles)} reconstructions for tiles [{begin}, {end})")
    device = frames_u8.device
    out = torch.empty((end - begin,), dtype=torch.int64, device=device)
    if end == begin:
        return out
    dtype = recon_tiles[0].dtype
    for t in recon_tiles:
        _lib.require_gpu(t, "tile_sse")
        if t.dtype != dtype or t.device != device or tuple(t.shape) != (3,) + plan.tile or not t.is_contiguous():
            raise ValueError(f"reconstructions must be contiguous {(3,) + plan.tile} of one dtype on the frames' device, got {t.dtype} "
                             f"{tuple(t.shape)} on {t.device}")
    ptrs = [t.data_ptr() for t in recon_tiles]
    host = (_lib.vp * len(ptrs))(*ptrs)
    # from pinned memory and without waiting: a pageable upload would hold the host until the stream has run everything queued
    # before it - the forward that made these tiles - and the next batch of the pipeline could not be queued meanwhile
    table = torch.tensor(ptrs, dtype=torch.int64).pin_memory().to(device, non_blocking=True)
    cp = plan.c_plan()
    if yuv:
        cf = frames_u8.c_frames()
        _lib.check(_lib.lib().ttv_video_tile_sse_yuv420(C.byref(cf), C.byref(cp), int(begin), end, host, table.data_ptr(),
                                                        _lib.dtype_code(dtype), out.data_ptr(), _lib.stream_ptr(device)), "ttv_video_tile_sse_yuv420")
        return out
    _lib.check(_lib.lib().ttv_video_tile_sse_u8(frames_u8.data_ptr(), C.byref(cp), int(begin), end, host, table.data_ptr(),
                                                _lib.dtype_code(dtype), out.data_ptr(), _lib.stream_ptr(device)), "ttv_video_tile_sse_u8")
    return out


# ---- per-frame quality of what comes back ---------------------------------------------------------------------------------------------
def _frame_pair(a, b, b_stride: int, what: str, min_rgb: int, min_yuv: int):
    """The checks `frame_sse` and `frame_ssim` share: (yuv, n, H, W, device).  Shapes and kinds are judged before the device, so a
    malformed call is a ValueError wherever its tensors live."""
    b_stride = int(b_stride)
    if b_stride < 1:
        raise ValueError(f"{what}: b_stride must be at least 1, got {b_stride}")
    yuv = isinstance(a, YUV420Frames)
    if yuv != isinstance(b, YUV420Frames):
        raise ValueError(f"{what}: a and b must both be uint8 [.,H,W,3] tensors or both YUV420Frames, got {type(a).__name__} and "
                         f"{type(b).__name__}")
    if yuv:
        sa, sb = a.shape, b.shape
        if (a.matrix, a.range, a.siting) != (b.matrix, b.range, b.siting):
            raise ValueError(f"{what}: planes of different colour descriptions are not comparable sample by sample: "
                             f"{(a.matrix, a.range, a.siting)} and {(b.matrix, b.range, b.siting)}")
    else:
        for name, t in (("a", a), ("b", b)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 4 or t.shape[-1] != 3 or not t.is_contiguous():
                raise ValueError(f"{what}: {name} must be contiguous uint8 [.,H,W,3], got {getattr(t, 'dtype', type(t))} "
                                 f"{tuple(getattr(t, 'shape', ()))}")
        sa, sb = tuple(a.shape[:3]), tuple(b.shape[:3])
    if sa[1:] != sb[1:]:
        raise ValueError(f"{what}: frames of {sa[1:]} against frames of {sb[1:]}")
    n, least = sa[0], min_yuv if yuv else min_rgb
    if min(sa[1:]) < least:
        raise ValueError(f"{what}: frames of {sa[1:]}; H and W must be at least {least}")
    if n > 0 and sb[0] < (n - 1) * b_stride + 1:
        raise ValueError(f"{what}: b holds {sb[0]} frames, {n} frames at b_stride {b_stride} need {(n - 1) * b_stride + 1}")
    if not yuv:
        _lib.require_gpu(a, what)
        _lib.require_gpu(b, what)
    if a.device != b.device:
        raise ValueError(f"{what}: a on {a.device}, b on {b.device}")
    return yuv, n, sa[1], sa[2], a.device


def frame_sse(a, b, b_stride: int = 1) -> torch.Tensor:
    """Per frame and component the sum of squared level differences between frame j of `a` and frame j * b_stride of `b`: int64 [n, 3]
    on the GPU, exact integers.  `a`, `b`: both contiguous uint8 [.,H,W,3] on the GPU (components R, G, B) or both `YUV420Frames` of
    one colour description (Y of H x W, U and V of ceil(H / 2) x ceil(W / 2); layouts and pitches may differ).  One call into the
    library on the current stream (`ttv_video_frame_sse_u8` / `ttv_video_frame_sse_yuv420`)."""
    yuv, n, H, W, device = _frame_pair(a, b, b_stride, "frame_sse", 1, 1)
    out = torch.empty((n, 3), dtype=torch.int64, device=device)
    if n == 0:
        return out
    if yuv:
        ca, cb = a.c_frames(), b.c_frames()
        _lib.check(_lib.lib().ttv_video_frame_sse_yuv420(C.byref(ca), C.byref(cb), n, int(b_stride), H, W, out.data_ptr(),
                                                         _lib.stream_ptr(device)), "ttv_video_frame_sse_yuv420")
    else:
        _lib.check(_lib.lib().ttv_video_frame_sse_u8(a.data_ptr(), b.data_ptr(), n, int(b_stride), H, W, out.data_ptr(),
                                                     _lib.stream_ptr(device)), "ttv_video_frame_sse_u8")
    return out


def frame_ssim(a, b, b_stride: int = 1) -> torch.Tensor:
    """Per frame and component the SSIM between frame j of `a` and frame j * b_stride of `b`: float64 [n, 3] on the GPU.  The
    arguments are `frame_sse`'s; include/titok_hip.h has the definition (levels 0 .. 255, the 11-tap Gaussian, the windows wholly
    inside a plane), so H and W must be at least 11, and at least 21 for `YUV420Frames`, whose chroma planes are half the size.
    One call into the library on the current stream (`ttv_video_frame_ssim_u8` / `ttv_video_frame_ssim_yuv420`)."""
    yuv, n, H, W, device = _frame_pair(a, b, b_stride, "frame_ssim", 11, 21)
    out = torch.empty((n, 3), dtype=torch.float64, device=device)
    if n == 0:
        return out
    h = _lib.lib()
    need = int(h.ttv_video_frame_ssim_workspace_bytes(n, H, W, int(yuv)))
    if need < 0:
        _lib.check(1, "ttv_video_frame_ssim_workspace_bytes")
    work = torch.empty((need // 8,), dtype=torch.float64, device=device)
    if yuv:
        ca, cb = a.c_frames(), b.c_frames()
        _lib.check(h.ttv_video_frame_ssim_yuv420(C.byref(ca), C.byref(cb), n, int(b_stride), H, W, out.data_ptr(), work.data_ptr(), need,
                                                 _lib.stream_ptr(device)), "ttv_video_frame_ssim_yuv420")
    else:
        _lib.check(h.ttv_video_frame_ssim_u8(a.data_ptr(), b.data_ptr(), n, int(b_stride), H, W, out.data_ptr(), work.data_ptr(), need,
                                             _lib.stream_ptr(device)), "ttv_video_frame_ssim_u8")
    return out


class VideoQuality:
    """Per-frame PSNR and SSIM per component of a video against its source, from `frame_sse` and `frame_ssim`.

    `components` is ('r', 'g', 'b') or ('y', 'u', 'v'); `elements[c]` the samples of component c in a frame (H W, and
    ceil(H / 2) ceil(W / 2) for 4:2:0 chroma).  `update` queues the measurement of a frame range and keeps its results on the GPU;
    `finish` reads everything back once.  After it `sse[frame][c]` holds Python ints and `ssim[frame][c]` floats (`ssim` is None when
    no range was measured with it); frame 0 is timeline frame `t0`, the start of the first range."""

    def __init__(self, height: int, width: int, yuv420: bool = False):
        H, W = int(height), int(width)
        if min(H, W) < 1:
            raise ValueError(f"VideoQuality: frames of {(H, W)}")
        self.yuv420 = bool(yuv420)
        self.components = ("y", "u", "v") if self.yuv420 else ("r", "g", "b")
        chroma = ((H + 1) // 2) * ((W + 1) // 2)
        self.elements = (H * W, chroma, chroma) if self.yuv420 else (H * W,) * 3
        self.shape = (H, W)
        self.t0 = 0
        self.sse: Optional[List[List[int]]] = None
        self.ssim: Optional[List[List[float]]] = None
        self._parts: List[Tuple[int, torch.Tensor, Optional[torch.Tensor]]] = []

    def update(self, decoded, source, t0: int, frame_stride: int = 1, ssim: bool = True) -> None:
        """Queue `decoded` - the frames of a range of the timeline that starts at frame `t0` - against `source[frame_stride * (t0 + j)]`
        on the current stream.  Every range of one object is measured with or without SSIM, as the first one was."""
        t0, frame_stride = int(t0), int(frame_stride)
        if t0 < 0 or frame_stride < 1:
            raise ValueError(f"VideoQuality.update: t0 {t0}, frame_stride {frame_stride}")
        kind = "YUV420Frames" if self.yuv420 else "uint8 [T,H,W,3]"
        if not isinstance(source, (YUV420Frames, torch.Tensor)) or isinstance(source, YUV420Frames) != self.yuv420:
            raise ValueError(f"VideoQuality.update: the source must be {kind} of {self.shape}, got {type(source).__name__}")
        shape = tuple(source.shape[:3])
        if len(shape) != 3 or shape[1:] != self.shape:
            raise ValueError(f"VideoQuality.update: the source must be {kind} of {self.shape}, got {tuple(source.shape)}")
        first = frame_stride * t0
        if first >= shape[0]:
            raise ValueError(f"VideoQuality.update: timeline frame {t0} at frame_stride {frame_stride} is source frame {first} of {shape[0]}")
        if self._parts and (self._parts[0][2] is not None) != bool(ssim):
            raise ValueError("VideoQuality.update: every range is measured with SSIM or none is")
        yardstick = source.frames(first, shape[0]) if self.yuv420 else source[first:]
        self._parts.append((t0, frame_sse(decoded, yardstick, frame_stride), frame_ssim(decoded, yardstick, frame_stride) if ssim else None))

    def finish(self) -> "VideoQuality":
        """Read the queued results back (one transfer) and order them by frame.  The ranges must follow each other without a gap."""
        if not self._parts:
            raise ValueError("VideoQuality.finish: nothing was measured")
        parts = sorted(self._parts, key=lambda p: p[0])
        at = parts[0][0]
        for t0, sse, _ in parts:
            if t0 != at:
                raise ValueError(f"VideoQuality.finish: a range starts at frame {t0}, the one before it ends at {at}")
            at += sse.shape[0]
        with_ssim = parts[0][2] is not None
        flat = [p[1].reshape(-1) for p in parts] + ([p[2].view(torch.int64).reshape(-1) for p in parts] if with_ssim else [])
        host = torch.cat(flat).cpu()
        n = at - parts[0][0]
        self.t0 = parts[0][0]
        self.sse = host[:3 * n].view(n, 3).tolist()
        self.ssim = host[3 * n:].view(torch.float64).view(n, 3).tolist() if with_ssim else None
        self._parts = []
        return self

    def _done(self) -> List[List[int]]:
        if self.sse is None:
            raise ValueError("VideoQuality: call finish() first")
        return self.sse

    @staticmethod
    def _db(sse: int, elements: int) -> float:
        return math.inf if sse == 0 else 10.0 * math.log10(65025 * elements / sse)

    def psnr(self) -> List[List[float]]:
        """[frame][c] 10 log10(65025 elements[c] / sse) in float64 (levels 0 .. 255), inf where the sum is 0."""
        return [[self._db(v, e) for v, e in zip(row, self.elements)] for row in self._done()]

    def psnr_overall(self) -> List[float]:
        """Per component, from the sums over all frames."""
        sse = self._done()
        return [self._db(sum(row[c] for row in sse), len(sse) * self.elements[c]) for c in range(3)]

    def psnr_pooled(self) -> float:
        """All three components together: summed sums over summed sample counts.  For 4:2:0 this weights Y : U : V as 4 : 1 : 1 (by
        their sample counts), the usual single-number PSNR of a 4:2:0 codec comparison."""
        sse = self._done()
        return self._db(sum(sum(row) for row in sse), len(sse) * sum(self.elements))

    def ssim_mean(self) -> Optional[List[float]]:
        """Per component the mean over the frames, or None without SSIM."""
        self._done()
        return None if self.ssim is None else [sum(row[c] for row in self.ssim) / len(self.ssim) for c in range(3)]

    def worst_frame(self, c: int = 0) -> int:
        """The timeline frame whose component `c` has the largest sum of squares (the lowest PSNR); the first of equals."""
        sse = self._done()
        return self.t0 + max(range(len(sse)), key=lambda j: (sse[j][c], -j))

    def as_dict(self) -> dict:
        """Everything as plain lists and numbers (`json.dumps` takes it); an infinite PSNR is None."""
        def fin(v):
            return None if math.isinf(v) else v
        return {"components": list(self.components), "elements": list(self.elements), "t0": self.t0, "frames": len(self._done()),
                "sse": [list(row) for row in self.sse], "ssim": None if self.ssim is None else [list(row) for row in self.ssim],
                "psnr": [[fin(v) for v in row] for row in self.psnr()], "psnr_overall": [fin(v) for v in self.psnr_overall()],
                "psnr_pooled": fin(self.psnr_pooled()), "ssim_mean": self.ssim_mean(), "worst_frame": [self.worst_frame(c) for c in range(3)]}


# ---- the token container ----------------------------------------------------------------------------------------------------------------
def index_bits(codebook_size: int) -> int:
    """Bits per stored index: max(1, ceil(log2(codebook_size)))."""
    return max(1, (int(codebook_size) - 1).bit_length())


def pack_indices(indices: np.ndarray, bits: int) -> bytes:
    """Index i in bits [i * bits, (i + 1) * bits) of the stream, least significant bit first, bytes little-endian."""
    idx = np.asarray(indices, dtype=np.uint32).reshape(-1)
    planes = ((idx[:, None] >> np.arange(bits, dtype=np.uint32)) & 1).astype(np.uint8)
    return np.packbits(planes.reshape(-1), bitorder="little").tobytes()


def unpack_indices(data: bytes, n: int, bits: int) -> np.ndarray:
    planes = np.unpackbits(np.frombuffer(data, dtype=np.uint8), bitorder="little")[:n * bits].reshape(n, bits).astype(np.int64)
    return (planes << np.arange(bits, dtype=np.int64)).sum(axis=1).astype(np.int32)


class VideoTokens:
    """What `encode_video` returns: `indices` int32 [sum counts] in tile order, `counts` tokens per tile, the plan's parameters
    (`video`, `tile`, `overlap`, `patch`, `frame_stride`), `fps` of the timeline (source fps / frame_stride, or None), `codebook_size`
    and `quantizer` ('fsq' or 'l2')."""

    def __init__(self, indices, counts, video, tile, overlap, patch, frame_stride, fps, codebook_size, quantizer):
        self.indices = indices if isinstance(indices, torch.Tensor) else torch.as_tensor(np.asarray(indices), dtype=torch.int32)
        self.counts = [int(c) for c in counts]
        self.video, self.tile, self.overlap, self.patch = _triple(video, "video"), _triple(tile, "tile"), _triple(overlap, "overlap"), _triple(patch, "patch")
        self.frame_stride, self.fps = int(frame_stride), (None if fps is None else float(fps))
        self.codebook_size, self.quantizer = int(codebook_size), str(quantizer)
        if self.indices.dim() != 1 or self.indices.numel() != sum(self.counts):
            raise ValueError(f"{self.indices.numel()} indices for counts that sum to {sum(self.counts)}")

    def plan(self) -> TilePlan:
        return TilePlan(self.video, self.tile, self.overlap, self.patch, self.frame_stride)

    def to_bytes(self) -> bytes:
        """MAGIC (8 bytes) | version uint32 | header length uint32 (both little-endian) | JSON header | the indices packed at
        max(1, ceil(log2(codebook_size))) bits each, least significant bit first."""
        bits = index_bits(self.codebook_size)
        idx = self.indices.detach().to("cpu").numpy().astype(np.int64)
        if idx.size and (idx.min() < 0 or idx.max() >= self.codebook_size):
            raise ValueError(f"indices outside 0 .. {self.codebook_size - 1}")
        uniform = len(set(self.counts)) <= 1
        header = json.dumps({"video": self.video, "tile": self.tile, "overlap": self.overlap, "patch": self.patch,
                             "frame_stride": self.frame_stride, "fps": self.fps, "codebook_size": self.codebook_size,
                             "quantizer": self.quantizer, "n_tiles": len(self.counts),
                             "counts": (self.counts[0] if self.counts else 0) if uniform else self.counts,
                             "n_indices": int(idx.size), "bits": bits}, separators=(",", ":")).encode("utf-8")
        return MAGIC + struct.pack("<II", VERSION, len(header)) + header + pack_indices(idx, bits)

    @classmethod
    def from_bytes(cls, data: bytes) -> "VideoTokens":
        data = bytes(data)
        if len(data) < 16 or data[:8] != MAGIC:
            raise ValueError("not a TTVTOK token stream")
        version, hlen = struct.unpack("<II", data[8:16])
        if version != VERSION:
            raise ValueError(f"token stream version {version}, this reader knows {VERSION}")
        if len(data) < 16 + hlen:
            raise ValueError("token stream is truncated inside its header")
        try:
            h = json.loads(data[16:16 + hlen].decode("utf-8"))
            n, bits, n_tiles = int(h["n_indices"]), int(h["bits"]), int(h["n_tiles"])
            counts = [int(h["counts"])] * n_tiles if isinstance(h["counts"], int) else [int(c) for c in h["counts"]]
            fields = [h[k] for k in ("video", "tile", "overlap", "patch", "frame_stride", "fps", "codebook_size", "quantizer")]
        except (ValueError, KeyError, TypeError) as e:
            raise ValueError(f"token stream header is damaged: {e}") from None
        if bits != index_bits(fields[6]) or len(counts) != n_tiles or sum(counts) != n:
            raise ValueError("token stream header is inconsistent")
        body = data[16 + hlen:]
        if len(body) != (n * bits + 7) // 8:
            raise ValueError(f"token stream holds {len(body)} bytes of indices, its header promises {(n * bits + 7) // 8}")
        idx = unpack_indices(body, n, bits)
        if n and int(idx.max()) >= int(fields[6]):
            raise ValueError("token stream holds an index outside its codebook")
        return cls(torch.from_numpy(idx), counts, *fields)

    def save(self, path) -> None:
        with open(path, "wb") as f:
            f.write(self.to_bytes())

    @classmethod
    def load(cls, path) -> "VideoTokens":
        with open(path, "rb") as f:
            return cls.from_bytes(f.read())

    @property
    def bits_per_pixel(self) -> float:
        """8 * len(to_bytes()) / (T' * H * W): the whole container over the pixels of the timeline."""
        t = -(-self.video[0] // self.frame_stride)
        return 8.0 * len(self.to_bytes()) / (t * self.video[1] * self.video[2])


# ---- rate and distortion ------------------------------------------------------------------------------------------------------------------
def _check_ladder(ladder) -> Tuple[int, ...]:
    out = tuple(int(k) for k in ladder)
    if not out or out[0] < 1 or any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError(f"a ladder is ascending distinct token counts of at least 1, got {tuple(ladder)!r}")
    return out


def default_ladder(tokens_per_tile: int) -> Tuple[int, ...]:
    """tokens_per_tile / 8, / 4, / 2 and tokens_per_tile itself, rounded up, the distinct ones."""
    k = int(tokens_per_tile)
    if k < 1:
        raise ValueError(f"tokens_per_tile must be at least 1, got {tokens_per_tile}")
    return tuple(sorted({-(-k // d) for d in (8, 4, 2, 1)}))


class RateTable:
    """What every tile of a video costs at every token count of a ladder (`VideoTokenizer.rate_distortion`).  `ladder`: ascending
    distinct counts; `sse[tile][level]`: Python ints, the tile's `tile_sse` when coded with `ladder[level]` tokens; `elements[tile]`:
    the samples that sum runs over (`TilePlan.tile_elements`); `indices[tile][level]`: the int32 indices the probe produced, or None
    for a table that only feeds `allocate_tokens`."""

    def __init__(self, ladder, sse, elements, indices=None):
        self.ladder = _check_ladder(ladder)
        self.sse = [[int(v) for v in row] for row in sse]
        self.elements = [int(e) for e in elements]
        self.indices = indices
        if len(self.elements) != len(self.sse) or any(len(row) != len(self.ladder) for row in self.sse):
            raise ValueError(f"sse must be [n_tiles][{len(self.ladder)}] with one element count per tile")
        if any(v < 0 for row in self.sse for v in row) or any(e < 1 for e in self.elements):
            raise ValueError("sums of squares are at least 0 and element counts at least 1")
        if indices is not None and (len(indices) != len(self.sse) or any(len(row) != len(self.ladder) for row in indices)):
            raise ValueError(f"indices must be [n_tiles][{len(self.ladder)}]")

    @property
    def n_tiles(self) -> int:
        return len(self.sse)

    def psnr(self) -> List[List[float]]:
        """[tile][level] 10 log10(65025 elements / sse) in float64 (levels 0 .. 255), inf where the sum is 0."""
        return [[math.inf if v == 0 else 10.0 * math.log10(65025 * e / v) for v in row] for row, e in zip(self.sse, self.elements)]


def _hull_levels(ladder: Sequence[int], row: Sequence[int]) -> List[int]:
    """Levels of the lower convex hull of the points (ladder[l], row[l]) from level 0 on, as far as it falls: each step of it lowers
    the sum, and the drop per token shrinks from step to step.  Integer cross-multiplication, no division."""
    hull = [0]
    for l in range(1, len(ladder)):
        while len(hull) >= 2:
            a, b = hull[-2], hull[-1]
            # b stays only when it lies strictly below the chord a -> l
            if (row[b] - row[a]) * (ladder[l] - ladder[a]) >= (row[l] - row[a]) * (ladder[b] - ladder[a]):
                hull.pop()
            else:
                break
        hull.append(l)
    keep = [0]
    for l in hull[1:]:
        if row[l] >= row[keep[-1]]:
            break
        keep.append(l)
    return keep


def allocate_tokens(table: RateTable, target_psnr: Optional[float] = None, total_tokens: Optional[int] = None) -> List[int]:
    """One ladder count per tile from measured distortion; exactly one of the two arguments.  Pure Python on the table's exact
    integers, and nothing assumes that a tile's sum falls as its count grows.

    target_psnr: per tile the smallest count whose `RateTable.psnr` reaches the target; where none does, the count of the least sum
    (the smaller count on a tie).
    total_tokens: every tile starts at ladder[0] (ValueError when the budget is below n_tiles * ladder[0]).  Each tile's candidates
    are the steps of its lower convex hull from ladder[0] on, as far as the hull falls.  Among the tiles' next steps that still fit
    what is left of the budget, the one with the largest drop of the sum per token is taken (the lower tile index on a tie), until
    no step fits.  If a uniform ladder count that fits the budget has a lower total than the result, the best such count is returned
    for every tile (the smaller count on a tie): the result is never worse than uniform at the same budget."""
    if (target_psnr is None) == (total_tokens is None):
        raise ValueError("allocate_tokens: give exactly one of target_psnr and total_tokens")
    ladder, sse, n = table.ladder, table.sse, table.n_tiles
    if target_psnr is not None:
        target, out = float(target_psnr), []
        for row, quality in zip(sse, table.psnr()):
            reached = [l for l, q in enumerate(quality) if q >= target]
            out.append(ladder[reached[0] if reached else min(range(len(row)), key=lambda l: (row[l], l))])
        return out
    budget = int(total_tokens)
    if budget < n * ladder[0]:
        raise ValueError(f"total_tokens {budget} is below {n} tiles at the ladder's least count {ladder[0]}")
    hulls = [_hull_levels(ladder, row) for row in sse]
    at = [0] * n                                            # position on the tile's hull
    left = budget - n * ladder[0]
    while True:
        best = None                                         # (drop, tokens, tile)
        for j in range(n):
            if at[j] + 1 == len(hulls[j]):
                continue
            a, b = hulls[j][at[j]], hulls[j][at[j] + 1]
            tokens, drop = ladder[b] - ladder[a], sse[j][a] - sse[j][b]
            if tokens <= left and (best is None or drop * best[1] > best[0] * tokens):
                best = (drop, tokens, j)
        if best is None:
            break
        at[best[2]] += 1
        left -= best[1]
    levels = [hulls[j][at[j]] for j in range(n)]
    total = sum(sse[j][levels[j]] for j in range(n))
    uniform = [(sum(row[l] for row in sse), l) for l in range(len(ladder)) if n * ladder[l] <= budget]
    if uniform and min(uniform)[0] < total:
        return [ladder[min(uniform)[1]]] * n
    return [ladder[l] for l in levels]


# ---- the public surface -----------------------------------------------------------------------------------------------------------------
def _budget_ranges(rows: Sequence[int], begin: int, end: int, seq_len: int) -> List[Tuple[int, int]]:
    """Consecutive ranges of [begin, end) under the reference's token budget (data.dynamic_batches): a range is closed when the next
    tile's rows would take it past seq_len."""
    out, a, cur = [], begin, 0
    for i in range(begin, end):
        if cur + rows[i] > seq_len and i > a:
            out.append((a, i))
            a, cur = i, 0
        cur += rows[i]
    if end > a:
        out.append((a, end))
    return out


class VideoTokenizer:
    """A `TiTok` on the GPU applied to whole decoded videos.  `tile` defaults to `config.training.sampling.max_grid` when the model's
    config has it; `tokens_per_tile` is one count or one per tile; `seq_len` is the packed-row budget of a batch (rows = patches +
    tokens, the reference's rule); `dtype` is the compute dtype of the tiles (the model's); `depth` batches are in flight at a time
    while encoding (`ForwardPipeline`; 1 = everything on the current stream)."""

    def __init__(self, model, tile=None, overlap=(4, 16, 16), tokens_per_tile=128, seq_len: int = 6144,
                 dtype: torch.dtype = torch.bfloat16, depth: int = 2):
        self.model = model
        self.device = next(model.parameters()).device
        if self.device.type != "cuda":
            raise RuntimeError("VideoTokenizer needs a GPU model: titok_video_amd runs on MI355X (HIP) only, there is no CPU path")
        self.patch = _triple(model.config.tokenizer.model.patch_size, "patch_size")
        if tile is None:
            sampling = getattr(getattr(model.config, "training", None), "sampling", None)
            tile = getattr(sampling, "max_grid", None)
            if tile is None:
                raise ValueError("tile is required: the model's config has no training.sampling.max_grid")
        self.tile, self.overlap = _triple(tile, "tile"), _triple(overlap, "overlap")
        TilePlan(self.tile, self.tile, self.overlap, self.patch)           # refuses a tile off the patch lattice or a bad overlap
        self.tokens_per_tile = tokens_per_tile if isinstance(tokens_per_tile, int) else [int(k) for k in tokens_per_tile]
        self.seq_len, self.dtype, self.depth = int(seq_len), dtype, int(depth)
        _lib.dtype_code(dtype)
        if self.depth < 1:
            raise ValueError("depth must be >= 1")
        self.quantizer = model.quantizer_kind
        self.codebook_size = int(model.quantize.codebook_size)
        self._pipe = None
        self._probe_pipe = None

    def _counts(self, n_tiles: int) -> List[int]:
        k = self.tokens_per_tile
        counts = [k] * n_tiles if isinstance(k, int) else list(k)
        if len(counts) != n_tiles or min(counts) < 1:
            raise ValueError(f"tokens_per_tile: {len(counts)} counts for {n_tiles} tiles (each at least 1)")
        return counts

    def _ranges(self, plan: TilePlan, counts, begin, end):
        rows = [plan.patches_per_tile + k for k in counts]
        if max(rows) > self.seq_len:
            raise ValueError(f"a tile of {plan.tile} with {max(counts)} tokens is {max(rows)} rows, seq_len is {self.seq_len}")
        return _budget_ranges(rows, begin, end, self.seq_len)

    def _encode_batch(self, clips, counts):
        return self.model.encode(clips, counts)[1]["indices"]

    def _probe_batch(self, frames_u8, plan: TilePlan, a: int, b: int, count: int):
        """Tiles [a, b) coded at `count` tokens each and measured: (sums int64 [b - a], indices int32 [(b - a) * count]), all on the
        current stream.  The reconstructions are dropped here."""
        clips = list(gather_tiles(frames_u8, plan, a, b, self.dtype).unbind(0))
        recon, info = self.model(clips, [count] * (b - a))
        return tile_sse(frames_u8, plan, recon, a, b), info["indices"].to(torch.int32)

    def rate_distortion(self, frames_u8, ladder: Sequence[int], frame_stride: int = 1) -> RateTable:
        """What every tile costs at every count of `ladder`.  Per count, all tiles are coded at that count, in tile order, in the
        batches the token budget gives; a batch is gathered, run through the model and measured against the same frames (`tile_sse`)
        on one stream - a side stream of the pipeline when `depth` > 1 - and only its sums and indices are kept: memory is that of
        `depth` batches, whatever the video's length.  The table describes these reconstructions, batch for batch."""
        video = _frames_shape(frames_u8, "rate_distortion")
        ladder = _check_ladder(ladder)
        plan = TilePlan(video, self.tile, self.overlap, self.patch, frame_stride)
        n = plan.n_tiles
        if self.depth > 1 and self._probe_pipe is None:
            from .pipeline import ForwardPipeline
            self._probe_pipe = ForwardPipeline(self.model, depth=self.depth, device=self.device, fn=self._probe_batch)
        sums, indices = [], []
        with torch.no_grad():
            for count in ladder:
                parts, inflight = [], []
                for a, b in self._ranges(plan, [count] * n, 0, n):
                    if self.depth == 1:
                        parts.append(self._probe_batch(frames_u8, plan, a, b, count))
                        continue
                    inflight.append(self._probe_pipe.submit(frames_u8, plan, a, b, count))
                    if len(inflight) >= self.depth:                                          # at most `depth` batches of tiles alive
                        parts.append(self._probe_pipe.result(inflight.pop(0)))
                parts += [self._probe_pipe.result(t) for t in inflight]
                sums.append(torch.cat([p[0] for p in parts]))
                indices.append(torch.cat([p[1] for p in parts]).view(n, count))
            sse = torch.stack(sums, dim=1).cpu().tolist()                                    # [n_tiles][len(ladder)], one read
        return RateTable(ladder, sse, [plan.tile_elements(j) for j in range(n)],
                         [[level[j] for level in indices] for j in range(n)])

    def encode_video(self, frames_u8, fps: Optional[float] = None, frame_stride: int = 1, ladder: Optional[Sequence[int]] = None,
                     target_psnr: Optional[float] = None, total_tokens: Optional[int] = None) -> VideoTokens:
        """Decoded frames uint8 [T,H,W,3] on the GPU, or `YUV420Frames`, -> tokens of every `frame_stride`-th frame.  Tiles are gathered in tile order into
        batches under the token budget and encoded; equal tile shapes mean one cached batch plan per batch size.

        With `target_psnr` (dB per tile, levels 0 .. 255) or `total_tokens` (a budget for the whole video) the count of every tile is
        chosen from measured distortion: `rate_distortion` over `ladder` (default `default_ladder(tokens_per_tile)`), then
        `allocate_tokens`.  The tokens are the probe's own indices at the chosen count of each tile - there is no second encoding
        pass - and `counts` is the allocation.  The table describes the probe's reconstructions, batch for batch: a tile decoded later
        in another batch goes through the same arithmetic on its own rows, but nothing here decodes it again to check (`quality` does,
frame by frame, after the blend)."""
        plan = TilePlan(_frames_shape(frames_u8, "encode_video"), self.tile, self.overlap, self.patch, frame_stride)
        if target_psnr is not None or total_tokens is not None:
            if ladder is None:
                if not isinstance(self.tokens_per_tile, int):
                    raise ValueError("a ladder is required when tokens_per_tile is one count per tile")
                ladder = default_ladder(self.tokens_per_tile)
            if (target_psnr is None) == (total_tokens is None):
                raise ValueError("encode_video: give at most one of target_psnr and total_tokens")
            ladder = _check_ladder(ladder)
            if total_tokens is not None and int(total_tokens) < plan.n_tiles * ladder[0]:        # before the probe, not after it
                raise ValueError(f"total_tokens {total_tokens} is below {plan.n_tiles} tiles at the ladder's least count {ladder[0]}")
            table = self.rate_distortion(frames_u8, ladder, frame_stride)
            counts = allocate_tokens(table, target_psnr=target_psnr, total_tokens=total_tokens)
            indices = torch.cat([table.indices[j][table.ladder.index(k)] for j, k in enumerate(counts)])
            return VideoTokens(indices, counts, plan.video, self.tile, self.overlap, self.patch, plan.frame_stride,
                               None if fps is None else float(fps) / plan.frame_stride, self.codebook_size, self.quantizer)
        if ladder is not None:
            raise ValueError("encode_video: a ladder needs target_psnr or total_tokens")
        counts = self._counts(plan.n_tiles)
        ranges = self._ranges(plan, counts, 0, plan.n_tiles)
        parts, inflight = [], []
        if self.depth > 1 and self._pipe is None:
            from .pipeline import ForwardPipeline
            self._pipe = ForwardPipeline(self.model, depth=self.depth, device=self.device, fn=self._encode_batch)
        with torch.no_grad():
            for a, b in ranges:
                clips = list(gather_tiles(frames_u8, plan, a, b, self.dtype).unbind(0))      # on the current stream, as the frames are
                if self.depth == 1:
                    parts.append(self._encode_batch(clips, counts[a:b]))
                    continue
                inflight.append(self._pipe.submit(clips, counts[a:b]))
                if len(inflight) >= self.depth:                                              # at most `depth` batches of tiles alive
                    parts.append(self._pipe.result(inflight.pop(0)))
            parts += [self._pipe.result(t) for t in inflight]
            indices = torch.cat(parts).to(torch.int32)
        return VideoTokens(indices, counts, plan.video, self.tile, self.overlap, self.patch, plan.frame_stride,
                           None if fps is None else float(fps) / plan.frame_stride, self.codebook_size, self.quantizer)

    def _check_tokens(self, tok: VideoTokens) -> TilePlan:
        if tok.codebook_size != self.codebook_size or tok.quantizer != self.quantizer:
            raise ValueError(f"tokens of a {tok.quantizer} codebook of {tok.codebook_size}, the model has {self.quantizer} of {self.codebook_size}")
        if tok.patch != self.patch:
            raise ValueError(f"tokens of patch {tok.patch}, the model's is {self.patch}")
        plan = tok.plan()                                                   # refuses a tile that is no multiple of the patch
        if len(tok.counts) != plan.n_tiles:
            raise ValueError(f"{len(tok.counts)} token counts for {plan.n_tiles} tiles")
        return plan

    @torch.no_grad()
    def _decode_layer(self, plan: TilePlan, tok: VideoTokens, indices, offsets, kt: int):
        a0, b0 = kt * plan.tiles_per_layer, (kt + 1) * plan.tiles_per_layer
        out = []
        for a, b in self._ranges(plan, tok.counts, a0, b0):
            out += self.model.decode_indices(indices[offsets[a]:offsets[b]], [plan.tile] * (b - a), tok.counts[a:b])
        return out

    def decode_video_iter(self, tok: VideoTokens, output=None) -> Iterator[Tuple[int, torch.Tensor]]:
        """(t0, frames uint8 [n,H,W,3] on the GPU) in timeline order, gap-free.  `output`: None for RGB; 'i420' | 'nv12' | 'nv21' for
        new `YUV420Frames` per range (BT.709, limited range, left-sited); or a `YUV420Frames` of the whole timeline, whose planes are
        written and of which each range is yielded as a view.  The temporal tile layers are decoded in order; a frame
        range is blended and yielded as soon as every tile that holds it is decoded, and the reconstructions of layers that hold no
        unfinished frame are dropped: memory is that of a few layers, whatever the video's length."""
        plan = self._check_tokens(tok)
        if output is not None and not isinstance(output, YUV420Frames) and output not in YUV_LAYOUTS:
            raise ValueError(f"output must be None, one of {YUV_LAYOUTS} or YUV420Frames, got {output!r}")
        if isinstance(output, YUV420Frames) and output.shape != plan.timeline:
            raise ValueError(f"output must hold the timeline {plan.timeline}, got {output.shape}")
        yield from self._decode_ranges(plan, tok, lambda a, b: output.frames(a, b) if isinstance(output, YUV420Frames) else output)

    def _decode_ranges(self, plan: TilePlan, tok: VideoTokens, out_for):
        """The streaming decode behind `decode_video_iter` and `quality`: (t0, blended frames [t0, t1)) in timeline order, with
        `out_for(t0, t1)` as the `out` of each range's `blend_tiles`.  Holds the reconstructions of a few layers and nothing else."""
        indices = tok.indices.to(self.device)
        offsets = [0]
        for k in tok.counts:
            offsets.append(offsets[-1] + k)
        per_layer, starts, n_frames = plan.tiles_per_layer, plan.origins[0], plan.timeline[0]
        live: List[Optional[torch.Tensor]] = [None] * plan.n_tiles
        first_live, done = 0, 0
        for kt in range(plan.counts[0]):
            live[kt * per_layer:(kt + 1) * per_layer] = self._decode_layer(plan, tok, indices, offsets, kt)
            upto = starts[kt + 1] if kt + 1 < plan.counts[0] else n_frames         # the next layer starts here: frames below are complete
            if upto > done:
                yield done, blend_tiles(live, plan, done, upto, out_for(done, upto))
                done = upto
            while first_live <= kt and starts[first_live] + plan.tile[0] <= done:  # every frame of the layer is out
                live[first_live * per_layer:(first_live + 1) * per_layer] = [None] * per_layer
                first_live += 1

    def decode_video(self, tok: VideoTokens, output=None):
        """uint8 [T',H,W,3] on the GPU: the ranges of `decode_video_iter`, concatenated.  With `output` (a layout name or a
        `YUV420Frames` of the timeline, as for `decode_video_iter`) the ranges are blended into the planes of one `YUV420Frames`, which
        is returned."""
        if output is None:
            return torch.cat([part for _, part in self.decode_video_iter(tok)], dim=0)
        if not isinstance(output, YUV420Frames):
            if output not in YUV_LAYOUTS:
                raise ValueError(f"output must be None, one of {YUV_LAYOUTS} or YUV420Frames, got {output!r}")
            t, h, w = tok.plan().timeline
            output = YUV420Frames.empty(t, h, w, output, self.device)
        for _ in self.decode_video_iter(tok, output):
            pass
        return output

    def quality(self, frames, tok: VideoTokens, ssim: bool = True) -> "VideoQuality":
        """What `decode_video(tok)` is worth against the video it was made from: the finished `VideoQuality` of every timeline frame
        against `frames[tok.frame_stride * t]`.  `frames` is the source, uint8 [T,H,W,3] on the GPU (decoded to RGB) or `YUV420Frames`
        (decoded into planes of the source's own layout, matrix, range and siting, compared plane by plane).  The ranges of the
        streaming decode are measured and dropped one by one: beyond the source, memory is that of a few tile layers, whatever the
        video's length; the sums stay on the GPU until one read at the end."""
        plan = self._check_tokens(tok)
        if _frames_shape(frames, "quality") != plan.video:
            raise ValueError(f"frames must be the video {plan.video} of the tokens, got {_frames_shape(frames, 'quality')}")
        yuv = isinstance(frames, YUV420Frames)
        q = VideoQuality(plan.video[1], plan.video[2], yuv420=yuv)
        for t0, part in self._decode_ranges(plan, tok, (lambda a, b: frames.like(b - a)) if yuv else (lambda a, b: None)):
            q.update(part, frames, t0, plan.frame_stride, ssim)
            del part
        return q.finish()
