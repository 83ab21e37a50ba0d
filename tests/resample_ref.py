"""Float64 restatement of ttv_clip_resample_u8 for the tests: aten's `_upsample_bicubic2d_aa` (the float path of torchvision's
`resize(..., BICUBIC, antialias=True)`), torchvision's rounding of a float result back to uint8 levels, and this repository's
normalisation `level / 127.5 - 1`.  numpy only in the arithmetic; no torch op takes part.

Along one axis, n_in -> n_out samples:
    scale = n_in / n_out;  support = 2 scale if scale >= 1 else 2;  inv = 1 / scale if scale >= 1 else 1
    output i: c = scale (i + 0.5);  lo = max(0, int(c - support + 0.5));  hi = min(int(c + support + 0.5), n_in)
    w_j = cubic((j - c + 0.5) inv), lo <= j < hi, Keys kernel with a = -0.5, divided by their sum.
Width pass, then height pass, nothing rounded in between.  A geometry is the tuple the C ABI takes per clip:
(T, Hs, Ws, Hr, Wr, oy, ox, Ho, Wo, flip): resample Hs x Ws to the virtual size Hr x Wr, keep the window Ho x Wo at (oy, ox), mirror it
along W when flip is set.
"""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple

import numpy as np

A = -0.5


def cubic(x: np.ndarray) -> np.ndarray:
    x = np.abs(np.asarray(x, dtype=np.float64))
    near = ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0
    far = (((x - 5.0) * x + 8.0) * x - 4.0) * A
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def axis_taps(n_in: int, n_out: int) -> List[Tuple[int, np.ndarray]]:
    """[(lo, normalised float64 weights of taps lo .. lo + len)] for every output index of the axis."""
    scale = n_in / n_out
    support = 2.0 * scale if scale >= 1.0 else 2.0
    inv = 1.0 / scale if scale >= 1.0 else 1.0
    out = []
    for i in range(n_out):
        c = scale * (i + 0.5)
        lo = max(0, int(c - support + 0.5))
        hi = min(int(c + support + 0.5), n_in)
        w = cubic((np.arange(lo, hi) - c + 0.5) * inv)
        out.append((lo, w / w.sum()))
    return out


def axis_matrix(n_in: int, n_out: int, first: int = 0, count: int = None) -> np.ndarray:
    """[count][n_in] float64: rows first .. first + count of the axis' resampling matrix."""
    taps = axis_taps(n_in, n_out)
    count = n_out - first if count is None else count
    m = np.zeros((count, n_in), dtype=np.float64)
    for r in range(count):
        lo, w = taps[first + r]
        m[r, lo:lo + len(w)] = w
    return m


def prerounding(frames_u8: np.ndarray, geom: Sequence[int]) -> np.ndarray:
    """frames uint8 [T][Hs][Ws][3] -> float64 [3][T][Ho][Wo] on the 0 .. 255 scale, before any rounding."""
    t, hs, ws, hr, wr, oy, ox, ho, wo, flip = (int(g) for g in geom)
    assert frames_u8.shape == (t, hs, ws, 3) and frames_u8.dtype == np.uint8
    mx = axis_matrix(ws, wr, ox, wo)                 # [Wo][Ws]
    my = axis_matrix(hs, hr, oy, ho)                 # [Ho][Hs]
    x = frames_u8.astype(np.float64)
    wide = np.einsum("thwc,xw->thxc", x, mx)         # width pass
    out = np.einsum("thxc,yh->ctyx", wide, my)       # height pass
    return out[..., ::-1].copy() if flip else out


def round_half_even(v: np.ndarray) -> np.ndarray:
    return np.rint(v)                                # numpy rounds half to even


def levels(frames_u8: np.ndarray, geom: Sequence[int]) -> np.ndarray:
    """int64 [3][T][Ho][Wo]: clamp(round_half_even(prerounding), 0, 255)."""
    return np.clip(round_half_even(prerounding(frames_u8, geom)), 0, 255).astype(np.int64)


def normalise(level: np.ndarray, dtype: str) -> np.ndarray:
    """What the kernels store for a level: fp32(fp32(level / 127.5) - 1), then one rounding to `dtype` ('f32' or 'bf16'); returned as
    float32 (bf16 values are exact in it).  The division and the subtraction are done in float64 and rounded to float32 one at a time:
    a quotient or difference of two float32 numbers rounded from float64 is the correctly rounded float32 result (double rounding is
    innocuous for these operations at 53 >= 2 * 24 + 2 bits)."""
    q = (np.asarray(level, dtype=np.float64) / 127.5).astype(np.float32)
    v = (q.astype(np.float64) - 1.0).astype(np.float32)
    if dtype == "f32":
        return v
    assert dtype == "bf16"
    u = v.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16   # round to nearest even on the upper 16 bits (no NaN / overflow in [-1, 1])
    return u.astype(np.uint32).view(np.float32)


def decode_levels(out: np.ndarray) -> np.ndarray:
    """Level a stored value stands for: round((out + 1) * 127.5).  Exact in both dtypes: levels are 1 / 127.5 = 7.8e-3 apart and a
    bf16 value in [-1, 1] is at most 2^-9 = 2.0e-3 (0.25 level) from the fp32 value it was rounded from."""
    return np.rint((np.asarray(out, dtype=np.float64) + 1.0) * 127.5).astype(np.int64)


def tie_distance(pre: np.ndarray) -> np.ndarray:
    """Distance of each pre-rounding value to the nearest half-integer (where the level decision flips)."""
    f = pre - np.floor(pre)
    return np.abs(f - 0.5)


def train_geom(t: int, hs: int, ws: int, ho: int, wo: int, flip: int = 0) -> Tuple[int, ...]:
    """Training geometry: the whole source array (= the crop box) goes to Ho x Wo."""
    return (t, hs, ws, ho, wo, 0, 0, ho, wo, flip)


def resized_hw(h: int, w: int, size: int) -> Tuple[int, int]:
    """torchvision's Resize(size=int): the shorter side becomes `size`, the longer one int(size * long / short)."""
    if h <= w:
        return size, int(size * w / h)
    return int(size * h / w), size


def eval_geom(t: int, hs: int, ws: int, ho: int, wo: int) -> Tuple[int, ...]:
    """Evaluation geometry: Resize(max(Ho, Wo)) then CenterCrop((Ho, Wo))."""
    hr, wr = resized_hw(hs, ws, max(ho, wo))
    assert hr >= ho and wr >= wo
    return (t, hs, ws, hr, wr, int(round((hr - ho) / 2.0)), int(round((wr - wo) / 2.0)), ho, wo, 0)


def noise_frames(seed: int, t: int, h: int, w: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, size=(t, h, w, 3), dtype=np.uint8)


def smooth_frames(seed: int, t: int, h: int, w: int) -> np.ndarray:
    """Low-frequency seeded content (a few sinusoids per channel, drifting over time), no overshoot-heavy edges."""
    g = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(h) / h, np.arange(w) / w, indexing="ij")
    out = np.zeros((t, h, w, 3))
    for c in range(3):
        for _ in range(3):
            fy, fx, ph, dr = g.uniform(0.5, 3.0), g.uniform(0.5, 3.0), g.uniform(0, 2 * math.pi), g.uniform(0.0, 0.3)
            for k in range(t):
                out[k, :, :, c] += np.sin(2 * math.pi * (fy * yy + fx * xx) + ph + dr * k)
    out = (out / 3.0 * 0.45 + 0.5) * 255.0
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def torch_float_path(frames_u8: np.ndarray, geom: Sequence[int]) -> np.ndarray:
    """fp32 result of torch-CPU F.interpolate(x.float(), (Hr, Wr), mode='bicubic', antialias=True) on the same geometry, window and
    flip applied: float32 [3][T][Ho][Wo], 0 .. 255 scale, unrounded.  The yardstick the tests take their tie band from."""
    import torch
    import torch.nn.functional as F
    t, hs, ws, hr, wr, oy, ox, ho, wo, flip = (int(g) for g in geom)
    x = torch.from_numpy(frames_u8).permute(0, 3, 1, 2).float()
    y = F.interpolate(x, size=(hr, wr), mode="bicubic", antialias=True, align_corners=False)
    y = y[:, :, oy:oy + ho, ox:ox + wo]
    if flip:
        y = y.flip(-1)
    return y.permute(1, 0, 2, 3).contiguous().numpy()
