"""numpy restatement of the whole-video path (include/titok_hip.h, "whole videos"; titok_video_amd/video.py): the tile plan, the value
`ttv_video_tiles_u8` stores, the blend of `ttv_video_blend_u8` in float32 arithmetic step by step, and the bit packing of the token
container.  Written from the definitions, not from video.py: nothing of the package is imported here.

Tiles are float32 arrays whatever the dtype under test: a bf16 tile holds values that bf16 represents exactly (`to_dtype`)."""
import json
import struct

import numpy as np

F32 = np.float32


# ---- plan -------------------------------------------------------------------------------------------------------------------------------
def axis_plan(n, tile, overlap, patch):
    """(effective tile, origins) of one axis of length n."""
    if n < tile:
        return -(-n // patch) * patch, [0]
    stride = tile - overlap
    m = -(-(n - tile) // stride) + 1
    return tile, [k * stride for k in range(m - 1)] + [n - tile]


class Plan:
    def __init__(self, video, tile, overlap, patch, frame_stride=1):
        self.video, self.overlap, self.frame_stride = tuple(video), tuple(overlap), frame_stride
        self.timeline = (-(-video[0] // frame_stride), video[1], video[2])
        axes = [axis_plan(n, t, o, p) for n, t, o, p in zip(self.timeline, tile, overlap, patch)]
        self.tile = tuple(a[0] for a in axes)
        self.origins = [a[1] for a in axes]
        self.counts = tuple(len(o) for o in self.origins)
        self.n_tiles = self.counts[0] * self.counts[1] * self.counts[2]

    def origin(self, index):
        kt, r = divmod(index, self.counts[1] * self.counts[2])
        kh, kw = divmod(r, self.counts[2])
        return self.origins[0][kt], self.origins[1][kh], self.origins[2][kw]

    def weights(self, axis):
        t, o = self.tile[axis], self.overlap[axis]
        return np.array([min(u + 1, t - u, o + 1) for u in range(t)], dtype=np.int64)


# ---- values -----------------------------------------------------------------------------------------------------------------------------
def to_dtype(x, dtype):
    """One rounding of float32 values to `dtype` ('f32' or 'bf16', round to nearest even), returned as float32."""
    x = np.ascontiguousarray(x, dtype=F32)
    if dtype == "f32":
        return x
    assert dtype == "bf16" and not np.isnan(x).any()
    u = x.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(F32).reshape(x.shape)


def unit_from_u8(levels, dtype):
    """u8 / 127.5 - 1 in float32 (one division, one subtraction), rounded once to `dtype`."""
    q = np.asarray(levels).astype(F32) / F32(127.5)
    return to_dtype(q - F32(1.0), dtype)


def gather(frames, plan, begin, end, dtype):
    """frames uint8 [T,H,W,3] -> float32 [end - begin, 3, Tt, Ht, Wt]: element (c, i, y, x) of the tile at (t0, h0, w0) is the pixel
    (frame_stride * min(t0 + i, T' - 1), min(h0 + y, H - 1), min(w0 + x, W - 1), c)."""
    Tn, H, W = plan.timeline
    Tt, Ht, Wt = plan.tile
    out = np.empty((end - begin, 3, Tt, Ht, Wt), dtype=F32)
    for k in range(begin, end):
        t0, h0, w0 = plan.origin(k)
        ti = plan.frame_stride * np.minimum(t0 + np.arange(Tt), Tn - 1)
        yi = np.minimum(h0 + np.arange(Ht), H - 1)
        xi = np.minimum(w0 + np.arange(Wt), W - 1)
        px = frames[ti[:, None, None], yi[None, :, None], xi[None, None, :]]            # [Tt,Ht,Wt,3]
        out[k - begin] = unit_from_u8(px, dtype).transpose(3, 0, 1, 2)
    return out


def clamp(x):
    """torch's clamp(-1, 1): a NaN stays a NaN."""
    with np.errstate(invalid="ignore"):
        return np.where(x < F32(-1), F32(-1), np.where(x > F32(1), F32(1), x)).astype(F32)


def levels_of(q):
    """t = q + 1; t = t * 127.5 (float32, each rounded); round half to even; t < 0 -> 0, t >= 255 -> 255, NaN -> 0."""
    assert q.dtype == F32
    with np.errstate(invalid="ignore"):
        t = q + F32(1.0)
        t = t * F32(127.5)
        assert t.dtype == F32
        t = np.where(t >= 0, t, F32(0.0))               # negatives and NaN
        t = np.minimum(t, F32(255.0))
        return np.rint(t).astype(np.uint8)


def blend(tiles, plan, t0=0, t1=None):
    """tiles: per tile index a float32 [3,Tt,Ht,Wt] or None -> uint8 [t1 - t0, H, W, 3].  Tiles are visited in ascending index, so every
    element's sum runs in ascending index of the tiles that cover it."""
    Tn, H, W = plan.timeline
    t1 = Tn if t1 is None else t1
    Tt, Ht, Wt = plan.tile
    wt, wh, ww = plan.weights(0), plan.weights(1), plan.weights(2)
    n = t1 - t0
    num = np.zeros((n, H, W, 3), dtype=F32)
    only = np.zeros((n, H, W, 3), dtype=F32)
    den = np.zeros((n, H, W), dtype=np.int64)
    cnt = np.zeros((n, H, W), dtype=np.int64)
    for k in range(plan.n_tiles):
        a0, h0, w0 = plan.origin(k)
        ta, tb = max(a0, t0), min(a0 + Tt, Tn, t1)
        hb, wb = min(h0 + Ht, H), min(w0 + Wt, W)
        if ta >= tb:
            continue
        assert tiles[k] is not None, f"tile {k} covers frames [{t0}, {t1}) and is missing"
        tile = np.asarray(tiles[k])
        assert tile.dtype == F32 and tile.shape == (3, Tt, Ht, Wt)
        v = clamp(tile[:, ta - a0:tb - a0, :hb - h0, :wb - w0]).transpose(1, 2, 3, 0)
        w = wt[ta - a0:tb - a0, None, None] * wh[None, :hb - h0, None] * ww[None, None, :wb - w0]
        region = (slice(ta - t0, tb - t0), slice(h0, hb), slice(w0, wb))
        with np.errstate(invalid="ignore"):
            prod = w.astype(F32)[..., None] * v
            assert prod.dtype == F32
            num[region] = num[region] + prod
        only[region] = v
        den[region] += w
        cnt[region] += 1
    assert (cnt >= 1).all()
    with np.errstate(invalid="ignore"):
        q = np.where((cnt == 1)[..., None], only, num / den.astype(F32)[..., None]).astype(F32)
    return levels_of(q)


# ---- container --------------------------------------------------------------------------------------------------------------------------
MAGIC = b"TTVTOK\r\n"


def index_bits(codebook_size):
    b = 1
    while (1 << b) < codebook_size:
        b += 1
    return b


def pack(indices, bits):
    """Index i in bits [i * bits, (i + 1) * bits) of one little-endian integer."""
    acc = 0
    for i, v in enumerate(indices):
        assert 0 <= int(v) < (1 << bits)
        acc |= int(v) << (i * bits)
    return acc.to_bytes((len(indices) * bits + 7) // 8, "little")


def unpack(data, n, bits):
    acc = int.from_bytes(data, "little")
    return [(acc >> (i * bits)) & ((1 << bits) - 1) for i in range(n)]


def parse_container(data):
    """(header dict, indices) of a token stream: magic, version uint32, header length uint32, JSON header, packed indices."""
    assert data[:8] == MAGIC
    version, hlen = struct.unpack("<II", data[8:16])
    assert version == 1
    header = json.loads(data[16:16 + hlen].decode("utf-8"))
    return header, unpack(data[16 + hlen:], header["n_indices"], header["bits"])
