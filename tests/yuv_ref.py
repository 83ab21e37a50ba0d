"""numpy restatement of the Y'CbCr 4:2:0 side of the whole-video path (include/titok_hip.h, "Y'CbCr 4:2:0 frames in and out"): the
integer coefficients, the chroma upsampling, the source pixel N and its level, the value `ttv_video_tiles_yuv420` stores, and the planes
`ttv_video_blend_yuv420` makes of blended RGB levels.  Integers (int64) all the way; only the gather's last division and subtraction are
`np.float32`.  Written from the definitions: nothing of the package is imported here; the tile geometry is tests/video_ref.py's."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import video_ref as VR  # noqa: E402

F32 = np.float32
N_MAX = 255 * 65536
K10000 = {"bt601": (2990, 1140), "bt709": (2126, 722)}        # (Kr, Kb) in 1 / 10000


def rhu(num, den):
    """round-half-up of num / den for positive integers."""
    return (2 * num + den) // (2 * den)


class Coef:
    """The integer coefficients of one (matrix, range), by integer arithmetic on Kr, Kb in 1/10000 and the scales as fractions."""

    def __init__(self, matrix, rng):
        kr, kb = K10000[matrix]
        kg = 10000 - kr - kb
        lim = rng == "limited"
        assert rng in ("limited", "full")
        syn, syd = (255, 219) if lim else (1, 1)               # sy = syn / syd, ys = syd / syn
        scn, scd = (255, 224) if lim else (1, 1)               # sc = scn / scd, cs = scd / scn
        self.y0 = 16 if lim else 0
        self.ky = rhu(syn * 4096, syd)
        self.rv = rhu(2 * (10000 - kr) * scn * 4096, 10000 * scd)
        self.bu = rhu(2 * (10000 - kb) * scn * 4096, 10000 * scd)
        self.gu = -rhu(2 * (10000 - kb) * kb * scn * 4096, 10000 * kg * scd)
        self.gv = -rhu(2 * (10000 - kr) * kr * scn * 4096, 10000 * kg * scd)
        self.ytot = rhu(syd * 65536, syn)
        self.yr = rhu(kr * syd * 65536, 10000 * syn)
        self.yb = rhu(kb * syd * 65536, 10000 * syn)
        self.yg = self.ytot - self.yr - self.yb
        self.ub = self.vr = rhu(scd * 32768, scn)
        self.ur = -rhu(kr * scd * 65536, 2 * (10000 - kb) * scn)
        self.ug = -(self.ur + self.ub)
        self.vb = -rhu(kb * scd * 65536, 2 * (10000 - kr) * scn)
        self.vg = -(self.vr + self.vb)
        self.y_clip = (16, 235) if lim else (0, 255)
        self.c_clip = (16, 240) if lim else (0, 255)

    def to_rgb(self):
        return (self.ky, self.rv, self.gu, self.gv, self.bu)

    def from_rgb(self):
        return ((self.yr, self.yg, self.yb), (self.ur, self.ug, self.ub), (self.vr, self.vg, self.vb))


# ---- upsampling -------------------------------------------------------------------------------------------------------------------------
def taps(p, n, center):
    """For luma positions p (int array) of an axis whose chroma plane has n samples: (a, b, wa, wb), the two chroma indices, clamped,
    and their weights (sum 4)."""
    p = np.asarray(p, dtype=np.int64)
    j, odd = p >> 1, (p & 1) == 1
    if center:
        a, b = np.where(odd, j, j - 1), np.where(odd, j + 1, j)
        wa, wb = np.where(odd, 3, 1), np.where(odd, 1, 3)
    else:
        a, b = j, np.where(odd, j + 1, j)
        wa, wb = np.where(odd, 2, 4), np.where(odd, 2, 0)
    return np.clip(a, 0, n - 1), np.clip(b, 0, n - 1), wa.astype(np.int64), wb.astype(np.int64)


def chroma16(plane, ys, xs, siting):
    """C16 [len(ys), len(xs)] of one chroma plane [Hc,Wc] at the luma positions ys x xs: rows always by the centred rule."""
    c = np.asarray(plane).astype(np.int64)
    ra, rb, wra, wrb = taps(ys, c.shape[0], True)
    ca, cb, wca, wcb = taps(xs, c.shape[1], siting == "center")
    rows = wra[:, None] * c[ra] + wrb[:, None] * c[rb]                                   # [len(ys), Wc]
    return rows[:, ca] * wca[None, :] + rows[:, cb] * wcb[None, :]


# ---- source pixel -----------------------------------------------------------------------------------------------------------------------
def n_unclamped(k, Y, U16, V16):
    Y, U16, V16 = (np.asarray(a).astype(np.int64) for a in (Y, U16, V16))
    yc, u, v = 16 * k.ky * (Y - k.y0), U16 - 2048, V16 - 2048
    return np.stack([yc + k.rv * v, yc + k.gu * u + k.gv * v, yc + k.bu * u], axis=-1)


def n_of(k, Y, U16, V16):
    return np.clip(n_unclamped(k, Y, U16, V16), 0, N_MAX)


def source_n(y, u, v, ys, xs, k, siting):
    """N [len(ys), len(xs), 3] of one frame (y [H,W], u and v [Hc,Wc]) at the pixels ys x xs."""
    ys, xs = np.asarray(ys, dtype=np.int64), np.asarray(xs, dtype=np.int64)
    return n_of(k, np.asarray(y)[ys[:, None], xs[None, :]], chroma16(u, ys, xs, siting), chroma16(v, ys, xs, siting))


def level_of_n(n):
    return (np.asarray(n, dtype=np.int64) + 32768) >> 16


def unit_from_n(n, dtype):
    """float(N) / 8355840 - 1 in float32 (one division, one subtraction), rounded once to `dtype`."""
    q = np.asarray(n).astype(F32) / F32(8355840.0)
    assert q.dtype == F32
    return VR.to_dtype(q - F32(1.0), dtype)


def source_levels(y, u, v, matrix, rng, siting):
    """uint8 [T,H,W,3]: the source level of every pixel of a video (y [T,H,W], u and v [T,Hc,Wc])."""
    k = Coef(matrix, rng)
    T, H, W = y.shape
    out = np.empty((T, H, W, 3), dtype=np.uint8)
    for t in range(T):
        out[t] = level_of_n(source_n(y[t], u[t], v[t], np.arange(H), np.arange(W), k, siting))
    return out


def gather(y, u, v, plan, begin, end, dtype, matrix, rng, siting):
    """float32 [end - begin, 3, Tt, Ht, Wt]: element (c, i, y, x) of the tile at (t0, h0, w0) is unit_from_n of the pixel
    (frame_stride * min(t0 + i, T' - 1), min(h0 + y, H - 1), min(w0 + x, W - 1)); the chroma rule sees the clamped coordinates."""
    k = Coef(matrix, rng)
    Tn, H, W = plan.timeline
    Tt, Ht, Wt = plan.tile
    out = np.empty((end - begin, 3, Tt, Ht, Wt), dtype=F32)
    for j in range(begin, end):
        t0, h0, w0 = plan.origin(j)
        yi = np.minimum(h0 + np.arange(Ht), H - 1)
        xi = np.minimum(w0 + np.arange(Wt), W - 1)
        for i in range(Tt):
            t = plan.frame_stride * min(t0 + i, Tn - 1)
            out[j - begin, :, i] = unit_from_n(source_n(y[t], u[t], v[t], yi, xi, k, siting), dtype).transpose(2, 0, 1)
    return out


# ---- RGB levels -> planes ---------------------------------------------------------------------------------------------------------------
def planes_from_levels(levels, matrix, rng, siting):
    """levels uint8 [T,H,W,3] -> (y [T,H,W], u [T,Hc,Wc], v [T,Hc,Wc]) uint8."""
    k = Coef(matrix, rng)
    L = np.asarray(levels).astype(np.int64)
    T, H, W, _ = L.shape
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    (yr, yg, yb), cu, cv = k.from_rgb()
    Y = k.y0 + ((yr * L[..., 0] + yg * L[..., 1] + yb * L[..., 2] + 32768) >> 16)
    r0, r1 = np.minimum(2 * np.arange(Hc), H - 1), np.minimum(2 * np.arange(Hc) + 1, H - 1)
    rows = L[:, r0] + L[:, r1]                                                          # [T,Hc,W,3]
    i2 = 2 * np.arange(Wc)
    if siting == "center":
        S, D = rows[:, :, np.minimum(i2, W - 1)] + rows[:, :, np.minimum(i2 + 1, W - 1)], 4
    else:
        S = rows[:, :, np.clip(i2 - 1, 0, W - 1)] + 2 * rows[:, :, np.minimum(i2, W - 1)] + rows[:, :, np.minimum(i2 + 1, W - 1)]
        D = 8
    out = []
    for a, b, c in (cu, cv):
        num = a * S[..., 0] + b * S[..., 1] + c * S[..., 2] + D * 32768
        out.append(128 + num // (D * 65536))                                            # floor division, also of negatives
    return (np.clip(Y, *k.y_clip).astype(np.uint8), np.clip(out[0], *k.c_clip).astype(np.uint8),
            np.clip(out[1], *k.c_clip).astype(np.uint8)), (out[0], out[1])
