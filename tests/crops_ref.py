"""Float64 restatement of the perceptual crop operator (csrc/ttv_crops.hip, include/titok_hip.h: ttv_lpips_crops_forward / backward)
and of its transpose with the clamp mask, for the tests.

One crop: a frame [3, H, W], the reconstruction clamped to [-1, 1], resized to the virtual frame Hr x Wr by torch's bicubic rule
(align_corners=False, no antialiasing) unless (Hr, Wr) == (H, W), and the window of `size` x `size` at (oy, ox) of it.  The resize
is separable and linear, so per axis it is a matrix R [window, n_in] whose row d holds the four Keys weights (A = -0.75) of output
index o + d at the tap columns i0 - 1 .. i0 + 2 clamped to [0, n_in - 1] (clamped taps add up in one column):
    forward   out = Ry v Rx^T            backward  dx = 1[-1 <= x <= 1] * (Ry^T g Rx)
Products and sums are float64 throughout.  The taps come in three modes:
  "f32": as the kernel states them.  scale = float32(n_in) / float32(n_out); src = fmaf(scale, dst + 0.5f, -0.5f); i0 = floor(src);
         t = src - i0; the weight polynomials of cubic_taps in float32, one rounding per operation.  The fmaf is reproduced exactly:
         scale has 24 significant bits and dst + 0.5 at most 16, so their product and the sum with -0.5 are exact in float64, and the
         one rounding of .astype(float32) is the fmaf's own.  floor and src - i0 are exact in float32.
  "f32c": the same, with the polynomials as a compiler contracts them under -ffp-contract=on (a multiply that feeds an add of the
         same expression becomes one fma): c1(x) = fma(fma(A + 2, x, -(A + 3)) * x, x, 1), c2(x) = fma(fma(fma(A, x, -5 A), x, 8 A),
         x, -4 A).  `fma32` is exact: the product of two float32 is exact in float64, the float64 sum with c is rounded once
         (TwoSum gives its error), and the cast to float32 can only differ from the single rounding of the exact value when the
         float64 sum sits exactly on a float32 midpoint - there the sign of the TwoSum error decides.
         Which of the two a build uses is the compiler's choice, made once per call site; the GPU tests accept either, whole
         array by whole array, and add no slack for it.
  "f64": scale, src, t and the polynomials in float64: the definition torch's float64 kernels evaluate.
Besides R, `axis` returns A (the sum of |weight| per column) and N (the number of taps per column): the tests' bounds are built from
them.  A frame that is not resized has R = A = N = the window's selection matrix.
"""
from __future__ import annotations

import numpy as np

A_KEYS = -0.75
U32 = 2.0 ** -24          # unit roundoff of float32

# |w_computed - w_exact| for one Keys weight evaluated in float32 from an exact t, contracted or not (a contraction only removes
# roundings).  c2 on [1, 2]: s1 = A x - 5 A in [2.25, 3] (|A x| <= 1.5: 1.5 u, then 3 u), s2 = s1 x + 8 A (|s1 x| <= 4.5: 4.5 u,
# |s2| <= 3: 3 u), s3 = s2 x - 4 A (|s2 x| <= 6: 6 u, |s3| <= 1: u); an error of s1 reaches s3 times x^2 <= 4, one of s2 times
# x <= 2: 4 * 4.5 + 2 * 7.5 + 7 = 40 u.  c1 on [0, 1] and the arguments t + 1, 1 - t, 2 - t (one rounding each, <= 2 u, times
# |c'| <= 3) stay below that: 40 u + 6 u.  Used by the CPU test that compares the float32 modes with the float64 one only.
POLY_EPS = 46.0 * U32


def fma32(a, b, c):
    """fmaf(a, b, c) for float32 arrays, exactly (see the module docstring)."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b                                  # exact
    r = p + c
    bb = r - p
    e = (p - (r - bb)) + (c - bb)              # TwoSum: p + c = r + e exactly
    r32 = r.astype(np.float32)
    d = r - r32.astype(np.float64)             # exact
    other = np.nextafter(r32, np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    tie = (d != 0) & (np.abs(d) == np.abs(other.astype(np.float64) - r))
    move = tie & (np.sign(e) == np.sign(d))
    return np.where(move, other, r32).astype(np.float32)


def resized_hw(H, W, size):
    """torchvision resize(size=int): the short edge becomes `size`, the long edge int(size * long / short)."""
    short, long = (W, H) if W <= H else (H, W)
    new_short, new_long = size, int(size * long / short)
    return (new_long, new_short) if W <= H else (new_short, new_long)


def taps(n_in, n_out, mode="f32"):
    """(idx [n_out, 4] int64, w [n_out, 4] float64) of every output index of the axis."""
    dst = np.arange(n_out)
    if mode in ("f32", "f32c"):
        f = np.float32
        scale = f(n_in) / f(n_out)
        src = (np.float64(scale) * (dst.astype(np.float64) + 0.5) - 0.5).astype(f)       # == fmaf(scale, dst + 0.5f, -0.5f)
        fl = np.floor(src)
        t = (src - fl).astype(f)
        A = f(A_KEYS)

        if mode == "f32":
            def c1(x):
                return ((A + f(2)) * x - (A + f(3))) * x * x + f(1)

            def c2(x):
                return ((A * x - f(5) * A) * x + f(8) * A) * x - f(4) * A
        else:
            def c1(x):
                return fma32(fma32(A + f(2), x, -(A + f(3))) * x, x, f(1))

            def c2(x):
                return fma32(fma32(fma32(A, x, -(f(5) * A)), x, f(8) * A), x, -(f(4) * A))

        w = np.stack([c2(t + f(1)), c1(t), c1(f(1) - t), c2(f(2) - t)], axis=1)
        assert w.dtype == np.float32
        w = w.astype(np.float64)
    elif mode == "f64":
        scale = n_in / n_out
        src = scale * (dst + 0.5) - 0.5
        fl = np.floor(src)
        t = src - fl
        A = A_KEYS

        def c1(x):
            return ((A + 2) * x - (A + 3)) * x * x + 1

        def c2(x):
            return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A

        w = np.stack([c2(t + 1), c1(t), c1(1 - t), c2(2 - t)], axis=1)
    else:
        raise ValueError(mode)
    i0 = fl.astype(np.int64)
    idx = np.clip(i0[:, None] + np.arange(-1, 3)[None, :], 0, n_in - 1)
    return idx, w


def axis(n_in, n_out, o, length, mode="f32"):
    """R, A, N [length, n_in] of the outputs o .. o + length - 1 of the axis n_in -> n_out (see the module docstring)."""
    R = np.zeros((length, n_in))
    Aw = np.zeros((length, n_in))
    N = np.zeros((length, n_in))
    if n_in == n_out:
        d = np.arange(length)
        R[d, o + d] = Aw[d, o + d] = N[d, o + d] = 1.0
        return R, Aw, N
    idx, w = taps(n_in, n_out, mode)
    for d in range(length):
        for k in range(4):
            R[d, idx[o + d, k]] += w[o + d, k]
            Aw[d, idx[o + d, k]] += abs(w[o + d, k])
            N[d, idx[o + d, k]] += 1.0
    return R, Aw, N


def operators(geom, size, mode="f32", window=None):
    """((Ry, Ay, Ny), (Rx, Ax, Nx)) of a crop geom = (H, W, Hr, Wr, oy, ox).  `window` = (rows, columns) other than size x size."""
    H, W, Hr, Wr, oy, ox = geom
    rows, cols = (size, size) if window is None else window
    if (Hr, Wr) == (H, W):                 # not resized: both axes select
        return axis(H, H, oy, rows, mode), axis(W, W, ox, cols, mode)
    # resized: both axes go through the taps, also one whose length does not change
    ys = _resized_axis(H, Hr, oy, rows, mode)
    xs = _resized_axis(W, Wr, ox, cols, mode)
    return ys, xs


def _resized_axis(n_in, n_out, o, length, mode):
    if n_in != n_out:
        return axis(n_in, n_out, o, length, mode)
    # scale 1: src = dst exactly, t = 0, weights (0, 1, 0, 0) exactly in every mode - the selection, with four taps counted
    R, Aw, N = axis(n_in, n_in, o, length, mode)
    return R, Aw, 4.0 * N


def clamp(v):
    return np.minimum(np.maximum(v, -1.0), 1.0)


def forward(frame, geom, size, clamped, mode="f32", window=None):
    """(out [3, rows, cols], S, Sw) float64.  frame [3, H, W] float64; S = sum |wy| |wx| |v| and Sw = sum (|wy| + |wx|) |v| over the
    taps of each output element (what an error of the accumulation, resp. of the weights, scales with)."""
    v = clamp(frame) if clamped else frame
    (Ry, Ay, Ny), (Rx, Ax, Nx) = operators(geom, size, mode, window)
    out = Ry @ v @ Rx.T
    av = np.abs(v)
    S = Ay @ av @ Ax.T
    Sw = Ay @ av @ Nx.T + Ny @ av @ Ax.T
    return out, S, Sw


def backward(g, frame, geom, size, mode="f32", window=None):
    """(dx [3, H, W], S, Sw, n) float64: dx = 1[-1 <= x <= 1] (Ry^T g Rx) for the reconstruction frame x; S and Sw as in `forward`
    over the gathered terms; n [H, W] = the number of fmaf steps of the gather at that pixel (row taps + column taps)."""
    (Ry, Ay, Ny), (Rx, Ax, Nx) = operators(geom, size, mode, window)
    mask = ((frame >= -1.0) & (frame <= 1.0)).astype(np.float64)
    dx = mask * (Ry.T @ g @ Rx)
    ag = np.abs(g)
    S = Ay.T @ ag @ Ax
    Sw = Ay.T @ ag @ Nx + Ny.T @ ag @ Ax
    n = Ny.sum(0)[:, None] + Nx.sum(0)[None, :]
    return dx, S, Sw, n


def touched(geom, size, mode="f32"):
    """[H, W] bool: the pixels some tap of the window touches (the footprint)."""
    (_Ry, _Ay, Ny), (_Rx, _Ax, Nx) = operators(geom, size, mode)
    return (Ny.sum(0)[:, None] > 0) & (Nx.sum(0)[None, :] > 0)


def half_ulp(v, dtype):
    """Half a unit in the last place of `dtype` ("bf16": 8 significant bits, "f32": 24) at |v|, elementwise; normal range."""
    bits = {"bf16": 8, "f32": 24}[dtype]
    a = np.maximum(np.abs(v), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - bits)


def gamma(n):
    """Higham's gamma_n for float32: the relative error bound of a chain of n roundings."""
    return n * U32 / (1.0 - n * U32)


def plan_table(frame_owner, plan):
    """Rows (clip, frame, H, W, Hr, Wr, oy, ox) of a perceptual_crop_plan over frames whose (clip, frame) is frame_owner[k]."""
    return [tuple(frame_owner[k]) + (H, W, Hr, Wr, oy, ox) for k, H, W, Hr, Wr, oy, ox, _r in plan]
