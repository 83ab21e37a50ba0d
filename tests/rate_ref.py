"""numpy / Python restatement of the rate side of the whole-video path (include/titok_hip.h, `ttv_video_tile_sse_u8`;
titok_video_amd/video.py, `allocate_tokens`): the level of a reconstructed element, the per-tile sum of squared level differences on
top of `video_ref.Plan`, and both allocation rules.  Written from the definitions, not from video.py: nothing of the package is
imported here.  Sums and allocations are Python ints throughout."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from video_ref import F32  # noqa: E402


# ---- values -----------------------------------------------------------------------------------------------------------------------------
def level(v):
    """float32 array -> int64 levels: clamp to [-1, 1] (a NaN stays), t = v + 1, t = t * 127.5 (each a float32 rounding), then NaN or
    t < 0 -> 0, t >= 255 -> 255, else round half to even.  Element by element in the order the header states it."""
    v = np.ascontiguousarray(v, dtype=F32)
    out = np.empty(v.shape, dtype=np.int64)
    flat, res = v.reshape(-1), out.reshape(-1)
    for k in range(flat.size):
        q = flat[k]
        if q < F32(-1.0):
            q = F32(-1.0)
        elif q > F32(1.0):
            q = F32(1.0)
        if np.isnan(q):
            res[k] = 0
            continue
        t = F32(F32(q + F32(1.0)) * F32(127.5))
        if t < F32(0.0):
            res[k] = 0
        elif t >= F32(255.0):
            res[k] = 255
        else:
            lo = math.floor(float(t))
            frac = float(t) - lo                      # exact: t is a float32 below 256
            res[k] = lo + 1 if frac > 0.5 or (frac == 0.5 and lo % 2 == 1) else lo
    return out


def level_fast(v):
    """`level` for many elements: float32 arithmetic on whole arrays, the same steps."""
    v = np.ascontiguousarray(v, dtype=F32)
    with np.errstate(invalid="ignore"):
        q = np.where(v < F32(-1), F32(-1), np.where(v > F32(1), F32(1), v)).astype(F32)
        t = (q + F32(1.0)).astype(F32)
        t = (t * F32(127.5)).astype(F32)
        nan = np.isnan(t)
        t = np.where(nan, F32(0.0), t)
        t = np.minimum(np.maximum(t, F32(0.0)), F32(255.0))
        return np.rint(t.astype(np.float64)).astype(np.int64)


def counted(plan, index):
    """(nt, nh, nw): samples of tile `index` per axis that lie inside the timeline, min(tile, n - origin)."""
    return tuple(min(t, n - o) for t, n, o in zip(plan.tile, plan.timeline, plan.origin(index)))


def elements(plan, index):
    nt, nh, nw = counted(plan, index)
    return 3 * nt * nh * nw


def tile_sse(frames, plan, index, recon):
    """frames uint8 [T,H,W,3], recon float32 [3,Tt,Ht,Wt] of tile `index` -> the Python int
    sum over c, i < nt, y < nh, x < nw of (level(recon[c,i,y,x]) - frames[frame_stride (t0 + i), h0 + y, w0 + x, c])^2."""
    t0, h0, w0 = plan.origin(index)
    nt, nh, nw = counted(plan, index)
    recon = np.asarray(recon)
    assert recon.dtype == F32 and recon.shape == (3,) + tuple(plan.tile)
    src = frames[plan.frame_stride * (t0 + np.arange(nt))][:, h0:h0 + nh, w0:w0 + nw, :].astype(np.int64)      # [nt,nh,nw,3]
    lev = level_fast(recon[:, :nt, :nh, :nw]).transpose(1, 2, 3, 0)
    d = lev - src
    return int((d * d).sum())


def psnr(sse, n_elements):
    return math.inf if sse == 0 else 10.0 * math.log10(65025 * n_elements / sse)


# ---- allocation -------------------------------------------------------------------------------------------------------------------------
def allocate_target(ladder, sse, n_elements, target):
    """Per tile the smallest count whose PSNR is >= target; if none, the count of least sum, the smaller count on a tie."""
    out = []
    for row, e in zip(sse, n_elements):
        pick = None
        for k, v in zip(ladder, row):
            if psnr(v, e) >= target:
                pick = k
                break
        if pick is None:
            least = min(row)
            pick = ladder[row.index(least)]
        out.append(pick)
    return out


def lower_hull(ladder, row):
    """Levels of the lower convex hull of (ladder[l], row[l]) that starts at level 0, by brute force: from the current level go to the
    later level with the steepest fall per token (the farthest one among equals); stop when nothing later lies lower."""
    hull, at = [0], 0
    while True:
        best = None
        for l in range(at + 1, len(ladder)):
            drop, tokens = row[at] - row[l], ladder[l] - ladder[at]
            if drop <= 0:
                continue
            if best is None or drop * best[1] >= best[0] * tokens:           # >=: the farthest of equally steep ones
                best = (drop, tokens, l)
        if best is None:
            return hull
        at = best[2]
        hull.append(at)


def allocate_budget(ladder, sse, budget):
    n = len(sse)
    if budget < n * ladder[0]:
        raise ValueError("budget below the ladder's least count for every tile")
    hulls = [lower_hull(ladder, row) for row in sse]
    pos, left = [0] * n, budget - n * ladder[0]
    while True:
        cand = []
        for j in range(n):
            if pos[j] + 1 < len(hulls[j]):
                a, b = hulls[j][pos[j]], hulls[j][pos[j] + 1]
                if ladder[b] - ladder[a] <= left:
                    cand.append((sse[j][a] - sse[j][b], ladder[b] - ladder[a], j))
        if not cand:
            break
        best = cand[0]
        for c in cand[1:]:
            if c[0] * best[1] > best[0] * c[1]:                                # strictly steeper only: ties stay with the lower tile
                best = c
        pos[best[2]] += 1
        left -= best[1]
    counts = [ladder[hulls[j][pos[j]]] for j in range(n)]
    total = total_sse(ladder, sse, counts)
    best_uniform = None
    for k in ladder:
        if n * k <= budget:
            t = total_sse(ladder, sse, [k] * n)
            if best_uniform is None or t < best_uniform[0]:
                best_uniform = (t, k)
    if best_uniform is not None and best_uniform[0] < total:
        return [best_uniform[1]] * n
    return counts


def total_sse(ladder, sse, counts):
    return sum(row[list(ladder).index(k)] for row, k in zip(sse, counts))
