"""numpy restatement of what csrc/ttv_vq_train.hip computes for the L2 quantiser's training pieces (include/titok_hip.h states the
values): the commitment loss and its gradient in float64, the per-entry statistics in float32 with the kernel's order (np.add.at adds
the rows of an entry one after the other in ascending row order), the EMA update in float32 with the kernel's operation sequence and
in float64, the fixed-order reductions, and the restart draw (Philox4x32-10 of tests/gp_noise_ref.py).
Not a test module: tests/test_vq_train_cpu.py and tests/test_hip_vq_train.py import it."""
import numpy as np

try:
    from gp_noise_ref import philox4x32_10
except ImportError:                       # imported as a package member
    from .gp_noise_ref import philox4x32_10

U = 2.0 ** -24                            # unit roundoff of float32
F = np.float32


# ---- commitment term ------------------------------------------------------------------------------------------------------------------
def commit_loss(z, e):
    """mean (z - e)^2 over rows and C, float64."""
    d = np.asarray(z, np.float64) - np.asarray(e, np.float64)
    return float((d * d).mean())


def commit_grad(g, z, e, beta):
    """g + beta 2 (z - e) / (rows C), float64."""
    z = np.asarray(z, np.float64)
    return np.asarray(g, np.float64) + (2.0 * beta / z.size) * (z - np.asarray(e, np.float64))


def commit_loss_depth(rows, c):
    """Rounding steps on the longest path of the kernel's sum: the difference and the fmaf of an element count 3 relative to its own
    square (2 for d^2 from a rounded d, 1 for the fmaf), then one per further addition on the path: a thread folds
    ceil(64 c / 256) elements, 8 tree levels, the finishing block folds ceil(P / 256) partials and 8 levels; the scaling is 2: the
    factor (float)(1 / (rows c)) is itself rounded, and so is the product."""
    p = -(-rows // 64)
    return 3 + (-(-64 * c // 256)) + 8 + (-(-p // 256)) + 8 + 2


# ---- statistics -----------------------------------------------------------------------------------------------------------------------
def stats_f32(z32, idx, n):
    """count [n] int64, sum [n, C] float32: rows added in ascending row order in float32, starting from 0."""
    z32 = np.asarray(z32, F)
    idx = np.asarray(idx, np.int64)
    s = np.zeros((n, z32.shape[1]), F)
    np.add.at(s, idx, z32)
    return np.bincount(idx, minlength=n).astype(np.int64), s


def stats_f64(z, idx, n):
    s = np.zeros((n, np.asarray(z).shape[1]), np.float64)
    np.add.at(s, np.asarray(idx, np.int64), np.asarray(z, np.float64))
    return s


def draw(seed, step, n, world, rows):
    """(rank [n], row [n]) of the restart candidates: words 0 and 1 of Philox4x32-10 on counter (entry, 0, step low, step high) under
    key (seed low, seed high); word 0 % world names the rank, word 1 % rows that rank's row."""
    ent = np.arange(n, dtype=np.uint64)
    ctr = [ent, np.zeros(n, np.uint64), np.full(n, step & 0xFFFFFFFF, np.uint64), np.full(n, (step >> 32) & 0xFFFFFFFF, np.uint64)]
    w = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return (w[0] % np.uint32(world)).astype(np.int64), (w[1] % np.uint32(rows)).astype(np.int64)


def candidates(z32, cluster_size, t, seed, step, rank=0, world=1):
    """cand [n, C] float32 of one rank: the drawn row of z for entries with cluster_size < t that the draw gives to this rank, else 0."""
    z32 = np.asarray(z32, F)
    n = len(cluster_size)
    rk, row = draw(seed, step, n, world, z32.shape[0])
    cand = np.zeros((n, z32.shape[1]), F)
    pick = (np.asarray(cluster_size, F) < F(t)) & (rk == rank)
    cand[pick] = z32[row[pick]]
    return cand


def flat_stats(count, s, cand):
    """The buffer the ranks all-reduce: count | sum | cand, float32 [n (2 C + 1)]."""
    return np.concatenate([np.asarray(count, F).reshape(-1), np.asarray(s, F).reshape(-1), np.asarray(cand, F).reshape(-1)])


# ---- update ---------------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf in float32: the product of two float32 is exact in float64; the sum is rounded to float64 and then to float32, which differs
    from the single rounding of fmaf only when the float64 sum lands within 2^-53 relative of a float32 tie."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def tree_sum_f32(v, width):
    """The kernels' block sum: thread t of `width` folds v[t], v[t + width], .. in order, then the threads meet by halves."""
    v = np.asarray(v, F)
    pad = (-len(v)) % width
    m = np.concatenate([v, np.zeros(pad, F)]).reshape(-1, width)
    acc = np.zeros(width, F)
    for row in m:
        acc = (acc + row).astype(F)
    s = width // 2
    while s > 0:
        acc[:s] = (acc[:s] + acc[s:2 * s]).astype(F)
        s //= 2
    return F(acc[0])


def update_f32(cluster_size, embed_avg, count, s, cand, decay, eps, t):
    """The update in float32 with the kernel's operation sequence.  Returns (cluster_size, embed_avg, codebook, dead, total, smoothed)."""
    d, m, eps, t = F(decay), F(1.0 - float(decay)), F(eps), F(t)
    cs0, ea0 = np.asarray(cluster_size, F), np.asarray(embed_avg, F)
    n = len(cs0)
    dead = cs0 < t
    cs = np.where(dead, t, fma32(d, cs0, (m * np.asarray(count, F)).astype(F))).astype(F)
    total = tree_sum_f32(cs, 1024)
    ea = fma32(d, ea0, (m * np.asarray(s, F)).astype(F))
    denom = F(fma32(F(n), eps, total))
    smoothed = (((cs + eps).astype(F) / denom).astype(F) * total).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        cb = (ea / smoothed[:, None]).astype(F)
    cand = np.asarray(cand, F)
    ea = np.where(dead[:, None], (t * cand).astype(F), ea).astype(F)
    cb = np.where(dead[:, None], cand, cb).astype(F)
    return cs, ea, cb, dead, total, smoothed


def update_f64(cluster_size, embed_avg, count, s, cand, decay, eps, t):
    """The same update in float64, on the float32 values of decay, 1 - decay, eps and t that the kernel receives."""
    d, m, eps, t = (float(F(v)) for v in (decay, 1.0 - float(decay), eps, t))
    cs0, ea0 = np.asarray(cluster_size, np.float64), np.asarray(embed_avg, np.float64)
    n = len(cs0)
    dead = cs0 < t
    cs = np.where(dead, t, d * cs0 + m * np.asarray(count, np.float64))
    total = float(cs.sum())
    ea = d * ea0 + m * np.asarray(s, np.float64)
    smoothed = (cs + eps) / (total + n * eps) * total
    with np.errstate(divide="ignore", invalid="ignore"):
        cb = ea / smoothed[:, None]
    cand = np.asarray(cand, np.float64)
    ea = np.where(dead[:, None], t * cand, ea)
    cb = np.where(dead[:, None], cand, cb)
    return cs, ea, cb, dead, total, smoothed


def update_bounds(cluster_size, embed_avg, count, s, decay, eps, t):
    """Bounds of |float32 update - float64 update| counted from the rounding steps (u = 2^-24), for live entries:
      cluster_size: the product m count and the fmaf: 2 roundings of terms bounded by a = |d cs| + |m count|            -> 2 u a
      embed_avg:    likewise with b = |d ea| + |m sum|                                                                   -> 2 u b
      total:        n terms each off by <= 2 u a_n, summed in float32 (at most n additions on a path: n u sum|cs|)       -> 2 u sum a + n u sum cs
      smoothed:     cs + eps (1), fmaf(n, eps, total) (1), the division (1), the product (1) = 4 roundings, plus the relative
                    errors carried in: cs (2 u a / (cs + eps)), total twice (once in the denominator, once in the product)
      codebook:     ea / smoothed: the division (1) plus the carried errors of ea (absolute) and smoothed (relative).
    Second-order terms are covered by the factor 1.01.  Returns (b_cs, b_ea, b_total, rel_smoothed, b_cb)."""
    d, m, eps, t = (float(F(v)) for v in (decay, 1.0 - float(decay), eps, t))
    cs0, ea0 = np.asarray(cluster_size, np.float64), np.asarray(embed_avg, np.float64)
    n = len(cs0)
    cs, ea, cb, dead, total, smoothed = update_f64(cluster_size, embed_avg, count, s, np.zeros_like(ea0), decay, eps, t)
    a = np.where(dead, 0.0, np.abs(d * cs0) + np.abs(m * np.asarray(count, np.float64)))
    b = np.abs(d * ea0) + np.abs(m * np.asarray(s, np.float64))
    b_cs, b_ea = 2 * U * a, 2 * U * b
    b_total = 2 * U * a.sum() + n * U * np.abs(cs).sum()
    rel_total = b_total / total
    rel_sm = 4 * U + b_cs / (cs + eps) + 2 * rel_total
    with np.errstate(divide="ignore", invalid="ignore"):
        b_cb = b_ea / smoothed[:, None] + np.abs(cb) * (rel_sm[:, None] + U)
    return 1.01 * b_cs, 1.01 * b_ea, 1.01 * b_total, 1.01 * rel_sm, 1.01 * b_cb
