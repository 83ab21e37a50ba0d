"""Inputs of the per-op deterministic-mode tests, and the float64 terms every destination sums (no GPU needed).

tests/test_hip_deterministic.py runs the ops on these inputs; tests/test_deterministic_cases_cpu.py checks what that test rests on.

Every destination of an op is a sum of n terms.  The inputs are built so that the order of the sum matters: the magnitudes of a
destination's terms walk 2^-10 .. 2^10 (about 2^20 between the smallest and the largest) and their signs are mixed, so two orders of
the same fp32 sum differ in their last bits.  Where a term is a product with a derived factor (a normalised row, the chain's h) that
factor is held near one - inputs of magnitude 2^-0.5 .. 2^0.5 - and may take a few powers of two off the range: at least 2^16 stays.  All values are bf16 numbers, so the bf16 and the fp32 run of an op read the same inputs.

A case is a dict: the op's inputs (torch tensors on the CPU, float32 holding bf16 numbers), and "terms": float64 [n, destinations]
(zero where a term does not belong to a destination, with "count" [destinations] the number of terms that do).  The bound the GPU
test holds a destination to is n * 2^-24 * sum |term| around the float64 sum of its terms: n - 1 additions of relative error 2^-24
each act on partial sums no larger than sum |term| - the classical bound of ANY summation order in fp32 (Higham, Accuracy and
Stability of Numerical Algorithms, 4.2) - and the last of the n covers the rounding of the terms themselves.
"""
import numpy as np
import torch

EPS = 1e-5
U = 2.0 ** -24


def bf16(t):
    return t.to(torch.bfloat16).float()


def spread(rows, cols, seed, per_row=False):
    """sign * 2^u, bf16: per column (or for the whole row) u is a seeded permutation of linspace(-10, 10, rows); signs are drawn."""
    g = torch.Generator().manual_seed(seed)
    u = torch.linspace(-10.0, 10.0, rows, dtype=torch.float64)
    if per_row:
        e = u[torch.randperm(rows, generator=g)][:, None].expand(rows, cols)
    else:
        e = torch.stack([u[torch.randperm(rows, generator=g)] for _ in range(cols)], dim=1)
    # three of four positive: mixed signs, and no column whose terms cancel to nothing (the bound would then say nothing)
    sign = (torch.rand(rows, cols, generator=g) < 0.75).double() * 2 - 1
    sign[0], sign[1] = 1.0, -1.0          # both signs in every column, however few the rows
    return bf16((sign * torch.pow(2.0, e)).float())


def normal(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    return bf16(torch.randn(rows, cols, generator=g))


def unit(rows, cols, seed, signed=True):
    """sign * 2^v, bf16, v uniform in [-0.5, 0.5]: factors of magnitude about one, of either sign or positive."""
    g = torch.Generator().manual_seed(seed)
    sign = torch.randint(0, 2, (rows, cols), generator=g).float() * 2 - 1 if signed else 1.0
    return bf16(sign * torch.pow(2.0, torch.rand(rows, cols, generator=g) - 0.5))


def _count(terms):
    return (terms != 0).sum(0)


# ------------------------------------------------------------------------------------------------ RMSNorm backward (gain gradients)
RMS_SHAPES = [(9, 256), (300, 256), (9, 320), (300, 320)]


def rmsnorm_case(rows, width, maps):
    """dgain[c] = sum_r dy[dy_rows[r], c] * xhat[x_rows[r], c]; dy's magnitude is per row (one 2^u for the whole row, signs per element),
    so that a row's own reductions stay well conditioned and the spread is ACROSS the rows a gain element sums."""
    xs, ds = unit(rows, width, 100 + rows + width, signed=False), spread(rows, width, 200 + rows + width, per_row=True)      # row r of the op
    gain = bf16(1.0 + 0.25 * normal(1, width, 7))[0]
    g = torch.Generator().manual_seed(rows)
    x_rows = dy_rows = dx_rows = None
    x, dy = xs, ds
    if maps:          # the buffers have three rows more than the op has; the maps say where row r lives
        x_rows, dy_rows, dx_rows = (torch.randperm(rows + 3, generator=g)[:rows].int() for _ in range(3))
        x, dy = unit(rows + 3, width, 5), unit(rows + 3, width, 6)
        x[x_rows.long()], dy[dy_rows.long()] = xs, ds
    xs, ds = xs.double(), ds.double()
    xhat = xs / torch.sqrt((xs * xs).mean(1, keepdim=True) + EPS)
    terms = (ds * xhat).numpy()
    return {"x": x, "dy": dy, "gain": gain, "x_rows": x_rows, "dy_rows": dy_rows, "dx_rows": dx_rows, "rows": rows, "width": width,
            "terms": terms, "count": _count(terms)}


def chain_case(rows, width):
    """ttv_rmsnorm_backward_chain: h = acc + rmsnorm_bwd(x, gain1, dy), out = rmsnorm_bwd(y, gain2, h).
    dgain1[c] = sum_r dy * xhat ; dgain2[c] = sum_r h * yhat.  Destinations: gain 1's columns, then gain 2's."""
    # x of either sign, so that the row mean of gv * xhat is small beside gv (a dy parallel to x is what the norm's backward projects
    # out) and h keeps dy's magnitude and sign; gain 1's terms then take x's sign as well: with 9 rows a few columns end up one-signed
    x, y = unit(rows, width, 300 + rows + width), unit(rows, width, 301 + rows + width, signed=False)
    dy = spread(rows, width, 302 + rows + width, per_row=True)
    scale = dy.abs().amax(1, keepdim=True)
    acc = bf16(0.125 * unit(rows, width, 303 + rows + width) * scale)     # the residual gradient: an eighth of the row's magnitude
    gain1 = bf16(1.0 + 0.25 * normal(1, width, 8))[0]
    gain2 = bf16(1.0 + 0.25 * normal(1, width, 9))[0]
    xd, yd, dd, ad, g1 = x.double(), y.double(), dy.double(), acc.double(), gain1.double()
    xhat = xd / torch.sqrt((xd * xd).mean(1, keepdim=True) + EPS)
    rstd1 = 1.0 / torch.sqrt((xd * xd).mean(1, keepdim=True) + EPS)
    gv = dd * g1
    h = ad + rstd1 * (gv - xhat * (gv * xhat).mean(1, keepdim=True))
    yhat = yd / torch.sqrt((yd * yd).mean(1, keepdim=True) + EPS)
    terms = torch.cat([dd * xhat, h * yhat], dim=1).numpy()
    return {"x": x, "y": y, "dy": dy, "acc": acc, "gain1": gain1, "gain2": gain2, "rows": rows, "width": width, "terms": terms,
            "count": _count(terms)}


# ------------------------------------------------------------------------------------------------ column sums, the sum of all, outer
def colsum_case():
    a = spread(200, 320, 400)                  # four row blocks of 64 (the last of 8), two column tiles of 256 (the second of 64)
    terms = a.double().numpy()
    return {"a": a, "terms": terms, "count": _count(terms)}


def sumall_case():
    a = spread(600, 1, 500).reshape(3, 200)    # three blocks of 256 elements, the last of 88
    terms = (0.5 * a.double()).reshape(-1, 1).numpy()
    return {"a": a, "scale": 0.5, "terms": terms, "count": _count(terms)}


def outer_small_case():
    rows, C, d = 300, 5, 256                   # ten row blocks of 32, the last of 12
    a = spread(rows, C, 600)
    b = unit(rows, d, 601, signed=False)
    terms = (a.double()[:, :, None] * b.double()[:, None, :]).reshape(rows, C * d).numpy()      # destination c * d + f
    return {"a": a, "b": b, "rows": rows, "C": C, "d": d, "terms": terms, "count": _count(terms)}


# ------------------------------------------------------------------------------------------------ the two loss sums
CLIP_SIZES = [5000, 4099, 17]                  # three blocks for the first two clips (2048 elements each, the last short), one for the third


def clips_case():
    """target t and recon r = t + delta, |delta| = 2^(u / 2) with u walking -20 .. 0 (so delta^2 walks 2^-20 .. 1) and mixed signs;
    t is zero for three elements of four (r = delta exactly) and a bf16 number of [-1, 1] for the fourth, where r rounds."""
    recon, target = [], []
    for i, n in enumerate(CLIP_SIZES):
        g = torch.Generator().manual_seed(700 + i)
        u = torch.linspace(-20.0, 0.0, n, dtype=torch.float64)[torch.randperm(n, generator=g)]
        delta = (torch.randint(0, 2, (n,), generator=g).double() * 2 - 1) * torch.pow(2.0, u / 2)
        t = bf16(torch.rand(n, generator=g) * 2 - 1) * (torch.arange(n) % 4 == 3)
        r = bf16((t.double() + delta).float())
        r[::97] = 3.0                                       # outside [-1, 1]: the squared error clamps these, the L1 term does not
        recon.append(r)
        target.append(t)
    n_clips = len(CLIP_SIZES)
    l1 = np.concatenate([(r.double() - t.double()).abs().numpy() / (len(r) * n_clips) for r, t in zip(recon, target)])[:, None]
    sq = np.concatenate([((r.double().clamp(-1, 1) - t.double()) ** 2).numpy() for r, t in zip(recon, target)])[:, None]
    return {"recon": recon, "target": target, "l1_terms": l1, "sq_terms": sq}


# ------------------------------------------------------------------------------------------------ codebook gradient
def vq_case():
    rows, N, C = 300, 16, 5
    g = torch.Generator().manual_seed(800)
    others = [e for e in range(N) if e not in (3, 7)]
    idx = torch.tensor([3 if r % 2 == 0 else others[int(torch.randint(0, len(others), (1,), generator=g))] for r in range(rows)]).int()
    dcodes = spread(rows, C, 801)
    terms = np.zeros((rows, N * C))
    for r in range(rows):
        terms[r, int(idx[r]) * C:(int(idx[r]) + 1) * C] = dcodes[r].double().numpy()      # destination entry * C + c
    count = np.repeat(np.bincount(idx.numpy(), minlength=N), C)
    assert count[3 * C] == rows // 2 and count[7 * C] == 0
    # "walk_min": only the entry with half the rows is sure to see the whole range of magnitudes
    return {"dcodes": dcodes, "idx": idx, "rows": rows, "N": N, "C": C, "terms": terms, "count": count, "walk_min": 100}


# ------------------------------------------------------------------------------------------------ weight gradient
WGRAD_N, WGRAD_K = 136, 72                      # two ragged 128-wide tiles (128 + 8) by one of 72; 64-wide: 3 (the last of 8) by 2 (the last of 8)


def wgrad_case(L):
    dy = spread(L, WGRAD_N, 900 + L, per_row=True)
    x = unit(L, WGRAD_K, 901 + L, signed=False)
    terms = (dy.double()[:, :, None] * x.double()[:, None, :]).reshape(L, WGRAD_N * WGRAD_K).numpy()
    return {"dy": dy, "x": x, "L": L, "terms": terms, "count": _count(terms)}


# ------------------------------------------------------------------------------------------------ what the checks rest on
def f64_sum_and_bound(terms, count):
    """float64 sum per destination and the bound count * 2^-24 * sum |term| around it."""
    return terms.sum(0), count * U * np.abs(terms).sum(0)


def sequential_f32(terms):
    """The float32 sum of every destination's terms, one after the other from the first row down."""
    acc = np.zeros(terms.shape[1], dtype=np.float32)
    for row in terms.astype(np.float32):
        acc = (acc + row).astype(np.float32)
    return acc


def fold_f32(prefill, partials):
    """The second stage as the header states it: the partials of a destination added in ascending block index starting from block 0's,
    then the total added onto the destination - float32 (float64 for double partials) throughout."""
    total = partials[0].copy()
    for p in partials[1:]:
        total = (total + p).astype(partials.dtype)
    return (prefill + total).astype(partials.dtype)
