"""Block-wise error measure and float64 attention reference for the attention tests (no GPU needed; imported by
tests/test_hip_backward_shapes.py and checked by tests/test_blockwise_cpu.py).

A global relative Frobenius error hides one wrong tile: among the 36 864 rows of a 32-clip batch a single 64-row block of one head
carries ~4 % of the norm, so a block that is off by 5 % moves the global figure by 0.2 %.  `block_errors` measures every
(sequence, head, 64-row block) on its own - the granularity at which the attention kernels tile the rows of a sequence (64-row
backward blocks, half of a 128-row query block) - and `check_blockwise` asserts both figures.  `tile_errors` / `check_tiles` do the
same per 128 x 128 tile of a weight gradient (tests/test_hip_backward_bf16.py).

For the inference forward (tests/test_hip_forward_shapes.py): `attention_forward_reference` (float64, no autograd, chunked over query
rows), `check_row_tiles` (dense [M, N] outputs per 16-row x 64-column tile: one MFMA row group of one wave), `check_rows` (single
planted rows), `floored_blocks` (which blocks `block_errors` would measure against its floor: a test that may not leave a block out
asserts there are none) and `bf16_store` (the rounding points of a reference-only rounding model)."""
import torch


def row_blocks(cu_seqlens, block: int = 64):
    """Block id of every packed row (blocks restart at each sequence start; a sequence's last block may be short) and the count."""
    ids, n = [], 0
    for b in range(len(cu_seqlens) - 1):
        s = int(cu_seqlens[b + 1]) - int(cu_seqlens[b])
        ids.append(n + torch.arange(s) // block)
        n += -(-s // block)
    return (torch.cat(ids) if ids else torch.zeros(0, dtype=torch.long)), n


def block_errors(x, ref, cu_seqlens, heads: int, block: int = 64):
    """[n_blocks, heads] relative Frobenius error ||x - ref|| / ||ref|| per (sequence, head, `block`-row block).  x, ref: [L, heads * w]
    (any dtype, compared in float64).  A reference block whose norm is far below the typical block's (< 1e-2 of the root-mean-square
    block norm) is measured against that floor instead: such a block is a cancellation (dQ of a one-row sequence is exactly zero: its
    softmax is 1 and dS = dP - delta), where the kernel's rounding residue has no meaningful relative size.  An all-zero reference
    block with an O(1) result is still an error far beyond any bound."""
    x, ref = x.double().cpu(), ref.double().cpu()
    L = ref.shape[0]
    assert x.shape == ref.shape and ref.shape[1] % heads == 0, (tuple(x.shape), tuple(ref.shape), heads)
    ids, n = row_blocks(cu_seqlens, block)
    assert ids.numel() == L, (ids.numel(), L)
    d2 = (x - ref).pow(2).view(L, heads, -1).sum(-1)
    r2 = ref.pow(2).view(L, heads, -1).sum(-1)
    num = torch.zeros(n, heads, dtype=torch.float64).index_add_(0, ids, d2)
    den = torch.zeros(n, heads, dtype=torch.float64).index_add_(0, ids, r2)
    floor = 1e-4 * float(den.mean()) + 1e-300
    return (num / den.clamp_min(floor)).sqrt()


def floored_blocks(ref, cu_seqlens, heads: int, block: int = 64):
    """[n_blocks, heads] bool: the (sequence, head, block) cells of `ref` whose energy is under the floor of `block_errors` (1e-4 of the
    mean block energy).  Such a cell is measured against the floor, not against itself - a way to leave it out; a test that must
    measure every block asserts that this mask is empty, from the reference alone."""
    ref = ref.double().cpu()
    L = ref.shape[0]
    ids, n = row_blocks(cu_seqlens, block)
    assert ids.numel() == L and ref.shape[1] % heads == 0, (ids.numel(), tuple(ref.shape), heads)
    den = torch.zeros(n, heads, dtype=torch.float64).index_add_(0, ids, ref.pow(2).view(L, heads, -1).sum(-1))
    return den < 1e-4 * float(den.mean()) + 1e-300


def global_error(x, ref) -> float:
    x, ref = x.double().cpu(), ref.double().cpu()
    return float((x - ref).norm() / (ref.norm() + 1e-30))


def check_blockwise(x, ref, cu_seqlens, heads: int, block_tol: float, global_tol: float, what: str = ""):
    """Assert that x is finite, within `global_tol` of ref as a whole and within `block_tol` in every (sequence, head, block).
    Returns (worst block error, global error) for the report."""
    assert bool(torch.isfinite(x.double()).all()), f"{what}: non-finite values"
    glob = global_error(x, ref)
    err = block_errors(x, ref, cu_seqlens, heads)
    worst = float(err.max()) if err.numel() else 0.0
    assert glob < global_tol, f"{what}: global relative error {glob:.3e} >= {global_tol:.1e}"
    if err.numel():
        blk, head = divmod(int(err.argmax()), err.shape[1])
        assert worst < block_tol, f"{what}: block {blk} head {head}: relative error {worst:.3e} >= {block_tol:.1e} (global {glob:.3e})"
    return worst, glob


def attention_reference(qkvg, dout, cu_seqlens, hq: int, hkv: int):
    """float64 per-sequence softmax attention (non-causal, scale 1/8, GQA: q-head h reads kv-head h // (hq / hkv)) on the packed
    [L, 2d + 2g] rows q | gate | k | v of the attention kernels, and its autograd backward for the upstream gradient `dout` [L, d].
    Returns out [L, d] (ungated), gated = out * sigmoid(gate), lse [L, hq] (natural log of the row sums of exp(scores)) and
    grad [L, 2d + 2g] (gradient of <out, dout> w.r.t. q, k, v; zero in the gate columns).  Autograd runs per (sequence, kv-head) so a
    1152-row sequence costs a few 10 MB.  (The oracle's attention_varlen computes in float32 whatever its inputs.)"""
    x, do = qkvg.detach().double().cpu(), dout.detach().double().cpu()
    L, d, g, rep = x.shape[0], hq * 64, hkv * 64, hq // hkv
    out = torch.zeros(L, d, dtype=torch.float64)
    lse = torch.zeros(L, hq, dtype=torch.float64)
    grad = torch.zeros_like(x)
    for b in range(len(cu_seqlens) - 1):
        s, e = int(cu_seqlens[b]), int(cu_seqlens[b + 1])
        n = e - s
        for kh in range(hkv):
            qc = slice(kh * rep * 64, (kh + 1) * rep * 64)
            kc = slice(2 * d + kh * 64, 2 * d + (kh + 1) * 64)
            vc = slice(2 * d + g + kh * 64, 2 * d + g + (kh + 1) * 64)
            q = x[s:e, qc].reshape(n, rep, 64).transpose(0, 1).clone().requires_grad_(True)      # [rep, n, 64]
            k = x[s:e, kc].clone().requires_grad_(True)
            v = x[s:e, vc].clone().requires_grad_(True)
            sc = q @ k.T * 0.125
            o = torch.softmax(sc, -1) @ v
            o.backward(do[s:e, qc].reshape(n, rep, 64).transpose(0, 1))
            with torch.no_grad():
                out[s:e, qc] = o.transpose(0, 1).reshape(n, rep * 64)
                lse[s:e, kh * rep:(kh + 1) * rep] = torch.logsumexp(sc, -1).T
            grad[s:e, qc] = q.grad.transpose(0, 1).reshape(n, rep * 64)
            grad[s:e, kc] = k.grad
            grad[s:e, vc] = v.grad
    gated = out * torch.sigmoid(x[:, d:2 * d])
    return out, gated, lse, grad


def tile_errors(x, ref, tile: int = 128):
    """[ceil(N / tile), ceil(K / tile)] relative Frobenius error per `tile` x `tile` tile of 2-D [N, K] matrices - the output tile of
    the weight-gradient GEMM (k_wgrad128_bf16): one wrong tile or split of it shows here and nowhere in a global figure.  Edge tiles
    are short.  Same floor as block_errors: a tile whose reference norm is below 1e-2 of the root-mean-square tile norm is measured
    against that floor."""
    x, ref = x.double().cpu(), ref.double().cpu()
    assert x.shape == ref.shape and ref.dim() == 2, (tuple(x.shape), tuple(ref.shape))
    N, K = ref.shape
    tn, tk = -(-N // tile), -(-K // tile)

    def sums(v):
        v = torch.nn.functional.pad(v.pow(2), (0, tk * tile - K, 0, tn * tile - N))
        return v.view(tn, tile, tk, tile).sum((1, 3))
    num, den = sums(x - ref), sums(ref)
    floor = 1e-4 * float(den.mean()) + 1e-300
    return (num / den.clamp_min(floor)).sqrt()


def check_tiles(x, ref, tile_tol: float, global_tol: float, what: str = "", tile: int = 128):
    """Assert that the matrix x is finite, within `global_tol` of ref as a whole and within `tile_tol` in every tile.  Returns
    (worst tile error, global error)."""
    assert bool(torch.isfinite(x.double()).all()), f"{what}: non-finite values"
    glob = global_error(x, ref)
    err = tile_errors(x, ref, tile)
    worst = float(err.max())
    assert glob < global_tol, f"{what}: global relative error {glob:.3e} >= {global_tol:.1e}"
    tn, tk = divmod(int(err.argmax()), err.shape[1])
    assert worst < tile_tol, f"{what}: tile ({tn}, {tk}): relative error {worst:.3e} >= {tile_tol:.1e} (global {glob:.3e})"
    return worst, glob


def bf16_store(x):
    """One store to bfloat16 (round to nearest even) and back to float64: a rounding point of a reference-only rounding model."""
    return x.to(torch.bfloat16).double()


CHUNK_ELEMENTS = 1 << 24      # float64 scores of one chunk of attention_forward_reference: 128 MB


def attention_forward_reference(qkvg, cu_seqlens, hq: int, hkv: int, c_exp=None):
    """float64 forward of `attention_reference` without autograd, chunked over query rows (a chunk's [rep, rows, S] scores stay under
    ~128 MB, so one 9 216-row sequence with 12 / 4 heads costs a few hundred MB where the autograd graph of `attention_reference`
    would keep ~6 GB).  Returns out [L, d] (ungated) and gated = out * sigmoid(gate).
    c_exp None: scores = q . k / 8, softmax with e.  c_exp given (head_dim^-0.5 * log2(e)): the q columns of `qkvg` ALREADY carry that
    factor - pass the pre-scaled q as rounded to bf16, the operand the pre-scaled kernels read - and the softmax is 2^(q . k)."""
    x = qkvg.detach().double().cpu()
    L, d, g, rep = x.shape[0], hq * 64, hkv * 64, hq // hkv
    assert x.shape[1] == 2 * d + 2 * g and hq % hkv == 0, (tuple(x.shape), hq, hkv)
    fac = 0.125 if c_exp is None else 0.6931471805599453            # natural exponent per unit of q . k
    out = torch.zeros(L, d, dtype=torch.float64)
    with torch.no_grad():
        for b in range(len(cu_seqlens) - 1):
            s, e = int(cu_seqlens[b]), int(cu_seqlens[b + 1])
            n = e - s
            step = max(64, CHUNK_ELEMENTS // (rep * max(n, 1)))
            for kh in range(hkv):
                qc = slice(kh * rep * 64, (kh + 1) * rep * 64)
                k = x[s:e, 2 * d + kh * 64:2 * d + (kh + 1) * 64]
                v = x[s:e, 2 * d + g + kh * 64:2 * d + g + (kh + 1) * 64]
                kt = (k * fac).T.contiguous()
                for r0 in range(0, n, step):
                    r1 = min(r0 + step, n)
                    q = x[s + r0:s + r1, qc].reshape(r1 - r0, rep, 64).transpose(0, 1)      # [rep, rows, 64]
                    o = torch.softmax(q @ kt, -1) @ v
                    out[s + r0:s + r1, qc] = o.transpose(0, 1).reshape(r1 - r0, rep * 64)
    gated = out * torch.sigmoid(x[:, d:2 * d])
    return out, gated


def row_tile_errors(x, ref, rows: int = 16, cols: int = 64):
    """[ceil(M / rows), N / cols] relative Frobenius error per `rows` x `cols` tile of a dense [M, N] output: 16 x 64 is one MFMA row
    group of one wave in the width-256 kernels.  A ragged last tile is short.  It is `block_errors` on one sequence of M rows with
    N / cols heads (same floor rule)."""
    assert ref.shape[1] % cols == 0, (tuple(ref.shape), cols)
    return block_errors(x, ref, [0, ref.shape[0]], ref.shape[1] // cols, rows)


def check_row_tiles(x, ref, rows: int = 16, cols: int = 64, tile_tol: float = 0.0, global_tol: float = 0.0, what: str = "",
                    leave_out=()):
    """Assert that the dense [M, N] output x is finite, within `global_tol` of ref as a whole and within `tile_tol` in every
    `rows` x `cols` tile.  `leave_out`: rows that are measured elsewhere (`check_rows`) and taken out of both figures - a planted row
    of 100 x the norm of its neighbours would otherwise be all its tile says.  Returns (worst tile error, global error)."""
    assert bool(torch.isfinite(x.double()).all()), f"{what}: non-finite values"
    x, ref = x.double().cpu(), ref.double().cpu()
    if len(leave_out):
        idx = torch.as_tensor(list(leave_out), dtype=torch.long)
        x, ref = x.clone(), ref.clone()
        x[idx] = 0.0
        ref[idx] = 0.0
    glob = global_error(x, ref)
    err = row_tile_errors(x, ref, rows, cols)
    worst = float(err.max()) if err.numel() else 0.0
    assert glob < global_tol, f"{what}: global relative error {glob:.3e} >= {global_tol:.1e}"
    if err.numel():
        t, c = divmod(int(err.argmax()), err.shape[1])
        assert worst < tile_tol, (f"{what}: tile rows {t * rows}..{min((t + 1) * rows, ref.shape[0]) - 1} columns {c * cols}..{(c + 1) * cols - 1}: "
                                  f"relative error {worst:.3e} >= {tile_tol:.1e} (global {glob:.3e})")
    return worst, glob


def row_errors(x, ref, rows, heads: int = 1):
    """[len(rows), heads] relative error ||x - ref|| / ||ref|| of the given rows, per `heads` equal column groups.  No floor: a
    reference row of norm zero with an exact result gives 0, with any other result inf."""
    idx = torch.as_tensor(list(rows), dtype=torch.long)
    x, ref = x.double().cpu()[idx], ref.double().cpu()[idx]
    num = (x - ref).pow(2).view(len(idx), heads, -1).sum(-1).sqrt()
    den = ref.pow(2).view(len(idx), heads, -1).sum(-1).sqrt()
    return torch.where(num == 0, torch.zeros_like(num), num / den)


def check_rows(x, ref, rows, tol, what: str = "", heads: int = 1):
    """Assert that each of the given rows of x is finite and within `tol` (a number, or one bound per row) of the same row of ref, per
    `heads` column groups.  Returns the worst relative error."""
    rows = list(rows)
    if not rows:
        return 0.0
    assert bool(torch.isfinite(x.double()[rows]).all()), f"{what}: non-finite values in rows {rows}"
    err = row_errors(x, ref, rows, heads)
    bound = torch.as_tensor(tol, dtype=torch.float64).expand(len(rows)) if not isinstance(tol, (int, float)) else torch.full((len(rows),), float(tol), dtype=torch.float64)
    over = err >= bound.unsqueeze(1)
    if bool(over.any()):
        i, h = divmod(int((err / bound.unsqueeze(1)).argmax()), heads)
        raise AssertionError(f"{what}: row {rows[i]} head {h}: relative error {float(err[i, h]):.3e} >= {float(bound[i]):.1e}")
    return float(err.max())
