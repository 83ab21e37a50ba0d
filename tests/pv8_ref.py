"""TEST INFRASTRUCTURE - float64 / numpy restatement of the e4m3 P.V attention (csrc/ttv_attn_pv8.hip): the V
image (block membership, byte layout, slots), the exact-softmax reference on the DEQUANTISED image, the element bound of the P
quantisation and a float64 model of the kernel's P rounding.  Builds on the CPU; only tests import it.

Numerics restated (fixed by the issue that introduced the kernel):
  * q arrives pre-scaled by head_dim^-0.5 * log2(e): a score s = q . k IS the exponent; p = 2^(s - m_ref), m_ref <= the row maximum, lagging
    it by at most LAG = 2 log2 units; P enters the product as e4m3_rne(p * 2^K), K = 6 (2^(K + LAG) = 256 <= 448: never
    saturated); the row sum adds p before its rounding; the factor 2^K cancels in O / l.
  * V enters as an OCP-MX e4m3 image: a block = the 32 keys of one NATURAL HALF of a 64-key tile (tiles counted from the sequence's first
    row) times one head-dim column; E8M0 scale by oracle.fp8_oracle.mx_quantize's rule; keys past the sequence end are zero bytes.
"""
import numpy as np
import torch

from oracle.fp8_oracle import mx_dequantize, mx_quantize

KB = 64                  # keys per tile
TILE_BYTES = 4224        # 4096 element bytes + 128 scale bytes
K_LOG2 = 6               # P is quantised as p * 2^6
LAG = 2.0                # the kernel's reference lags the running row maximum by at most 2 log2 units
C_EXP = 0.125 * 1.4426950408889634


def keys_by_block() -> np.ndarray:
    """[2, 32]: the keys (0 .. 63 within a tile) of block t, in the order their 32 values enter mx_quantize.  Natural halves."""
    return np.arange(64).reshape(2, 32)


def fragment_key(h, b):
    """Key (within its tile) that byte b of lane half h of an A / B fragment holds: b = 16 t + e, e = the score accumulator's register,
    whose MFMA row is 8 (e >> 2) + 4 h + (e & 3)."""
    t, e = b >> 4, b & 15
    return 32 * t + 8 * (e >> 2) + 4 * h + (e & 3)


def tile_byte_positions() -> np.ndarray:
    """[64 keys, 64 d] -> byte offset of V[key][d]'s e4m3 byte inside its 4 224-byte tile: [dt = d >> 5][lane = 32 h + (d & 31)][b]."""
    pos = np.zeros((64, 64), dtype=np.int64)
    for h in range(2):
        for b in range(32):
            key = fragment_key(h, b)
            for d in range(64):
                pos[key, d] = (d >> 5) * 2048 + (32 * h + (d & 31)) * 32 + b
    return pos


def scale_byte_positions() -> np.ndarray:
    """[2 blocks, 64 d] -> byte offset of block (t, d)'s E8M0 byte inside its tile."""
    t, d = np.meshgrid(np.arange(2), np.arange(64), indexing="ij")
    return 4096 + (d >> 5) * 64 + 32 * t + (d & 31)


def tile_slot(cu, seq) -> int:
    """Slot of a sequence's first tile: the tiles of sequence i start at (cu[i] >> 6) + i, slots between sequences stay unused."""
    return (int(cu[seq]) >> 6) + seq


def image_bytes(total_rows, n_seqs, kv_heads) -> int:
    return ((total_rows >> 6) + n_seqs) * kv_heads * TILE_BYTES


def v_image(v: torch.Tensor, cu, kv_heads, fill=0):
    """v [L, kv_heads * 64] (bf16 values) -> (image uint8 [image_bytes] with unused slots = fill, dequantised V float64 [L, kv_heads * 64])."""
    L = int(cu[-1])
    n_seqs = len(cu) - 1
    img = np.full(image_bytes(L, n_seqs, kv_heads), fill, dtype=np.uint8)
    deq = torch.zeros(L, kv_heads * 64, dtype=torch.float64)
    pos, spos, kb = tile_byte_positions(), scale_byte_positions(), keys_by_block()
    vf = v.float()
    for s in range(n_seqs):
        s0, S = int(cu[s]), int(cu[s + 1] - cu[s])
        for kt in range((S + KB - 1) // KB):
            n = min(KB, S - kt * KB)
            for kvh in range(kv_heads):
                tile = torch.zeros(64, 64)
                tile[:n] = vf[s0 + kt * KB:s0 + kt * KB + n, kvh * 64:(kvh + 1) * 64]
                # rows of the regrouped matrix: block (t, d) = tile[keys_by_block()[t], d]
                x = torch.stack([tile[torch.from_numpy(kb[t])].t() for t in range(2)]).reshape(128, 32)
                q, e8, _ = mx_quantize(x)
                base = ((tile_slot(cu, s) + kt) * kv_heads + kvh) * TILE_BYTES
                qn = q.view(2, 64, 32).numpy()
                for t in range(2):
                    img[base + pos[kb[t]].T] = qn[t]                   # [d, j] <- byte of key kb[t][j], column d
                img[base + spos] = e8.view(2, 64).numpy()
                dq = mx_dequantize(q, e8).view(2, 64, 32)
                back = torch.zeros(64, 64, dtype=torch.float64)
                for t in range(2):
                    back[torch.from_numpy(kb[t])] = dq[t].t()
                deq[s0 + kt * KB:s0 + kt * KB + n, kvh * 64:(kvh + 1) * 64] = back[:n]
    return img, deq


def _heads(x, cu, hq, hkv):
    """Yields (rows slice, q-head, q [S, 64], k [S, 64], kv-head) in float64 for every sequence and q-head of packed rows q | gate | k | v."""
    d, g = hq * 64, hkv * 64
    xd = x.double()
    for s in range(len(cu) - 1):
        rows = slice(int(cu[s]), int(cu[s + 1]))
        for hd in range(hq):
            kvh = hd // (hq // hkv)
            yield rows, hd, xd[rows, hd * 64:(hd + 1) * 64], xd[rows, 2 * d + kvh * 64:2 * d + (kvh + 1) * 64], kvh


def _gate(x, rows, hd, hq, gate):
    d = hq * 64
    return torch.sigmoid(x[rows, d + hd * 64:d + (hd + 1) * 64].double()) if gate else None


def pv8_attention(x, cu, hq, hkv, v_deq, gate):
    """Exact float64 attention on the bf16 q, k (q pre-scaled: scores are base-2 exponents) and the DEQUANTISED V image.
    Returns (O [L, d], bound_terms) where bound_terms = dict of [L, d] / [L, hq] float64 arrays the element bound is made of:
      quant  (1/l) sum_t max(2^-4 p_t, 2^-(10 + K)) |V_td|   with p relative to the row maximum (the kernel's reference is never higher,
             so its p are never smaller and its subnormal floor never coarser)
      A      (1/l) sum_t p_t |V_td|
      qk     max_t sum_i |q_i k_ti|     (the fp32 score accumulation's scale)
      g      the gate factor (1 without)"""
    L, d = x.shape[0], hq * 64
    O = torch.zeros(L, d, dtype=torch.float64)
    quant, A, g = torch.zeros_like(O), torch.zeros_like(O), torch.ones_like(O)
    qk = torch.zeros(L, hq, dtype=torch.float64)
    floor = 2.0 ** -(10 + K_LOG2)
    for rows, hd, q, k, kvh in _heads(x, cu, hq, hkv):
        s = q @ k.t()
        p = torch.exp2(s - s.amax(1, keepdim=True))
        l = p.sum(1, keepdim=True)
        v = v_deq[rows, kvh * 64:(kvh + 1) * 64]
        cols = slice(hd * 64, (hd + 1) * 64)
        O[rows, cols] = (p @ v) / l
        quant[rows, cols] = (torch.maximum(p / 16.0, torch.full_like(p, floor)) @ v.abs()) / l
        A[rows, cols] = (p @ v.abs()) / l
        qk[rows, hd] = (q.abs() @ k.abs().t()).amax(1)
        if gate:
            g[rows, cols] = _gate(x, rows, hd, hq, True)
    return O * g, dict(quant=quant, A=A, qk=qk, g=g)


def element_bound(o_ref, terms, cu, hq):
    """The bound of tests/test_hip_attn_pv8.py (its docstring counts the constants) for every output element."""
    L, d = o_ref.shape
    S = torch.zeros(L, 1, dtype=torch.float64)
    for s in range(len(cu) - 1):
        S[int(cu[s]):int(cu[s + 1])] = float(cu[s + 1] - cu[s])
    nkt = torch.ceil(S / KB)
    eps_p = np.log(2.0) * (2.0 ** -18 * terms["qk"] + 2.0 ** -24 * 160.0) + 2.0 ** -21            # [L, hq]
    eps_p = eps_p.repeat_interleave(64, dim=1)
    acc = (64.0 + nkt + 8.0 + S + 2.0) * 2.0 ** -24
    pre = (terms["quant"] + (2.0 * eps_p + acc) * terms["A"]) * terms["g"] * (1.0 + 2.0 ** -20)
    return pre + 2.0 ** -9 * (o_ref.abs() + pre)


def pv8_model(x, cu, hq, hkv, v_deq, gate, lag=0.0):
    """float64 model of the kernel's ONE inexact step: P rounded to e4m3 at p * 2^K against a reference `lag` below the row maximum,
    row sums from the unrounded p; everything else exact.  (torch's float8_e4m3fn cast rounds to nearest even.)"""
    L, d = x.shape[0], hq * 64
    O = torch.zeros(L, d, dtype=torch.float64)
    for rows, hd, q, k, kvh in _heads(x, cu, hq, hkv):
        s = q @ k.t()
        p = torch.exp2(s - (s.amax(1, keepdim=True) - lag) + K_LOG2)
        assert float(p.max()) <= 448.0 * (1 + 1e-12)
        p8 = p.float().to(torch.float8_e4m3fn).double()
        o = (p8 @ v_deq[rows, kvh * 64:(kvh + 1) * 64]) / p.sum(1, keepdim=True)
        if gate:
            o = o * _gate(x, rows, hd, hq, True)
        O[rows, hd * 64:(hd + 1) * 64] = o
    return O


def attention_f64(x, cu, hq, hkv, gate):
    """Exact float64 attention on the bf16 rows as they are (V not quantised): what both kernels approximate."""
    d = hq * 64
    return pv8_attention(x, cu, hq, hkv, x[:, 2 * d + hkv * 64:2 * d + 2 * hkv * 64].double(), gate)[0]


# ---------------------------------------------------------------------------------------------- inputs and work tables
def table(cu, hq, half_rows=()):
    """int32 [n, 4] work table (sequence, first query row, q-head, mode): 128-row items, except that in the sequences named in half_rows
    every 128-row block is issued as two 64-row mode-1 items; one padding entry in front and one at the end."""
    out = [(-1, 0, 0, 0)]
    for s in range(len(cu) - 1):
        S = int(cu[s + 1] - cu[s])
        for hd in range(hq):
            for q0 in range(0, S, 128):
                if s in half_rows:
                    out += [(s, q0, hd, 1)] + ([(s, q0 + 64, hd, 1)] if q0 + 64 < S else [])
                else:
                    out.append((s, q0, hd, 0))
    out.append((-1, 0, 0, 0))
    return torch.tensor(out, dtype=torch.int32)


SHAPES = {
    # name: (sequence lengths, q-heads, kv-heads, gate, sequences issued as mode-1 items)
    "s128": ([128], 1, 1, False, ()),
    "s200_gqa_gate": ([200], 4, 2, True, ()),
    "packed": ([64, 129, 320], 4, 2, True, ()),
    "packed_mode1": ([64, 129, 320], 2, 2, False, (1, 2)),
}


def rows(shape, spread, seed=0):
    """bf16 packed rows q | gate | k | v with q PRE-SCALED (scores of standard deviation ~`spread` log2 units), and cu_seqlens."""
    lens, hq, hkv, gate, half = SHAPES[shape]
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    d, g = hq * 64, hkv * 64
    gen = torch.Generator().manual_seed(1000 * seed + 17 * hq + hkv + int(10 * spread) + sum(lens))
    x = torch.randn(int(cu[-1]), 2 * d + 2 * g, generator=gen)
    x[:, :d] *= spread / 8.0
    return x.to(torch.bfloat16), cu


def spiked_rows(seed=3):
    """One sequence of 320 rows (5 tiles), 2 / 1 heads, spread 1.5, with keys spiked against one query direction: each spike arrives after
    the first tile and lies more than 140 log2 units above everything before it - lower lane half (key 64 + 2: h = 0), upper lane half
    (key 128 + 4 + 1: h = 1), a key >= 32 of its tile (key 192 + 40), and the last tile.  Returns (x bf16, cu, aligned query rows)."""
    hq, hkv = 2, 1
    cu = np.array([0, 320], dtype=np.int32)
    d, g = hq * 64, hkv * 64
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(320, 2 * d + 2 * g, generator=gen)
    x[:, :d] *= 1.5 / 8.0
    sign = torch.sign(torch.randn(64, generator=gen))
    for key, a in ((66, 2.5), (133, 5.0), (232, 7.5), (300, 10.0)):          # scores 160, 320, 480, 640 for an aligned query
        x[key, 2 * d:2 * d + 64] = a * sign
    aligned = [3, 40, 70, 100, 127, 130, 200, 319]                           # every wave of the first block, later blocks, the last row
    for r in aligned:
        x[r, :d] = sign.repeat(hq)
    return x.to(torch.bfloat16), cu, aligned
