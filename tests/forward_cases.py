"""Seeded inputs of tests/test_hip_forward_shapes.py, built on the CPU (no GPU needed: tests/test_blockwise_cpu.py evaluates the
no-floored-block condition on the same inputs the GPU tests launch).

Attention batches (packed rows q | gate | k | v, one sequence per clip: K latent rows + the clip's patch grid):

  bench      32 x (16,128,128), K = 128: the benchmark launch, 36 864 rows, full items by the default rule
  five       5 x the same: half items by the default rule
  ragged     1025, 317, 53 and 1 rows (the batch of tests/test_hip_backward_shapes.py): short last blocks, a one-row sequence
  far        the same rows with FAR_ROWS: rows whose every score sits -100 / -40 / +90 log2-units from zero (same construction)
  spikes6 /  `ragged` with keys spiked (size 6 / 30, growing with the position) against one query direction in two sequences, that
  spikes30   direction copied into queries of other waves, blocks and sequences (SPIKE_KEYS, SPIKE_QUERIES)
  ragged_k   1152 (K = 128), 456 (K = 200: two latent query blocks), 53 (K = 5) and 1 rows: the restricted work tables
  base       1 x (32,256,256), K = 1024: 9 216 rows, 144 key tiles, 72 query blocks
"""
import torch

C_EXP = 0.125 * 1.4426950408889634          # head_dim^-0.5 * log2(e): what pre-scaled q carries
PATCH = (4, 8, 8)
_RAGGED = ([(16, 128, 128), (16, 64, 64), (8, 32, 48), (4, 8, 8)], [1, 61, 5, 0])
BATCHES = {
    "bench": ([(16, 128, 128)] * 32, [128] * 32),
    "five": ([(16, 128, 128)] * 5, [128] * 5),
    "ragged": _RAGGED,
    "far": _RAGGED,
    "spikes6": _RAGGED,
    "spikes30": _RAGGED,
    "ragged_k": ([(16, 128, 128), (16, 64, 64), (8, 32, 48), (4, 8, 8)], [128, 200, 5, 0]),
    "base": ([(32, 256, 256)], [1024]),
}
# rows of the "far" batch whose every score sits `level` log2-units from zero (sequences 0, 1 and 2; first, middle and last blocks):
# tests/test_hip_backward_shapes.py FAR_ROWS, asserted equal in tests/test_hip_forward_shapes.py
FAR_ROWS = {5: -100.0, 700: 90.0, 1024: -40.0, 1025 + 64: 90.0, 1025 + 316: -100.0, 1025 + 317 + 52: -40.0}
# (sequence, key position in it, added to the spike size).  Sequence 0 (1025 rows = 16 key tiles of 64 and a last tile of ONE key):
# inside the first tile (3: the reference already holds it), the first tile behind the reference (70), the next tile higher again
# (130: a shifted score set is shifted again), the lower lane half of a lane pair (200), beyond row 1 000 (1010) and the masked last
# tile (1024).  Each is higher than the one before, so the row maximum of an aligned query moves at every one of them.  Sequence 1
# (317 rows, last tile of 61 keys): 70 and the UPPER lane half (204), and the masked last tile (316).
SPIKE_KEYS = [(0, 3, 0.0), (0, 70, 2.0), (0, 130, 4.0), (0, 200, 6.0), (0, 1010, 8.0), (0, 1024, 10.0),
              (1, 70, 0.0), (1, 204, 4.0), (1, 316, 6.0)]
# packed query rows that carry the spiked direction in every q-head: row 5 (whose head 0 defines it), another wave (40) and block (140)
# of its sequence, a far block (1000), the one-row last block (1024); first, middle and last block of sequence 1.  (Every head: a
# head of row 1024 that is not aligned may average ~1 000 values into an output of 1e-4 of a block's usual energy, which
# block_errors would measure against its floor.)
SPIKE_QUERIES = [5, 40, 140, 1000, 1024, 1025 + 5, 1025 + 140, 1025 + 300]


def cu_seqlens(batch):
    shapes, counts = BATCHES[batch]
    cu = [0]
    for (t, h, w), k in zip(shapes, counts):
        cu.append(cu[-1] + k + (t // PATCH[0]) * (h // PATCH[1]) * (w // PATCH[2]))
    return cu


def attention_inputs(batch, hq, hkv):
    """fp32 rows [L, 2d + 2g] before any rounding, and the packed rows that get a per-row check (far / spiked-direction queries)."""
    cu = cu_seqlens(batch)
    d, gq = hq * 64, hkv * 64
    g = torch.Generator().manual_seed(100 * hq + hkv + len(batch))
    x = torch.randn(cu[-1], 2 * d + 2 * gq, generator=g)
    rows = []
    if batch == "far":      # tests/test_hip_backward_shapes.py _case, line for line
        x *= 0.5
        u = torch.randn(64, generator=g)
        u = u / u.norm() * 4.0                                          # |u| = 4; every key of every kv-head carries u exactly:
        kk = x[:, 2 * d:2 * d + gq].view(-1, hkv, 64)                   # the keys' own noise is made orthogonal to u
        kk -= (kk @ u / 16.0).unsqueeze(-1) * u
        x[:, 2 * d:2 * d + gq] += u.repeat(hkv)
        for row, level in FAR_ROWS.items():
            x[row, :d] += (level / (C_EXP * 16.0)) * u.repeat(hq)        # q . u * scale * log2(e) = level, every q-head
        rows = list(FAR_ROWS)
    elif batch.startswith("spikes"):    # tests/test_hip_ops.py test_attention_swp_reference_shift_branch, in two sequences
        spike = float(batch[len("spikes"):])
        x *= 0.5
        direction = x[5, :64].clone()
        for seq, pos, add in SPIKE_KEYS:
            x[cu[seq] + pos, 2 * d:2 * d + gq] = (spike + add) * torch.sign(direction).repeat(hkv)
        for row in SPIKE_QUERIES:
            x[row, :d] = direction.repeat(hq)
        rows = list(SPIKE_QUERIES)
    return x, rows


def attention_operands(x, hq):
    """The two bf16 operand sets of one case: `plain` (every column rounded once; the fp32 kernels get the same values) and `scaled`
    (the q columns multiplied by C_EXP BEFORE their one rounding, what a tower with qkv_q_prescaled emits)."""
    d = hq * 64
    plain = x.to(torch.bfloat16)
    scaled = plain.clone()
    scaled[:, :d] = (x[:, :d] * C_EXP).to(torch.bfloat16)
    return plain, scaled


# ---------------------------------------------------------------------------------------------- dense launches at width 256
DENSE_M = [36864, 36865, 5760, 1025, 143]
# clips whose packed rows give those M (the rotary table of ttv_linear_qkv_rope comes from a BatchPlan)
DENSE_PLANS = {
    36864: ([(16, 128, 128)] * 32, [128] * 32),
    36865: ([(16, 128, 128)] * 32 + [(4, 8, 8)], [128] * 32 + [0]),
    5760: ([(16, 128, 128)] * 5, [128] * 5),
    1025: ([(16, 128, 128)], [1]),
    143: ([(8, 32, 48)], [95]),
}


def planted_rows(M):
    """{row: kind} with kind 100.0 (row scaled by 100), 1e-3 or 0.0 (all-zero row): one of each at the first rows, at the last rows
    of the first 16-row tile, in the middle and at the very end (inside the ragged last tile where there is one).  The kinds rotate,
    so that the first row, row 15 and the last row each see a different one."""
    kinds = [100.0, 1e-3, 0.0]
    out = {}
    for n, r0 in enumerate((0, 13, M // 2, M - 3)):
        for i in range(3):
            out[r0 + i] = kinds[(i + 2 * n) % 3]
    return out


def plant(t, rows):
    for r, kind in rows.items():
        t[r] *= kind
    return t
