"""Per-batch metadata, computed on the host from Python ints and uploaded once per distinct batch shape.

Replaces the reference's device-side bookkeeping and the host syncs it causes (model/base/blocks.py:80-88,
154-162: grids//patch, cu_seqlens, bool mask by repeat_interleave; model/base/rope.py:57-71: per-sample Python
loop).  Row layout of a packed batch: clip b owns rows [cu[b], cu[b+1]); its K_b latent tokens come first, then
its P_b patch tokens in (t,h,w) raster order (blocks.py:85-86).

The RoPE table follows rope.py:40-54 exactly: fp64 `theta**linspace(0,1,F) * pi/2` times the fp32 position ids,
`torch.polar` in fp64, then cast to fp32 (the reference casts to complex64 at apply time, rope.py:24).
"""
from __future__ import annotations

import ctypes as C
import functools
import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, streams, switches

QBLOCK = 128  # query rows per attention workgroup (csrc/ttv_attn.hip QB)
ATTN_SLOTS = 1024  # table size below which the last third of every sequence's blocks become half items (set when the kernel held 4 blocks per CU; it holds 3 = 768 since round 2 - the rule was re-measured, not re-derived: see attention_table)


@functools.lru_cache(maxsize=8)
def _rope_base_table(head_dim: int, nd: int, n_ids: int, theta: float = 10000.0):
    """fp32 cos/sin of inv_freq[f] * n for every integer position id n < n_ids, evaluated exactly like the reference
    (rope.py:40-54: fp64 `theta**linspace(0,1,F) * pi/2`, fp64 product with the id, torch.polar, cast to fp32).  Position
    ids are small integers (latent index, or grid coordinate + token count), so every table entry the reference computes
    per row is one of these n_ids * F values - rows are gathered from here instead of re-evaluating fp64 trigonometry."""
    f = head_dim // (2 * nd)
    inv = torch.pow(theta, torch.linspace(0.0, 1.0, f, dtype=torch.float64)) * torch.pi / 2.0
    ids = torch.arange(n_ids, dtype=torch.float32).to(torch.float64)
    ang = ids.view(-1, 1) * inv.view(1, -1)                       # [n_ids, F]; same fp64 product as inv * id
    fc = torch.polar(torch.ones(1, dtype=torch.float64), ang)
    return fc.real.to(torch.float32).numpy(), fc.imag.to(torch.float32).numpy()


_copy_streams = {}
_pinned_stage = {}


def _upload(host: np.ndarray, device) -> torch.Tensor:
    """Host table -> device, complete on return, without waiting for compute.  A plain `.to(device)` from pageable memory is
    ordered after everything queued on the current stream, i.e. it waits for the previous batch's forward, which serialises the
    host with the GPU when every batch needs a new plan (ragged batches from a loader).  Here the copy goes through pinned
    memory on a stream of its own and only that copy is waited for (~10 us), so the table can be used from any stream."""
    t = torch.from_numpy(host)
    dev = torch.device(device)
    if dev.type != "cuda":
        return t.to(dev)
    cs = _copy_streams.get(str(dev))
    if cs is None:
        cs = _copy_streams[str(dev)] = torch.cuda.Stream(device=dev)
    # staging through a CACHED pinned buffer: `pin_memory()` per table is a hipHostMalloc (~1 ms; six tables per training step on
    # ragged batches).  The copy is waited for before return, so one buffer per device can be reused by the next call.
    nbytes = t.numel() * t.element_size()
    stage = _pinned_stage.get(str(dev))
    if stage is None or stage.numel() < nbytes:
        stage = _pinned_stage[str(dev)] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8).pin_memory()
    view = stage[:nbytes].view(t.dtype).view(t.shape)
    # numpy, not Tensor.copy_: above 32 K elements torch's CPU copy is a parallel region of its intra-op pool, and waking that pool
    # (128 threads on a 16-CPU container share) starves the launch path of the whole process (train.limit_host_threads)
    np.copyto(view.numpy(), host)
    with torch.cuda.stream(cs):
        out = view.to(dev, non_blocking=True)
    cs.synchronize()
    return out


@functools.lru_cache(maxsize=16)
def _rope_base_device(head_dim: int, nd: int, n_ids: int, device: str):
    c, s_ = _rope_base_table(head_dim, nd, n_ids)
    return torch.from_numpy(c).to(device).contiguous(), torch.from_numpy(s_).to(device).contiguous()


@functools.lru_cache(maxsize=16)
def _rope_base_interleaved(head_dim: int, nd: int, n_ids: int, device: str):
    """fp32 [n_ids + 1, F, 2] = (cos, sin) of every (position id, frequency), row n_ids = (1, 0): the table the to_qkv kernel gathers
    its rotary factors from (same values as _rope_base_table, i.e. as the reference's freqs_cis after the fp32 cast)."""
    c, s_ = _rope_base_table(head_dim, nd, n_ids)
    t = np.empty((n_ids + 1, c.shape[1], 2), dtype=np.float32)
    t[:n_ids, :, 0] = c
    t[:n_ids, :, 1] = s_
    t[n_ids, :, 0] = 1.0
    t[n_ids, :, 1] = 0.0
    return torch.from_numpy(t).to(device).contiguous()


def _rope_clip_table(grid: Tuple[int, ...], k: int, head_dim: int) -> np.ndarray:
    """fp32 [K+P, 64] = cos[32] | sin[32] for one clip; pairs beyond 3*F keep (1, 0) (rope.py:24 leaves them alone).
    Row ids: latent i -> (i,i,i); patch (t,h,w) -> (t,h,w) + K (rope.py:59-67); column f*nd + axis (interleaved)."""
    nd = len(grid)
    f = head_dim // (2 * nd)
    half = head_dim // 2
    n_ids = 1
    while n_ids < k + max(grid) + 1:
        n_ids *= 2
    n_ids = max(n_ids, 512)
    cos_t, sin_t = _rope_base_table(head_dim, nd, n_ids)
    p = int(np.prod(grid))
    ids = np.empty((k + p, nd), dtype=np.int64)
    ids[:k] = np.arange(k)[:, None]
    coords = np.indices(grid).reshape(nd, -1).T                     # raster order == torch.cartesian_prod
    ids[k:] = coords + k
    out = np.zeros((k + p, 2 * half), dtype=np.float32)
    out[:, :half] = 1.0
    # out[row, f*nd + axis] = table[ids[row, axis], f]
    out[:, : nd * f] = cos_t[ids].transpose(0, 2, 1).reshape(k + p, nd * f)
    out[:, half: half + nd * f] = sin_t[ids].transpose(0, 2, 1).reshape(k + p, nd * f)
    return out


@functools.lru_cache(maxsize=512)
def _clip_rope_ids(grid: Tuple[int, ...], k: int, n_ids: int) -> np.ndarray:
    """uint16 [K + P, 4] rotary position ids of one clip (rope.py:59-67): latent i -> (i, i, i), patch (t, h, w) -> (t, h, w) + K in raster
    order, slot 3 = the identity row of the base table (pairs 30, 31).  Read-only (cached)."""
    p = int(np.prod(grid))
    ids = np.empty((k + p, 4), dtype=np.uint16)
    ids[:, 3] = n_ids
    ids[:k, :3] = np.arange(k, dtype=np.uint16)[:, None]
    coords = np.indices(grid).reshape(len(grid), -1).T                      # raster order (t, h, w)
    ids[k:, :3] = np.minimum(coords + k, n_ids - 1).astype(np.uint16)
    ids.setflags(write=False)
    return ids


def _deal_xcd(weights) -> List[List[int]]:
    """Greedy deal of weighted units over the 8 XCD lists (`deal` of csrc/ttv_plan_host.cpp): units in descending order of their
    integer weight (stable: equal weights keep index order), each to the first list of minimum load.  Returns the unit indices of
    every list in the order they were dealt."""
    lists, load = [[] for _ in range(8)], [0] * 8
    for i in sorted(range(len(weights)), key=weights.__getitem__, reverse=True):
        x = min(range(8), key=load.__getitem__)
        lists[x].append(i)
        load[x] += weights[i]
    return lists


def _xcd_interleave(units) -> np.ndarray:
    """(sequence, first row) entries of the attention backward's 64-row blocks, ordered for the 8 XCDs: block b of a launch runs on XCD
    b % 8 under round-robin dispatch (a speed assumption only), and every block of a sequence streams that sequence's Q / dO (key
    blocks) or K / V (query blocks) tiles.  In sequence-major order one sequence's blocks were dealt over all 8 XCDs, every XCD's
    4 MB L2 saw every sequence, and the launch fetched 674 MB from HBM / MALL for ~100 MB of operands at the benchmark batch
    (profiles/r04_train_pmc.txt).  Sequences go to 8 lists (greedy by block count), entry i of the table comes from list i % 8; when the
    short lists run out the rest follows in list order (no padding entries: the kernels take the table as it is)."""
    if not switches.flag("TTV_BWD_XCD", True):       # A/B: sequence-major order
        return np.asarray([e for u in units for e in u], dtype=np.int32).reshape(-1, 2)
    lists = [[e for i in dealt for e in units[i]] for dealt in _deal_xcd([len(u) for u in units])]
    depth = min(len(l) for l in lists)
    out = [lists[x][k] for k in range(depth) for x in range(8)]
    for l in lists:
        out.extend(l[depth:])
    return np.asarray(out, dtype=np.int32).reshape(-1, 2)


PAD4 = (-1, -1, -1, -1)     # padding entry of the 4-wide attention work tables: sequence -1, the kernel returns at once


def _xcd_table(lists, pad_row, device) -> torch.Tensor:
    """Eight per-list entry sequences -> the flat int32 [n, len(pad_row)] table on `device`: entry i comes from list i % 8, shorter
    lists are padded with `pad_row`, and only the padding entries behind the last real one are dropped (interior padding keeps the
    i % 8 alignment).  Table::write of the port."""
    depth = max(len(l) for l in lists)
    table = np.empty((depth, 8, len(pad_row)), dtype=np.int32)
    table[:] = pad_row
    for x, l in enumerate(lists):
        if l:
            table[: len(l), x, :] = np.asarray(l, dtype=np.int32)
    last = max((len(l) - 1) * 8 + x + 1 for x, l in enumerate(lists) if l)
    return _upload(np.ascontiguousarray(table.reshape(-1, len(pad_row))[:last]), device)


class _Unit(NamedTuple):
    """One (sequence, kv-head) unit of a 4-wide attention work table, as the port's Unit: full items of the query blocks [f0, f1) first;
    behind ALL first parts of its XCD list the blocks [s0, s1), as full items or (second_half) as half items: two per block and q-head,
    the second only where its 64 rows begin inside the sequence."""
    b: int
    kvh: int
    length: int
    f0: int
    f1: int
    s0: int
    s1: int
    second_half: bool


def _attn_units_table(units: List[_Unit], rep: int, device) -> torch.Tensor:
    """int32 [n,4] attention work table (sequence, first query row, q-head, mode) of these units on `device`.  A unit keeps one XCD list
    for both its parts and weighs 2 * full + half items (Table::finish of the port: the order of full + half / 2, in integers)."""
    first, second = [], []
    for u in units:
        heads = range(u.kvh * rep, u.kvh * rep + rep)
        first.append([(u.b, qb * QBLOCK, hd, 0) for qb in range(u.f0, u.f1) for hd in heads])
        if u.second_half:
            second.append([(u.b, q0, hd, 1) for qb in range(u.s0, u.s1) for hd in heads for q0 in (qb * QBLOCK, qb * QBLOCK + 64) if q0 < u.length])
        else:
            second.append([(u.b, qb * QBLOCK, hd, 0) for qb in range(u.s0, u.s1) for hd in heads])
    dealt = _deal_xcd([2 * len(f) + (1 if u.second_half else 2) * len(h) for u, f, h in zip(units, first, second)])
    return _xcd_table([[e for part in (first, second) for i in l for e in part[i]] for l in dealt], PAD4, device)


class _PlanBase:
    """What the two builders of a plan share: the normalised arguments and the patch grids, the stream ownership of the device tables
    (streams.py), and the views into `int_tables`.  A builder checks its arguments in `_check_arguments`, then fills `int_tables`,
    `_offs` (word offsets of cu_seqlens, latent_rows, patch_rows, clip_desc, blocks64, row_seq, rope_ids), `rope_cs`, `_rope_by_id`
    and, on a GPU, `_owned`."""

    def __init__(self, pixel_grids: Sequence[Sequence[int]], token_counts: Sequence[int], patch: Sequence[int],
                 device: torch.device, head_dim: int = 64):
        if head_dim != 64:
            raise ValueError("head_dim is fixed at 64 (reference model/base/utils.py:8)")
        self.device = torch.device(device)
        self.patch = tuple(int(p) for p in patch)
        self.pixel_grids = [tuple(int(v) for v in g) for g in pixel_grids]
        self.token_counts = [int(k) for k in token_counts]
        self._check_arguments()
        self.grids = [tuple(v // p for v, p in zip(pg, self.patch)) for pg in self.pixel_grids]
        self.grid_sizes = [math.prod(g) for g in self.grids]
        self._attn = {}
        self._owned: Optional[streams.StreamOwned] = None       # host plans own no stream
        self._rope_by_id = (None, None)                         # device pointers (ttv_batch.rope_ids, rope_base), or None twice

    def _check_arguments(self) -> None:
        """ValueError, in the builder's own words, unless every clip shape is a positive multiple of the patch and has a count >= 0."""
        raise NotImplementedError

    def use_on_current_stream(self) -> None:
        """Stream safety of the cached plan (see ForwardPipeline): wait for the build on foreign streams, remember the readers."""
        if self._owned is not None:
            self._owned.use(torch.cuda.current_stream(self.device))

    def retire(self) -> None:
        """Before the tables are released (cache eviction): the releasing stream and the build stream wait for every stream that read them."""
        if self._owned is not None:
            self._owned.retire(torch.cuda.current_stream(self.device))

    def uniform_geometry(self) -> Optional[tuple]:
        """(patch grid, latent count, rotary id table size) when every clip of the batch has the same patch grid and latent count, else
        None: what the rows of a decoder's constant block (ttv_dec_l0_const) depend on besides the weights."""
        g, k = self.grids[0], self.token_counts[0]
        if any(gb != g for gb in self.grids) or any(kb != k for kb in self.token_counts):
            return None
        return (g, k, self.n_rope_ids)

    def clip0_patch_rope(self) -> Tuple[int, Optional[int], Optional[int]]:
        """Device pointers to the rotary tables of the FIRST clip's patch rows: (rope_cs rows, rope_ids rows or None, rope_base or None)."""
        k = self.token_counts[0]
        ids, base = self._rope_by_id
        return (self.rope_cs.data_ptr() + 4 * self.rope_cs.shape[1] * k, ids + 8 * k if ids else None, base if ids else None)

    # views used by tests that call single ops
    def table(self, i: int, n: int) -> torch.Tensor:
        return self.int_tables[self._offs[i]: self._offs[i] + n]

    @property
    def cu_dev(self):
        return self.table(0, len(self.cu_seqlens))

    @property
    def latent_rows_dev(self):
        return self.table(1, self.sum_tokens)

    @property
    def patch_rows_dev(self):
        return self.table(2, self.sum_patches)

    @property
    def clip_desc_dev(self):
        return self.table(3, 8 * len(self.grids))


class BatchPlan(_PlanBase):
    """Device tables + the ttv_batch struct for one (clip shapes, token counts) combination."""

    def _check_arguments(self) -> None:
        if len(self.pixel_grids) != len(self.token_counts) or not self.pixel_grids:
            raise ValueError("need one token count per clip and at least one clip")
        for pg in self.pixel_grids:
            if len(pg) != len(self.patch) or any(v <= 0 or v % p for v, p in zip(pg, self.patch)):
                raise ValueError(f"clip shape {pg} is not a positive multiple of patch size {self.patch}")
        if any(k < 0 for k in self.token_counts):
            raise ValueError("token counts must be >= 0")

    def __init__(self, pixel_grids: Sequence[Sequence[int]], token_counts: Sequence[int], patch: Sequence[int],
                 device: torch.device, head_dim: int = 64):
        super().__init__(pixel_grids, token_counts, patch, device, head_dim)
        grids, sizes = self.grids, self.grid_sizes
        B = len(grids)
        cu = [0]
        for k, p in zip(self.token_counts, sizes):
            if k + p <= 0:
                raise ValueError("empty sequence")
            cu.append(cu[-1] + k + p)
        self.cu_seqlens = cu
        self.total_rows = cu[-1]
        self.sum_tokens = sum(self.token_counts)
        self.sum_patches = sum(sizes)
        self.max_seqlen = max(k + p for k, p in zip(self.token_counts, sizes))

        latent_rows = np.concatenate([np.arange(cu[b], cu[b] + self.token_counts[b], dtype=np.int32) for b in range(B)])
        patch_rows = np.concatenate([np.arange(cu[b] + self.token_counts[b], cu[b + 1], dtype=np.int32) for b in range(B)])
        desc = np.zeros((B, 8), dtype=np.int32)
        pbase = 0
        for b in range(B):
            T, H, W = self.pixel_grids[b]
            desc[b] = (T, H, W, grids[b][0], grids[b][1], grids[b][2], pbase, 3)
            pbase += sizes[b]
        # rotary position ids per row (rope.py:59-67), four uint16 per row = two int32: (t | h << 16, w | identity << 16)
        n_ids = 512
        while n_ids < max(k + max(g) for g, k in zip(grids, self.token_counts)) + 1:
            n_ids *= 2
        self.n_rope_ids = n_ids
        # (per clip cached by (grid, K, table size): the loader's batches repeat a handful of clip shapes, and a step that needs three new
        # plans at ~5 clips is bound by this host code)
        ids = np.concatenate([_clip_rope_ids(grids[b], self.token_counts[b], n_ids) for b in range(B)], axis=0)
        rope_ids = ids.view(np.int32).reshape(-1)
        blocks64 = _xcd_interleave([[(b, r0) for r0 in range(0, cu[b + 1] - cu[b], 64)] for b in range(B)])
        row_seq = np.concatenate([np.full(cu[b + 1] - cu[b], b, dtype=np.int32) for b in range(B)])
        self.n_blocks64 = int(blocks64.shape[0])
        parts = [np.asarray(cu, dtype=np.int32), latent_rows, patch_rows, desc.reshape(-1), blocks64.reshape(-1), row_seq, rope_ids]
        offs, total = [], 0
        for p in parts:
            offs.append(total)
            total += (p.size + 3) // 4 * 4      # keep every table 16-byte aligned
        host = np.zeros(total, dtype=np.int32)
        for o, p in zip(offs, parts):
            host[o:o + p.size] = p
        self.int_tables = _upload(host, self.device)
        base = self.int_tables.data_ptr()
        if self.device.type == "cuda":
            # gather on the device from the (cached, device-resident) base table: no per-batch trigonometry, no big upload
            bc, bs = _rope_base_device(head_dim, len(self.patch), n_ids, str(self.device))
            self.rope_cs = torch.empty((self.total_rows, head_dim), dtype=torch.float32, device=self.device)
            rc = _lib.lib().ttv_rope_table_build(bc.data_ptr(), bs.data_ptr(), n_ids, bc.shape[1], base + 4 * offs[3], base + 4 * offs[0],
                                                 base + 4 * offs[5], self.rope_cs.data_ptr(), self.total_rows,
                                                 _lib.stream_ptr(self.device))
            _lib.check(rc, "ttv_rope_table_build")
            # the table is written by a kernel on the building stream: other streams wait for this event before their first use
            build = torch.cuda.current_stream(self.device)
            self._owned = streams.StreamOwned(build, build.record_event())
        else:   # host tensors (CPU-side tests of the plan): same table, gathered with numpy
            rope = np.concatenate([_rope_clip_table(g, k, head_dim) for g, k in zip(grids, self.token_counts)], axis=0)
            self.rope_cs = torch.from_numpy(rope).to(self.device)

        self._base_fields = dict(
            n_clips=B, total_rows=self.total_rows, sum_tokens=self.sum_tokens, sum_patches=self.sum_patches,
            max_patches_per_clip=max(sizes),
            # (ttv_batch.tokens_per_clip: the promise that every clip has this K and the same number of patches)
            tokens_per_clip=self.token_counts[0] if len(set(self.token_counts)) == 1 and len(set(sizes)) == 1 else 0,
            cu_seqlens=base + 4 * offs[0], latent_rows=base + 4 * offs[1], patch_rows=base + 4 * offs[2],
            clip_desc=base + 4 * offs[3], rope_cs=self.rope_cs.data_ptr(),
            blocks64=base + 4 * offs[4], row_seq=base + 4 * offs[5], n_blocks64=self.n_blocks64)
        # rotary factors by position id (ttv_batch.rope_ids / rope_base): the width-256 to_qkv kernel reads 8 bytes per row and gathers
        # from the cached base table instead of streaming the 256-byte fp32 row of rope_cs (TTV_ROPE_IDS=0: the table path, A/B)
        if self.device.type == "cuda" and len(self.patch) == 3 and switches.flag("TTV_ROPE_IDS", True):
            self._rope_base_cs = _rope_base_interleaved(head_dim, len(self.patch), n_ids, str(self.device))
            self._rope_by_id = (base + 4 * offs[6], self._rope_base_cs.data_ptr())
            self._base_fields.update(rope_ids=self._rope_by_id[0], rope_base=self._rope_by_id[1])
        self._offs = offs
        self._attn_all_full = {}
        self._batch_structs = {}

    def _sequences(self):
        """(b, length, query blocks, query blocks that hold latent rows only) of every sequence."""
        for b, k in enumerate(self.token_counts):
            s = self.cu_seqlens[b + 1] - self.cu_seqlens[b]
            yield b, s, -(-s // QBLOCK), k // QBLOCK

    def attention_table(self, q_heads: int, kv_heads: int, split: Optional[bool] = None) -> torch.Tensor:
        """int32 [n,4] attention work table (sequence, first query row, q-head, mode) for this batch, XCD-aware.

        Workgroups are dealt round-robin over the 8 XCDs (MI355X_MICROARCH.md: blocks b and b+8 share an XCD - a speed
        assumption only, never correctness).  All blocks of one (sequence, kv-head) unit re-read the same K/V, so units
        are distributed over 8 lists (greedy by block count) and the lists are interleaved: entry i goes to list i % 8.
        Shorter lists are padded with sequence = -1 entries (the kernel returns immediately).

        Half items (mode 1: 64 query rows, the key range split between the wave pairs of the block and merged in LDS) cost
        ~0.6 of a full item for half the work.  They pay when the grid alone cannot fill the part: with fewer items than the
        ATTN_SLOTS = 1024 blocks that are resident at once (batches below ~28 benchmark-size clips, e.g. the reference's
        6144-token training batches) the last third of every sequence's query blocks is issued as half items and the launch
        gets shorter (5 clips: 33 -> 27 us).  Larger grids keep full items: with a second batch in flight (pipeline.py) the
        tail of one launch is filled by the other chain and the extra work of half items only costs (-3 % measured), alone
        they are worth +1 % (TTV_ATTN_TAIL_DIV=8 halves the last eighth of every sequence's blocks on large grids: exactly
        the 128 items beyond 1024 slots at the benchmark batch, +1.5 % one batch at a time, -1 % with two in flight).  Within either regime the choice depends only on the sequence's own length, so a clip's bf16
        result does not depend on what it is packed with (the fp32 kernel computes the same way in both modes).
        `split`: None = that rule, False = never, True = every item (tests)."""
        if split is None and switches.text("TTV_ATTN_SPLIT") in ("0", "1"):      # diagnostics: A/B timing of the table kinds
            split = switches.text("TTV_ATTN_SPLIT") == "1"
        key = (int(q_heads), int(kv_heads), split)
        t = self._attn.get(key)
        if t is None:
            n_items = sum(nq for _b, _s, nq, _lat in self._sequences()) * q_heads
            tail_div = 3 if n_items < ATTN_SLOTS else switches.integer("TTV_ATTN_TAIL_DIV", 0)
            units = []
            for b, s, nq, _lat in self._sequences():
                first_half = 0 if split else (nq if (split is False or tail_div <= 0) else nq - nq // tail_div)
                units += [_Unit(b, kvh, s, 0, first_half, first_half, nq, True) for kvh in range(kv_heads)]
            t = self._attn[key] = _attn_units_table(units, q_heads // kv_heads, self.device)
            self._attn_all_full[t.data_ptr()] = all(u.s0 == u.s1 for u in units)      # no half item
        return t

    def attention_table_latent(self, q_heads: int, kv_heads: int) -> torch.Tensor:
        """int32 [n,4] attention work table like `attention_table`, restricted to the query blocks that hold LATENT tokens (rows
        [0, K_b) of every sequence; full items only).  The encoder reads its output from the latent rows alone (reference
        blocks.py:101-103), so its last layer needs attention outputs for these query rows only (`ttv_batch.qblocks_latent`): at the
        benchmark shape 128 entries instead of 1152.  Same XCD interleaving as the full table (a (sequence, kv-head) unit keeps one list)."""
        key = ("latent", int(q_heads), int(kv_heads))
        t = self._attn.get(key)
        if t is None:
            # blocks [0, ceil(K_b / 128)) hold latent rows
            units = [_Unit(b, kvh, s, 0, -(-self.token_counts[b] // QBLOCK), 0, 0, False) for b, s, _nq, _lat in self._sequences() for kvh in range(kv_heads)]
            t = self._attn[key] = _attn_units_table(units, q_heads // kv_heads, self.device)
        return t

    def attention_table_patch(self, q_heads: int, kv_heads: int) -> Optional[torch.Tensor]:
        """int32 [n,4] attention work table like `attention_table` (full items only) WITHOUT the query blocks that hold latent rows only
        (block q of sequence b with (q + 1) * 128 <= K_b), or None when no sequence has such a block.  The decoder reads its output from
        the patch rows alone (reference blocks.py:171), so its last layer needs no attention output for those query rows
        (`ttv_batch.qblocks_patch`): at the benchmark shape 1024 entries instead of 1152.  Same XCD interleaving as the full table."""
        key = ("patch", int(q_heads), int(kv_heads))
        if key not in self._attn:
            # blocks [0, lat) hold latent rows only; a table only when a block was dropped and one remains
            units = [_Unit(b, kvh, s, lat, nq, 0, 0, False) for b, s, nq, lat in self._sequences() for kvh in range(kv_heads)]
            dropped, remains = any(u.f0 > 0 for u in units), any(u.f0 < u.f1 for u in units)
            self._attn[key] = _attn_units_table(units, q_heads // kv_heads, self.device) if dropped and remains else None
        return self._attn[key]

    def attention_table_l0(self, q_heads: int, kv_heads: int) -> torch.Tensor:
        """int32 [n,4] attention work table like `attention_table` (full items only) for the decoder's layer 0 with a constant block
        (`ttv_dec_l0_const.qblocks`): every XCD list holds the LATENT query blocks of its (sequence, kv-head) units first - they loop over
        every key - and the patch query blocks, which loop over the latent keys only, behind them, so the long items start first."""
        key = ("l0", int(q_heads), int(kv_heads))
        t = self._attn.get(key)
        if t is None:
            units = [_Unit(b, kvh, s, 0, lat, lat, nq, False) for b, s, nq, lat in self._sequences() for kvh in range(kv_heads)]
            t = self._attn[key] = _attn_units_table(units, q_heads // kv_heads, self.device)
        return t

    def attention_table64(self, q_heads: int, kv_heads: int) -> torch.Tensor:
        """int32 [n,8] work table of ttv_attention64 (the 64-query-rows-per-wave kernel): one entry per workgroup =
        (sequence, kv-head, 4 x wave item, first packed row of the sequence, its length); a wave item is
        q-head | (first query row // 64) << 8, or -1 for an idle wave.

        All wave items of one (sequence, kv-head) unit - every 64-row slice of every q-head of the group - read the same K / V, so a
        unit's items are dealt four at a time to workgroups (the four waves of a workgroup share each K / V tile through LDS) and the
        unit's workgroups go to one of 8 lists (greedy by count); entry i of the flat table belongs to list i % 8 (blocks b, b + 8
        share an XCD under round-robin dispatch: L2 affinity only, never correctness).  Shorter lists are padded with sequence -1."""
        key = ("w64", int(q_heads), int(kv_heads))
        t = self._attn.get(key)
        if t is None:
            rep = q_heads // kv_heads
            units = []
            for b, s, _nq, _lat in self._sequences():
                n64 = -(-s // 64)
                for kvh in range(kv_heads):
                    items = [(kvh * rep + r) | (q << 8) for q in range(n64) for r in range(rep)]
                    items += [-1] * (-len(items) % 4)
                    units.append([(b, kvh, *items[i:i + 4], self.cu_seqlens[b], s) for i in range(0, len(items), 4)])
            dealt = _deal_xcd([len(u) for u in units])
            t = self._attn[key] = _xcd_table([[e for i in l for e in units[i]] for l in dealt], (-1, 0, 0, 0, 0, 0, 0, 0), self.device)
        return t

    def batch_for(self, q_heads: int, kv_heads: int) -> "_lib.Batch":
        """ttv_batch struct whose attention work table matches the tower's head counts (built once per head counts: every tower call of a
        step asks for it, and a ctypes struct of ~30 fields is 40 us of host time in a step that is launch-bound at small batches)."""
        skey = (int(q_heads), int(kv_heads)) + tuple(switches.text(k) for k in ("TTV_ATTN_SPLIT", "TTV_ATTN_PAIRED", "TTV_ATTN64", "TTV_ATTN_TAIL_DIV"))
        cached = self._batch_structs.get(skey)       # (the diagnostic switches that pick the tables are part of the key)
        if cached is not None:
            return cached
        t = self.attention_table(q_heads, kv_heads)
        # every (sequence, kv-head) unit contributes its entries in runs of `rep` q-heads per query block, full items first:
        # with an even rep, entries 2j and 2j+1 of an XCD list are two q-heads of one kv-head on the same query rows
        # (opt-in, TTV_ATTN_PAIRED=1: the 8-wave blocks halve the K/V tile traffic - +1.5 % with two batches in flight - but make
        # the grid coarser: the launch alone is 10 % slower)
        paired = 1 if (q_heads // kv_heads) % 2 == 0 and switches.flag("TTV_ATTN_PAIRED", False) else 0
        all_full = 1 if self._attn_all_full.get(t.data_ptr()) else 0
        # the 64-rows-per-wave kernel (ttv_attention64) for inference towers with pre-scaled q: OPT-IN (TTV_ATTN64=1).  Measured in
        # round 3 (profiles/r03_attn64_stamps.txt): per SIMD its key loop needs ~1 060 cycles per 32-query x
        # 64-key unit at two waves per SIMD against ~885 for the 32-rows-per-wave kernel at three, a block's prologue + epilogue
        # are 18 % of its life and 576 workgroups on 512 resident slots leave a tail: 77-80 us against 60-62 us at the benchmark
        # batch; at S = 9216 both kernels reach the same 0.37 of the MFMA peak (1 119 vs 1 120 us).
        t64 = self.attention_table64(q_heads, kv_heads) if (q_heads <= 255 and switches.flag("TTV_ATTN64", False)) else None
        # the encoder's last layer on its latent rows only (ttv_batch.qblocks_latent; TTV_ENC_LATENT_LAST=0 in the library: A/B)
        tl = self.attention_table_latent(q_heads, kv_heads) if sum(int(k) for k in self.token_counts) > 0 else None
        # the decoder's last layer without the query blocks that hold latent rows only (ttv_batch.qblocks_patch; TTV_DEC_PATCH_LAST=0: A/B)
        # (only beside a table of full items: the last layer must run the kernel, and the item kind, the all-blocks forward runs)
        tp = self.attention_table_patch(q_heads, kv_heads) if all_full else None
        self._batch_structs[skey] = out = _lib.Batch(n_qblocks=int(t.shape[0]), qblocks=t.data_ptr(), qblocks_paired=paired, qblocks_all_full=all_full,
                          items64=t64.data_ptr() if t64 is not None else None, n_items64=int(t64.shape[0]) if t64 is not None else 0,
                          qblocks_latent=tl.data_ptr() if tl is not None else None, n_qblocks_latent=int(tl.shape[0]) if tl is not None else 0,
                          qblocks_patch=tp.data_ptr() if tp is not None else None, n_qblocks_patch=int(tp.shape[0]) if tp is not None else 0,
                          **self._base_fields)
        return out


# ---- the same plan built by the library (ttv_plan_* of include/titok_hip.h): TTV_NATIVE_PLAN=1 -------------------------------------------
def _i32s(values) -> "C.Array":
    return (C.c_int32 * len(values))(*values)


def _split_code(split: Optional[bool]) -> int:
    return -1 if split is None else (1 if split else 0)


def native_host_tables(pixel_grids, token_counts, patch, q_heads: int, kv_heads: int, split: Optional[bool] = None, tail_div: int = 0,
                       bwd_xcd: bool = True) -> dict:
    """The library's host-only plan calls (no device): the sizes, the host segment's tables and the attention work tables of one
    (q_heads, kv_heads) as numpy arrays.  What a C host computes before it touches the GPU; tests/test_native_plan_cpu.py holds it to
    BatchPlan, tools/plan_host_time.py times it."""
    lib = _lib.lib()
    n = len(pixel_grids)
    dims, counts, pt = _i32s([int(v) for g in pixel_grids for v in g]), _i32s([int(k) for k in token_counts]), _i32s([int(p) for p in patch])
    sz = _lib.PlanSizes()
    _lib.check(lib.ttv_plan_rows_sizes(dims, counts, n, pt, C.byref(sz)), "ttv_plan_rows_sizes")
    seg = np.empty(int(sz.host_words), dtype=np.int32)
    _lib.check(lib.ttv_plan_rows_fill(dims, counts, n, pt, 1 if bwd_xcd else 0, seg.ctypes.data, seg.size), "ttv_plan_rows_fill")
    cu = seg[sz.off_cu_seqlens: sz.off_cu_seqlens + n + 1]
    az = _lib.PlanAttn()
    args = (cu.ctypes.data, counts, n, int(q_heads), int(kv_heads), _split_code(split), int(tail_div))
    _lib.check(lib.ttv_plan_attn_sizes(*args, C.byref(az)), "ttv_plan_attn_sizes")
    tab = np.empty(int(az.words), dtype=np.int32)
    _lib.check(lib.ttv_plan_attn_fill(*args, tab.ctypes.data, tab.size), "ttv_plan_attn_fill")

    def part(off, entries):
        return tab[off: off + 4 * entries].reshape(-1, 4) if entries else None
    out = {k: int(getattr(sz, k)) for k, _ in _lib.PlanSizes._fields_}
    out.update(cu_seqlens=cu, clip_desc=seg[sz.off_clip_desc: sz.off_clip_desc + 8 * n].reshape(n, 8),
               blocks64=seg[sz.off_blocks64: sz.off_blocks64 + 2 * sz.n_blocks64].reshape(-1, 2), host_segment=seg,
               qblocks=part(az.off_qblocks, az.n_qblocks), qblocks_all_full=int(az.qblocks_all_full),
               qblocks_latent=part(az.off_qblocks_latent, az.n_qblocks_latent), qblocks_patch=part(az.off_qblocks_patch, az.n_qblocks_patch),
               qblocks_l0=part(az.off_qblocks_l0, az.n_qblocks_l0))
    return out


_STAGE_MAX_SLOTS = 64       # pinned staging buffers per device (64 KiB each unless a segment is larger): a training step takes ~6, and the host runs several steps ahead of the GPU
_STAGE_MIN_WORDS = 1 << 14


class _StageRing:
    """Pinned host buffers for the segments the library copies to the device (ttv_plan_rows_build, ttv_plan_attn_set).  The copy is only
    queued when the call returns, so a slot carries the event recorded behind its copy and is rewritten only once that event has
    completed (as optim._Tables guards its slots).  A busy oldest slot is not waited for: the ring grows up to _STAGE_MAX_SLOTS, and
    only a host that is that many segments ahead of the GPU waits - for the oldest copy alone, never for a stream."""

    def __init__(self):
        self.slots = []
        self.next = 0

    def take(self, words: int) -> dict:
        # slots are handed out in ring order and their copies complete in that order (per stream), so only the oldest is looked at
        n = len(self.slots)
        slot = self.slots[self.next] if n else None
        if slot is not None and (slot["event"] is None or slot["event"].query()):
            self.next = (self.next + 1) % n
        elif n < _STAGE_MAX_SLOTS:
            slot = {"host": None, "event": None, "words": 0}
            self.slots.insert(self.next, slot)      # (in front of the oldest, which stays the next one to be looked at)
            self.next = (self.next + 1) % (n + 1)
        else:
            self.next = (self.next + 1) % n
            slot["event"].synchronize()
        slot["event"] = None
        if slot["words"] < words:       # (the slot's last copy has run: its buffer may go)
            cap = max(int(words), _STAGE_MIN_WORDS)
            slot["host"] = torch.empty(cap, dtype=torch.int32).pin_memory()
            slot["np"], slot["ptr"], slot["words"] = slot["host"].numpy(), slot["host"].data_ptr(), cap
        return slot


_stage_rings = {}


def _stage_ring(device) -> _StageRing:
    ring = _stage_rings.get(str(device))
    if ring is None:
        ring = _stage_rings[str(device)] = _StageRing()
    return ring


class NativeBatchPlan(_PlanBase):
    """BatchPlan's device tables and ttv_batch structs, built by the library: the host writes cu_seqlens, the clip descriptors, the
    backward blocks and the attention work tables in C++ (csrc/ttv_plan_host.cpp) into pinned staging, the copies are queued on the
    building stream without waiting for them, and the per-row tables (latent_rows, patch_rows, row_seq, rope_ids) are written on the
    device by one kernel (csrc/ttv_plan.hip).  Same attributes and methods as BatchPlan, the same tables element for element
    (tests/test_native_plan_cpu.py, tests/test_hip_native_plan.py); GPU only, three patch axes.  items64 and the paired flag (opt-in
    kernels, TTV_ATTN64 / TTV_ATTN_PAIRED) are not built: the struct leaves them NULL / 0."""

    def _check_arguments(self) -> None:
        """The library's checks and message (ttv_plan_rows_sizes); its sizes and the ctypes arrays of the arguments are kept."""
        if self.device.type != "cuda" or len(self.patch) != 3:
            raise ValueError("NativeBatchPlan: GPU plans with three patch axes only (BatchPlan builds the others)")
        if len(self.pixel_grids) != len(self.token_counts) or not self.pixel_grids or any(len(g) != 3 for g in self.pixel_grids):
            raise ValueError("need one token count per clip, at least one clip, and three dimensions per clip")
        lib = _lib.lib()
        self._counts = _i32s(self.token_counts)
        self._dims, self._pt = _i32s([v for g in self.pixel_grids for v in g]), _i32s(self.patch)
        self._sizes = _lib.PlanSizes()
        if lib.ttv_plan_rows_sizes(self._dims, self._counts, len(self.pixel_grids), self._pt, C.byref(self._sizes)) != 0:
            raise ValueError(lib.ttv_error_string().decode("utf-8", "replace"))

    def __init__(self, pixel_grids: Sequence[Sequence[int]], token_counts: Sequence[int], patch: Sequence[int],
                 device: torch.device, head_dim: int = 64):
        super().__init__(pixel_grids, token_counts, patch, device, head_dim)
        lib, sz, dims, pt = _lib.lib(), self._sizes, self._dims, self._pt
        B = len(self.pixel_grids)
        self.total_rows, self.sum_tokens, self.sum_patches = int(sz.total_rows), int(sz.sum_tokens), int(sz.sum_patches)
        self.max_seqlen, self.n_rope_ids, self.n_blocks64 = int(sz.max_seqlen), int(sz.n_rope_ids), int(sz.n_blocks64)
        self._ring = _stage_ring(self.device)
        slot = self._ring.take(int(sz.host_words))
        _lib.check(lib.ttv_plan_rows_fill(dims, self._counts, B, pt, 1 if switches.flag("TTV_BWD_XCD", True) else 0, slot["ptr"], slot["words"]),
                   "ttv_plan_rows_fill")
        self.cu_seqlens = slot["np"][sz.off_cu_seqlens: sz.off_cu_seqlens + B + 1].tolist()
        self._cu = _i32s(self.cu_seqlens)
        self.int_tables = torch.empty(int(sz.dev_words), dtype=torch.int32, device=self.device)
        self.rope_cs = torch.empty((self.total_rows, head_dim), dtype=torch.float32, device=self.device)
        bc, bs = _rope_base_device(head_dim, 3, self.n_rope_ids, str(self.device))
        # rotary factors by position id beside the table, as in BatchPlan (TTV_ROPE_IDS=0: the table path alone, A/B)
        self._rope_base_cs = _rope_base_interleaved(head_dim, 3, self.n_rope_ids, str(self.device)) if switches.flag("TTV_ROPE_IDS", True) else None
        self._base = _lib.Batch()
        build = torch.cuda.current_stream(self.device)
        rc = lib.ttv_plan_rows_build(C.byref(sz), slot["ptr"], self.int_tables.data_ptr(), bc.data_ptr(), bs.data_ptr(), bc.shape[1],
                                     self.rope_cs.data_ptr(), _lib.ptr(self._rope_base_cs), C.byref(self._base), build.cuda_stream)
        # the tables are written by a copy and two kernels on the building stream: other streams wait for this event before their
        # first use, and the staging slot is rewritten only once it has completed
        self._owned = streams.StreamOwned(build, build.record_event())
        slot["event"] = self._owned.ready
        _lib.check(rc, "ttv_plan_rows_build")
        self._rope_by_id = (self._base.rope_ids, self._base.rope_base)
        self._offs = [int(o) for o in (sz.off_cu_seqlens, sz.off_latent_rows, sz.off_patch_rows, sz.off_clip_desc, sz.off_blocks64,
                                       sz.off_row_seq, sz.off_rope_ids)]

    def _tables(self, q_heads: int, kv_heads: int, split: Optional[bool], tail_div: int) -> dict:
        """The four attention work tables of these head counts on the device (one buffer), with the ttv_batch that points at them.
        Copied on the building stream, whose pool owns every table of the plan (retire); any other stream waits for the copy's event."""
        key = (int(q_heads), int(kv_heads), split, int(tail_div))
        cur = torch.cuda.current_stream(self.device)
        ent = self._attn.get(key)
        if ent is None:
            lib = _lib.lib()
            az = _lib.PlanAttn()
            args = (self._cu, self._counts, len(self.grids), key[0], key[1], _split_code(split), key[3])
            _lib.check(lib.ttv_plan_attn_sizes(*args, C.byref(az)), "ttv_plan_attn_sizes")
            slot = self._ring.take(int(az.words))
            _lib.check(lib.ttv_plan_attn_fill(*args, slot["ptr"], slot["words"]), "ttv_plan_attn_fill")
            build = self._owned.build_stream
            if cur == build:
                dev = torch.empty(int(az.words), dtype=torch.int32, device=self.device)
            else:
                with torch.cuda.stream(build):
                    dev = torch.empty(int(az.words), dtype=torch.int32, device=self.device)
            batch = _lib.Batch.from_buffer_copy(self._base)
            rc = lib.ttv_plan_attn_set(C.byref(az), slot["ptr"], dev.data_ptr(), C.byref(batch), build.cuda_stream)
            slot["event"] = build.record_event()
            _lib.check(rc, "ttv_plan_attn_set")
            ent = self._attn[key] = dict(dev=dev, sizes=az, batch=batch, done=streams.EventOnce(build, slot["event"]))
        ent["done"].wait_once(cur)
        return ent

    def _switched(self, q_heads: int, kv_heads: int) -> dict:
        """The tables the diagnostics switches select (read here, passed down as arguments: the library reads no environment for this)."""
        s = switches.text("TTV_ATTN_SPLIT")
        return self._tables(q_heads, kv_heads, (s == "1") if s in ("0", "1") else None, switches.integer("TTV_ATTN_TAIL_DIV", 0))

    @staticmethod
    def _view(ent: dict, off: int, entries: int) -> Optional[torch.Tensor]:
        return ent["dev"][off: off + 4 * entries].view(-1, 4) if entries else None

    def attention_table(self, q_heads: int, kv_heads: int, split: Optional[bool] = None) -> torch.Tensor:
        ent = self._switched(q_heads, kv_heads) if split is None else self._tables(q_heads, kv_heads, split, switches.integer("TTV_ATTN_TAIL_DIV", 0))
        return self._view(ent, ent["sizes"].off_qblocks, ent["sizes"].n_qblocks)

    def attention_table_latent(self, q_heads: int, kv_heads: int) -> Optional[torch.Tensor]:
        ent = self._switched(q_heads, kv_heads)
        return self._view(ent, ent["sizes"].off_qblocks_latent, ent["sizes"].n_qblocks_latent)

    def attention_table_patch(self, q_heads: int, kv_heads: int) -> Optional[torch.Tensor]:
        ent = self._switched(q_heads, kv_heads)
        return self._view(ent, ent["sizes"].off_qblocks_patch, ent["sizes"].n_qblocks_patch)

    def attention_table_l0(self, q_heads: int, kv_heads: int) -> torch.Tensor:
        ent = self._switched(q_heads, kv_heads)
        return self._view(ent, ent["sizes"].off_qblocks_l0, ent["sizes"].n_qblocks_l0)

    def batch_for(self, q_heads: int, kv_heads: int) -> "_lib.Batch":
        """ttv_batch struct whose attention work tables match the tower's head counts (ttv_plan_attn_set filled it)."""
        return self._switched(q_heads, kv_heads)["batch"]


_plan_cache = {}
_PLAN_CACHE_MAX = 64


def get_plan(pixel_grids, token_counts, patch, device) -> _PlanBase:
    dev = torch.device(device)
    # TTV_NATIVE_PLAN=1 (opt-in, read at call time and part of the key): the library builds the plan (NativeBatchPlan)
    native = switches.flag("TTV_NATIVE_PLAN", False) and dev.type == "cuda" and len(patch) == 3
    key = (tuple(tuple(int(v) for v in g) for g in pixel_grids), tuple(int(k) for k in token_counts),
           tuple(int(p) for p in patch), str(dev), native)
    plan = _plan_cache.get(key)
    if plan is None:
        if len(_plan_cache) >= _PLAN_CACHE_MAX:
            _plan_cache.pop(next(iter(_plan_cache))).retire()
        plan = (NativeBatchPlan if native else BatchPlan)(key[0], key[1], key[2], device)
        _plan_cache[key] = plan
    plan.use_on_current_stream()
    return plan


def host_ints(v) -> List[int]:
    """token_counts / grids as Python ints.  A device tensor costs one host sync (the reference syncs several times
    per tower for the same information); pass lists or CPU tensors to avoid it."""
    if isinstance(v, torch.Tensor):
        return v.detach().to("cpu").tolist()
    return [x.tolist() if hasattr(x, "tolist") else x for x in v]
