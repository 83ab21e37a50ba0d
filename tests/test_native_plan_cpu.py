"""The library's host-side plan builder (ttv_plan_rows_*, ttv_plan_attn_*, ttv_rope_base_table: csrc/ttv_plan_host.cpp) against
BatchPlan(device="cpu"), which stays the definition: every integer table with ==, the fp32 rotary base table bit for bit.  No
tolerance anywhere.  The calls touch no device, so all of this runs without a GPU."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

from titok_video_amd import _lib
from titok_video_amd.model.base.utils import get_model_dims
from titok_video_amd.plan import BatchPlan, _rope_base_table, native_host_tables

PATCH = (4, 8, 8)
HEADS = sorted({(4, 2), tuple(get_model_dims("tiny")[2]), tuple(get_model_dims("base")[2])})
BASE32 = ([(16, 128, 128)] * 32, [128] * 32)
RAGGED = ([(16, 128, 128), (8, 64, 96), (4, 8, 8), (12, 96, 128)], [128, 0, 1, 37])

# name -> (clip shapes, token counts, split, tail_div, bwd_xcd)
CASES = {
    "base32": BASE32 + (None, 0, True),                                        # large grid: full items, patch table present
    "small5": ([(16, 128, 128)] * 5, [128] * 5, None, 0, True),                # small grid: the last third as half items
    "ragged": RAGGED + (None, 0, True),                                        # K = 0, a 2-row sequence, lengths off 64 and 128
    "latent_blocks": ([(4, 128, 128), (8, 64, 64)], [256, 130], None, 0, True),  # latent-only query blocks, different per clip
    "k600": ([(8, 64, 64)], [600], None, 0, True),                             # n_rope_ids = 1024
    "base32_tail8": BASE32 + (None, 8, True),
    "ragged_split0": RAGGED + (False, 0, True),
    "ragged_split1": RAGGED + (True, 0, True),
    "base32_split0": BASE32 + (False, 0, True),
    "small5_split1": ([(16, 128, 128)] * 5, [128] * 5, True, 0, True),
    "ragged_no_bwd_xcd": RAGGED + (None, 0, False),
    "base32_no_bwd_xcd": BASE32 + (None, 0, False),
    # several (sequence, kv-head) units of equal weight between heavier and lighter ones: the stable order and the first-minimum rule
    "ties": ([(8, 64, 64), (16, 128, 128), (8, 64, 64), (8, 64, 64), (16, 128, 128), (4, 64, 64), (8, 64, 64)] * 2,
             [64, 128, 64, 64, 128, 64, 64] * 2, None, 0, True),
}


def _env(monkeypatch, split, tail_div, bwd_xcd):
    """BatchPlan reads these switches; the library takes them as arguments."""
    for name, value in (("TTV_ATTN_SPLIT", None if split is None else str(int(split))), ("TTV_ATTN_TAIL_DIV", str(tail_div) if tail_div else None),
                        ("TTV_BWD_XCD", None if bwd_xcd else "0"), ("TTV_ATTN_PAIRED", None), ("TTV_ATTN64", None)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)


def _same(native, expected, what):
    if expected is None:
        assert native is None, f"{what}: the library built a table BatchPlan does not have"
        return
    expected = np.asarray(expected)
    assert native is not None and native.dtype == np.int32 and native.shape == expected.shape, what
    assert np.array_equal(native, expected), what


def _compare(shapes, counts, split, tail_div, bwd_xcd, heads):
    ref = BatchPlan(shapes, counts, PATCH, "cpu")
    for hq, hkv in heads:
        nat = native_host_tables(shapes, counts, PATCH, hq, hkv, split=split, tail_div=tail_div, bwd_xcd=bwd_xcd)
        rb = ref.batch_for(hq, hkv)
        for name, want in (("n_clips", len(shapes)), ("total_rows", ref.total_rows), ("sum_tokens", ref.sum_tokens),
                           ("sum_patches", ref.sum_patches), ("max_patches_per_clip", rb.max_patches_per_clip),
                           ("max_seqlen", ref.max_seqlen), ("n_rope_ids", ref.n_rope_ids), ("n_blocks64", ref.n_blocks64)):
            assert nat[name] == want, name
        offsets = [nat[k] for k in nat if k.startswith("off_")] + [nat["host_words"], nat["dev_words"]]
        assert all(o % 4 == 0 for o in offsets), "every table starts 16-byte aligned"
        _same(nat["cu_seqlens"], ref.cu_seqlens, "cu_seqlens")
        _same(nat["clip_desc"], ref.clip_desc_dev.numpy().reshape(-1, 8), "clip_desc")
        _same(nat["blocks64"], ref.table(4, 2 * ref.n_blocks64).numpy().reshape(-1, 2), "blocks64")
        used = np.zeros(nat["host_words"], dtype=bool)
        for off, n in ((nat["off_cu_seqlens"], len(shapes) + 1), (nat["off_clip_desc"], 8 * len(shapes)), (nat["off_blocks64"], 2 * ref.n_blocks64)):
            used[off: off + n] = True
        assert not nat["host_segment"][~used].any(), "the words between the host tables are zero"
        _same(nat["qblocks"], ref.attention_table(hq, hkv).numpy(), "qblocks")
        assert nat["qblocks_all_full"] == rb.qblocks_all_full
        assert nat["qblocks"].shape[0] == rb.n_qblocks
        _same(nat["qblocks_latent"], ref.attention_table_latent(hq, hkv).numpy() if rb.qblocks_latent else None, "qblocks_latent")
        assert (0 if nat["qblocks_latent"] is None else nat["qblocks_latent"].shape[0]) == rb.n_qblocks_latent
        _same(nat["qblocks_patch"], ref.attention_table_patch(hq, hkv).numpy() if rb.qblocks_patch else None, "qblocks_patch")
        assert (0 if nat["qblocks_patch"] is None else nat["qblocks_patch"].shape[0]) == rb.n_qblocks_patch
        _same(nat["qblocks_l0"], ref.attention_table_l0(hq, hkv).numpy(), "layer-0 table")
    return ref


@pytest.mark.parametrize("name", list(CASES))
def test_named_cases_equal_batchplan(name, monkeypatch):
    shapes, counts, split, tail_div, bwd_xcd = CASES[name]
    _env(monkeypatch, split, tail_div, bwd_xcd)
    ref = _compare(shapes, counts, split, tail_div, bwd_xcd, HEADS)
    # what each case is there for
    tab = ref.attention_table(4, 2).numpy()
    real = tab[tab[:, 0] >= 0]
    if name == "base32":
        assert not real[:, 3].any() and ref.batch_for(4, 2).qblocks_patch
    if name == "small5":
        assert real[:, 3].any() and not real[:, 3].all()
    if name == "base32_tail8":
        assert real[:, 3].any()
    if name == "k600":
        assert ref.n_rope_ids == 1024
    if name == "latent_blocks":
        assert [k // 128 for k in counts] == [2, 1] and ref.batch_for(4, 2).n_qblocks_latent > 0
    if name == "ragged":
        assert 0 in counts and 2 in np.diff(ref.cu_seqlens) and any(s % 64 for s in np.diff(ref.cu_seqlens))


def test_seeded_ragged_batches_equal_batchplan(monkeypatch):
    """The 200 seeded batches of tests/probes/plan_host_probe.py: 4-7 clips of its six shapes, K in {32, 64, 128}."""
    _env(monkeypatch, None, 0, True)
    rng = random.Random(0)
    shapes = [(16, 128, 128), (8, 64, 96), (16, 64, 64), (4, 128, 96), (12, 96, 128), (16, 96, 96)]
    for _ in range(200):
        n = rng.randint(4, 7)
        g = [rng.choice(shapes) for _ in range(n)]
        c = [rng.choice([32, 64, 128]) for _ in range(n)]
        _compare(g, c, None, 0, True, [(4, 2)])


@pytest.mark.parametrize("n_ids", [512, 1024, 4096])
def test_rope_base_table_bit_for_bit(n_ids):
    want_c, want_s = _rope_base_table(64, 3, n_ids)
    cos, sin = np.full((n_ids, 10), np.nan, dtype=np.float32), np.full((n_ids, 10), np.nan, dtype=np.float32)
    _lib.check(_lib.lib().ttv_rope_base_table(64, 3, n_ids, 10000.0, cos.ctypes.data, sin.ctypes.data), "ttv_rope_base_table")
    assert want_c.shape == cos.shape and want_s.shape == sin.shape
    assert np.array_equal(cos.view(np.int32), want_c.view(np.int32)), f"{int((cos.view(np.int32) != want_c.view(np.int32)).sum())} cos entries differ"
    assert np.array_equal(sin.view(np.int32), want_s.view(np.int32)), f"{int((sin.view(np.int32) != want_s.view(np.int32)).sum())} sin entries differ"


CANARY = 0x5A5A5A5A


def _i32(*v):
    return (C.c_int32 * len(v))(*v)


@functools.lru_cache(maxsize=1)
def _good():
    return _i32(16, 128, 128, 8, 64, 96), _i32(128, 0), _i32(*PATCH)


ROWS_BAD = {
    "not a multiple of the patch": (lambda d, c, p: (_i32(16, 130, 128, 8, 64, 96), c, 2, p), b"not a positive multiple"),
    "zero dimension": (lambda d, c, p: (_i32(16, 128, 128, 0, 64, 96), c, 2, p), b"not a positive multiple"),
    "negative dimension": (lambda d, c, p: (_i32(16, 128, 128, -8, 64, 96), c, 2, p), b"not a positive multiple"),
    "negative count": (lambda d, c, p: (d, _i32(128, -1), 2, p), b"negative"),
    "no clips": (lambda d, c, p: (d, c, 0, p), b"no clips"),
    "null dims": (lambda d, c, p: (None, c, 2, p), b"null"),
    "null counts": (lambda d, c, p: (d, None, 2, p), b"null"),
    "null patch": (lambda d, c, p: (d, c, 2, None), b"null"),
    "zero patch": (lambda d, c, p: (d, c, 2, _i32(4, 0, 8)), b"patch"),
    "ids beyond uint16": (lambda d, c, p: (d, _i32(128, 40000), 2, p), b"uint16"),
}


@pytest.mark.parametrize("name", list(ROWS_BAD))
def test_invalid_rows_input_is_refused_and_writes_nothing(name):
    lib = _lib.lib()
    make, message = ROWS_BAD[name]
    args = make(*_good())
    sz = _lib.PlanSizes()
    C.memset(C.byref(sz), 0x5A, C.sizeof(sz))
    assert lib.ttv_plan_rows_sizes(*args, C.byref(sz)) == 1
    assert message in lib.ttv_error_string()
    assert bytes(sz) == b"\x5a" * C.sizeof(sz)
    seg = np.full(256, CANARY, dtype=np.int32)
    assert lib.ttv_plan_rows_fill(*args, 1, seg.ctypes.data, seg.size) == 1
    assert message in lib.ttv_error_string()
    assert (seg == CANARY).all()


def test_invalid_output_buffers_are_refused():
    lib = _lib.lib()
    d, c, p = _good()
    assert lib.ttv_plan_rows_sizes(d, c, 2, p, None) == 1 and b"null" in lib.ttv_error_string()
    assert lib.ttv_plan_rows_fill(d, c, 2, p, 1, None, 1 << 20) == 1 and b"null" in lib.ttv_error_string()
    sz = _lib.PlanSizes()
    assert lib.ttv_plan_rows_sizes(d, c, 2, p, C.byref(sz)) == 0
    seg = np.full(int(sz.host_words) + 8, CANARY, dtype=np.int32)
    assert lib.ttv_plan_rows_fill(d, c, 2, p, 1, seg.ctypes.data, int(sz.host_words) - 1) == 1 and b"too small" in lib.ttv_error_string()
    assert (seg == CANARY).all()
    assert lib.ttv_plan_rows_fill(d, c, 2, p, 1, seg.ctypes.data, int(sz.host_words)) == 0
    assert (seg[int(sz.host_words):] == CANARY).all(), "nothing behind the host segment is written"
    cu = _i32(0, 1152, 1248)
    az = _lib.PlanAttn()
    assert lib.ttv_plan_attn_sizes(cu, c, 2, 4, 2, -1, 0, C.byref(az)) == 0
    tab = np.full(int(az.words) + 8, CANARY, dtype=np.int32)
    assert lib.ttv_plan_attn_fill(cu, c, 2, 4, 2, -1, 0, tab.ctypes.data, int(az.words) - 1) == 1 and b"too small" in lib.ttv_error_string()
    assert (tab == CANARY).all()
    assert lib.ttv_plan_attn_fill(cu, c, 2, 4, 2, -1, 0, tab.ctypes.data, int(az.words)) == 0
    assert (tab[int(az.words):] == CANARY).all() and (tab[:int(az.words)] != CANARY).all()
    assert lib.ttv_rope_base_table(64, 3, 512, 10000.0, None, None) == 1 and b"null" in lib.ttv_error_string()
    assert lib.ttv_rope_base_table(64, 0, 512, 10000.0, tab.ctypes.data, tab.ctypes.data) == 1 and b"rope_base_table" in lib.ttv_error_string()


ATTN_BAD = {
    "empty sequence": ((_i32(0, 1152, 1152), _i32(128, 0), 2, 4, 2, -1, 0), b"empty sequence"),
    "shrinking cu_seqlens": ((_i32(0, 1152, 1000), _i32(128, 0), 2, 4, 2, -1, 0), b"empty sequence"),
    "negative count": ((_i32(0, 1152, 1248), _i32(128, -1), 2, 4, 2, -1, 0), b"token count"),
    "count beyond the sequence": ((_i32(0, 1152, 1248), _i32(128, 97), 2, 4, 2, -1, 0), b"token count"),
    "no clips": ((_i32(0, 1152, 1248), _i32(128, 0), 0, 4, 2, -1, 0), b"no clips"),
    "null cu_seqlens": ((None, _i32(128, 0), 2, 4, 2, -1, 0), b"null"),
    "null counts": ((_i32(0, 1152, 1248), None, 2, 4, 2, -1, 0), b"null"),
    "heads do not divide": ((_i32(0, 1152, 1248), _i32(128, 0), 2, 4, 3, -1, 0), b"heads"),
    "no heads": ((_i32(0, 1152, 1248), _i32(128, 0), 2, 0, 0, -1, 0), b"heads"),
    "split out of range": ((_i32(0, 1152, 1248), _i32(128, 0), 2, 4, 2, 2, 0), b"split"),
}


@pytest.mark.parametrize("name", list(ATTN_BAD))
def test_invalid_attention_input_is_refused_and_writes_nothing(name):
    lib = _lib.lib()
    args, message = ATTN_BAD[name]
    az = _lib.PlanAttn()
    C.memset(C.byref(az), 0x5A, C.sizeof(az))
    assert lib.ttv_plan_attn_sizes(*args, C.byref(az)) == 1
    assert message in lib.ttv_error_string()
    assert bytes(az) == b"\x5a" * C.sizeof(az)
    tab = np.full(4096, CANARY, dtype=np.int32)
    assert lib.ttv_plan_attn_fill(*args, tab.ctypes.data, tab.size) == 1
    assert message in lib.ttv_error_string()
    assert (tab == CANARY).all()
