"""The inference forward kernels at the shapes the benchmark launches, per block against float64 (`-m gpu`).

The benchmarked forward is three launches per layer (to_qkv + rotary, attention, the fused layer tail) over 32 x 1152 = 36 864 packed
rows, and the base towers at one 9 216-row sequence.  tests/test_hip_ops.py holds these kernels to one relative Frobenius error over
the whole output, against a float32 attention oracle, at sequences of at most 1 152 rows.  Here:

  * attention (`ttv_attention`, `ttv_attention64`): every route of the dispatch - unscaled k_attn_bf16 ("plain"), k_attn_swp ("swp"),
    pre-scaled k_attn_bf16 with the software pipeline bypassed ("bf16qs"), with the default work table ("mixed": half items on the
    5-clip batch) and with half items only ("half"), paired items ("paired"), k_attn_pipe ("pipe"), the 64-rows-per-wave kernel
    ("w64"), k_attn_f32 ("f32") and k_attn_split3 ("split3") - against tests/blockwise.py attention_forward_reference (float64 on the
    operands the kernel reads: for pre-scaled routes the pre-scaled q as rounded to bf16), per (sequence, head, 64-row block) and
    globally, gate on and off, on the batches of tests/forward_cases.py; far and spiked-direction query rows one by one
    (`check_rows`, per head); the restricted work tables (latent / patch query blocks): rows inside right, every other row of the
    NaN-filled output still NaN, nothing past the last row.
  * the dense launches of a layer at width 256 (`ttv_linear_qkv_rope`, `ttv_mlp_fused`, `ttv_layer_tail_fused` with and without the
    next layer's QKV, default deal and the forced 144-token deal) per 16-row x 64-column tile at M = 36 864, 36 865, 5 760, 1 025 and
    143, with rows scaled by 100, by 1e-3 and all-zero rows planted at the first rows, the end of the first tile, the middle and the
    very end.

Bounds.  Nothing is tuned against the kernels.
  * Attention bf16 / f32: FWD_TOL of tests/test_hip_backward_shapes.py (per block 6e-3 / 1e-5, global 4e-3 / 2e-6), every route the
    same.  A single (row, head) gets the block bound: an element's one bf16 store is at most 2^-9 = 1.95e-3 off, P's one rounding
    to bf16 in front of the PV product at most another 2^-9, and both fully correlated would be 3.9e-3.
  * split3: the kernel claims ~2^-17 per product (include/titok_hip.h) where fp32 has 2^-24.  A derivation through the 64-term dot
    product, the exponential (an absolute score error e is a relative error e in p) and the normalised sum depends on how peaked the
    row is and is not tight, so the bound is the ceiling: the f32 bound x 2^-17 / 2^-24 = 1.28e-3 per block, 2.56e-4 global; the
    measured figure is reported.
  * Dense kernels: a reference-only rounding model - the float64 definition with one bf16 store at the points the references of
    tests/test_hip_ops.py name (x1 as the residual stream, h in front of the w3 product, the stored y the next QKV reads, the final
    store) - against the same definition without any rounding is what the necessary roundings cost per tile; the bound of a case is
    2 x the model's worst tile (global: 2 x its global error), computed in the test.  The factor is for what the model leaves out
    (fp32 summation order, the fast GELU / rsqrt).  Planted rows: 2 x the model's error in that row; an all-zero input row has an
    exactly zero output (zero through every linear, 0 * rsqrt(eps) through every norm, gelu(0) * 0) and must be stored as zeros.
  * No block or tile of a forward reference may fall under the floor of `block_errors` (which would measure it against the floor, not
    itself); asserted from the reference alone before the launch.  Tiles that hold planted rows only are exempt (`check_rows`).

Measured on MI355X, worst over all cases (block / tile, global) next to the bound; the model figure is box-independent:
  attention, bound per block 6e-3 / global 4e-3 (a bf16 store of the float64 reference alone: worst block 1.96e-3, median 1.66e-3):
    plain   2.9e-3 / 2.3e-3      swp     5.5e-3 / 2.4e-3 (spikes30 4/2 ungated; 4.0e-3 on `ragged`: the least exact route)
    bf16qs  3.3e-3 / 2.4e-3      mixed   3.2e-3 / 2.4e-3      half    3.2e-3 / 2.3e-3      paired  3.3e-3 / 2.3e-3
    pipe    3.3e-3 / 2.3e-3      w64     3.3e-3 / 2.3e-3      swp, latent table 2.6e-3 / 2.4e-3, patch table 5.4e-3 / 2.4e-3
    worst far / spiked-direction (row, head): 4.5e-3 (swp), 3.4e-3 (every other bf16 route)
    f32     2.7e-6 / 1.71e-6 (bounds 1e-5 / 2e-6; far rows 7.7e-6 per (row, head))
    split3  3.9e-6 / 2.4e-6 (ceilings 1.28e-3 / 2.56e-4: the kernel is ~300 x inside its stated 2^-17)
    float64 reference: 3.9 s for `base` at 12 / 4 heads, 3.6 s for `bench` at 12 / 4, < 1 s elsewhere (16 threads)
  dense, worst tile / global of the kernel against the reference with the named roundings; [model worst tile / global = bound / 2]:
    to_qkv k_qkv256    1.86e-3 / 1.66e-3  [1.86e-3 / 1.66e-3]     planted rows 1.76e-3 [1.76e-3]
    mlp_fused          1.86e-3 / 1.67e-3  [2.02e-3 / 1.82e-3]     planted rows 2.27e-3 [2.81e-3]
    layer_tail y       1.87e-3 / 1.67e-3  [2.82e-3 / 2.50e-3]     planted rows 1.82e-3 [3.76e-3]
    layer_tail qkv     1.87e-3 / 1.66e-3  [3.44e-3 / 3.01e-3]     planted rows 1.84e-3 [4.28e-3]
    (model figures: the largest over the cases; each case is held to 2 x its own.)  Every all-zero input row: exact zeros.
  The whole file: 106 s on the GPU machine (220 passed, 4 skipped: paired tables at 3 q-heads per kv-head).
"""
import ctypes as C
import functools
import os
import time

import pytest
import torch

from oracle import titok_oracle as O
from tests import forward_cases as FC
from tests.blockwise import (attention_forward_reference, bf16_store, check_blockwise, check_row_tiles, check_rows, floored_blocks,
                             global_error, row_errors, row_tile_errors)
from tests.test_hip_backward_shapes import BATCHES as BWD_BATCHES, FAR_ROWS as BWD_FAR_ROWS, FWD_TOL
from titok_video_amd import _lib
from titok_video_amd.plan import BatchPlan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
GATE, PAIRED, QSCALED, ALLFULL, PIPE, SPLIT3 = 1, 2, 4, 8, 16, 32
NO_SWP = _lib.DBG_ATTN_NO_SWP      # ttv_debug_set bit 20: ttvk_attention keeps k_attn_bf16 where it would take k_attn_swp
TOL = dict(FWD_TOL, split3=(FWD_TOL["f32"][0] * 2.0 ** 7, FWD_TOL["f32"][1] * 2.0 ** 7))
HEADS = [(4, 2), (8, 2), (12, 4)]


def L():
    return _lib.lib()


def S():
    return _lib.stream_ptr(torch.device(DEV))


def report(*parts):
    print("MEASURED", *parts, flush=True)


def test_the_shared_batches_are_the_backward_file_s():
    assert FC.FAR_ROWS == BWD_FAR_ROWS
    for name in ("ragged", "far", "five"):
        assert FC.BATCHES[name] == BWD_BATCHES[name]


# ---------------------------------------------------------------------------------------------- attention
# route: operands ("plain" / "scaled"), kernel dtype, flags, work table (split argument of BatchPlan.attention_table; "w64": the
# table of ttv_attention64), ttv_debug_set bits
ROUTES = {
    "plain": ("plain", "bf16", 0, None, 0),
    "swp": ("scaled", "bf16", QSCALED | ALLFULL, False, 0),
    "bf16qs": ("scaled", "bf16", QSCALED | ALLFULL, False, NO_SWP),
    "mixed": ("scaled", "bf16", QSCALED, None, 0),
    "half": ("scaled", "bf16", QSCALED, True, 0),
    "paired": ("scaled", "bf16", QSCALED | PAIRED, False, 0),
    "pipe": ("scaled", "bf16", QSCALED | ALLFULL | PIPE, False, 0),
    "w64": ("scaled", "bf16", QSCALED, "w64", 0),
    "f32": ("plain", "f32", 0, None, 0),
    "split3": ("plain", "f32", SPLIT3, None, 0),
}
EVERY = ["bench", "far", "spikes6", "spikes30"]                      # what every route sees
ROUTE_BATCHES = {
    "plain": EVERY, "swp": ["bench", "five", "ragged", "far", "spikes6", "spikes30"], "bf16qs": EVERY, "mixed": EVERY + ["five"],
    "half": EVERY + ["ragged"], "paired": EVERY, "pipe": EVERY, "w64": EVERY + ["ragged"],
    "f32": EVERY + ["ragged"], "split3": EVERY + ["ragged"],
}
CASES = [(r, b, h) for r in ROUTES for b in ROUTE_BATCHES[r] for h in HEADS]
CASES += [(r, "base", (12, 4)) for r in ("swp", "plain", "w64", "f32", "split3")]


@functools.lru_cache(maxsize=8)
def _inputs(batch, hq, hkv):
    x, rows = FC.attention_inputs(batch, hq, hkv)
    plain, scaled = FC.attention_operands(x, hq)
    return {"plain": plain, "scaled": scaled}, rows


@functools.lru_cache(maxsize=None)
def _plan(batch):
    plan = BatchPlan(*FC.BATCHES[batch], FC.PATCH, DEV)
    assert plan.cu_seqlens == FC.cu_seqlens(batch)
    return plan


@functools.lru_cache(maxsize=6)
def _reference(batch, hq, hkv, ops):
    """(out, gated) in float64 for one operand set, the seconds it took, and the no-floored-block condition on both."""
    x = _inputs(batch, hq, hkv)[0][ops]
    cu = FC.cu_seqlens(batch)
    t0 = time.time()
    out, gated = attention_forward_reference(x, cu, hq, hkv, c_exp=FC.C_EXP if ops == "scaled" else None)
    dt = time.time() - t0
    for name, r in (("out", out), ("gated", gated)):
        assert not bool(floored_blocks(r, cu, hq).any()), f"{batch} {hq}/{hkv} {ops} {name}: a reference block is under the floor"
    return out, gated, dt


def _attention(route, plan, xd, Lr, hq, hkv, gate, tab):
    ops, dt, flags, table, debug = ROUTES[route]
    d = hq * 64
    ld = 2 * d + 2 * hkv * 64
    tdt = BF if dt == "bf16" else torch.float32
    o = torch.full((Lr + 1, d), float("nan"), dtype=tdt, device=DEV)              # one guard row behind the last
    L().ttv_debug_set(debug)
    try:
        if table == "w64":
            rc = L().ttv_attention64(xd.data_ptr(), ld, o.data_ptr(), d, plan.cu_dev.data_ptr(), tab.data_ptr(), tab.shape[0], hq, hkv, 64,
                                     flags | gate, _lib.TTV_BF16, S())
        else:
            rc = L().ttv_attention(xd.data_ptr(), ld, o.data_ptr(), d, plan.cu_dev.data_ptr(), tab.data_ptr(), tab.shape[0], hq, hkv, 64,
                                   flags | gate, _lib.dtype_code(tdt), S())
        _lib.check(rc, "attention")
        torch.cuda.synchronize()
    finally:
        L().ttv_debug_set(0)
    oc = o.cpu()
    assert bool(torch.isnan(oc[Lr]).all()), "written past the last row"
    return oc[:Lr]


@pytest.mark.parametrize("route,batch,heads", CASES, ids=[f"{r}-{b}-{h[0]}_{h[1]}" for r, b, h in CASES])
def test_attention_forward_routes_per_block(route, batch, heads):
    hq, hkv = heads
    ops, dt, flags, table, debug = ROUTES[route]
    if route == "paired" and (hq // hkv) % 2:
        pytest.skip("paired tables need an even number of q-heads per kv-head")
    if route == "swp" and os.environ.get("TTV_ATTN_SWP", "1")[:1] == "0":
        pytest.skip("TTV_ATTN_SWP=0 in the environment: the dispatch would not take k_attn_swp")
    plan = _plan(batch)
    Lr, cu = plan.total_rows, plan.cu_seqlens
    ref_out, ref_gated, secs = _reference(batch, hq, hkv, ops)           # includes the floor condition, before any launch
    xs, rows = _inputs(batch, hq, hkv)
    tab = plan.attention_table64(hq, hkv) if table == "w64" else plan.attention_table(hq, hkv, table)
    if table != "w64":
        halves = bool((tab[:, 3] == 1).any())
        if route == "mixed" and batch == "five":
            assert halves, "the 5-clip batch is expected to carry half items under the default rule"
        if flags & ALLFULL or (route in ("plain", "mixed", "f32", "split3") and batch == "bench"):
            assert not halves, "full items expected"
        if route == "half":
            assert bool((tab[tab[:, 0] >= 0, 3] == 1).all())
    xd = xs[ops].to(DEV, BF if dt == "bf16" else torch.float32)
    bt, gt = TOL["split3" if route == "split3" else dt]
    for gate in (GATE, 0):
        got = _attention(route, plan, xd, Lr, hq, hkv, gate, tab)
        ref = ref_gated if gate else ref_out
        tag = f"attention {route} {batch} {hq}/{hkv} gate {gate}"
        wb, gl = check_blockwise(got, ref, cu, hq, bt, gt, tag)
        wr = check_rows(got, ref, rows, bt, tag, heads=hq)
        report(f"{tag}: worst block {wb:.2e} (bound {bt:.1e}) global {gl:.2e} (bound {gt:.1e})"
               + (f"; worst planted (row, head) {wr:.2e}" if rows else "") + f"; float64 reference {secs:.1f} s")


RESTRICTED = [(b, h, w) for b in ("bench", "ragged_k") for h in HEADS for w in ("latent", "patch")]


@pytest.mark.parametrize("batch,heads,which", RESTRICTED, ids=[f"{w}-{b}-{h[0]}_{h[1]}" for b, h, w in RESTRICTED])
def test_attention_restricted_tables_write_their_rows_only(batch, heads, which):
    """The encoder's (latent query blocks) and the decoder's (all but the latent-only query blocks) last-layer tables through
    k_attn_swp: the rows of the query blocks the table names against float64, every other row still NaN."""
    hq, hkv = heads
    if os.environ.get("TTV_ATTN_SWP", "1")[:1] == "0":
        pytest.skip("TTV_ATTN_SWP=0 in the environment: the dispatch would not take k_attn_swp")
    plan = _plan(batch)
    Lr, cu = plan.total_rows, plan.cu_seqlens
    ref_out, ref_gated, secs = _reference(batch, hq, hkv, "scaled")
    tab = plan.attention_table_latent(hq, hkv) if which == "latent" else plan.attention_table_patch(hq, hkv)
    assert tab is not None, "the batch is chosen so that the patch table exists"
    # rows the plan says are inside: query blocks of 128 rows that hold a latent row / that do not hold latent rows only
    inside = torch.zeros(Lr, dtype=torch.bool)
    for b, k in enumerate(plan.token_counts):
        s = cu[b + 1] - cu[b]
        if which == "latent":
            inside[cu[b]:cu[b] + min(-(-k // 128) * 128, s)] = True
        else:
            inside[cu[b] + k // 128 * 128:cu[b + 1]] = True
    named = torch.zeros(Lr, hq, dtype=torch.bool)                       # ... and what the table's entries name
    for seq, q0, head, mode in tab.cpu().tolist():
        if seq >= 0:
            assert mode == 0
            named[cu[seq] + q0:min(cu[seq] + q0 + 128, cu[seq + 1]), head] = True
    assert torch.equal(named, inside[:, None].expand(Lr, hq))
    n_out = int((~inside).sum())
    assert 0 < n_out < Lr
    xd = _inputs(batch, hq, hkv)[0]["scaled"].to(DEV)
    bt, gt = TOL["bf16"]
    for gate in (GATE, 0):
        got = _attention("swp", plan, xd, Lr, hq, hkv, gate, tab)
        stayed = torch.isnan(got.float()).all(1)
        assert bool(stayed[~inside].all()), "a row outside the table was written"
        assert not bool(torch.isnan(got[inside].float()).any())
        ref = ref_gated if gate else ref_out
        icu = _inside_cu(inside, cu)
        assert not bool(floored_blocks(ref[inside], icu, hq).any())
        tag = f"attention swp {which} table {batch} {hq}/{hkv} gate {gate}"
        wb, gl = check_blockwise(got[inside], ref[inside], icu, hq, bt, gt, tag)
        report(f"{tag}: {int(stayed.sum())} rows stayed NaN ({n_out} outside the table), {int(inside.sum())} rows inside: "
               f"worst block {wb:.2e} (bound {bt:.1e}) global {gl:.2e} (bound {gt:.1e})")
        assert int(stayed.sum()) == n_out


def _inside_cu(inside, cu):
    """cu_seqlens of the rows that are inside (they start at a multiple of 128 rows in each sequence, so 64-row blocks stay aligned)."""
    out = [0]
    for b in range(len(cu) - 1):
        n = int(inside[cu[b]:cu[b + 1]].sum())
        if n:
            out.append(out[-1] + n)
    return out


# ---------------------------------------------------------------------------------------------- dense launches at width 256
D, INNER, GQ = 256, 704, 128
NQ = 2 * D + 2 * GQ
EPS = 1e-5


def _norm(t):
    return t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + EPS)


def _rot(t, cs):
    """Interleaved pairs, per 64-wide head; cs [M, 64] = cos | sin."""
    th = t.reshape(t.shape[0], -1, 32, 2)
    c, sn = cs[:, None, :32], cs[:, None, 32:]
    return torch.stack([th[..., 0] * c - th[..., 1] * sn, th[..., 0] * sn + th[..., 1] * c], -1).reshape(t.shape[0], -1)


def _id(t):
    return t


def _tail_definition(w, x, ao, keel, rnd, tail=True):
    """transformer.py:104,129-130 / 141-145, 47-56 as tests/test_hip_ops.py test_layer_tail_fused / test_mlp_fused write it; `rnd` is
    applied at the rounding points those references name (x1 as the residual stream, h in front of the w3 product)."""
    alpha = 8.0 if keel else 1.0
    if tail:
        y1 = alpha * x + ao @ w["wo"].T
        x1 = rnd(_norm(y1) * w["ag"] if keel else y1)
    else:
        x1 = x
    a, gate = (_norm(x1) @ w["w12f"].T).chunk(2, -1)
    h = rnd(torch.nn.functional.gelu(gate) * a)
    y = alpha * x1 + h @ w["w3"].T
    return _norm(y) * w["pg"] if keel else y


def _qkv_definition(w, y, cs):
    q = _norm(y) @ w["wqf"].T
    return torch.cat([_rot(q[:, :D], cs), q[:, D:2 * D], _rot(q[:, 2 * D:2 * D + GQ], cs), q[:, 2 * D + GQ:]], 1)


def _weights(seed, M):
    g = torch.Generator().manual_seed(seed)
    w = {"wo": (torch.randn(D, D, generator=g) * D ** -0.5).to(BF), "w12": (torch.randn(2 * INNER, D, generator=g) * D ** -0.5).to(BF),
         "w3": (torch.randn(D, INNER, generator=g) * INNER ** -0.5).to(BF), "wq": (torch.randn(NQ, D, generator=g) * D ** -0.5).to(BF)}
    ng, ag, pg, qg = (1 + 0.1 * torch.randn(D, generator=g) for _ in range(4))
    w["w12f"] = (w["w12"].float() * ng[None, :]).to(BF)                   # the pre-norm gains folded into the columns
    w["wqf"] = (w["wq"].float() * qg[None, :]).to(BF)
    w["ag"], w["pg"] = ag, pg
    ang = torch.rand(M, 32, generator=g) * 6.28
    w["cs"] = torch.cat([ang.cos(), ang.sin()], 1).float()
    return w, g


def _tile_floor_ok(ref, planted, what):
    """No 16 x 64 tile of the reference under the floor, except tiles that hold planted rows only (measured by check_rows)."""
    r = ref.clone()
    r[list(planted)] = 0.0
    low = floored_blocks(r, [0, r.shape[0]], r.shape[1] // 64, 16).any(1)
    for t in torch.nonzero(low).flatten().tolist():
        assert all(row in planted for row in range(16 * t, min(16 * t + 16, r.shape[0]))), f"{what}: the tile at row {16 * t} is under the floor"


def _check_dense(got, named, model, exact, planted, what):
    """`got` against the reference with the named roundings, bounds from the rounding model (see the module docstring)."""
    big = [r for r, k in planted.items() if k == 100.0]
    zero = [r for r, k in planted.items() if k == 0.0]
    other = [r for r, k in planted.items() if k != 0.0]
    _tile_floor_ok(named, planted, what)
    m, e = model.clone(), exact.clone()
    m[big] = 0.0
    e[big] = 0.0
    mt, mg = float(row_tile_errors(m, e).max()), global_error(m, e)
    wt, gl = check_row_tiles(got, named, 16, 64, 2 * mt, 2 * mg, what, leave_out=big)
    vs_exact = float(row_tile_errors(_zeroed(got, big), e).max())
    mrow = row_errors(model, exact, other)[:, 0]
    wr = check_rows(got, named, other, 2 * mrow, what)
    assert bool((got[zero] == 0).all()), f"{what}: an all-zero input row did not give an all-zero output row"
    report(f"{what}: worst tile {wt:.2e} (model {mt:.2e}, bound {2 * mt:.2e}) global {gl:.2e} (model {mg:.2e}); against the unrounded "
           f"definition {vs_exact:.2e}; planted rows worst {wr:.2e} (model {float(mrow.max()):.2e}), {len(zero)} zero rows exact")


def _zeroed(t, rows):
    t = t.double().cpu().clone()
    t[rows] = 0.0
    return t


@pytest.mark.parametrize("M", FC.DENSE_M)
def test_to_qkv_rope_width_256_per_tile(M):
    """k_qkv256 (the default behind ttv_linear_qkv_rope at K = 256) per tile against float64; k_gemm_k256<EPI_QKV_ROPE>
    (ttv_debug_set bit 15) gives the same bits."""
    plan = BatchPlan(*FC.DENSE_PLANS[M], FC.PATCH, DEV)
    assert plan.total_rows == M
    planted = FC.planted_rows(M)
    g = torch.Generator().manual_seed(M + 1)
    x = FC.plant(torch.randn(M, D, generator=g), planted).to(BF)
    w = (torch.randn(NQ, D, generator=g) * D ** -0.5).to(BF)
    cos, sin = O.rope_table(plan.grids, plan.token_counts)
    cs = torch.cat([torch.nn.functional.pad(cos.double(), (0, 32 - cos.shape[1]), value=1.0),
                    torch.nn.functional.pad(sin.double(), (0, 32 - sin.shape[1]), value=0.0)], 1)
    r = x.double() @ w.double().T
    exact = torch.cat([_rot(r[:, :D], cs), r[:, D:2 * D], _rot(r[:, 2 * D:2 * D + GQ], cs), r[:, 2 * D + GQ:]], 1)
    xd, wd = x.to(DEV), w.to(DEV)
    outs = []
    try:
        for bits in (0, _lib.DBG_QKV256_OFF):
            y = torch.full((M + 1, NQ), float("nan"), dtype=BF, device=DEV)
            L().ttv_debug_set(bits)
            _lib.check(L().ttv_linear_qkv_rope(xd.data_ptr(), D, wd.data_ptr(), D, y.data_ptr(), NQ, M, D, GQ, plan.rope_cs.data_ptr(),
                                               _lib.TTV_BF16, S()), "qkv")
            torch.cuda.synchronize()
            outs.append(y.cpu())
    finally:
        L().ttv_debug_set(0)
    assert bool(torch.isnan(outs[0][M]).all()) and bool(torch.isnan(outs[1][M]).all()), "written past the last row"
    _check_dense(outs[0][:M], exact, bf16_store(exact), exact, planted, f"to_qkv k_qkv256 M {M}")
    assert torch.equal(outs[0][:M], outs[1][:M]), "k_qkv256 differs from k_gemm_k256"


@pytest.mark.parametrize("M", FC.DENSE_M)
@pytest.mark.parametrize("keel", [True, False], ids=["keel", "plain"])
@pytest.mark.parametrize("deal9", [False, True], ids=["default", "deal9"])
def test_mlp_fused_width_256_per_tile(M, keel, deal9):
    planted = FC.planted_rows(M)
    w, g = _weights(M + 11, M)
    x = FC.plant(torch.randn(M, D, generator=g) * 1.3, planted).to(BF)
    w12d, w3d, pgd = w["w12f"].to(DEV), w["w3"].to(DEV), w["pg"].to(DEV)
    y = torch.full((M + 1, D), float("nan"), dtype=BF, device=DEV)     # in place on the residual stream, as the towers run it; one guard row
    y[:M] = x.to(DEV)
    pack = torch.empty(L().ttv_mlp_pack_bytes(INNER, 0), dtype=torch.uint8, device=DEV)
    _lib.check(L().ttv_mlp_pack(w12d.data_ptr(), w3d.data_ptr(), None, None, 0, INNER, D, _lib.TTV_BF16, pack.data_ptr(), S()), "mlp_pack")
    L().ttv_debug_set(_lib.DBG_MLP_TILES9 if deal9 else 0)
    try:
        _lib.check(L().ttv_mlp_fused(y.data_ptr(), D, pack.data_ptr(), INNER, y.data_ptr(), D, pgd.data_ptr() if keel else None,
                                     8.0 if keel else 1.0, EPS, M, D, _lib.TTV_BF16, S()), "mlp_fused")
        torch.cuda.synchronize()
    finally:
        L().ttv_debug_set(0)
    yc = y.cpu()
    assert bool(torch.isnan(yc[M]).all()), "written past the last row"
    wd = {k: v.double() for k, v in w.items()}
    named = _tail_definition(wd, x.double(), None, keel, bf16_store, tail=False)
    exact = _tail_definition(wd, x.double(), None, keel, _id, tail=False)
    _check_dense(yc[:M], named, bf16_store(named), exact, planted, f"mlp_fused M {M} {'keel' if keel else 'plain'} {'deal9' if deal9 else 'default'}")


@pytest.mark.parametrize("M", FC.DENSE_M)
@pytest.mark.parametrize("keel", [True, False], ids=["keel", "plain"])
@pytest.mark.parametrize("back", [False, True], ids=["tail", "tail+qkv"])
@pytest.mark.parametrize("deal9", [False, True], ids=["default", "deal9"])
def test_layer_tail_fused_width_256_per_tile(M, keel, back, deal9):
    planted = FC.planted_rows(M)
    w, g = _weights(M + 7, M)
    x = FC.plant(torch.randn(M, D, generator=g) * 1.3, planted).to(BF)
    ao = FC.plant(torch.randn(M, D, generator=g), planted).to(BF)
    aod, w12d, w3d, wod, wqd, agd, pgd, csd = (t.to(DEV) for t in (ao, w["w12f"], w["w3"], w["wo"], w["wqf"], w["ag"], w["pg"], w["cs"]))
    rows = NQ if back else 0
    pack = torch.empty(L().ttv_mlp_pack_bytes(INNER, rows), dtype=torch.uint8, device=DEV)
    _lib.check(L().ttv_mlp_pack(w12d.data_ptr(), w3d.data_ptr(), wod.data_ptr(), wqd.data_ptr() if back else None, rows, INNER, D,
                                _lib.TTV_BF16, pack.data_ptr(), S()), "mlp_pack")
    y = torch.full((M + 1, D), float("nan"), dtype=BF, device=DEV)     # in place on the residual stream, as the towers run it; one guard row
    y[:M] = x.to(DEV)
    qkv = torch.full((M + 1, NQ), float("nan"), dtype=BF, device=DEV)
    nx = _lib.NextQkv(qkv=qkv.data_ptr(), ld=NQ, rope_cs=csd.data_ptr(), rows=NQ, rope_q_end=D, rope_k_begin=2 * D, rope_k_end=2 * D + GQ)
    alpha = 8.0 if keel else 1.0
    L().ttv_debug_set(_lib.DBG_MLP_TILES9 if deal9 else 0)
    try:
        _lib.check(L().ttv_layer_tail_fused(aod.data_ptr(), D, agd.data_ptr() if keel else None, alpha, y.data_ptr(), D, pack.data_ptr(), INNER,
                                            y.data_ptr(), D, pgd.data_ptr() if keel else None, alpha, EPS, M, D, _lib.TTV_BF16,
                                            C.byref(nx) if back else None, S()), "layer_tail_fused")
        torch.cuda.synchronize()
    finally:
        L().ttv_debug_set(0)
    yc, qc = y.cpu(), qkv.cpu()
    assert bool(torch.isnan(yc[M]).all()) and bool(torch.isnan(qc[M]).all()), "written past the last row"
    wd = {k: v.double() for k, v in w.items()}
    named = _tail_definition(wd, x.double(), ao.double(), keel, bf16_store)
    exact = _tail_definition(wd, x.double(), ao.double(), keel, _id)
    model = bf16_store(named)
    tag = f"layer_tail M {M} {'keel' if keel else 'plain'} {'tail+qkv' if back else 'tail'} {'deal9' if deal9 else 'default'}"
    _check_dense(yc[:M], named, model, exact, planted, tag + ": y")
    if back:
        # the projection reads the stored (bf16) rows: the kernel's own y for the reference, the model's stored y for the model
        _check_dense(qc[:M], _qkv_definition(wd, yc[:M].double(), wd["cs"]), bf16_store(_qkv_definition(wd, model, wd["cs"])),
                     _qkv_definition(wd, exact, wd["cs"]), planted, tag + ": qkv")
    else:
        assert bool(torch.isnan(qc).all()), "the next layer's qkv was written without being asked for"
