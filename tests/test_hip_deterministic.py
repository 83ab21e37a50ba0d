"""Deterministic mode on the GPU (`-m gpu`): every float sum of the training path that more than one block adds to, per op through the
C ABI and through whole training steps.

Per op (inputs and float64 terms: tests/deterministic_cases.py, whose premises tests/test_deterministic_cases_cpu.py checks), mode on:
  (a) three runs on the same input give the same bits, destination and scratch alike;
  (b) the destination, pre-filled with non-zero values, equals bit for bit the pre-fill plus the sequential sum of the block partials
      read back from the scratch, in ascending block index (the layouts: include/titok_hip.h beside the size functions) - float32, double
      for the squared-error sums.  The single-writer forms (weight gradients, the owner kernels) have no partials: (a) stands alone;
  (c) the value lies within n * 2^-24 * sum |term| of the float64 sum of its terms, the pre-fill counted as one more term.
Mode off, the same call is held to (c): the bound holds for any order of an fp32 sum, so it is the bound of the atomics as well.

Shapes: the smallest with more than one block per destination and a ragged last block (the geometry is asserted from the size
functions).  Whole steps: the tiny tokenizer on three ragged clips, 4x16x16, 8x32x16 and 4x32x32 with 3, 8 and 1 tokens.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import deterministic_cases as DC
from tests.test_hip_backward import _hip_grads, _reference_grads, config, rel
from titok_video_amd import _lib
from titok_video_amd.model.titok import TiTok
from titok_video_amd.synthetic import seeded_titok_state, synthetic_clips

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"bf16": torch.bfloat16, "f32": torch.float32}
SHAPES, COUNTS = [(4, 16, 16), (8, 32, 16), (4, 32, 32)], [3, 8, 1]


def L():
    return _lib.lib()


def S():
    return _lib.stream_ptr(DEV)


@pytest.fixture()
def det():
    """Mode on for the test, whatever it was put back afterwards."""
    before = L().ttv_set_deterministic(1)
    yield
    torch.cuda.synchronize()
    L().ttv_set_deterministic(before)


def prefill(n, dtype=torch.float32):
    return (0.5 + 1e-3 * torch.arange(n, dtype=torch.float64)).to(dtype)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()


def scratch_for(nbytes):
    assert nbytes >= 0
    return torch.full((max(int(nbytes), 16),), 0xAB, dtype=torch.uint8, device=DEV)


def check_bound(name, got, pre, terms, count):
    """(c): got [destinations] against the float64 sum of terms + pre-fill, n + 1 terms."""
    got, pre = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(pre, dtype=np.float64).reshape(-1)
    total = terms.sum(0) + pre
    bound = (np.asarray(count) + 1) * DC.U * (np.abs(terms).sum(0) + np.abs(pre))
    err = np.abs(got - total)
    worst = float((err / bound).max())
    print(f"{name}: worst error / bound over {len(got)} destinations {worst:.3f}")
    assert np.all(err <= bound), (name, worst)


def three_runs(name, run):
    """(a): run() -> (destination tensor, scratch bytes tensor or None), three times; returns the first run's pair."""
    outs = [run() for _ in range(3)]
    torch.cuda.synchronize()
    for k in (1, 2):
        assert bits(outs[k][0]) == bits(outs[0][0]), f"{name}: destination of run {k + 1} differs from run 1"
        if outs[0][1] is not None:
            assert bits(outs[k][1]) == bits(outs[0][1]), f"{name}: scratch of run {k + 1} differs from run 1"
    return outs[0]


def check_fold(name, got, pre, part):
    """(b): part [blocks][elements] read back, pre the pre-fill, got the destination - all of one dtype."""
    assert part.shape[0] >= 2, f"{name}: {part.shape[0]} block(s) per destination - the shape does not exercise the fold"
    want = DC.fold_f32(np.asarray(pre, dtype=part.dtype).reshape(-1), part)
    assert np.asarray(got).reshape(-1).astype(part.dtype).tobytes() == want.tobytes(), f"{name}: not the partials' sum in ascending block index"


def partials(scr, nbytes, shape, dtype=torch.float32):
    return scr[:nbytes].view(dtype).reshape(shape).cpu().numpy()


# ---------------------------------------------------------------------------------------------- RMSNorm backward
def _rms_call(case, dt, scr, nbytes):
    rows, width, code = case["rows"], case["width"], _lib.dtype_code(DT[dt])
    x, dy, gain = case["x"].to(DEV, DT[dt]), case["dy"].to(DEV, DT[dt]), case["gain"].to(DEV)
    dx = torch.zeros(x.shape, dtype=DT[dt], device=DEV)
    dgain = prefill(width).to(DEV)
    maps = [None if m is None else m.to(DEV) for m in (case["x_rows"], case["dy_rows"], case["dx_rows"])]
    _lib.check(L().ttv_rmsnorm_backward_det(x.data_ptr(), width, dy.data_ptr(), width, gain.data_ptr(), dx.data_ptr(), width, dgain.data_ptr(),
                                            rows, width, DC.EPS, code, *[_lib.ptr(m) for m in maps], scr.data_ptr(), nbytes, S()),
               "ttv_rmsnorm_backward_det")
    return dgain


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("maps", [False, True], ids=["plain", "maps"])
@pytest.mark.parametrize("rows,width", DC.RMS_SHAPES)
def test_rmsnorm_gain_gradient(det, rows, width, maps, dt):
    case = DC.rmsnorm_case(rows, width, maps)
    name = f"rmsnorm_bwd {rows}x{width} maps={maps} {dt}"
    nbytes = L().ttv_rmsnorm_backward_det_scratch_bytes(rows, width)
    blocks = nbytes // (4 * width)
    assert blocks == -(-rows // 4) >= 2                            # four rows per block at these sizes (9 rows: the last block holds one)
    scr = scratch_for(nbytes)
    got = three_runs(name, lambda: (_rms_call(case, dt, scr, nbytes), scr.clone()))[0]
    check_fold(name, got.cpu().numpy(), prefill(width).numpy(), partials(scr, nbytes, (blocks, width)))
    check_bound(name, got.cpu().numpy(), prefill(width).numpy(), case["terms"], case["count"])
    L().ttv_set_deterministic(0)
    off = _rms_call(case, dt, scr, 0)
    check_bound(name + " mode off", off.cpu().numpy(), prefill(width).numpy(), case["terms"], case["count"])


def _chain_call(case, dt, scr, nbytes):
    rows, width, code = case["rows"], case["width"], _lib.dtype_code(DT[dt])
    x, dy = case["x"].to(DEV, DT[dt]), case["dy"].to(DEV, DT[dt])
    y, dx = case["y"].to(DEV), case["acc"].to(DEV).clone()
    g1, g2 = case["gain1"].to(DEV), case["gain2"].to(DEV)
    d1, d2 = prefill(width).to(DEV), (2 * prefill(width)).to(DEV)
    cast = torch.empty(rows, width, dtype=DT[dt], device=DEV)
    _lib.check(L().ttv_rmsnorm_backward_chain_det(x.data_ptr(), width, dy.data_ptr(), width, g1.data_ptr(), d1.data_ptr(), dx.data_ptr(), width,
                                                  y.data_ptr(), width, g2.data_ptr(), d2.data_ptr(), 0.5, cast.data_ptr(), width, rows, width,
                                                  DC.EPS, code, scr.data_ptr(), nbytes, S()), "ttv_rmsnorm_backward_chain_det")
    return torch.cat([d1, d2])


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("rows,width", DC.RMS_SHAPES)
def test_rmsnorm_chain_gain_gradients(det, rows, width, dt):
    case = DC.chain_case(rows, width)
    name = f"rmsnorm_bwd_chain {rows}x{width} {dt}"
    nbytes = L().ttv_rmsnorm_backward_chain_det_scratch_bytes(rows, width)
    blocks = nbytes // (8 * width)
    assert blocks == -(-rows // 4) >= 2
    scr = scratch_for(nbytes)
    pre = torch.cat([prefill(width), 2 * prefill(width)]).numpy()
    got = three_runs(name, lambda: (_chain_call(case, dt, scr, nbytes), scr.clone()))[0].cpu().numpy()
    part = partials(scr, nbytes, (2, blocks, width))             # gain 1's array, gain 2's behind it
    check_fold(name + " gain 1", got[:width], pre[:width], part[0])
    check_fold(name + " gain 2", got[width:], pre[width:], part[1])
    check_bound(name, got, pre, case["terms"], case["count"])
    L().ttv_set_deterministic(0)
    check_bound(name + " mode off", _chain_call(case, dt, scr, 0).cpu().numpy(), pre, case["terms"], case["count"])


# ---------------------------------------------------------------------------------------------- colsum, sumall, outer_small
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_colsum(det, dt):
    case = DC.colsum_case()
    rows, n = case["a"].shape
    a = case["a"].to(DEV, DT[dt])
    nbytes = L().ttv_colsum_det_scratch_bytes(rows, n)
    assert nbytes == 4 * n * 4 and rows % 64 != 0 and n > 256 and n % 256 != 0
    scr = scratch_for(nbytes)

    def run():
        out = prefill(n).to(DEV)
        _lib.check(L().ttv_colsum_accumulate(a.data_ptr(), _lib.dtype_code(DT[dt]), n, None, rows, n, out.data_ptr(), scr.data_ptr(), nbytes, S()), "colsum")
        return out, scr.clone()
    got = three_runs(f"colsum {dt}", run)[0].cpu().numpy()
    check_fold(f"colsum {dt}", got, prefill(n).numpy(), partials(scr, nbytes, (4, n)))
    check_bound(f"colsum {dt}", got, prefill(n).numpy(), case["terms"], case["count"])
    L().ttv_set_deterministic(0)
    check_bound(f"colsum {dt} mode off", run()[0].cpu().numpy(), prefill(n).numpy(), case["terms"], case["count"])


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_sumall(det, dt):
    case = DC.sumall_case()
    rows, n = case["a"].shape
    a = case["a"].to(DEV, DT[dt])
    nbytes = L().ttv_sumall_det_scratch_bytes(rows, n)
    assert nbytes == 3 * 4 and (rows * n) % 256 != 0
    scr = scratch_for(nbytes)

    def run():
        out = prefill(1).to(DEV)
        _lib.check(L().ttv_sumall_accumulate(a.data_ptr(), _lib.dtype_code(DT[dt]), n, rows, n, case["scale"], out.data_ptr(), scr.data_ptr(), nbytes,
                                             S()), "sumall")
        return out, scr.clone()
    got = three_runs(f"sumall {dt}", run)[0].cpu().numpy()
    check_fold(f"sumall {dt}", got, prefill(1).numpy(), partials(scr, nbytes, (3, 1)))
    check_bound(f"sumall {dt}", got, prefill(1).numpy(), case["terms"], case["count"])
    L().ttv_set_deterministic(0)
    check_bound(f"sumall {dt} mode off", run()[0].cpu().numpy(), prefill(1).numpy(), case["terms"], case["count"])


@pytest.mark.parametrize("transpose", [0, 1], ids=["c-major", "transposed"])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_outer_small(det, dt, transpose):
    case = DC.outer_small_case()
    rows, Cc, d = case["rows"], case["C"], case["d"]
    a, b = case["a"].to(DEV), case["b"].to(DEV, DT[dt])           # the token-side operand fp32 (dz), the d-side one in the tower's dtype
    nbytes = L().ttv_outer_small_det_scratch_bytes(rows, Cc, d)
    assert nbytes == 10 * Cc * d * 4 and rows % 32 != 0
    scr = scratch_for(nbytes)
    name = f"outer_small {dt} transpose={transpose}"

    def run():
        dw = prefill(Cc * d).reshape(Cc, d)
        dw = (dw.T.contiguous() if transpose else dw).to(DEV)
        _lib.check(L().ttv_outer_small_accumulate(a.data_ptr(), _lib.TTV_F32, Cc, Cc, b.data_ptr(), _lib.dtype_code(DT[dt]), d, dw.data_ptr(),
                                                  Cc if transpose else d, transpose, rows, d, scr.data_ptr(), nbytes, S()), "outer_small")
        return (dw.T.contiguous() if transpose else dw), scr.clone()          # as [C][d] either way
    got = three_runs(name, run)[0].cpu().numpy()
    check_fold(name, got, prefill(Cc * d).numpy(), partials(scr, nbytes, (10, Cc * d)))
    check_bound(name, got, prefill(Cc * d).numpy(), case["terms"], case["count"])
    L().ttv_set_deterministic(0)
    check_bound(name + " mode off", run()[0].cpu().numpy(), prefill(Cc * d).numpy(), case["terms"], case["count"])


# ---------------------------------------------------------------------------------------------- the two loss sums
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_l1_loss_and_sq_err(det, dt):
    case = DC.clips_case()
    n = len(DC.CLIP_SIZES)
    recon = [r.to(DEV, DT[dt]) for r in case["recon"]]
    target = [t.to(DEV, DT[dt]) for t in case["target"]]
    sizes = (C.c_int32 * n)(*DC.CLIP_SIZES)
    code = _lib.dtype_code(DT[dt])
    nb_l1, nb_sq = L().ttv_l1_loss_det_scratch_bytes(sizes, n), L().ttv_sq_err_accumulate_det_scratch_bytes(sizes, n)
    assert nb_l1 == n * 3 * 4 and nb_sq == n * 3 * 16              # three blocks per clip (2048 elements each), the short clips' last ones idle or ragged
    s1, s2 = scratch_for(nb_l1), scratch_for(nb_sq)

    def run_l1(det_call=True):
        loss = prefill(1).to(DEV)
        grads = [torch.empty_like(r) for r in recon]
        fn, tail = (L().ttv_l1_loss_det, (s1.data_ptr(), nb_l1, S())) if det_call else (L().ttv_l1_loss, (S(),))
        _lib.check(fn(_lib.ptr_array(recon), _lib.ptr_array(target), _lib.ptr_array(grads), sizes, n, code, loss.data_ptr(), *tail), "l1_loss")
        return loss, s1.clone()

    def run_sq(det_call=True):
        acc = prefill(2, torch.float64).to(DEV)
        fn, tail = (L().ttv_sq_err_accumulate_det, (s2.data_ptr(), nb_sq, S())) if det_call else (L().ttv_sq_err_accumulate, (S(),))
        _lib.check(fn(_lib.ptr_array(recon), _lib.ptr_array(target), sizes, n, code, 1, acc.data_ptr(), *tail), "sq_err")
        return acc, s2.clone()
    n_terms = np.array([sum(DC.CLIP_SIZES)])
    got = three_runs(f"l1_loss {dt}", run_l1)[0].cpu().numpy()
    check_fold(f"l1_loss {dt}", got, prefill(1).numpy(), partials(s1, nb_l1, (n * 3, 1)))
    check_bound(f"l1_loss {dt}", got, prefill(1).numpy(), case["l1_terms"], n_terms)
    got = three_runs(f"sq_err {dt}", run_sq)[0].cpu().numpy()
    part = partials(s2, nb_sq, (n * 3, 2), torch.float64)
    check_fold(f"sq_err {dt}", got, prefill(2, torch.float64).numpy(), part)
    assert got[1] == prefill(2, torch.float64).numpy()[1] + sum(DC.CLIP_SIZES)         # the element count, exact
    check_bound(f"sq_err {dt}", got[:1], prefill(2, torch.float64).numpy()[:1], case["sq_terms"], n_terms)
    L().ttv_set_deterministic(0)
    check_bound(f"l1_loss {dt} mode off", run_l1(False)[0].cpu().numpy(), prefill(1).numpy(), case["l1_terms"], n_terms)
    check_bound(f"sq_err {dt} mode off", run_sq(False)[0].cpu().numpy()[:1], prefill(2, torch.float64).numpy()[:1], case["sq_terms"], n_terms)


# ---------------------------------------------------------------------------------------------- codebook gradient
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_vq_lookup_backward(det, dt):
    case = DC.vq_case()
    rows, N, Cc = case["rows"], case["N"], case["C"]
    dcodes, idx = case["dcodes"].to(DEV, DT[dt]), case["idx"].to(DEV)
    assert L().ttv_vq_lookup_backward_det_scratch_bytes(rows, N, Cc) == 0

    def run(sibling=True):
        dcb = prefill(N * Cc).reshape(N, Cc).to(DEV)
        if sibling:
            rc = L().ttv_vq_lookup_backward_det(dcodes.data_ptr(), _lib.dtype_code(DT[dt]), Cc, idx.data_ptr(), rows, N, Cc, dcb.data_ptr(), Cc, None, 0, S())
        else:
            rc = L().ttv_vq_lookup_backward(dcodes.data_ptr(), _lib.dtype_code(DT[dt]), Cc, idx.data_ptr(), rows, Cc, dcb.data_ptr(), Cc, S())
        _lib.check(rc, "vq_lookup_backward")
        return dcb, None
    got = three_runs(f"vq_lookup_bwd {dt}", run)[0].cpu().numpy().reshape(-1)
    pre = prefill(N * Cc).numpy()
    assert got[7 * Cc:8 * Cc].tobytes() == pre[7 * Cc:8 * Cc].tobytes()                # the entry no row chose keeps its bits
    # an owner adds its rows in ascending order: the sequential float32 sum of the entry's terms, then onto the pre-fill
    want = (pre + DC.sequential_f32(case["terms"])).astype(np.float32)
    assert got.tobytes() == want.tobytes(), "not the rows of an entry added in ascending row order"
    check_bound(f"vq_lookup_bwd {dt}", got, pre, case["terms"], case["count"])
    L().ttv_set_deterministic(0)
    check_bound(f"vq_lookup_bwd {dt} mode off", run(False)[0].cpu().numpy(), pre, case["terms"], case["count"])


# ---------------------------------------------------------------------------------------------- weight gradient
def _wgrad(case, dt, ws_bytes, offset=0):
    Lr, N, K = case["L"], DC.WGRAD_N, DC.WGRAD_K
    pad = torch.zeros(offset, dtype=DT[dt])
    dyb = torch.cat([pad, case["dy"].to(DT[dt]).reshape(-1)]).to(DEV)
    xb = torch.cat([pad, case["x"].to(DT[dt]).reshape(-1)]).to(DEV)
    es = dyb.element_size()
    dw = prefill(N * K).reshape(N, K).to(DEV)
    ws = scratch_for(ws_bytes)
    _lib.check(L().ttv_linear_wgrad(dyb.data_ptr() + offset * es, N, xb.data_ptr() + offset * es, K, dw.data_ptr(), K, Lr, N, K,
                                    _lib.dtype_code(DT[dt]), ws.data_ptr() if ws_bytes else None, ws_bytes, S()), "linear_wgrad")
    return dw, None


@pytest.mark.parametrize("path", ["bf16 split", "bf16 no workspace", "bf16 unaligned", "f32"])
def test_weight_gradient_paths(det, path):
    """L: the smallest with two token ranges per output tile on the path's mode-off geometry - 65 for the bf16 kernels (ranges of 64
    tokens; the split plan's size function says two partial tiles per output tile), 1025 for the fp32 kernel (ranges of 1024)."""
    dt = "f32" if path == "f32" else "bf16"
    Lr = 1025 if path == "f32" else 65
    case = DC.wgrad_case(Lr)
    need = L().ttv_linear_wgrad_workspace_bytes(Lr, DC.WGRAD_N, DC.WGRAD_K)
    # two token ranges per output tile with the mode off, on every path: the split plan by its size function (2 x 1 tiles of 128 x 128,
    # 64 KB per partial tile); the two kernels without partial tiles by their documented ranges - 64 tokens (the 64 x 64 bf16 kernel and
    # the 128 x 128 one without a workspace, whose plan is the split plan's) and 1024 tokens (fp32)
    if dt == "bf16":
        assert need == 2 * 1 * 2 * 65536 and -(-Lr // 64) == 2 and Lr % 64 != 0
    else:
        assert -(-Lr // 1024) == 2 and Lr % 1024 != 0
    # "bf16 split": the partial tiles (fragment order) are k_wgrad_reduce's from before this mode and are not read back: (a) and (c)
    ws_bytes = need if path == "bf16 split" else 0
    offset = 4 if path == "bf16 unaligned" else 0                  # 8 bytes off: the 64 x 64 kernel
    pre = prefill(DC.WGRAD_N * DC.WGRAD_K).numpy()
    got = three_runs(f"wgrad {path}", lambda: _wgrad(case, dt, ws_bytes, offset))[0].cpu().numpy()
    check_bound(f"wgrad {path}", got, pre, case["terms"], case["count"])
    L().ttv_set_deterministic(0)
    check_bound(f"wgrad {path} mode off", _wgrad(case, dt, ws_bytes, offset)[0].cpu().numpy(), pre, case["terms"], case["count"])


# ---------------------------------------------------------------------------------------------- fp32 attention backward
@pytest.mark.parametrize("qlim", [False, True], ids=["every-row", "qlim"])
def test_attention_backward_f32(det, qlim):
    """Two sequences of 130 and 70 rows (2 and 6 latent tokens in front of 128 and 64 patches), 4 q-heads on 2 kv-heads.  With the clip
    descriptors (ttv_attention_backward_qlim) the first sequence keeps its query rows [0, 128) and drops rows 128 and 129 - the
    owner kernel's nq < S branch - and the second keeps all 70 (ceil(6 / 128) * 128 > 70).  Three runs with the mode on agree bit for
    bit; dq, dk and dv are held to a float64 restatement (autograd through the oracle's attention, the loss taken over the kept query
    rows only) at the fp32 bound of tests/test_hip_backward.py, 2e-4 relative per part; the dropped rows' dq is exactly zero; and dq is
    the mode-off kernel's, bit for bit."""
    from oracle import titok_oracle as O
    from titok_video_amd.plan import BatchPlan
    shapes, counts = [(8, 64, 64), (4, 64, 64)], [2, 6]
    plan = BatchPlan(shapes, counts, (4, 8, 8), DEV)
    cu = [int(v) for v in plan.cu_seqlens]
    assert [b - a for a, b in zip(cu[:-1], cu[1:])] == [130, 70]
    hq, hkv, d, gq = 4, 2, 256, 128
    ld, Lr = 2 * d + 2 * gq, plan.total_rows
    g = torch.Generator().manual_seed(7)
    qkvg = torch.randn(Lr, ld, generator=g)
    dout = torch.randn(Lr, d, generator=g) * torch.pow(2.0, torch.randint(-10, 11, (Lr, 1), generator=g).float())   # rows spread over 2^20
    kept = torch.ones(Lr, dtype=torch.bool)
    if qlim:
        kept[cu[0] + 128:cu[1]] = False
        assert int((~kept).sum()) == 2
    f = qkvg.double().requires_grad_(True)
    q, _gate, k, v = f.split([d, d, gq, gq], dim=-1)
    ref_o = O.attention_varlen(q.unflatten(-1, (hq, 64)), k.unflatten(-1, (hkv, 64)), v.unflatten(-1, (hkv, 64)), plan.cu_seqlens).flatten(-2)
    (ref_o * dout.double() * kept[:, None]).sum().backward()
    gref = f.grad
    xd, dod = qkvg.to(DEV), dout.to(DEV)
    o, lse = torch.empty(Lr, d, device=DEV), torch.empty(Lr, hq, device=DEV)
    tab = plan.attention_table(hq, hkv)
    _lib.check(L().ttv_attention_lse(xd.data_ptr(), ld, o.data_ptr(), d, plan.cu_dev.data_ptr(), tab.data_ptr(), tab.shape[0], hq, hkv, 64, 0,
                                     _lib.TTV_F32, lse.data_ptr(), S()), "attention_lse")
    bt, rs = plan.table(4, 2 * plan.n_blocks64), plan.table(5, Lr)
    desc = plan.clip_desc_dev if qlim else None

    def run():
        dq = torch.full((Lr, ld), 7.0, device=DEV)
        delta, scratch = torch.empty(Lr, hq, device=DEV), torch.empty(Lr, 2 * gq, device=DEV)
        _lib.check(L().ttv_attention_backward_qlim(xd.data_ptr(), ld, o.data_ptr(), d, dod.data_ptr(), d, lse.data_ptr(), delta.data_ptr(),
                                                   plan.cu_dev.data_ptr(), bt.data_ptr(), plan.n_blocks64, rs.data_ptr(), dq.data_ptr(), ld,
                                                   scratch.data_ptr(), Lr, hq, hkv, _lib.TTV_F32, None, _lib.ptr(desc), S()),
                   "attention_backward_qlim")
        return dq, None
    name = f"attention_bwd f32 qlim={qlim}"
    got = three_runs(name, run)[0]
    assert torch.equal(got[:, d:2 * d], torch.full((Lr, d), 7.0, device=DEV)), "the gate columns are not this kernel's to write"
    if qlim:
        assert float(got[~kept.to(DEV), :d].abs().max()) == 0.0
    for part, sl in (("dq", slice(0, d)), ("dk", slice(2 * d, 2 * d + gq)), ("dv", slice(2 * d + gq, ld))):
        e = rel(got[:, sl].cpu().double(), gref[:, sl])
        print(f"{name} {part}: relative error against float64 {e:.2e}")
        assert e < 2e-4, (name, part, e)
    L().ttv_set_deterministic(0)
    off = run()[0]
    assert torch.equal(got[:, :d], off[:, :d]), "dq is computed as it is with the mode off"
    for part, sl in (("dk", slice(2 * d, 2 * d + gq)), ("dv", slice(2 * d + gq, ld))):
        assert rel(off[:, sl].cpu().double(), gref[:, sl]) < 2e-4, (name, part, "mode off")


# ---------------------------------------------------------------------------------------------- whole steps
def _model(dtype, recompute=False, frozen_encoder=False):
    m = TiTok(config())
    m.load_state_dict(seeded_titok_state(0), strict=True)
    m = m.to(DEV, dtype).train().set_activation_recompute(recompute)
    if frozen_encoder:
        for p in m.encoder.parameters():
            p.requires_grad_(False)
    return m


def _step(dtype, recompute=False, frozen_encoder=False):
    """Forward with tape, L1 against half the clips, backward: everything the step computed, on the host."""
    from titok_video_amd.train import l1_reconstruction_loss
    model = _model(dtype, recompute, frozen_encoder)
    clips = [c.requires_grad_(True) for c in synthetic_clips(SHAPES, seed=31, dtype=dtype, device=DEV)]
    recon, _ = model(clips, list(COUNTS))
    loss = l1_reconstruction_loss(recon, [c.detach() * 0.5 for c in clips])
    loss.backward()
    torch.cuda.synchronize()
    out = {"param " + n: p.grad.float().cpu() for n, p in model.named_parameters() if p.grad is not None}
    out.update({f"dclip {i}": c.grad.float().cpu() for i, c in enumerate(clips)})
    out.update({f"recon {i}": r.detach().float().cpu() for i, r in enumerate(recon)})
    out["loss"] = loss.detach().float().cpu()
    return out


def _same(a, b, what):
    assert set(a) == set(b), what
    differ = [n for n in a if not torch.equal(a[n], b[n])]
    assert not differ, f"{what}: {len(differ)} of {len(a)} outputs differ: {differ[:8]}"


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_step_is_bit_reproducible_stored_and_recompute(det, dt):
    """Three steps from the same weights: every parameter gradient (gains, biases, mask tokens and the token-width projections
    included), dclips, the reconstructions and the loss scalar agree bit for bit; and the recompute tape gives the stored tape's bits
    with no exception - the list tests/test_hip_recompute.py has to set aside with the mode off."""
    a = _step(DT[dt])
    names = [n for n in a if n.startswith("param ")]
    assert len(names) == len(list(_model(DT[dt]).parameters()))
    assert any(n.endswith("encoder.proj_out.weight") for n in names) and any(n.endswith("mask_token") for n in names)
    _same(a, _step(DT[dt]), f"{dt} step, second run")
    _same(a, _step(DT[dt]), f"{dt} step, third run")
    _same(a, _step(DT[dt], recompute=True), f"{dt} step, recompute tape against the stored tape")


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_frozen_encoder_step_is_bit_reproducible(det, dt):
    """grads == NULL for the encoder (every parameter frozen, the clips want their gradient)."""
    a = _step(DT[dt], frozen_encoder=True)
    assert not [n for n in a if n.startswith("param encoder.")]
    _same(a, _step(DT[dt], frozen_encoder=True), f"{dt} frozen encoder, second run")
    _same(a, _step(DT[dt], frozen_encoder=True), f"{dt} frozen encoder, third run")
    _same(a, _step(DT[dt], recompute=True, frozen_encoder=True), f"{dt} frozen encoder, recompute")


def test_mode_touches_only_the_listed_sites(det):
    """bf16: the weight matrices' gradients (split partial tiles, summed in a fixed order) and everything in front of them are
    reproducible with the mode off as well, and bit-identical with the mode on and off; the outputs that differ are atomically summed."""
    on = _step(torch.bfloat16)
    L().ttv_set_deterministic(0)
    off = _step(torch.bfloat16)
    matrices = [n for n in on if n.startswith("param ") and any(k in n for k in ("to_qkv", "out_proj", "w12", "w3")) and n.endswith("weight")]
    assert len(matrices) == 2 * 4 * 4
    fixed = matrices + [n for n in on if n.startswith(("recon", "dclip"))]
    differ = [n for n in fixed if not torch.equal(on[n], off[n])]
    assert not differ, differ
    for n in on:
        if not torch.equal(on[n], off[n]):
            t = on[n]
            assert n == "loss" or t.dim() < 2 or min(t.shape) == 1 or n.endswith(("encoder.proj_out.weight", "decoder.proj_in.weight")), n


def test_fp32_gradients_hold_the_oracle_bound(det):
    """The mode changes the order of a sum, not what is summed: the fp32 step against the float64-free fp32 oracle, the bound of
    tests/test_hip_backward.py (2e-3 relative per tensor)."""
    ref_loss, ref_idx, sd, ref_clips = _reference_grads(SHAPES, COUNTS, 31)
    loss, idx, model, clips = _hip_grads(torch.float32, SHAPES, COUNTS, 31)
    assert torch.equal(idx.cpu(), ref_idx)
    assert abs(float(loss) - float(ref_loss)) < 1e-4 * abs(float(ref_loss))
    worst = max((rel(p.grad, sd[n].grad), n) for n, p in model.named_parameters())
    print(f"deterministic fp32 step: worst relative gradient error {worst[0]:.2e} ({worst[1]})")
    assert worst[0] < 2e-3, worst
    for c, rc in zip(clips, ref_clips):
        assert rel(c.grad, rc.grad) < 2e-3


def test_bf16_gradients_hold_the_float64_replay(det):
    from tests.test_hip_backward_bf16 import check_against_replay, hip_grads
    check_against_replay(hip_grads("tiny-full"), "tiny-full", "deterministic bf16 tiny-full")


def _train(n_steps, graphed=False):
    from titok_video_amd.optim import HipAdamW
    from titok_video_amd.train import GraphedTrainingStep, make_optimizer, training_step
    torch.manual_seed(0)
    model = TiTok(config())
    model.load_state_dict(seeded_titok_state(0), strict=True)
    model = model.to(DEV).train()                                  # fp32 master weights, bf16 compute
    opt = make_optimizer(model, lr=1e-3, hip_capturable=True)      # HipAdamW's device path: eager and under capture alike
    assert isinstance(opt, HipAdamW)
    clips = synthetic_clips(SHAPES, seed=31, dtype=torch.bfloat16, device=DEV)
    step = GraphedTrainingStep(model, opt, clips, list(COUNTS)) if graphed else None
    losses = []
    for _ in range(n_steps):
        loss = step(clips)[0] if graphed else training_step(model, clips, list(COUNTS), opt)[0]
        losses.append(loss.detach().float().cpu().clone())
    torch.cuda.synchronize()
    out = {"param " + n: p.detach().float().cpu() for n, p in model.named_parameters()}
    for i, p in enumerate(model.parameters()):
        for k, v in opt.state[p].items():
            if torch.is_tensor(v):
                out[f"state {i} {k}"] = v.detach().float().cpu()
    out.update({f"loss {i}": l for i, l in enumerate(losses)})
    return out


def test_training_steps_are_bit_reproducible(det):
    """Three training_steps (forward, L1, backward, clip, HipAdamW) from the same seed, twice: all weights, all optimizer state and
    the three loss scalars agree bit for bit."""
    a = _train(3)
    assert any(k.startswith("state ") for k in a)
    _same(a, _train(3), "three training steps, second run")


def test_graphed_step_replays_the_eager_deterministic_step(det):
    """GraphedTrainingStep captured with the mode on (the launchers read it at capture): two replays from the same state leave the
    weights, the optimizer state and the losses of two eager deterministic steps, bit for bit."""
    _same(_train(2), _train(2, graphed=True), "graph replays against eager steps")


_SWITCH_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from titok_video_amd import _lib
from tests.test_hip_deterministic import _step
assert _lib.is_deterministic()                       # TTV_DETERMINISTIC=1 in the environment
a, b = _step(torch.bfloat16), _step(torch.bfloat16)
differ = [n for n in a if not torch.equal(a[n], b[n])]
print("DIFFER", len(a), differ)
"""


@pytest.mark.parametrize("switch", ["TTV_TRAIN_FUSED_NORMS=1", "TTV_WGRAD_TILE64=1", "TTV_WGRAD_BATCHED=0", "TTV_WGRAD_SIDE=0"])
def test_ab_switches_stay_deterministic(switch):
    """The A/B switches that reach the backward (read once per process, so a child process each, started with TTV_DETERMINISTIC=1): the
    bf16 step twice, every output bit for bit.  TTV_TRAIN_FUSED_NORMS gives the chain kernel fp32 sums, TTV_WGRAD_TILE64 the 64 x 64
    weight-gradient kernel (one token range per tile under the mode), TTV_WGRAD_BATCHED=0 one summing launch per weight."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    name, value = switch.split("=")
    env = dict(os.environ, TTV_DETERMINISTIC="1", **{name: value})
    out = subprocess.run([sys.executable, "-c", _SWITCH_CHILD, root], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("DIFFER")][0]
    assert line.endswith("[]"), (switch, line)


def _gan_train(n_steps):
    """gan_training_step on the L2-quantiser model: L1 + the relativistic GAN term through the frozen discriminator + the perceptual
    term on seeded LPIPS weights (as tests/test_hip_lpips.py builds them), then the discriminator's own step."""
    import random
    from types import SimpleNamespace
    from titok_video_amd.model.losses.loss_module import ReconstructionLoss
    from titok_video_amd.optim import HipAdamW
    from titok_video_amd.synthetic import seeded_lpips_state, seeded_tower_state
    from titok_video_amd.train import gan_training_step, make_discriminator_optimizer, make_optimizer
    cfg = SimpleNamespace(
        tokenizer=SimpleNamespace(model=SimpleNamespace(patch_size=[4, 8, 8], fsq_levels=None, quantizer="l2", codebook_size=64, token_size=8,
                                                        encoder_size="tiny", decoder_size="tiny"),
                                  losses=SimpleNamespace(disc_weight=0.4, perceptual_weight=1.0, gram_weight=0.0,
                                                         perceptual_samples_per_step=6, perceptual_sampling_size=64)),
        discriminator=SimpleNamespace(model=SimpleNamespace(patch_size=[4, 8, 8], model_size="tiny"),
                                      losses=SimpleNamespace(gp_weight=0.1, gp_noise=0.1, centering_weight=0.01)),
        training=SimpleNamespace(main=SimpleNamespace(torch_compile=False, max_steps=1000)))
    random.seed(0)
    torch.manual_seed(0)
    model = TiTok(cfg)
    model.load_state_dict(seeded_titok_state(0, token_size=8), strict=False)       # the towers; the codebook keeps its seeded start
    model = model.to(DEV, torch.bfloat16).train()
    lm = ReconstructionLoss(cfg, perceptual_weights=seeded_lpips_state(2))
    lm.disc_model.load_state_dict(seeded_tower_state("encoder", "tiny", (4, 8, 8), 3, 1, seed=77))
    lm = lm.to(DEV, torch.bfloat16).train()
    clips = synthetic_clips([(4, 64, 64), (8, 64, 64)], seed=1, dtype=torch.bfloat16, device=DEV)
    og, od = make_optimizer(model), make_discriminator_optimizer(lm)
    assert isinstance(og, HipAdamW) and isinstance(od, HipAdamW)
    cb = model.quantize.codebook
    assert any(p is cb for grp in og.param_groups for p in grp["params"]), "the codebook is trained by its gradient"
    out = {}
    for i in range(n_steps):
        ld, idx = gan_training_step(model, lm, clips, [3, 8], og, od)
        if i == 0:
            assert cb.grad is not None and float(cb.grad.float().abs().sum()) > 0, "no codebook gradient: the lookup backward did not run"
        out.update({f"step {i} {k}": torch.as_tensor(v).detach().float().cpu().clone() for k, v in ld.items()})
        out[f"step {i} indices"] = idx.detach().cpu().clone()
    torch.cuda.synchronize()
    for tag, module, opt in (("gen", model, og), ("disc", lm.disc_model, od)):
        for n, p in module.named_parameters():
            out[f"{tag} param {n}"] = p.detach().float().cpu()
            for k, v in opt.state.get(p, {}).items():
                if torch.is_tensor(v):
                    out[f"{tag} state {n} {k}"] = v.detach().float().cpu()
    return out


def test_gan_training_steps_are_bit_reproducible(det):
    """Three gan_training_steps from the same seeds, twice: every weight of the tokenizer (the codebook among them) and of the
    discriminator, all HipAdamW state and every logged scalar agree bit for bit."""
    a = _gan_train(3)
    assert any(" state " in k for k in a) and any(k.startswith("gen param quantize") for k in a) and any("perceptual" in k for k in a)
    _same(a, _gan_train(3), "three GAN training steps, second run")


def test_psnr_accumulator_is_bit_reproducible(det):
    from titok_video_amd.model.metrics.eval_metrics import EvalMetrics
    clips = synthetic_clips(SHAPES, seed=5, dtype=torch.bfloat16, device=DEV)
    recon = [(c.float() * 0.9 + 0.05).to(torch.bfloat16) for c in clips]
    accs = []
    for _ in range(3):
        m = EvalMetrics()
        assert m.names == ["psnr"]
        m.update(recon, clips)
        m.update(clips, recon)
        torch.cuda.synchronize()
        accs.append(m._acc.cpu())
    assert bits(accs[0]) == bits(accs[1]) == bits(accs[2])
    assert float(accs[0][1]) == 2 * sum(c.numel() for c in clips) and float(accs[0][0]) > 0
