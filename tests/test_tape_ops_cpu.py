"""tests/tape_ops_ref.py checked without a GPU: the host model of the fast GEGLU Phi meets the project's stated figures over every
finite bf16 gate with |g| <= 2^20, the float64 references agree with autograd through the oracle's gate and GEGLU, every case of
tests/test_hip_tape_ops.py is what its label says, and every bound rejects a result that is off by 4 x the bound.  Also the argument
checks of the new entry points: they return before any launch, so they run here."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import titok_oracle as O
from tests import tape_ops_ref as R
from tests.blockwise import bf16_store
from titok_video_amd import _lib


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------- the fast Phi
def test_fast_phi_meets_the_stated_figures():
    """max |g Phi~ - gelu| <= 2.6e-5 (ttv_common.h) and max |Phi~ + g phi - gelu'| <= 5.1e-5 (computed: 5.04e-5 at g = 0.4238), over
    all finite bf16 g with |g| <= 2^20 - and not beyond: the clamp at -8 leaves Phi~ = 1.01e-12, g Phi~ = -1.01e-12 |g|."""
    assert R.all_finite_bf16().numel() == 65280
    print(f"FAST_GELU_ERR {R.FAST_GELU_ERR:.4e}  FAST_DGELU_ERR {R.FAST_DGELU_ERR:.4e} at g = {R.FAST_DGELU_ARGMAX}")
    assert R.FAST_GELU_ERR <= 2.6e-5 * 1.02
    assert 5.0e-5 <= R.FAST_DGELU_ERR <= 5.1e-5
    assert abs(R.FAST_DGELU_ARGMAX - 0.4238) < 1e-3
    cdf, _ = R.fast_phi_model(np.float32([-8.0, -9.0, -2.0 ** 20, -2.0 ** 26]))
    assert np.all(cdf == cdf[0]) and 1.0e-12 < cdf[0] < 1.03e-12            # frozen by the clamp
    assert abs(cdf[2] * -2.0 ** 20) < 2.6e-5 < abs(cdf[3] * -2.0 ** 26)      # the stated figure holds at 2^20, not "over all g"


def test_fast_model_mismatch_count_sees_a_two_percent_coefficient():
    """The count of bf16 outputs that differ from bf16(host model) (fast_store_mismatch_limit) is what finds a slightly wrong polynomial
    under the output store: the g^5 coefficient off by 2 % moves thousands of the exhaustive sweep's outputs, the limit allows a few
    hundred - while the per-element bound, dominated by the store's half ulp, lets the same change through."""
    g, I = R.geglu_exhaustive_gates(96), 96
    x, dh = torch.randn(g.shape, generator=gen(0)).bfloat16(), torch.randn(g.shape, generator=gen(1)).bfloat16()
    u = torch.cat([x, g], 1)
    good = R.fast_geglu_backward_model(u, dh, I).bfloat16()
    off = R.fast_geglu_backward_model(u, dh, I, R.C5_FAST * 1.02).bfloat16()
    limit = R.fast_store_mismatch_limit(good.numel())
    assert int((good != off).sum()) > 10 * limit
    # the committed formula itself is inside the fast path's bound, stored or not
    ref = R.geglu_backward_ref(u, dh, I)
    assert R.worst_ratio(good, ref, R.geglu_backward_bound(u, dh, I, ref, "bf16", True, k=2.0)) <= 1.0
    assert R.worst_ratio(R.fast_geglu_backward_model(u, dh, I), ref, R.geglu_backward_bound(u, dh, I, ref, "f32", True, k=2.0)) <= 1.0


def test_one_bf16_store_is_half_an_ulp_not_two_to_the_minus_nine():
    """half_ulp(r) bounds bf16_store exactly and is attained; 2^-9 |r| is not a bound of a correctly rounded store."""
    r = torch.cat([torch.randn(100000, generator=gen(2), dtype=torch.float64) * 10.0 ** torch.randint(-6, 6, (100000,), generator=gen(3)),
                   torch.tensor([132608.0, 0.0, 1.0, -0.75])])
    err = (bf16_store(r) - r).abs()
    assert bool((err <= R.half_ulp(r)).all())
    assert float(err[-4]) == 512.0 == float(R.half_ulp(r)[-4]) and 512.0 > 2.0 ** -9 * 132608.0
    assert bool((R.half_ulp(r) <= R.U16 * r.abs()).all()) and float(R.half_ulp(r)[-3]) == 0.0


# ---------------------------------------------------------------------------------------------- references against the oracle
def test_gate_reference_agrees_with_the_oracles_attention_sublayer():
    """Attn.forward (oracle.attn_sublayer) on one-row sequences is out_proj(v * sigmoid(gate)): softmax over one key is 1.  With identity
    norm gain and out_proj, its value and its autograd gradient w.r.t. the to_qkv output are gate_forward_ref / gate_backward_ref; the
    oracle computes in float32, hence 64 * 2^-24."""
    n, d = 7, 64
    x = torch.randn(n, d, generator=gen(4))
    w = torch.randn(4 * d, d, generator=gen(5)) * d ** -0.5
    sd = {"p.pre_ln.weight": torch.ones(d), "p.to_qkv.weight": w.clone().requires_grad_(True), "p.out_proj.weight": torch.eye(d)}
    out = O.attn_sublayer(x, sd, "p.", (1, 1), torch.ones(n, 30), torch.zeros(n, 30), list(range(n + 1)))
    dag = torch.randn(n, d, generator=gen(6))
    out.backward(dag)
    qkv = torch.nn.functional.linear(O.rmsnorm(x, torch.ones(d)), w).detach()
    gate, v = qkv[:, d:2 * d], qkv[:, 3 * d:]
    ref = R.gate_forward_ref(v, gate)
    da, dgate = R.gate_backward_ref(dag, v, gate)
    tol = 64 * R.U32
    assert float((out.detach().double() - ref).abs().max()) <= tol * float(ref.abs().max())
    h = O.rmsnorm(x, torch.ones(d)).double()
    dw = sd["p.to_qkv.weight"].grad.double()           # dL/dW = dqkv^T h: compare the gate and v row blocks
    assert float((dw[d:2 * d] - dgate.T @ h).abs().max()) <= tol * float((dgate.abs().T @ h.abs()).max())
    assert float((dw[3 * d:] - da.T @ h).abs().max()) <= tol * float((da.abs().T @ h.abs()).max())
    assert float(dw[:d].abs().max()) <= tol and float(dw[2 * d:3 * d].abs().max()) <= tol       # q, k: no gradient through one key


def test_geglu_reference_agrees_with_the_oracles_geglu_sublayer():
    """GEGLU.forward (oracle.geglu_sublayer) with identity w12 and w3 is gelu(gate) * x of the normed input."""
    n, I = 9, 32
    x = (torch.randn(n, 2 * I, generator=gen(7)) * 2).requires_grad_(True)
    sd = {"p.norm.weight": torch.ones(2 * I), "p.w12.weight": torch.eye(2 * I), "p.w3.weight": torch.eye(I)}
    u = O.rmsnorm(x, torch.ones(2 * I))
    u.retain_grad()
    out = O.geglu_sublayer(x, sd, "p.")
    dh = torch.randn(n, I, generator=gen(8))
    u2 = O.rmsnorm(x.detach(), torch.ones(2 * I)).requires_grad_(True)          # gradient w.r.t. the GEGLU input alone
    h2 = torch.nn.functional.gelu(u2[:, I:]) * u2[:, :I]
    h2.backward(dh)
    assert torch.equal(h2.detach(), out.detach())
    ref, du = R.geglu_forward_ref(u2.detach(), I), R.geglu_backward_ref(u2.detach(), dh, I)
    tol = 64 * R.U32
    assert float((out.detach().double() - ref).abs().max()) <= tol * float(ref.abs().max())
    assert float((u2.grad.double() - du).abs().max()) <= tol * float(du.abs().max())


# ---------------------------------------------------------------------------------------------- the cases are what they say
def test_cases_cross_the_grid_cap_and_select_the_fallback():
    cap = R.GRID_CAP
    assert R.GATE_CAP["rows"] * R.GATE_CAP["d"] // 4 == cap + 64
    assert R.GEGLU_FWD_CAP["rows"] * R.GEGLU_FWD_CAP["I"] // 4 > cap and R.GEGLU_BWD_CAP["rows"] * R.GEGLU_BWD_CAP["I"] // 8 > cap
    assert R.SCALE_CAST_N[-1] // 4 == cap + 1 and all(n % 4 == 0 for n in R.SCALE_CAST_N) and R.SCALE_CAST_REFUSED_N % 4 != 0
    assert R.EXPAND_CAP["rows"] * R.EXPAND_CAP["d"] > cap
    for I in R.GEGLU_INNER + (R.GEGLU_BWD_CAP["I"],):
        lay = R.geglu_layout(I)
        assert R.geglu_v8(lay) and lay["ldu"] > 2 * I and lay["ldh"] > I and lay["lddh"] > I and lay["lddu"] > 2 * I
    assert sorted(R.GEGLU_FALLBACK) == ["I100", "dh_off", "lddu"]
    for name, lay in R.GEGLU_FALLBACK.items():
        assert not R.geglu_v8(lay), name
        I = lay["I"]                                   # ... and each is still a legal call: multiples of 4, 4-element aligned
        assert I % 4 == 0 and all(lay[k] % 4 == 0 for k in ("ldu", "ldh", "lddh", "lddu")) and lay["dh_off"] % 4 == 0
    # one demand fails in each: the inner size, lddu, dh's address
    assert R.GEGLU_FALLBACK["I100"]["I"] % 8 and R.GEGLU_FALLBACK["lddu"]["lddu"] % 8 and R.GEGLU_FALLBACK["dh_off"]["dh_off"] * 2 % 16
    g = R.geglu_exhaustive_gates(96)
    want = R.all_finite_bf16(R.FAST_DOMAIN)
    assert g.shape[1] == 96 and torch.equal(g.flatten()[:want.numel()].view(torch.int16), want.view(torch.int16))
    assert float(want.double().abs().max()) == 2.0 ** 20 and g.numel() >= 8 * want.numel()
    assert R.DEC_EMBED_C[0] <= _lib.TTV_MAX_FSQ < R.DEC_EMBED_C[1] and R.DEC_EMBED_C[1] % 4 == 0 and R.DEC_EMBED_C[2] % 4 != 0 and R.DEC_EMBED_C[2] > _lib.TTV_MAX_FSQ
    assert R.GATE_WIDTH_NO_DELTA % 64 != 0 and R.GATE_WIDTH_NO_DELTA % 4 == 0 and all(d % 64 == 0 for d in R.GATE_WIDTHS)


# ---------------------------------------------------------------------------------------------- no bound is vacuous
def _rejects(ref, bound):
    """ref passes; ref off by 4 x the bound in one element (the one with the smallest bound, and the largest) fails."""
    assert bool(torch.isfinite(bound).all()) and bool((bound > 0).all())
    assert R.worst_ratio(ref, ref, bound) == 0.0
    for i in (int(bound.argmin()), int(bound.argmax())):
        off = ref.clone()
        off.view(-1)[i] += 4.0 * bound.view(-1)[i]
        assert R.worst_ratio(off, ref, bound) > 3.9
    nan = ref.clone()
    nan.view(-1)[0] = float("nan")
    assert R.worst_ratio(nan, ref, bound) == float("inf")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_every_bound_rejects_four_times_itself(dt):
    T = R.DT[dt]
    rows, d, I = 5, 64, 32
    a, gate, dag = (torch.randn(rows, d, generator=gen(s)).to(T) for s in (10, 11, 12))
    gate = gate * 6
    ref = R.gate_forward_ref(a, gate)
    _rejects(ref, R.gate_forward_bound(a, gate, ref, dt))
    da, dg = R.gate_backward_ref(dag, a, gate)
    for r, b in zip((da, dg), R.gate_backward_bounds(dag, a, gate, da, dg, dt)):
        _rejects(r, b)
    _rejects(*R.delta_ref(da, a, dt))
    u, dh = (torch.randn(rows, 2 * I, generator=gen(13)) * 3).to(T), torch.randn(rows, I, generator=gen(14)).to(T)
    ref = R.geglu_forward_ref(u, I)
    _rejects(ref, R.geglu_forward_bound(u, I, ref, dt))
    du = R.geglu_backward_ref(u, dh, I)
    _rejects(du, R.geglu_backward_bound(u, dh, I, du, dt, fast=False))
    _rejects(du, R.geglu_backward_bound(u, dh, I, du, dt, fast=True))
    av, w = torch.randn(rows, 5, generator=gen(15)), torch.randn(5, d, generator=gen(16)).to(T)
    _rejects(*R.expand_small_ref(av, w, 1, dt))
    _rejects(*R.reduce_small_ref(a, torch.tensor([4, 0, 2, 1, 3]), torch.randn(d, 5, generator=gen(17)).to(T)))
    for mask in R.CONST_ROWS_MASK:
        colsum, gain = torch.randn(d, generator=gen(18)), 1 + 0.1 * torch.randn(d, generator=gen(19))
        dgain, dmask, eg, em = R.const_rows_backward_ref(colsum, mask, gain, 1e-5, torch.ones(d), torch.tensor([2.0]), dt)
        _rejects(dgain, eg)
        _rejects(dmask, em)
        if mask == 0.0:      # dgain += 0, dmask += sum colsum gain / sqrt(eps)
            assert torch.equal(dgain, torch.ones(d, dtype=torch.float64))
            assert abs(float(dmask) - 2.0 - float((colsum.double() * gain.double()).sum()) / 1e-5 ** 0.5) < 1e-9 * abs(float(dmask))
    cos, sin = O.rope_table([(1, 2, 2)], [1])
    cs = R.rope_cs_table(cos, sin)
    x = torch.randn(cs.shape[0], 128, generator=gen(20)).to(T)
    for conj in (0, 1):
        out, mag = R.rope_ref(x, cs, 2, conj)
        _rejects(out, R.K_ROPE * R.U32 * mag + R.TINY + R.store(out, dt))
    back, _ = R.rope_ref(R.rope_ref(x, cs, 2, 0)[0], cs, 2, 1)          # the table's cos^2 + sin^2 is 1 to fp32 rounding
    assert float(((back - x.double()).abs() / R.pair_norm(x, 2)).max()) < 2 * R.U32
    codes, w, bias = torch.randn(rows, 13, generator=gen(21)).to(T), torch.randn(d, 13, generator=gen(22)).to(T), torch.randn(d, generator=gen(23)).to(T)
    _rejects(*R.dec_embed_hpre_ref(codes, w, bias, 0.3, dt))


# ---------------------------------------------------------------------------------------------- argument checks (no launch)
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


def test_entry_points_refuse_bad_arguments_before_any_launch(lib):
    """TTV_ERR_INVALID (1) for a width, leading dimension, pointer or count that is not in whole 4-element vectors, for delta with a
    width that is not whole heads, for exactly one of dgain / dmask, for an unsupported dtype triple; rows == 0 accepts NULL."""
    buf = (C.c_float * 4096)()
    base = (C.addressof(buf) + 63) // 64 * 64
    p, q, r = base, base + 4096, base + 8192
    bf, f32 = _lib.TTV_BF16, _lib.TTV_F32
    bad = [
        ("gate_forward width % 4", lib.ttv_gate_forward(p, 72, q, 72, r, 72, 2, 66, f32, None)),
        ("gate_forward ld < width", lib.ttv_gate_forward(p, 64, q, 60, r, 64, 2, 64, f32, None)),
        ("gate_forward ld % 4", lib.ttv_gate_forward(p, 66, q, 64, r, 64, 2, 64, bf, None)),
        ("gate_forward pointer", lib.ttv_gate_forward(p + 4, 64, q, 64, r, 64, 2, 64, bf, None)),
        ("gate_forward null", lib.ttv_gate_forward(None, 64, q, 64, r, 64, 2, 64, bf, None)),
        ("gate_forward dtype", lib.ttv_gate_forward(p, 64, q, 64, r, 64, 2, 64, 7, None)),
        ("gate_backward delta at 68", lib.ttv_gate_backward(p, 68, q, 68, r, 68, p, 68, q, 68, 2, 68, f32, r, None)),
        ("gate_backward ld % 4", lib.ttv_gate_backward(p, 64, q, 64, r, 64, p, 64, q, 70, 2, 64, f32, None, None)),
        ("gate_backward pointer", lib.ttv_gate_backward(p, 64, q, 64, r, 64, p + 8, 64, q, 64, 2, 64, f32, None, None)),
        ("geglu_forward inner % 4", lib.ttv_geglu_forward(p, 64, q, 32, 2, 30, bf, None)),
        ("geglu_forward ldu < 2 I", lib.ttv_geglu_forward(p, 60, q, 32, 2, 32, bf, None)),
        ("geglu_backward lddu % 4", lib.ttv_geglu_backward(p, 64, q, 32, r, 66, 2, 32, bf, None)),
        ("geglu_backward pointer", lib.ttv_geglu_backward(p, 64, q + 2, 32, r, 64, 2, 32, bf, None)),
        ("scale_cast n % 4", lib.ttv_scale_cast(p, 1.0, q, r, bf, R.SCALE_CAST_REFUSED_N, None)),
        ("scale_cast pointer", lib.ttv_scale_cast(p, 1.0, q + 4, r, bf, 8, None)),
        ("cast_to_f32 n % 4", lib.ttv_cast_to_f32(p, bf, q, 6, 0, None)),
        ("cast_to_f32 pointer", lib.ttv_cast_to_f32(p + 2, bf, q, 8, 0, None)),
        ("expand_small dtypes", lib.ttv_expand_small(p, bf, 5, 5, q, bf, 64, 1, r, bf, 64, 2, 64, None)),
        ("reduce_small dtypes", lib.ttv_reduce_small(p, bf, 64, None, q, f32, 5, 5, r, 5, 2, 64, None)),
        ("const_rows_backward dgain only", lib.ttv_const_rows_backward(p, q, r, f32, 1e-5, p, None, 64, None)),
        ("const_rows_backward dmask only", lib.ttv_const_rows_backward(p, q, r, f32, 1e-5, None, p, 64, None)),
        ("rope_apply_conj ld", lib.ttv_rope_apply_conj(p, f32, 60, 2, 1, q, None)),
        ("decoder_embed_tape ld", lib.ttv_decoder_embed_tape(p, 5, q, r, p, q, r, f32, 62, p, 2, 64, 1e-5, None, None)),
        ("negative rows", lib.ttv_gate_forward(p, 64, q, 64, r, 64, -1, 64, f32, None)),
    ]
    for what, rc in bad:
        assert rc == 1, what
    assert lib.ttv_gate_backward(p, 68, q, 68, r, 68, p, 68, q, 68, 2, 68, f32, r, None) == 1 and b"delta" in lib.ttv_error_string()
    ok = [
        lib.ttv_gate_forward(None, 0, None, 0, None, 0, 0, 64, bf, None),
        lib.ttv_gate_backward(None, 0, None, 0, None, 0, None, 0, None, 0, 0, 64, bf, None, None),
        lib.ttv_geglu_forward(None, 0, None, 0, 0, 96, bf, None),
        lib.ttv_geglu_backward(None, 0, None, 0, None, 0, 0, 96, bf, None),
        lib.ttv_scale_cast(None, 1.0, None, None, bf, 0, None),
        lib.ttv_cast_to_f32(None, bf, None, 0, 1, None),
        lib.ttv_expand_small(None, f32, 0, 5, None, bf, 0, 1, None, bf, 0, 0, 64, None),
        lib.ttv_reduce_small(None, f32, 0, None, None, f32, 0, 5, None, 0, 0, 64, None),
        lib.ttv_const_rows_backward(None, None, None, f32, 1e-5, None, None, 64, None),
        lib.ttv_rope_apply_conj(None, bf, 0, 0, 4, None, None),
        lib.ttv_decoder_embed_tape(None, 5, None, None, None, None, None, bf, 0, None, 0, 64, 1e-5, None, None),
    ]
    assert ok == [0] * len(ok)
