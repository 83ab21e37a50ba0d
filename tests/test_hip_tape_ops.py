"""The training tape's elementwise and small-projection kernels (ttv_bwd.hip, ttv_elem.hip), one op at a time against float64
references - the kernels between the GEMMs, attention and the norms, which the tower gradient tests reach only through whole towers.

References, bounds and case lists: tests/tape_ops_ref.py (its docstring derives |got - r| <= E32 + half_ulp(r) + A; checked on the CPU
by tests/test_tape_ops_cpu.py).  Every output is allocated with a leading dimension larger than its width and one extra row, filled with
NaN: padding and the extra row must stay NaN, everything inside must be finite.  Inputs sit at non-trivial leading dimensions; the gate
and a come from inside one (q | gate | k | v) row.  `check` prints a MEASURED line per comparison before it asserts - the worst
|got - r| as a fraction of the bound, for the fp32 path also in units of 2^-24 cond (what K_GATE / K_GEGLU are set from) and as a plain
relative error; profiles/tape_ops_bounds.txt keeps the figures of one MI355X run."""
import gc

import pytest
import torch

from oracle import titok_oracle as O
from tests import tape_ops_ref as R
from tests.test_hip_ops import assert_close
from titok_video_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


@pytest.fixture
def leave_no_device_memory_behind():
    """The grid-cap cases hold a few hundred MB of float64 references on the device: collected and returned before the next test."""
    yield
    gc.collect()
    torch.cuda.empty_cache()


def L():
    return _lib.lib()


def S():
    return _lib.stream_ptr(torch.device(DEV))


def gen(seed):
    return torch.Generator().manual_seed(seed)


def code(dt):
    return _lib.dtype_code(R.DT[dt])


def nan_out(rows, ld, T):
    return torch.full((rows + 1, ld), NAN, dtype=T, device=DEV)


def untouched(out, rows, width):
    """Padding columns and the extra row are still NaN."""
    return bool(torch.isnan(out[rows:]).all()) and bool(torch.isnan(out[:rows, width:]).all())


def check(what, got, ref, bound, k=None):
    """Assert |got - ref| <= bound everywhere (and got finite).  k: the fp32 path's E32 constant inside `bound` - the worst error is then
    also printed in units of 2^-24 cond."""
    ratio, rel = R.worst_ratio(got, ref, bound), R.worst_relative(got, ref)
    unit = f", {ratio * k:.2f} x 2^-24 cond (k = {k})" if k is not None else ""
    print(f"MEASURED {what}: worst |got - r| / bound {ratio:.3f}{unit}, worst relative {rel:.2e}")
    assert ratio <= 1.0, f"{what}: |got - r| reaches {ratio:.3f} x its bound"


# ---------------------------------------------------------------------------------------------- gate
def run_gate(dt, rows, d, seed, gate_vals=None, want_delta=True, on_device=False):
    """Forward, backward and delta at (rows, d); returns the pieces the callers look at further."""
    T, c = R.DT[dt], code(dt)
    nq = 2 * d + 128                                            # q | gate | k | v with two kv heads
    g = gen(seed)
    qkvg = torch.randn(rows, nq, generator=g)
    qkvg[:, d:2 * d] = gate_vals if gate_vals is not None else qkvg[:, d:2 * d] * 4
    dag = torch.randn(rows, d + 4, generator=g)
    qkvg_d, dag_d = qkvg.to(T).to(DEV), dag.to(T).to(DEV)
    a_d, gate_d = qkvg_d[:, :d], qkvg_d[:, d:2 * d]
    ag, da, dgate = nan_out(rows, d + 8, T), nan_out(rows, d + 4, T), nan_out(rows, nq, T)
    delta = torch.full((rows + 1, max(d // 64, 1)), NAN, dtype=torch.float32, device=DEV)
    _lib.check(L().ttv_gate_forward(a_d.data_ptr(), nq, gate_d.data_ptr(), nq, ag.data_ptr(), d + 8, rows, d, c, S()), "gate_forward")
    _lib.check(L().ttv_gate_backward(dag_d.data_ptr(), d + 4, a_d.data_ptr(), nq, gate_d.data_ptr(), nq, da.data_ptr(), d + 4, dgate.data_ptr(), nq,
                                     rows, d, c, delta.data_ptr() if want_delta else None, S()), "gate_backward")
    torch.cuda.synchronize()
    assert untouched(ag, rows, d) and untouched(da, rows, d) and untouched(dgate, rows, d)
    where = DEV if on_device else "cpu"
    a, gate, dg = a_d.to(where), gate_d.to(where), dag_d[:, :d].to(where)
    k = R.K_GATE if dt == "f32" else None
    tag = f"gate {dt} rows {rows} d {d}"
    ref = R.gate_forward_ref(a, gate)
    check(f"{tag} ag", ag[:rows, :d].to(where), ref, R.gate_forward_bound(a, gate, ref, dt), k)
    da_ref, dgate_ref = R.gate_backward_ref(dg, a, gate)
    e_da, e_dg = R.gate_backward_bounds(dg, a, gate, da_ref, dgate_ref, dt)
    check(f"{tag} da", da[:rows, :d].to(where), da_ref, e_da, k)
    check(f"{tag} dgate", dgate[:rows, :d].to(where), dgate_ref, e_dg, k)
    if want_delta:
        # delta is defined on da as the kernel stored it; every (row, head) written, the extra row not
        assert bool(torch.isnan(delta[rows:]).all()) and not bool(torch.isnan(delta[:rows]).any())
        d_ref, d_bound = R.delta_ref(da[:rows, :d].to(where), a, dt)
        check(f"{tag} delta", delta[:rows].to(where), d_ref, d_bound)
    else:
        assert bool(torch.isnan(delta).all())
    return a_d, gate_d, dag_d[:, :d], ag[:rows, :d], da[:rows, :d], dgate[:rows, :d]


@pytest.mark.parametrize("rows", R.ROWS)
@pytest.mark.parametrize("d", R.GATE_WIDTHS + (R.GATE_WIDTH_NO_DELTA,))
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_gate(dt, d, rows):
    """ag = a sigmoid(gate), da, dgate against float64 autograd; delta against the float64 sum of (da as stored) * a per 64-wide head.
    Width 68 (not whole heads) runs without delta, and asking for delta there is refused."""
    run_gate(dt, rows, d, seed=1000 * d + rows, want_delta=d % 64 == 0)
    if d % 64:
        p = torch.zeros(4 * d, device=DEV).data_ptr()
        assert L().ttv_gate_backward(p, d, p, d, p, d, p, d, p, d, 1, d, code(dt), p, S()) == 1


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_gate_exhaustive(dt):
    """The gate takes every finite bf16 value (255 x 256): sigma and sigma (1 - sigma) across both saturations.  sigma(-big) is exactly
    0, sigma(+big) exactly 1 with dgate = 0, nothing is NaN."""
    vals = R.all_finite_bf16().float().view(255, 256)
    a, gate, dag, ag, da, dgate = run_gate(dt, 255, 256, seed=7, gate_vals=vals)
    lo, hi = (gate.float() <= -128.0), (gate.float() >= 128.0)
    assert int(lo.sum()) > 10000 and int(hi.sum()) > 10000
    assert bool((ag[lo] == 0).all()) and bool((da[lo] == 0).all()) and bool((dgate[lo] == 0).all())
    assert bool((ag[hi] == a[hi]).all()) and bool((da[hi] == dag[hi]).all()) and bool((dgate[hi] == 0).all())


def test_gate_crosses_the_grid_cap_and_runs_in_place(leave_no_device_memory_behind):
    """rows = 32 769, d = 256 in bf16: 8192 * 256 + 64 four-wide items, so the capped grid takes a second stride (references in float64
    on the device).  Then the forward with ag = a: every element is read and written exactly once, a second visit would gate it twice."""
    rows, d = R.GATE_CAP["rows"], R.GATE_CAP["d"]
    a, gate, _, ag, _, _ = run_gate("bf16", rows, d, seed=11, on_device=True)
    buf = a.clone().contiguous()
    _lib.check(L().ttv_gate_forward(buf.data_ptr(), d, gate.data_ptr(), 2 * d + 128, buf.data_ptr(), d, rows, d, code("bf16"), S()), "gate_forward in place")
    assert torch.equal(buf, ag)


# ---------------------------------------------------------------------------------------------- GEGLU
def run_geglu(dt, rows, lay, seed, gates=None, on_device=False, model_count=False, backward_only=False):
    """Forward and backward for one layout (tape_ops_ref.geglu_layout); returns (u, dh, du as stored, du reference, du bound)."""
    T, c, I = R.DT[dt], code(dt), lay["I"]
    g = gen(seed)
    u = torch.randn(rows, lay["ldu"], generator=g)
    u[:, I:2 * I] = gates.float() if gates is not None else u[:, I:2 * I] * 2.5
    dhb = torch.randn(rows * lay["lddh"] + lay["dh_off"], generator=g)
    u_d, dhb_d = u.to(T).to(DEV), dhb.to(T).to(DEV)
    dh_d = dhb_d[lay["dh_off"]:].view(rows, lay["lddh"])
    h, du = nan_out(rows, lay["ldh"], T), nan_out(rows, lay["lddu"], T)
    fast = dt == "bf16" and R.geglu_v8(lay, 2, u_d.data_ptr(), dhb_d.data_ptr(), du.data_ptr())
    assert fast == (dt == "bf16" and R.geglu_v8(lay)), "the buffers are 16-byte aligned: the layout alone decides the kernel"
    if not backward_only:
        _lib.check(L().ttv_geglu_forward(u_d.data_ptr(), lay["ldu"], h.data_ptr(), lay["ldh"], rows, I, c, S()), "geglu_forward")
    _lib.check(L().ttv_geglu_backward(u_d.data_ptr(), lay["ldu"], dh_d.data_ptr(), lay["lddh"], du.data_ptr(), lay["lddu"], rows, I, c, S()), "geglu_backward")
    torch.cuda.synchronize()
    assert untouched(du, rows, 2 * I) and (backward_only or untouched(h, rows, I))
    where = DEV if on_device else "cpu"
    uu, dh = u_d[:, :2 * I].to(where), dh_d[:, :I].to(where)
    k = R.K_GEGLU if dt == "f32" else None
    tag = f"geglu {dt} rows {rows} I {I} lddu {lay['lddu']} dh_off {lay['dh_off']} ({'8-wide fast' if fast else '4-wide erf'})"
    if not backward_only:
        ref = R.geglu_forward_ref(uu, I)
        check(f"{tag} h", h[:rows, :I].to(where), ref, R.geglu_forward_bound(uu, I, ref, dt), k)
    du_ref = R.geglu_backward_ref(uu, dh, I)
    du_bound = R.geglu_backward_bound(uu, dh, I, du_ref, dt, fast)
    got = du[:rows, :2 * I].to(where)
    check(f"{tag} du[:, :I]", got[:, :I], du_ref[:, :I], du_bound[:, :I], k)
    check(f"{tag} du[:, I:]", got[:, I:], du_ref[:, I:], du_bound[:, I:], k)
    if model_count:
        # under the store's half ulp the bound cannot see a slightly wrong polynomial: the stored values against bf16(host model of
        # the committed formula), which may differ only where v_exp_f32 / v_rcp_f32's last ulp moves a value across a rounding boundary
        assert fast
        model = R.fast_geglu_backward_model(uu.cpu(), dh.cpu(), I).bfloat16()
        n_off, limit = int((model != got.cpu()).sum()), R.fast_store_mismatch_limit(model.numel())
        print(f"MEASURED {tag}: {n_off} of {model.numel()} outputs differ from bf16(host model), limit {limit}")
        assert n_off <= limit
    return uu, dh, got, du_ref, du_bound


@pytest.mark.parametrize("rows", R.ROWS)
@pytest.mark.parametrize("I", R.GEGLU_INNER)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_geglu(dt, I, rows):
    """GEGLU and its gradient against float64 autograd: fp32 (erff) and bf16 on the 8-wide fast-Phi kernel."""
    run_geglu(dt, rows, R.geglu_layout(I), seed=100 * I + rows, model_count=dt == "bf16" and rows == 257)


@pytest.mark.parametrize("rows", R.ROWS)
@pytest.mark.parametrize("name", sorted(R.GEGLU_FALLBACK))
def test_geglu_bf16_fallback(name, rows):
    """The 4-wide bf16 kernel, reached three ways: I % 8 != 0, a leading dimension that is no multiple of 8, dh 8 bytes off 16-byte
    alignment.  Its bound has no approximation term (erff / expf in fp32, one store)."""
    run_geglu("bf16", rows, R.GEGLU_FALLBACK[name], seed=1000 * sorted(R.GEGLU_FALLBACK).index(name) + rows)


def test_geglu_exhaustive_both_bf16_kernels(leave_no_device_memory_behind):
    """g takes every finite bf16 value with |g| <= 2^20 (eight x, dh each) through the 8-wide and the 4-wide kernel; each within its own
    bound, and the two within the sum of their bounds of each other."""
    gates = R.geglu_exhaustive_gates(96)
    rows = gates.shape[0]
    _, _, fast, _, b_fast = run_geglu("bf16", rows, R.geglu_layout(96), seed=5, gates=gates, model_count=True)
    _, _, slow, _, b_slow = run_geglu("bf16", rows, R.geglu_layout(96, "lddu"), seed=5, gates=gates)
    check("geglu bf16 exhaustive: 8-wide against 4-wide", fast, slow.double(), b_fast + b_slow)


def test_geglu_crosses_the_grid_cap(leave_no_device_memory_behind):
    """Forward at rows = 6100 and the 8-wide backward at rows = 12 200 with I = 1376: both grids are capped and take a second stride."""
    I = R.GEGLU_FWD_CAP["I"]
    T = torch.bfloat16
    rows = R.GEGLU_FWD_CAP["rows"]
    lay = R.geglu_layout(I)
    u = (torch.randn(rows, lay["ldu"], generator=gen(21)) * 2.5).to(T).to(DEV)
    h = nan_out(rows, lay["ldh"], T)
    _lib.check(L().ttv_geglu_forward(u.data_ptr(), lay["ldu"], h.data_ptr(), lay["ldh"], rows, I, code("bf16"), S()), "geglu_forward")
    assert untouched(h, rows, I)
    ref = R.geglu_forward_ref(u[:, :2 * I], I)
    check(f"geglu bf16 rows {rows} I {I} h (grid cap)", h[:rows, :I], ref, R.geglu_forward_bound(u[:, :2 * I], I, ref, "bf16"))
    run_geglu("bf16", R.GEGLU_BWD_CAP["rows"], R.geglu_layout(R.GEGLU_BWD_CAP["I"]), seed=22, on_device=True, backward_only=True)


# ---------------------------------------------------------------------------------------------- scale_cast / cast_to_f32
@pytest.mark.parametrize("n", R.SCALE_CAST_N)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_scale_cast_is_exact(dt, n):
    """b = alpha a is one fp32 multiply, c = (T) a one store (or a copy): bit for bit; b aliasing a, b = NULL, c = NULL; the four
    elements behind n are left alone."""
    T, alpha = R.DT[dt], 0.3
    a = torch.randn(n, generator=gen(n)).to(DEV)
    want_b, want_c = a * alpha, a.to(T)
    for b_mode, c_on in (("own", True), ("alias", True), (None, True), ("own", False)):
        src = torch.cat([a, torch.full((4,), NAN, device=DEV)])
        b = src if b_mode == "alias" else torch.full((n + 4,), NAN, device=DEV)
        c = torch.full((n + 4,), NAN, dtype=T, device=DEV)
        _lib.check(L().ttv_scale_cast(src.data_ptr(), alpha, b.data_ptr() if b_mode else None, c.data_ptr() if c_on else None, code(dt), n, S()),
                   "scale_cast")
        assert bool(torch.isnan(b[n:]).all()) and bool(torch.isnan(c[n:]).all()) and bool(torch.isnan(src[n:]).all())
        assert torch.equal(b[:n], want_b) if b_mode else bool(torch.isnan(b).all())
        assert torch.equal(c[:n], want_c) if c_on else bool(torch.isnan(c).all())
        if b_mode != "alias":
            assert torch.equal(src[:n], a)
    assert L().ttv_scale_cast(a.data_ptr(), alpha, a.data_ptr(), None, code(dt), R.SCALE_CAST_REFUSED_N, S()) == 1      # no silent tail


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("n", R.SCALE_CAST_N)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_cast_to_f32_is_exact(dt, n, accumulate):
    T = R.DT[dt]
    a = torch.randn(n, generator=gen(n + 1)).to(T).to(DEV)
    old = torch.randn(n, generator=gen(n + 2)).to(DEV)
    b = torch.cat([old, torch.full((4,), NAN, device=DEV)])
    _lib.check(L().ttv_cast_to_f32(a.data_ptr(), code(dt), b.data_ptr(), n, accumulate, S()), "cast_to_f32")
    assert torch.equal(b[:n], a.float() + old if accumulate else a.float()) and bool(torch.isnan(b[n:]).all())
    assert L().ttv_cast_to_f32(a.data_ptr(), code(dt), b.data_ptr(), R.SCALE_CAST_REFUSED_N, accumulate, S()) == 1


# ---------------------------------------------------------------------------------------------- expand_small / reduce_small
EXPAND_TRIPLES = [("f32", "bf16", "bf16"), ("f32", "f32", "f32"), ("f32", "bf16", "f32")]
REDUCE_PAIRS = [("bf16", "bf16"), ("f32", "f32"), ("f32", "bf16")]


def run_expand(C, d, rows, triple, w_cf, seed):
    a_dt, w_dt, o_dt = triple
    g = gen(seed)
    lda, ldw, ldo = C + 3, (d if w_cf else C) + 5, d + 7
    a = torch.randn(rows, lda, generator=g).to(R.DT[a_dt]).to(DEV)
    w = torch.randn((C if w_cf else d), ldw, generator=g).to(R.DT[w_dt]).to(DEV)
    out = nan_out(rows, ldo, R.DT[o_dt])
    _lib.check(L().ttv_expand_small(a.data_ptr(), code(a_dt), lda, C, w.data_ptr(), code(w_dt), ldw, w_cf, out.data_ptr(), code(o_dt), ldo, rows, d, S()),
               "expand_small")
    assert untouched(out, rows, d)
    big = rows > 1000
    av, wv = a[:, :C], w[:, :(d if w_cf else C)]
    ref, bound = R.expand_small_ref(av if big else av.cpu(), wv if big else wv.cpu(), w_cf, o_dt)
    check(f"expand_small {triple} C {C} d {d} rows {rows} w_cf {w_cf}", out[:rows, :d], ref, bound)


@pytest.mark.parametrize("w_cf", [0, 1], ids=["w_fc", "w_cf"])
@pytest.mark.parametrize("triple", EXPAND_TRIPLES, ids=["-".join(t) for t in EXPAND_TRIPLES])
@pytest.mark.parametrize("d", R.SMALL_D)
@pytest.mark.parametrize("C", R.SMALL_C)
def test_expand_small(C, d, triple, w_cf):
    """out[r, f] = sum_c a[r, c] w[c, f] (w_cf) or w[f, c]: both orientations, the three dtype triples, C 2^-24 sum |terms| + the store."""
    for rows in R.ROWS:
        run_expand(C, d, rows, triple, w_cf, seed=C * d + rows + w_cf)


def test_expand_small_crosses_the_grid_cap_and_refuses_other_dtypes(leave_no_device_memory_behind):
    run_expand(5, R.EXPAND_CAP["d"], R.EXPAND_CAP["rows"], EXPAND_TRIPLES[0], 1, seed=31)
    p = torch.zeros(4096, device=DEV).data_ptr()
    assert L().ttv_expand_small(p, code("bf16"), 5, 5, p, code("bf16"), 64, 1, p, code("bf16"), 64, 2, 64, S()) == 1
    assert L().ttv_reduce_small(p, code("bf16"), 64, None, p, code("f32"), 5, 5, p, 5, 2, 64, S()) == 1


@pytest.mark.parametrize("pair", REDUCE_PAIRS, ids=["-".join(t) for t in REDUCE_PAIRS])
@pytest.mark.parametrize("d", R.SMALL_D)
@pytest.mark.parametrize("C", R.SMALL_C)
def test_reduce_small(C, d, pair):
    """out[r, c] = sum_f a[a_rows[r]][f] w[f, c] in fp32: identity and permuted row maps, (d / 64 + 6) 2^-24 sum |terms|."""
    a_dt, w_dt = pair
    for rows in R.ROWS:
        g = gen(C * d + rows)
        lda, ldw, ldo = d + 4, C + 3, C + 2
        a = torch.randn(rows + 2, lda, generator=g).to(R.DT[a_dt]).to(DEV)
        w = torch.randn(d, ldw, generator=g).to(R.DT[w_dt]).to(DEV)
        for perm in (None, torch.randperm(rows + 2, generator=g)[:rows].to(torch.int32)):
            out = nan_out(rows, ldo, torch.float32)
            pd = perm.to(DEV) if perm is not None else None
            _lib.check(L().ttv_reduce_small(a.data_ptr(), code(a_dt), lda, _lib.ptr(pd), w.data_ptr(), code(w_dt), ldw, C, out.data_ptr(), ldo, rows, d, S()),
                       "reduce_small")
            assert untouched(out, rows, C)
            ref, bound = R.reduce_small_ref(a[:, :d].cpu() if perm is not None else a[:rows, :d].cpu(), perm, w[:, :C].cpu())
            check(f"reduce_small {pair} C {C} d {d} rows {rows} {'permuted' if perm is not None else 'identity'}", out[:rows, :C], ref, bound)


# ---------------------------------------------------------------------------------------------- const_rows_backward
@pytest.mark.parametrize("d", R.CONST_ROWS_D)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_const_rows_backward(dt, d):
    """dgain and dmask accumulate into non-zero values, against float64 autograd of v[f] = m rsqrt(m^2 + eps) gain[f] contracted with
    colsum (bf16: m = bf16_store(mask), straight through) at mask in {0, 1e-3, 0.7, -3}.  Both NULL: a no-op.  Exactly one NULL is refused
    by the launcher (the kernel writes both unconditionally): asserted from the return code, nothing is launched."""
    eps = 1e-5
    for i, mask in enumerate(R.CONST_ROWS_MASK):
        g = gen(d + i)
        colsum, gain = torch.randn(d, generator=g), 1 + 0.1 * torch.randn(d, generator=g)
        dgain0, dmask0 = torch.randn(d, generator=g), torch.tensor([1.5])
        dgain = torch.cat([dgain0, torch.full((4,), NAN)]).to(DEV)
        dmask = torch.tensor([1.5, NAN], device=DEV)
        cs_d, m_d, g_d = colsum.to(DEV), torch.tensor([mask], device=DEV), gain.to(DEV)
        _lib.check(L().ttv_const_rows_backward(cs_d.data_ptr(), m_d.data_ptr(), g_d.data_ptr(), code(dt), eps, dgain.data_ptr(), dmask.data_ptr(), d, S()),
                   "const_rows_backward")
        assert bool(torch.isnan(dgain[d:]).all()) and bool(torch.isnan(dmask[1:]).all())
        r_gain, r_mask, e_gain, e_mask = R.const_rows_backward_ref(colsum, mask, gain, eps, dgain0, dmask0, dt)
        check(f"const_rows_backward {dt} d {d} mask {mask} dgain", dgain[:d], r_gain, e_gain)
        check(f"const_rows_backward {dt} d {d} mask {mask} dmask", dmask[:1], r_mask, e_mask)
        if mask == 0.0:
            assert torch.equal(dgain[:d].cpu(), dgain0)
        before = (dgain[:d].clone(), dmask[:1].clone())
        assert L().ttv_const_rows_backward(cs_d.data_ptr(), m_d.data_ptr(), g_d.data_ptr(), code(dt), eps, None, None, d, S()) == 0
        assert L().ttv_const_rows_backward(cs_d.data_ptr(), m_d.data_ptr(), g_d.data_ptr(), code(dt), eps, dgain.data_ptr(), None, d, S()) == 1
        assert L().ttv_const_rows_backward(cs_d.data_ptr(), m_d.data_ptr(), g_d.data_ptr(), code(dt), eps, None, dmask.data_ptr(), d, S()) == 1
        torch.cuda.synchronize()
        assert torch.equal(dgain[:d], before[0]) and torch.equal(dmask[:1], before[1])          # neither call added anything


# ---------------------------------------------------------------------------------------------- inverse rotary
@pytest.mark.parametrize("heads", [4, 12])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_rope_apply_conj(dt, heads):
    """The inverse rotation on a ragged batch with the oracle's factor table: conj is the float64 rotation by -theta, and apply then
    conj returns the input - within 4 * 2^-24 of each pair's norm in fp32, within two bf16 stores (2^-8 of the pair's norm each) in bf16."""
    T = R.DT[dt]
    grids, counts = [(1, 2, 3), (2, 4, 4), (1, 1, 1)], [5, 32, 1]
    cos, sin = O.rope_table(grids, counts)
    cs = R.rope_cs_table(cos, sin)
    rows, ld = cs.shape[0], heads * 64 + 8
    x = torch.randn(rows, heads * 64, generator=gen(heads)).to(T)
    buf = nan_out(rows, ld, T)
    buf[:rows, :heads * 64] = x.to(DEV)
    cs_d = cs.to(DEV)
    _lib.check(L().ttv_rope_apply_conj(buf.data_ptr(), code(dt), ld, rows, heads, cs_d.data_ptr(), S()), "rope_apply_conj")
    assert untouched(buf, rows, heads * 64)
    ref, mag = R.rope_ref(x, cs, heads, conj=1)
    check(f"rope conj {dt} heads {heads}", buf[:rows, :heads * 64], ref, R.K_ROPE * R.U32 * mag + R.TINY + R.store(ref, dt))
    assert float((ref - R.rope_ref(x, cs, heads, conj=0)[0]).abs().max()) > 0.5          # the direction matters on these rows
    buf[:rows, :heads * 64] = x.to(DEV)
    _lib.check(L().ttv_rope_apply(buf.data_ptr(), code(dt), ld, rows, heads, cs_d.data_ptr(), S()), "rope_apply")
    _lib.check(L().ttv_rope_apply_conj(buf.data_ptr(), code(dt), ld, rows, heads, cs_d.data_ptr(), S()), "rope_apply_conj")
    tol = R.ROPE_ROUNDTRIP_F32 if dt == "f32" else 2 * R.U16 + R.ROPE_ROUNDTRIP_F32
    check(f"rope apply then conj {dt} heads {heads}", buf[:rows, :heads * 64], x.double(), tol * R.pair_norm(x, heads) + R.TINY)


# ---------------------------------------------------------------------------------------------- decoder_embed_tape
@pytest.mark.parametrize("d", R.DEC_EMBED_D)
@pytest.mark.parametrize("C", R.DEC_EMBED_C)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_decoder_embed_tape(dt, C, d):
    """ttv_decoder_embed plus the tape's pre-norm row, through the three inner-product paths of k_dec_embed (C <= 8, C % 4 == 0, other):
    x with hpre requested is x without, bit for bit; hpre is the float64 proj_in(codes) + bias + mask with its two roundings;
    rmsnorm(hpre) * gain reproduces x within the RMSNorm tolerance of tests/test_hip_ops.py."""
    T, c, rows, eps, mask = R.DT[dt], code(dt), 37, 1e-5, 0.3
    g = gen(C * d)
    codes = torch.randn(rows, C, generator=g).to(T)
    w, bias = (torch.randn(d, C, generator=g) * C ** -0.5).to(T), (0.1 * torch.randn(d, generator=g)).to(T)
    gain = 1 + 0.1 * torch.randn(d, generator=g)
    rows_map = torch.randperm(rows + 3, generator=g)[:rows].to(torch.int32)
    dev = [t.to(DEV) for t in (codes, w, bias, torch.tensor([mask]), gain, rows_map)]
    ld = d + 8
    outs = []
    for want_hpre in (False, True):
        x = torch.full((rows + 3, ld), NAN, dtype=T, device=DEV)
        hpre = torch.full((rows + 1, d), NAN, dtype=T, device=DEV)
        _lib.check(L().ttv_decoder_embed_tape(dev[0].data_ptr(), C, dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), dev[4].data_ptr(),
                                              x.data_ptr(), c, ld, dev[5].data_ptr(), rows, d, eps, hpre.data_ptr() if want_hpre else None, S()),
                   "decoder_embed_tape")
        outs.append((x.cpu(), hpre.cpu()))
    (x0, h0), (x1, h1) = outs
    assert bool(torch.isnan(h0).all()) and bool(torch.isnan(h1[rows:]).all())
    assert torch.equal(x0.view(torch.int16 if dt == "bf16" else torch.int32), x1.view(torch.int16 if dt == "bf16" else torch.int32))
    written = torch.zeros(rows + 3, dtype=torch.bool)
    written[rows_map.long()] = True
    assert bool(torch.isnan(x1[~written]).all()) and bool(torch.isnan(x1[:, d:]).all())
    ref, bound = R.dec_embed_hpre_ref(codes, w, bias, mask, dt)
    check(f"decoder_embed_tape {dt} C {C} d {d} hpre", h1[:rows], ref, bound)
    assert_close(x1[rows_map.long(), :d].float(), O.rmsnorm(h1[:rows].float(), gain, eps).float(), dt)


def test_zero_rows_accept_null_pointers():
    bf, f32 = code("bf16"), code("f32")
    rcs = [L().ttv_gate_forward(None, 0, None, 0, None, 0, 0, 64, bf, S()),
           L().ttv_gate_backward(None, 0, None, 0, None, 0, None, 0, None, 0, 0, 64, bf, None, S()),
           L().ttv_geglu_forward(None, 0, None, 0, 0, 96, bf, S()),
           L().ttv_geglu_backward(None, 0, None, 0, None, 0, 0, 96, bf, S()),
           L().ttv_scale_cast(None, 1.0, None, None, bf, 0, S()),
           L().ttv_cast_to_f32(None, bf, None, 0, 1, S()),
           L().ttv_expand_small(None, f32, 0, 5, None, bf, 0, 1, None, bf, 0, 0, 64, S()),
           L().ttv_reduce_small(None, f32, 0, None, None, f32, 0, 5, None, 0, 0, 64, S()),
           L().ttv_rope_apply_conj(None, bf, 0, 0, 4, None, S()),
           L().ttv_decoder_embed_tape(None, 5, None, None, None, None, None, bf, 0, None, 0, 64, 1e-5, None, S())]
    assert rcs == [0] * len(rcs)
