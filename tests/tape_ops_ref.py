"""float64 restatements, error bounds and case lists for the training tape's elementwise and small-projection ops (no GPU needed;
imported by tests/test_hip_tape_ops.py, checked by tests/test_tape_ops_cpu.py).

The ops: ttv_gate_forward / _backward, ttv_geglu_forward / _backward, ttv_scale_cast, ttv_cast_to_f32, ttv_expand_small,
ttv_reduce_small, ttv_const_rows_backward, ttv_rope_apply_conj, ttv_decoder_embed_tape (include/titok_hip.h).

References are the reference model's formulas in float64 (a * sigmoid(gate), transformer.py:103; gelu_erf(gate) * x, transformer.py:47-56;
...), gradients come from torch autograd in float64, never from a hand-derived formula.

Bounds.  For an output with float64 reference r:   |got - r| <= E32 + [bf16 output: half_ulp(r)] + A.
  half_ulp  one round-to-nearest store to bfloat16: half the spacing of bfloat16 at r, 2^(floor(log2 |r|) - 8).  bfloat16 keeps 8
            significant bits, so this runs from 2^-9 |r| at the top of a binade to 2^-8 |r| at its bottom: 2^-9 |r| itself is not a
            bound of the store (132 608 lies midway between 132 096 and 133 120: either neighbour is 512 = 2^-8.05 |r| away;
            tests/test_tape_ops_cpu.py holds bf16_store to both statements).
  A         the approximation term: zero except for the bf16 fast GEGLU gradient (FAST_GELU_ERR, FAST_DGELU_ERR below).
  E32       the fp32 evaluation error  k * 2^-24 * cond + 2^-126 (1 + s): `cond` is the magnitude that one rounding of each
            intermediate is relative to - |r| where the expression has no cancellation, and the sum of the magnitudes of the terms where
            it has one (1 - sigma for a saturated gate, 1 + erf for a negative GEGLU gate, the argument rounding |v| 2^-24 of an
            exp(v) evaluated as exp2(v log2 e)).  Each function below says which.  k is one number per op: derived where the op
            has no library call (sums, rotations), set to about twice the worst figure measured on the MI355X's fp32 path where
            __expf / erff decide (MEASURED lines; profiles/tape_ops_bounds.txt).  2^-126 (1 + s), s the magnitude of the factor the
            transcendental is multiplied by: below the smallest normal number neither format keeps its relative precision, and
            sigma < 2^-126 may be returned as 0.
No bound is taken from a kernel's output and none leaves an element out."""
import math

import numpy as np
import torch

from tests.blockwise import bf16_store

U32 = 2.0 ** -24                 # unit roundoff of fp32
U16 = 2.0 ** -8                  # unit roundoff of bf16: the most one store costs relative to |r| (half_ulp() is the exact figure)
TINY = 2.0 ** -126               # smallest normal of fp32 and bf16
GRID_CAP = 8192 * 256            # work items one pass of a capped elementwise grid covers (ew_blocks() in ttv_bwd.hip)
DT = {"bf16": torch.bfloat16, "f32": torch.float32}

# ---------------------------------------------------------------------------------------------- E32 constants (see the docstring)
# k of E32 per op.  "derived": counted from the kernel's operations.  "measured": 2 x the worst |got - r| / (2^-24 cond) of the fp32
# path over every case of tests/test_hip_tape_ops.py on an MI355X, the figure in the comment (profiles/tape_ops_bounds.txt).
K_GATE = 7.0          # MEASURED 3.36 (dgate; ag 2.67, da 2.64): __expf, 1 + e, the division, the products
K_GEGLU = 7.5         # MEASURED 3.64 (du[:, I:]; du[:, :I] 2.85, h 2.90): erff, __expf, the products
K_ROPE = 3.0          # derived: two products and one sum per output (fewer with contraction)
K_CONST_GAIN = 8.0    # derived: m*m + eps, sqrt, 1/x, two products, the product with colsum, the add into dgain
ROPE_ROUNDTRIP_F32 = 4.0 * U32


def half_ulp(r):
    """Half the spacing of bfloat16 at r (float64): 2^(floor(log2 |r|) - 8), 0 at r = 0."""
    _, e = torch.frexp(r)                      # |r| = m 2^e, m in [0.5, 1)
    return torch.where(r == 0, torch.zeros_like(r), torch.ldexp(torch.ones_like(r), e - 9))


def store(r, dt):
    return half_ulp(r) if dt == "bf16" else torch.zeros_like(r)


def all_finite_bf16(limit=None):
    """Every finite bfloat16 value (65 280 = 255 exponents x 256), or those with |g| <= limit, as a bfloat16 tensor in bit order."""
    bits = np.arange(65536, dtype=np.uint32)
    bits = bits[(bits & 0x7F80) != 0x7F80].astype(np.uint16)
    v = torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16)
    return v if limit is None else v[v.double().abs() <= limit]


# ---------------------------------------------------------------------------------------------- gate
def gate_forward_ref(a, gate):
    return a.double() * torch.sigmoid(gate.double())


def gate_backward_ref(dag, a, gate):
    """(da, dgate) by autograd through gate_forward_ref."""
    a64, g64 = a.double().clone().requires_grad_(True), gate.double().clone().requires_grad_(True)
    gate_forward_ref(a64, g64).backward(dag.double())
    return a64.grad, g64.grad


def _sigma_cond(g):
    """sigma and the magnitude its fp32 error is relative to: sigma (1 + (1 - sigma) |g|) - the roundings of 1 + e and of the division,
    and e = __expf(-g) = exp2(-g log2 e) whose argument rounding costs |g| 2^-24 relative in e, (1 - sigma) of which reaches sigma."""
    s = torch.sigmoid(g)
    return s, s * (1.0 + (1.0 - s) * g.abs())


def gate_forward_bound(a, gate, ref, dt, k=K_GATE):
    a, g = a.double(), gate.double()
    _, c = _sigma_cond(g)
    return k * U32 * a.abs() * c + TINY * (1.0 + a.abs()) + store(ref, dt)


def gate_backward_bounds(dag, a, gate, da_ref, dgate_ref, dt, k=K_GATE):
    """da = dag sigma as the forward.  dgate = dag a sigma (1 - sigma) with 1 - sigma formed as 1.0f - sigma: an absolute error of sigma's
    own, so the error of sigma enters times |1 - 2 sigma| (d/dsigma of sigma (1 - sigma)) beside the relative roundings of the products.
    For gate > 17 sigma rounds to 1 and dgate is exactly 0 where the true value is dag a e^-gate: inside this bound, 2^-25 |dag a|."""
    dag, a, g = dag.double(), a.double(), gate.double()
    s, c = _sigma_cond(g)
    prod = (dag * a).abs()
    e_da = k * U32 * dag.abs() * c + TINY * (1.0 + dag.abs()) + store(da_ref, dt)
    e_dg = k * U32 * prod * (s * (1.0 - s) + (1.0 - 2.0 * s).abs() * c) + TINY * (1.0 + prod) + store(dgate_ref, dt)
    return e_da, e_dg


def delta_ref(da_got, a, dt):
    """delta[r, h] as the kernel defines it: the sum over head h's 64 dims of (da as stored) * a, and the sum of |terms| for its
    bound 64 * 2^-24 * sum |terms| (one fma per term, four additions across the 16 lanes)."""
    da = bf16_store(da_got.double()) if dt == "bf16" else da_got.double()
    t = (da * a.double()).view(a.shape[0], -1, 64)
    return t.sum(-1), 64.0 * U32 * t.abs().sum(-1) + TINY


# ---------------------------------------------------------------------------------------------- GEGLU
RSQRT2 = 0.70710678118654752440


def phi_cdf(g):
    """Phi(g) in float64 without the cancellation of 1 + erf at negative g."""
    return 0.5 * torch.special.erfc(-g * RSQRT2)


def gelu64(g):
    return g * phi_cdf(g)


def geglu_forward_ref(u, I):
    u = u.double()
    return gelu64(u[:, I:2 * I]) * u[:, :I]


def geglu_backward_ref(u, dh, I):
    """du [rows, 2 I] by autograd through geglu_forward_ref."""
    u64 = u.double()[:, :2 * I].clone().requires_grad_(True)
    geglu_forward_ref(u64, I).backward(dh.double())
    return u64.grad


def dgelu64(g):
    """gelu'(g) by autograd (for FAST_DGELU_ERR)."""
    g64 = g.double().clone().requires_grad_(True)
    gelu64(g64).sum().backward()
    return g64.grad


def _gelu_cond(g):
    """What the fp32 errors of gelu = 0.5 g (1 + erff(g / sqrt 2)) and gelu' = 0.5 (1 + erff) + g phi, phi = c __expf(-g^2 / 2), are
    relative to: 0.5 |g| (1 + |erf|) (the sum 1 + erf cancels for g < 0: gelu(-6) is returned as 0) and
    0.5 (1 + |erf|) + |g| phi (1 + g^2 / 2) (the exponent's argument rounding)."""
    erf = torch.erf(g * RSQRT2).abs()
    phi = torch.exp(-0.5 * g * g) / math.sqrt(2.0 * math.pi)
    return 0.5 * g.abs() * (1.0 + erf), 0.5 * (1.0 + erf) + g.abs() * phi * (1.0 + 0.5 * g * g)


def geglu_forward_bound(u, I, ref, dt, k=K_GEGLU):
    u = u.double()
    x, g = u[:, :I], u[:, I:2 * I]
    c, _ = _gelu_cond(g)
    return k * U32 * x.abs() * c + TINY * (1.0 + x.abs()) + store(ref, dt)


def geglu_backward_bound(u, dh, I, ref, dt, fast, k=K_GEGLU):
    """[rows, 2 I] bound of du.  fast: the 8-wide bf16 kernel's approximation term A - FAST_GELU_ERR |dh| and FAST_DGELU_ERR |dh x| plus
    8 * 2^-24 times the same factors for the 1-ulp v_exp_f32 / v_rcp_f32."""
    u, dh = u.double(), dh.double()
    x, g = u[:, :I], u[:, I:2 * I]
    c0, c1 = _gelu_cond(g)
    f0, f1 = dh.abs(), (dh * x).abs()
    e = torch.cat([k * U32 * f0 * c0 + TINY * (1.0 + f0), k * U32 * f1 * c1 + TINY * (1.0 + f1)], 1) + store(ref, dt)
    if fast:
        e = e + torch.cat([(FAST_GELU_ERR + 8.0 * U32) * f0, (FAST_DGELU_ERR + 8.0 * U32) * f1], 1)
    return e


C5_FAST = 1.014262858e-03       # the g^5 coefficient of -log2(e) p(g) in k_geglu_bwd_bf16 / geglu_fast()


def _fma(a, b, c):
    # the product of two fp32 numbers is exact in float64: one rounding to fp32 at the end, as fmaf()
    return (a.astype(np.float64) * b.astype(np.float64) + np.float64(c)).astype(np.float32)


def fast_phi_model(g, c5=C5_FAST):
    """(Phi~, phi) of k_geglu_bwd_bf16 / geglu_fast() (ttv_bwd.hip, ttv_common.h) operation by operation in fp32 on the host: the clamp to
    +-8, the two fmaf() of the polynomial, sigmoid by exp2 and a reciprocal, and the pdf by one exp2.  numpy's exp2 and division are
    correctly rounded where v_exp_f32 / v_rcp_f32 are good to 1 ulp."""
    g = np.asarray(g, dtype=np.float32)
    one = np.float32(1.0)
    with np.errstate(over="ignore", under="ignore"):
        gc = np.clip(g, np.float32(-8.0), np.float32(8.0))
        g2 = gc * gc
        q = _fma(g2, np.float32(c5), np.float32(-1.067757308e-01))
        q = _fma(q, g2, np.float32(-2.301121361e+00))
        cdf = one / (one + np.exp2(q * gc))
        pdf = np.float32(0.39894228040143267794) * np.exp2(np.float32(-0.72134752044448170368) * (g * g))
    return cdf, pdf


def fast_geglu_backward_model(u, dh, I, c5=C5_FAST):
    """du of k_geglu_bwd_bf16 before its bf16 store, in the kernel's order of fp32 operations: d (g Phi~) | (d x) fma(g, phi, Phi~)."""
    u32, d = u.float().numpy(), dh.float().numpy()
    x, g = u32[:, :I], u32[:, I:2 * I]
    cdf, pdf = fast_phi_model(g, c5)
    return torch.from_numpy(np.concatenate([d * (g * cdf), (d * x) * _fma(g, pdf, cdf)], 1))


FAST_DOMAIN = 2.0 ** 20          # |g| beyond which g Phi~ of a clamped negative g (-1.01e-12 |g|) starts to matter


def _fast_errors():
    g = all_finite_bf16(FAST_DOMAIN)
    cdf, pdf = fast_phi_model(g.float().numpy())
    g32 = g.float().numpy()
    g64 = g.double()
    e0 = (torch.from_numpy((g32 * cdf).astype(np.float64)) - gelu64(g64)).abs()
    e1 = (torch.from_numpy(_fma(g32, pdf, cdf).astype(np.float64)) - dgelu64(g64)).abs()
    return float(e0.max()), float(e1.max()), float(g64[e1.argmax()])


FAST_GELU_ERR, FAST_DGELU_ERR, FAST_DGELU_ARGMAX = _fast_errors()


def fast_store_mismatch_limit(n):
    """How many of n bf16 outputs of the fast kernel may differ from bf16(host model): the two differ before the store by at most
    8 * 2^-24 relative (v_exp_f32 / v_rcp_f32), an ulp of bf16 is at least 2^-8 relative, so a rounding boundary falls between them
    with probability <= 2^-13 per element; 4 x that expectation + 16 is far out in the Poisson tail."""
    return 4 * math.ceil(n * 2.0 ** -13) + 16


# ---------------------------------------------------------------------------------------------- small projections
def expand_small_ref(a, w, w_cf, o_dt):
    """out = a @ (w if w_cf else w.T) and its bound C 2^-24 sum |terms| + store (C products and additions in the order of c)."""
    a, w = a.double(), w.double()
    wm = w if w_cf else w.T
    ref = a @ wm
    return ref, a.shape[1] * U32 * (a.abs() @ wm.abs()) + TINY + store(ref, o_dt)


def reduce_small_ref(a, a_rows, w):
    """out = a[a_rows] @ w, fp32 out: (d / 64 + 6) 2^-24 sum |terms| (d / 64 terms per lane, a 6-step wave sum)."""
    a, w = a.double(), w.double()
    if a_rows is not None:
        a = a[a_rows.long()]
    ref = a @ w
    return ref, (a.shape[1] / 64.0 + 6.0) * U32 * (a.abs() @ w.abs()) + TINY


def const_rows_backward_ref(colsum, mask, gain, eps, dgain0, dmask0, dt):
    """dgain, dmask after the op accumulated into (dgain0, dmask0): float64 autograd of v[f] = m rsqrt(m^2 + eps) gain[f] contracted with
    colsum, m = mask (bf16: bf16_store(mask), straight through).  Bounds: K_CONST_GAIN roundings relative to |old| + |increment| for
    dgain; for dmask the d products, d / 256 + 8 additions (strided partial sums, a 6-step wave sum, four waves) and the eight roundings
    of eps rstd^3, relative to sum |terms|, plus the add into the old value."""
    m = torch.tensor(float(mask), dtype=torch.float64)
    if dt == "bf16":
        m = bf16_store(m)
    m = m.clone().requires_grad_(True)
    g = gain.double().clone().requires_grad_(True)
    c = colsum.double()
    ((m * torch.rsqrt(m * m + eps) * g) * c).sum().backward()
    d = g.numel()
    dgain, dmask = dgain0.double() + g.grad, dmask0.double() + m.grad
    e_gain = K_CONST_GAIN * U32 * (dgain0.double().abs() + g.grad.abs()) + TINY
    terms = float((c * g.detach()).abs().sum()) * eps * float(m.detach() ** 2 + eps) ** -1.5
    e_mask = (d / 256.0 + 16.0) * U32 * terms + 2.0 * U32 * (dmask0.double().abs() + m.grad.abs()) + TINY
    return dgain, dmask, e_gain, e_mask


def rope_cs_table(cos, sin):
    """fp32 [L, 64] table of ttv_rope_apply from the oracle's float64 (cos, sin) [L, 30]: cos[32] | sin[32], entries 30, 31 = (1, 0)."""
    L = cos.shape[0]
    cs = torch.zeros(L, 64, dtype=torch.float32)
    cs[:, :30], cs[:, 30:32], cs[:, 32:62] = cos.float(), 1.0, sin.float()
    return cs


def rope_ref(x, cs, heads, conj):
    """float64 rotation of the (re, im) pairs of x [L, heads * 64] by +theta (conj = 0) or -theta (conj = 1) with the fp32 table the kernel
    reads, and the bound K_ROPE 2^-24 (|re c| + |im s|) + store per output."""
    L = x.shape[0]
    p = x.double().view(L, heads, 32, 2)
    c, s = cs.double()[:, None, :32], cs.double()[:, None, 32:] * (-1.0 if conj else 1.0)
    re, im = p[..., 0], p[..., 1]
    out = torch.stack([re * c - im * s, re * s + im * c], -1).view(L, heads * 64)
    mag = torch.stack([(re * c).abs() + (im * s).abs(), (re * s).abs() + (im * c).abs()], -1).view(L, heads * 64)
    return out, mag


def pair_norm(x, heads):
    """|(re, im)| of the pair each element belongs to, same shape as x."""
    p = x.double().view(x.shape[0], heads, 32, 2)
    return p.norm(dim=-1, keepdim=True).expand_as(p).reshape(x.shape)


def dec_embed_hpre_ref(codes, w, bias, mask, dt):
    """The decoder tape's pre-norm row in float64, proj_in(codes) + bias + (T) mask, and its bound: C 2^-24 sum |terms| for the inner
    product, then the two stated roundings to T - of h + bias and of that + mask."""
    c, w64, b = codes.double(), w.double(), bias.double()
    m = bf16_store(torch.tensor(float(mask), dtype=torch.float64)) if dt == "bf16" else torch.tensor(float(np.float32(mask)), dtype=torch.float64)
    h = c @ w64.T + b
    ref = h + m
    u = U16 if dt == "bf16" else U32
    bound = (c.shape[1] + 1) * U32 * (c.abs() @ w64.abs().T + b.abs()) + u * (h.abs() + ref.abs()) * 1.01 + TINY
    return ref, bound


# ---------------------------------------------------------------------------------------------- the one comparison
def worst_ratio(got, ref, bound):
    """max |got - ref| / bound (inf when got is not finite): <= 1 passes."""
    got, ref, bound = got.double().cpu(), ref.double().cpu(), bound.double().cpu()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - ref).abs() / bound).max()) if got.numel() else 0.0


def worst_relative(got, ref):
    """max |got - ref| / |ref| over |ref| >= 1e-30 (report only)."""
    got, ref = got.double().cpu(), ref.double().cpu()
    m = ref.abs() >= 1e-30
    return float(((got - ref).abs()[m] / ref.abs()[m]).max()) if bool(m.any()) else 0.0


# ---------------------------------------------------------------------------------------------- cases
ROWS = (1, 3, 257)
GATE_WIDTHS = (64, 256, 768)
GATE_WIDTH_NO_DELTA = 68
GATE_CAP = {"rows": 32769, "d": 256}                       # 4-wide items: 8192 * 256 + 64
GEGLU_INNER = (96, 704, 1376)
GEGLU_FWD_CAP = {"rows": 6100, "I": 1376}                  # 4-wide items
GEGLU_BWD_CAP = {"rows": 12200, "I": 1376}                 # 8-wide items
SCALE_CAST_N = (4, 1028, 8192 * 1024 + 4)
SCALE_CAST_REFUSED_N = 1030
EXPAND_CAP = {"rows": 8193, "d": 256}
SMALL_C = (5, 32, 64)
SMALL_D = (256, 100)
CONST_ROWS_D = (256, 260, 1024)
CONST_ROWS_MASK = (0.0, 1e-3, 0.7, -3.0)
DEC_EMBED_C = (5, 32, 13)                                  # registers (C <= 8), four per load (C % 4 == 0), scalar loop
DEC_EMBED_D = (256, 768)


def geglu_layout(I, variant="v8"):
    """Leading dimensions and the element offset of dh for a GEGLU case; every ld exceeds its width.  variant: "v8" (the 8-wide bf16 kernel's
    demands met), "lddu" (lddu = 2 I + 4) or "dh_off" (dh starts 4 elements = 8 bytes into its 16-byte aligned buffer)."""
    lay = {"I": I, "ldu": 2 * I + 8, "ldh": I + 8, "lddh": I + 8, "lddu": 2 * I + 8, "dh_off": 0}
    if variant == "lddu":
        lay["lddu"] = 2 * I + 4
    elif variant == "dh_off":
        lay["dh_off"] = 4
    else:
        assert variant == "v8", variant
    return lay


GEGLU_FALLBACK = {"I100": geglu_layout(100), "lddu": geglu_layout(96, "lddu"), "dh_off": geglu_layout(96, "dh_off")}


def geglu_v8(lay, elem_bytes=2, u_addr=0, dh_addr=0, du_addr=0):
    """The predicate of ttvk_geglu_bwd (ttv_bwd.hip) for the 8-wide bf16 kernel, TTV_GEGLU_BWD_ERF unset: addresses are those of the
    buffers (16-byte aligned allocations: 0 stands for any of them), dh_off elements are added to dh's."""
    dh = dh_addr + lay["dh_off"] * elem_bytes
    return (lay["I"] % 8 == 0 and lay["ldu"] % 8 == 0 and lay["lddh"] % 8 == 0 and lay["lddu"] % 8 == 0 and u_addr % 16 == 0
            and dh % 16 == 0 and du_addr % 16 == 0)


def geglu_exhaustive_gates(I=96):
    """Every finite bf16 g with |g| <= 2^20, eight times over (eight different x, dh per g), zero-padded to whole rows of I."""
    g = all_finite_bf16(FAST_DOMAIN).repeat(8)
    rows = -(-g.numel() // I)
    out = torch.zeros(rows * I, dtype=torch.bfloat16)
    out[:g.numel()] = g
    return out.view(rows, I)
