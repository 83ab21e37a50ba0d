"""Float64 replay of one `HipAdamW` step (titok_video_amd/optim.py, `k_opt_gradsq` / `k_opt_adamw` in csrc/ttv_optim.hip) and a counted
bound on how far the kernels may be from it.  Plain numpy / torch, no GPU.  Used by tests/test_adamw_ref_cpu.py (the bound is valid and
it bites) and tests/test_hip_adamw_f64.py (the kernels against the replay).

THE REPLAY.  From the stored p, g, m, v before the step (fp32 or bf16 numbers, widened exactly) and the Python doubles the caller gave:
  ge = coef g ;  p1 = p - lr wd p ;  m' = m + (1 - b1)(ge - m) ;  v' = b2 v + (1 - b2) ge^2 ;
  p' = p1 - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps) ,  bc1 = 1 - b1^t , bc2 = 1 - b2^t ,
with coef = min(1, max_norm / (norm + 1e-6)) over the float64 norm of ALL gradients of the step (1 without clipping).

THE BOUND, counted from the rounding steps of `opt_update` with u = 2^-24 and gamma_n = n u / (1 - n u).  A float handed to the kernel
(lr, wd, eps, beta1, beta2, 1 - beta1, 1 - beta2, bc1, sqrt(bc2), max_norm) is a double rounded once: one u each.  sqrtf and the two
divisions are counted at 1 ulp = 2 u, as tests/test_hip_grad_norms.py counts sqrtf.  The compiler may contract a product and a sum into
one fma: that only removes a rounding of the count.  Every product that can underflow adds TINY = 2^-126 absolutely (flushed or rounded
as a denormal).  Errors are carried per element; |.| of exact quantities below.
  * gradient: the kernel's ge is g coef_k (1 + d), coef_k within Ec (relative) of coef: Eg = Ec + u + Ec u relative; without
    clipping coef_k is 1.0f and the product exact: Eg = 0.
  * decay  p1 = fl(p - fl(fl(lr wd) p)): lr, wd, their product, the product with p: 4 roundings on lr wd |p|, one on the difference:
      E_p1 = u |p1| + gamma_5 lr wd |p| + 2 TINY.
  * first moment, 1 - b1 < 0.5:  fl(m + fl(w fl(ge - m))): the difference, w, the product:
      T = (1 - b1) (|ge - m| gamma_3 + |ge| Eg (1 + gamma_3)) ;
    1 - b1 >= 0.5:  fl(ge - fl(fl(ge - m) b1)): the same three on the product, and ge itself once more:
      T = b1 (|ge - m| gamma_3 + |ge| Eg (1 + gamma_3)) + |ge| Eg ;
    then the last sum:  E_m = u |m'| + (1 + u) T + 2 TINY.  It scales with |m| + |ge|.
  * second moment  fl(fl(b2 v) + fl(fl(w2 ge) ge)): b2 and its product: 2; w2 and two products: 3; ge^2 carries (1 + Eg)^2:
      E_v = u v' + (1 + u) (gamma_2 b2 v + (1 - b2) ge^2 ((1 + gamma_3)(1 + Eg)^2 - 1)) + 3 TINY.  It scales with v + ge^2.
  * the quotient, S = sqrt(v'), Dn = S / sqrt(bc2) + eps, N = (lr / bc1) m', Uo = N / Dn (the update):
      E_S  = min(E_v / S, sqrt(E_v)) (1 + 2 u) + 2 u S                 (|sqrt a - sqrt b| <= |a - b| / sqrt b and <= sqrt |a - b|)
      E_Q  = (E_S (1 + gamma_3) + gamma_3 S) / sqrt(bc2)                (sqrt(bc2) once, the division twice)
      E_Dn = E_Q + u eps + u (Dn + E_Q + u eps) + TINY                  (eps once, the sum once)
      E_N  = (lr / bc1) (E_m (1 + gamma_5) + gamma_5 |m'|) + TINY       (lr, bc1, their division twice, the product with m')
      E_U  = (E_N + |Uo| E_Dn) / (Dn - E_Dn) (1 + gamma_2) + gamma_2 |Uo| + TINY      (n_k / d_k - N / Dn = ((n_k - N) Dn - N (d_k - Dn)) / (d_k Dn))
      E_p  = E_p1 + E_U + u (|p'| + E_p1 + E_U).   It scales with |p| + |Uo|; where Dn <= E_Dn there is no bound (infinity).
  * the clip factor.  A partial of k_opt_gradsq is within gamma_40 of its chunk's sum of squares (tests/test_hip_grad_norms.py: D = 40).
    k_opt_adamw adds the partials with a stride of 256, ceil(n_partials / 256) additions per thread, then the block sum, 8 levels:
    gamma_(40 + passes + 8) on the sum of squares, all terms >= 0; sqrtf halves it and rounds: gamma_n / 2 + 3 u on the norm, plus
    sqrt(numel) 2^-63 absolutely for squares below 2^-126.  max_norm / (norm + 1e-6f): max_norm, 1e-6f, the sum, the division at
    2 u: Ec = (En + gamma_5) / (1 - En - gamma_5), En the norm's relative bound.  The clamp at 1 does not widen it.
For fp32 tensors the stored value is the computed one.  For bf16 tensors the kernel computes in fp32 and rounds once, to nearest-even:
the stored value lies between RN_bf16(replay - b) and RN_bf16(replay + b), b the fp32 bound above - it IS RN_bf16(replay) except where
the replay sits within b of a rounding midpoint (`accept`).  bf16 values of the tests stay normal numbers and far from overflow."""
import math

import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
CHUNK = 8192          # OPT_CHUNK
D_CHUNK = 40          # roundings a square passes through inside k_opt_gradsq (tests/test_hip_grad_norms.py)
G_MIN = 2.0 ** -40    # gradients stay normal numbers: g^2 >= 2^-80
SIZES = [1, 7, 8, 9, 2047, 2049, 8191, 8192, 8193, 8192 + 2048 + 3, 20000]
ZERO_GRAD_SIZE = 2049          # one more tensor of the list, whose gradient is all zero

# the hyper-parameter grid on SIZES: every value of the issue's lists appears (with fp32 and with bf16: the tests run each row in both)
GRID = {
    "default":       dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=None),
    "default_clip":  dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=1.0),
    "default_open":  dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=1e6),
    "half_096_eps":  dict(lr=1e-3, betas=(0.5, 0.96), eps=1e-3, weight_decay=0.0, max_norm=1e6),
    "zero_betas":    dict(lr=1e-3, betas=(0.0, 0.0), eps=1e-8, weight_decay=1e-2, max_norm=None),
    "lr0_clip":      dict(lr=0.0, betas=(0.9, 0.96), eps=1e-3, weight_decay=1e-2, max_norm=1.0),
    "half_0999":     dict(lr=1e-3, betas=(0.5, 0.999), eps=1e-8, weight_decay=0.0, max_norm=None),
    "b1zero_clip":   dict(lr=1e-3, betas=(0.0, 0.96), eps=1e-3, weight_decay=1e-2, max_norm=1.0),
    "b2zero_clip":   dict(lr=1e-3, betas=(0.9, 0.0), eps=1e-8, weight_decay=0.0, max_norm=1.0),
}
GRAD_SCALE = 0.05          # norm over SIZES ~ 12: max_norm = 1 clips, 1e6 does not


def gamma(n):
    return n * U / (1.0 - n * U)


# ------------------------------------------------------------------------------------------------------------------ inputs
def make_values(n, seed, scale, dtype):
    """CPU tensor of `dtype` with n normal deviates times scale."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g, dtype=torch.float32) * scale).to(dtype)


def make_grad(n, seed, scale, dtype):
    """As make_values, magnitudes held at or above 2^-40 so that g^2 is a normal fp32 number."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g, dtype=torch.float32) * scale
    x = torch.where(x.abs() < G_MIN, torch.copysign(torch.full_like(x, G_MIN), x), x)
    return x.to(dtype)


def list_params(dtype, seed=0):
    """The parameters of the size list (and the one whose gradient is zero)."""
    return [make_values(n, 100 * seed + i, 0.5, dtype) for i, n in enumerate(SIZES + [ZERO_GRAD_SIZE])]


def list_grads(dtype, step, seed=0):
    gs = [make_grad(n, 7000 + 1000 * step + 100 * seed + i, GRAD_SCALE * (step + 1), dtype) for i, n in enumerate(SIZES)]
    return gs + [torch.zeros(ZERO_GRAD_SIZE, dtype=dtype)]


def f64(t):
    """A stored tensor widened exactly."""
    return t.detach().double().cpu().numpy().reshape(-1)


# ------------------------------------------------------------------------------------------------------------------ bf16
def _quantum(x):
    _, e = np.frexp(x)
    return np.ldexp(1.0, np.maximum(e - 8, -133))


def rn_bf16(x):
    """float64 -> the nearest bf16 value (ties to even), as float64.  Denormals included; no overflow handling."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        q = _quantum(np.where(np.isfinite(x), x, 0.0))
        return np.where(np.isfinite(x), np.rint(x / q) * q, x)


def trunc_bf16(x):
    """float64 -> bf16 by dropping bits (toward zero): the planted wrong cast."""
    x = np.asarray(x, dtype=np.float64)
    q = _quantum(x)
    return np.trunc(x / q) * q


def accept(stored, replay, bound, bf16):
    """Per element: is the stored value one the kernel may have written?"""
    if not bf16:
        return np.abs(stored - replay) <= bound
    return (rn_bf16(replay - bound) <= stored) & (stored <= rn_bf16(replay + bound))


# ------------------------------------------------------------------------------------------------------------------ the replay
def replay_step(p, g, m, v, hyper, t, coef=1.0):
    """One step in float64 from stored values; returns (p', m', v')."""
    lr, (b1, b2), eps, wd = hyper["lr"], hyper["betas"], hyper["eps"], hyper["weight_decay"]
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    ge = g * coef
    p1 = p - lr * wd * p
    m1 = m + (1.0 - b1) * (ge - m)
    v1 = b2 * v + (1.0 - b2) * ge * ge
    p2 = p1 - (lr / bc1) * m1 / (np.sqrt(v1) / math.sqrt(bc2) + eps)
    return p2, m1, v1


def grad_norm(grads):
    return math.sqrt(sum(float(np.sum(np.square(np.asarray(g, dtype=np.float64)))) for g in grads))


def clip_coef(grads, max_norm):
    """(coef, norm): the float64 norm over all given gradients and min(1, max_norm / (norm + 1e-6))."""
    norm = grad_norm(grads)
    return min(1.0, max_norm / (norm + 1e-6)), norm


def n_chunks(numels):
    return sum(-(-n // CHUNK) for n in numels)


def norm_bound(norm, n_partials, numel):
    """Absolute bound on |out_norm - norm| for the norm k_opt_adamw forms from n_partials partials."""
    passes = -(-n_partials // 256)
    return (gamma(D_CHUNK + passes + 8) / 2.0 + 3.0 * U) * norm + math.sqrt(numel) * 2.0 ** -63


def coef_rel_bound(norm, n_partials, numel):
    """Relative bound Ec on the kernel's clip factor."""
    en = norm_bound(norm, n_partials, numel) / norm if norm > 0 else 0.0
    x = en + gamma(5)
    return x / (1.0 - x)


def bounds(p, g, m, v, hyper, t, coef=1.0, coef_rel=0.0, clipping=False):
    """Per-element absolute bounds (bp, bm, bv) on |kernel - replay| in fp32, and the scales (sp, sm, sv) they are relative to:
    |p| + |update|, |m| + |ge|, v + ge^2."""
    lr, (b1, b2), eps, wd = hyper["lr"], hyper["betas"], hyper["eps"], hyper["weight_decay"]
    bc1, bc2s = 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t)
    g2, g3, g5 = gamma(2), gamma(3), gamma(5)
    eg = coef_rel + U + coef_rel * U if clipping else 0.0
    ge = g * coef
    age = np.abs(ge)
    # decay
    p1 = p - lr * wd * p
    e_p1 = U * np.abs(p1) + g5 * lr * wd * np.abs(p) + 2 * TINY
    # first moment
    inner = np.abs(ge - m) * g3 + age * eg * (1.0 + g3)
    if float(np.float32(1.0 - b1)) < 0.5:
        tm = (1.0 - b1) * inner
    else:
        tm = b1 * inner + age * eg
    m1 = m + (1.0 - b1) * (ge - m)
    e_m = U * np.abs(m1) + (1.0 + U) * tm + 2 * TINY
    # second moment
    v1 = b2 * v + (1.0 - b2) * ge * ge
    e_v = U * v1 + (1.0 + U) * (g2 * b2 * v + (1.0 - b2) * ge * ge * ((1.0 + g3) * (1.0 + eg) ** 2 - 1.0)) + 3 * TINY
    # quotient
    s = np.sqrt(v1)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_s0 = np.where(s > 0, np.minimum(e_v / np.where(s > 0, s, 1.0), np.sqrt(e_v)), np.sqrt(e_v))
    e_s = e_s0 * (1.0 + 2 * U) + 2 * U * s
    e_q = (e_s * (1.0 + g3) + g3 * s) / bc2s
    dn = s / bc2s + eps
    e_dn = e_q + U * eps + U * (dn + e_q + U * eps) + TINY
    n = (lr / bc1) * m1
    e_n = (lr / bc1) * (e_m * (1.0 + g5) + g5 * np.abs(m1)) + TINY
    uo = n / dn
    safe = dn > e_dn
    e_u = (e_n + np.abs(uo) * e_dn) / np.where(safe, dn - e_dn, 1.0) * (1.0 + g2) + g2 * np.abs(uo) + TINY
    p2 = p1 - uo
    e_p = e_p1 + e_u + U * (np.abs(p2) + e_p1 + e_u)
    e_p = np.where(safe, e_p, np.inf)
    return (e_p, e_m, e_v), (np.abs(p) + np.abs(uo), np.abs(m) + age, v + ge * ge)


class Stats:
    """Largest relative bound and largest observed error (in the same unit, and as a fraction of the bound) per quantity."""

    def __init__(self):
        self.rel_bound = {}
        self.rel_err = {}
        self.frac = {}
        self.off_rn = {}          # bf16: elements whose stored value is not RN_bf16(replay) (all within the bound)
        self.elements = 0

    def add(self, key, bound, scale, err):
        ok = np.isfinite(bound) & (scale > 0)
        if not ok.any():
            return
        self.rel_bound[key] = max(self.rel_bound.get(key, 0.0), float(np.max(bound[ok] / scale[ok])))
        self.rel_err[key] = max(self.rel_err.get(key, 0.0), float(np.max(err[ok] / scale[ok])))
        self.frac[key] = max(self.frac.get(key, 0.0), float(np.max(err[ok] / bound[ok])))

    def report(self, tag):
        for k in sorted(self.rel_bound):
            print(f"{tag} {k}: largest relative bound {self.rel_bound[k]:.3e}, largest observed error {self.rel_err[k]:.3e} "
                  f"({self.frac[k]:.3f} of its bound)" + (f", {self.off_rn[k]} stored values off RN_bf16(replay)" if k in self.off_rn else ""))


def check_step(before, after, hyper, t, coef, coef_rel, clipping, bf16, stats, tag):
    """before = (p, g, m, v), after = (p, m, v): float64 arrays of stored values of ONE tensor.  Returns a list of failure strings."""
    want = replay_step(*before, hyper, t, coef)
    (bs, scales) = bounds(*before, hyper, t, coef, coef_rel, clipping)
    fails = []
    kind = "bf16" if bf16 else "fp32"
    for name, got, w, b, sc in zip("pmv", after, want, bs, scales):
        ok = accept(got, w, b, bf16)
        if not bf16:
            stats.add(f"{kind} {name}", b, sc, np.abs(got - w))
        else:
            stats.add(f"{kind} {name} (fp32 bound)", b, sc, np.zeros_like(w))
            k = f"{kind} {name} (fp32 bound)"
            stats.off_rn[k] = stats.off_rn.get(k, 0) + int(np.sum(got != rn_bf16(w)))
        if not ok.all():
            i = int(np.argmin(ok))
            fails.append(f"{tag} {name}[{i}] of {got.size}: stored {got[i]!r} replay {w[i]!r} err {abs(got[i] - w[i]):.3e} bound {b[i]:.3e} "
                         f"({int((~ok).sum())} elements outside)")
    stats.elements += before[0].size
    return fails
