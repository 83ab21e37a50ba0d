"""float64 torch restatement of `ttv_disc_head` (include/titok_hip.h) with the rounding bound of every output.  Not a test module:
tests/test_hip_disc_head.py and tests/test_hip_disc_fused.py import it.

THE BOUND, counted from the kernel's rounding steps with u = 2^-24 (half an ulp, relative), nothing tuned to what the kernel gives:
  * a logit is the sum of R = 4 fp32 values (3 roundings) divided by R (1): |error| <= delta = 4 u max|per-token value|.  bf16 inputs
    in these tests are multiples of 2^-6 below 64, whose sum is exact in fp32 and whose mean then rounds to bf16 exactly as the
    float64 mean does: delta = 0.  A difference x of two logits (m, real - noisy real, real + fake) carries a(x) = 2 delta + u |x|.
  * per clip: softplus is 1-Lipschitz and costs expf, an addition inside log1pf and log1pf itself, at most 6 ulp = 12 u of its value
    (OpenCL bounds: exp 3 ulp damped by z / ((1 + z) log1p(z)) <= 1, log1p 2 ulp): t = a(m) + 12 u f.  logits_relative: a(m).
    A square x^2 (and 0.5 x^2): 2 |x| a(x) + 4 u x^2.
  * a mean over n clips: at most ceil(n / 256) - 1 adds in a thread, 6 in the wave, 3 across waves, 1 division: <= 12 u mean|f| for
    n <= 512 (the tests stay below 268 terms).  total = d + w_gp (r1 + r2) + w_c c: the terms' bounds, weighted, + 4 u of the sum of
    the weighted magnitudes.
  * gradient per token, before the cast to the input dtype: the softplus derivative z / (z + 1) is 1/4-Lipschitz and costs 8 u of its
    value; 2 w_gp x costs 2 w_gp a(x) + 3 u of its value; w_c x costs w_c a(x) + 2 u; their sum and the scaling by 1 / (n R) at most
    4 roundings of the summed magnitudes (12 u in all, with the 8 above); then, for bf16 inputs, one rounding to bf16 (8 significant bits: half an ulp is at most 2^-8 relative).
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -24
TERMS = ("total", "loss", "logits_relative", "r1_penalty", "r2_penalty", "centering_loss")      # the kernel's terms[0 .. 5]


def head_ref(per_token, mode, n, R, gp_scale, centering_weight, dtype):
    """per_token: CPU tensor of G n R values (any shape) holding the values the kernel reads.  Returns (terms, tol, grad, grad_tol):
    dicts of float64 scalars keyed by TERMS, and float64 tensors shaped like per_token."""
    x = per_token.detach().double().reshape(-1, n, R).clone().requires_grad_(True)
    G = x.shape[0]
    exact = x.mean(-1)
    logit = exact + (exact.detach().to(dtype).double() - exact.detach())          # rounded once to the input dtype, straight through
    delta = 0.0 if dtype == torch.bfloat16 else 4 * U * float(x.detach().abs().max())
    a = lambda v: 2 * delta + U * v.detach().abs()
    sr, sf = logit[0], logit[1]
    m = sr - sf
    out, tol = {}, {}
    mean_tol = lambda t, f: float(t.mean() + 12 * U * f.detach().abs().mean())
    comp = torch.zeros_like(x)                                                     # summed magnitudes of a token's gradient components
    lips = torch.zeros_like(x)                                                     # their sensitivity to the logits' errors
    if mode == "generator":
        f = F.softplus(m)
        out["loss"], tol["loss"] = f.mean(), mean_tol(a(m) + 12 * U * f.detach(), f)
        out["total"], tol["total"] = out["loss"], tol["loss"]
        sig = torch.sigmoid(m.detach())
        comp[0] += sig[:, None]; comp[1] += sig[:, None]
        lips[0] += 0.25 * a(m)[:, None]; lips[1] += 0.25 * a(m)[:, None]
    else:
        f = F.softplus(-m)
        out["loss"], tol["loss"] = f.mean(), mean_tol(a(m) + 12 * U * f.detach(), f)
        out["logits_relative"], tol["logits_relative"] = m.mean(), mean_tol(a(m), m)
        total, total_tol, mags = out["loss"], tol["loss"], float(f.detach().mean())
        sig = torch.sigmoid(-m.detach())
        comp[0] += sig[:, None]; comp[1] += sig[:, None]
        lips[0] += 0.25 * a(m)[:, None]; lips[1] += 0.25 * a(m)[:, None]
        if G == 4:
            for k, (name, clean) in enumerate((("r1_penalty", sr), ("r2_penalty", sf))):
                d = clean - logit[2 + k]
                sq = d.square()
                out[name], tol[name] = sq.mean(), mean_tol(2 * d.detach().abs() * a(d) + 4 * U * sq.detach(), sq)
                total, total_tol, mags = total + gp_scale * out[name], total_tol + gp_scale * tol[name], mags + gp_scale * float(sq.detach().mean())
                for g in (k, 2 + k):
                    comp[g] += (2 * gp_scale * d.detach().abs())[:, None]
                    lips[g] += (2 * gp_scale * a(d))[:, None]
        if centering_weight > 0.0:
            sc = sr + sf
            cen = 0.5 * sc.square()
            out["centering_loss"], tol["centering_loss"] = cen.mean(), mean_tol(2 * sc.detach().abs() * a(sc) + 4 * U * cen.detach(), cen)
            total, total_tol, mags = total + centering_weight * out["centering_loss"], total_tol + centering_weight * tol["centering_loss"], \
                mags + centering_weight * float(cen.detach().mean())
            for g in (0, 1):
                comp[g] += (centering_weight * sc.detach().abs())[:, None]
                lips[g] += (centering_weight * a(sc))[:, None]
        out["total"], tol["total"] = total, total_tol + 4 * U * mags
    (grad,) = torch.autograd.grad(out["total"], x)
    grad_tol = (lips + 12 * U * comp) / (n * R)
    if dtype == torch.bfloat16:
        grad_tol = grad_tol + 2.0 ** -8 * (grad.abs() + grad_tol)
    shape = per_token.shape
    return {k: float(v.detach()) for k, v in out.items()}, tol, grad.reshape(shape), grad_tol.reshape(shape) + 1e-30


def head_inputs(G, n, R, dtype, seed):
    """Per-token values [G, n, R] on the CPU in `dtype`: logits of a few units with real - fake beyond +-20 on both sides in two clips
    (when there are that many), equal real and fake logits in one, and the noisy groups close to the clean ones.  bf16: multiples of
    2^-6 below 64 (see the bound)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((G, n, R), generator=g, dtype=torch.float64) * 2.0
    x[0, 0] += 15.0; x[1, 0] -= 15.0                                   # m ~ +30: softplus(-m) tiny, softplus(m) linear
    if n > 1:
        x[0, 1] -= 14.0; x[1, 1] += 14.0                               # m ~ -28
    if n > 2:
        x[1, 2] = x[0, 2]                                              # equal logits
    if G == 4:
        x[2:] = x[:2] + 0.05 * torch.randn((2, n, R), generator=g, dtype=torch.float64)
    if dtype == torch.bfloat16:
        x = (x * 64).round() / 64
    x = x.to(dtype)
    if dtype == torch.bfloat16:
        assert float(x.abs().max()) < 64 and bool(((x.double() * 64) % 1 == 0).all())
    return x
