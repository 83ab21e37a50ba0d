"""Float64 replay of one `WeightEMA` update (titok_video_amd/ema.py, `k_opt_ema_update` in csrc/ttv_optim.hip) and a counted bound on
how far the kernel may be from it.  Plain numpy / torch, no GPU.  Used by tests/test_weight_ema_cpu.py (the bound is valid and it
bites) and tests/test_hip_weight_ema.py (the kernel against the replay).

THE REPLAY.  From the stored parameter p (fp32 or bf16, widened exactly) and the stored fp32 shadow s before the update, and the Python
double w = 1 - decay_t the caller formed:  s* = s + w (p - s)  in float64.

THE BOUND, counted from the kernel's rounding steps as tests/adamw_ref.py counts its own, with u = 2^-24 and gamma_n = n u / (1 - n u).
The kernel computes  fl(s + fl(wf fl(p - s)))  with wf = fl(w):
  * wf is the double rounded once: one u;  the difference: one u;  the product: one u.  Together the product the kernel adds is
    w (p - s) (1 + theta_3), |theta_3| <= gamma_3.  A product that underflows adds TINY = 2^-126 absolutely (flushed, or rounded as a
    denormal).
  * the last sum rounds once: relative u on the result, which is within (1 + u) of s* plus the product's error; a result in the
    denormal range is off by at most TINY more.
      |s_kernel - s*| <= u |s*| + (1 + u) gamma_3 w |p - s| + 2 TINY.
The compiler may contract the product and the sum into one fma: that only removes a rounding of the count.  The widening of a bf16
parameter to float is exact.  The shadow is fp32 whatever the parameter's dtype, so there is no second rounding to a storage format."""
import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
CHUNK = 8192          # OPT_CHUNK

# 1 - decay as the caller forms it, in double: the two decays of practice, the decay of the model-level tests, and no memory at all
W_GRID = [1.0 - 0.9999, 1.0 - 0.999, 0.5, 1.0]


def gamma(n):
    return n * U / (1.0 - n * U)


def f64(t):
    """A stored tensor widened exactly."""
    return t.detach().double().cpu().numpy().reshape(-1)


def replay(p, s, w):
    """One update in float64 from stored values (float64 arrays) and the double w."""
    return s + w * (p - s)


def bound(p, s, w):
    """Per-element absolute bound on |kernel - replay|."""
    want = replay(p, s, w)
    return U * np.abs(want) + (1.0 + U) * gamma(3) * w * np.abs(p - s) + 2.0 * TINY


def check(p, s, s_after, w, tag=""):
    """p, s, s_after: float64 arrays of stored values of ONE tensor (s_after what the kernel wrote).  Returns a list of failure
    strings, and the largest error as a fraction of its bound."""
    want, b = replay(p, s, w), bound(p, s, w)
    err = np.abs(s_after - want)
    ok = err <= b
    fails = []
    if not ok.all():
        i = int(np.argmin(ok))
        fails.append(f"{tag} [{i}] of {want.size}: stored {s_after[i]!r} replay {want[i]!r} err {err[i]:.3e} bound {b[i]:.3e} "
                     f"(p {p[i]!r}, s {s[i]!r}, w {w!r}; {int((~ok).sum())} elements outside)")
    return fails, float(np.max(err / b)) if want.size else 0.0


def make_values(n, seed, scale, dtype):
    """CPU tensor of `dtype` with n normal deviates times scale."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g, dtype=torch.float32) * scale).to(dtype)
