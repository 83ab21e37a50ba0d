"""The float64 replay of the optimizer step and its counted bound (tests/adamw_ref.py), without a GPU: a numpy restatement of
`opt_update` and of the clip norm in float32 arithmetic (csrc/ttv_optim.hip, both lerp branches, one rounding per operation - the
kernel's fma contractions only remove some) stays inside the bound on the GPU tests' own inputs and hyper-parameter grid, and each
planted defect leaves it."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adamw_ref as A  # noqa: E402

F = np.float32
DTYPES = [torch.float32, torch.bfloat16]
STEPS = 3


def restated_coef(grads, max_norm):
    """k_opt_gradsq + the head of k_opt_adamw in float32: (coef, norm, n_partials)."""
    partials = []
    for g in grads:
        g32 = g.astype(F)
        for c in range(0, g32.size, A.CHUNK):
            partials.append(np.sum(g32[c:c + A.CHUNK] * g32[c:c + A.CHUNK], dtype=F))
    norm = np.sqrt(np.sum(np.asarray(partials, dtype=F), dtype=F))
    r = F(max_norm) / (norm + F(1e-6))
    return (F(1.0) if r >= F(1.0) else r), norm, len(partials)


def restated_update(p, g, m, v, hyper, t, coef, bf16, variant=None):
    """`opt_update` and the stores in float32 arithmetic on float64 arrays of stored values; returns stored (p', m', v') as float64."""
    lr, (b1, b2), eps, wd = hyper["lr"], hyper["betas"], hyper["eps"], hyper["weight_decay"]
    p, g, m, v = (x.astype(F) for x in (p, g, m, v))
    lr_f, b1_f, b2_f, eps_f, wd_f = F(lr), F(b1), F(b2), F(eps), F(wd)
    om1, om2 = F(1.0 - b1), F(1.0 - b2)
    if variant == "f32_complements":
        om1, om2 = F(1.0) - b1_f, F(1.0) - b2_f
    bc1, bc2s = F(1.0 - b1 ** t), F(math.sqrt(1.0 - b2 ** t))
    if variant == "no_bc2":
        bc2s = F(1.0)
    gk = g if variant == "coef_on_m" else g * F(coef)
    store = (lambda x: A.trunc_bf16(x.astype(np.float64))) if variant == "truncate" else (lambda x: A.rn_bf16(x.astype(np.float64)))
    if not bf16:
        store = lambda x: x.astype(np.float64)          # noqa: E731
    if variant != "wd_after":
        p = p - (lr_f * wd_f) * p
    d = gk - m
    m1 = m + om1 * d if om1 < F(0.5) else gk - d * b1_f
    if variant == "coef_on_m":
        m1 = m1 * F(coef)
    if variant == "v_term_rounded":          # b2 v rounded to bf16 before the sum, the sum rounded again
        v1 = store(b2_f * v).astype(F) + (om2 * gk) * gk
    else:
        v1 = b2_f * v + (om2 * gk) * gk
    if variant == "v_rounded_before_use":          # the update computed from the bf16 v that is stored, not from the fp32 one
        v1 = store(v1).astype(F)
    step_size = lr_f / bc1
    if variant == "eps_in_sqrt":
        denom = np.sqrt(v1 + eps_f) / bc2s
    else:
        denom = np.sqrt(v1) / bc2s + eps_f
    p = p - (step_size * m1) / denom
    if variant == "wd_after":
        p = p - (lr_f * wd_f) * p
    return store(p), store(m1), store(v1)


def run_case(name, dtype, variant=None, stats=None):
    """Three steps over the size list from the restatement's own state; returns the failures of every step."""
    hyper = A.GRID[name]
    bf16 = dtype == torch.bfloat16
    ps = [A.f64(x) for x in A.list_params(dtype)]
    ms = [np.zeros_like(x) for x in ps]
    vs = [np.zeros_like(x) for x in ps]
    stats = stats or A.Stats()
    fails = []
    for step in range(STEPS):
        gs = [A.f64(x) for x in A.list_grads(dtype, step)]
        clipping = hyper["max_norm"] is not None
        coef = coef_k = 1.0
        coef_rel = 0.0
        if clipping:
            coef, norm = A.clip_coef(gs, hyper["max_norm"])
            coef_k, norm_k, n_partials = restated_coef(gs, hyper["max_norm"])
            numel = sum(g.size for g in gs)
            assert n_partials == A.n_chunks(g.size for g in gs)
            assert abs(float(norm_k) - norm) <= A.norm_bound(norm, n_partials, numel)
            coef_rel = A.coef_rel_bound(norm, n_partials, numel)
            assert abs(float(coef_k) - coef) <= coef_rel * coef
        for i in range(len(ps)):
            before = (ps[i], gs[i], ms[i], vs[i])
            after = restated_update(*before, hyper, step + 1, coef_k, bf16, variant)
            fails += A.check_step(before, after, hyper, step + 1, coef, coef_rel, clipping, bf16, stats, f"{name} step {step} tensor {i}")
            ps[i], ms[i], vs[i] = after
    return fails, stats


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", list(A.GRID))
def test_restated_kernel_stays_inside_the_bound(name, dtype):
    fails, stats = run_case(name, dtype)
    stats.report(f"{name}")
    assert not fails, fails[:5]
    assert all(math.isfinite(v) for v in stats.rel_bound.values())


def test_grid_has_every_value_of_the_lists():
    rows = A.GRID.values()
    assert {r["betas"][0] for r in rows} == {0.9, 0.5, 0.0} and {r["betas"][1] for r in rows} == {0.999, 0.96, 0.0}
    assert {r["weight_decay"] for r in rows} == {0.0, 1e-2} and {r["eps"] for r in rows} == {1e-8, 1e-3} and {r["lr"] for r in rows} == {1e-3, 0.0}
    default = [r["max_norm"] for r in rows if r["betas"] == (0.9, 0.999)]
    assert None in default and 1.0 in default and 1e6 in default          # step(), clipping, not clipping
    # the gradients are normal numbers whose squares are too, and one tensor's gradient is all zero
    for dtype in DTYPES:
        gs = A.list_grads(dtype, 0)
        assert all(float(g.double().abs().min()) >= A.G_MIN for g in gs[:-1]) and not gs[-1].any()
        coef, norm = A.clip_coef([A.f64(g) for g in gs], 1.0)
        assert coef < 0.5 and A.clip_coef([A.f64(g) for g in gs], 1e6)[0] == 1.0


# the planted defects: (variant, grid row it is planted in, storage types in which it must leave the bound)
PLANTED = [
    ("f32_complements", "default", DTYPES),
    ("f32_complements", "default_clip", DTYPES),
    ("truncate", "default", [torch.bfloat16]),
    ("v_rounded_before_use", "default", [torch.bfloat16]),
    ("v_term_rounded", "default", [torch.bfloat16]),
    ("no_bc2", "default", DTYPES),
    ("wd_after", "default", [torch.float32]),
    ("coef_on_m", "default_clip", DTYPES),
    ("eps_in_sqrt", "half_096_eps", DTYPES),
]


@pytest.mark.parametrize("variant,name,dtypes", PLANTED, ids=[f"{v}-{n}" for v, n, _ in PLANTED])
def test_planted_defect_leaves_the_bound(variant, name, dtypes):
    for dtype in dtypes:
        fails, _ = run_case(name, dtype, variant)
        print(variant, name, dtype, len(fails), fails[:1])
        assert fails, (variant, name, dtype)
        if variant == "f32_complements":
            assert any(" v[" in f for f in fails), "the float32 complements show on exp_avg_sq"


def test_rn_bf16_is_torchs_cast_ties_included():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(20000, generator=g) * torch.exp(torch.randn(20000, generator=g) * 5)          # far from bf16's overflow
    bits = torch.randint(0, 0x7F00, (20000,), generator=g, dtype=torch.int32)
    ties = ((bits << 16) | 0x8000).view(torch.float32)          # exactly half way between two bf16 values, odd and even below
    near = ((bits << 16) | 0x7FFF).view(torch.float32)
    tiny = torch.tensor([0.0, -0.0, 2.0 ** -126, 2.0 ** -133, 2.0 ** -134, 3 * 2.0 ** -134, 2.0 ** -135, -(2.0 ** -127 + 2.0 ** -134), 1.0, -1.5])
    for t in (x, ties, -ties, near, tiny):
        want = t.to(torch.bfloat16).double().numpy()
        got = A.rn_bf16(t.double().numpy())
        assert np.array_equal(got, want)
        assert np.array_equal(np.signbit(got), np.signbit(want))
    assert np.array_equal(A.trunc_bf16(ties.double().numpy()), (bits << 16).view(torch.float32).double().numpy())


@pytest.mark.parametrize("max_norm", [1.0, 1e6])
def test_clip_coef_is_clip_grad_norm(max_norm):
    params = [torch.nn.Parameter(torch.zeros(n, dtype=torch.float64)) for n in (1, 7, 8193)]
    grads = [A.make_grad(n, 40 + i, 0.05, torch.float32).double() for i, n in enumerate((1, 7, 8193))]
    for p, g in zip(params, grads):
        p.grad = g.clone()
    norm_ref = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    coef, norm = A.clip_coef([g.numpy() for g in grads], max_norm)
    assert norm == pytest.approx(norm_ref, rel=1e-14)
    for p, g in zip(params, grads):
        assert np.allclose(p.grad.numpy(), g.numpy() * coef, rtol=1e-14, atol=0.0)
    assert (coef == 1.0) == (max_norm == 1e6)
