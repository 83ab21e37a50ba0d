"""`HipAdamW` (titok_video_amd/optim.py; `k_opt_gradsq` / `k_opt_adamw`, csrc/ttv_optim.hip) on the MI355X against a float64 replay of
every step, inside the bound counted in tests/adamw_ref.py.  `-m gpu`.

Every step: clone p, g, m, v on the device, step, compare the stored p, m, v with the replay of the clones inside the bound, and go on
from the kernel's own state (bounds do not compound).  fp32 tensors: |stored - replay| <= bound per element.  bf16 tensors: the stored
value lies between RN_bf16(replay - bound) and RN_bf16(replay + bound).  The largest relative bounds and observed errors are printed
per test (`-s`).  With 1 - beta taken from float32 betas (the kernel before its complements came from the host in double) the
beta2 = 0.999 rows fail on exp_avg_sq: 1.3e-5 relative against a bound of 1.8e-7."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adamw_ref as A  # noqa: E402

from titok_video_amd.optim import HipAdamW  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]


def bits(t):
    return t.detach().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def step_value(st):
    s = st["step"]
    return float(s.item()) if torch.is_tensor(s) else float(s)


def take_step(opt, max_norm=None):
    """Clone what the step will read, step, clone what it wrote.  No host synchronisation (the step counts live on the host).
    Returns the record `verify` replays."""
    rec = {"max_norm": max_norm, "tensors": []}
    for gi, group in enumerate(opt.param_groups):
        hyper = {k: group[k] for k in ("lr", "betas", "eps", "weight_decay")}
        for pi, p in enumerate(group["params"]):
            if p.grad is None:
                continue
            st = opt.state.get(p)
            if st:
                t = step_value(st) + 1.0
                m, v = st["exp_avg"].to(DEV, p.dtype).clone(), st["exp_avg_sq"].to(DEV, p.dtype).clone()      # a loaded state is converted first
            else:
                t, m, v = 1.0, torch.zeros_like(p), torch.zeros_like(p)
            rec["tensors"].append({"tag": f"group {gi} param {pi}", "p": p, "hyper": hyper, "t": t,
                                   "before": (p.detach().clone(), p.grad.clone(), m, v)})
    rec["norm"] = opt.step() if max_norm is None else opt.clip_and_step(max_norm)
    for e in rec["tensors"]:
        st = opt.state[e["p"]]
        assert step_value(st) == e["t"] and st["exp_avg"].dtype == e["p"].dtype and st["exp_avg_sq"].dtype == e["p"].dtype
        e["after"] = (e["p"].detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone())
    return rec


def verify(rec, stats, tag=""):
    clipping = rec["max_norm"] is not None
    coef, coef_rel = 1.0, 0.0
    if clipping:
        grads = [A.f64(e["before"][1]) for e in rec["tensors"]]
        coef, norm = A.clip_coef(grads, rec["max_norm"])
        n_partials, numel = A.n_chunks(g.size for g in grads), sum(g.size for g in grads)
        nb = A.norm_bound(norm, n_partials, numel)
        got = float(rec["norm"])
        print(f"{tag} norm: got {got!r} want {norm!r} err {abs(got - norm):.3e} bound {nb:.3e} (relative {nb / norm if norm else 0.0:.3e}), "
              f"{n_partials} partials, coef {coef:.6e}")
        assert rec["norm"].is_cuda and abs(got - norm) <= nb, (tag, got, norm, nb)
        stats.rel_bound["norm"] = max(stats.rel_bound.get("norm", 0.0), nb / norm if norm else 0.0)
        stats.rel_err["norm"] = max(stats.rel_err.get("norm", 0.0), abs(got - norm) / norm if norm else 0.0)
        stats.frac["norm"] = max(stats.frac.get("norm", 0.0), abs(got - norm) / nb)
        coef_rel = A.coef_rel_bound(norm, n_partials, numel)
    else:
        assert rec["norm"] is None
    fails = []
    for e in rec["tensors"]:
        bf16 = e["p"].dtype == torch.bfloat16
        before, after = tuple(A.f64(x) for x in e["before"]), tuple(A.f64(x) for x in e["after"])
        fails += A.check_step(before, after, e["hyper"], e["t"], coef, coef_rel, clipping, bf16, stats, f"{tag} {e['tag']}")
        if e["hyper"]["lr"] == 0.0:
            assert torch.equal(bits(e["after"][0]), bits(e["before"][0])), "lr = 0 leaves the parameters bit-unchanged"
            if before[1].any():
                assert not np.array_equal(after[1], before[2]) and not np.array_equal(after[2], before[3]), "lr = 0: m and v still move"
    assert not fails, fails[:5]


def list_case(dtype, hyper):
    params = [torch.nn.Parameter(x.to(DEV)) for x in A.list_params(dtype)]
    opt = HipAdamW(params, **{k: v for k, v in hyper.items() if k != "max_norm"})
    return params, opt


# ------------------------------------------------------------------------------------------------ sizes and hyper-parameters
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(A.GRID))
def test_size_list_over_the_hyper_parameter_grid(name, dtype):
    """Eleven sizes on and around the 8-element vector, the 2048-element pass and the 8192-element chunk, and one all-zero gradient; three
    steps; step(), clip_and_step clipping and not clipping at torch's default betas, the other rows of the grid once each."""
    hyper = A.GRID[name]
    params, opt = list_case(dtype, hyper)
    stats = A.Stats()
    for step in range(3):
        for p, g in zip(params, A.list_grads(dtype, step)):
            p.grad = g.to(DEV)
        verify(take_step(opt, hyper["max_norm"]), stats, f"{name} step {step}")
    stats.report(name)
    assert stats.elements == 3 * (sum(A.SIZES) + A.ZERO_GRAD_SIZE)
    zero = opt.state[params[-1]]
    assert not zero["exp_avg"].any() and not zero["exp_avg_sq"].any()


# ------------------------------------------------------------------------------------------------ off the 16-byte grid
VIEW_SIZES = [9, 8193, 20000]
PAD = 24
MISALIGNED = [(torch.float32, w, 1) for w in ("p", "g", "m", "v", "pgmv")] + \
             [(torch.bfloat16, w, o) for o in (1, 4) for w in ("p", "g", "m", "v", "pgmv")] + [(torch.bfloat16, "pgmv", 8)]


@pytest.mark.parametrize("dtype,which,offset", MISALIGNED, ids=[f"{'fp32' if d == torch.float32 else 'bf16'}-{w}-{o}" for d, w, o in MISALIGNED])
def test_views_off_the_16_byte_grid(dtype, which, offset):
    """Parameter, gradient and preloaded exp_avg / exp_avg_sq as contiguous views at an element offset into larger buffers: the
    element-wise loops of both kernels (offset 8 in bf16 is aligned: the vector path from a shifted start).  What lies outside the
    views in the backing buffers keeps its bits."""
    hyper = A.GRID["default_clip"]
    item = 4 if dtype == torch.float32 else 2
    backing, views = [], []
    for i, n in enumerate(VIEW_SIZES):
        row = {}
        for j, k in enumerate("pgmv"):
            buf = A.make_values(n + 2 * PAD, 500 + 10 * i + j, 0.5 if k == "p" else 0.05, dtype)
            if k == "v":
                buf = (buf.float() ** 2).to(dtype)
            buf = buf.to(DEV)
            off = offset if k in which else 0
            view = buf[off:off + n]
            assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + off * item and buf.data_ptr() % 16 == 0
            assert (view.data_ptr() % 16 != 0) == (k in which and offset * item % 16 != 0)
            backing.append((buf, buf.clone(), off, n))
            row[k] = view
        views.append(row)
    params = [torch.nn.Parameter(r["p"]) for r in views]
    opt = HipAdamW(params, **{k: v for k, v in hyper.items() if k != "max_norm"})
    for p, r in zip(params, views):
        assert p.data_ptr() == r["p"].data_ptr()
        p.grad = r["g"]
        opt.state[p] = {"step": torch.tensor(3.0), "exp_avg": r["m"], "exp_avg_sq": r["v"]}
    stats = A.Stats()
    for step in range(2):
        if step:
            for i, r in enumerate(views):
                r["g"].copy_(A.make_grad(r["g"].numel(), 900 + i, 0.1, dtype).to(DEV))
        verify(take_step(opt, hyper["max_norm"]), stats, f"{which}+{offset} step {step}")
    stats.report(f"{which}+{offset}")
    for p, r in zip(params, views):          # the kernels wrote through the views, not into copies
        st = opt.state[p]
        assert p.data_ptr() == r["p"].data_ptr() and st["exp_avg"].data_ptr() == r["m"].data_ptr() and st["exp_avg_sq"].data_ptr() == r["v"].data_ptr()
    for buf, was, off, n in backing:
        assert torch.equal(bits(buf[:off]), bits(was[:off])) and torch.equal(bits(buf[off + n:]), bits(was[off + n:]))


# ------------------------------------------------------------------------------------------------ mixed buckets, one norm
def test_mixed_dtype_buckets_and_two_groups_share_one_norm():
    sizes = [(8193, torch.float32), (20000, torch.bfloat16), (7, torch.float32), (2049, torch.bfloat16), (9, torch.float32),
             (8192, torch.bfloat16), (10243, torch.float32)]
    params = [torch.nn.Parameter(A.make_values(n, 300 + i, 0.5, dt).to(DEV)) for i, (n, dt) in enumerate(sizes)]
    nograd = 4
    opt = HipAdamW([dict(params=params[:5]), dict(params=params[5:], lr=3e-3, weight_decay=0.0)], lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-2)
    before = params[nograd].detach().clone()
    stats = A.Stats()
    for step in range(3):
        for i, (p, (n, dt)) in enumerate(zip(params, sizes)):
            if i != nograd:
                p.grad = A.make_grad(n, 400 + 10 * step + i, 0.05 * (step + 1), dt).to(DEV)
        rec = take_step(opt, 1.0)
        assert len(rec["tensors"]) == len(params) - 1 and {e["hyper"]["lr"] for e in rec["tensors"]} == {1e-3, 3e-3}
        verify(rec, stats, f"mixed step {step}")
    stats.report("mixed")
    assert torch.equal(bits(params[nograd]), bits(before)) and not opt.state.get(params[nograd])


# ------------------------------------------------------------------------------------------------ more than 256 partials
def test_more_than_256_partials_and_a_clip_factor_that_reaches_every_tensor():
    """269 chunks in one bf16 tensor beside the fp32 size list: the strided sum of the partials takes a second pass.  Second step:
    one gradient element of 1e15 in a small tensor - the factor 1e-9 it forces shows in every tensor's update."""
    big_n = 269 * A.CHUNK - 5
    big = torch.nn.Parameter(A.make_values(big_n, 77, 0.5, torch.bfloat16).to(DEV))
    small = [torch.nn.Parameter(x.to(DEV)) for x in A.list_params(torch.float32)]
    opt = HipAdamW([big] + small, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    stats = A.Stats()
    for step, max_norm in enumerate((1.0, 1e6)):
        big.grad = A.make_grad(big_n, 78 + step, 0.05, torch.bfloat16).to(DEV)
        for p, g in zip(small, A.list_grads(torch.float32, step)):
            p.grad = g.to(DEV)
        if step:
            small[3].grad[4] = 1.0e15
        rec = take_step(opt, max_norm)
        assert A.n_chunks(e["before"][1].numel() for e in rec["tensors"]) > 256
        verify(rec, stats, f"big step {step}")
        if step:
            assert 0.99e15 < float(rec["norm"]) < 1.01e15
            # the second moment moved by (1 - beta2) (1e-9 g)^2 and bf16 rounding only: the unclipped (1 - beta2) g^2 is 2.5e-6
            e = rec["tensors"][0]
            dv = A.f64(e["after"][2]) - 0.999 * A.f64(e["before"][3])
            assert float(np.max(np.abs(dv))) < 1e-9
    stats.report("big")


# ------------------------------------------------------------------------------------------------ long runs and the host paths
def test_nine_steps_without_synchronisation_then_replayed():
    """Fresh gradient tensors every step and nothing that waits for the device until the end: the four table slots are each reused
    twice.  lr changes after the fifth step.  Every step is replayed afterwards from its clones."""
    dtype = torch.bfloat16
    params, opt = list_case(dtype, A.GRID["default"])
    grads = [[g.to(DEV) for g in A.list_grads(dtype, step % 3, seed=step)] for step in range(9)]
    torch.cuda.synchronize()
    recs = []
    for step in range(9):
        if step == 5:
            opt.param_groups[0]["lr"] = 2.5e-4
        for p, g in zip(params, grads[step]):
            p.grad = g
        recs.append(take_step(opt, 1.0 if step % 2 else None))
    torch.cuda.synchronize()
    assert len(opt._tables.slots) == 4 and [e["hyper"]["lr"] for e in (recs[4]["tensors"][0], recs[5]["tensors"][0])] == [1e-3, 2.5e-4]
    stats = A.Stats()
    for step, rec in enumerate(recs):
        assert rec["tensors"][0]["t"] == step + 1
        verify(rec, stats, f"long step {step}")
    stats.report("long")


def test_a_gradient_that_goes_and_comes_back():
    """A changed parameter list rebuilds the tables.  A parameter in a group of its own goes on with its own step count; in a
    group with others the step counts then differ, which raises as documented - before anything is stepped."""
    mk = lambda n, s: torch.nn.Parameter(A.make_values(n, s, 0.5, torch.float32).to(DEV))          # noqa: E731
    a, b, c = mk(8193, 1), mk(9, 2), mk(2049, 3)
    opt = HipAdamW([dict(params=[a, b]), dict(params=[c])], lr=1e-3, betas=(0.9, 0.999))
    stats = A.Stats()

    def grads(step, skip=()):
        for i, p in enumerate((a, b, c)):
            p.grad = None if any(p is q for q in skip) else A.make_grad(p.numel(), 50 + 10 * step + i, 0.05, torch.float32).to(DEV)
    grads(0)
    verify(take_step(opt, 1.0), stats, "all")
    grads(1, skip=(c,))
    c_was = c.detach().clone()
    rec = take_step(opt, 1.0)
    assert len(rec["tensors"]) == 2
    verify(rec, stats, "without c")
    assert torch.equal(c, c_was) and step_value(opt.state[c]) == 1.0
    grads(2)
    rec = take_step(opt, 1.0)
    assert [e["t"] for e in rec["tensors"]] == [3.0, 3.0, 2.0]
    verify(rec, stats, "c again")
    grads(3, skip=(a,))
    verify(take_step(opt, None), stats, "without a")
    grads(4)
    was = [p.detach().clone() for p in (a, b, c)]
    with pytest.raises(RuntimeError, match="different step counts"):
        opt.step()
    torch.cuda.synchronize()
    assert all(torch.equal(p, w) for p, w in zip((a, b, c), was)) and [step_value(opt.state[p]) for p in (a, b, c)] == [3.0, 4.0, 3.0]
    stats.report("none-grad")


# ------------------------------------------------------------------------------------------------ loaded state
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("step_at,step_kind", [(10.0, "float"), (1e5, "float"), (10.0, "cpu"), (1e5, "device")])
def test_loaded_torch_state(dtype, step_at, step_kind):
    """A torch.optim.AdamW state_dict (fp32 state; `step` edited to 10 or 1e5, where the bias corrections approach 1, and held as a
    Python float, a CPU tensor or a device tensor) loaded into HipAdamW over fp32 or bf16 parameters: converted, then it replays."""
    hyper = {k: v for k, v in A.GRID["default"].items() if k != "max_norm"}
    sizes = [9, 8193, 20000]
    ref = [torch.nn.Parameter(A.make_values(n, 600 + i, 0.5, torch.float32).to(DEV)) for i, n in enumerate(sizes)]
    opt_ref = torch.optim.AdamW(ref, foreach=False, fused=False, **hyper)
    for i, r in enumerate(ref):
        r.grad = A.make_grad(r.numel(), 610 + i, 0.05, torch.float32).to(DEV)
    opt_ref.step()
    sd = opt_ref.state_dict()
    for st in sd["state"].values():
        st["step"] = {"float": step_at, "cpu": torch.tensor(step_at), "device": torch.tensor(step_at, device=DEV)}[step_kind]
    params = [torch.nn.Parameter(r.detach().to(dtype)) for r in ref]
    opt = HipAdamW(params, **hyper)
    opt.load_state_dict(sd)
    if step_kind == "cpu":          # and the conversion HipAdamW does itself: state assigned directly, in another dtype
        for p, r in zip(params, ref):
            opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"] = opt_ref.state[r]["exp_avg"].double(), opt_ref.state[r]["exp_avg_sq"].double()
    stats = A.Stats()
    for step in range(2):
        for i, p in enumerate(params):
            p.grad = A.make_grad(p.numel(), 620 + 10 * step + i, 0.05, dtype).to(DEV)
        rec = take_step(opt, 1.0 if step else None)
        assert all(e["t"] == step_at + 1 + step for e in rec["tensors"])
        assert all(float(e["before"][3].float().abs().max()) > 0 for e in rec["tensors"]), "the loaded second moment is in use"
        verify(rec, stats, f"loaded step {step}")
    stats.report(f"loaded {step_at} {step_kind}")


# ------------------------------------------------------------------------------------------------ errors
def test_the_three_errors_launch_nothing():
    def fresh():
        p = torch.nn.Parameter(A.make_values(24, 9, 0.5, torch.float32).view(4, 6).to(DEV))
        return p, HipAdamW([p], lr=1e-3)

    def untouched(p, opt, was):
        torch.cuda.synchronize()
        assert torch.equal(bits(p), bits(was)) and len(opt.state) == 0 and opt._tables is None
    for entry in ("step", "clip"):
        run = (lambda o: o.step()) if entry == "step" else (lambda o: o.clip_and_step(1.0))
        # a parameter on the host
        q = torch.nn.Parameter(torch.ones(8))
        q.grad = torch.ones(8)
        oq = HipAdamW([q], lr=1e-3)
        with pytest.raises(RuntimeError, match="GPU only"):
            run(oq)
        assert torch.equal(q.detach(), torch.ones(8)) and len(oq.state) == 0 and oq._tables is None
        # a gradient that is not contiguous
        p, opt = fresh()
        was = p.detach().clone()
        p.grad = torch.ones(6, 4, device=DEV).t()
        assert not p.grad.is_contiguous()
        with pytest.raises(RuntimeError, match="contiguous gradients of the parameter's dtype"):
            run(opt)
        untouched(p, opt, was)
        # a gradient of another dtype (the parameter was cast after its gradient was made)
        p, opt = fresh()
        p.grad = torch.ones(4, 6, device=DEV)
        p.data = p.data.to(torch.bfloat16)
        was = p.detach().clone()
        assert p.grad.dtype == torch.float32 and p.dtype == torch.bfloat16
        with pytest.raises(RuntimeError, match="contiguous gradients of the parameter's dtype"):
            run(opt)
        untouched(p, opt, was)
