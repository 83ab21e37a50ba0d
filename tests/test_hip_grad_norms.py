"""Per-parameter gradient norms (`ttv_opt_param_norms` behind `optim.HipAdamW` and `train.grad_norm_dict`) on the MI355X against
float64 norms of the same stored gradients.  `-m gpu`.

Parameters of 1, 7, 8192, 8193 and 20 000 elements (on and around the 8192-element chunk: one chunk with a tail, exactly one, one
and a single element, three), in fp32 and bf16 within ONE parameter group (two buckets, so parameter order differs from bucket
order), one parameter without a gradient, one all-zero gradient, one gradient with a single huge element.

THE BOUND, counted from the kernels' rounding steps with u = 2^-24 and gamma_n = n u / (1 - n u):
  * k_opt_gradsq, per chunk: a thread adds squares with fmaf (the product is exact inside the fmaf, one rounding per addition).  On
    the 16-byte path it takes 8 per pass, at most 4 passes (8192 / (256 x 8)): 32; a thread that also takes the tail of a chunk
    whose length is no multiple of 8 has made at most 3 passes and adds at most 7 more: 31.  Element by element (a gradient off
    the 16-byte grid) it is 8192 / 256 = 32 again.  So 32 roundings at most.  The block sum is 6 butterfly levels in the wave and
    2 levels over the four waves: 8 more.  A square passes through at most D = 40 rounded additions and every term is >= 0, so
    a partial is within gamma_40 of the exact sum, relatively.
  * k_opt_param_norms adds the K partials of a parameter in ascending order: K - 1 more roundings, gamma_(D + K - 1) in all.  The
    bucket norm adds all C chunks of the bucket: gamma_(D + C - 1).
  * sqrtf halves a relative error and rounds once (within 1 ulp = 2 u); with the cross term: gamma_n / 2 + 3 u.
  * A square below 2^-126 may be flushed or rounded as a denormal: at most 2^-126 absolute per element, sqrt(numel) 2^-63 on the
    norm.  (The huge element is 1e15: its square, 1e30, is far from fp32's end.)
  * The norm over all buckets is taken on the host in float64 from the bucket norms: its relative error is the largest bucket's.
For the largest case here (three chunks of a parameter, eight of a bucket) that is gamma_47 / 2 + 3 u = 1.6e-6 relative; printed per run."""
import math

import pytest
import torch

from titok_video_amd.optim import HipAdamW
from titok_video_amd.train import grad_norm_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
D = 40
CHUNK = 8192
HUGE = 1.0e15


def gamma(n):
    return n * U / (1.0 - n * U)


def rel_bound(n_roundings):
    return gamma(n_roundings) / 2.0 + 3.0 * U


class Net(torch.nn.Module):
    SPEC = [("a1", 1, torch.float32), ("b7", 7, torch.bfloat16), ("c8192", 8192, torch.float32), ("d8193", 8193, torch.bfloat16),
            ("e20000", 20000, torch.float32), ("f20000", 20000, torch.bfloat16), ("nograd7", 7, torch.float32),
            ("zero8193", 8193, torch.float32), ("huge8192", 8192, torch.bfloat16), ("g7", 7, torch.float32)]

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(11)
        for name, n, dt in self.SPEC:
            self.register_parameter(name, torch.nn.Parameter(torch.randn(n, generator=g).to(dt)))


def make(seed=3):
    """A module on the GPU with the planted gradients; returns (module, optimizer)."""
    net = Net().to(DEV)
    g = torch.Generator().manual_seed(seed)
    for name, p in net.named_parameters():
        if name == "nograd7":
            continue
        grad = torch.randn(p.numel(), generator=g)
        if name == "zero8193":
            grad.zero_()
        if name == "huge8192":
            grad[4097] = HUGE
        p.grad = grad.to(p.dtype).to(DEV)
    return net, HipAdamW(net.parameters(), lr=1e-3, betas=(0.5, 0.96), weight_decay=1e-4)


def check_against_float64(net, params, norms):
    with_grad = [(n, p) for n, p in net.named_parameters() if p.grad is not None]
    assert [id(p) for p in params] == [id(p) for _, p in with_grad], "parameter order, the one without a gradient left out"
    n_buckets = len({p.dtype for p in params})
    assert norms.dtype == torch.float32 and norms.is_cuda and norms.numel() == len(params) + n_buckets == len(params) + 2
    host = norms.double().cpu().tolist()
    worst = 0.0
    for (name, p), got in zip(with_grad, host):
        want = float(p.grad.double().norm())
        tol = rel_bound(D + -(-p.numel() // CHUNK) - 1) * want + math.sqrt(p.numel()) * 2.0 ** -63
        print(f"{name}: got {got!r} want {want!r} err {abs(got - want):.3e} bound {tol:.3e}")
        assert abs(got - want) <= tol, (name, got, want, abs(got - want), tol)
        worst = max(worst, tol / want if want else 0.0)
        if name == "zero8193":
            assert got == 0.0
    # bucket norms, in the order the optimizer forms its buckets: the dtypes in order of first appearance
    dtypes = []
    for p in params:
        if p.dtype not in dtypes:
            dtypes.append(p.dtype)
    for dt, got in zip(dtypes, host[len(params):]):
        ps = [p for p in params if p.dtype == dt]
        want = math.sqrt(sum(float(p.grad.double().pow(2).sum()) for p in ps))
        chunks = sum(-(-p.numel() // CHUNK) for p in ps)
        tol = rel_bound(D + chunks - 1) * want + math.sqrt(sum(p.numel() for p in ps)) * 2.0 ** -63
        print(f"bucket {dt}: got {got!r} want {want!r} err {abs(got - want):.3e} bound {tol:.3e}")
        assert abs(got - want) <= tol, (dt, got, want, tol)
        worst = max(worst, tol / want)
    total = HipAdamW.total_norm(host[len(params):])
    want = math.sqrt(sum(float(p.grad.double().pow(2).sum()) for p in params))
    tol = worst * want
    print(f"total: got {total!r} want {want!r} err {abs(total - want):.3e} bound {tol:.3e}; largest relative bound {worst:.2e}")
    assert abs(total - want) <= tol
    return host


def test_param_grad_norms_against_float64_and_twice_the_same_bits():
    net, opt = make()
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    params, norms = opt.param_grad_norms()
    check_against_float64(net, params, norms)
    params2, norms2 = opt.param_grad_norms()
    assert norms2 is not norms and torch.equal(norms.view(torch.int32), norms2.view(torch.int32))
    assert [id(p) for p in params2] == [id(p) for p in params]
    # nothing was stepped and no optimizer state was made
    assert all(torch.equal(p, before[n]) for n, p in net.named_parameters()) and len(opt.state) == 0


def test_clip_and_step_norms_and_a_step_that_is_bit_identical_to_its_twin():
    net, opt = make()
    twin_net, twin = make()
    want_grads = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
    for step in range(2):                # the second step runs on non-zero moments
        gnorm = opt.clip_and_step(1.0, want_param_norms=True)
        twin_gnorm = twin.clip_and_step(1.0)
        params, norms = opt.last_param_norms()
        assert all(torch.equal(p.grad, want_grads[n]) for n, p in net.named_parameters() if p.grad is not None)     # p.grad is left alone
        check_against_float64(net, params, norms)
        assert torch.equal(gnorm.view(torch.int32), twin_gnorm.view(torch.int32))
        for (n, p), (_, q) in zip(net.named_parameters(), twin_net.named_parameters()):
            assert torch.equal(p.view(torch.int16 if p.dtype == torch.bfloat16 else torch.int32),
                               q.view(torch.int16 if q.dtype == torch.bfloat16 else torch.int32)), (step, n)
            if p.grad is None:
                assert p not in opt.state
                continue
            for k in ("exp_avg", "exp_avg_sq"):
                a, b = opt.state[p][k], twin.state[q][k]
                it = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
                assert torch.equal(a.view(it), b.view(it)), (step, n, k)
            assert float(opt.state[p]["step"]) == float(twin.state[q]["step"]) == step + 1
    # the same gradients through the other entry: the same bits
    _, again = opt.param_grad_norms()
    assert torch.equal(again.view(torch.int32), norms.view(torch.int32))
    with pytest.raises(RuntimeError, match="no norms yet"):
        twin.last_param_norms()


def test_grad_norm_dict_keys_order_total_and_reuse():
    net, opt = make()
    d = grad_norm_dict(net, opt)
    names = [n for n, p in net.named_parameters() if p.grad is not None]
    assert "nograd7" not in names and len(names) == len(Net.SPEC) - 1
    assert list(d) == [f"grad_2.0_norm/{n}" for n in names] + ["grad_2.0_norm_total"]
    assert all(isinstance(v, float) for v in d.values())
    listed = [d[f"grad_2.0_norm/{n}"] for n in names]
    assert d["grad_2.0_norm_total"] == pytest.approx(math.sqrt(sum(v * v for v in listed)), rel=1e-14)
    params, norms = opt.last_param_norms()
    assert listed == norms.cpu().tolist()[:len(params)]
    # reuse=True reads what the step has just taken, and launches nothing
    opt.clip_and_step(1.0, want_param_norms=True)
    assert grad_norm_dict(net, opt, norm_type=2.0, reuse=True) == d
    # by default the norms are taken afresh: after a gradient was written in place ...
    net.a1.grad.mul_(2.0)
    d2 = grad_norm_dict(net, opt)
    assert d2["grad_2.0_norm/a1"] == 2.0 * d["grad_2.0_norm/a1"] and d2["grad_2.0_norm/b7"] == d["grad_2.0_norm/b7"]
    with pytest.raises(ValueError, match="norm_type"):
        grad_norm_dict(net, opt, norm_type=1)
    # a module whose parameters have no gradient: Lightning returns an empty dict
    assert grad_norm_dict(torch.nn.Linear(2, 2).to(DEV), opt) == {}
    other = torch.nn.Linear(2, 2).to(DEV)
    other.weight.grad = torch.ones_like(other.weight)
    with pytest.raises(RuntimeError, match="does not belong"):
        grad_norm_dict(other, opt)


def test_fresh_gradient_tensors_give_fresh_norms():
    """The training loop's pattern: zero_grad(set_to_none=True), then new gradient tensors (version 0 again, and very likely the
    blocks the allocator has just got back).  Every read without reuse=True shows the new gradients, from either entry."""
    net, opt = make()
    first = grad_norm_dict(net, opt)
    for round_, scale in enumerate((3.0, 0.25)):
        shapes = {n: (p.grad.clone(), p.dtype) for n, p in net.named_parameters() if p.grad is not None}
        opt.zero_grad(set_to_none=True)
        assert all(p.grad is None for p in net.parameters())
        for n, p in net.named_parameters():
            if n in shapes:
                p.grad = (shapes[n][0].float() * scale).to(p.dtype)
                assert p.grad._version == 0
        if round_ == 0:
            got = grad_norm_dict(net, opt)
        else:
            params, norms = opt.param_grad_norms()
            got = dict(zip([f"grad_2.0_norm/{n}" for n in shapes], norms.cpu().tolist()))
        for n, p in net.named_parameters():
            if n not in shapes or n == "zero8193":
                continue
            want = float(p.grad.double().norm())
            tol = rel_bound(D + -(-p.numel() // CHUNK) - 1) * want + math.sqrt(p.numel()) * 2.0 ** -63
            assert abs(got[f"grad_2.0_norm/{n}"] - want) <= tol, (round_, n, got[f"grad_2.0_norm/{n}"], want)
            assert got[f"grad_2.0_norm/{n}"] != first[f"grad_2.0_norm/{n}"], (round_, n)
    assert list(grad_norm_dict(net, opt)) == list(first)
