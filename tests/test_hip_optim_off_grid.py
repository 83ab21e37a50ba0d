"""The chunk walk of csrc/ttv_optim.hip (`opt_walk`) off the 16-byte grid, for the kernels tests/test_hip_adamw_f64.py does not take
there: device-path AdamW, the EMA update, the EMA exchange and the gradient sums.  `-m gpu`.

Every tensor is a contiguous view of 9, 8193 or 20000 elements (a tail shorter than 8; one element past a chunk; three chunks with a
ragged end) at an element offset into a 16-byte-aligned buffer of sentinels.  What lies outside a view keeps its bits.  The bounds
are the existing ones: tests/weight_ema_ref.py for the update, the gamma_40 of tests/test_hip_grad_norms.py for a chunk's sum; the
rest is equality of bits."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adamw_ref as A  # noqa: E402
import weight_ema_ref as R  # noqa: E402

from titok_video_amd import _lib  # noqa: E402
from titok_video_amd.ema import WeightEMA  # noqa: E402
from titok_video_amd.optim import HipAdamW  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, BF16 = torch.float32, torch.bfloat16
VIEW_SIZES = [9, 8193, 20000]
PAD = 24                   # sentinel elements in front of and behind a view at offset 0: 96 bytes of float, 48 of bf16
SENTINEL = -12345.0        # a bf16 value too


def name(dtype):
    return "fp32" if dtype == F32 else "bf16"


def bits(t):
    return t.detach().view(torch.int16 if t.dtype == BF16 else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


class View:
    """`values` (a CPU tensor) in a view that starts `offset` elements past the 16-byte-aligned element PAD of a sentinel buffer."""

    def __init__(self, values, offset):
        n, item = values.numel(), values.element_size()
        self.buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=values.dtype, device=DEV)
        self.lo, self.hi = PAD + offset, PAD + offset + n
        self.t = self.buf[self.lo:self.hi]
        self.t.copy_(values)
        assert self.buf.data_ptr() % 16 == 0 and self.t.is_contiguous() and self.t.data_ptr() % 16 == offset * item % 16

    def outside_intact(self):
        want = torch.full_like(self.buf, SENTINEL)
        return same_bits(self.buf[:self.lo], want[:self.lo]) and same_bits(self.buf[self.hi:], want[self.hi:])


def tables(rows):
    """Device OptEntry table and chunk list over rows of (p, g, m, v, n), a missing column None; returns (table, chunks, n_chunks)."""
    words, chunks = [], []
    for i, (p, g, m, v, n) in enumerate(rows):
        words += [t.data_ptr() if t is not None else 0 for t in (p, g, m, v)] + [n]
        chunks += [i | (first << 32) for first in range(0, n, R.CHUNK)]
    return torch.tensor(words, dtype=torch.int64).to(DEV), torch.tensor(chunks, dtype=torch.int64).to(DEV), len(chunks)


# ------------------------------------------------------------------------------------------------ device-path AdamW
DEVICE_CASES = [(F32, "pgmv", 1), (BF16, "pgmv", 1), (BF16, "pgmv", 4), (BF16, "pgmv", 8)] + [(BF16, w, 1) for w in "pgmv"]


def adamw_views(dtype, which, offset):
    rows = []
    for i, n in enumerate(VIEW_SIZES):
        row = {}
        for j, k in enumerate("pgmv"):
            values = A.make_values(n, 500 + 10 * i + j, 0.5 if k == "p" else 0.05, dtype)
            if k == "v":
                values = (values.float() ** 2).to(dtype)
            row[k] = View(values, offset if k in which else 0)
        rows.append(row)
    return rows


@pytest.mark.parametrize("dtype,which,offset", DEVICE_CASES, ids=[f"{name(d)}-{w}-{o}" for d, w, o in DEVICE_CASES])
def test_device_path_adamw_off_the_grid_equals_the_host_path(dtype, which, offset):
    """Two clipped steps of HipAdamW(capturable=True) on parameter, gradient and preloaded moments off the grid (bf16 offset 8: on it,
    from a shifted start): the bits of the host path on the same values in the same places."""
    hyper = {k: v for k, v in A.GRID["default_clip"].items() if k != "max_norm"}
    sides = []
    for capturable in (False, True):
        rows = adamw_views(dtype, which, offset)
        params = [torch.nn.Parameter(r["p"].t) for r in rows]
        opt = HipAdamW(params, capturable=capturable, **hyper)
        for p, r in zip(params, rows):
            assert p.data_ptr() == r["p"].t.data_ptr()
            p.grad = r["g"].t
            opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": r["m"].t, "exp_avg_sq": r["v"].t}
        sides.append((rows, params, opt))
    for step in range(2):
        norms = []
        for rows, params, opt in sides:
            if step:
                for i, r in enumerate(rows):
                    r["g"].t.copy_(A.make_grad(r["g"].t.numel(), 900 + i, 0.1, dtype))
            norms.append(opt.clip_and_step(1.0))
        assert same_bits(norms[0], norms[1]) and float(norms[0]) > 1.0, f"step {step}: the clip is active and both paths see one norm"
        (host_rows, _, _), (dev_rows, _, dev) = sides
        assert dev.device_block(0)["updates"] == step + 1 and dev.device_block(0)["clip_coef"] < 1.0
        for i, (h, d) in enumerate(zip(host_rows, dev_rows)):
            for k in "pgmv":
                assert same_bits(h[k].t, d[k].t), f"step {step} tensor {i} ({VIEW_SIZES[i]}) column {k}"
                assert d[k].outside_intact() and h[k].outside_intact(), f"step {step} tensor {i} column {k}: a sentinel was overwritten"
    for rows, params, opt in sides:          # the kernels wrote through the views, and they moved something
        for p, r in zip(params, rows):
            st = opt.state[p]
            assert p.data_ptr() == r["p"].t.data_ptr() and st["exp_avg"].data_ptr() == r["m"].t.data_ptr()
            assert st["exp_avg_sq"].data_ptr() == r["v"].t.data_ptr()
            assert not torch.equal(r["p"].t.cpu(), A.make_values(p.numel(), 500 + 10 * VIEW_SIZES.index(p.numel()), 0.5, dtype))


# ------------------------------------------------------------------------------------------------ EMA update
class Views(torch.nn.Module):
    def __init__(self, dtype, offset):
        super().__init__()
        self.views = [View(R.make_values(n, 10 + i, 0.5, dtype), offset) for i, n in enumerate(VIEW_SIZES)]
        for i, v in enumerate(self.views):
            self.register_parameter(f"w{i}", torch.nn.Parameter(v.t))


def check_update(params, shadows, launch, w, tag):
    """Perturb the parameters, launch, hold every shadow to the float64 replay from the stored state before; twice."""
    worst = 0.0
    for step in range(2):
        for i, p in enumerate(params):
            p.copy_((p.float().cpu() + R.make_values(p.numel(), 2000 + 100 * step + i, 0.02, F32)).to(p.dtype))
        p_was, s_was = [p.clone() for p in params], [s.clone() for s in shadows]
        launch()
        torch.cuda.synchronize()
        fails = []
        for i, (p, pw, s, sw) in enumerate(zip(params, p_was, shadows, s_was)):
            assert same_bits(p, pw), f"{tag} step {step} tensor {i}: the launch wrote a parameter"
            assert not torch.equal(s, sw), f"{tag} step {step} tensor {i}: the shadow did not move"
            f, frac = R.check(R.f64(pw), R.f64(sw), R.f64(s), w, f"{tag} step {step} tensor {i} ({p.numel()})")
            fails += f
            worst = max(worst, frac)
        assert not fails, fails[:5]
    print(f"{tag}: largest error {worst:.3f} of its bound")
    assert worst <= 1.0


@pytest.mark.parametrize("dtype,offset", [(F32, 1), (BF16, 1), (BF16, 4)], ids=["fp32-1", "bf16-1", "bf16-4"])
def test_ema_update_of_parameters_off_the_grid(dtype, offset):
    model = Views(dtype, offset)
    ema = WeightEMA(model, decay=0.999, warmup=False)
    params = [v.t for v in model.views]
    shadows = [ema.shadow[f"w{i}"] for i in range(len(params))]
    assert all(p.data_ptr() % 16 != 0 for p in params) and all(s.data_ptr() % 16 == 0 and s.dtype == F32 for s in shadows)
    w = 1.0 - ema.decay_at(0)
    assert w == 1.0 - ema.decay_at(1)
    with torch.no_grad():
        check_update(params, shadows, ema.update, w, f"{name(dtype)} parameter + {offset}")
    assert all(v.outside_intact() for v in model.views)


def test_ema_update_with_parameter_and_shadow_off_the_grid():
    """A hand-built table (as tools/val_bench.py builds one): bf16 parameters 2 bytes and fp32 shadows 4 bytes past a boundary."""
    ps = [View(R.make_values(n, 10 + i, 0.5, BF16), 1) for i, n in enumerate(VIEW_SIZES)]
    ss = [View(p.t.float().cpu() + R.make_values(p.t.numel(), 40 + i, 0.05, F32), 1) for i, p in enumerate(ps)]
    assert all(p.t.data_ptr() % 16 == 2 for p in ps) and all(s.t.data_ptr() % 16 == 4 for s in ss)
    table, chunks, n_chunks = tables([(p.t, None, s.t, None, p.t.numel()) for p, s in zip(ps, ss)])
    w = 1.0 - 0.999

    def launch():
        _lib.check(_lib.lib().ttv_opt_ema_update(table.data_ptr(), chunks.data_ptr(), n_chunks, _lib.TTV_BF16, w, _lib.stream_ptr(DEV)),
                   "ttv_opt_ema_update")
    check_update([p.t for p in ps], [s.t for s in ss], launch, w, "bf16 parameter + 1, shadow + 1")
    assert all(x.outside_intact() for x in ps + ss)


# ------------------------------------------------------------------------------------------------ EMA exchange
NAN_PAYLOAD = {F32: 0x7FA00001, BF16: 0x7FA1}          # signalling NaNs: a widening or rounding copy would return them quiet
EXCHANGE_CASES = [(F32, w, 1) for w in ("p", "b", "pb")] + [(BF16, w, o) for o in (1, 4) for w in ("p", "b", "pb")]


@pytest.mark.parametrize("dtype,which,offset", EXCHANGE_CASES, ids=[f"{name(d)}-{w}-{o}" for d, w, o in EXCHANGE_CASES])
def test_ema_exchange_off_the_grid(dtype, which, offset):
    """Apply: backup = the parameter's bits, parameter = the shadow cast (round to nearest even for bf16).  Restore: the parameter's old
    bits, a NaN payload and -0.0 in its last elements included.  The shadow is never written."""
    ps = [View(R.make_values(n, 10 + i, 0.5, dtype), offset if "p" in which else 0) for i, n in enumerate(VIEW_SIZES)]
    ss = [View(p.t.float().cpu() + R.make_values(p.t.numel(), 40 + i, 0.05, F32), 0) for i, p in enumerate(ps)]
    bs = [View(torch.full((n,), 7.0, dtype=dtype), offset if "b" in which else 0) for n in VIEW_SIZES]
    for p in ps:
        bits(p.t)[-1] = NAN_PAYLOAD[dtype]
        bits(p.t)[-2] = -0x8000 if dtype == BF16 else -0x80000000          # -0.0
        assert bool(torch.isnan(p.t[-1])) and float(p.t[-2]) == 0.0 and bool(torch.signbit(p.t[-2]))
    table, chunks, n_chunks = tables([(p.t, None, s.t, b.t, p.t.numel()) for p, s, b in zip(ps, ss, bs)])
    p_was, s_was = [p.t.clone() for p in ps], [s.t.clone() for s in ss]

    def exchange(mode):
        _lib.check(_lib.lib().ttv_opt_ema_exchange(table.data_ptr(), chunks.data_ptr(), n_chunks, _lib.dtype_code(dtype), mode,
                                                   _lib.stream_ptr(DEV)), "ttv_opt_ema_exchange")
        torch.cuda.synchronize()
    exchange(0)
    for i, (p, pw, s, sw, b) in enumerate(zip(ps, p_was, ss, s_was, bs)):
        assert same_bits(b.t, pw), f"tensor {i}: the backup is not the old parameter's bits"
        assert same_bits(p.t.cpu(), sw.cpu().to(dtype)), f"tensor {i}: the parameter is not the shadow cast on the host"
        assert same_bits(s.t, sw), f"tensor {i}: apply wrote a shadow"
    assert all(x.outside_intact() for x in ps + ss + bs)
    exchange(1)
    for i, (p, pw, s, sw, b) in enumerate(zip(ps, p_was, ss, s_was, bs)):
        assert same_bits(p.t, pw), f"tensor {i}: restore did not bring the parameter's bits back"
        assert int(bits(p.t)[-1]) == NAN_PAYLOAD[dtype]
        assert same_bits(s.t, sw) and same_bits(b.t, pw), f"tensor {i}: restore wrote a shadow or a backup"
    assert all(x.outside_intact() for x in ps + ss + bs)


# ------------------------------------------------------------------------------------------------ gradient sums
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32-1", "bf16-1"])
def test_grad_sumsq_of_gradients_off_the_grid(dtype):
    """A chunk's partial against the float64 sum of its squares: every square passes through at most D_CHUNK = 40 rounded additions
    of non-negative terms (tests/test_hip_grad_norms.py), so gamma_40 relatively; make_grad keeps the squares normal numbers."""
    gs = [View(A.make_grad(n, 700 + i, 0.05, dtype), 1) for i, n in enumerate(VIEW_SIZES)]
    assert all(g.t.data_ptr() % 16 != 0 for g in gs)
    table, chunks, n_chunks = tables([(None, g.t, None, None, g.t.numel()) for g in gs])
    partials = torch.full((n_chunks + 2,), SENTINEL, dtype=F32, device=DEV)
    _lib.check(_lib.lib().ttv_opt_grad_sumsq(table.data_ptr(), chunks.data_ptr(), n_chunks, _lib.dtype_code(dtype), partials.data_ptr() + 4,
                                             _lib.stream_ptr(DEV)), "ttv_opt_grad_sumsq")
    got = partials.double().cpu().tolist()
    assert got[0] == SENTINEL and got[-1] == SENTINEL and n_chunks == 6
    c = 1
    for g in gs:
        x = A.f64(g.t)
        for first in range(0, x.size, A.CHUNK):
            want = float(np.sum(np.square(x[first:first + A.CHUNK])))
            tol = A.gamma(A.D_CHUNK) * want
            print(f"{name(dtype)} {x.size} chunk at {first}: got {got[c]!r} want {want!r} err {abs(got[c] - want):.3e} bound {tol:.3e}")
            assert want > 0.0 and abs(got[c] - want) <= tol
            c += 1
        assert g.outside_intact()
