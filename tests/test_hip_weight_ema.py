"""`WeightEMA` (titok_video_amd/ema.py; `k_opt_ema_update` / `k_opt_ema_exchange`, csrc/ttv_optim.hip) on the MI355X: the update against
the float64 replay of tests/weight_ema_ref.py inside its counted bound, the exchange bit for bit, the tiny tokenizer trained with the
average beside it (FSQ and the L2 quantiser), the state dict, and `ValidationLoop(..., ema=)`.  `-m gpu`.

Every shadow and backup handed to the C entries sits inside a larger buffer between sentinel values; parameters, shadows and
sentinels are compared as bits around every launch."""
import copy
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adamw_ref as A  # noqa: E402
import weight_ema_ref as R  # noqa: E402

from titok_video_amd import _lib  # noqa: E402
from titok_video_amd.ema import WeightEMA  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
PAD = 8                    # sentinel elements on either side: 32 bytes of float, 16 of bf16 - the tensor between them stays 16-byte aligned
SENTINEL = -12345.0        # a bf16 value too
OFF_GRID_SIZE = 4099       # the tensor whose parameter starts one element (4 or 2 bytes) off the 16-byte grid


def bits(t):
    return t.detach().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(bits(a), bits(b))


class Guarded:
    """n elements of `dtype` between PAD sentinels on either side."""

    def __init__(self, n, dtype):
        self.buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=dtype, device=DEV)
        self.t = self.buf[PAD:PAD + n]
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == 0

    def intact(self):
        want = torch.full((PAD,), SENTINEL, dtype=self.buf.dtype, device=DEV)
        return same_bits(self.buf[:PAD], want) and same_bits(self.buf[PAD + self.t.numel():], want)


class Case:
    """One entry table over adamw_ref.SIZES and the off-grid tensor: parameters of `dtype`, fp32 shadows, backups of `dtype`."""

    def __init__(self, dtype):
        self.dtype = dtype
        item = 4 if dtype == torch.float32 else 2
        sizes = A.SIZES + [OFF_GRID_SIZE]
        self.params, self.shadows, self.backups = [], [], []
        for i, n in enumerate(sizes):
            if i == len(sizes) - 1:
                base = torch.zeros(n + 8, dtype=dtype, device=DEV)
                p = base[1:1 + n]
                assert p.data_ptr() % 16 == item and p.is_contiguous()
            else:
                p = torch.zeros(n, dtype=dtype, device=DEV)
                assert p.data_ptr() % 16 == 0
            p.copy_(R.make_values(n, 10 + i, 0.5, dtype))
            self.params.append(p)
            self.shadows.append(Guarded(n, torch.float32))
            self.backups.append(Guarded(n, dtype))
        words, chunks = [], []
        for i, (p, s, b) in enumerate(zip(self.params, self.shadows, self.backups)):
            words += [p.data_ptr(), 0, s.t.data_ptr(), b.t.data_ptr(), p.numel()]
            chunks += [i | (first << 32) for first in range(0, p.numel(), R.CHUNK)]
        self.n_chunks = len(chunks)
        self.table = torch.tensor(words, dtype=torch.int64).to(DEV)
        self.chunks = torch.tensor(chunks, dtype=torch.int64).to(DEV)
        assert self.n_chunks == A.n_chunks(sizes) and self.n_chunks > len(sizes)

    def set_shadows(self, seed, equal_rows=()):
        for i, (p, s) in enumerate(zip(self.params, self.shadows)):
            if i in equal_rows:
                s.t.copy_(p.float())
            else:
                s.t.copy_((p.float().cpu() + R.make_values(p.numel(), seed + i, 0.05, torch.float32)).to(DEV))

    def perturb_params(self, seed):
        for i, p in enumerate(self.params):
            p.copy_((p.float().cpu() + R.make_values(p.numel(), seed + i, 0.02, torch.float32)).to(self.dtype))

    def update(self, w):
        _lib.check(_lib.lib().ttv_opt_ema_update(self.table.data_ptr(), self.chunks.data_ptr(), self.n_chunks, _lib.dtype_code(self.dtype), w,
                                                 _lib.stream_ptr(DEV)), "ttv_opt_ema_update")

    def exchange(self, mode):
        _lib.check(_lib.lib().ttv_opt_ema_exchange(self.table.data_ptr(), self.chunks.data_ptr(), self.n_chunks, _lib.dtype_code(self.dtype), mode,
                                                   _lib.stream_ptr(DEV)), "ttv_opt_ema_exchange")

    def guards_intact(self):
        return all(g.intact() for g in self.shadows + self.backups)


# ------------------------------------------------------------------------------------------------ the update, through the C ABI
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_update_against_the_float64_replay(dtype):
    """Every w of the grid: three updates with the parameters perturbed in between, each held to the replay from the stored state
    before it.  Row 2 starts with shadow == parameter and stays so as a number through its first update.  The launch writes neither the
    parameters nor anything outside the shadows."""
    case = Case(dtype)
    for wi, w in enumerate(R.W_GRID):
        case.set_shadows(1000 * (wi + 1), equal_rows=(2, 9))
        worst = 0.0
        for step in range(3):
            if step:
                case.perturb_params(2000 * (wi + 1) + 100 * step)
            p_was = [p.clone() for p in case.params]
            s_was = [s.t.clone() for s in case.shadows]
            case.update(w)
            torch.cuda.synchronize()
            fails = []
            for i, (p, pw, s, sw) in enumerate(zip(case.params, p_was, case.shadows, s_was)):
                assert same_bits(p, pw), f"w {w} step {step} tensor {i}: the launch wrote a parameter"
                f, frac = R.check(R.f64(pw), R.f64(sw), R.f64(s.t), w, f"w {w!r} step {step} tensor {i} ({p.numel()})")
                fails += f
                worst = max(worst, frac)
                if step == 0 and i in (2, 9):
                    assert torch.equal(s.t, sw), f"w {w}: p == s must leave s unchanged as a number (tensor {i})"
                elif w * float((pw.float() - sw).abs().max()) > 0:
                    assert not torch.equal(s.t, sw), f"w {w} step {step} tensor {i}: the shadow did not move"
            assert not fails, fails[:5]
            assert case.guards_intact(), f"w {w} step {step}: a sentinel was overwritten"
        print(f"{IDS[DTYPES.index(dtype)]} w = {w!r}: largest error {worst:.3f} of its bound")
        assert worst <= 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_weight_zero_leaves_every_shadow_bit(dtype):
    case = Case(dtype)
    case.set_shadows(77)
    # values whose sum with a zero product would not keep their bits, or whose product with zero is not zero
    case.shadows[3].t[:4] = torch.tensor([-0.0, float("inf"), float("nan"), 1e-40], device=DEV)
    case.params[4][:2] = torch.tensor([float("inf"), float("nan")], device=DEV).to(dtype)
    p_was, s_was = [p.clone() for p in case.params], [s.t.clone() for s in case.shadows]
    case.update(0.0)
    torch.cuda.synchronize()
    for p, pw, s, sw in zip(case.params, p_was, case.shadows, s_was):
        assert same_bits(p, pw) and same_bits(s.t, sw)
    assert case.guards_intact()


# ------------------------------------------------------------------------------------------------ the exchange
def _f32_from_bits(words):
    return torch.from_numpy(np.array(words, dtype=np.uint32).view(np.float32).copy())


SPECIALS = _f32_from_bits([0x00000000, 0x80000000,          # +0, -0
                           0x00400000,                      # a denormal (2^-127: a bf16 denormal too)
                           0x7F800000, 0xFF800000,          # +inf, -inf
                           0x7FC00000,                      # NaN
                           0x3F808000,                      # halfway between bf16 0x3F80 (even) and 0x3F81: rounds down
                           0x3F818000,                      # halfway between bf16 0x3F81 (odd) and 0x3F82: rounds up
                           0x7F7F0001,                      # just above bf16's largest finite value: rounds to it
                           0x7F7F8000])                     # halfway between it and infinity: rounds to infinity


def assert_same_values(got, want, what):
    """Bit for bit, except that a NaN is any NaN."""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), what
    assert torch.equal(bits(got)[~nan], bits(want)[~nan]), what


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exchange_applies_the_cast_shadow_and_restores_the_parameter_bits(dtype):
    case = Case(dtype)
    case.set_shadows(500)
    k = SPECIALS.numel()
    for s in case.shadows:          # at the head of every tensor (vector path, or the element loop of the off-grid one) and at its tail
        n = s.t.numel()
        s.t[:min(n, k)] = SPECIALS[:min(n, k)].to(DEV)
        if n >= 2 * k:
            s.t[n - k:] = SPECIALS.flip(0).to(DEV)
    case.params[5][:3] = torch.tensor([float("nan"), float("-inf"), -0.0], device=DEV).to(dtype)          # the backup keeps bits
    p_was, s_was = [p.clone() for p in case.params], [s.t.clone() for s in case.shadows]
    assert same_bits(s_was[-1][:k].cpu(), SPECIALS)
    case.exchange(0)
    torch.cuda.synchronize()
    for i, (p, pw, s, sw, b) in enumerate(zip(case.params, p_was, case.shadows, s_was, case.backups)):
        assert same_bits(b.t, pw), f"tensor {i}: the backup is not the old parameter"
        assert_same_values(p.cpu(), sw.cpu().to(dtype), f"tensor {i}: the parameter is not the shadow cast on the host")
        assert same_bits(s.t, sw), f"tensor {i}: the exchange wrote a shadow"
    assert case.guards_intact()
    if dtype == torch.bfloat16:
        head = bits(case.params[-2][:k].cpu()).tolist()          # the 20000-element tensor: the vector path
        assert [h & 0xFFFF for h in head] == [0x0000, 0x8000, 0x0040, 0x7F80, 0xFF80, head[5] & 0xFFFF, 0x3F80, 0x3F82, 0x7F7F, 0x7F80]
    case.exchange(1)
    torch.cuda.synchronize()
    for i, (p, pw, s, sw, b) in enumerate(zip(case.params, p_was, case.shadows, s_was, case.backups)):
        assert same_bits(p, pw), f"tensor {i}: restore did not bring the parameter's bits back"
        assert same_bits(s.t, sw) and same_bits(b.t, pw)
    assert case.guards_intact()


# ------------------------------------------------------------------------------------------------ through the model
CLIP_SHAPES, COUNTS = [(4, 16, 16), (8, 16, 24)], [3, 5]


def model_cfg(kind):
    if kind == "fsq":
        m = SimpleNamespace(patch_size=[4, 8, 8], fsq_levels=[7, 5, 5, 5, 5], encoder_size="tiny", decoder_size="tiny")
    else:
        m = SimpleNamespace(patch_size=[4, 8, 8], fsq_levels=None, quantizer="l2", codebook_size=256, token_size=8, encoder_size="tiny",
                            decoder_size="tiny")
    return SimpleNamespace(tokenizer=SimpleNamespace(model=m))


def new_model(kind):
    from titok_video_amd.model.titok import TiTok
    torch.manual_seed(0)
    return TiTok(model_cfg(kind)).to(DEV, torch.float32).train()


def twin_of(kind, state):
    m = new_model(kind)
    m.load_state_dict(state, strict=True)
    return m


def forward(model, clips):
    with torch.no_grad():
        recon, info = model(clips, COUNTS)
    return [r.clone() for r in recon], info["indices"].clone()


def same_forward(a, b):
    return all(same_bits(x, y) for x, y in zip(a[0], b[0])) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("kind", ["fsq", "l2"])
def test_training_with_the_average_and_validation_on_it(kind):
    from titok_video_amd.synthetic import synthetic_clips
    from titok_video_amd.train import make_optimizer, training_step
    clips = synthetic_clips(CLIP_SHAPES, seed=31, dtype=torch.float32, device=DEV)
    model = new_model(kind)
    opt = make_optimizer(model)
    ema = WeightEMA(model, decay=0.5, warmup=False)
    names = [n for n, p in model.named_parameters() if p.is_floating_point()]
    assert list(ema.shadow) == names and all(same_bits(ema.shadow[n], p.detach()) for n, p in model.named_parameters())
    if kind == "l2":
        assert "quantize.codebook" in ema.shadow
    # three steps, every update against the replay of that step from the snapshots
    for step in range(3):
        loss, _, _ = training_step(model, clips, COUNTS, opt)
        assert torch.isfinite(loss)
        s_was = {n: s.clone() for n, s in ema.shadow.items()}
        p_was = {n: p.detach().clone() for n, p in model.named_parameters()}
        ema.update()
        torch.cuda.synchronize()
        assert ema.num_updates == step + 1
        fails, moved = [], 0
        for n, p in model.named_parameters():
            assert same_bits(p.detach(), p_was[n])
            f, _ = R.check(R.f64(p_was[n]), R.f64(s_was[n]), R.f64(ema.shadow[n]), 0.5, f"{kind} step {step} {n}")
            fails += f
            moved += int(not torch.equal(ema.shadow[n], s_was[n]))
        assert not fails, fails[:5]
        assert moved > len(names) // 2, "decay 0.5: the shadows move visibly"
    # the average in the model: the forward of a second model that loaded model_state_dict(), bit for bit
    raw_state = {k: v.clone() for k, v in model.state_dict().items()}
    before = forward(model, clips)
    averaged = twin_of(kind, ema.model_state_dict())
    want = forward(averaged, clips)
    assert not same_forward(before, want), "the average differs from the raw weights after three steps"
    with ema.applied():
        assert same_forward(forward(model, clips), want)
        for n, p in model.named_parameters():
            assert same_bits(p.detach(), ema.shadow[n].to(p.dtype)), n
        with pytest.raises(RuntimeError, match="nest"):
            with ema.applied():
                pass
        with pytest.raises(RuntimeError, match="applied"):
            ema.update()
    # and out again: the raw weights bit for bit, and nothing that cached the averaged ones
    for k, v in model.state_dict().items():
        assert same_bits(v, raw_state[k]), k
    assert same_forward(forward(model, clips), before)
    # an exception inside the block still restores
    with pytest.raises(ZeroDivisionError):
        with ema.applied():
            assert same_forward(forward(model, clips), want)
            1 // 0
    for k, v in model.state_dict().items():
        assert same_bits(v, raw_state[k]), k
    assert same_forward(forward(model, clips), before)
    assert ema.num_updates == 3
    # a further training step beside a twin the average never touched (same weights, same optimizer state).  The forward is
    # deterministic: the same token indices.  The L1 sum is 10 block partials (5 blocks per clip, ttvk_l1_loss) added with atomics in
    # arrival order, all terms >= 0: two orders differ by at most 2 gamma_10 of the loss.  The gradients carry the backward's own
    # atomic-order noise, held as tests/test_hip_dp_train.py holds two runs of one backward: 1e-4 of the tensor's largest entry.
    twin = twin_of(kind, raw_state).train()
    opt_twin = make_optimizer(twin)
    opt_twin.load_state_dict(copy.deepcopy(opt.state_dict()))          # its own moments: load_state_dict keeps tensors that already fit
    loss_a, _, idx_a = training_step(model, clips, COUNTS, opt)
    loss_b, _, idx_b = training_step(twin, clips, COUNTS, opt_twin)
    torch.cuda.synchronize()
    assert torch.equal(idx_a, idx_b)
    assert abs(float(loss_a) - float(loss_b)) <= 2 * A.gamma(10) * float(loss_b), (float(loss_a), float(loss_b))
    grads_b = dict(twin.named_parameters())
    for n, p in model.named_parameters():
        q = grads_b[n]
        assert (p.grad is None) == (q.grad is None), n
        if p.grad is not None:
            scale = float(q.grad.abs().max()) + 1e-12
            assert float((p.grad - q.grad).abs().max()) < 1e-4 * scale, n


# ------------------------------------------------------------------------------------------------ state
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_loaded_average_continues_bit_for_bit(dtype):
    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.ws = torch.nn.ParameterList([torch.nn.Parameter(R.make_values(n, 40 + i, 0.5, dtype)) for i, n in enumerate([9, 8193, 20000])])
            self.frozen = torch.nn.Parameter(R.make_values(2049, 50, 0.5, torch.float32), requires_grad=False)          # a second dtype bucket under bf16
            self.register_buffer("count", torch.zeros(3))
    net = Net().to(DEV)
    ema = WeightEMA(net, decay=0.999, warmup=True)
    for step in range(4):
        with torch.no_grad():
            for i, p in enumerate(net.parameters()):
                p.add_(R.make_values(p.numel(), 60 + 10 * step + i, 0.02, p.dtype).to(DEV))
        ema.update()
    state = ema.state_dict()
    assert state["num_updates"] == 4 and list(state["shadow"]) == [n for n, _ in net.named_parameters()]
    other_net = Net().to(DEV)
    other_net.load_state_dict(net.state_dict())
    other = WeightEMA(other_net, decay=0.5, warmup=False)
    other.load_state_dict({**state, "shadow": {k: v.cpu() for k, v in state["shadow"].items()}})          # as a checkpoint holds them
    assert (other.decay, other.warmup, other.num_updates) == (0.999, True, 4)
    for n in (net, other_net):
        with torch.no_grad():
            for i, p in enumerate(n.parameters()):
                p.add_(R.make_values(p.numel(), 900 + i, 0.02, p.dtype).to(DEV))
    ema.update()
    other.update()
    torch.cuda.synchronize()
    assert ema.num_updates == other.num_updates == 5
    for k in ema.shadow:
        assert same_bits(ema.shadow[k], other.shadow[k]) and ema.shadow[k].data_ptr() != other.shadow[k].data_ptr(), k
    # reset(): the shadows are the parameters again
    ema.reset()
    assert ema.num_updates == 0 and all(same_bits(ema.shadow[n], p.detach().float()) for n, p in net.named_parameters())
    # the buffer is not averaged, and a parameter that is not a float is not either
    assert "count" not in ema.shadow


def test_construction_refuses_what_the_kernels_do_not_take():
    lin = torch.nn.Linear(4, 4)
    with pytest.raises(RuntimeError, match="GPU only"):
        WeightEMA(lin)
    with pytest.raises(RuntimeError, match="fp32 or bf16"):
        WeightEMA(torch.nn.Linear(4, 4).to(DEV, torch.float16))
    strided = torch.nn.Linear(4, 4).to(DEV)
    strided.weight = torch.nn.Parameter(torch.randn(4, 8, device=DEV)[:, ::2])
    with pytest.raises(RuntimeError, match="contiguous"):
        WeightEMA(strided)
    with pytest.raises(ValueError, match="decay"):
        WeightEMA(torch.nn.Linear(4, 4).to(DEV), decay=1.5)


# ------------------------------------------------------------------------------------------------ ValidationLoop(..., ema=)
def test_validation_loop_runs_on_the_average_and_leaves_the_weights():
    from titok_video_amd.model.metrics.eval_metrics import EvalMetrics
    from titok_video_amd.synthetic import synthetic_clips
    from titok_video_amd.train import ValidationLoop, make_optimizer, training_step
    cfg = model_cfg("fsq")
    cfg.training = SimpleNamespace(eval=SimpleNamespace(log_metrics=["psnr"]))
    clips = synthetic_clips(CLIP_SHAPES, seed=31, dtype=torch.float32, device=DEV)
    model = new_model("fsq")
    opt = make_optimizer(model)
    ema = WeightEMA(model, decay=0.5, warmup=False)
    for _ in range(2):
        training_step(model, clips, COUNTS, opt)
        ema.update()
    batches = [{"video": synthetic_clips(CLIP_SHAPES, seed=40 + k, dtype=torch.float32, device=DEV), "fps": [8, 12.5], "token_counts": COUNTS}
               for k in range(2)]
    averaged = twin_of("fsq", ema.model_state_dict())

    def epoch(loop):
        loop.start()
        logged = [loop.step(b) for b in batches]
        return logged, loop.end()
    want_logged, want = epoch(ValidationLoop(averaged, EvalMetrics(cfg), log_recon_num=2, eval_samples=4, random_recon=False))
    raw_logged, raw = epoch(ValidationLoop(model, EvalMetrics(cfg), log_recon_num=2, eval_samples=4, random_recon=False))
    was = {k: v.clone() for k, v in model.state_dict().items()}
    got_logged, got = epoch(ValidationLoop(model, EvalMetrics(cfg), log_recon_num=2, eval_samples=4, random_recon=False, ema=ema))
    assert set(got) == {"eval/psnr"} and got == want and got != raw
    for a, b in zip(got_logged, want_logged):
        assert len(a) == len(b) and all(x["key"] == y["key"] and np.array_equal(x["video"], y["video"]) for x, y in zip(a, b))
    for k, v in model.state_dict().items():
        assert same_bits(v, was[k]), k
    assert not ema._applied
    # and the loop without an average is what it was
    assert epoch(ValidationLoop(model, EvalMetrics(cfg), log_recon_num=2, eval_samples=4, random_recon=False))[1] == raw
