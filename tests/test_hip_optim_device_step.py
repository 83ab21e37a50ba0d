"""HipAdamW's device path (titok_video_amd/optim.py: capturable=True / skip_nonfinite=True; csrc/ttv_optim.hip k_opt_prepare,
k_opt_adamw_dev): the step count, both bias corrections, the learning rate and the skip decision live in a device block.

The yardsticks: Python doubles rounded once (the block's floats, bit for bit), the host path on the same tensors and gradients (bit
for bit: the element arithmetic and the floats are the same; the host path itself is held to float64 by tests/test_hip_adamw_f64.py),
and for the towers' training step the bounds of tests/test_hip_backward.py's graph test.  `-m gpu`."""
import copy
import math
import os
import struct
import sys
from types import SimpleNamespace

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import adamw_ref as A  # noqa: E402

from titok_video_amd.optim import HipAdamW  # noqa: E402
from titok_video_amd.schedule import CosineWarmupLR, cosine_warmup_lr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SIZES = [1, 7, 8191, 8192, 8193, 20000]          # one chunk is 8192 elements
OFFSET_SIZE = 1000                                # one more tensor per dtype, viewed 4 bytes off the 16-byte grid
HYPER = dict(lr=1e-3, betas=(0.5, 0.96), eps=1e-8, weight_decay=1e-2)
SMALL = dict(warmup_steps=4, training_steps=12, base_lr=1e-3, end_lr=1e-4)
LONG = [0, 1, 2, 999, 1000, 1001, 300500, 599999, 600000, 600001, 900000, 1200000]
GOLDEN_SETS = [((1e-4, 1e-5, 1000, 600000), LONG), ((1.5e-5, 1.5e-6, 1000, 600000), LONG), ((1e-4, 0.0, 0, 10), list(range(25))),
               ((3e-4, 1e-5, 5, 5), list(range(25))), ((1e-3, 1e-4, 4, 12), list(range(1, 30)))]


def f32(x: float) -> float:
    """A Python double rounded once to float32, widened again."""
    return struct.unpack("<f", struct.pack("<f", x))[0]


def _off_grid(values):
    """The values in a tensor whose storage starts 4 bytes past a 16-byte boundary."""
    k = 4 // values.element_size()
    base = torch.empty(values.numel() + k, dtype=values.dtype, device=DEV)
    view = base[k:]
    view.copy_(values)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _tensors(seed, scale, grad=False, step=0):
    """Every size in fp32 and in bf16, plus the off-grid tensor of each dtype: a list of 14 device tensors."""
    make = A.make_grad if grad else A.make_values
    out = []
    for j, dt in enumerate((torch.float32, torch.bfloat16)):
        for i, n in enumerate(SIZES):
            out.append(make(n, seed + 1000 * step + 100 * j + i, scale, dt).to(DEV))
        out.append(_off_grid(make(OFFSET_SIZE, seed + 1000 * step + 100 * j + 50, scale, dt).to(DEV)))
    return out


def _params(seed=3):
    return [torch.nn.Parameter(t) for t in _tensors(seed, 0.5)]


def _groups(ps, **second):
    """Two groups, each with both dtypes: the small sizes, and the rest with hyper-parameters of its own."""
    first = [p for p in ps if p.numel() <= 8192 and p.numel() != OFFSET_SIZE]
    rest = [p for p in ps if not any(p is q for q in first)]
    return [{"params": first}, dict({"params": rest, "weight_decay": 0.0}, **second)]


def _set_grads(ps, step, scale=0.05, seed=7000):
    for p, g in zip(ps, _tensors(seed, scale * (step + 1), grad=True, step=step)):
        p.grad = g


def _state_bits(opt, ps):
    """Parameters and both moments as CPU tensors (moments that do not exist yet: None)."""
    out = []
    for p in ps:
        st = opt.state.get(p) or {}
        out.append((p.detach().cpu().clone(), st["exp_avg"].cpu().clone() if "exp_avg" in st else None,
                    st["exp_avg_sq"].cpu().clone() if "exp_avg_sq" in st else None))
    return out


def _same_bits(a, b, what=""):
    for i, (x, y) in enumerate(zip(a, b)):
        for name, u, v in zip("pmv", x, y):
            assert (u is None) == (v is None), (what, i, name)
            if u is not None:      # compare bits, so that NaN equals NaN and -0 differs from 0
                iu, iv = u.view(torch.int16 if u.dtype == torch.bfloat16 else torch.int32), v.view(torch.int16 if v.dtype == torch.bfloat16 else torch.int32)
                assert torch.equal(iu, iv), (what, i, name, int((iu != iv).sum()), u.numel())


def _bits_of(t: torch.Tensor) -> int:
    return int(t.detach().reshape(1).cpu().view(torch.int32).item())


# ------------------------------------------------------------------------------------------------------ the block's floats
@pytest.mark.parametrize("betas", [(0.5, 0.96), (0.9, 0.999)])
def test_bias_corrections_are_python_doubles_rounded_once(betas):
    """t from {1..10, 100, 1000, 100000, 2^24 + 1}, set by loading step = t - 1; lr_constant as well."""
    p = torch.nn.Parameter(torch.ones(7, device=DEV))
    opt = HipAdamW([p], lr=1e-3, betas=betas, capturable=True)
    p.grad = torch.full_like(p, 0.01)
    opt.step()
    template = copy.deepcopy(opt.state_dict())
    b1, b2 = betas
    for t in list(range(1, 11)) + [100, 1000, 100000, 2 ** 24 + 1]:
        sd = copy.deepcopy(template)
        sd["state"][0]["step"] = torch.tensor(float(t - 1), dtype=torch.float32)
        opt.load_state_dict(sd)
        assert opt.applied_updates() == t - 1
        opt.step()
        blk = opt.device_block()
        print(f"betas {betas} t {t}: bc1 {blk['bc1']!r} bc2_sqrt {blk['bc2_sqrt']!r}")
        assert blk["updates"] == t and blk["skip_now"] == 0 and blk["schedule_index"] == 0
        assert blk["bc1"] == f32(1.0 - b1 ** float(t)), t
        assert blk["bc2_sqrt"] == f32(math.sqrt(1.0 - b2 ** float(t))), t
        assert blk["lr"] == f32(1e-3) and blk["clip_coef"] == 1.0


@pytest.mark.parametrize("which", range(len(GOLDEN_SETS)))
def test_scheduled_rate_is_the_python_double_rounded_once(which):
    (base_lr, end_lr, warmup, total), indices = GOLDEN_SETS[which]
    p = torch.nn.Parameter(torch.ones(7, device=DEV))
    opt = HipAdamW([p], lr=base_lr, capturable=True)
    sched = CosineWarmupLR(opt, warmup, total, base_lr, end_lr)
    assert sched.on_device
    p.grad = torch.full_like(p, 0.01)
    opt.step()
    template = copy.deepcopy(opt.state_dict())
    for k in indices:
        sd = copy.deepcopy(template)
        sd["state"][0]["step"] = torch.tensor(float(k), dtype=torch.float32)          # update number k runs at index k
        opt.load_state_dict(sd)
        opt.step()
        blk = opt.device_block()
        want = cosine_warmup_lr(k, warmup, total, base_lr, end_lr)
        print(f"set {which} index {k}: lr {blk['lr']!r} want {f32(want)!r}")
        assert blk["schedule_index"] == k and blk["updates"] == k + 1
        assert blk["lr"] == f32(want), (k, blk["lr"], want)
        assert _bits_of(opt.last_lr()) == struct.unpack("<i", struct.pack("<f", want))[0]
        assert sched.get_last_lr() == [f32(want)] and sched.last_epoch == k + 1


def test_first_and_stride_on_the_device():
    p = torch.nn.Parameter(torch.ones(7, device=DEV))
    for first, stride, want in ((-1, 2, [0, 1, 3, 5]), (0, 2, [0, 2, 4, 6])):
        opt = HipAdamW([p], lr=1e-3, capturable=True)
        CosineWarmupLR(opt, first=first, stride=stride, **SMALL)
        seen = []
        for _ in want:
            p.grad = torch.full_like(p, 0.01)
            opt.step()
            blk = opt.device_block()
            seen.append(blk["schedule_index"])
            assert blk["lr"] == f32(cosine_warmup_lr(blk["schedule_index"], **SMALL))
        assert seen == want


# ------------------------------------------------------------------------------------------------------ device path == host path
@pytest.mark.parametrize("max_norm", [1.0, None])
def test_device_path_equals_host_path_bit_for_bit(max_norm):
    """Nine updates at a constant rate, clipped at 1.0 (the gradients' norm is above 10 and grows) and unclipped."""
    host_p, dev_p = _params(), _params()
    host = HipAdamW(_groups(host_p, lr=3e-4), **HYPER)
    dev = HipAdamW(_groups(dev_p, lr=3e-4), capturable=True, **HYPER)
    for step in range(9):
        _set_grads(host_p, step)
        _set_grads(dev_p, step)
        if max_norm is None:
            host.step(), dev.step()
        else:
            nh, nd = host.clip_and_step(max_norm), dev.clip_and_step(max_norm)
            assert _bits_of(nh) == _bits_of(nd) and float(nh) > max_norm, step
            assert dev.device_block(1)["norm"] == float(nd) and dev.device_block(0)["clip_coef"] < 1.0
        _same_bits(_state_bits(host, host_p), _state_bits(dev, dev_p), f"step {step}")
    sd = dev.state_dict()
    assert all(float(st["step"]) == 9.0 for st in sd["state"].values()) and len(sd["state"]) == len(dev_p)
    assert [g["skipped"] for g in sd["param_groups"]] == [0, 0]


def test_scheduled_run_equals_host_path_with_the_schedule_fed_by_hand():
    """Twenty updates with the schedule on the device and no host work between them, then the same on the host path with
    group['lr'] = cosine_warmup_lr(u, ..)."""
    host_p, dev_p = _params(), _params()
    dev = HipAdamW(_groups(dev_p), capturable=True, **HYPER)
    sched = CosineWarmupLR(dev, **SMALL)
    rates = []
    for u in range(20):
        _set_grads(dev_p, u % 5)
        dev.clip_and_step(1.0)
        rates.append(dev.last_lr())          # device scalars: nothing is read until the loop is over
    snap = _state_bits(dev, dev_p)
    assert [float(r) for r in rates] == [f32(cosine_warmup_lr(u, **SMALL)) for u in range(20)]
    assert rates[0].item() == 0.0 and sched.last_epoch == 20
    host = HipAdamW(_groups(host_p), **HYPER)
    for u in range(20):
        _set_grads(host_p, u % 5)
        for g in host.param_groups:
            g["lr"] = cosine_warmup_lr(u, **SMALL)
        host.clip_and_step(1.0)
    _same_bits(_state_bits(host, host_p), snap)


# ------------------------------------------------------------------------------------------------------ skip
def _run_with_bad_step(bad, skip_nonfinite=True):
    """Six calls; call 3 (counting from 1) has one bad element in one gradient.  Returns (optimizer, parameters, bits before the bad
    call, bits after it)."""
    ps = _params()
    opt = HipAdamW(_groups(ps), capturable=True, skip_nonfinite=skip_nonfinite, **HYPER)
    CosineWarmupLR(opt, **SMALL)
    before = after = None
    good = 0
    for call in range(1, 7):
        _set_grads(ps, good)
        if call == 3:
            ps[4].grad = ps[4].grad.clone()
            ps[4].grad[4321] = bad
            before = _state_bits(opt, ps)
        norm = opt.clip_and_step(1.0)
        if call == 3:
            after = _state_bits(opt, ps)
            assert not math.isfinite(float(norm))
            if not skip_nonfinite:
                return opt, ps, before, after
            assert opt.skipped_steps() == 1 and opt.skipped_steps(1) == 1
            sd = opt.state_dict()
            assert all(float(st["step"]) == 2.0 for st in sd["state"].values()) and sd["param_groups"][0]["skipped"] == 1
            assert opt.device_block()["skip_now"] == 1
            continue
        if call == 4:
            blk = opt.device_block()          # the update after the bad call: t = 3, the rate of three applied updates' index
            assert blk["updates"] == 3 and blk["schedule_index"] == 2 and blk["skip_now"] == 0
            assert blk["lr"] == f32(cosine_warmup_lr(2, **SMALL)) and blk["bc1"] == f32(1.0 - 0.5 ** 3.0)
        good += 1
    return opt, ps, before, after


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_step_is_skipped_and_counted(bad):
    opt, ps, before, after = _run_with_bad_step(bad)
    _same_bits(before, after, "the skipped call")
    clean_p = _params()
    clean = HipAdamW(_groups(clean_p), capturable=True, skip_nonfinite=True, **HYPER)
    CosineWarmupLR(clean, **SMALL)
    for u in range(5):
        _set_grads(clean_p, u)
        clean.clip_and_step(1.0)
    _same_bits(_state_bits(clean, clean_p), _state_bits(opt, ps), "against a run that never saw the bad step")
    assert opt.applied_updates() == clean.applied_updates() == 5 and clean.skipped_steps() == 0 and opt.skipped_steps() == 1


def test_without_skip_a_nan_norm_poisons_every_parameter_as_before():
    opt, ps, before, after = _run_with_bad_step(float("nan"), skip_nonfinite=False)
    assert all(bool(torch.isnan(p.float()).all()) for p, _, _ in after)
    assert opt.applied_updates() == 3 and opt.skipped_steps() == 0


# ------------------------------------------------------------------------------------------------------ capture
def test_captured_step_replays_with_the_count_it_finds():
    """A graph over clip_and_step, replayed five times with new gradient values in the captured buffers == five eager calls."""
    eager_p, graph_p = _params(), _params()
    eager = HipAdamW(_groups(eager_p), capturable=True, **HYPER)
    graphed = HipAdamW(_groups(graph_p), capturable=True, **HYPER)
    CosineWarmupLR(eager, **SMALL), CosineWarmupLR(graphed, **SMALL)
    _set_grads(graph_p, 0)
    buffers = [p.grad for p in graph_p]
    start = _state_bits(graphed, graph_p)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        graphed.clip_and_step(1.0)          # the warm-up step: state, tables, the block
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize(DEV)
    saved = copy.deepcopy(graphed.state_dict())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        norm = graphed.clip_and_step(1.0)
    with torch.no_grad():                   # undo the warm-up in place: the graph holds these addresses
        for p, (q, _, _) in zip(graph_p, start):
            p.copy_(q)
    empty = {"state": {}, "param_groups": saved["param_groups"]}
    graphed.restore_in_place(empty)
    assert graphed.applied_updates() == 0
    retired = graphed._tables.retired[0]["host"].clone()
    for step in range(5):
        _set_grads(eager_p, step)
        for buf, p in zip(buffers, eager_p):
            buf.copy_(p.grad)
        graph.replay()
        norm_e = eager.clip_and_step(1.0)
        assert _bits_of(norm) == _bits_of(norm_e), step
        _same_bits(_state_bits(eager, eager_p), _state_bits(graphed, graph_p), f"replay {step}")
    sd = graphed.state_dict()
    assert all(float(st["step"]) == 5.0 for st in sd["state"].values()) and graphed.applied_updates() == 5
    # the table the replays read has left the rotation: eager steps in between never rewrite it
    graphed.clip_and_step(1.0)
    assert torch.equal(graphed._tables.retired[0]["host"], retired) and len(graphed._tables.retired) == 1


@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_plain_hip_adamw_refuses_capture_before_any_launch():
    ps = _params()
    opt = HipAdamW(_groups(ps), **HYPER)
    _set_grads(ps, 0)
    opt.clip_and_step(1.0)
    torch.cuda.synchronize(DEV)
    bits = _state_bits(opt, ps)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="capturable=True"):
        with torch.cuda.graph(graph, stream=side):
            opt.clip_and_step(1.0)
    torch.cuda.synchronize(DEV)
    assert not torch.cuda.is_current_stream_capturing()
    _same_bits(bits, _state_bits(opt, ps), "nothing was launched")
    assert all(float(opt.state[p]["step"]) == 1.0 for p in ps)
    opt.clip_and_step(1.0)                  # and the optimizer still works
    torch.cuda.synchronize(DEV)
    assert all(float(opt.state[p]["step"]) == 2.0 for p in ps)


# ------------------------------------------------------------------------------------------------------ the towers' training step
SHAPES, COUNTS = [(4, 16, 16), (8, 32, 48), (4, 8, 24)], [2, 5, 3]
SCHEDULE = dict(warmup_steps=2, training_steps=8, base_lr=1e-3, end_lr=1e-4)


def _model():
    from titok_video_amd.model.titok import TiTok
    from titok_video_amd.synthetic import seeded_titok_state
    cfg = SimpleNamespace(tokenizer=SimpleNamespace(model=SimpleNamespace(patch_size=[4, 8, 8], fsq_levels=[7, 5, 5, 5, 5], encoder_size="tiny",
                                                                          decoder_size="tiny")))
    m = TiTok(cfg)
    m.load_state_dict(seeded_titok_state(0), strict=True)
    return m.to(DEV).train()          # fp32 master weights, bf16 compute


def test_graphed_training_step_with_the_hip_optimizer_and_schedule():
    from titok_video_amd.synthetic import synthetic_clips
    from titok_video_amd.train import GraphedTrainingStep, make_optimizer, training_step
    clips = synthetic_clips(SHAPES, seed=31, dtype=torch.bfloat16, device=DEV)
    eager, graphed = _model(), _model()
    opt_e, sched_e = make_optimizer(eager, lr=1e-3, hip_capturable=True, schedule=SCHEDULE)
    opt_g, sched_g = make_optimizer(graphed, lr=1e-3, hip_capturable=True, schedule=SCHEDULE)
    assert type(opt_g) is HipAdamW and opt_g.capturable and sched_g.on_device
    step = GraphedTrainingStep(graphed, opt_g, clips, COUNTS)
    assert opt_g.applied_updates() == 0
    for (n, p), (_, q) in zip(eager.named_parameters(), graphed.named_parameters()):
        assert torch.equal(p, q), n                                   # the capture's warm-up steps were undone
    losses = []
    for u in range(4):
        le, _, ie = training_step(eager, clips, COUNTS, opt_e)
        lg, _, ig = step(clips)
        losses.append((float(le), float(lg)))
        assert torch.equal(ie, ig)
        assert _bits_of(opt_e.last_lr()) == _bits_of(opt_g.last_lr()) and float(opt_g.last_lr()) == f32(cosine_warmup_lr(u, **SCHEDULE)), u
    for le, lg in losses:
        assert abs(le - lg) < 2e-3 * abs(le), losses
    assert opt_g.applied_updates() == opt_e.applied_updates() == 4 and sched_g.last_epoch == 4
    for (n, p), (_, q) in zip(eager.named_parameters(), graphed.named_parameters()):
        assert float((p - q).detach().abs().max()) < 2e-3 * max(1.0, float(p.detach().abs().max())), n


def test_resume_of_a_training_run_through_a_checkpoint(tmp_path):
    from titok_video_amd.checkpoint import load_checkpoint, save_checkpoint
    from titok_video_amd.ema import WeightEMA
    from titok_video_amd.synthetic import synthetic_clips
    from titok_video_amd.train import make_optimizer, training_step
    clips = synthetic_clips(SHAPES, seed=31, dtype=torch.bfloat16, device=DEV)
    model = _model()
    opt, sched = make_optimizer(model, lr=1e-3, hip_capturable=True, skip_nonfinite=True, schedule=SCHEDULE)
    ema = WeightEMA(model, decay=0.99)
    for _ in range(3):
        training_step(model, clips, COUNTS, opt)
        ema.update()
    path = str(tmp_path / "resume.pt")
    save_checkpoint(path, model, global_step=3, ema=ema, optimizers=[opt], schedulers=[sched])

    model2 = _model()
    with torch.no_grad():
        for p in model2.parameters():
            p.mul_(0.5)
    opt2, sched2 = make_optimizer(model2, lr=1e-3, hip_capturable=True, skip_nonfinite=True, schedule=SCHEDULE)
    ema2 = WeightEMA(model2, decay=0.5)
    assert load_checkpoint(path, model2, strict=True, ema=ema2, optimizers=[opt2], schedulers=[sched2]) == 3
    for (n, p), (_, q) in zip(model.named_parameters(), model2.named_parameters()):
        assert torch.equal(p, q), n
    sa, sb = opt.state_dict(), opt2.state_dict()
    assert sa["state"].keys() == sb["state"].keys() and len(sa["state"]) > 0
    for k in sa["state"]:
        assert float(sa["state"][k]["step"]) == float(sb["state"][k]["step"]) == 3.0
        for name in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(sa["state"][k][name], sb["state"][k][name]), (k, name)
    a, b = opt.device_block(), opt2.device_block()
    for key in ("updates", "skipped", "schedule_index", "lr", "bc1", "bc2_sqrt"):
        assert a[key] == b[key], key
    assert b["updates"] == 3 and b["skipped"] == 0 and b["schedule_index"] == 2
    assert sched2.last_epoch == sched.last_epoch == 3 and sched2.get_last_lr() == sched.get_last_lr()
    assert ema2.num_updates == ema.num_updates == 3 and ema2.decay == ema.decay
    for k in ema.shadow:
        assert torch.equal(ema.shadow[k], ema2.shadow[k]), k
    training_step(model2, clips, COUNTS, opt2)
    blk = opt2.device_block()
    assert blk["updates"] == 4 and blk["schedule_index"] == 3 and blk["lr"] == f32(cosine_warmup_lr(3, **SCHEDULE))
    assert blk["bc1"] == f32(1.0 - 0.5 ** 4.0) and blk["bc2_sqrt"] == f32(math.sqrt(1.0 - 0.96 ** 4.0))


def test_six_straight_equals_three_save_load_three(tmp_path):
    """Gradients fed by hand in place of the towers: the resumed optimization is the straight one, bit for bit."""
    from titok_video_amd.checkpoint import load_checkpoint, save_checkpoint

    class Holder(torch.nn.Module):
        def __init__(self, ps):
            super().__init__()
            self.ps = torch.nn.ParameterList(ps)

    def build():
        ps = _params()
        opt = HipAdamW(_groups(ps), capturable=True, skip_nonfinite=True, **HYPER)
        return ps, opt, CosineWarmupLR(opt, **SMALL), Holder(ps)

    ps, opt, sched, _ = build()
    for u in range(6):
        _set_grads(ps, u)
        opt.clip_and_step(1.0)
    qs, opt_a, sched_a, holder_a = build()
    for u in range(3):
        _set_grads(qs, u)
        opt_a.clip_and_step(1.0)
    path = str(tmp_path / "three.pt")
    save_checkpoint(path, holder_a, global_step=3, optimizers=[opt_a], schedulers=[sched_a])
    rs, opt_b, sched_b, holder_b = build()
    assert load_checkpoint(path, holder_b, strict=True, optimizers=[opt_b], schedulers=[sched_b]) == 3
    for p, (n, q) in zip(rs, holder_b.named_parameters()):
        assert p is q
    for u in range(3, 6):
        _set_grads(rs, u)
        opt_b.clip_and_step(1.0)
    _same_bits(_state_bits(opt, ps), _state_bits(opt_b, rs))
    assert opt_b.applied_updates() == 6 and _bits_of(opt_b.last_lr()) == _bits_of(opt.last_lr())


# ------------------------------------------------------------------------------------------------------ state dict
def test_state_dict_loads_into_torch_adamw_and_back():
    """Bounds of tests/test_hip_optim.py::test_state_dict_round_trip_with_torch_adamw (fp32, 2e-6 on the parameters)."""
    g = torch.Generator().manual_seed(3)
    shapes = [(256,), (1,), (64, 129), (8193,)]
    a = [torch.nn.Parameter((torch.randn(s, generator=g) * 0.5).to(DEV)) for s in shapes]
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    oa = HipAdamW(a, capturable=True, **HYPER)

    def grads(step):
        gg = torch.Generator().manual_seed(100 + step)
        return [(torch.randn(s, generator=gg) * 0.05).to(DEV) for s in shapes]
    for step in range(2):
        for p, gr in zip(a, grads(step)):
            p.grad = gr
        oa.step()
    for p, q in zip(a, b):
        q.data.copy_(p.data)
    ob = torch.optim.AdamW(b, foreach=False, fused=False, **HYPER)
    ob.load_state_dict(copy.deepcopy(oa.state_dict()))
    assert all(float(ob.state[q]["step"]) == 2.0 for q in b)
    for p, q, gr in zip(a, b, grads(2)):
        p.grad, q.grad = gr.clone(), gr.clone()
    oa.step(), ob.step()
    for p, q in zip(a, b):
        assert (p.detach() - q.detach()).abs().max().item() <= 2e-6
        assert float(ob.state[q]["step"]) == 3.0
    # and back: torch's dict (no 'skipped', its own extra group keys) into the device path
    oc = HipAdamW(a, skip_nonfinite=True, **HYPER)
    oc.load_state_dict(copy.deepcopy(ob.state_dict()))
    assert oc.applied_updates() == 3 and oc.skipped_steps() == 0
    # parameters of one group that disagree on `step`: the host path's error, at load time
    sd = copy.deepcopy(oa.state_dict())
    sd["state"][1]["step"] = torch.tensor(7.0)
    with pytest.raises(RuntimeError, match="different step counts"):
        HipAdamW(a, capturable=True, **HYPER).load_state_dict(sd)
