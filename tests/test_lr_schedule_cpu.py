"""The learning-rate schedule on the host (titok_video_amd/schedule.py) against the reference's recorded rates and torch's LambdaLR,
bit for bit, and the argument checks of the device-side entry points (they return before any launch: no GPU needed)."""
import ctypes as C
import math
import os
import warnings

import numpy as np
import pytest
import torch

from titok_video_amd import _lib
from titok_video_amd.schedule import CosineWarmupLR, cosine_warmup_lr, schedule_index

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lr_schedule_kat.npz")
LONG = [0, 1, 2, 999, 1000, 1001, 300500, 599999, 600000, 600001, 900000, 1200000]
SETS = {"gen": (1e-4, 1e-5, 1000, 600000, LONG), "disc": (1.5e-5, 1.5e-6, 1000, 600000, LONG),
        "nowarm": (1e-4, 0.0, 0, 10, list(range(25))), "allwarm": (3e-4, 1e-5, 5, 5, list(range(25)))}


@pytest.mark.parametrize("name", sorted(SETS))
def test_rates_equal_the_reference_scheduler_bit_for_bit(name):
    z = np.load(GOLDEN)
    base_lr, end_lr, warmup, total, indices = SETS[name]
    assert z[name + "_params"].tolist() == [base_lr, end_lr, warmup, total] and z[name + "_indices"].tolist() == indices
    for k, want in zip(indices, z[name + "_rates"].tolist()):
        got = cosine_warmup_lr(k, warmup, total, base_lr, end_lr)
        assert got == want and math.copysign(1.0, got) == math.copysign(1.0, want), (name, k, got, want)


def test_the_three_facts_of_the_reference_schedule():
    assert cosine_warmup_lr(0, 1000, 600000, 1e-4, 1e-5) == 0.0                      # the first update moves the moments only
    assert cosine_warmup_lr(900000, 1000, 600000, 1e-4, 1e-5) > cosine_warmup_lr(600000, 1000, 600000, 1e-4, 1e-5)      # the cosine goes on
    # base_lr is the formula's argument, the optimizer's initial lr the multiplier
    assert cosine_warmup_lr(500, 1000, 600000, 1e-4, 1e-5, initial_lr=2e-4) == 2e-4 * (500.0 / 1000.0)
    assert cosine_warmup_lr(1000, 1000, 600000, 1e-4, 1e-5, initial_lr=3.0) == 3.0 * ((1e-5 + (1e-4 - 1e-5) * 1.0) / 1e-4)


def _lambda(warmup, total, base_lr, end_lr, cycles=0.5):
    def fn(step):          # the schedule's definition, written out once more for torch's LambdaLR
        if step < warmup:
            return float(step) / float(max(1, warmup))
        progress = float(step - warmup) / float(max(1, total - warmup))
        ratio = max(0.0, 0.5 * (1.0 + math.cos(math.pi * float(cycles) * 2.0 * progress)))
        return (end_lr + (base_lr - end_lr) * ratio) / base_lr
    return fn


@pytest.mark.parametrize("params", [(1e-3, 1e-4, 4, 12), (1e-4, 1e-5, 1000, 600000), (1e-4, 0.0, 0, 10)])
def test_against_torch_lambdalr(params):
    base_lr, end_lr, warmup, total = params
    mine = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=base_lr)
    theirs = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=base_lr)
    a = CosineWarmupLR(mine, warmup, total, base_lr, end_lr)
    b = torch.optim.lr_scheduler.LambdaLR(theirs, _lambda(warmup, total, base_lr, end_lr))
    assert a.last_epoch == b.last_epoch == 0
    assert a.get_last_lr() == b.get_last_lr() and mine.param_groups[0]["lr"] == theirs.param_groups[0]["lr"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(30):
            mine.step(), theirs.step()
            a.step(), b.step()
            assert a.last_epoch == b.last_epoch
            assert a.get_last_lr() == b.get_last_lr() and mine.param_groups[0]["lr"] == theirs.param_groups[0]["lr"]
        for k in (0, 3, 4, 5, 11, 12, 13, 999, 1000, 1001, 600000, 5):
            a.step(k), b.step(k)
            assert a.last_epoch == b.last_epoch == k
            assert a.get_last_lr() == b.get_last_lr() and mine.param_groups[0]["lr"] == theirs.param_groups[0]["lr"]


def test_state_dict_round_trip():
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1e-3)
    a = CosineWarmupLR(opt, 4, 12, 1e-3, 1e-4, first=-1, stride=2)
    for _ in range(7):
        a.step()
    state = a.state_dict()
    assert state["last_epoch"] == 7 and state["_last_lr"] == a.get_last_lr()
    opt2 = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1e-3)
    b = CosineWarmupLR(opt2, 1, 2, 1e-3, 0.0)
    b.load_state_dict(state)
    assert b.last_epoch == 7 and b.get_last_lr() == a.get_last_lr() and opt2.param_groups[0]["lr"] == opt.param_groups[0]["lr"]
    assert b.state_dict() == state
    a.step(), b.step()
    assert b.get_last_lr() == a.get_last_lr() == [cosine_warmup_lr(15, 4, 12, 1e-3, 1e-4)]


def test_first_and_stride_give_lightnings_index_lists():
    assert [schedule_index(u, -1, 2) for u in range(4)] == [0, 1, 3, 5]          # the reference's generator beside a discriminator
    assert [schedule_index(u, 0, 2) for u in range(4)] == [0, 2, 4, 6]           # its discriminator
    assert [schedule_index(u) for u in range(4)] == [0, 1, 2, 3]
    for first, stride, want in ((-1, 2, [0, 1, 3, 5]), (0, 2, [0, 2, 4, 6])):
        opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1e-3)
        s = CosineWarmupLR(opt, 4, 12, 1e-3, 1e-4, first=first, stride=stride)
        seen = []
        for _ in want:
            seen.append(opt.param_groups[0]["lr"])
            s.step()
        assert seen == [cosine_warmup_lr(i, 4, 12, 1e-3, 1e-4) for i in want]
    with pytest.raises(ValueError):
        CosineWarmupLR(opt, 4, 3, 1e-3, 1e-4)
    with pytest.raises(ValueError):
        CosineWarmupLR(opt, 4, 12, 1e-3, 1e-4, stride=0)


# ---- the C ABI's refusals (include/titok_hip.h, ttv_opt_prepare / ttv_opt_adamw_step_dev): code 1, a message, no launch
@pytest.fixture(scope="module")
def handle():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


def _cosine(**kw):
    base = dict(kind=_lib.TTV_OPT_SCHEDULE_COSINE, warmup_steps=4, training_steps=12, base_lr=1e-3, end_lr=1e-4, num_cycles=0.5,
                initial_lr=1e-3, first=0, stride=1)
    base.update(kw)
    return _lib.OptSchedule(**base)


def test_struct_sizes_match_the_header():
    assert C.sizeof(_lib.OptState) == 48 and _lib.OptState.lr.offset == 28 and _lib.OptState.norm.offset == 44
    assert C.sizeof(_lib.OptSchedule) == 72 and _lib.OptSchedule.first.offset == 56


def test_prepare_refuses_bad_arguments_without_a_launch(handle):
    state = C.create_string_buffer(48)          # host memory: a launch would never be handed it - the calls return before one
    sp = C.addressof(state)
    part = C.addressof(C.create_string_buffer(16))
    none = _lib.OptSchedule(kind=_lib.TTV_OPT_SCHEDULE_NONE)
    cases = [((None, none, 0.9, 0.999, 1e-3, 0.0, None, 0, 0, None, None), b"null state"),
             ((sp, none, 0.9, 0.999, 1e-3, 1.0, None, 3, 0, None, None), b"null partials"),
             ((sp, none, 0.9, 0.999, 1e-3, 1.0, part, -1, 0, None, None), b"negative"),
             ((sp, _lib.OptSchedule(kind=7), 0.9, 0.999, 1e-3, 0.0, None, 0, 0, None, None), b"kind"),
             ((sp, _cosine(warmup_steps=13), 0.9, 0.999, 1e-3, 0.0, None, 0, 0, None, None), b"training_steps"),
             ((sp, _cosine(stride=0), 0.9, 0.999, 1e-3, 0.0, None, 0, 0, None, None), b"stride")]
    for args, word in cases:
        assert handle.ttv_opt_prepare(*args) == 1
        assert word in handle.ttv_error_string(), (word, handle.ttv_error_string())
    assert state.raw == b"\0" * 48


def test_step_dev_refuses_bad_arguments_without_a_launch(handle):
    sp = C.addressof(C.create_string_buffer(48))
    tab = C.addressof(C.create_string_buffer(40))
    hyper = (0.9, 0.999, 0.1, 0.001, 1e-8, 1e-2)
    assert handle.ttv_opt_adamw_step_dev(tab, tab, 1, _lib.TTV_F32, None, *hyper, None) == 1 and b"null state" in handle.ttv_error_string()
    assert handle.ttv_opt_adamw_step_dev(None, tab, 1, _lib.TTV_F32, sp, *hyper, None) == 1 and b"null buffer" in handle.ttv_error_string()
    assert handle.ttv_opt_adamw_step_dev(tab, None, 1, _lib.TTV_F32, sp, *hyper, None) == 1 and b"null buffer" in handle.ttv_error_string()
    assert handle.ttv_opt_adamw_step_dev(tab, tab, 1, 7, sp, *hyper, None) == 1 and b"dtype" in handle.ttv_error_string()
    assert handle.ttv_opt_adamw_step_dev(tab, tab, -1, _lib.TTV_F32, sp, *hyper, None) == 1
    assert handle.ttv_opt_adamw_step_dev(None, None, 0, _lib.TTV_F32, sp, *hyper, None) == 0          # nothing to do, nothing launched


def test_plain_hip_adamw_keeps_its_counters_on_the_host():
    from titok_video_amd.optim import HipAdamW
    p = torch.nn.Parameter(torch.ones(8))
    opt = HipAdamW([p], lr=1e-3)
    assert not opt.device_path and not opt.capturable
    with pytest.raises(RuntimeError, match="capturable=True"):
        opt.skipped_steps()
    assert set(opt.state_dict()["param_groups"][0]) == {"lr", "betas", "eps", "weight_decay", "params"}
    dev = HipAdamW([p], lr=1e-3, skip_nonfinite=True)
    assert dev.device_path and not dev.capturable
    assert dev.skipped_steps() == 0 and dev.applied_updates() == 0          # no block yet: zeros, and still no GPU needed
    assert dev.state_dict()["param_groups"][0]["skipped"] == 0
