"""Optimizer and scheduler state in checkpoints (titok_video_amd/checkpoint.py: Lightning's keys 'optimizer_states' and
'lr_schedulers'), with CPU modules and torch.optim.AdamW.  The HipAdamW device path through the same calls: tests/test_hip_optim_device_step.py."""
import torch

import pytest

from titok_video_amd.checkpoint import load_checkpoint, save_checkpoint
from titok_video_amd.schedule import CosineWarmupLR

SCHEDULE = dict(warmup_steps=4, training_steps=12, base_lr=1e-3, end_lr=1e-4)


def _setup(seed):
    torch.manual_seed(seed)
    model = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.Tanh(), torch.nn.Linear(7, 3))
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, betas=(0.5, 0.96), weight_decay=1e-4)
    return model, opt, CosineWarmupLR(opt, **SCHEDULE)


def _train(model, opt, sched, steps, seed):
    g = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        x = torch.randn(6, 5, generator=g)
        opt.zero_grad()
        model(x).square().mean().backward()
        opt.step()
        sched.step()


def _assert_same_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert sa["param_groups"] == sb["param_groups"]
    assert sa["state"].keys() == sb["state"].keys() and len(sa["state"]) == 4
    for k in sa["state"]:
        for name in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(sa["state"][k][name], sb["state"][k][name]), (k, name)


def test_round_trip_restores_optimizer_and_scheduler(tmp_path):
    model, opt, sched = _setup(0)
    _train(model, opt, sched, 3, seed=5)
    path = str(tmp_path / "ck.pt")
    save_checkpoint(path, model, global_step=3, optimizers=[opt], schedulers=[sched])
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert {"state_dict", "global_step", "optimizer_states", "lr_schedulers"} <= set(ck)
    assert len(ck["optimizer_states"]) == 1 and len(ck["lr_schedulers"]) == 1 and ck["lr_schedulers"][0]["last_epoch"] == 3
    assert all(v.device.type == "cpu" for st in ck["optimizer_states"][0]["state"].values() for v in st.values() if torch.is_tensor(v))

    model2, opt2, sched2 = _setup(1)
    assert load_checkpoint(path, model2, strict=True, optimizers=[opt2], schedulers=[sched2]) == 3
    _assert_same_state(opt, opt2)
    assert all(float(st["step"]) == 3.0 for st in opt2.state_dict()["state"].values())
    assert sched2.last_epoch == sched.last_epoch == 3 and sched2.get_last_lr() == sched.get_last_lr()
    assert opt2.param_groups[0]["lr"] == opt.param_groups[0]["lr"]
    # the resumed run continues the straight one bit for bit
    _train(model, opt, sched, 3, seed=6)
    _train(model2, opt2, sched2, 3, seed=6)
    for p, q in zip(model.parameters(), model2.parameters()):
        assert torch.equal(p, q)
    _assert_same_state(opt, opt2)


def test_file_without_the_keys_leaves_optimizer_and_scheduler_alone(tmp_path):
    model, opt, sched = _setup(0)
    _train(model, opt, sched, 2, seed=5)
    path = str(tmp_path / "old.pt")
    save_checkpoint(path, model, global_step=2)          # as written before the keys existed (and as the reference's init files are)
    assert set(torch.load(path, map_location="cpu", weights_only=False)) == {"state_dict", "global_step"}
    model2, opt2, sched2 = _setup(1)
    _train(model2, opt2, sched2, 1, seed=9)
    import copy
    before, before_s = copy.deepcopy(opt2.state_dict()), sched2.state_dict()
    assert load_checkpoint(path, model2, strict=True, optimizers=[opt2], schedulers=[sched2]) == 2
    after = opt2.state_dict()
    assert after["param_groups"] == before["param_groups"] and sched2.state_dict() == before_s
    for k in before["state"]:
        for name in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(after["state"][k][name], before["state"][k][name])
    for p, q in zip(model.parameters(), model2.parameters()):
        assert torch.equal(p, q)
    # and a file WITH the keys loads as before for a caller that passes neither list
    save_checkpoint(path, model, global_step=2, optimizers=[opt], schedulers=[sched])
    assert load_checkpoint(path, model2, strict=True) == 2
    assert sched2.state_dict() == before_s


def test_list_length_mismatch_raises(tmp_path):
    model, opt, sched = _setup(0)
    _train(model, opt, sched, 1, seed=5)
    path = str(tmp_path / "ck.pt")
    save_checkpoint(path, model, global_step=1, optimizers=[opt], schedulers=[sched])
    model2, opt2, sched2 = _setup(1)
    with pytest.raises(ValueError, match="optimizer_states"):
        load_checkpoint(path, model2, optimizers=[opt2, opt2], schedulers=[sched2])
    with pytest.raises(ValueError, match="lr_schedulers"):
        load_checkpoint(path, model2, optimizers=[opt2], schedulers=[])
    assert not opt2.state_dict()["state"]          # nothing was loaded
