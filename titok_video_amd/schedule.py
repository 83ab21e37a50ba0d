"""The reference's learning-rate schedule: cosine with warm-up and a final rate (train_utils/lr_schedulers.py:30-63, used for both
optimizers at train.py:170-215 with warmup_steps=1000, max_steps=600000), on the host and - for `optim.HipAdamW(capturable=True)` - as
the parameters of the optimizer's device block (include/titok_hip.h, ttv_opt_schedule).

`cosine_warmup_lr` restates the reference's `lr_lambda` operation by operation in Python doubles and applies `LambdaLR`'s product, so
its value is the very double the reference's scheduler writes into `param_group['lr']` (tests/golden/lr_schedule_kat.npz).  Three
properties of the reference are kept as they are: with a warm-up the rate at index 0 is 0.0 (the first update moves the moments only);
past `training_steps` the cosine goes on and the rate climbs again; `base_lr` is the formula's argument while the optimizer's own
initial `lr` is the multiplier (the reference passes the same number for both).

Pure host code; the device evaluation lives in csrc/ttv_optim.hip (k_opt_prepare)."""
from __future__ import annotations

import math
from typing import List, Optional


def cosine_warmup_lr(index: int, warmup_steps: int, training_steps: int, base_lr: float, end_lr: float, num_cycles: float = 0.5,
                     initial_lr: Optional[float] = None) -> float:
    """`initial_lr * lr_lambda(index)` of the reference's get_cosine_schedule_with_warmup; `initial_lr` defaults to `base_lr`."""
    if index < warmup_steps:
        factor = float(index) / float(max(1, warmup_steps))
    else:
        progress = float(index - warmup_steps) / float(max(1, training_steps - warmup_steps))
        ratio = max(0.0, 0.5 * (1.0 + math.cos(math.pi * float(num_cycles) * 2.0 * progress)))
        factor = (end_lr + (base_lr - end_lr) * ratio) / base_lr
    return (base_lr if initial_lr is None else initial_lr) * factor


def schedule_index(update: int, first: int = 0, stride: int = 1) -> int:
    """The schedule index of update number `update` (counted from 0): max(0, first + stride * update)."""
    return max(0, first + stride * update)


class CosineWarmupLR:
    """The surface the reference uses from `LambdaLR` - `step(epoch=None)`, `get_last_lr()`, `last_epoch`, `state_dict()`,
    `load_state_dict()` - over `cosine_warmup_lr`.

    `last_epoch` counts the optimizer updates made so far; update number u runs at index max(0, first + stride * u).  The defaults
    (0, 1) are a run with one optimizer.  Lightning counts `global_step` per optimizer step, so with a discriminator the reference's
    generator sees the indices 0, 1, 3, 5, .. (first=-1, stride=2) and its discriminator 0, 2, 4, .. (first=0, stride=2).

    With a torch optimizer or a plain `HipAdamW` the rate is written into `group['lr']` at construction and by every `step()`, as
    `LambdaLR` does.  With a `HipAdamW(capturable=True)` the parameters are installed in the optimizer's device block once: the
    optimizer's own update count is the schedule's clock, `step()` has nothing to do, and `last_epoch` / `get_last_lr()` read the block
    (one device-to-host copy each)."""

    def __init__(self, optimizer, warmup_steps: int, training_steps: int, base_lr: float, end_lr: float, num_cycles: float = 0.5,
                 first: int = 0, stride: int = 1):
        if warmup_steps < 0 or training_steps < warmup_steps:
            raise ValueError(f"CosineWarmupLR: training_steps {training_steps} below warmup_steps {warmup_steps} (or a negative warm-up)")
        if stride < 1:
            raise ValueError(f"CosineWarmupLR: stride {stride} is below 1")
        self.optimizer = optimizer
        self.params = dict(warmup_steps=int(warmup_steps), training_steps=int(training_steps), base_lr=float(base_lr), end_lr=float(end_lr),
                           num_cycles=float(num_cycles))
        self.first, self.stride = int(first), int(stride)
        for g in optimizer.param_groups:          # LambdaLR: the multiplier is the group's rate at construction
            g.setdefault("initial_lr", g["lr"])
        self.base_lrs: List[float] = [g["initial_lr"] for g in optimizer.param_groups]
        self.on_device = bool(getattr(optimizer, "capturable", False)) and hasattr(optimizer, "set_schedule")
        self._last_epoch = 0
        self._install()

    def value(self, update: int, group: int = 0) -> float:
        """The rate of update number `update` for parameter group `group`, as a Python double."""
        return cosine_warmup_lr(schedule_index(update, self.first, self.stride), initial_lr=self.base_lrs[group], **self.params)

    def _install(self):
        if self.on_device:
            for i, lr0 in enumerate(self.base_lrs):
                self.optimizer.set_schedule(i, dict(self.params, initial_lr=lr0, first=self.first, stride=self.stride))
        else:
            self._last_lr = [self.value(self._last_epoch, i) for i in range(len(self.base_lrs))]
            for g, lr in zip(self.optimizer.param_groups, self._last_lr):
                g["lr"] = lr

    @property
    def last_epoch(self) -> int:
        return self.optimizer.applied_updates() if self.on_device else self._last_epoch

    def step(self, epoch: Optional[int] = None) -> None:
        if self.on_device:
            if epoch is not None:
                raise RuntimeError("CosineWarmupLR.step(epoch): the optimizer's device block holds the count; load an optimizer state to move it")
            return
        self._last_epoch = self._last_epoch + 1 if epoch is None else int(epoch)
        self._install()

    def get_last_lr(self) -> List[float]:
        """Host mode: the doubles in `group['lr']`.  Device mode: the float32 rates of the last applied update, widened (before the first
        update: the doubles the first one will round)."""
        if not self.on_device:
            return list(self._last_lr)
        if self.optimizer.applied_updates() == 0:
            return [self.value(0, i) for i in range(len(self.base_lrs))]
        return [float(self.optimizer.last_lr(i).item()) for i in range(len(self.base_lrs))]

    def state_dict(self) -> dict:
        return {"last_epoch": self.last_epoch, "base_lrs": list(self.base_lrs), "first": self.first, "stride": self.stride,
                "_last_lr": self.get_last_lr(), **self.params}

    def load_state_dict(self, state: dict) -> None:
        """Restores the schedule's parameters and, in host mode, the count.  In device mode the count comes back with the optimizer's
        own state; this call re-installs the parameters, so the order of the two loads does not matter."""
        for k in self.params:
            if k in state:
                self.params[k] = type(self.params[k])(state[k])
        self.first, self.stride = int(state.get("first", self.first)), int(state.get("stride", self.stride))
        self.base_lrs = list(state.get("base_lrs", self.base_lrs))
        self._last_epoch = int(state["last_epoch"])
        self._install()
