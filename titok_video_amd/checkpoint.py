"""Checkpoint compatibility with the reference trainer.

The reference saves Lightning checkpoints of `TitokTrainer` (train.py:28-37): a dict whose 'state_dict' holds the tokenizer under
`model.` and the discriminator under `loss_module.disc_model.`, with metric / LPIPS entries filtered out (train.py:218-220);
`init_from_checkpoint` loads it with strict=False (train.py:265-267).  The mirrors keep the reference's parameter names, so these
helpers only add / strip the trainer prefixes.  Pure host code (no GPU needed).
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Optional, Tuple

import torch

MODEL_PREFIX = "model."
LOSS_PREFIX = "loss_module."
_SKIP = ("eval_metrics", "perceptual_model")      # never saved by the reference (train.py:218-220)


def trainer_state_dict(model: torch.nn.Module, loss_module: Optional[torch.nn.Module] = None) -> "OrderedDict[str, torch.Tensor]":
    """What `TitokTrainer.state_dict()` returns for these two modules."""
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for k, v in model.state_dict().items():
        out[MODEL_PREFIX + k] = v
    if loss_module is not None:
        for k, v in loss_module.state_dict().items():
            if not any(s in k for s in _SKIP):
                out[LOSS_PREFIX + k] = v
    return out


def split_trainer_state_dict(state_dict: Dict[str, torch.Tensor]) -> Tuple[Dict[str, torch.Tensor], Dict[str, torch.Tensor]]:
    """(tokenizer entries, loss-module entries) with the trainer prefixes removed; metric / LPIPS entries dropped."""
    model_sd, loss_sd = OrderedDict(), OrderedDict()
    for k, v in state_dict.items():
        if any(s in k for s in _SKIP):
            continue
        if k.startswith(MODEL_PREFIX):
            model_sd[k[len(MODEL_PREFIX):]] = v
        elif k.startswith(LOSS_PREFIX):
            loss_sd[k[len(LOSS_PREFIX):]] = v
    return model_sd, loss_sd


def load_trainer_state_dict(state_dict: Dict[str, torch.Tensor], model: torch.nn.Module, loss_module: Optional[torch.nn.Module] = None,
                            strict: bool = True):
    """Load a reference trainer state dict into the mirrors.  A bare tokenizer state dict (no prefixes) is accepted too."""
    model_sd, loss_sd = split_trainer_state_dict(state_dict)
    if not model_sd and not loss_sd:
        model_sd = state_dict
    res = [model.load_state_dict(model_sd, strict=strict)]
    if loss_module is not None and (loss_sd or strict):
        res.append(loss_module.load_state_dict(loss_sd, strict=strict))
    return res


WEIGHT_EMA_KEY = "weight_ema"          # not a reference key: the reference ignores top-level entries it does not read
OPTIMIZER_KEY, SCHEDULER_KEY = "optimizer_states", "lr_schedulers"          # Lightning's keys: lists of state dicts


def _to_cpu(obj):
    """A state dict with every tensor detached and on the CPU (containers rebuilt, everything else as it is)."""
    if torch.is_tensor(obj):
        return obj.detach().cpu()
    if isinstance(obj, dict):
        return type(obj)((k, _to_cpu(v)) for k, v in obj.items())
    if isinstance(obj, (list, tuple)):
        return type(obj)(_to_cpu(v) for v in obj)
    return obj


def save_checkpoint(path: str, model: torch.nn.Module, loss_module: Optional[torch.nn.Module] = None, global_step: int = 0,
                    ema=None, optimizers=None, schedulers=None) -> None:
    """Write the subset of a Lightning checkpoint the reference reads back (train.py:265-267: ['state_dict'], 'global_step').
    `ema` (ema.WeightEMA / ema.ShadowState): its state_dict() goes under the top-level key 'weight_ema' as CPU tensors; 'state_dict'
    and 'global_step' are what they are without it.
    `optimizers`, `schedulers` (lists, in the training loop's order): their state_dict()s go under Lightning's keys
    'optimizer_states' and 'lr_schedulers' (what `ckpt_path=resume_path` restores, reference train.py:239-286), tensors on the CPU.
    Out of scope: the data order and the state of Python's / torch's random generators - a resumed run continues the optimization
    exactly and draws new batches."""
    sd = OrderedDict((k, v.detach().cpu()) for k, v in trainer_state_dict(model, loss_module).items())
    ck = {"state_dict": sd, "global_step": int(global_step)}
    if ema is not None:
        state = dict(ema.state_dict())
        state["shadow"] = OrderedDict((k, v.detach().cpu()) for k, v in state["shadow"].items())
        ck[WEIGHT_EMA_KEY] = state
    if optimizers is not None:
        ck[OPTIMIZER_KEY] = [_to_cpu(o.state_dict()) for o in optimizers]
    if schedulers is not None:
        ck[SCHEDULER_KEY] = [_to_cpu(s.state_dict()) for s in schedulers]
    torch.save(ck, path)


def load_checkpoint(path: str, model: torch.nn.Module, loss_module: Optional[torch.nn.Module] = None, strict: bool = False,
                    ema=None, optimizers=None, schedulers=None) -> int:
    """`init_from_checkpoint` (train.py:265-267; the reference loads with strict=False).  Returns the stored global step.
    `ema`: loads the file's 'weight_ema' entry (strict on names and shapes); a file without one - the reference's, or one saved without
    an average - restarts the average from the loaded weights (`ema.reset()`).
    `optimizers`, `schedulers`: restored from 'optimizer_states' / 'lr_schedulers' when given AND present; a file without the keys
    (the reference's init checkpoints, or one saved without them) leaves them as they are.  A list of another length than the
    file's raises ValueError before anything is loaded.  Data order and random-generator state are not restored (save_checkpoint)."""
    ck = torch.load(path, map_location="cpu", weights_only=False)
    for key, given in ((OPTIMIZER_KEY, optimizers), (SCHEDULER_KEY, schedulers)):
        if given is not None and key in ck and len(ck[key]) != len(given):
            raise ValueError(f"load_checkpoint: the file's '{key}' holds {len(ck[key])} entries, {len(given)} objects were given")
    load_trainer_state_dict(ck["state_dict"], model, loss_module, strict=strict)
    if ema is not None:
        if WEIGHT_EMA_KEY in ck:
            ema.load_state_dict(ck[WEIGHT_EMA_KEY])
        else:
            ema.reset()
    for key, given in ((OPTIMIZER_KEY, optimizers), (SCHEDULER_KEY, schedulers)):
        if given is not None and key in ck:
            for obj, state in zip(given, ck[key]):
                obj.load_state_dict(state)
    return int(ck.get("global_step", 0))
