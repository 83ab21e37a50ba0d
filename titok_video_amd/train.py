"""Generator training step on the HIP path (mirrors reference train.py:65-83 with the reconstruction term of
model/losses/loss_module.py:118: L1 between target and reconstruction, mean over clips of per-clip means).

    forward (tape) -> L1 loss -> backward (HIP kernels) -> [DP: count-weighted gradient all-reduce over RCCL]
    -> clip_grad_norm(max_grad_norm) -> optimizer.step()

`gan_training_step` adds the reference's discriminator step (train.py:86-107) on top of `model/losses/loss_module.py`'s
mirror; LPIPS is outside this path's scope (network-fetched weights).

Logging and validation (reference train.py:78-79, :102-103, :118-160): `grad_norm_dict` is the gradient-norm log from the sums the
optimizer's clip already takes, `recon_panels` the logged side-by-side videos as uint8 from one HIP launch and one device-to-host
copy, `ValidationLoop` the three validation hooks without a logger.  `make_weight_ema` builds the optional fp32 average of the generator's
weights (ema.py) that `ValidationLoop(..., ema=)` validates on.
"""
from __future__ import annotations

import math
import os
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import dp, switches
from .optim import HipAdamW, use_hip_adamw


class _L1LossFn(torch.autograd.Function):
    """Value and gradient of the L1 term for all clips in one HIP launch (ttv_l1_loss; in deterministic mode ttv_l1_loss_det with the
    scratch this class keeps for the block partials)."""

    _det_scratch = None

    @staticmethod
    def forward(ctx, n, *tensors):
        import ctypes as C
        from . import _lib
        recon = [t.contiguous() for t in tensors[:n]]
        target = [t.detach().to(recon[0].dtype).contiguous() for t in tensors[n:]]
        dev, dt = recon[0].device, recon[0].dtype
        loss = torch.zeros((), dtype=torch.float32, device=dev)
        grads = [torch.empty_like(r) for r in recon]
        sizes = (C.c_int32 * n)(*[int(r.numel()) for r in recon])
        if _lib.is_deterministic():
            need = _lib.lib().ttv_l1_loss_det_scratch_bytes(sizes, n)
            if need < 0:
                _lib.check(1, "ttv_l1_loss_det_scratch_bytes")
            if _L1LossFn._det_scratch is None:
                _L1LossFn._det_scratch = _lib.DetScratch()
            scratch = _L1LossFn._det_scratch.get(need, dev)
            _lib.check(_lib.lib().ttv_l1_loss_det(_lib.ptr_array(recon), _lib.ptr_array(target), _lib.ptr_array(grads), sizes, n,
                                                  _lib.dtype_code(dt), loss.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                                  _lib.stream_ptr(dev)), "ttv_l1_loss_det")
        else:
            _lib.check(_lib.lib().ttv_l1_loss(_lib.ptr_array(recon), _lib.ptr_array(target), _lib.ptr_array(grads), sizes, n,
                                              _lib.dtype_code(dt), loss.data_ptr(), _lib.stream_ptr(dev)), "ttv_l1_loss")
        ctx.grads, ctx.n = grads, n
        return loss

    @staticmethod
    def backward(ctx, gout):
        grads = ctx.grads
        torch._foreach_mul_(grads, gout.to(grads[0].dtype))
        return (None, *grads, *([None] * ctx.n))


def l1_reconstruction_loss(recon: Sequence[torch.Tensor], target: Sequence[torch.Tensor]) -> torch.Tensor:
    """Mean over clips of mean |target - recon| (loss_module.py:118 with per-clip tensors of different shapes).
    GPU tensors: one HIP kernel for value + gradient; CPU tensors (host-side tests of the DP logic): plain torch ops."""
    if recon[0].is_cuda:
        return _L1LossFn.apply(len(recon), *recon, *target)
    terms = [(r.float() - t.float()).abs().mean() for r, t in zip(recon, target)]
    return torch.stack(terms).mean()


def freeze_python_gc() -> None:
    """Host-side tuning for training loops (opt-in, process-wide): a full Python garbage collection walks every tracked
    object of the process (~170 k after importing torch: 15-25 ms on the GPU box) and the per-step allocations of an
    autograd step trigger one almost every step.  Freezing the objects that exist after set-up takes them out of the
    collector's view, so later collections only see what a step creates.  Measured: 29.5 -> 18 ms per training step."""
    import gc
    gc.collect()
    gc.freeze()


def host_cpu_share() -> int:
    """CPUs this process may actually use: the scheduler affinity, capped by the cgroup quota (a container sees every core of the
    host in os.cpu_count() - 256 on the GPU boxes - while its quota is 16)."""
    import os
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            with open(path) as f:
                parts = f.read().split()
            if path.endswith("cpu.max"):
                if parts[0] != "max":
                    n = min(n, max(1, int(parts[0]) // int(parts[1])))
            else:
                quota = int(parts[0])
                with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                    period = int(f.read())
                if quota > 0:
                    n = min(n, max(1, quota // period))
            break
        except (OSError, ValueError, IndexError):
            continue
    return max(1, n)


def limit_host_threads(max_threads: int = 4) -> int:
    """Host-side tuning for training loops (opt-in, process-wide): torch sizes its intra-op thread pool by os.cpu_count() (128
    threads on a GPU box whose cgroup grants 16 CPUs).  The first CPU-side tensor operation above the parallel grain size wakes
    the whole pool and its workers then spin between parallel regions: the autograd thread, the loader's upload thread and the HIP
    runtime's own threads are starved (measured on BASELINE config #3, tools/train_host_diag.sh: hipLaunchKernel 5 -> 20 us, a
    training step 8.1 -> 33-40 ms although the GPU work is 8 ms).  A training process has no CPU-side tensor work worth more
    than a few threads; returns the thread count set."""
    n = max(1, min(int(max_threads), host_cpu_share(), torch.get_num_threads()))
    torch.set_num_threads(n)
    return n


def _bump_versions(optimizer, args, kwargs) -> None:
    """Step post-hook of the torch AdamW `_make_adamw` builds.  torch's fused AdamW writes the parameters with one multi-tensor kernel
    and leaves their version counters where they were (its foreach and single-tensor forms bump them), like any kernel behind
    autograd's back: the towers' weight packs and the L2 quantiser's norms are keyed on the counters, so they are told here, whoever
    called `step()`.  A host-side counter: nothing is launched, also under capture."""
    torch.autograd.graph.increment_version([p for g in optimizer.param_groups for p in g["params"] if p.grad is not None])


def _make_adamw(params, lr, beta1, beta2, weight_decay, capturable, hip_capturable, skip_nonfinite, schedule):
    """The optimizer of make_optimizer / make_discriminator_optimizer; with `schedule` (a dict of schedule.CosineWarmupLR's
    arguments) the pair (optimizer, scheduler)."""
    device_path = hip_capturable or skip_nonfinite
    if device_path and not (use_hip_adamw(params) and switches.flag("TTV_HIP_ADAMW", True)):
        raise RuntimeError("make_optimizer: hip_capturable / skip_nonfinite are optim.HipAdamW's device path - parameters on one GPU and "
                           "TTV_HIP_ADAMW not switched off")
    # parameters on the GPU: clip + AdamW as two HIP launches (optim.HipAdamW; TTV_HIP_ADAMW=0 keeps torch's multi-tensor kernels, and
    # so does capturable=True - torch's capturable AdamW; hip_capturable=True is HipAdamW with its scalar state on the device)
    if use_hip_adamw(params) and (device_path or not capturable) and switches.flag("TTV_HIP_ADAMW", True):
        extra = dict(capturable=hip_capturable, skip_nonfinite=skip_nonfinite) if device_path else {}
        opt = HipAdamW(params, lr=lr, betas=(beta1, beta2), weight_decay=weight_decay, **extra)
    else:
        fused = bool(params) and all(p.is_cuda for p in params)      # one multi-tensor kernel instead of a launch per parameter
        opt = torch.optim.AdamW(params, lr=lr, betas=(beta1, beta2), weight_decay=weight_decay, fused=fused, capturable=capturable and fused)
        if fused:
            opt.register_step_post_hook(_bump_versions)
    if schedule is None:
        return opt
    from .schedule import CosineWarmupLR
    return opt, CosineWarmupLR(opt, **schedule)


def make_optimizer(model: torch.nn.Module, lr: float = 1e-4, beta1: float = 0.5, beta2: float = 0.96, weight_decay: float = 1e-4,
                   capturable: bool = False, hip_capturable: bool = False, skip_nonfinite: bool = False, schedule: Optional[dict] = None):
    """AdamW with the reference's hyper-parameters (configs/tiny.yaml:39-46, train.py:170-190).  capturable=True: torch's AdamW with
    the step counter on the device, so that the step can be recorded into a HIP graph (GraphedTrainingStep).  hip_capturable=True:
    `HipAdamW(capturable=True)`, which can be recorded too and runs a schedule on the device; skip_nonfinite=True: its
    skip-and-count of steps with a NaN or infinite gradient norm.  `schedule`: a dict of `schedule.CosineWarmupLR`'s arguments
    (warmup_steps, training_steps, base_lr, end_lr, optionally num_cycles, first, stride) - the call then returns
    (optimizer, scheduler); the reference: get_scheduler('cosine', .., warmup_steps=1000, max_steps=600000, base_lr, end_lr)."""
    params = [p for p in model.parameters() if p.requires_grad]
    return _make_adamw(params, lr, beta1, beta2, weight_decay, capturable, hip_capturable, skip_nonfinite, schedule)


def make_weight_ema(model: torch.nn.Module, config):
    """The weight average of `model` that `config.training.main` asks for, or None: `ema_decay` (absent or <= 0: no average) and
    `ema_warmup` (default True: decay_t = min(ema_decay, (1 + t) / (10 + t))).  Not reference keys: the reference keeps no average.
    Call `ema.update()` after every optimizer step and hand the instance to `ValidationLoop` and `save_checkpoint`."""
    from .ema import WeightEMA

    def key(node, name):          # attribute-style (OmegaConf, SimpleNamespace) and mapping-style nodes alike; absent or null -> None
        if node is None:
            return None
        return node.get(name) if isinstance(node, dict) else getattr(node, name, None)
    main = key(key(config, "training"), "main")
    decay = key(main, "ema_decay")
    if decay is None or not float(decay) > 0.0:
        return None
    warmup = key(main, "ema_warmup")
    return WeightEMA(model, decay=float(decay), warmup=True if warmup is None else bool(warmup))


def _param_list(module) -> list:
    """module.parameters() as a list, cached on the module: the generator walks the module tree on every call (~0.1 ms for the tokenizer)
    and a training step that is launch-bound at the reference's batch sizes walked it three times.  A training loop does not register
    parameters between steps; one that does deletes module._ttv_param_list."""
    cached = module.__dict__.get("_ttv_param_list")
    if cached is None:
        cached = list(module.parameters())
        module.__dict__["_ttv_param_list"] = cached
    return cached


def clip_and_step(optimizer, params, max_grad_norm):
    """clip_grad_norm_(params, max_grad_norm) (skipped when max_grad_norm is falsy) + optimizer.step(); returns the gradient norm or None.
    HipAdamW does both in its own two launches (the norm is taken over the optimizer's parameters that have a gradient - the same set)."""
    if isinstance(optimizer, HipAdamW):
        if max_grad_norm:
            return optimizer.clip_and_step(max_grad_norm)
        optimizer.step()
        return None
    gnorm = torch.nn.utils.clip_grad_norm_(params, max_grad_norm) if max_grad_norm else None
    optimizer.step()
    return gnorm


def _reducer_for(model, group, overlap: bool):
    """The dp.GradReducer of a model's towers (created on first use, cached on the model) when torch.distributed is active and the
    gradients live on a GPU; None otherwise (single process, or `overlap=False`: the sequential reference path)."""
    rank, ws = dp.world()
    if ws == 1 or not overlap:
        return None
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        return None
    red = model.__dict__.get("_dp_reducer")
    if red is None or red.group is not group:
        red = dp.GradReducer(dev, group)
        model.__dict__["_dp_reducer"] = red
    return red


def _towers(*modules):
    from .model.base.blocks import _Tower
    return [m for mod in modules for m in mod.modules() if isinstance(m, _Tower)]


def training_step(model, clips: List[torch.Tensor], token_counts, optimizer, max_grad_norm: float = 1.0,
                  target: Optional[List[torch.Tensor]] = None, group=None, overlap: bool = True):
    """One generator step on this rank's clips.  Returns (loss, grad_norm, indices).

    Under torch.distributed the gradients are reduced as sum(count * grad) / sum(count).  overlap=True (default): layer by layer
    on a communication stream while the backward is still running (dp.GradReducer); overlap=False: after the backward, in flat
    buckets (dp.allreduce_mean_by_count) - same values, kept as the reference for the overlapped path."""
    optimizer.zero_grad(set_to_none=True)
    red = _reducer_for(model, group, overlap)
    towers = _towers(model) if red is not None else []
    if red is not None:
        red.attach(*towers)
        red.begin_step(len(clips))
    try:
        recon, out = model(clips, token_counts)
        loss = l1_reconstruction_loss(recon, target if target is not None else clips)
        loss.backward()
    finally:
        if red is not None:
            red.detach(*towers)
    if red is not None:
        red.finish()                                   # joins the communication stream and delivers the towers' gradients
    params = [p for p in _param_list(model) if p.grad is not None]
    if red is not None:
        red.reduce_rest(params, len(clips))            # trainable parameters outside the towers (none in the reference's TiTok)
    else:
        dp.allreduce_mean_by_count([p.grad for p in params], len(clips), group=group)
    gnorm = clip_and_step(optimizer, params, max_grad_norm)
    return loss.detach(), gnorm, out["indices"]


class GraphedTrainingStep:
    """One generator training step (training_step: forward with tape, L1, backward, clip, AdamW) recorded ONCE into a HIP graph for a
    fixed batch shape and replayed per step ("HIP-graph capture of the training step").

    The tower entry points only enqueue kernels on the current stream (no allocation, no synchronisation inside the library) and the
    plans are built during the warm-up steps.  Every optimizer step bumps the parameters' version counters (HipAdamW behind its
    kernels, torch's fused AdamW through the step post-hook `_make_adamw` gives it), so the captured step starts from versions its towers have not seen: the weight packs
    and the backward's W^T copies it reads are rebuilt inside the capture, from the graph's own memory pool, and every replay
    rebuilds them from the weights the replay before it wrote - a replay is exact.  A replay runs no Python, so `__call__` bumps
    the versions itself afterwards: an eager forward of the model between replays (validation) builds its packs from the current
    weights.  Constraints: one batch shape per instance (clip
    shapes and token counts fixed; ragged token-budget batches need one instance per shape signature), an optimizer created with
    capturable=True (torch's AdamW) or hip_capturable=True (HipAdamW with its step count on the device), single process (the overlapped DP reducer launches collectives from Python callbacks).

    Measured (tools/bench_train.py GRAPH=1): the replay runs at the speed of the eager step, 3.48 ms at 5 clips and 8.1 ms at 32 -
    with the Python garbage collector frozen the host issues the ~300 launches of a step faster than the GPU runs them (3.6 ms of
    kernel time at 5 clips: the small kernels are latency-bound at ~12 us each), so on this stack a graph buys nothing; what would
    is fewer launches.  Kept as a tested utility for hosts that ARE issue-bound.

        step = GraphedTrainingStep(model, opt, example_clips, counts)
        loss, grad_norm, indices = step(clips)          # copies the clips into the graph's input buffers, replays"""

    def __init__(self, model, optimizer, example_clips, token_counts, max_grad_norm: float = 1.0, warmup: int = 3):
        import copy
        dev = next(model.parameters()).device
        self.model, self.optimizer, self.counts = model, optimizer, list(token_counts)
        self.inputs = [c.detach().clone() for c in example_clips]
        params = [p for p in model.parameters()]
        saved_params = [p.detach().clone() for p in params]
        saved_opt = copy.deepcopy(optimizer.state_dict())          # empty state for a fresh optimizer
        self.graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):                   # warm-up on the capture stream: plans, packs, optimizer state, allocator pool
            for _ in range(warmup):
                training_step(model, self.inputs, self.counts, optimizer, max_grad_norm, overlap=False)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        with torch.cuda.graph(self.graph, stream=side):
            self.loss, self.gnorm, self.indices = training_step(model, self.inputs, self.counts, optimizer, max_grad_norm, overlap=False)
        # the warm-up steps trained on the example batch: put parameters and optimizer state back IN PLACE (the graph holds their
        # addresses); a fresh optimizer goes back to zero moments and step 0
        with torch.no_grad():
            for p, q in zip(params, saved_params):
                p.copy_(q)
            old = saved_opt["state"]
            if isinstance(optimizer, HipAdamW):         # moments and the device block's counters (HipAdamW(capturable=True))
                optimizer.restore_in_place(saved_opt)
            for i, p in enumerate(optimizer.param_groups[0]["params"] if not isinstance(optimizer, HipAdamW) else ()):
                st = optimizer.state.get(p, {})
                for k, v in st.items():
                    if torch.is_tensor(v):
                        if i in old and k in old[i]:
                            v.copy_(old[i][k])
                        else:
                            v.zero_()
        # the packs the towers hold were made from the warm-up weights, inside the capture: dropping them here returns their memory
        # to the graph's private pool, which only this graph allocates from, so the replays keep reading and rewriting it safely
        for mod in model.modules():
            if hasattr(mod, "invalidate_packs"):
                mod.invalidate_packs()
        self._params = params

    def __call__(self, clips):
        torch._foreach_copy_(self.inputs, list(clips))
        self.graph.replay()
        torch.autograd.graph.increment_version(self._params)          # the replayed optimizer kernels moved them; Python is told here
        return self.loss, self.gnorm, self.indices


def make_discriminator_optimizer(loss_module: torch.nn.Module, lr: float = 1e-4, disc_lr_ratio: float = 0.15, beta1: float = 0.5,
                                 beta2: float = 0.96, weight_decay: float = 1e-4, hip_capturable: bool = False, skip_nonfinite: bool = False,
                                 schedule: Optional[dict] = None):
    """AdamW over `loss_module.disc_model` at lr * disc_lr_ratio (reference train.py:195-201, configs/tiny.yaml:46).  The three
    last arguments as make_optimizer's; the reference gives this schedule base_lr = lr * disc_lr_ratio and end_lr scaled alike."""
    params = list(loss_module.disc_model.parameters())
    return _make_adamw(params, lr * disc_lr_ratio, beta1, beta2, weight_decay, False, hip_capturable, skip_nonfinite, schedule)


def gan_training_step(model, loss_module, clips: List[torch.Tensor], token_counts, opt_g, opt_d=None, max_grad_norm: float = 1.0,
                      group=None, overlap: bool = True):
    """One generator step followed by one discriminator step on this rank's clips (reference train.py:64-107).

    generator:      recon = model(clips); loss = loss_module(target=clips, recon=recon)  [L1 + disc_weight * relativistic GAN term
                    through the frozen discriminator]; backward; clip; opt_g.step()
    discriminator:  loss_module(target=clips, recon=recon, disc_forward=True)  [both detached inside: relativistic loss + R1/R2
                    finite-difference penalty + centering]; backward; clip; opt_d.step()      (skipped when disc_weight == 0)
    Under torch.distributed both gradient sets are reduced as sum(count * grad) / sum(count), as in `training_step` (overlap=True:
    slice by slice behind the backward on a communication stream, dp.GradReducer).
    Returns the merged {'gen/..', 'disc/..'} dictionary of detached scalars and the token indices."""
    red = _reducer_for(model, group, overlap)
    g_towers = _towers(model) if red is not None else []
    d_towers = _towers(loss_module) if red is not None else []
    opt_g.zero_grad(set_to_none=True)
    if red is not None:
        red.attach(*g_towers)          # the discriminator's towers stay detached: frozen in this step, no gradients of their own
        red.begin_step(len(clips))
    try:
        recon, out = model(clips, token_counts)
        loss, loss_dict = loss_module(target=clips, recon=recon)
        loss.backward()
    finally:
        if red is not None:
            red.detach(*g_towers)
    if red is not None:
        red.finish()
    g_params = [p for p in _param_list(model) if p.grad is not None]
    if red is not None:
        red.reduce_rest(g_params, len(clips))
    else:
        dp.allreduce_mean_by_count([p.grad for p in g_params], len(clips), group=group)
    clip_and_step(opt_g, g_params, max_grad_norm)
    if opt_d is not None and getattr(loss_module, "disc_weight", 0.0) > 0.0:
        opt_d.zero_grad(set_to_none=True)
        if red is not None:
            red.attach(*d_towers)
            red.begin_step(len(clips))
        try:
            d_loss, d_dict = loss_module(target=clips, recon=recon, disc_forward=True)
            loss_dict.update(d_dict)
            d_loss.backward()
        finally:
            if red is not None:
                red.detach(*d_towers)
        if red is not None:
            red.finish()
        d_params = [p for p in _param_list(loss_module.disc_model) if p.grad is not None]
        if red is not None:
            red.reduce_rest(d_params, len(clips))
        else:
            dp.allreduce_mean_by_count([p.grad for p in d_params], len(clips), group=group)
        clip_and_step(opt_d, d_params, max_grad_norm)
    return loss_dict, out["indices"]


# ---- logging and validation (reference train.py:78-79, :102-103, :118-160) ------------------------------------------------------------
def grad_norm_dict(module: torch.nn.Module, optimizer: HipAdamW, norm_type=2, reuse: bool = False) -> dict:
    """What `lightning.pytorch.utilities.grad_norm(module, norm_type=2)` returns (reference train.py:78-79, :102-103), from
    `optimizer`'s kernels and ONE device-to-host copy.  Lightning 2.x defines it as
        norms = {f"grad_{float(norm_type)}_norm/{name}": p.grad.data.norm(norm_type)
                 for name, p in module.named_parameters() if p.grad is not None}
        if norms: norms[f"grad_{float(norm_type)}_norm_total"] = torch.tensor(list(norms.values())).norm(norm_type)
    so the keys are `grad_2.0_norm/<name>` in `named_parameters()` order plus `grad_2.0_norm_total`, the 2-norm of the listed norms;
    an empty dict when no parameter has a gradient.  Lightning is not installed where this package is built and tested: the
    definition above is restated from its source, not pinned by a fixture.  Values are Python floats; the total is taken in float64
    from the listed fp32 norms (Lightning takes it in fp32).
    The norms are taken here, by `optimizer.param_grad_norms()` (two launches per bucket, no step), unless the caller says
    `reuse=True`: then the norms of the optimizer's last `clip_and_step(max_norm, want_param_norms=True)` are read and nothing is
    launched - for the caller who has just made that step on these very gradients; nothing checks it.  They are norms of
    `p.grad` as stored: HipAdamW clips in registers, so after a clip the reference's log shows these values times
    min(1, max_norm / (total + 1e-6)).  Every parameter of `module` that has a gradient must belong to `optimizer`."""
    if float(norm_type) != 2.0:
        raise ValueError(f"grad_norm_dict: norm_type {norm_type!r}; the optimizer's kernels take 2-norms only")
    if not isinstance(optimizer, HipAdamW):
        raise TypeError("grad_norm_dict: the norms come from optim.HipAdamW's kernels; got " + type(optimizer).__name__)
    named = [(name, p) for name, p in module.named_parameters() if p.grad is not None]
    if not named:
        return {}
    params, norms = optimizer.last_param_norms() if reuse else optimizer.param_grad_norms()
    host = norms.cpu().tolist()          # the one copy (synchronises the stream)
    at = {id(p): i for i, p in enumerate(params)}
    out = {}
    for name, p in named:
        if id(p) not in at:
            raise RuntimeError(f"grad_norm_dict: parameter '{name}' has a gradient but does not belong to the optimizer")
        out[f"grad_2.0_norm/{name}"] = host[at[id(p)]]
    out["grad_2.0_norm_total"] = math.sqrt(sum(v * v for v in out.values()))
    return out


def recon_panels(target: Sequence[torch.Tensor], recon: Sequence[torch.Tensor]) -> List[np.ndarray]:
    """The logged videos of reference train.py:141-142, one per clip pair ([3,T,H,W] each, any shapes):
        torch.cat((y, x.clamp(-1, 1)), dim=-1).permute(1, 0, 2, 3).cpu().float().numpy();  ((v + 1) / 2 * 255).astype(np.uint8)
    as uint8 arrays [T,3,H,2W] - the target on the left, the clamped reconstruction on the right, bit for bit what the expression
    gives (include/titok_hip.h, ttv_recon_panels_u8; a target outside [-1, 1] saturates, NaN gives 0).  One HIP launch per 64 clips
    into one device buffer, one device-to-host copy of it into pinned memory (a quarter of the reference's fp32 bytes); the arrays
    are views of that host buffer.  bf16 or fp32 clips; a bf16 / fp32 pair is widened to fp32 as torch.cat would.  GPU only."""
    import ctypes as C
    from . import _lib
    if len(target) != len(recon):
        raise ValueError(f"recon_panels: {len(target)} targets, {len(recon)} reconstructions")
    if not len(recon):
        return []
    for y, x in zip(target, recon):
        _lib.require_gpu(x, "recon_panels")
        _lib.require_gpu(y, "recon_panels")
        if x.dim() != 4 or x.shape[0] != 3 or x.shape != y.shape:
            raise ValueError(f"recon_panels: clips must be [3,T,H,W] pairs of one shape, got {tuple(y.shape)} and {tuple(x.shape)}")
    dev = recon[0].device
    dt = recon[0].dtype if all(t.dtype == recon[0].dtype for t in list(recon) + list(target)) else torch.float32
    ys = [t.detach().to(dt).contiguous() for t in target]
    xs = [t.detach().to(dt).contiguous() for t in recon]
    sizes = [int(x.numel()) * 2 for x in xs]                     # bytes of a panel: T * 3 * H * 2W
    offsets, total = [], 0
    for n in sizes:
        offsets.append(total)
        total += (n + 15) // 16 * 16                              # every panel 16-byte aligned
    buf = torch.empty(total, dtype=torch.uint8, device=dev)
    dims = (C.c_int32 * (3 * len(xs)))(*[int(d) for x in xs for d in x.shape[1:]])
    outs = (C.c_void_p * len(xs))(*[buf.data_ptr() + o for o in offsets])
    _lib.check(_lib.lib().ttv_recon_panels_u8(_lib.ptr_array(ys), _lib.ptr_array(xs), dims, len(xs), _lib.dtype_code(dt), outs,
                                              _lib.stream_ptr(dev)), "ttv_recon_panels_u8")
    host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    host.copy_(buf, non_blocking=True)
    torch.cuda.current_stream(dev).synchronize()
    flat = host.numpy()
    return [flat[o:o + n].reshape(x.shape[1], 3, x.shape[2], 2 * x.shape[3]) for o, n, x in zip(offsets, sizes, xs)]


class ValidationLoop:
    """The validation hooks of the reference's TitokTrainer (train.py:118-160) without Lightning and without a logger:

        loop = ValidationLoop(model, eval_metrics, log_recon_num, eval_samples, random_recon, codebook_logger)
        loop.start()                                   # on_validation_epoch_start
        for batch in eval_loader:                      # {'video': clips, 'fps': .., 'token_counts': ..}
            for v in loop.step(batch):                 # validation_step
                logger.log_video(key=v["key"], videos=[v["video"]], fps=[v["fps"]], caption=[v["caption"]], format=["mp4"])
        logger.log_metrics(loop.end())                 # on_validation_epoch_end

    `start()` draws the logged clips: `torch.randperm(eval_samples)[:log_recon_num]` when `random_recon`, else the first
    `log_recon_num`; `seen_eval` and `seen_recon` go to zero.  `step()` runs the model and `eval_metrics.update(recon, orig)` under
    no_grad, then builds the panels of the selected clips of the batch with one `recon_panels` call; `seen_eval` counts every clip,
    selected or not, `seen_recon` numbers the logged ones from 1.  `end()` returns `eval_metrics.compute()` (then `reset()`),
    merged with the codebook scores when a logger is given and ready.

    `ema` (an `ema.WeightEMA` of `model`, default None): `start()` enters `ema.applied()` and `end()` leaves it, so every `step()` and
    every metric see the averaged weights and training resumes on the raw ones, bit for bit."""

    def __init__(self, model, eval_metrics, log_recon_num: int, eval_samples: int, random_recon: bool, codebook_logger=None, ema=None):
        self.model, self.eval_metrics, self.codebook_logger = model, eval_metrics, codebook_logger
        self.ema, self._ema_block = ema, None
        self.log_recon_num, self.eval_samples, self.random_recon = int(log_recon_num), int(eval_samples), bool(random_recon)
        self.recon_indexes: List[int] = []
        self.seen_eval = 0
        self.seen_recon = 0

    def start(self) -> None:
        if self.random_recon:
            self.recon_indexes = torch.randperm(self.eval_samples)[:self.log_recon_num].tolist()
        else:
            self.recon_indexes = list(range(self.log_recon_num))
        self.seen_eval = 0
        self.seen_recon = 0
        if self.ema is not None:
            self._ema_block = self.ema.applied()
            self._ema_block.__enter__()

    def step(self, batch) -> List[dict]:
        orig, fps, token_counts = batch["video"], batch["fps"], batch["token_counts"]
        with torch.no_grad():
            recon, _ = self.model(orig, token_counts)
            self.eval_metrics.update(recon, orig)
        picked = []
        for i in range(len(recon)):
            if self.seen_eval in self.recon_indexes:
                picked.append(i)
            self.seen_eval += 1
        if not picked:
            return []
        panels = recon_panels([orig[i] for i in picked], [recon[i] for i in picked])
        logged = []
        for i, video in zip(picked, panels):
            self.seen_recon += 1
            f, t = fps[i], token_counts[i]
            logged.append({"key": f"Video recon {self.seen_recon}", "video": video, "fps": f.item() if torch.is_tensor(f) else f,
                           "caption": f"{int(t)} tokens"})
        return logged

    def end(self) -> dict:
        try:
            metrics = dict(self.eval_metrics.compute())
        finally:
            if self._ema_block is not None:
                block, self._ema_block = self._ema_block, None
                block.__exit__(None, None, None)
        self.eval_metrics.reset()
        if self.codebook_logger is not None and self.codebook_logger.is_score_ready():
            metrics.update(self.codebook_logger.get_scores() or {})
        return metrics
