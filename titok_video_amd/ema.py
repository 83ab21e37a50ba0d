"""Exponential moving average of the tokenizer's weights in fp32 shadow tensors (`ttv_opt_ema_update`, `ttv_opt_ema_exchange`;
kernels beside the optimizer's in csrc/ttv_optim.hip).

Not a reference module: the reference validates and saves its raw weights.  Tokenizer recipes in the VQGAN line evaluate and export
the average instead - with beta1 = 0.5 and a GAN term the raw weights move from step to step.  Built from eager `torch._foreach_*`
calls the average is a multi-launch stretch after every step, and it goes wrong quietly in two ways this module closes: a shadow kept
in bf16 never moves at decay 0.9999 (the increment is below half an ulp), and weights swapped in through `p.data.copy_` leave the
towers' weight packs and the L2 quantiser's lookup cache serving the old values (neither sees a write that does not bump the
parameter's version counter).

    ema = WeightEMA(model, decay=0.9999, warmup=True)   # shadows = exact fp32 copies of the parameters as they stand
    ... training_step(...) / gan_training_step(...)
    ema.update()                                        # after the optimizer step: one launch per parameter dtype
    with ema.applied():                                 # validation / export on the averaged weights
        recon, _ = model(clips, counts)                 # on leaving, the training weights are back bit for bit

Averaged: every floating-point entry of `model.named_parameters()`, trainable or not (the L2 quantiser's codebook in either of its
update modes).  Buffers are not averaged and stay as they are under `applied()`.  GPU only: like `HipAdamW` there is no host path for
`update()` / `applied()`; the schedule and the state-dict layout (`ShadowState`) are host code and work on any tensors.

Data parallelism: after the optimizer step the parameters are identical on every rank, so every rank's shadows are too.  No collective
is involved."""
from __future__ import annotations

import contextlib
from collections import OrderedDict

import torch

from . import _lib
from .optim import _CHUNK, _Tables


class ShadowState:
    """The host half of `WeightEMA`: which tensors are averaged, the decay schedule, the fp32 shadows and their state-dict layout.
    Device-agnostic (checkpoint code and its tests use it on CPU tensors); it never launches anything."""

    def __init__(self, model: torch.nn.Module, decay: float = 0.9999, warmup: bool = True):
        decay = float(decay)
        if not 0.0 <= decay <= 1.0:
            raise ValueError(f"WeightEMA: decay must lie in [0, 1], got {decay}")
        self.model, self.decay, self.warmup, self.num_updates = model, decay, bool(warmup), 0
        self._named = [(name, p) for name, p in model.named_parameters() if p.is_floating_point()]
        self.shadow = OrderedDict((name, p.detach().to(torch.float32, copy=True)) for name, p in self._named)      # widening: exact

    # -- schedule -------------------------------------------------------------------------------------------------------------------
    def decay_at(self, t: int) -> float:
        """The decay of update number t (t updates done so far), a Python double: min(decay, (1 + t) / (10 + t)) under warm-up -
        0.1 at the first update, so the start values are forgotten quickly - else decay."""
        if self.warmup:
            return min(self.decay, (1.0 + t) / (10.0 + t))
        return self.decay

    # -- state ----------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def reset(self) -> None:
        """Shadows = the parameters as they stand; num_updates = 0."""
        for name, p in self._named:
            self.shadow[name].copy_(p.detach())
        self.num_updates = 0

    def state_dict(self) -> dict:
        """{'decay', 'warmup', 'num_updates', 'shadow': OrderedDict(name -> fp32 tensor)}; the tensors are the live shadows, as a
        module's state_dict() hands out its parameters."""
        return {"decay": self.decay, "warmup": self.warmup, "num_updates": self.num_updates, "shadow": OrderedDict(self.shadow)}

    @torch.no_grad()
    def load_state_dict(self, state: dict) -> None:
        """Strict on names and shapes; the values are copied into the existing shadows (any device, any floating dtype - saved ones
        are fp32)."""
        shadow = state["shadow"]
        missing = [k for k in self.shadow if k not in shadow]
        unexpected = [k for k in shadow if k not in self.shadow]
        if missing or unexpected:
            raise KeyError(f"WeightEMA.load_state_dict: missing {missing}, unexpected {unexpected}")
        for k, s in self.shadow.items():
            if tuple(shadow[k].shape) != tuple(s.shape):
                raise ValueError(f"WeightEMA.load_state_dict: '{k}' has shape {tuple(shadow[k].shape)}, the parameter {tuple(s.shape)}")
        decay = float(state["decay"])
        if not 0.0 <= decay <= 1.0:
            raise ValueError(f"WeightEMA.load_state_dict: decay {decay}")
        for k, s in self.shadow.items():
            s.copy_(shadow[k])
        self.decay, self.warmup, self.num_updates = decay, bool(state["warmup"]), int(state["num_updates"])

    def model_state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        """The model's state_dict() with every averaged parameter replaced by its shadow cast to the parameter's dtype: same keys and
        order, buffers as they are - the inference checkpoint in the reference's format."""
        name_of = {id(p): name for name, p in self._named}
        sd = self.model.state_dict()
        for key, p in self.model.named_parameters(remove_duplicate=False):
            if key in sd and id(p) in name_of:
                sd[key] = self.shadow[name_of[id(p)]].to(p.dtype)
        return sd


class WeightEMA(ShadowState):
    """fp32 shadows of `model`'s parameters on the HIP kernels.  `update()` after the optimizer step, `applied()` around validation or
    export; `state_dict()` / `load_state_dict()` / `model_state_dict()` / `reset()` / `decay_at()` from `ShadowState`.

    All parameters on one GPU, contiguous, fp32 or bf16 (anything else raises here).  The parameter objects are held: a model whose
    parameters are replaced or cast afterwards needs a new instance."""

    def __init__(self, model: torch.nn.Module, decay: float = 0.9999, warmup: bool = True):
        named = [(name, p) for name, p in model.named_parameters() if p.is_floating_point()]
        if not named:
            raise ValueError("WeightEMA: the model has no floating-point parameters")
        for name, p in named:
            if not p.is_cuda:
                raise RuntimeError(f"WeightEMA: parameter '{name}' is on {p.device}; the EMA kernels run on the GPU only")
            if p.dtype not in (torch.float32, torch.bfloat16) or not p.is_contiguous() or p.numel() >= 1 << 31:
                raise RuntimeError(f"WeightEMA: parameter '{name}' ({p.dtype}, {tuple(p.shape)}): contiguous fp32 or bf16 tensors of fewer "
                                   "than 2^31 elements only")
        dev = named[0][1].device
        if any(p.device != dev for _, p in named):
            raise RuntimeError("WeightEMA: all parameters must live on one device")
        super().__init__(model, decay, warmup)
        self.device = dev
        # One entry table per dtype, built once: element counts and chunk lists here, the pointer columns in _sync_tables.
        by_dt = {}
        for name, p in self._named:
            by_dt.setdefault(p.dtype, []).append((name, p))
        self._buckets = list(by_dt.items())
        words, chunk_words, self._layout = [], [], []
        e_off = c_off = 0
        for dt, entries in self._buckets:
            c0 = c_off
            for i, (name, p) in enumerate(entries):
                words += [0, 0, 0, 0, p.numel()]
                for first in range(0, p.numel(), _CHUNK):
                    chunk_words.append(i | (first << 32))      # int2 {entry index within the bucket's table, first element}
                    c_off += 1
            self._layout.append((e_off, len(entries), c0, c_off - c0))
            e_off += len(entries)
        self._words, self._n_words, self._n_chunks = torch.tensor(words + chunk_words, dtype=torch.int64), len(words), c_off
        self._flat = [(name, p, p.dtype, p.numel()) for _, entries in self._buckets for name, p in entries]
        self._tables = _Tables(dev)
        self._slot = None
        self._uploaded = None          # (stream, pointer columns) of the table in self._slot
        self._backup = None            # name -> tensor like the parameter, allocated by the first applied()
        self._applied = False

    # -- tables ---------------------------------------------------------------------------------------------------------------------
    def _sync_tables(self, stream: int):
        """The device table with the pointers as they are NOW (a load_state_dict() or a .data assignment may have replaced a tensor),
        uploaded again only when one changed or the stream did (the copy is ordered on the stream that made it)."""
        ptrs = []
        for name, p, dt, n in self._flat:
            if p.dtype != dt or p.numel() != n or p.device != self.device or not p.is_contiguous():
                raise RuntimeError(f"WeightEMA: parameter '{name}' changed its dtype, size, device or layout after construction")
            ptrs += [p.data_ptr(), 0, self.shadow[name].data_ptr(), self._backup[name].data_ptr() if self._backup is not None else 0]
        if self._uploaded != (stream, ptrs):
            self._words[:self._n_words].view(-1, 5)[:, :4] = torch.tensor(ptrs, dtype=torch.int64).view(-1, 4)
            slot = self._tables.take(self._n_words // 5, self._n_chunks)
            total = self._words.numel()
            slot["host"][:total].copy_(self._words)
            slot["dev"][:total].copy_(slot["host"][:total], non_blocking=True)
            self._slot, self._uploaded = slot, (stream, ptrs)
        return self._slot["dev"].data_ptr()

    def _launch(self, call):
        """call(entry table, chunk list, chunks, dtype code, stream) once per dtype, on the current stream."""
        stream = _lib.stream_ptr(self.device)
        base = self._sync_tables(stream)
        chunks_base = base + 8 * self._n_words
        for (dt, _), (eo, ne, co, nc) in zip(self._buckets, self._layout):
            call(base + 40 * eo, chunks_base + 8 * co, nc, _lib.dtype_code(dt), stream)
        ev = self._slot["event"] or torch.cuda.Event()          # behind the kernels that read the slot: _Tables.take waits for it
        ev.record(torch.cuda.current_stream(self.device))
        self._slot["event"] = ev

    @staticmethod
    def _refuse_capture(what: str) -> None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"WeightEMA.{what}: the stream is capturing a graph; the weight and the pointer tables are host values "
                               "that a replay would repeat")

    # -- the average ----------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def update(self) -> None:
        """shadow += (1 - decay_t) (parameter - shadow), t = num_updates; then num_updates += 1.  1 - decay_t is formed in double and
        rounded to float once."""
        self._refuse_capture("update")
        if self._applied:
            raise RuntimeError("WeightEMA.update: inside applied() the parameters ARE the average")
        weight = 1.0 - self.decay_at(self.num_updates)
        lib = _lib.lib()
        self._launch(lambda tab, chunks, nc, code, stream: _lib.check(lib.ttv_opt_ema_update(tab, chunks, nc, code, weight, stream), "opt_ema_update"))
        self.num_updates += 1

    def reset(self) -> None:
        if self._applied:
            raise RuntimeError("WeightEMA.reset: inside applied() the parameters ARE the average")
        super().reset()

    # -- running the model on the average -----------------------------------------------------------------------------------------------
    def _exchange(self, mode: int) -> None:
        lib = _lib.lib()
        self._launch(lambda tab, chunks, nc, code, stream: _lib.check(lib.ttv_opt_ema_exchange(tab, chunks, nc, code, mode, stream), "opt_ema_exchange"))
        self._refresh_caches()

    def _refresh_caches(self) -> None:
        """The exchange writes behind autograd's back: whatever caches on a parameter's version counter is told."""
        for mod in self.model.modules():
            if hasattr(mod, "invalidate_packs"):
                mod.invalidate_packs()
            if hasattr(mod, "invalidate_lookup_cache"):
                mod.invalidate_lookup_cache()

    @contextlib.contextmanager
    def applied(self):
        """The model's parameters hold the average (cast to their dtype) inside the block and their own bits again after it, also
        when the block raises.  One launch per dtype each way; the backups are allocated by the first use and kept.  Not nestable."""
        if self._applied:
            raise RuntimeError("WeightEMA.applied: already applied (the block does not nest)")
        self._refuse_capture("applied")
        if self._backup is None:
            self._backup = {name: torch.empty_like(p) for name, p in self._named}
        self._exchange(0)
        self._applied = True
        try:
            yield self
        finally:
            self._exchange(1)
            self._applied = False
