"""AdamW + gradient-norm clipping of the training loop as two HIP launches (`ttv_opt_grad_sumsq`, `ttv_opt_adamw_step`), or - opt-in,
`HipAdamW(capturable=True)` / `(skip_nonfinite=True)` - as three with the step count, bias corrections, learning rate (constant or
the reference's cosine schedule) and the skip decision formed on the device (`ttv_opt_prepare`, `ttv_opt_adamw_step_dev`).

The reference steps `torch.optim.AdamW` after `clip_gradients` (train.py:76-77, :183-190).  On MI355X torch's multi-tensor path costs
seven launches and ~230 us per step for the tiny tokenizer's 7 M parameters; `HipAdamW` keeps torch's interface, hyper-parameters and
state layout (`step`, `exp_avg`, `exp_avg_sq` per parameter: a `state_dict()` loads into `torch.optim.AdamW` and back) and does the
arithmetic in csrc/ttv_optim.hip.  GPU only: there is no host fallback (parameters on the CPU raise)."""
import math
import struct
from typing import Iterable, List, Optional

import torch

from . import _lib

_CHUNK = 8192          # OPT_CHUNK of csrc/ttv_optim.hip
_SLOTS = 4             # host / device table buffers in rotation: a slot is reused only after the step that read it has finished


class _Tables:
    """Pinned host + device buffers for the per-step pointer tables (gradients are fresh tensors every step, so the table is rebuilt and
    uploaded each time: ~4 KB).  A slot's event is recorded behind the kernels that read it and waited for before the slot is rewritten."""

    def __init__(self, device):
        self.device = device
        self.slots = []
        self.next = 0
        self.spare = None          # a slot no eager step uses: the one a stream capture takes (HipAdamW(capturable=True))
        self.retired = []          # slots a captured upload reads on every replay: never rewritten, alive as long as the optimizer

    @staticmethod
    def _new_slot(need: int, device):
        cap = max(need, 4096)
        return {"host": torch.empty(cap, dtype=torch.int64).pin_memory(), "dev": torch.empty(cap, dtype=torch.int64, device=device),
                "event": None}

    def provision_spare(self, n_entries: int, n_chunks: int, entry_words: int = 5):
        """Outside capture: make sure a capture finds a slot of this size without allocating, pinning or waiting."""
        need = n_entries * entry_words + n_chunks
        if self.spare is None or self.spare["host"].numel() < need:
            self.spare = self._new_slot(need, self.device)

    def take_for_capture(self, n_entries: int, n_chunks: int, entry_words: int = 5):
        """Under capture: the spare slot leaves the rotation for good (the replayed copy reads its pinned memory)."""
        need = n_entries * entry_words + n_chunks
        s = self.spare
        if s is None or s["host"].numel() < need:
            raise RuntimeError(HipAdamW._NO_WARMUP)
        self.spare = None
        self.retired.append(s)
        return s

    def take(self, n_entries: int, n_chunks: int, entry_words: int = 5):
        if len(self.slots) < _SLOTS:
            self.slots.append(None)
        i = self.next
        self.next = (self.next + 1) % _SLOTS
        need = n_entries * entry_words + n_chunks           # int64 words: 5 per optimizer entry, one per chunk (two int32)
        s = self.slots[i]
        if s is None or s["host"].numel() < need:
            s = self._new_slot(need, self.device)
            self.slots[i] = s
        elif s["event"] is not None:
            s["event"].synchronize()
        return s


class HipAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW (amsgrad=False, maximize=False) on the HIP kernels.  `step()` = AdamW; `clip_and_step(max_norm)` = clip_grad_norm_
    over every parameter of every group followed by AdamW, and returns the gradient norm (a device scalar, no synchronisation).  The clip
    factor is applied inside the update: `p.grad` keeps its unclipped values.

    capturable=True: the scalar state lives in a device block per group, so the step may be recorded into a HIP graph after one eager
    step (a plain HipAdamW raises under capture) and `schedule.CosineWarmupLR` runs on the device.  skip_nonfinite=True: a call whose
    gradient norm is NaN or infinite changes no parameter and no moment and is counted (`skipped_steps()`); the step count does not
    advance.  Either flag selects the device path; the arithmetic per element and the floats it uses are the host path's."""

    def __init__(self, params: Iterable, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 capturable: bool = False, skip_nonfinite: bool = False):
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1):
            raise ValueError("HipAdamW: invalid hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        # Either flag selects the device path (the `on_device` branch of `_run`): the update count, the bias corrections, the learning rate and the
        # skip decision live in one 48-byte block per group (include/titok_hip.h, ttv_opt_state).  Kept as attributes, not as group
        # keys: torch reads a group key `capturable` as "move `step` to the device" when a state dict is loaded.
        self.capturable, self.skip_nonfinite = bool(capturable), bool(skip_nonfinite)
        self.device_path = self.capturable or self.skip_nonfinite
        self._blocks = None               # int64 [groups, 6] on the device: one ttv_opt_state per row
        self._counters = None             # host rows (bytes) waiting for the block's first allocation (a state loaded before the first step)
        self._schedules = {}              # group index -> the dict CosineWarmupLR installed
        self._schedule_structs = {}       # the same as ttv_opt_schedule structs, built on first use
        self._tables = None
        self._partials = None
        self._norm = None
        self._static = {}
        self._param_norms = None          # (parameters, device norms) of the last norms launch

    # -- state ----------------------------------------------------------------------------------------------------------------------
    def _state_for(self, p):
        st = self.state[p]
        if not st:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    @staticmethod
    def _step_value(st) -> float:
        s = st["step"]
        return float(s.item()) if torch.is_tensor(s) else float(s)

    # -- the device block (device path) -------------------------------------------------------------------------------------------
    _DIFFERENT_STEPS = "HipAdamW: parameters of one group with different step counts are not supported"
    _NO_WARMUP = ("HipAdamW: stream capture without a warm-up step on the same parameters - run the step eagerly once first (it allocates "
                  "what a capture may not)")

    def _row(self, gi: int, updates: int, skipped: int) -> bytes:
        """One ttv_opt_state as bytes: the counters, and what the last applied update was formed with (the host's doubles rounded
        once, which is what the device writes: tests/test_hip_optim_device_step.py)."""
        index, lr, bc1, bc2s = 0, 0.0, 0.0, 0.0
        if updates > 0:
            g = self.param_groups[gi]
            b1, b2 = g["betas"]
            sch = self._schedules.get(gi)
            lr = float(g["lr"])
            if sch is not None:
                from .schedule import cosine_warmup_lr, schedule_index
                index = schedule_index(updates - 1, sch["first"], sch["stride"])
                lr = cosine_warmup_lr(index, sch["warmup_steps"], sch["training_steps"], sch["base_lr"], sch["end_lr"], sch["num_cycles"],
                                      sch["initial_lr"])
            bc1, bc2s = 1.0 - b1 ** float(updates), math.sqrt(1.0 - b2 ** float(updates))
        return struct.pack("<qqqifffff", updates, skipped, index, 0, lr, bc1, bc2s, 1.0, 0.0)

    def _write_counters(self, gi: int, updates: int, skipped: int) -> None:
        """In place: a captured graph holds the block's address."""
        row = self._row(gi, updates, skipped)
        if self._blocks is None or gi >= self._blocks.shape[0]:
            if self._counters is None:
                self._counters = {}
            self._counters[gi] = row
        else:
            self._blocks[gi].copy_(torch.frombuffer(bytearray(row), dtype=torch.int64))

    def _ensure_blocks(self, dev, capturing: bool) -> None:
        n = len(self.param_groups)
        if self._blocks is not None and self._blocks.device == dev and self._blocks.shape[0] == n:
            return
        if capturing:
            raise RuntimeError(self._NO_WARMUP)
        pending = self._counters or {}
        rows = [pending.get(gi) or self._row(gi, 0, 0) for gi in range(n)]
        fresh = torch.frombuffer(bytearray(b"".join(rows)), dtype=torch.int64).view(n, 6).to(dev)
        if self._blocks is not None:          # a group added after the first step, or parameters moved: the old rows keep their counts
            k = min(n, self._blocks.shape[0])
            fresh[:k].copy_(self._blocks[:k])
        self._blocks, self._counters = fresh, None

    def _read_blocks(self) -> torch.Tensor:
        """Every group's block on the host, int64 [groups, 6]: one device-to-host copy (synchronises)."""
        n = len(self.param_groups)
        if self._blocks is not None and self._blocks.shape[0] == n:
            return self._blocks.cpu()
        pending = self._counters or {}
        rows = [pending.get(gi) or self._row(gi, 0, 0) for gi in range(n)]
        host = torch.frombuffer(bytearray(b"".join(rows)), dtype=torch.int64).view(n, 6).clone()
        if self._blocks is not None:
            k = min(n, self._blocks.shape[0])
            host[:k].copy_(self._blocks[:k])
        return host

    def _require_device_path(self, what: str) -> None:
        if not self.device_path:
            raise RuntimeError(f"HipAdamW.{what}: the optimizer keeps its counters on the host - create it with capturable=True or skip_nonfinite=True")

    def applied_updates(self, group: int = 0) -> int:
        """Updates applied to parameter group `group` (synchronises).  Device path only."""
        self._require_device_path("applied_updates")
        return int(self._read_blocks()[group, 0])

    def skipped_steps(self, group: int = 0) -> int:
        """Calls dropped for a gradient norm that was NaN or infinite (`skip_nonfinite=True`; synchronises)."""
        self._require_device_path("skipped_steps")
        return int(self._read_blocks()[group, 1])

    def last_lr(self, group: int = 0) -> torch.Tensor:
        """The float32 learning rate of the last applied update of `group`: a device scalar, no synchronisation."""
        self._require_device_path("last_lr")
        if self._blocks is None:          # before the first step (a state was loaded, or nothing happened yet): the block is made now
            dev = self.param_groups[0]["params"][0].device
            if dev.type != "cuda":
                raise RuntimeError("HipAdamW.last_lr: parameter on " + str(dev) + "; the block lives on the GPU")
            self._ensure_blocks(dev, torch.cuda.is_current_stream_capturing())
        return self._blocks.view(torch.float32)[group, 7].clone()

    def device_block(self, group: int = 0) -> dict:
        """The fields of `group`'s ttv_opt_state on the host (synchronises); the floats as stored, widened."""
        self._require_device_path("device_block")
        row = self._read_blocks()[group]
        f, i = row.view(torch.float32), row.view(torch.int32)
        return {"updates": int(row[0]), "skipped": int(row[1]), "schedule_index": int(row[2]), "skip_now": int(i[6]), "lr": float(f[7]),
                "bc1": float(f[8]), "bc2_sqrt": float(f[9]), "clip_coef": float(f[10]), "norm": float(f[11])}

    def set_schedule(self, group: int, schedule: dict) -> None:
        """Install a learning-rate schedule for `group`'s device block: the keys of ttv_opt_schedule (schedule.CosineWarmupLR calls
        this).  From the next update on `ttv_opt_prepare` forms the rate from the update count."""
        self._require_device_path("set_schedule")
        self._schedules[group] = dict(schedule)
        self._schedule_structs = {}
        if self._blocks is not None or self._counters:          # the block's description of the last update follows the schedule
            row = self._read_blocks()[group]
            self._write_counters(group, int(row[0]), int(row[1]))

    def _schedule_struct(self, gi: int):
        structs = self._schedule_structs
        if gi not in structs:
            sch = self._schedules.get(gi)
            if sch is None:
                structs[gi] = _lib.OptSchedule(kind=_lib.TTV_OPT_SCHEDULE_NONE)
            else:
                structs[gi] = _lib.OptSchedule(kind=_lib.TTV_OPT_SCHEDULE_COSINE, warmup_steps=int(sch["warmup_steps"]),
                                               training_steps=int(sch["training_steps"]), base_lr=float(sch["base_lr"]), end_lr=float(sch["end_lr"]),
                                               num_cycles=float(sch["num_cycles"]), initial_lr=float(sch["initial_lr"]), first=int(sch["first"]),
                                               stride=int(sch["stride"]))
        return structs[gi]

    def state_dict(self):
        """torch's layout.  Device path: the counters are read with one copy and written into the per-parameter `step` entries, so the
        dict loads into `torch.optim.AdamW` and back; every group carries `skipped`."""
        if self.device_path:
            rows = self._read_blocks()
            for gi, g in enumerate(self.param_groups):
                g["skipped"] = int(rows[gi, 1])
                for p in g["params"]:
                    st = self.state.get(p)
                    if st:
                        st["step"] = torch.tensor(float(rows[gi, 0]), dtype=torch.float32)
        return super().state_dict()

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        if self.device_path:
            for gi, g in enumerate(self.param_groups):
                steps = {self._step_value(self.state[p]) for p in g["params"] if p in self.state and self.state[p]}
                if len(steps) > 1:
                    raise RuntimeError(self._DIFFERENT_STEPS)
                self._write_counters(gi, int(steps.pop()) if steps else 0, int(g.get("skipped", 0)))

    @torch.no_grad()
    def restore_in_place(self, saved_state_dict) -> None:
        """Put moments and counters back to `saved_state_dict` (a `state_dict()` of this optimizer) without replacing a tensor: every
        address a captured graph holds stays valid.  State that the saved dict does not have goes back to zero."""
        old = saved_state_dict["state"]
        for gi, (g, sg) in enumerate(zip(self.param_groups, saved_state_dict["param_groups"])):
            steps = set()
            for p, idx in zip(g["params"], sg["params"]):
                st, o = self.state.get(p), old.get(idx, {})
                if not st:
                    continue
                for k in ("exp_avg", "exp_avg_sq"):
                    if k in o:
                        st[k].copy_(o[k])
                    else:
                        st[k].zero_()
                step = self._step_value(o) if "step" in o else 0.0
                st["step"] = torch.tensor(step, dtype=torch.float32)
                steps.add(step)
            if len(steps) > 1:
                raise RuntimeError(self._DIFFERENT_STEPS)
            if self.device_path:
                self._write_counters(gi, int(steps.pop()) if steps else 0, int(sg.get("skipped", 0)))

    # -- the step -------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._run(None)
        return loss

    @torch.no_grad()
    def clip_and_step(self, max_norm: float, want_param_norms: bool = False) -> torch.Tensor:
        """want_param_norms=True: one more launch per (group, dtype) bucket (`ttv_opt_param_norms`) turns the per-chunk sums of squares
        the clip has just computed into one 2-norm per parameter, read with `last_param_norms()`.  The step itself - launches,
        arithmetic, return value - is the same with and without."""
        return self._run(float(max_norm), want_norms=want_param_norms)

    @torch.no_grad()
    def param_grad_norms(self):
        """`last_param_norms()` of the gradients as they stand, without stepping: `ttv_opt_grad_sumsq` + `ttv_opt_param_norms` per
        bucket.  For loops that do not clip (max_grad_norm falsy) and for modules that are not being stepped; creates no
        optimizer state."""
        self._run(None, want_norms=True, update=False)
        return self.last_param_norms()

    def last_param_norms(self):
        """(params, norms) of the last `clip_and_step(.., want_param_norms=True)` or `param_grad_norms()`: `params` the parameters
        that had a gradient, in parameter order (group by group, as `param_groups` lists them); `norms` a float32 device tensor of
        len(params) + B entries - the 2-norm of each parameter's gradient, then the 2-norm over each of the B (group, dtype)
        buckets (B = 1 for one group of one dtype).  No synchronisation, and no check that the gradients are still the ones the norms
        were taken from: that is the caller's knowledge.  The norm over ALL parameters is taken from the bucket
        norms in float64 on the host at read time: `HipAdamW.total_norm(norms.cpu()[len(params):])`.
        The gradients are the unclipped ones (`clip_and_step` scales in registers and leaves `p.grad` alone)."""
        if self._param_norms is None:
            raise RuntimeError("HipAdamW.last_param_norms: no norms yet - clip_and_step(max_norm, want_param_norms=True) or param_grad_norms()")
        return self._param_norms

    @staticmethod
    def total_norm(bucket_norms) -> float:
        """2-norm over all buckets from the bucket norms (host values), in float64."""
        return math.sqrt(sum(float(v) ** 2 for v in bucket_norms))

    def _run(self, max_norm: Optional[float], want_norms: bool = False, update: bool = True):
        # buckets: (group, dtype) -> parameters with a gradient
        buckets = []
        for g in self.param_groups:
            by_dt = {}
            for p in g["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda:
                    raise RuntimeError("HipAdamW: parameter on " + str(p.device) + "; the optimizer kernels run on the GPU only")
                if p.grad.is_sparse or p.grad.dtype != p.dtype or not p.is_contiguous() or not p.grad.is_contiguous():
                    raise RuntimeError("HipAdamW: dense contiguous gradients of the parameter's dtype only")
                by_dt.setdefault(p.dtype, []).append(p)
            for dt, ps in by_dt.items():
                buckets.append((g, dt, ps))
        clip = max_norm is not None
        if not buckets:
            if want_norms:
                self._param_norms = ([], torch.zeros(0, dtype=torch.float32, device="cuda"))
            return torch.zeros((), device="cuda") if clip else None
        dev = buckets[0][2][0].device
        if any(p.device != dev for _, _, ps in buckets for p in ps):
            raise RuntimeError("HipAdamW: all parameters must live on one device")
        capturing = torch.cuda.is_current_stream_capturing()
        if capturing and not self.capturable:
            # the host path hands the step count and both bias corrections to the kernel as arguments: a graph would replay them
            raise RuntimeError("HipAdamW: this step is being captured into a graph, and only HipAdamW(capturable=True) keeps its step count, "
                               "bias corrections and learning rate on the device; nothing was launched")
        on_device = update and self.device_path
        lib = _lib.lib()
        stream = _lib.stream_ptr(dev)
        if self._tables is None or self._tables.device != dev:
            self._tables = _Tables(dev)
            self._norm = torch.zeros(1, dtype=torch.float32, device=dev)
            self._static = {}
        # Host tables.  Element counts, chunk lists and offsets of a parameter list are built once; the pointers every step.
        if update:
            for _, _, ps in buckets:
                for p in ps:
                    self._state_for(p)
        key = tuple((id(g), dt, tuple((id(p), p.numel()) for p in ps)) for g, dt, ps in buckets)
        st = self._static.get(key)
        if st is None:
            words, chunk_words, layout = [], [], []
            e_off = c_off = 0
            for g, dt, ps in buckets:
                c0 = c_off
                for i, p in enumerate(ps):
                    words += [0, 0, 0, 0, p.numel()]
                    for first in range(0, p.numel(), _CHUNK):
                        chunk_words.append(i | (first << 32))      # int2 {entry index within the bucket's table, first element}
                        c_off += 1
                layout.append((e_off, len(ps), c0, c_off - c0))
                e_off += len(ps)
            # parameter order -> slot of the norms buffer (bucket b writes its entries and then its own total: e_off + b onwards)
            slot_of = {}
            for b, ((g, dt, ps), (eo, ne, _, _)) in enumerate(zip(buckets, layout)):
                for i, p in enumerate(ps):
                    slot_of[id(p)] = eo + b + i
            ordered = [p for g in self.param_groups for p in g["params"] if id(p) in slot_of]
            order = [slot_of[id(p)] for p in ordered] + [eo + b + ne for b, (eo, ne, _, _) in enumerate(layout)]
            st = {"words": torch.tensor(words + chunk_words, dtype=torch.int64), "n_words": len(words), "layout": layout, "n_chunks": c_off,
                  "ordered": ordered, "order": order, "order_dev": None}
            self._static = {key: st}          # one live parameter list at a time
        tmpl, n_words, layout, n_chunks = st["words"], st["n_words"], st["layout"], st["n_chunks"]
        # the four pointer columns are read afresh (a load_state_dict() or a .data assignment may have replaced a tensor)
        flat = [p for _, _, ps in buckets for p in ps]
        ptrs = []
        for p in flat:
            if not update:                # norms only: the kernels read the gradient column alone
                ptrs += [p.data_ptr(), p.grad.data_ptr(), 0, 0]
                continue
            sp = self.state[p]
            if sp["exp_avg"].dtype != p.dtype or sp["exp_avg"].device != p.device:          # a loaded state_dict: bring it to the parameter
                sp["exp_avg"] = sp["exp_avg"].to(device=p.device, dtype=p.dtype)
                sp["exp_avg_sq"] = sp["exp_avg_sq"].to(device=p.device, dtype=p.dtype)
            ptrs += [p.data_ptr(), p.grad.data_ptr(), sp["exp_avg"].data_ptr(), sp["exp_avg_sq"].data_ptr()]
        tmpl[:n_words].view(-1, 5)[:, :4] = torch.tensor(ptrs, dtype=torch.int64).view(-1, 4)
        if capturing:          # no allocation, no pinning, no event wait: all of it happened in an eager step
            if self._partials is None or self._partials.numel() < max(n_chunks, 1) or self._partials.device != dev:
                raise RuntimeError(self._NO_WARMUP)
            slot = self._tables.take_for_capture(n_words // 5, n_chunks)
        else:
            if self.capturable:
                self._tables.provision_spare(n_words // 5, n_chunks)
            slot = self._tables.take(n_words // 5, n_chunks)
        total = tmpl.numel()
        slot["host"][:total].copy_(tmpl)
        dev_buf = slot["dev"]
        dev_buf[:total].copy_(slot["host"][:total], non_blocking=True)
        base = dev_buf.data_ptr()
        chunks_base = base + 8 * n_words
        if self._partials is None or self._partials.numel() < max(n_chunks, 1) or self._partials.device != dev:
            self._partials = torch.empty(max(n_chunks, 1024), dtype=torch.float32, device=dev)
        use_norm = clip or (on_device and self.skip_nonfinite)
        if use_norm or want_norms:
            for (g, dt, ps), (eo, ne, co, nc) in zip(buckets, layout):
                _lib.check(lib.ttv_opt_grad_sumsq(base + 40 * eo, chunks_base + 8 * co, nc, _lib.dtype_code(dt),
                                                  self._partials.data_ptr() + 4 * co, stream), "opt_grad_sumsq")
        if want_norms:
            # a fresh buffer per call: the tensor handed out by last_param_norms() is never rewritten
            raw = torch.empty(n_words // 5 + len(layout), dtype=torch.float32, device=dev)
            for b, (eo, ne, co, nc) in enumerate(layout):
                _lib.check(lib.ttv_opt_param_norms(base + 40 * eo, chunks_base + 8 * co, nc, ne, self._partials.data_ptr() + 4 * co,
                                                   raw.data_ptr() + 4 * (eo + b), stream), "opt_param_norms")
            if st["order"] != list(range(raw.numel())):          # several buckets: parameter order, then the bucket norms
                if st["order_dev"] is None or st["order_dev"].device != dev:
                    st["order_dev"] = torch.tensor(st["order"], dtype=torch.int64, device=dev)
                raw = raw.index_select(0, st["order_dev"])
            self._param_norms = (st["ordered"], raw)
        if on_device:
            # one ttv_opt_prepare per group forms t, the bias corrections, the rate, the clip factor and the skip decision in the
            # group's block; the update kernels of the group's buckets read them there.  No host value depends on the step count.
            self._ensure_blocks(dev, capturing)
            group_index = {id(g): gi for gi, g in enumerate(self.param_groups)}
            flags = _lib.TTV_OPT_SKIP_NONFINITE if self.skip_nonfinite else 0
            prepared = set()
            for (g, dt, ps), (eo, ne, co, nc) in zip(buckets, layout):
                gi = group_index[id(g)]
                block = self._blocks.data_ptr() + 48 * gi
                b1, b2 = g["betas"]
                if gi not in prepared:
                    prepared.add(gi)
                    _lib.check(lib.ttv_opt_prepare(block, self._schedule_struct(gi), float(b1), float(b2), float(g["lr"]),
                                                   float(max_norm) if clip else 0.0, self._partials.data_ptr(), n_chunks if use_norm else 0,
                                                   flags, self._norm.data_ptr() if clip else None, stream), "opt_prepare")
                _lib.check(lib.ttv_opt_adamw_step_dev(base + 40 * eo, chunks_base + 8 * co, nc, _lib.dtype_code(dt), block, float(b1), float(b2),
                                                      1.0 - b1, 1.0 - b2, float(g["eps"]), float(g["weight_decay"]), stream),
                           "opt_adamw_step_dev")
        for (g, dt, ps), (eo, ne, co, nc) in zip(buckets, layout) if (update and not on_device) else ():
            # torch keeps a step count per parameter; they differ only when parameters join a group late, which this path does not support
            steps = {self._step_value(self.state[p]) for p in ps}
            if len(steps) != 1:
                raise RuntimeError(self._DIFFERENT_STEPS)
            t = steps.pop() + 1.0
            b1, b2 = g["betas"]
            _lib.check(lib.ttv_opt_adamw_step(base + 40 * eo, chunks_base + 8 * co, nc, _lib.dtype_code(dt), self._partials.data_ptr(),
                                              n_chunks if clip else 0, float(g["lr"]), float(b1), float(b2), 1.0 - b1, 1.0 - b2,
                                              float(g["eps"]), float(g["weight_decay"]), 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t),
                                              float(max_norm) if clip else 0.0, self._norm.data_ptr() if clip else None, stream),
                       "opt_adamw_step")
            for p in ps:          # one tensor PER parameter, as torch keeps them (its single-tensor step increments each in place)
                sp = self.state[p]
                if torch.is_tensor(sp["step"]) and sp["step"].device.type == "cpu":
                    sp["step"].fill_(t)
                else:
                    sp["step"] = torch.tensor(t, dtype=torch.float32)
        if update:
            # the kernels wrote the parameters behind autograd's back: whatever caches on a parameter's version counter (the towers'
            # weight packs, the L2 quantiser's norms) must see a new version.  A host-side counter: nothing is launched, and under
            # capture the warm-up steps bump it too, so the captured forward builds its packs inside the graph.
            torch.autograd.graph.increment_version(flat)
        if not capturing:          # a captured slot has left the rotation: nothing waits for it
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(dev))
            slot["event"] = ev
        return self._norm[0].clone() if clip else None


def use_hip_adamw(params: List[torch.nn.Parameter]) -> bool:
    """The HIP optimizer applies when every parameter is a dense tensor on one GPU."""
    return bool(params) and all(p.is_cuda for p in params) and len({p.device for p in params}) == 1
