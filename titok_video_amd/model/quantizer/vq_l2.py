"""Nearest-codebook-entry (L2) vector quantiser on the HIP path (csrc/ttv_vq.hip).

Not a reference module: the reference quantises with FSQ only (model/quantizer/fsq.py).  BASELINE.json's north_star / configs
#4, #5 name this formulation ("nearest-codebook-entry L2 distance + straight-through lookup", codebooks 8192x32 / 16384x64), so it
is provided with FSQ's call shape:  `codes, {'indices': int32}` = vq(z).  `FSQ.lattice_codebook()` gives the codebook on which this
quantiser reproduces FSQ's own indices (applied to `FSQ.bounded(z)`).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ... import _lib


UPDATES = ("grad", "ema")


class L2Quantizer(nn.Module):
    """codebook [N, C].  forward(z [rows, C]) -> (codes [rows, C] with straight-through gradient d codes / d z = I, {'indices': int32 [rows]}).

    With the defaults the codebook is a Parameter that learns from the decoder's token gradient alone (`_LookupFn`) and the module has
    no buffers.  Two opt-in pieces make it a trainable VQ layer (csrc/ttv_vq_train.hip; INTEGRATION.md has the update order):

    commitment_weight = beta > 0: info['commit_loss'] = mean (z - e)^2 (detached fp32 scalar, e the selected entries as the argmin read
        them) and the term's gradient beta 2 (z - e) / (rows C) is ADDED to z's gradient inside backward (gradient injection): the
        caller's loss stays what it was, a training step needs no edit, and the injected term does not follow a scaled loss.
    codebook_update = "ema": the codebook stops being a trainable parameter (requires_grad False) and is moved inside forward() - when
        self.training and grad mode is on - by an exponential moving average of per-entry counts and sums of z (`decay`, `eps`); entries
        whose moving count is below `dead_code_threshold` are redrawn from rows of this step's z (counter-based generator keyed by
        `seed`, the step and the entry).  fp32 buffers cluster_size [N] (zeros), embed_avg [N, C] (the codebook) and int64 ema_step [1]
        hold the state.  With the buffers at these initial values and a threshold > 0 the first step redraws every entry: that is the
        data-dependent initialisation.  A loaded state dict brings its own cluster_size.  Under torch.distributed the statistics are
        summed with one all-reduce of N (2 C + 1) floats (`process_group`; gloo goes through host memory)."""

    def __init__(self, codebook: torch.Tensor, commitment_weight: float = 0.0, codebook_update: str = "grad", decay: float = 0.99,
                 eps: float = 1e-5, dead_code_threshold: float = 0.0, seed: int = 0, process_group=None):
        super().__init__()
        if codebook.dim() != 2 or codebook.shape[1] > 64:
            raise ValueError("codebook must be [N, C] with C <= 64")
        if codebook_update not in UPDATES:
            raise ValueError(f"codebook_update must be one of {UPDATES}, got {codebook_update!r}")
        if not 0.0 < float(decay) < 1.0:
            raise ValueError(f"decay must lie strictly between 0 and 1, got {decay}")
        if float(commitment_weight) < 0.0 or float(dead_code_threshold) < 0.0:
            raise ValueError("commitment_weight and dead_code_threshold must not be negative")
        if not float(eps) > 0.0:
            # eps = 0 with an entry whose moving count is 0 (t = 0, never selected) makes smoothed 0 and the codebook row inf / NaN
            raise ValueError(f"eps must be positive, got {eps}")
        self.commitment_weight, self.codebook_update = float(commitment_weight), codebook_update
        self.decay, self.eps, self.dead_code_threshold = float(decay), float(eps), float(dead_code_threshold)
        self.seed, self.process_group = int(seed) & (2 ** 64 - 1), process_group
        ema = codebook_update == "ema"
        # "ema": an fp32 master that make_optimizer() leaves out; "grad": a trainable parameter in the dtype given
        self.codebook = nn.Parameter(codebook.detach().to(torch.float32 if ema else codebook.dtype).clone(), requires_grad=not ema)
        if ema:
            self.register_buffer("cluster_size", torch.zeros(codebook.shape[0], dtype=torch.float32))
            self.register_buffer("embed_avg", codebook.detach().to(torch.float32).clone())
            self.register_buffer("ema_step", torch.zeros(1, dtype=torch.int64))
        self._norms = None
        self._norms_key = None
        self._epoch = 0          # counts the in-place EMA updates, which do not bump codebook._version

    @property
    def codebook_size(self) -> int:
        return int(self.codebook.shape[0])

    @property
    def codebook_dim(self) -> int:
        return int(self.codebook.shape[1])

    def _cb_key(self, dtype):
        cb = self.codebook
        return (cb.data_ptr(), cb._version, self._epoch, dtype, str(cb.device))

    def _cb(self, dtype):
        cb = self.codebook.detach()
        key = self._cb_key(dtype)
        if self._norms_key != key:
            cbd = cb.to(dtype).contiguous()
            norms = torch.empty(cbd.shape[0], dtype=torch.float32, device=cbd.device)
            _lib.check(_lib.lib().ttv_vq_codebook_norms(cbd.data_ptr(), _lib.dtype_code(dtype), cbd.shape[1], cbd.shape[0], cbd.shape[1],
                                                        norms.data_ptr(), _lib.stream_ptr(cbd.device)), "ttv_vq_codebook_norms")
            self._norms, self._norms_key = (cbd, norms), key
        return self._norms

    def invalidate_lookup_cache(self) -> None:
        """Forget the compute-dtype copy of the codebook and its norms.  The key sees what bumps the codebook's version counter and this
        module's own EMA updates; code that writes the codebook any other way (a kernel, `.data`) calls this afterwards."""
        self._norms, self._norms_key = None, None

    @torch.no_grad()
    def indices(self, z: torch.Tensor, want_distance: bool = False):
        _lib.require_gpu(z, "L2Quantizer")
        if z.dim() != 2 or z.shape[1] != self.codebook_dim:
            raise ValueError(f"z must be [rows, {self.codebook_dim}]")
        z = z.contiguous()
        cbd, norms = self._cb(z.dtype)
        idx = torch.empty(z.shape[0], dtype=torch.int32, device=z.device)
        dist = torch.empty(z.shape[0], dtype=torch.float32, device=z.device) if want_distance else None
        ws = torch.empty(int(_lib.lib().ttv_vq_workspace_bytes(z.shape[0])) // 8, dtype=torch.int64, device=z.device)
        _lib.check(_lib.lib().ttv_vq_l2_argmin(z.data_ptr(), _lib.dtype_code(z.dtype), z.shape[1], cbd.data_ptr(), cbd.shape[1], norms.data_ptr(),
                                               z.shape[0], cbd.shape[0], cbd.shape[1], idx.data_ptr(), _lib.ptr(dist), ws.data_ptr(),
                                               ws.numel() * 8, _lib.stream_ptr(z.device)), "ttv_vq_l2_argmin")
        return (idx, dist) if want_distance else idx

    @torch.no_grad()
    def lookup(self, indices: torch.Tensor, dtype=None) -> torch.Tensor:
        dtype = dtype or self.codebook.dtype
        cbd, _ = self._cb(dtype)
        idx = indices.to(torch.int32).contiguous()
        out = torch.empty((idx.shape[0], cbd.shape[1]), dtype=dtype, device=idx.device)
        _lib.check(_lib.lib().ttv_vq_lookup(cbd.data_ptr(), _lib.dtype_code(dtype), cbd.shape[1], idx.data_ptr(), idx.shape[0], cbd.shape[1],
                                            out.data_ptr(), cbd.shape[1], _lib.stream_ptr(idx.device)), "ttv_vq_lookup")
        return out

    def forward(self, z: torch.Tensor):
        """Straight-through quantiser: VALUE codebook[idx]; gradient identity towards z (the reference's FSQ estimator, fsq.py:48-51)
        and, with codebook_update = "grad", through the lookup towards the codebook rows that were selected (scatter-add of the decoder's
        token gradient: `_LookupFn`).  commitment_weight and codebook_update = "ema" add what the class docstring says."""
        idx = self.indices(z.detach())
        info = {"indices": idx}
        grad, ema = torch.is_grad_enabled(), self.codebook_update == "ema"
        through = grad and (z.requires_grad or self.codebook.requires_grad)
        if through and not ema:
            q = _LookupFn.apply(self, idx, z.dtype, self.codebook)
        else:
            q = self.lookup(idx, z.dtype)
        z_seen = z.detach()
        if self.commitment_weight > 0.0:
            info["commit_loss"] = self._commit_loss(z_seen, idx)
            if grad and z.requires_grad and z.numel():
                z = _CommitFn.apply(z, q.detach(), 2.0 * self.commitment_weight / z.numel())
        codes = q + (z - z.detach()) if through and z.requires_grad else q
        if ema and self.training and grad and z_seen.shape[0]:
            self._ema_update(z_seen, idx)                 # after the lookup and the loss: both read the codebook the argmin read
        return codes, info

    # ---- commitment term / EMA update (csrc/ttv_vq_train.hip) ------------------------------------------------------------------------
    @staticmethod
    def _workspace(rows: int, n: int, device):
        nbytes = int(_lib.lib().ttv_vq_train_workspace_bytes(rows, n))
        return torch.empty(nbytes // 8, dtype=torch.int64, device=device), nbytes

    @torch.no_grad()
    def _commit_loss(self, z: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
        loss = torch.zeros((), dtype=torch.float32, device=z.device)
        if z.shape[0] == 0:
            return loss
        z = z.contiguous()
        cbd, _ = self._cb(z.dtype)
        ws, nbytes = self._workspace(z.shape[0], cbd.shape[0], z.device)
        _lib.check(_lib.lib().ttv_vq_commit_forward(z.data_ptr(), _lib.dtype_code(z.dtype), z.shape[1], cbd.data_ptr(), cbd.shape[1], idx.data_ptr(),
                                                    z.shape[0], cbd.shape[0], cbd.shape[1], loss.data_ptr(), ws.data_ptr(), nbytes,
                                                    _lib.stream_ptr(z.device)), "ttv_vq_commit_forward")
        return loss

    def _world(self):
        dist = torch.distributed
        if dist.is_available() and dist.is_initialized():
            return dist.get_rank(self.process_group), dist.get_world_size(self.process_group)
        return 0, 1

    def reduce_stats(self, stats: torch.Tensor) -> torch.Tensor:
        """Sum the flat fp32 buffer count | sum | cand [N (2 C + 1)] over the ranks, in place: ONE all-reduce per step (cand is zero
        except on the rank the draw named and `dead` is the same everywhere, so no second collective is needed).  gloo reduces host
        memory, the device backend the buffer itself, as CodebookLogger.get_scores does.  Single process: nothing to do."""
        if self._world()[1] == 1:
            return stats
        dist = torch.distributed
        if stats.is_cuda and dist.get_backend(self.process_group) == "gloo":
            host = stats.cpu()
            dist.all_reduce(host, op=dist.ReduceOp.SUM, group=self.process_group)
            stats.copy_(host)
        else:
            dist.all_reduce(stats, op=dist.ReduceOp.SUM, group=self.process_group)
        return stats

    @torch.no_grad()
    def _ema_update(self, z: torch.Tensor, idx: torch.Tensor) -> None:
        cb = self.codebook
        if any(t.dtype != torch.float32 for t in (cb, self.cluster_size, self.embed_avg)) or not cb.is_contiguous():
            raise RuntimeError("L2Quantizer: the EMA update keeps the codebook, cluster_size and embed_avg as contiguous fp32 masters "
                               "(run the towers in bf16 through the clips' dtype or autocast, not by casting the module)")
        z = z.contiguous()
        rows, n, c = z.shape[0], cb.shape[0], cb.shape[1]
        rank, world = self._world()
        # the summed count of an entry is at most the rows of all ranks <= world * (the most rows on any rank): if no rank trips this,
        # the sum is below 2^24 whatever the shards' sizes (conservative for unequal shards; no collective needed to check it)
        if rows * world >= 1 << 24:
            raise ValueError(f"L2Quantizer: {rows} rows on this rank x {world} ranks reaches 2^24: a per-entry count summed over ranks "
                             "must stay exact in fp32 (the guard takes this rank's rows for every rank)")
        cbd, norms = self._cb(z.dtype)                    # the compute-dtype copy and ||c||^2 the next argmin reads: refreshed by the kernel
        stats = torch.empty(n * (2 * c + 1), dtype=torch.float32, device=z.device)
        ws, nbytes = self._workspace(rows, n, z.device)
        lib, stream, thr = _lib.lib(), _lib.stream_ptr(z.device), self.dead_code_threshold
        _lib.check(lib.ttv_vq_ema_stats(z.data_ptr(), _lib.dtype_code(z.dtype), c, idx.data_ptr(), rows, n, c,
                                        self.cluster_size.data_ptr() if thr > 0.0 else 0, thr, self.seed, self.ema_step.data_ptr(), rank, world,
                                        stats.data_ptr(), ws.data_ptr(), nbytes, stream), "ttv_vq_ema_stats")
        self.reduce_stats(stats)
        _lib.check(lib.ttv_vq_ema_update(stats.data_ptr(), self.cluster_size.data_ptr(), self.embed_avg.data_ptr(), cb.data_ptr(), cbd.data_ptr(),
                                         _lib.dtype_code(z.dtype), norms.data_ptr(), self.ema_step.data_ptr(), n, c, self.decay, 1.0 - self.decay,
                                         self.eps, thr, ws.data_ptr(), nbytes, stream), "ttv_vq_ema_update")
        self._epoch += 1
        self._norms_key = self._cb_key(z.dtype)           # the cache holds the new codebook: re-keyed, not rebuilt


class _CommitFn(torch.autograd.Function):
    """Identity on z whose backward adds the commitment term's gradient: dz = g + scale (z - e) (ttv_vq_commit_backward)."""

    @staticmethod
    def forward(ctx, z: torch.Tensor, e: torch.Tensor, scale: float):
        ctx.z, ctx.e, ctx.scale = z.detach().contiguous(), e.contiguous(), float(scale)
        return z.view_as(z)

    @staticmethod
    def backward(ctx, g):
        z, e = ctx.z, ctx.e
        g = g.to(z.dtype).contiguous()
        dz = torch.empty_like(z)
        c = z.shape[1]
        _lib.check(_lib.lib().ttv_vq_commit_backward(g.data_ptr(), c, z.data_ptr(), c, e.data_ptr(), c, _lib.dtype_code(z.dtype), z.shape[0], c,
                                                     ctx.scale, dz.data_ptr(), c, _lib.stream_ptr(z.device)), "ttv_vq_commit_backward")
        return dz, None, None


class _LookupFn(torch.autograd.Function):
    """codes = codebook[idx] on the HIP path; backward = ttv_vq_lookup_backward (fp32 scatter-add into the codebook gradient)."""

    _det_scratch = None

    @staticmethod
    def forward(ctx, vq: "L2Quantizer", idx: torch.Tensor, dtype, codebook: torch.Tensor):
        ctx.idx, ctx.shape, ctx.cb_dtype = idx, tuple(codebook.shape), codebook.dtype
        return vq.lookup(idx, dtype)

    @staticmethod
    def backward(ctx, dcodes):
        dcodes = dcodes.contiguous()
        if dcodes.dtype not in (torch.float32, torch.bfloat16):
            dcodes = dcodes.float()
        dcb = torch.zeros(ctx.shape, dtype=torch.float32, device=dcodes.device)
        if _lib.is_deterministic():      # an owner per codebook entry adds its rows in ascending order
            need = _lib.lib().ttv_vq_lookup_backward_det_scratch_bytes(dcodes.shape[0], ctx.shape[0], dcodes.shape[1])
            if need < 0:
                _lib.check(1, "ttv_vq_lookup_backward_det_scratch_bytes")
            scratch = None              # the owner form has no partials (need == 0); a form with partials would take them from here
            if need > 0:
                if _LookupFn._det_scratch is None:
                    _LookupFn._det_scratch = _lib.DetScratch()
                scratch = _LookupFn._det_scratch.get(need, dcodes.device)
            _lib.check(_lib.lib().ttv_vq_lookup_backward_det(dcodes.data_ptr(), _lib.dtype_code(dcodes.dtype), dcodes.shape[1], ctx.idx.data_ptr(),
                                                             dcodes.shape[0], ctx.shape[0], dcodes.shape[1], dcb.data_ptr(), ctx.shape[1],
                                                             _lib.ptr(scratch), need, _lib.stream_ptr(dcodes.device)),
                       "ttv_vq_lookup_backward_det")
        else:
            _lib.check(_lib.lib().ttv_vq_lookup_backward(dcodes.data_ptr(), _lib.dtype_code(dcodes.dtype), dcodes.shape[1], ctx.idx.data_ptr(), dcodes.shape[0],
                                                         dcodes.shape[1], dcb.data_ptr(), ctx.shape[1], _lib.stream_ptr(dcodes.device)), "ttv_vq_lookup_backward")
        return None, None, None, dcb.to(ctx.cb_dtype)
