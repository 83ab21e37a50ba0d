"""Mirror of the reference's `ReconstructionLoss` (model/losses/loss_module.py) for the L1 + GAN terms.

The discriminator is this package's `TiTokEncoder(out_channels=1)` called with K = 4 register tokens per clip
(loss_module.py:40-48,96-101): 6 of the 8 tower forwards of a reference training step are these calls, and the generator
step differentiates THROUGH the frozen discriminator into the reconstruction (loss_module.py:144-151) — both run on the HIP
path (tape forward + hand-written backward, input-clip gradients included).  Same constructor argument (the config tree),
same `forward(target, recon, disc_forward=False)` signature, same return value `(total_loss, {'gen/..' | 'disc/..': scalar})`
and the same state-dict keys (`disc_model.*`).

The LPIPS / Gram terms (loss_module.py:28-36,59-93,121-138) run on the HIP path too (model/metrics/lpips_gram.py).  Their weights
never come from the network: pass `perceptual_weights=` (a path or a state dict with the reference LPIPS keys) or set the config key
`tokenizer.losses.perceptual_weights` to a path; with neither, a non-zero `perceptual_weight` or `gram_weight` raises.  The module
sits under `perceptual_model` (never saved in trainer checkpoints, checkpoint.py).
"""
from __future__ import annotations

import random
from typing import List, Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import _lib, switches
from ..base.blocks import TiTokEncoder
from ..base.utils import init_weights
from ..metrics.lpips_gram import LPIPS
from ...optim import _Tables
from ...train import l1_reconstruction_loss


import os

_F32_HEAD = switches.flag("TTV_DISC_F32_HEAD", False)
_TWO_CALLS = switches.flag("TTV_DISC_TWO_CALLS", False)


def _resized_hw(H: int, W: int, size: int):
    """torchvision resize(size=int) output size: the short edge becomes `size`, the long edge int(size * long / short)."""
    short, long = (W, H) if W <= H else (H, W)
    new_short, new_long = size, int(size * long / short)
    return (new_long, new_short) if W <= H else (new_short, new_long)


def _fused_crops() -> bool:
    """TTV_LPIPS_CROPS=0 selects the eager crop path of `perceptual_preprocess` on GPU tensors too (A/B and tests)."""
    return switches.flag("TTV_LPIPS_CROPS", True)


def _fused_disc() -> bool:
    """TTV_DISC_FUSED=0 selects the eager noise and logit head of the discriminator step (and the eager g_loss of the generator
    step) on GPU tensors too (A/B and tests)."""
    return switches.flag("TTV_DISC_FUSED", True)


_GP_CHUNK = 8192       # GP_CHUNK of csrc/ttv_disc.hip
_HIP_DTYPES = (torch.bfloat16, torch.float32)


def gp_noise_layout(numels):
    """Where `ttv_gp_noise_add` puts the clips of a batch: (counter offsets, output offsets, padded output length, chunk words).
    A clip's counter offset is its element offset with the clips laid end to end, rounded up to a multiple of 4 (no Philox block
    straddles two clips); its output offset is rounded up to 8 elements, so that every per-clip view of the flat output is 16-byte
    aligned in both dtypes; a chunk word is (clip | first element << 32)."""
    ctr, out, chunks, c_at, o_at = [], [], [], 0, 0
    for i, n in enumerate(numels):
        if not 0 < n < 2 ** 31:
            raise ValueError(f"gp_noise_add: a clip of {n} elements (1 .. 2^31 - 1)")
        c_at = (c_at + 3) // 4 * 4
        o_at = (o_at + 7) // 8 * 8
        ctr.append(c_at)
        out.append(o_at)
        chunks += [i | (first << 32) for first in range(0, n, _GP_CHUNK)]
        c_at += n
        o_at += n
    return ctr, out, (o_at + 7) // 8 * 8, chunks


class DiscHead(torch.autograd.Function):
    """Per-token discriminator outputs -> loss terms and their gradient in one HIP launch (csrc/ttv_disc.hip, `ttv_disc_head`).
    `a` holds the groups (real, fake[, real + noise, fake + noise]) x n clips x R tokens, or their first half with `b` the second.
    Returns (total, terms): `terms` is the fp32 buffer [total, d_loss | g_loss, logits_relative, r1, r2, centering, 0, 0] of means
    over clips and is not differentiable; `total` is its element 0 and carries the gradient."""

    @staticmethod
    def forward(ctx, mode, n, R, gp_scale, centering_weight, a, b):
        parts = [a] if b is None else [a, b]
        for t in parts:
            _lib.require_gpu(t, "DiscHead")
            if t.dtype != a.dtype or not t.is_contiguous():
                raise ValueError("DiscHead: per-token outputs must be contiguous and of one dtype")
        count = sum(t.numel() for t in parts)
        G = count // (n * R)
        if G * n * R != count or (b is not None and a.numel() != b.numel()):
            raise ValueError(f"DiscHead: {count} per-token outputs are not groups x {n} clips x {R} tokens in two equal halves")
        terms = torch.empty(8, dtype=torch.float32, device=a.device)
        grad = torch.empty(count, dtype=torch.float32, device=a.device)
        _lib.check(_lib.lib().ttv_disc_head(a.data_ptr(), _lib.ptr(b), mode, G, n, R, _lib.dtype_code(a.dtype), gp_scale, centering_weight,
                                            terms.data_ptr(), grad.data_ptr(), _lib.stream_ptr(a.device)), "ttv_disc_head")
        ctx.save_for_backward(grad)
        ctx.parts = [(t.numel(), t.shape, t.dtype) for t in parts]
        ctx.mark_non_differentiable(terms)
        return terms[0], terms

    @staticmethod
    def backward(ctx, g, _g_terms):
        (grad,) = ctx.saved_tensors
        full = grad * g
        out, at = [], 0
        for k, (numel, shape, dtype) in enumerate(ctx.parts):
            out.append(full[at:at + numel].view(shape).to(dtype) if ctx.needs_input_grad[5 + k] else None)
            at += numel
        return (None,) * 5 + tuple(out) + (None,) * (2 - len(out))


def perceptual_crop_plan(frame_shapes, size: int, samples: int, resize_prob: float = 0.25):
    """The draws of the reference's perceptual_preprocess (loss_module.py:59-93) for frames of the given (H, W), consuming Python's
    `random` exactly as it does: one random() per frame for the shuffle (sorted(..., key=random.random())), then per taken frame a
    random() for the resize only when the frame is at least `size` on both edges, then randrange for the row and the column origin.
    The loop stops AFTER appending once i >= samples (24 -> 25 crops; -1 -> every frame).  Returns, in the order the crops are
    stacked, (frame index, H, W, Hr, Wr, oy, ox, resized): Hr x Wr is the frame the window is cut from (torchvision's resize(size):
    short edge -> size, long edge int(size * long / short)) and equals H x W when `resized` is False."""
    if samples == -1:
        samples = len(frame_shapes)
    plan = []
    for i, k in enumerate(sorted(range(len(frame_shapes)), key=lambda _k: random.random())):
        H, W = frame_shapes[k]
        resized = (H < size or W < size) or random.random() < resize_prob
        Hr, Wr = _resized_hw(H, W, size) if resized else (H, W)
        oy = random.randrange(0, (Hr - size) + 1)
        ox = random.randrange(0, (Wr - size) + 1)
        plan.append((k, H, W, Hr, Wr, oy, ox, resized))
        if i >= samples:
            break
    return plan


class PerceptualCrops(torch.autograd.Function):
    """The crops of a plan in one HIP launch (csrc/ttv_crops.hip) and their backward in one more.  `table` holds one
    (clip, frame, H, W, Hr, Wr, oy, ox) per crop; `clips` are the n reconstruction clips followed by the n target clips [3,T,H,W].
    Returns (recon crops, target crops) [F,3,size,size]; gradients flow into the reconstruction clips only."""

    @staticmethod
    def forward(ctx, table, size, n, *clips):
        recon, target = clips[:n], clips[n:]
        dev, dtype = recon[0].device, recon[0].dtype
        for c in clips:
            _lib.require_gpu(c, "PerceptualCrops")
            if c.dtype != dtype or c.dim() != 4 or c.shape[0] != 3 or not c.is_contiguous():
                raise ValueError(f"PerceptualCrops: clips must be contiguous [3,T,H,W] of one dtype, got {tuple(c.shape)} {c.dtype}")
        dt = _lib.dtype_code(dtype)
        dims = (_lib.i32 * (3 * n))(*[int(v) for c in recon for v in c.shape[1:]])
        crops = (_lib.i32 * (8 * len(table)))(*[int(v) for row in table for v in row])
        rec = torch.empty((len(table), 3, size, size), dtype=dtype, device=dev)
        trg = torch.empty_like(rec)
        _lib.check(_lib.lib().ttv_lpips_crops_forward(_lib.ptr_array(recon), _lib.ptr_array(target), dims, n, crops, len(table), size,
                                                      rec.data_ptr(), trg.data_ptr(), dt, _lib.stream_ptr(dev)), "ttv_lpips_crops_forward")
        ctx.mark_non_differentiable(trg)
        if any(ctx.needs_input_grad[3:3 + n]):
            ctx.save_for_backward(*recon)
            ctx.call = (dims, n, crops, len(table), size, dt)
        return rec, trg

    @staticmethod
    def backward(ctx, g, _g_target):
        dims, n, crops, n_crops, size, dt = ctx.call
        recon = ctx.saved_tensors
        dev = recon[0].device
        g = (torch.zeros((n_crops, 3, size, size), dtype=recon[0].dtype, device=dev) if g is None else g.to(recon[0].dtype)).contiguous()
        grads = [torch.empty_like(r) for r in recon]
        _lib.check(_lib.lib().ttv_lpips_crops_backward(_lib.ptr_array(recon), _lib.ptr_array(grads), dims, n, crops, n_crops, size,
                                                       g.data_ptr(), dt, _lib.stream_ptr(dev)), "ttv_lpips_crops_backward")
        return (None, None, None) + tuple(grads) + (None,) * n


class ReconstructionLoss(nn.Module):
    def __init__(self, config, perceptual_weights=None):
        super().__init__()
        self.config = config
        loss_c = config.tokenizer.losses
        loss_d = config.discriminator.losses
        self.perceptual_weight = float(loss_c.perceptual_weight)
        self.gram_weight = float(loss_c.gram_weight)
        if self.perceptual_weight > 0.0 or self.gram_weight > 0.0:
            source = perceptual_weights if perceptual_weights is not None else getattr(loss_c, "perceptual_weights", None)
            if source is None:
                raise NotImplementedError(
                    "the LPIPS / Gram terms need the VGG16 + LPIPS weights, which the reference fetches from the network "
                    "(lpips_gram.py:10-48): pass ReconstructionLoss(config, perceptual_weights=...) or set "
                    "tokenizer.losses.perceptual_weights to a state-dict file (see INTEGRATION.md), or set "
                    "tokenizer.losses.perceptual_weight = gram_weight = 0")
            if isinstance(source, (str, bytes, os.PathLike)):
                self.perceptual_model = LPIPS.from_file(source)
            else:
                self.perceptual_model = LPIPS()
                self.perceptual_model.load_state_dict(source, strict=True)
            self.perceptual_model.eval()
            for p in self.perceptual_model.parameters():
                p.requires_grad = False
        model_d = config.discriminator.model
        self.disc_weight = float(loss_c.disc_weight)
        if self.disc_weight > 0.0:
            self.disc_tokens = 4   # extra as register tokens (loss_module.py:42)
            self.disc_model = TiTokEncoder(model_size=model_d.model_size, patch_size=tuple(model_d.patch_size), in_channels=3,
                                           out_channels=1).apply(init_weights)
            # build-defined, absent = off: the discriminator tower's training tape in recompute mode (TiTok.set_activation_recompute)
            self.disc_model.activation_recompute = bool(getattr(model_d, "activation_recompute", False))
        self.gp_weight = float(loss_d.gp_weight)
        self.gp_noise = float(loss_d.gp_noise)
        self.centering_weight = float(loss_d.centering_weight)
        self.total_steps = config.training.main.max_steps

    # ---- perceptual crops (loss_module.py:59-93) ----------------------------------------------------------------------------
    def perceptual_preprocess(self, target, recon, resize_prob: float = 0.25):
        """Random crops of the frames, consuming Python's `random` exactly as the reference does, so the same `random.seed` picks
        the same frames and offsets: one random() per frame for the shuffle (sorted(..., key=random.random())), then per taken frame
        a random() for the resize only when the frame is at least the crop size on both edges, then randrange for the row and the
        column offsets.  The loop stops AFTER appending once i >= perceptual_samples_per_step (24 -> 25 crops; -1 -> all frames).
        The reconstruction is clamped to [-1, 1]; the resize is torchvision's resize(size=s) on a tensor (short edge -> s, long
        edge int(s * long / short), bicubic, align_corners=False, no antialias).  Returns (recon [F,C,s,s], target [F,C,s,s])."""
        target_out, recon_out = [], []
        size = int(self.config.tokenizer.losses.perceptual_sampling_size)
        samples = int(self.config.tokenizer.losses.perceptual_samples_per_step)
        plan = perceptual_crop_plan([tuple(t.shape[1:]) for t in target], size, samples, resize_prob)
        for k, _H, _W, new_h, new_w, dy, dx, resized in plan:
            trg, rec = target[k], recon[k].clamp(-1, 1)
            if resized:
                trg = F.interpolate(trg[None], size=(new_h, new_w), mode="bicubic", align_corners=False)[0]
                rec = F.interpolate(rec[None], size=(new_h, new_w), mode="bicubic", align_corners=False)[0]
            target_out.append(trg[:, dy:dy + size, dx:dx + size])
            recon_out.append(rec[:, dy:dy + size, dx:dx + size])
        return torch.stack(recon_out, dim=0).contiguous(), torch.stack(target_out, dim=0).contiguous()

    def perceptual_crops(self, target, recon, resize_prob: float = 0.25):
        """`perceptual_preprocess` of the clips' frames on the HIP path: the same draws (perceptual_crop_plan over the frames of clip 0,
        then clip 1, ...), the crops in one launch, their backward in one more; the per-frame views are never built.  `target` and
        `recon` are lists of GPU clips [3,T,H,W], bf16 or fp32 (what the kernels take: `_generator_step_loss` sends anything else down
        the eager path); clips that are not contiguous are made so and the target is cast to the reconstruction's dtype, as stacking
        the eager crops into one LPIPS batch does.  A frame that draws the resize but keeps its size is cut as a copy (the identity
        resize has the weights (0, 1, 0, 0) exactly).  Returns (recon [F,3,s,s], target [F,3,s,s])."""
        recon = [r.contiguous() for r in recon]
        target = [t.to(r.dtype).contiguous() for t, r in zip(target, recon)]
        size = int(self.config.tokenizer.losses.perceptual_sampling_size)
        samples = int(self.config.tokenizer.losses.perceptual_samples_per_step)
        shapes, owner = [], []
        for c, t in enumerate(target):
            T, H, W = t.shape[1:]
            shapes += [(H, W)] * T
            owner += [(c, f) for f in range(T)]
        plan = perceptual_crop_plan(shapes, size, samples, resize_prob)
        table = [owner[k] + (H, W, Hr, Wr, oy, ox) for k, H, W, Hr, Wr, oy, ox, _resized in plan]
        return PerceptualCrops.apply(table, size, len(recon), *recon, *target)

    # ---- discriminator access -------------------------------------------------------------------------------------------
    def disc_wrapper(self, x: Sequence[torch.Tensor]) -> torch.Tensor:
        """One logit per clip: the mean of the clip's 4 register-token outputs (loss_module.py:96-101)."""
        n = len(x)
        if _F32_HEAD:    # the tower's fp32 token outputs, averaged in fp32: no bf16 rounding of the logits themselves
            per_token = self.disc_model.forward_z(list(x), [self.disc_tokens] * n)  # fp32 [4 n, 1]
        else:            # the reference's dtype flow (encoder output cast to the clips' dtype, blocks.py:103)
            per_token = self.disc_model(list(x), [self.disc_tokens] * n)          # [4 n, 1]
        return per_token.view(n, -1).mean(dim=-1)

    def _disc_per_token(self, x: Sequence[torch.Tensor]) -> torch.Tensor:
        """The tower's output for the 4 register tokens of every clip, [4 n, 1]: what `disc_wrapper` averages."""
        n = len(x)
        if _F32_HEAD:
            return self.disc_model.forward_z(list(x), [self.disc_tokens] * n)
        return self.disc_model(list(x), [self.disc_tokens] * n)

    def gp_noise_add(self, real, fake, noise=None):
        """real + s and fake + s per clip with the same s in one HIP launch (`ttv_gp_noise_add`): s = noise[i] when `noise` is given,
        otherwise gp_noise times a standard normal drawn in the kernel from (torch.initial_seed(), this module's draw counter, the
        element's position in the batch) and never stored - tests/gp_noise_ref.py restates it.  The outputs are views of one flat
        allocation.  Clips: contiguous GPU tensors of one dtype, bf16 or fp32; `fake` and `noise` shaped like `real`."""
        n = len(real)
        dev, dtype = real[0].device, real[0].dtype
        for group in (real, fake) + (() if noise is None else (noise,)):
            if len(group) != n:
                raise ValueError("gp_noise_add: lists of different lengths")
            for t, r in zip(group, real):
                _lib.require_gpu(t, "gp_noise_add")
                if t.dtype != dtype or t.shape != r.shape or not t.is_contiguous() or t.device != dev:
                    raise ValueError("gp_noise_add: clips must be contiguous, of one dtype and device, and shaped alike across the lists")
        key = (tuple(t.numel() for t in real), dtype)
        st = self.__dict__.get("_gp_layout")
        if st is None or st["key"] != key:
            ctr, out, padded, chunks = gp_noise_layout(key[0])
            words = torch.zeros(7 * n + len(chunks), dtype=torch.int64)
            words[:7 * n].view(n, 7)[:, 5] = torch.tensor(key[0], dtype=torch.int64)
            words[:7 * n].view(n, 7)[:, 6] = torch.tensor(ctr, dtype=torch.int64)
            words[7 * n:] = torch.tensor(chunks, dtype=torch.int64)
            st = self.__dict__["_gp_layout"] = {"key": key, "out": out, "padded": padded, "words": words, "n_chunks": len(chunks)}
        tables = self.__dict__.get("_gp_tables")
        if tables is None or tables.device != dev:
            tables = self.__dict__["_gp_tables"] = _Tables(dev)
        flat = torch.empty(2 * st["padded"], dtype=dtype, device=dev)
        out_real = [flat[o:o + t.numel()].view_as(t) for o, t in zip(st["out"], real)]
        out_fake = [flat[st["padded"] + o:st["padded"] + o + t.numel()].view_as(t) for o, t in zip(st["out"], real)]
        words, n_chunks = st["words"], st["n_chunks"]
        ptrs = [[r.data_ptr(), f.data_ptr(), a.data_ptr(), b.data_ptr(), 0 if noise is None else noise[i].data_ptr()]
                for i, (r, f, a, b) in enumerate(zip(real, fake, out_real, out_fake))]
        words[:7 * n].view(n, 7)[:, :5] = torch.tensor(ptrs, dtype=torch.int64)
        slot = tables.take(n, n_chunks, entry_words=7)
        total = words.numel()
        slot["host"][:total].copy_(words)
        slot["dev"][:total].copy_(slot["host"][:total], non_blocking=True)
        base = slot["dev"].data_ptr()
        generate = noise is None
        draw = self.__dict__.get("_gp_draw", 0)
        _lib.check(_lib.lib().ttv_gp_noise_add(base, n, base + 56 * n, n_chunks, int(generate), torch.initial_seed() & (2 ** 64 - 1), draw,
                                               self.gp_noise, _lib.dtype_code(dtype), _lib.stream_ptr(dev)), "ttv_gp_noise_add")
        if generate:
            self.__dict__["_gp_draw"] = draw + 1       # once per generated draw: two steps never share counters
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        slot["event"] = ev
        return out_real, out_fake

    def _set_disc_trainable(self, flag: bool) -> None:
        params = self.__dict__.get("_disc_param_list")          # cached: parameters() walks the module tree, twice per step here
        if params is None:
            params = self.__dict__["_disc_param_list"] = list(self.disc_model.parameters())
        for p in params:
            p.requires_grad = flag

    @staticmethod
    def _report(prefix: str, terms) -> dict:
        """The reference's logging dictionary: every term reduced to a detached scalar under 'gen/..' or 'disc/..'."""
        return {f"{prefix}/{name}": value.clone().mean().detach() for name, value in terms.items()}

    def forward(self, target, recon, disc_forward: bool = False, gp_noise_tensors: Optional[List[torch.Tensor]] = None):
        if disc_forward:
            return self._discriminator_step_loss(target, recon, gp_noise_tensors)
        return self._generator_step_loss(target, recon)

    # ---- generator step (loss_module.py:110-162) -------------------------------------------------------------------------
    def _generator_step_loss(self, target, recon):
        real = [t.contiguous() for t in target]
        fake = [r.contiguous() for r in recon]
        # mean over clips of the per-clip L1 means (loss_module.py:118; value and gradient in one HIP launch).  The reference keeps
        # the [B] vector until the final .mean(); mean(a + w b) = mean(a) + w mean(b), so the scalar is carried instead.
        terms = {"recon_loss": l1_reconstruction_loss(fake, real)}
        total = terms["recon_loss"]
        if self.perceptual_weight > 0.0 or self.gram_weight > 0.0:              # (:123-137)
            # The reference unpacks preprocess's (recon, target) as (target, recon) and calls LPIPS(target crops, recon crops); both
            # terms are symmetric in their two arguments, so the crops go in as (recon, target) here and the gradient is taken
            # with respect to the HIP module's input.
            if _fused_crops() and all(c.is_cuda and c.dtype in (torch.bfloat16, torch.float32) for c in real + fake):
                rec_crops, trg_crops = self.perceptual_crops(real, fake)
            else:                                      # CPU tensors, other dtypes, or TTV_LPIPS_CROPS=0: the eager definition
                target_frames, recon_frames = [], []
                for t, r in zip(real, fake):
                    target_frames += t.unbind(1)
                    recon_frames += r.unbind(1)
                rec_crops, trg_crops = self.perceptual_preprocess(target_frames, recon_frames)
            lp, gr = self.perceptual_model(rec_crops, trg_crops.detach(), compute_gram=self.gram_weight > 0.0)
            if self.perceptual_weight > 0.0:
                terms["perceptual_loss"] = lp.mean()
                total = total + self.perceptual_weight * terms["perceptual_loss"]
            if self.gram_weight > 0.0:
                terms["gram_loss"] = gr.mean()
                total = total + self.gram_weight * terms["gram_loss"]
        if self.disc_weight > 0.0:
            self._set_disc_trainable(False)                                   # the generator sees a frozen critic (:144-146)
            if _fused_disc() and all(c.is_cuda and c.dtype in _HIP_DTYPES for c in real + fake):
                per_real = self._disc_per_token([t.detach() for t in real])   # no gradient path: runs the fused inference towers
                per_fake = self._disc_per_token(fake)                         # tape + inputs-only backward into the reconstruction
                g_mean, head = DiscHead.apply(_lib.TTV_DISC_HEAD_GENERATOR, len(real), self.disc_tokens, 0.0, 0.0, per_real, per_fake)
                total = total + self.disc_weight * g_mean
                report = self._report("gen", terms)
                report["gen/g_loss"] = head[1]                                # mean softplus(real - fake), from the head's buffer
                report.update(self._report("gen", {"total_loss": total}))
                return total, report
            score_real = self.disc_wrapper([t.detach() for t in real])        # no gradient path: runs the fused inference towers
            score_fake = self.disc_wrapper(fake)                              # tape + inputs-only backward into the reconstruction
            terms["g_loss"] = F.softplus(score_real - score_fake)             # softplus(-(fake - real)), relativistic (:149-151)
            total = total + self.disc_weight * terms["g_loss"].mean()
        terms["total_loss"] = total
        return total, self._report("gen", terms)

    # ---- discriminator step (loss_module.py:165-213) ----------------------------------------------------------------------
    def _discriminator_step_loss(self, target, recon, noise=None):
        # upstream marks both lists requires_grad (:168-169) for an autograd penalty it does not take on this path: the finite-difference
        # R1 / R2 below read logits only, so nothing reads d loss / d clip - without the flag the tower's backward skips its input
        # gradients (patch-embed dX for every packed clip) and autograd keeps no per-clip .grad.  Loss and parameter gradients are the same.
        real = [t.detach().contiguous() for t in target]
        fake = [r.detach().contiguous() for r in recon]
        self._set_disc_trainable(True)
        use_penalty = self.gp_weight > 0.0
        # The reference makes 2 (+2 with the penalty) discriminator calls; clips are independent inside the tower (block-diagonal
        # attention, per-row norms), so they are issued here as ONE packed call and the logits split afterwards: same values,
        # one tape / one backward / one set of weight-gradient launches instead of four.
        packed = real + fake
        hip = _fused_disc() and all(c.is_cuda and c.dtype in _HIP_DTYPES for c in packed)
        if hip:
            return self._discriminator_step_fused(real, fake, noise)
        if use_penalty:
            if noise is None:
                # one generator call for the whole batch instead of one per clip (a launch each), split into per-clip views
                flat = torch.randn(sum(t.numel() for t in real), dtype=real[0].dtype, device=real[0].device) * self.gp_noise
                noise, off = [], 0
                for t in real:
                    noise.append(flat[off:off + t.numel()].view_as(t))
                    off += t.numel()
            # multi-tensor adds: two launches instead of two per clip
            noisy = list(torch._foreach_add(real, list(noise))) + list(torch._foreach_add(fake, list(noise)))
        if use_penalty and _TWO_CALLS:
            # two packed calls with IDENTICAL plans: clip j and its noisy copy sit at the same packed rows of their call
            scores = torch.cat([self.disc_wrapper(packed), self.disc_wrapper(noisy)]).view(-1, len(real))
        else:
            if use_penalty:
                packed = packed + noisy
            scores = self.disc_wrapper(packed).view(-1, len(real))            # rows: real, fake, (real + noise, fake + noise)
        score_real, score_fake = scores[0], scores[1]
        margin = score_real - score_fake
        terms = {"d_loss": F.softplus(-margin), "logits_relative": margin}
        total = terms["d_loss"]
        if use_penalty:                                                       # finite-difference R1 / R2 (:187-198)
            terms["r1_penalty"] = (score_real - scores[2]).square()
            terms["r2_penalty"] = (score_fake - scores[3]).square()
            total = total + (self.gp_weight / self.gp_noise ** 2) * (terms["r1_penalty"] + terms["r2_penalty"])
        if self.centering_weight > 0.0:                                       # keeps real / fake logits centred on zero (:201-204)
            terms["centering_loss"] = 0.5 * (score_real + score_fake).square()
            total = total + self.centering_weight * terms["centering_loss"]
        total = total.mean()
        terms["total_loss"] = total
        return total, self._report("disc", terms)

    def _discriminator_step_fused(self, real, fake, noise):
        """The same step with the noise and both additions in one launch (`gp_noise_add`) and everything after the towers in one
        more (`DiscHead`): the reported scalars are views of the head's buffer."""
        n, packed = len(real), real + fake
        use_penalty = self.gp_weight > 0.0
        noisy = []
        if use_penalty:
            same = len({t.dtype for t in packed}) == 1 and all(r.shape == f.shape for r, f in zip(real, fake))
            if noise is not None:
                noise = [z.contiguous() for z in noise]
                same = same and len(noise) == n and all(z.is_cuda and z.dtype == r.dtype and z.shape == r.shape for z, r in zip(noise, real))
            if same:
                noisy_real, noisy_fake = self.gp_noise_add(real, fake, noise)
                noisy = noisy_real + noisy_fake
            elif noise is not None:            # mixed dtypes or shapes that broadcast: torch's promotion rules, as the eager route
                noisy = list(torch._foreach_add(real, list(noise))) + list(torch._foreach_add(fake, list(noise)))
            else:
                raise ValueError("the discriminator step draws its R1 / R2 noise for clips of one dtype, real and fake shaped alike")
        if use_penalty and _TWO_CALLS:
            a, b = self._disc_per_token(packed), self._disc_per_token(noisy)
        else:
            a, b = self._disc_per_token(packed + noisy), None
        gp_scale = self.gp_weight / self.gp_noise ** 2 if use_penalty else 0.0
        total, head = DiscHead.apply(_lib.TTV_DISC_HEAD_DISCRIMINATOR, n, self.disc_tokens, gp_scale, max(self.centering_weight, 0.0),
                                     a.contiguous(), None if b is None else b.contiguous())
        report = {"disc/d_loss": head[1], "disc/logits_relative": head[2]}
        if use_penalty:
            report["disc/r1_penalty"], report["disc/r2_penalty"] = head[3], head[4]
        if self.centering_weight > 0.0:
            report["disc/centering_loss"] = head[5]
        report["disc/total_loss"] = head[0]
        return total, report
