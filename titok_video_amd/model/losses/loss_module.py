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
