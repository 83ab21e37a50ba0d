"""TiTok: the reference tokenizer facade (model/titok.py:23-74) on the MI355X HIP path.

Same constructor (`config.tokenizer.model.{fsq_levels, encoder_size, decoder_size, patch_size}`), methods, return
types and state-dict keys (`encoder.*`, `decoder.*`; FSQ has no persistent keys).  Differences, on purpose:
  * `token_counts` / `grids` may be Python lists or CPU tensors (no host sync) as well as the reference's device tensors;
  * `encode(..., split_indices=True)` works (it raises TypeError upstream) and returns a tuple
    of per-clip index tensors;
  * the encoder tail and FSQ are one kernel, with the pre-quantisation tokens kept in fp32 (the reference rounds
    them to bf16 under autocast before `z.float()`, fsq.py:128);
  * BUILD-DEFINED, NOT REFERENCE-PINNED: `config.tokenizer.model.quantizer = "l2"` (with `codebook_size`, `token_size`) wires the
    nearest-codebook-entry quantiser of BASELINE.json's configs #4 / #5 (8192 x 32, 16384 x 64) into the one quantiser slot the
    reference has (titok.py:37,47-52): encode -> L2 argmin + straight-through lookup -> decode.  The reference itself ships FSQ only;
    the default (`quantizer` absent or "fsq") is the reference's model.  Trainable (round 4): under autograd the towers record their
    tape, the lookup is straight-through towards the encoder and passes the decoder's token gradient to the selected codebook rows;
  * BUILD-DEFINED: `config.tokenizer.model.activation_recompute = True` (absent: off) trains both towers on the recompute tape
    (`set_activation_recompute`): same gradients, a fraction of the activation memory, one more forward of the layers.
  * BUILD-DEFINED: `config.tokenizer.model.attention_pv = "fp8"` (absent / None: off) runs the attention's P.V product of both towers'
    bf16 inference forwards in e4m3 on the block-scaled 32x32x64 MFMA (`set_attention_pv`): an accuracy-for-arithmetic trade whose
    price INTEGRATION.md states; never a default, training forwards are unaffected.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..plan import host_ints
from .base.blocks import TiTokDecoder, TiTokEncoder
from .base.utils import init_weights
from .quantizer.fsq import FSQ
from .quantizer.vq_l2 import L2Quantizer


class TiTok(nn.Module):
    """encoder -> FSQ -> decoder over lists of [3,T,H,W] clips; parameters live in `encoder.*` and `decoder.*`."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        m = config.tokenizer.model
        patch = tuple(int(p) for p in m.patch_size)
        self.quantizer_kind = str(getattr(m, "quantizer", "fsq")).lower()
        if self.quantizer_kind == "fsq":
            fsq_levels = [int(v) for v in m.fsq_levels]
            n_code = len(fsq_levels)                   # one latent channel per FSQ level
            quantize = FSQ(levels=fsq_levels)
        elif self.quantizer_kind == "l2":
            n_code, n_entries = int(m.token_size), int(m.codebook_size)
            g = torch.Generator().manual_seed(int(getattr(m, "codebook_seed", 0)))
            # synthetic start; `quantize.codebook` is a Parameter.  The optional keys switch on the commitment term and the EMA codebook
            # with its data-dependent restart (vq_l2.py); absent, the quantiser is the plain straight-through lookup.
            quantize = L2Quantizer(torch.randn(n_entries, n_code, generator=g),
                                   commitment_weight=float(getattr(m, "commitment_weight", 0.0)),
                                   codebook_update=str(getattr(m, "codebook_update", "grad")).lower(),
                                   decay=float(getattr(m, "codebook_decay", 0.99)), eps=float(getattr(m, "codebook_eps", 1e-5)),
                                   dead_code_threshold=float(getattr(m, "dead_code_threshold", 0.0)), seed=int(getattr(m, "codebook_seed", 0)))
        else:
            raise ValueError(f"tokenizer.model.quantizer must be 'fsq' or 'l2', got {self.quantizer_kind!r}")
        towers = dict(encoder=TiTokEncoder(model_size=m.encoder_size, patch_size=patch, in_channels=3, out_channels=n_code),
                      quantize=quantize,
                      decoder=TiTokDecoder(model_size=m.decoder_size, patch_size=patch, in_channels=n_code, out_channels=3))
        for name, mod in towers.items():               # registration order = the reference's state-dict order
            setattr(self, name, mod)
        self.apply(init_weights)                       # nn.Linear / RMSNorm only: the L2 codebook keeps its start values
        self.last_bounded = None   # fp32 FSQ pre-rounding values of the last encode(want_bounded=True)
        # Index-exact inference (round 4): token indices are decided by the ENCODER alone (fsq.py:123-135 forces fp32 inside FSQ because
        # round() is discontinuous), so `encoder_dtype = torch.float32` runs the encoder on the exact-fp32 MFMA kernels - the reference's
        # fp32 indices bit for bit - whatever dtype the clips arrive in, while the decoder keeps computing in the clips' dtype (bf16).
        # `decoder_dtype` likewise fixes the decoder's compute dtype (its reconstructions come back in that dtype).  With fp32 master
        # parameters, `encoder_dtype = float32, decoder_dtype = bfloat16` is the index-exact configuration bench.py times as `exact_index`.
        # None (default): both towers follow the clips, as the reference's modules do.
        self.encoder_dtype = None
        self.decoder_dtype = None
        self.set_activation_recompute(bool(getattr(m, "activation_recompute", False)))
        self.set_attention_pv(getattr(m, "attention_pv", None))

    def set_activation_recompute(self, flag: bool):
        """Training memory: True makes both towers keep only the residual stream at the layer boundaries and rebuild one layer's
        activations at a time during the backward (blocks._Tower.activation_recompute); False (default) stores them all.  Takes
        effect with the next training forward; gradients are the stored tape's, bit for bit wherever those are reproducible."""
        self.encoder.activation_recompute = self.decoder.activation_recompute = bool(flag)
        return self

    def set_attention_pv(self, mode):
        """Inference arithmetic of the attention's second product in both towers: None (default) - bf16 P.V, today's kernels and bits;
        "fp8" - P as e4m3 and V as a block-scaled (OCP MX) e4m3 image on v_mfma_scale_f32_32x32x64_f8f6f4 (scores, softmax and row sums
        stay bf16 / fp32; ~2^-5 relative per probability and value instead of bf16's 2^-9).  bf16 inference forwards
        only: fp32 clips and the `set_index_exact` modes raise ValueError; forwards under autograd run as without it."""
        if mode not in (None, "fp8"):
            raise ValueError("attention_pv must be None or 'fp8'")
        if mode is not None and self.encoder_dtype is not None:
            raise ValueError("attention_pv='fp8' does not combine with set_index_exact modes (fp32 / split-bf16 encoder)")
        self.encoder.attention_pv = self.decoder.attention_pv = mode
        return self

    def set_index_exact(self, mode):
        """Inference arithmetic that keeps the reference's fp32 token indices (parameters must be fp32 masters):
        None     - both towers follow the clips' dtype (the reference's behaviour; default);
        "fp32"   - encoder on the exact-fp32 MFMA kernels (bit-exact indices), decoder bf16;
        "split3" - encoder on the split-bf16 three-pass kernels (~2^-17 per product: every index of the benchmark fixture kept, not a
                   bit-for-bit guarantee), decoder bf16.  About 2.5x the throughput of "fp32"."""
        if mode not in (None, "fp32", "split3"):
            raise ValueError("mode must be None, 'fp32' or 'split3'")
        if mode is not None and self.encoder.attention_pv is not None:
            raise ValueError("set_index_exact modes do not combine with attention_pv='fp8' (a bf16 inference mode)")
        self.encoder_dtype = None if mode is None else torch.float32
        self.decoder_dtype = None if mode is None else torch.bfloat16
        self.encoder.f32_split3 = mode == "split3"
        return self

    # ---- encode ---------------------------------------------------------------------------------------------------------
    def _encode_differentiable(self, clips, counts, grids, split_indices):
        """Training step (train.py:65-83): tape-recording towers with the HIP backward, straight-through FSQ."""
        z = self.encoder.forward_z(clips, counts, grids)               # fp32, carries the autograd graph
        codes, info = self.quantize(z)
        self.last_bounded = None
        if split_indices:
            info["indices"] = torch.split(info["indices"], counts, dim=0)
        return codes.to(clips[0].dtype), info

    def encode(self, x, token_counts, grids=None, split_indices=False, want_bounded=False):
        counts = host_ints(token_counts)
        if self.encoder_dtype is not None and x[0].dtype != self.encoder_dtype and not self.encoder._wants_grad(*x):
            out_dtype = x[0].dtype
            codes, info = self.encode([c.to(self.encoder_dtype) for c in x], counts, grids, split_indices, want_bounded)
            return codes.to(out_dtype), info
        if self.quantizer_kind == "l2":
            if self.encoder._wants_grad(*x):
                # training through the one quantiser slot (titok.py:47-52, train.py:65-83): tape-recording towers, straight-through lookup
                z = self.encoder.forward_z(x, counts, grids)                          # fp32, carries the autograd graph
                codes, info = self.quantize(z.to(x[0].dtype))
                self.last_bounded = None
                if split_indices:
                    info["indices"] = torch.split(info["indices"], counts, dim=0)
                return codes, info
            z = self.encoder.run(x, counts, grids, None, want_z=True)["z"]          # fp32 [sum K, token_size]
            codes, info = self.quantize(z.to(x[0].dtype))
            self.last_bounded = None
            if split_indices:
                info["indices"] = torch.split(info["indices"], counts, dim=0)
            return codes, info
        if self.encoder._wants_grad(*x):
            return self._encode_differentiable(x, counts, grids, split_indices)
        res = self.encoder.run(x, counts, grids, self.quantize.params, want_z=False, want_bounded=want_bounded)
        self.last_bounded = res["bounded"]
        idx = torch.split(res["indices"], counts, dim=0) if split_indices else res["indices"]
        return res["codes"], {"indices": idx}

    # ---- decode ---------------------------------------------------------------------------------------------------------
    def decode(self, x, token_counts, grids):
        if self.decoder_dtype is not None and x.dtype != self.decoder_dtype and not self.decoder._wants_grad(x):
            x = x.to(self.decoder_dtype)
        return self.decoder(x, token_counts, grids)

    def decode_indices(self, indices, grids, token_counts=None):
        if token_counts is None:                        # per-clip index tensors (titok.py:54-58)
            assert type(indices) in [list, tuple]
            token_counts = [int(part.shape[0]) for part in indices]
            indices = torch.cat(list(indices), dim=0)
        # reference: decoder parameter dtype (titok.py:61); under autocast (Lightning bf16-mixed, fp32 masters)
        # the towers compute in the autocast dtype, so follow it
        compute_dtype = torch.get_autocast_gpu_dtype() if torch.is_autocast_enabled() else next(self.decoder.parameters()).dtype
        if self.quantizer_kind == "l2":
            return self.decode(self.quantize.lookup(indices, compute_dtype), token_counts, grids)
        return self.decode(self.quantize.indices_to_codes(indices, dtype=compute_dtype), token_counts, grids)

    def forward(self, x, token_counts):
        pixel_grids = [tuple(clip.shape[1:]) for clip in x]     # host ints; the reference builds a device tensor (titok.py:70)
        counts = host_ints(token_counts)
        codes, info = self.encode(x, counts, pixel_grids)
        return self.decode(codes, counts, pixel_grids), info
