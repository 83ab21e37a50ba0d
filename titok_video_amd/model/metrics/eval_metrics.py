"""PSNR and SSIM of the evaluation loop on the GPU (reference model/metrics/eval_metrics.py:11-51, the 'psnr' and 'ssim' entries).

The reference builds torchmetrics' PeakSignalNoiseRatio(data_range=2) and StructuralSimilarityIndexMeasure(data_range=2) and feeds
them `x.clamp(-1, 1)` per clip, CTHW -> TCHW (eval_metrics.py:19-21, 32-37).
- PSNR: a running sum of squared errors and an element count, `10 * log10(data_range^2 / mse)` at compute().  Both sums live in one
  device buffer filled by `ttv_sq_err_accumulate` (one launch per update).
- SSIM: 11-tap Gaussian window (sigma 1.5), C1 = (0.01 * 2)^2, C2 = (0.03 * 2)^2, per frame the mean over C x (H-10) x (W-10) (the
  windows wholly inside the frame: exactly what torchmetrics' reflect-pad + crop keeps); a running sum of per-frame values and a
  frame count, so compute() is a mean of per-frame means, not a pixel-weighted mean.  Filled by `ttv_ssim_accumulate` (two launches
  per call of up to 64 clips; per-tile partials in a workspace this module owns, reduced in a fixed order: bit-reproducible).
  Deliberate deviations from torchmetrics: fp32 arithmetic for bf16 and fp32 inputs (under bf16 autocast torchmetrics convolves
  in bf16); frames with H < 11 or W < 11 are refused (torchmetrics gives NaN for 6-10 and raises for <= 5); no cross-rank sum
  in compute() (torchmetrics sums its state over ranks; PSNR here does not either).
- FVD (the 'fvd' entry, reference fvd.FVDCalculator): needs the I3D detector's weights from a local file, given as
  `EvalMetrics(config, fvd_detector=path)` or the optional config key `training.eval.fvd_detector`; without one 'fvd' raises as
  before.  The reconstruction is clamped, the target is not (eval_metrics.py:33), each clip goes in as a batch of one; see
  fvd.py for the preprocessing and the detector.  The detector's weights are not part of state_dict().
- JEDi (the 'jedi' entry, reference jedi.JEDiMetric): needs the V-JEPA encoder's and the SSv2 probe's weights from local files,
  given as `EvalMetrics(config, jedi_weights=..., jedi_probe=...)` or the optional config keys `training.eval.jedi_weights` /
  `training.eval.jedi_probe`; without them 'jedi' raises as before.  `training.eval.jedi_jepa_model` is honoured (vit_large only).
  Both clips are clamped (get_feats clamps again), each goes in as a batch of one; see jedi.py.  The weights are not part of
  state_dict().
- LPIPS (the 'lpips' entry): per-frame LPIPS of whole frames, `LPIPS.frame_distances` (lpips_gram.py; csrc/ttv_lpips.hip, the
  evaluation path: any frame size in 16 .. 2048 with floor max-pools, no tape).  Needs the VGG16 + LPIPS weights from a local file or
  state dict with the reference LPIPS keys, given as `EvalMetrics(config, lpips_weights=path_or_state_dict)` or the optional config key
  `training.eval.lpips_weights`, or an `LPIPS` module as `lpips_model=` (the loss module's `perceptual_model`, so the weights are
  loaded and packed once); without any of them 'lpips' raises as before.  The reconstruction is clamped, the target is not
  (eval_metrics.py:33-37), each frame pair is a batch entry of its own.  State: a running sum of per-frame values and a frame
  count (double, on the device), so compute() is a mean of per-frame values like SSIM; no cross-rank sum in compute(), as for PSNR
  and SSIM.  The weights are not part of state_dict().
- FID / IS / MMD (the 'fid', 'is' and 'mmd' entries, reference metrics.MetricCalculator): frame metrics on Inception-v3, which
  needs torchvision's `inception_v3` weights from a local file or state dict, given as `EvalMetrics(config, inception_weights=...)`
  or the optional config key `training.eval.inception_weights`; without them the three raise as before.  Every frame of every clip is
  one image, read in place; the reconstruction is clamped, the target is not, and the reconstructions are the "generated" set.  One
  extractor and one feature store serve the three entries (metrics.py InceptionStats); features stay on the device until compute(),
  which runs the float64 statistics on the host.  The weights are not part of state_dict().
No host sync until compute().
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Sequence

import torch
import torch.nn as nn

from ... import _lib

AVAILABLE = ("psnr", "ssim")


class EvalMetrics(nn.Module):
    def __init__(self, config=None, eval_prefix: str = "eval", fvd_detector=None, jedi_weights=None, jedi_probe=None,
                 lpips_weights=None, lpips_model=None, inception_weights=None):
        super().__init__()
        self.eval_prefix = eval_prefix
        names = ["psnr"]
        self._fvd = None
        self._jedi = None
        self._lpips = None
        self._inception = None
        if config is not None:
            names = [m for m in config.training.eval.log_metrics]
            if fvd_detector is None:
                fvd_detector = getattr(config.training.eval, "fvd_detector", None)
            if jedi_weights is None:
                jedi_weights = getattr(config.training.eval, "jedi_weights", None)
            if jedi_probe is None:
                jedi_probe = getattr(config.training.eval, "jedi_probe", None)
            if lpips_weights is None and lpips_model is None:
                lpips_weights = getattr(config.training.eval, "lpips_weights", None)
            if inception_weights is None:
                inception_weights = getattr(config.training.eval, "inception_weights", None)
            for m in names:
                if m == "lpips" and (lpips_model is not None or lpips_weights is not None):
                    from .lpips_gram import LPIPS
                    if lpips_model is None:
                        if isinstance(lpips_weights, (str, bytes)) or hasattr(lpips_weights, "__fspath__"):
                            lpips_model = LPIPS.from_file(lpips_weights)
                        else:
                            lpips_model = LPIPS()
                            lpips_model.load_state_dict(lpips_weights, strict=True)
                            lpips_model.eval()
                    self.__dict__["_lpips"] = lpips_model      # not a submodule: the weights stay out of state_dict(), like _fvd
                elif m == "fvd" and fvd_detector is not None:
                    from .fvd import FVDCalculator
                    self.__dict__["_fvd"] = FVDCalculator(detector=fvd_detector)
                elif m == "jedi" and jedi_weights is not None:
                    from .jedi import JEDiMetric
                    model_name = getattr(config.training.eval, "jedi_jepa_model", "vit_large")
                    self.__dict__["_jedi"] = JEDiMetric(model_name=model_name, weights=jedi_weights, probe=jedi_probe)
                elif m in ("fid", "is", "mmd") and inception_weights is not None:
                    if self._inception is None:      # one extractor and one feature store for the three entries
                        from .metrics import InceptionStats, make_extractor
                        self.__dict__["_inception"] = InceptionStats(make_extractor(inception_weights), names)
                elif m not in AVAILABLE:
                    raise NotImplementedError(f"metric '{m}' is not built: FVD / JEDi need weights fetched over the network "
                                              f"(reference model/metrics/); the available metrics are {', '.join(AVAILABLE)}")
        self.names = names
        self._acc = None         # psnr: (sum of squared errors, element count), double
        self._ssim_acc = None    # ssim: (sum of per-frame SSIM, frame count), double
        self._ssim_ws = None     # ssim: per-tile partial sums, grown as needed
        self._det_scratch = None # psnr in deterministic mode: the block partials, grown as needed
        self._lpips_acc = None   # lpips: (sum of per-frame LPIPS, frame count), double

    def _ssim_groups(self, rs, ts):
        """Host-side shapes and workspace sizes of every call of up to TTV_MAX_CLIPS_PER_LAUNCH clips (raises before any launch)."""
        groups = []
        for c0 in range(0, len(rs), _lib.TTV_MAX_CLIPS_PER_LAUNCH):
            r, t = rs[c0:c0 + _lib.TTV_MAX_CLIPS_PER_LAUNCH], ts[c0:c0 + _lib.TTV_MAX_CLIPS_PER_LAUNCH]
            for a, b in zip(r, t):
                if a.dim() != 4 or a.shape != b.shape:
                    raise ValueError(f"EvalMetrics ssim: clips must be [C,T,H,W] pairs of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
            dims = (C.c_int32 * (4 * len(r)))(*[int(d) for a in r for d in a.shape])
            nbytes = _lib.lib().ttv_ssim_workspace_bytes(dims, len(r))
            if nbytes < 0:
                _lib.check(1, "ttv_ssim_workspace_bytes")
            groups.append((r, t, dims, nbytes))
        return groups

    def update(self, recon: Sequence[torch.Tensor], target: Sequence[torch.Tensor]) -> None:
        if not self.names:
            return
        r0 = recon[0]
        _lib.require_gpu(r0, "EvalMetrics.update")
        rs = [t.contiguous() for t in recon]
        ts = [t.to(r0.dtype).contiguous() for t in target]
        dt, stream = _lib.dtype_code(r0.dtype), _lib.stream_ptr(r0.device)
        groups = self._ssim_groups(rs, ts) if "ssim" in self.names else []
        if self._lpips is not None:
            self._lpips._check_clips(rs, ts)      # raises before any launch
        if "psnr" in self.names:
            if self._acc is None or self._acc.device != r0.device:
                self._acc = torch.zeros(2, dtype=torch.float64, device=r0.device)
            sizes = (C.c_int32 * len(rs))(*[int(t.numel()) for t in rs])
            if _lib.is_deterministic():      # fixed-order sums: the block partials go through a scratch this object keeps
                need = _lib.lib().ttv_sq_err_accumulate_det_scratch_bytes(sizes, len(rs))
                if need < 0:
                    _lib.check(1, "ttv_sq_err_accumulate_det_scratch_bytes")
                if self._det_scratch is None:
                    self._det_scratch = _lib.DetScratch()
                scratch = self._det_scratch.get(need, r0.device)
                rc = _lib.lib().ttv_sq_err_accumulate_det(_lib.ptr_array(rs), _lib.ptr_array(ts), sizes, len(rs), dt, 1, self._acc.data_ptr(),
                                                          scratch.data_ptr(), scratch.numel(), stream)
                _lib.check(rc, "ttv_sq_err_accumulate_det")
            else:
                rc = _lib.lib().ttv_sq_err_accumulate(_lib.ptr_array(rs), _lib.ptr_array(ts), sizes, len(rs), dt, 1, self._acc.data_ptr(), stream)
                _lib.check(rc, "ttv_sq_err_accumulate")
        if groups:
            if self._ssim_acc is None or self._ssim_acc.device != r0.device:
                self._ssim_acc = torch.zeros(2, dtype=torch.float64, device=r0.device)
            need = max(g[3] for g in groups)
            if self._ssim_ws is None or self._ssim_ws.device != r0.device or self._ssim_ws.numel() < need:
                self._ssim_ws = torch.empty(need, dtype=torch.uint8, device=r0.device)
            for r, t, dims, nbytes in groups:
                rc = _lib.lib().ttv_ssim_accumulate(_lib.ptr_array(r), _lib.ptr_array(t), dims, len(r), dt, 1, self._ssim_acc.data_ptr(),
                                                    self._ssim_ws.data_ptr(), self._ssim_ws.numel(), stream)
                _lib.check(rc, "ttv_ssim_accumulate")
        if self._lpips is not None:
            if self._lpips_acc is None or self._lpips_acc.device != r0.device:
                self._lpips_acc = torch.zeros(2, dtype=torch.float64, device=r0.device)
            self._lpips.frame_distances(rs, ts, clamp_recon=True, acc=self._lpips_acc)
        if self._fvd is not None:
            self._fvd.update_clips(recon, target, clamp_recon=True)
        if self._jedi is not None:
            self._jedi.update_clips(recon, target)
        if self._inception is not None:
            def frames(clips):
                return [c[:, t] for c in (c.contiguous() for c in clips) for t in range(c.shape[1])]
            self._inception.update(frames(target), frames(recon), clamp_generated=True)

    def compute(self) -> dict:
        out = {}
        for name in self.names:
            if name == "psnr" and self._acc is not None:
                sq, n = (float(v) for v in self._acc.cpu())
                out[f"{self.eval_prefix}/psnr"] = 10.0 * math.log10(4.0 * n / sq) if sq > 0 else float("inf")
            elif name == "ssim" and self._ssim_acc is not None:
                s, n = (float(v) for v in self._ssim_acc.cpu())
                out[f"{self.eval_prefix}/ssim"] = s / n if n > 0 else float("nan")
            elif name == "lpips" and self._lpips_acc is not None:
                s, n = (float(v) for v in self._lpips_acc.cpu())
                out[f"{self.eval_prefix}/lpips"] = s / n if n > 0 else float("nan")
            elif name == "fvd" and self._fvd is not None:
                out[f"{self.eval_prefix}/fvd"] = self._fvd.compute()
            elif name == "jedi" and self._jedi is not None:
                out[f"{self.eval_prefix}/jedi"] = self._jedi.compute()
            elif name in ("fid", "is", "mmd") and self._inception is not None:
                out[f"{self.eval_prefix}/{name}"] = self._inception.compute(name)
        return out

    def reset(self) -> None:
        for acc in (self._acc, self._ssim_acc, self._lpips_acc):
            if acc is not None:
                acc.zero_()
        if self._fvd is not None:
            self._fvd.reset()
        if self._jedi is not None:
            self._jedi.reset()
        if self._inception is not None:
            self._inception.reset()
