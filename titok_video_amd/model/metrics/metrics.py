"""Mirror of the reference's frame metrics (model/metrics/metrics.py) on the HIP path (csrc/ttv_inception.hip): the Fréchet Inception
Distance ('fid'), the Inception Score ('is') and the polynomial-kernel MMD ('mmd') on torchvision's Inception-v3.

Same names: `MetricCalculator` with `reset()`, `forward(real, generated)` on lists of CHW images in [-1, 1] and `gather()`;
`calculate_fid`, `calculate_frechet_distance`, `calculate_activation_statistics`, `compute_inception_score` and `mmd_poly` in
float64 numpy with scipy's sqrtm, as the reference defines them.

What the extractor computes per image, as the reference's InceptionV3 wrapper does: no clamp and no ImageNet normalisation (the
wrapper calls torchvision's submodules one by one, so `transform_input` never runs), fp32 with autocast off,
`nn.Upsample(size=(299, 299), mode='bilinear', align_corners=True)`, the trunk Conv2d_1a_3x3 .. Mixed_7c (AuxLogits unused),
`avg_pool2d(8)` -> `acts` [2048], `fc` -> `softmax` -> `probs` [1000].  The preprocessing and the whole network run in HIP kernels
in fp32.  Features stay on the device until `gather()`; they are not gathered across ranks (neither are the reference's).

Differences from the reference, all deliberate:
  * the network's weights never come from the network.  `inception_weights` is torchvision's `inception_v3` checkpoint file
    (inception_v3_google-0cc3c7bd.pth) or a flat state dict with its keys; see `inception_state_dict`.  Without it the Inception
    metrics raise and say how to give one.
  * images are processed in launches of up to TTV_MAX_CLIPS_PER_LAUNCH, not one by one; every output is a fixed-order fp32 chain, so
    an image's features do not depend on what shares its launch.
  * `gather()` computes the statistics in float64 (the reference hands float32 features to numpy, which accumulates the means in
    float32) and returns Python floats.
  * `MetricCalculator`'s 'ssim' and 'psnr' are not built: torchmetrics' functional forms with the tuple `data_range=(-1, 1)` clamp both
    images and average per image, which the accumulate kernels behind `EvalMetrics` ('ssim', 'psnr': clamped reconstruction, unclamped
    target, frame- and element-weighted) do not do.  They raise NotImplementedError naming `EvalMetrics`.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import OrderedDict
from typing import Dict, List, Mapping, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from ... import _lib
from .jedi import mmd_poly as _mmd_poly

BN_EPS = 1e-3
INPUT_SIZE = _lib.TTV_INCEPTION_INPUT
FEATURES, CLASSES = _lib.TTV_INCEPTION_FEATURES, _lib.TTV_INCEPTION_CLASSES


# ---- architecture -----------------------------------------------------------------------------------------------------------
def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _u(name, cin, cout, k=1, s=1, p=0):
    return (name, cin, cout, _pair(k), _pair(s), _pair(p))


def _inception_a(name, cin, pf):
    units = [_u(f"{name}.branch1x1", cin, 64), _u(f"{name}.branch5x5_1", cin, 48), _u(f"{name}.branch5x5_2", 48, 64, 5, 1, 2),
             _u(f"{name}.branch3x3dbl_1", cin, 64), _u(f"{name}.branch3x3dbl_2", 64, 96, 3, 1, 1),
             _u(f"{name}.branch3x3dbl_3", 96, 96, 3, 1, 1), _u(f"{name}.branch_pool", cin, pf)]
    return units, [64, 64, 96, pf]


def _inception_b(name, cin):
    units = [_u(f"{name}.branch3x3", cin, 384, 3, 2), _u(f"{name}.branch3x3dbl_1", cin, 64),
             _u(f"{name}.branch3x3dbl_2", 64, 96, 3, 1, 1), _u(f"{name}.branch3x3dbl_3", 96, 96, 3, 2)]
    return units, [384, 96, cin]


def _inception_c(name, cin, c7):
    h, v = dict(k=(1, 7), p=(0, 3)), dict(k=(7, 1), p=(3, 0))
    units = [_u(f"{name}.branch1x1", cin, 192), _u(f"{name}.branch7x7_1", cin, c7), _u(f"{name}.branch7x7_2", c7, c7, **h),
             _u(f"{name}.branch7x7_3", c7, 192, **v), _u(f"{name}.branch7x7dbl_1", cin, c7), _u(f"{name}.branch7x7dbl_2", c7, c7, **v),
             _u(f"{name}.branch7x7dbl_3", c7, c7, **h), _u(f"{name}.branch7x7dbl_4", c7, c7, **v),
             _u(f"{name}.branch7x7dbl_5", c7, 192, **h), _u(f"{name}.branch_pool", cin, 192)]
    return units, [192, 192, 192, 192]


def _inception_d(name, cin):
    units = [_u(f"{name}.branch3x3_1", cin, 192), _u(f"{name}.branch3x3_2", 192, 320, 3, 2), _u(f"{name}.branch7x7x3_1", cin, 192),
             _u(f"{name}.branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3)), _u(f"{name}.branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0)),
             _u(f"{name}.branch7x7x3_4", 192, 192, 3, 2)]
    return units, [320, 192, cin]


def _inception_e(name, cin):
    h, v = dict(k=(1, 3), p=(0, 1)), dict(k=(3, 1), p=(1, 0))
    units = [_u(f"{name}.branch1x1", cin, 320), _u(f"{name}.branch3x3_1", cin, 384), _u(f"{name}.branch3x3_2a", 384, 384, **h),
             _u(f"{name}.branch3x3_2b", 384, 384, **v), _u(f"{name}.branch3x3dbl_1", cin, 448),
             _u(f"{name}.branch3x3dbl_2", 448, 384, 3, 1, 1), _u(f"{name}.branch3x3dbl_3a", 384, 384, **h),
             _u(f"{name}.branch3x3dbl_3b", 384, 384, **v), _u(f"{name}.branch_pool", cin, 192)]
    return units, [320, 384 + 384, 384 + 384, 192]


STEM = [_u("Conv2d_1a_3x3", 3, 32, 3, 2), _u("Conv2d_2a_3x3", 32, 32, 3), _u("Conv2d_2b_3x3", 32, 64, 3, 1, 1),
        _u("Conv2d_3b_1x1", 64, 80), _u("Conv2d_4a_3x3", 80, 192, 3)]
# (block, kind, in, its argument): kinds A (pool features), B, C (channels_7x7), D, E
BLOCK_ARGS = [("Mixed_5b", "A", 192, 32), ("Mixed_5c", "A", 256, 64), ("Mixed_5d", "A", 288, 64), ("Mixed_6a", "B", 288, None),
              ("Mixed_6b", "C", 768, 128), ("Mixed_6c", "C", 768, 160), ("Mixed_6d", "C", 768, 160), ("Mixed_6e", "C", 768, 192),
              ("Mixed_7a", "D", 768, None), ("Mixed_7b", "E", 1280, None), ("Mixed_7c", "E", 2048, None)]
_BUILDERS = {"A": _inception_a, "B": _inception_b, "C": _inception_c, "D": _inception_d, "E": _inception_e}


def blocks() -> "OrderedDict[str, dict]":
    """Block name -> {kind, cin, units, widths (of the concatenated slices, in order), cout}."""
    out = OrderedDict()
    for name, kind, cin, arg in BLOCK_ARGS:
        units, widths = _BUILDERS[kind](name, cin) if arg is None else _BUILDERS[kind](name, cin, arg)
        out[name] = dict(kind=kind, cin=cin, units=units, widths=widths, cout=sum(widths))
    return out


def unit_specs() -> List[Tuple[str, int, int, Tuple[int, int], Tuple[int, int], Tuple[int, int]]]:
    """The 94 units in the C ABI's order (torchvision's module order): (name, Cin, Cout, (kh, kw), (sh, sw), (ph, pw))."""
    specs = list(STEM)
    for b in blocks().values():
        specs += b["units"]
    return specs


UNIT_SPECS = unit_specs()
assert len(UNIT_SPECS) == _lib.TTV_INCEPTION_UNITS


def conv_out(n: int, k: int, s: int, p: int) -> int:
    return (n + 2 * p - k) // s + 1


def spatial_sizes() -> "OrderedDict[str, int]":
    """Stage -> side of its (square) output for the 299 x 299 input: the stem's units and max-pools, then every block."""
    out = OrderedDict(input=INPUT_SIZE)
    n = INPUT_SIZE
    for i, (name, _cin, _cout, k, s, p) in enumerate(STEM):
        n = conv_out(n, k[0], s[0], p[0])
        out[name] = n
        if name in ("Conv2d_2b_3x3", "Conv2d_4a_3x3"):
            n = conv_out(n, 3, 2, 0)
            out[f"maxpool{1 if i == 2 else 2}"] = n
    for name, b in blocks().items():
        if b["kind"] in ("B", "D"):
            n = conv_out(n, 3, 2, 0)
        out[name] = n
    return out


def canonical_shapes() -> "OrderedDict[str, Tuple[int, ...]]":
    """torchvision's state-dict keys and shapes of everything the extractor reads, in order."""
    out = OrderedDict()
    for unit, cin, cout, k, _s, _p in UNIT_SPECS:
        out[f"{unit}.conv.weight"] = (cout, cin, k[0], k[1])
        for p in ("weight", "bias", "running_mean", "running_var"):
            out[f"{unit}.bn.{p}"] = (cout,)
    out["fc.weight"] = (CLASSES, FEATURES)
    out["fc.bias"] = (CLASSES,)
    return out


def _check_shapes(sd: Mapping[str, torch.Tensor]) -> None:
    for key, shape in canonical_shapes().items():
        if key not in sd:
            raise ValueError(f"inception_state_dict: '{key}' is missing")
        if tuple(sd[key].shape) != shape:
            raise ValueError(f"inception_state_dict: '{key}' has shape {tuple(sd[key].shape)}, Inception-v3 needs {shape}")


def inception_state_dict(path_or_mapping) -> "OrderedDict[str, torch.Tensor]":
    """torchvision's `inception_v3` checkpoint (a path, read with weights_only=True on the CPU) or a flat state dict with its keys
    (`<unit>.conv.weight`, `<unit>.bn.{weight,bias,running_mean,running_var}`, `fc.{weight,bias}`) -> the tensors the extractor
    reads, checked against the architecture, fp32 on the CPU.  `AuxLogits.*` and `num_batches_tracked` are ignored."""
    if isinstance(path_or_mapping, Mapping):
        sd = path_or_mapping
    else:
        sd = torch.load(os.fspath(path_or_mapping), map_location="cpu", weights_only=True)
        if not isinstance(sd, Mapping):
            raise ValueError(f"inception_state_dict: {path_or_mapping} holds a {type(sd).__name__}, not a state dict")
    _check_shapes(sd)
    return OrderedDict((key, sd[key].detach().to("cpu", torch.float32).contiguous()) for key in canonical_shapes())


def fold_unit(sd: Mapping[str, torch.Tensor], unit: str) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(weight image [K][Cout], scale [Cout], shift [Cout]) of one unit: eval BatchNorm folded in float64, rounded once to fp32.
    K runs over (dh, dw, ci), ci innermost (channels-last operands)."""
    w = sd[f"{unit}.conv.weight"]
    cout = w.shape[0]
    img = w.permute(2, 3, 1, 0).reshape(-1, cout).float().contiguous()
    scale = sd[f"{unit}.bn.weight"].double() / torch.sqrt(sd[f"{unit}.bn.running_var"].double() + BN_EPS)
    shift = sd[f"{unit}.bn.bias"].double() - sd[f"{unit}.bn.running_mean"].double() * scale
    return img, scale.float().contiguous(), shift.float().contiguous()


def _rows_dense(img: torch.Tensor) -> bool:
    return img.stride(2) == 1 and img.stride(1) == img.shape[2] and img.stride(0) >= img.shape[1] * img.shape[2]


class InceptionV3:
    """The extractor's folded weights and the C-ABI weight table.  Folded on the CPU at construction, uploaded to the device of the
    first images it sees.  Deliberately not an nn.Module: the weights are frozen and never part of a trainer checkpoint."""

    def __init__(self, state_dict: Mapping[str, torch.Tensor]):
        _check_shapes(state_dict)
        self.host = [fold_unit(state_dict, unit) for unit, *_ in UNIT_SPECS]
        self.host_fc = (state_dict["fc.weight"].float().t().contiguous(), state_dict["fc.bias"].float().contiguous())
        self.device = None
        self.tensors = []
        self.table = _lib.InceptionWeights()
        self._ws = None
        self._x = None

    @classmethod
    def from_file(cls, path) -> "InceptionV3":
        return cls(inception_state_dict(path))

    def to(self, device) -> "InceptionV3":
        device = torch.device(device)
        if self.device != device:
            self.tensors, self._ws, self._x = [], None, None
            for i, unit in enumerate(self.host):
                img, scale, shift = (t.to(device) for t in unit)
                self.tensors += [img, scale, shift]
                self.table.unit[i].w, self.table.unit[i].scale, self.table.unit[i].shift = img.data_ptr(), scale.data_ptr(), shift.data_ptr()
            fc_w, fc_b = (t.to(device) for t in self.host_fc)
            self.tensors += [fc_w, fc_b]
            self.table.fc_w, self.table.fc_b = fc_w.data_ptr(), fc_b.data_ptr()
            self.device = device
        return self

    def _buffers(self, n: int):
        need = _lib.lib().ttv_inception_workspace_bytes(n)
        if need < 0:
            _lib.check(1, "ttv_inception_workspace_bytes")
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        xn = n * INPUT_SIZE * INPUT_SIZE * 3
        if self._x is None or self._x.numel() < xn:
            self._x = None
            self._x = torch.empty(xn, dtype=torch.float32, device=self.device)
        return self._x, self._ws

    def _launch(self, items, acts, probs) -> None:
        """One call of up to TTV_MAX_CLIPS_PER_LAUNCH (image, clamp) items: a preprocessing launch per run of one clamp and dtype."""
        n = len(items)
        x, ws = self._buffers(n)
        stream = _lib.stream_ptr(self.device)
        at = 0
        while at < n:
            end = at
            while end < n and items[end][1] == items[at][1] and items[end][0].dtype == items[at][0].dtype:
                end += 1
            imgs = [im for im, _ in items[at:end]]
            dims = (C.c_int64 * (3 * len(imgs)))(*[v for im in imgs for v in (im.shape[1], im.shape[2], im.stride(0))])
            out = x.data_ptr() + at * INPUT_SIZE * INPUT_SIZE * 3 * 4
            rc = _lib.lib().ttv_inception_preprocess(_lib.ptr_array(imgs), dims, len(imgs), _lib.dtype_code(imgs[0].dtype),
                                                     int(bool(items[at][1])), out, stream)
            _lib.check(rc, "ttv_inception_preprocess")
            at = end
        rc = _lib.lib().ttv_inception_features(C.byref(self.table), x.data_ptr(), n, acts.data_ptr(), _lib.ptr(probs), ws.data_ptr(),
                                               ws.numel(), stream)
        _lib.check(rc, "ttv_inception_features")

    def features(self, groups: Sequence[Tuple[Sequence[torch.Tensor], bool]], want_probs: bool = True):
        """(acts [n][2048], probs [n][1000] or None) in fp32 on the device for the images of `groups` ((images [3, H, W], clamp)
        pairs), in order.  An image may be a frame `clip[:, t]` of a contiguous clip [3, T, H, W]: it is read in place."""
        items = []
        for images, clamp in groups:
            for im in images:
                _lib.require_gpu(im, "Inception features")
                if im.dim() != 3 or im.shape[0] != 3 or im.dtype not in (torch.bfloat16, torch.float32):
                    raise ValueError(f"Inception features: images must be [3, H, W] in bfloat16 or float32, got {tuple(im.shape)} {im.dtype}")
                items.append((im if _rows_dense(im) else im.contiguous(), clamp))
        if not items:
            raise ValueError("Inception features: no images")
        self.to(items[0][0].device)
        acts = torch.empty(len(items), FEATURES, dtype=torch.float32, device=self.device)
        probs = torch.empty(len(items), CLASSES, dtype=torch.float32, device=self.device) if want_probs else None
        step = _lib.TTV_MAX_CLIPS_PER_LAUNCH
        for c0 in range(0, len(items), step):
            self._launch(items[c0:c0 + step], acts[c0:c0 + step], None if probs is None else probs[c0:c0 + step])
        return acts, probs


# ---- statistics (float64, host) ---------------------------------------------------------------------------------------------
def _f64(a) -> np.ndarray:
    return np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64)


def calculate_activation_statistics(act) -> Tuple[np.ndarray, np.ndarray]:
    act = _f64(act)
    return np.mean(act, axis=0), np.cov(act, rowvar=False)     # ddof = 1


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps: float = 1e-6) -> float:
    """|mu1 - mu2|^2 + tr(S1) + tr(S2) - 2 tr(sqrtm(S1 S2)).  A non-finite square root is retried with eps on both diagonals; an
    imaginary part above 1e-3 on the diagonal is an error, a smaller one is dropped."""
    from scipy import linalg

    mu1, mu2 = np.atleast_1d(_f64(mu1)), np.atleast_1d(_f64(mu2))
    sigma1, sigma2 = np.atleast_2d(_f64(sigma1)), np.atleast_2d(_f64(sigma2))
    if mu1.shape != mu2.shape or sigma1.shape != sigma2.shape:
        raise ValueError(f"calculate_frechet_distance: statistics of different sizes, {mu1.shape} {sigma1.shape} and {mu2.shape} {sigma2.shape}")
    diff = mu1 - mu2
    covmean, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
    if not np.isfinite(covmean).all():
        offset = np.eye(sigma1.shape[0]) * eps
        covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError(f"Imaginary component {np.max(np.abs(covmean.imag))}")
        covmean = covmean.real
    return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean))


def calculate_fid(real_activations, fake_activations) -> float:
    """The Fréchet distance of the two feature sets' Gaussians; nan with fewer than 2 images on either side (no covariance)."""
    real, fake = _f64(real_activations), _f64(fake_activations)
    if real.shape[0] < 2 or fake.shape[0] < 2:
        return float("nan")
    mu1, sigma1 = calculate_activation_statistics(real)
    mu2, sigma2 = calculate_activation_statistics(fake)
    return calculate_frechet_distance(mu1, sigma1, mu2, sigma2)


def compute_inception_score(softmax_outputs) -> float:
    """exp(mean_x sum_y p(y|x) (log p(y|x) - log p(y))) over the rows of softmax outputs."""
    p_yx = _f64(softmax_outputs)
    p_y = np.mean(p_yx, axis=0)
    kl = p_yx * (np.log(p_yx) - np.log(p_y))
    return float(np.exp(np.mean(np.sum(kl, axis=1))))


def mmd_poly(X, Y, degree=2, gamma=None, coef0=0) -> float:
    """The reference's mmd_poly (sklearn's polynomial_kernel, gamma = 1 / dim by default): jedi.mmd_poly, float64."""
    return _mmd_poly(X, Y, degree=degree, gamma=gamma, coef0=coef0)


NO_WEIGHTS = ("FID / IS / MMD need Inception-v3's weights, which are never fetched over the network: pass a local file, e.g. "
              "torchvision's inception_v3_google-0cc3c7bd.pth or a state dict from metrics.inception_state_dict(), as "
              "MetricCalculator(inception_weights=path), EvalMetrics(config, inception_weights=path) or the config key "
              "training.eval.inception_weights")
INCEPTION_METRICS = ("fid", "is", "mmd")


def make_extractor(weights) -> InceptionV3:
    """An InceptionV3 from an InceptionV3, a state dict or a checkpoint path."""
    if isinstance(weights, InceptionV3):
        return weights
    if isinstance(weights, Mapping):
        return InceptionV3(inception_state_dict(weights))
    return InceptionV3.from_file(weights)


class InceptionStats:
    """The features of the real and the generated images so far and the three statistics on them (shared by MetricCalculator and
    EvalMetrics).  `names` decides what is extracted: activations of both sets for 'fid' / 'mmd', the generated set's softmax
    for 'is'."""

    def __init__(self, extractor: InceptionV3, names: Sequence[str]):
        self.extractor = extractor
        self.want_acts = "fid" in names or "mmd" in names
        self.want_probs = "is" in names
        self.reset()

    def reset(self) -> None:
        self.real_acts: List[torch.Tensor] = []
        self.fake_acts: List[torch.Tensor] = []
        self.fake_probs: List[torch.Tensor] = []

    @torch.no_grad()
    def update(self, real: Sequence[torch.Tensor], generated: Sequence[torch.Tensor], clamp_generated: bool = False) -> None:
        if len(real) != len(generated):
            raise ValueError(f"Inception metrics: {len(real)} real images, {len(generated)} generated")
        if not generated:
            return
        groups = [(list(generated), clamp_generated)] + ([(list(real), False)] if self.want_acts else [])
        acts, probs = self.extractor.features(groups, want_probs=self.want_probs)
        n = len(generated)
        if self.want_acts:
            self.fake_acts.append(acts[:n])
            self.real_acts.append(acts[n:])
        if self.want_probs:
            self.fake_probs.append(probs[:n])

    def features(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(real acts, generated acts, generated probs) so far, fp32 on the device (empty where nothing was asked for)."""
        def cat(parts, width):
            return torch.cat(parts) if parts else torch.empty(0, width)
        return cat(self.real_acts, FEATURES), cat(self.fake_acts, FEATURES), cat(self.fake_probs, CLASSES)

    def compute(self, name: str) -> float:
        real, fake, probs = self.features()
        if name == "is":
            return compute_inception_score(probs) if probs.shape[0] else float("nan")
        if fake.shape[0] == 0:
            return float("nan")
        if name == "fid":
            return calculate_fid(real, fake)
        return mmd_poly(_f64(real), _f64(fake), degree=2, coef0=0) * 100


class MetricCalculator(nn.Module):
    def __init__(self, metrics=("fid", "ssim", "psnr"), log_prefix: str = "eval", inception_weights=None):
        """inception_weights: a path (see inception_state_dict), a state dict or an InceptionV3.  See the module docstring for why
        'ssim' and 'psnr' are refused here."""
        super().__init__()
        for m in metrics:
            if m in ("ssim", "psnr"):
                raise NotImplementedError(f"MetricCalculator: '{m}' is not built here (torchmetrics' tuple data_range clamps both images and "
                                          "averages per image); use EvalMetrics for 'ssim' and 'psnr'")
            if m not in INCEPTION_METRICS:
                raise NotImplementedError(f"MetricCalculator: unknown metric '{m}'; built: {', '.join(INCEPTION_METRICS)}")
        if metrics and inception_weights is None:
            raise ValueError(NO_WEIGHTS)
        self.metrics = tuple(metrics)
        self.log_prefix = log_prefix
        # a plain object, not a submodule: no Inception tensors in state_dict()
        self.__dict__["stats"] = InceptionStats(make_extractor(inception_weights), self.metrics) if metrics else None

    def reset(self) -> None:
        if self.stats is not None:
            self.stats.reset()

    @torch.no_grad()
    def forward(self, real: Sequence[torch.Tensor], generated: Sequence[torch.Tensor]) -> None:   # lists of CHW images, range [-1, 1]
        if self.stats is not None:
            self.stats.update(real, generated)

    def gather(self) -> Dict[str, float]:
        order = [m for m in ("fid", "mmd", "is") if m in self.metrics]       # the reference's order
        return {f"{self.log_prefix}/{m}": self.stats.compute(m) for m in order}
