"""Mirror of the reference's FVD metric (model/metrics/fvd.py) on the HIP path (csrc/ttv_i3d.hip).

Same names: `FVDCalculator` with `update(recon, target)`, `compute() -> float` and `reset()`; `compute_stats` and
`frechet_distance` in float64 numpy with scipy's sqrtm, as the reference defines them.

What `update` computes per clip, as the reference does (fvd.py `update`):
  * `F.interpolate(v, size=(v.shape[1], 224, 224), mode='trilinear', align_corners=False)` on BCTHW clips.  `v.shape[1]` is the
    channel count C = 3, not T, so the time axis of every clip is resampled to 3 frames whatever its length.  This looks like an
    upstream slip, but it defines the statistic the reference logs, so it is reproduced exactly (there is no option to change it).
  * `repeat_to_10_frames`: the last frame is repeated up to 10 frames, so the detector input is always [B, 3, 10, 224, 224].
  * the I3D detector with `rescale=False, resize=False, return_features=True`: the 400 Kinetics logits before the softmax,
    averaged over time.
The preprocessing and the whole network run in HIP kernels in fp32 (the reference runs the detector in fp32).  Features stay on
the device until `compute()`; they are not gathered across ranks (neither are the reference's).

Differences from the reference, all deliberate:
  * the detector's weights never come from the network.  `FVDCalculator(detector=path)` takes the reference's own
    `i3d_torchscript.pt` (read on the CPU with torch.jit.load) or a `torch.save`d state dict with the canonical keys below; see
    `i3d_state_dict`.  Without a detector it raises and says how to give one.
  * updates are processed in chunks of up to TTV_MAX_CLIPS_PER_LAUNCH / 2 clip pairs, in a workspace this object owns.
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

BN_EPS = 1e-3
INPUT_FRAMES, INPUT_SIZE = 10, 224

# Inception blocks and their branch widths (b0, b1a, b1b, b2a, b2b, b3b)
INCEPTION = OrderedDict([
    ("Mixed_3b", (64, 96, 128, 16, 32, 32)), ("Mixed_3c", (128, 128, 192, 32, 96, 64)),
    ("Mixed_4b", (192, 96, 208, 16, 48, 64)), ("Mixed_4c", (160, 112, 224, 24, 64, 64)),
    ("Mixed_4d", (128, 128, 256, 24, 64, 64)), ("Mixed_4e", (112, 144, 288, 32, 64, 64)),
    ("Mixed_4f", (256, 160, 320, 32, 128, 128)), ("Mixed_5b", (256, 160, 320, 32, 128, 128)),
    ("Mixed_5c", (384, 192, 384, 48, 128, 128)),
])
BRANCHES = ("b0", "b1a", "b1b", "b2a", "b2b", "b3b")


def conv_specs() -> List[Tuple[str, int, int, int]]:
    """The 58 convolutions in the C ABI's order: (unit name, Cin, Cout, kernel size).  The last one is the logits (bias, no BN)."""
    specs = [("Conv3d_1a_7x7", 3, 64, 7), ("Conv3d_2b_1x1", 64, 64, 1), ("Conv3d_2c_3x3", 64, 192, 3)]
    cin = 192
    for name, (b0, b1a, b1b, b2a, b2b, b3b) in INCEPTION.items():
        specs += [(f"{name}.b0", cin, b0, 1), (f"{name}.b1a", cin, b1a, 1), (f"{name}.b1b", b1a, b1b, 3),
                  (f"{name}.b2a", cin, b2a, 1), (f"{name}.b2b", b2a, b2b, 3), (f"{name}.b3b", cin, b3b, 1)]
        cin = b0 + b1b + b2b + b3b
    specs.append(("logits", cin, 400, 1))
    return specs


CONV_SPECS = conv_specs()
assert len(CONV_SPECS) == _lib.TTV_I3D_CONVS


def same_pad(n: int, k: int, s: int) -> Tuple[int, int, int]:
    """TF 'SAME': (out, front pad, back pad) with out = ceil(n / s), pad = max((out - 1) s + k - n, 0), front = pad // 2."""
    out = -(-n // s)
    pad = max((out - 1) * s + k - n, 0)
    return out, pad // 2, pad - pad // 2


def canonical_shapes() -> "OrderedDict[str, Tuple[int, ...]]":
    """Canonical state-dict keys and shapes, in order (BN `weight` included: it is optional in a checkpoint, see i3d_state_dict)."""
    out = OrderedDict()
    for unit, cin, cout, k in CONV_SPECS:
        if unit == "logits":
            out["logits.conv3d.weight"] = (cout, cin, 1, 1, 1)
            out["logits.conv3d.bias"] = (cout,)
            continue
        out[f"{unit}.conv3d.weight"] = (cout, cin, k, k, k)
        for p in ("weight", "bias", "running_mean", "running_var"):
            out[f"{unit}.bn.{p}"] = (cout,)
    return out


def _is_optional(key: str) -> bool:
    return key.endswith(".bn.weight")


def _from_names(sd: Mapping[str, torch.Tensor]) -> Dict[str, torch.Tensor] | None:
    """Map by name, allowing one common prefix; None when the canonical names are not there."""
    anchor = "Conv3d_1a_7x7.conv3d.weight"
    prefixes = [k[: -len(anchor)] for k in sd if k.endswith(anchor)]
    for pre in prefixes:
        out = {}
        for key in canonical_shapes():
            if pre + key in sd:
                out[key] = sd[pre + key]
            elif not _is_optional(key):
                break
        else:
            return out
    return None


def _from_shapes(tensors: Sequence[Tuple[str, torch.Tensor]]) -> Dict[str, torch.Tensor]:
    """Map the ordered floating tensors of a checkpoint whose names differ onto the canonical keys by their shapes.  Per unit: the
    5-D conv weight, then 3 (bias, running_mean, running_var) or 4 (weight first) vectors of Cout; the logits: weight, bias."""
    seq = [(n, t) for n, t in tensors if t.is_floating_point() and t.dim() >= 1]
    out, i = {}, 0

    def refuse(what):
        got = f"'{seq[i][0]}' of shape {tuple(seq[i][1].shape)}" if i < len(seq) else "the end of the checkpoint"
        raise ValueError(f"i3d_state_dict: the checkpoint does not match the I3D layout: expected {what}, found {got} "
                         f"(tensor {i} of {len(seq)})")

    for unit, cin, cout, k in CONV_SPECS:
        wshape = (cout, cin, 1, 1, 1) if unit == "logits" else (cout, cin, k, k, k)
        if i >= len(seq) or tuple(seq[i][1].shape) != wshape:
            refuse(f"{unit}.conv3d.weight {wshape}")
        out[f"{unit}.conv3d.weight"] = seq[i][1]
        i += 1
        j = i
        while j < len(seq) and tuple(seq[j][1].shape) == (cout,) and j - i < 4:
            j += 1
        vecs = [t for _, t in seq[i:j]]
        if unit == "logits":
            if len(vecs) != 1:
                refuse(f"logits.conv3d.bias ({cout},) and nothing after it")
            out["logits.conv3d.bias"] = vecs[0]
        elif len(vecs) == 4:
            for p, t in zip(("weight", "bias", "running_mean", "running_var"), vecs):
                out[f"{unit}.bn.{p}"] = t
        elif len(vecs) == 3:
            for p, t in zip(("bias", "running_mean", "running_var"), vecs):
                out[f"{unit}.bn.{p}"] = t
        else:
            refuse(f"3 or 4 BatchNorm vectors ({cout},) after {unit}.conv3d.weight")
        i = j
    if i != len(seq):
        refuse("the end of the checkpoint after logits.conv3d.bias")
    return out


def _check_shapes(sd: Mapping[str, torch.Tensor]) -> None:
    for key, shape in canonical_shapes().items():
        if key not in sd:
            if _is_optional(key):
                continue
            raise ValueError(f"i3d_state_dict: '{key}' is missing")
        if tuple(sd[key].shape) != shape:
            raise ValueError(f"i3d_state_dict: '{key}' has shape {tuple(sd[key].shape)}, the I3D layout needs {shape}")


def i3d_state_dict(path) -> "OrderedDict[str, torch.Tensor]":
    """The canonical I3D state dict from `path`: a torch.save'd state dict with the canonical keys (`Conv3d_1a_7x7.conv3d.weight`,
    `Conv3d_1a_7x7.bn.{weight,bias,running_mean,running_var}`, ..., `Mixed_3b.b0.*` .. `Mixed_5c.b3b.*`,
    `logits.conv3d.{weight,bias}`), or a TorchScript archive such as the reference's `i3d_torchscript.pt` (loaded on the CPU).
    An archive is mapped by name first (a common prefix allowed), then by the ordered sequence of tensor shapes, which must match
    the architecture exactly; otherwise the first disagreement is named.  A missing BN `weight` means scale 1 (TF's I3D
    BatchNorm has no scale term).  Tensors come back as float32 on the CPU."""
    path = os.fspath(path)
    try:
        obj = torch.load(path, map_location="cpu", weights_only=True)
        named = list(obj.items()) if isinstance(obj, Mapping) else None
    except Exception:
        named = None
    if named is None:
        mod = torch.jit.load(path, map_location="cpu")
        named = list(mod.state_dict().items())
    sd = dict(named)
    mapped = _from_names(sd)
    if mapped is None:
        mapped = _from_shapes(named)
    _check_shapes(mapped)
    out = OrderedDict()
    for key in canonical_shapes():
        if key in mapped:
            out[key] = mapped[key].detach().to("cpu", torch.float32).contiguous()
    return out


def fold_unit(sd: Mapping[str, torch.Tensor], unit: str) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(weight image [K][Cout], scale [Cout], shift [Cout]) of one unit: eval BatchNorm folded in float64, rounded once to fp32.
    K runs over (dt, dh, dw, ci), ci innermost (channels-last operands)."""
    w = sd[f"{unit}.conv3d.weight"].double()
    cout = w.shape[0]
    img = w.permute(2, 3, 4, 1, 0).reshape(-1, cout).float().contiguous()
    if unit == "logits":
        return img, torch.ones(cout, dtype=torch.float32), sd["logits.conv3d.bias"].float().contiguous()
    gamma = sd[f"{unit}.bn.weight"].double() if f"{unit}.bn.weight" in sd else torch.ones(cout, dtype=torch.float64)
    scale = gamma / torch.sqrt(sd[f"{unit}.bn.running_var"].double() + BN_EPS)
    shift = sd[f"{unit}.bn.bias"].double() - sd[f"{unit}.bn.running_mean"].double() * scale
    return img, scale.float().contiguous(), shift.float().contiguous()


class I3D:
    """The detector's folded weights and the C-ABI weight table.  Folded on the CPU at construction, uploaded to the device of the
    first clips it sees.  Deliberately not an nn.Module: the weights are frozen and never part of a trainer checkpoint (the
    reference keeps its detector in a plain dict)."""

    def __init__(self, state_dict: Mapping[str, torch.Tensor]):
        _check_shapes(state_dict)
        self.host = [fold_unit(state_dict, unit) for unit, _cin, _cout, _k in CONV_SPECS]
        self.device = None
        self.tensors = []
        self.table = _lib.I3dWeights()
        self._ws = None
        self._x = None

    @classmethod
    def from_file(cls, path) -> "I3D":
        return cls(i3d_state_dict(path))

    def to(self, device) -> "I3D":
        device = torch.device(device)
        if self.device != device:
            self.tensors, self._ws, self._x = [], None, None
            for i, unit in enumerate(self.host):
                img, scale, shift = (t.to(device) for t in unit)
                self.tensors += [img, scale, shift]
                self.table.w[i], self.table.scale[i], self.table.shift[i] = img.data_ptr(), scale.data_ptr(), shift.data_ptr()
            self.device = device
        return self

    def _buffers(self, n: int):
        need = _lib.lib().ttv_i3d_workspace_bytes(n)
        if need < 0:
            _lib.check(1, "ttv_i3d_workspace_bytes")
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        xn = n * INPUT_FRAMES * INPUT_SIZE * INPUT_SIZE * 3
        if self._x is None or self._x.numel() < xn:
            self._x = None
            self._x = torch.empty(xn, dtype=torch.float32, device=self.device)
        return self._x, self._ws

    def features(self, groups: Sequence[Tuple[Sequence[torch.Tensor], bool]]) -> torch.Tensor:
        """[n][400] fp32 features of the clips of `groups` ((clips [3, T, H, W], clamp) pairs, n <= TTV_MAX_CLIPS_PER_LAUNCH in
        all), in order: preprocessing (one launch per group) and the network (one call)."""
        n = sum(len(c) for c, _ in groups)
        first = next(c[0] for c, _ in groups if c)
        _lib.require_gpu(first, "FVD")
        self.to(first.device)
        x, ws = self._buffers(n)
        stream = _lib.stream_ptr(self.device)
        at = 0
        for clips, clamp in groups:
            if not clips:
                continue
            dt = clips[0].dtype
            for c in clips:
                _lib.require_gpu(c, "FVD")
                if c.dim() != 4 or c.shape[0] != 3 or c.dtype != dt:
                    raise ValueError(f"FVD: clips must be [3, T, H, W] of one dtype, got {tuple(c.shape)} {c.dtype}")
            clips = [c.contiguous() for c in clips]
            dims = (C.c_int32 * (4 * len(clips)))(*[int(d) for c in clips for d in c.shape])
            out = x.data_ptr() + at * INPUT_FRAMES * INPUT_SIZE * INPUT_SIZE * 3 * 4
            rc = _lib.lib().ttv_fvd_preprocess(_lib.ptr_array(clips), dims, len(clips), _lib.dtype_code(dt), int(clamp), out, stream)
            _lib.check(rc, "ttv_fvd_preprocess")
            at += len(clips)
        feats = torch.empty(n, _lib.TTV_I3D_FEATURES, dtype=torch.float32, device=self.device)
        rc = _lib.lib().ttv_i3d_features(C.byref(self.table), x.data_ptr(), n, feats.data_ptr(), ws.data_ptr(), ws.numel(), stream)
        _lib.check(rc, "ttv_i3d_features")
        return feats


def compute_stats(feats: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    mu = feats.mean(axis=0)                    # [d]
    sigma = np.cov(feats, rowvar=False)        # [d, d], ddof = 1
    return mu, sigma


def frechet_distance(feats_fake: np.ndarray, feats_real: np.ndarray) -> float:
    """|mu_f - mu_r|^2 + tr(S_f + S_r - 2 sqrtm(S_f S_r)) (real part); the mean term alone for a single clip."""
    from scipy.linalg import sqrtm

    mu_gen, sigma_gen = compute_stats(feats_fake)
    mu_real, sigma_real = compute_stats(feats_real)
    m = np.square(mu_gen - mu_real).sum()
    if feats_fake.shape[0] > 1:
        s, _ = sqrtm(np.dot(sigma_gen, sigma_real), disp=False)
        fid = np.real(m + np.trace(sigma_gen + sigma_real - s * 2))
    else:
        fid = np.real(m)
    return float(fid)


NO_DETECTOR = ("FVD needs the I3D detector's weights, which are never fetched over the network: pass a local file, e.g. the "
               "reference's model/metrics/i3d_torchscript.pt or a state dict from fvd.i3d_state_dict(), as "
               "FVDCalculator(detector=path), EvalMetrics(config, fvd_detector=path) or the config key training.eval.fvd_detector")


class FVDCalculator(nn.Module):
    PAIRS_PER_CHUNK = _lib.TTV_MAX_CLIPS_PER_LAUNCH // 2

    def __init__(self, detector=None, device="cuda:0"):
        """detector: a path (see i3d_state_dict), a canonical state dict or an I3D.  The weights go to the device of the first
        update's clips (`device` is kept for the reference's signature)."""
        super().__init__()
        if detector is None:
            raise ValueError(NO_DETECTOR)
        if isinstance(detector, I3D):
            det = detector
        elif isinstance(detector, Mapping):
            det = I3D(detector)
        else:
            det = I3D.from_file(detector)
        self.detector = det       # a plain object, not a submodule: no detector tensors in state_dict()
        self.metric_name = "fvd"
        self.reset()

    def reset(self) -> None:
        self.fvd_fake_activations = []
        self.fvd_real_activations = []

    @torch.no_grad()
    def update_clips(self, recon: Sequence[torch.Tensor], target: Sequence[torch.Tensor], clamp_recon: bool = False) -> None:
        """Ragged clips [3, T, H, W]; clamp_recon clamps the reconstructions to [-1, 1] first (what EvalMetrics does)."""
        if len(recon) != len(target):
            raise ValueError(f"FVD: {len(recon)} reconstructions, {len(target)} targets")
        for c0 in range(0, len(recon), self.PAIRS_PER_CHUNK):
            r, t = list(recon[c0:c0 + self.PAIRS_PER_CHUNK]), list(target[c0:c0 + self.PAIRS_PER_CHUNK])
            f = self.detector.features([(r, clamp_recon), (t, False)])
            self.fvd_fake_activations.append(f[:len(r)])
            self.fvd_real_activations.append(f[len(r):])

    @torch.no_grad()
    def update(self, recon: torch.Tensor, target: torch.Tensor) -> None:   # BCTHW, range [-1, 1]
        self.update_clips(list(recon), list(target))

    def features(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(fake, real) features so far, [N][400] fp32 on the device."""
        if not self.fvd_fake_activations:
            e = torch.empty(0, _lib.TTV_I3D_FEATURES)
            return e, e
        return torch.cat(self.fvd_fake_activations), torch.cat(self.fvd_real_activations)

    def compute(self) -> float:
        fake, real = self.features()
        if fake.shape[0] == 0:
            return float("nan")
        return frechet_distance(fake.cpu().double().numpy(), real.cpu().double().numpy())

    def forward(self):
        pass
