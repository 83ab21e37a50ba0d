"""JEDi on the GPU (reference model/metrics/jedi.py JEDiMetric, the 'jedi' entry of EvalMetrics).

The reference embeds every clip with V-JEPA ViT-L/16 and the SSv2 attentive probe's pooler, then reports 100 x the degree-2
polynomial-kernel MMD between the target and the reconstruction features (`mmd_poly`).  Here:
  * the weights come from local files only (`vjepa_state_dict`, `probe_state_dict`): upstream's vitl16.pth.tar and
    ssv2-probe.pth.tar, or flat canonical state dicts; nothing is fetched over the network and no `jepa/` checkout is needed;
  * get_feats runs in ttv_vjepa.hip: `ttv_jedi_preprocess` (clamp both videos, (v + 1) / 2, bicubic resize of the shorter edge to
    224, ImageNet normalisation, the last frame repeated up to 16) and `ttv_vjepa_features` (patch embed, 24 blocks, final norm,
    pooler - or the token mean for finetuned=False) at the precision of the reference's bf16-autocast validation step;
  * the features stay on the device until compute(), which evaluates `mmd_poly` in float64.  Like the reference, features are not
    gathered across ranks.
Shapes the reference cannot run are refused before any launch: non-square frames and T > 16 (the reference's
interpolate_pos_encoding calls F.interpolate(mode='tricubic'), which raises), and vit_huge (head_dim 80 is not built).
"""
from __future__ import annotations

import ctypes as C
import re
from collections import OrderedDict
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from ... import _lib

WIDTH = _lib.TTV_VJEPA_WIDTH
TOKENS = _lib.TTV_VJEPA_TOKENS
PATCH_K = _lib.TTV_VJEPA_PATCH_K
HEADS = 16
MLP = 4 * WIDTH
FRAMES = 16
DEPTH = 24

NO_WEIGHTS = ("JEDi needs the V-JEPA encoder's weights (and, with finetuned=True, the SSv2 probe's), which are never fetched over the "
              "network: pass local files such as upstream's vitl16.pth.tar and ssv2-probe.pth.tar as JEDiMetric(weights=..., probe=...), "
              "EvalMetrics(config, jedi_weights=..., jedi_probe=...) or the config keys training.eval.jedi_weights / jedi_probe")
NO_HUGE = ("JEDi with vit_huge is not built: its width 1280 has 16 heads of head_dim 80 and the attention kernels take head_dim 64 "
           "only; use jedi_jepa_model: vit_large")


def mmd_poly(X, Y, degree=2, gamma=None, coef0=0) -> float:
    """MMD with the polynomial kernel k(x, y) = (gamma <x, y> + coef0)^degree (reference jedi.py mmd_poly, sklearn's
    polynomial_kernel with gamma = 1 / dim by default), in float64.  For degree 2 and coef0 0 the kernel means are
    gamma^2 ||X^T X / n - Y^T Y / m||_F^2 (O(n d^2), no n x m kernel matrix); other arguments take the direct kernel means."""
    X = np.asarray(X.detach().cpu() if isinstance(X, torch.Tensor) else X, dtype=np.float64)
    Y = np.asarray(Y.detach().cpu() if isinstance(Y, torch.Tensor) else Y, dtype=np.float64)
    if X.ndim != 2 or Y.ndim != 2 or X.shape[1] != Y.shape[1]:
        raise ValueError(f"mmd_poly: X {X.shape} and Y {Y.shape} must be [n, d] and [m, d]")
    g = 1.0 / X.shape[1] if gamma is None else float(gamma)
    if degree == 2 and coef0 == 0:
        A = X.T @ X / X.shape[0]
        B = Y.T @ Y / Y.shape[0]
        return float(g * g * np.square(A - B).sum())

    def k(a, b):
        return (g * (a @ b.T) + coef0) ** degree

    return float(k(X, X).mean() + k(Y, Y).mean() - 2 * k(X, Y).mean())


# ---- state dicts ----------------------------------------------------------------------------------------------------------------

def encoder_shapes(depth: int = DEPTH, width: int = WIDTH) -> "OrderedDict[str, Tuple[int, ...]]":
    """Canonical key -> shape of upstream's VisionTransformer (src/models/vision_transformer.py) at ViT-L/16, 16 x 224^2."""
    out = OrderedDict()
    out["patch_embed.proj.weight"] = (width, 3, 2, 16, 16)
    out["patch_embed.proj.bias"] = (width,)
    out["pos_embed"] = (1, TOKENS, width)
    for i in range(depth):
        p = f"blocks.{i}."
        out[p + "norm1.weight"] = (width,)
        out[p + "norm1.bias"] = (width,)
        out[p + "attn.qkv.weight"] = (3 * width, width)
        out[p + "attn.qkv.bias"] = (3 * width,)
        out[p + "attn.proj.weight"] = (width, width)
        out[p + "attn.proj.bias"] = (width,)
        out[p + "norm2.weight"] = (width,)
        out[p + "norm2.bias"] = (width,)
        out[p + "mlp.fc1.weight"] = (4 * width, width)
        out[p + "mlp.fc1.bias"] = (4 * width,)
        out[p + "mlp.fc2.weight"] = (width, 4 * width)
        out[p + "mlp.fc2.bias"] = (width,)
    out["norm.weight"] = (width,)
    out["norm.bias"] = (width,)
    return out


def probe_shapes(width: int = WIDTH) -> "OrderedDict[str, Tuple[int, ...]]":
    """Canonical key -> shape of the pooler of upstream's AttentiveClassifier (src/models/attentive_pooler.py, depth 1)."""
    p = "pooler.cross_attention_block."
    out = OrderedDict()
    out["pooler.query_tokens"] = (1, 1, width)
    for name, shape in (("norm1.weight", (width,)), ("norm1.bias", (width,)), ("xattn.q.weight", (width, width)), ("xattn.q.bias", (width,)),
                        ("xattn.kv.weight", (2 * width, width)), ("xattn.kv.bias", (2 * width,)), ("xattn.proj.weight", (width, width)),
                        ("xattn.proj.bias", (width,)), ("norm2.weight", (width,)), ("norm2.bias", (width,)),
                        ("mlp.fc1.weight", (4 * width, width)), ("mlp.fc1.bias", (4 * width,)), ("mlp.fc2.weight", (width, 4 * width)),
                        ("mlp.fc2.bias", (width,))):
        out[p + name] = shape
    return out


def _load(path_or_sd, keys: Sequence[str]) -> Mapping[str, torch.Tensor]:
    if isinstance(path_or_sd, Mapping):
        sd = path_or_sd
    else:
        sd = torch.load(path_or_sd, map_location="cpu", weights_only=True)
    for k in keys:
        if isinstance(sd, Mapping) and k in sd and isinstance(sd[k], Mapping):
            return sd[k]
    return sd


def _strip(sd: Mapping[str, torch.Tensor], prefixes: Sequence[str]) -> Dict[str, torch.Tensor]:
    out = {}
    for k, v in sd.items():
        if not isinstance(v, torch.Tensor):
            continue
        changed = True
        while changed:
            changed = False
            for p in prefixes:
                if k.startswith(p):
                    k, changed = k[len(p):], True
        out[k] = v
    return out


def _check(sd: Mapping[str, torch.Tensor], shapes: Mapping[str, Tuple[int, ...]], what: str) -> "OrderedDict[str, torch.Tensor]":
    out = OrderedDict()
    for k, shape in shapes.items():
        if k not in sd:
            raise ValueError(f"{what}: key '{k}' is missing")
        if tuple(sd[k].shape) != tuple(shape):
            raise ValueError(f"{what}: '{k}' has shape {tuple(sd[k].shape)}, expected {tuple(shape)}")
        out[k] = sd[k].detach().float().contiguous()
    return out


def vjepa_state_dict(path_or_sd) -> "OrderedDict[str, torch.Tensor]":
    """The encoder of upstream's vitl16.pth.tar (key 'target_encoder', else 'encoder'; 'module.' / 'backbone.' prefixes stripped) or
    a flat canonical state dict (path or mapping) -> canonical fp32 state dict.  The depth is the number of blocks found."""
    sd = _strip(_load(path_or_sd, ("target_encoder", "encoder")), ("module.", "backbone."))
    if "pos_embed" not in sd:
        raise ValueError("V-JEPA weights: no 'pos_embed' in the checkpoint; the encoder's position table is a frozen parameter stored with "
                         "the weights (uniform_power sincos) and must be present")
    width = int(sd["pos_embed"].shape[-1])
    if width == 1280:
        raise NotImplementedError(NO_HUGE)
    depth = 1 + max((int(m.group(1)) for m in (re.match(r"blocks\.(\d+)\.", k) for k in sd) if m), default=-1)
    if depth < 1:
        raise ValueError("V-JEPA weights: key 'blocks.0.norm1.weight' is missing")
    return _check(sd, encoder_shapes(depth), "V-JEPA weights")


def probe_state_dict(path_or_sd) -> "OrderedDict[str, torch.Tensor]":
    """The pooler of upstream's ssv2-probe.pth.tar (key 'classifier', 'module.' stripped) or a flat canonical state dict -> canonical
    fp32 state dict (the classification head 'linear.*' is not used by JEDi and is dropped)."""
    sd = _strip(_load(path_or_sd, ("classifier",)), ("module.",))
    q = sd.get("pooler.query_tokens")
    if q is not None and int(q.shape[-1]) == 1280:
        raise NotImplementedError(NO_HUGE)
    return _check(sd, probe_shapes(), "V-JEPA probe")


def _bf16(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16)


def pooler_query(probe: Mapping[str, torch.Tensor]) -> torch.Tensor:
    """xattn.q(query_tokens) as bf16 autocast computes it: bf16 operands, a float64 (exact enough) sum, bf16 result [1024]."""
    p = "pooler.cross_attention_block.xattn.q."
    qt = _bf16(probe["pooler.query_tokens"].reshape(WIDTH)).double()
    w, b = _bf16(probe[p + "weight"]).double(), _bf16(probe[p + "bias"]).double()
    return (w @ qt + b).to(torch.bfloat16)


class VJEPA:
    """The encoder (and optionally the probe's pooler) as device tensors plus the C-ABI weight table.  Not an nn.Module: the weights
    are frozen and never part of a trainer checkpoint."""

    def __init__(self, encoder: Mapping[str, torch.Tensor], probe: Optional[Mapping[str, torch.Tensor]] = None):
        self.host = encoder
        self.probe = probe
        self.depth = 1 + max(int(k.split(".")[1]) for k in encoder if k.startswith("blocks."))
        self.device = None
        self.tensors: List[torch.Tensor] = []
        self.table = _lib.VjepaWeights()
        self._layers = None
        self._ws = None
        self._x = None

    def to(self, device) -> "VJEPA":
        device = torch.device(device)
        if self.device == device:
            return self
        self.tensors, self._ws, self._x = [], None, None
        keep = self.tensors

        def up(t: torch.Tensor, bf16: bool) -> int:
            d = (t.to(torch.bfloat16) if bf16 else t.float()).contiguous().to(device)
            keep.append(d)
            return d.data_ptr()

        e, t = self.host, self.table
        t.width, t.heads, t.depth = WIDTH, HEADS, self.depth
        t.patch_w = up(e["patch_embed.proj.weight"].reshape(WIDTH, PATCH_K), True)
        t.patch_b = up(e["patch_embed.proj.bias"], True)
        t.pos_embed = up(e["pos_embed"].reshape(TOKENS, WIDTH), False)
        self._layers = (_lib.VjepaLayer * self.depth)()
        for i in range(self.depth):
            p, L = f"blocks.{i}.", self._layers[i]
            L.norm1_w, L.norm1_b = up(e[p + "norm1.weight"], False), up(e[p + "norm1.bias"], False)
            L.qkv_w, L.qkv_b = up(e[p + "attn.qkv.weight"], True), up(e[p + "attn.qkv.bias"], True)
            L.proj_w, L.proj_b = up(e[p + "attn.proj.weight"], True), up(e[p + "attn.proj.bias"], True)
            L.norm2_w, L.norm2_b = up(e[p + "norm2.weight"], False), up(e[p + "norm2.bias"], False)
            L.fc1_w, L.fc1_b = up(e[p + "mlp.fc1.weight"], True), up(e[p + "mlp.fc1.bias"], True)
            L.fc2_w, L.fc2_b = up(e[p + "mlp.fc2.weight"], True), up(e[p + "mlp.fc2.bias"], True)
        t.layers = C.cast(self._layers, C.POINTER(_lib.VjepaLayer))
        t.norm_w, t.norm_b = up(e["norm.weight"], False), up(e["norm.bias"], False)
        if self.probe is not None:
            q, p = self.probe, "pooler.cross_attention_block."
            t.query_tokens = up(q["pooler.query_tokens"].reshape(WIDTH), False)
            t.pool_q = up(pooler_query(q), True)
            t.pool_norm1_w, t.pool_norm1_b = up(q[p + "norm1.weight"], False), up(q[p + "norm1.bias"], False)
            t.pool_kv_w, t.pool_kv_b = up(q[p + "xattn.kv.weight"], True), up(q[p + "xattn.kv.bias"], True)
            t.pool_proj_w, t.pool_proj_b = up(q[p + "xattn.proj.weight"], True), up(q[p + "xattn.proj.bias"], True)
            t.pool_norm2_w, t.pool_norm2_b = up(q[p + "norm2.weight"], False), up(q[p + "norm2.bias"], False)
            t.pool_fc1_w, t.pool_fc1_b = up(q[p + "mlp.fc1.weight"], True), up(q[p + "mlp.fc1.bias"], True)
            t.pool_fc2_w, t.pool_fc2_b = up(q[p + "mlp.fc2.weight"], True), up(q[p + "mlp.fc2.bias"], True)
        self.device = device
        return self

    def _buffers(self, n: int):
        need = _lib.lib().ttv_vjepa_workspace_bytes(n)
        if need < 0:
            _lib.check(1, "ttv_vjepa_workspace_bytes")
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        if self._x is None or self._x.shape[0] < n * TOKENS:
            self._x = None
            self._x = torch.empty(n * TOKENS, PATCH_K, dtype=torch.bfloat16, device=self.device)
        return self._x, self._ws

    def preprocess(self, clips: Sequence[torch.Tensor], out: torch.Tensor) -> None:
        """ttv_jedi_preprocess of up to TTV_MAX_CLIPS_PER_LAUNCH clips [3, T, S, S] of one dtype into out (bf16 patch rows)."""
        check_clips(clips)
        clips = [c.contiguous() for c in clips]
        dims = (C.c_int32 * (4 * len(clips)))(*[int(d) for c in clips for d in c.shape])
        rc = _lib.lib().ttv_jedi_preprocess(_lib.ptr_array(clips), dims, len(clips), _lib.dtype_code(clips[0].dtype), out.data_ptr(),
                                            _lib.stream_ptr(clips[0].device))
        _lib.check(rc, "ttv_jedi_preprocess")

    def features(self, groups: Sequence[Sequence[torch.Tensor]], finetuned: bool = True) -> torch.Tensor:
        """[n][1024] fp32 features of the clips of `groups` (lists of [3, T, S, S] clips, each list one dtype; n <=
        TTV_MAX_CLIPS_PER_LAUNCH in all), in order."""
        if finetuned and self.probe is None:
            raise ValueError("VJEPA: finetuned features need the probe's pooler")
        n = sum(len(g) for g in groups)
        first = next(g[0] for g in groups if g)
        _lib.require_gpu(first, "JEDi")
        self.to(first.device)
        x, ws = self._buffers(n)
        at = 0
        for g in groups:
            if g:
                self.preprocess(g, x[at * TOKENS:])
                at += len(g)
        feats = torch.empty(n, WIDTH, dtype=torch.float32, device=self.device)
        rc = _lib.lib().ttv_vjepa_features(C.byref(self.table), x.data_ptr(), n, feats.data_ptr(), int(finetuned), ws.data_ptr(), ws.numel(),
                                           _lib.stream_ptr(self.device))
        _lib.check(rc, "ttv_vjepa_features")
        return feats


def check_clips(clips: Sequence[torch.Tensor]) -> None:
    """Raise ValueError for a clip the reference's get_feats cannot embed (before anything is launched)."""
    if not clips:
        return
    dt = clips[0].dtype
    for c in clips:
        _lib.require_gpu(c, "JEDi")
        if c.dim() != 4 or c.shape[0] != 3 or c.dtype != dt:
            raise ValueError(f"JEDi: clips must be [3, T, H, W] of one dtype, got {tuple(c.shape)} {c.dtype}")
        if c.dtype not in (torch.bfloat16, torch.float32):
            raise ValueError(f"JEDi: clips must be bfloat16 or float32, got {c.dtype}")
        _t, h, w = (int(v) for v in c.shape[1:])
        if h != w:
            raise ValueError(f"JEDi: frames of {h} x {w} are not square; the reference resizes the shorter edge to 224 and its "
                             "interpolate_pos_encoding then calls F.interpolate(mode='tricubic'), which raises")
        if not 1 <= _t <= FRAMES:
            raise ValueError(f"JEDi: a clip of {_t} frames; the reference pads to 16 and cannot interpolate its position embedding "
                             "to more (F.interpolate(mode='tricubic') raises)")


class JEDiMetric(nn.Module):
    PAIRS_PER_CHUNK = _lib.TTV_MAX_CLIPS_PER_LAUNCH // 2

    def __init__(self, model_name: str = "vit_large", finetuned: bool = True, weights=None, probe=None, device="cuda:0"):
        """weights: vitl16.pth.tar, a canonical state dict (path or mapping) or a VJEPA; probe: ssv2-probe.pth.tar or a canonical
        state dict (needed when finetuned).  The weights go to the device of the first update's clips (`device` is kept for the
        reference's signature)."""
        super().__init__()
        if model_name == "vit_huge":
            raise NotImplementedError(NO_HUGE)
        if model_name != "vit_large":
            raise ValueError(f"JEDi: model_name '{model_name}'; the reference knows vit_large and vit_huge")
        if weights is None or (finetuned and probe is None and not isinstance(weights, VJEPA)):
            raise ValueError(NO_WEIGHTS)
        if isinstance(weights, VJEPA):
            model = weights
        else:
            model = VJEPA(vjepa_state_dict(weights), probe_state_dict(probe) if finetuned else None)
        if finetuned and model.probe is None:
            raise ValueError(NO_WEIGHTS)
        self.model = model            # a plain object, not a submodule: no V-JEPA tensors in state_dict()
        self.finetuned = finetuned
        self.frames_per_clip = FRAMES
        self.metric_name = "jedi"
        self.reset()

    def reset(self) -> None:
        self.recon_feats = []
        self.target_feats = []

    @torch.no_grad()
    def update_clips(self, recon: Sequence[torch.Tensor], target: Sequence[torch.Tensor]) -> None:
        """Ragged clips [3, T, S, S], range [-1, 1] (both are clamped, as get_feats does)."""
        if len(recon) != len(target):
            raise ValueError(f"JEDi: {len(recon)} reconstructions, {len(target)} targets")
        check_clips(list(recon))
        check_clips(list(target))
        for c0 in range(0, len(recon), self.PAIRS_PER_CHUNK):
            r, t = list(recon[c0:c0 + self.PAIRS_PER_CHUNK]), list(target[c0:c0 + self.PAIRS_PER_CHUNK])
            f = self.model.features([r, t], self.finetuned)
            self.recon_feats.append(f[:len(r)])
            self.target_feats.append(f[len(r):])

    @torch.no_grad()
    def update(self, recon: torch.Tensor, target: torch.Tensor) -> None:   # BCTHW, range [-1, 1]
        self.update_clips(list(recon), list(target))

    def features(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(recon, target) features so far, [N][1024] fp32 on the device."""
        if not self.recon_feats:
            e = torch.empty(0, WIDTH)
            return e, e
        return torch.cat(self.recon_feats), torch.cat(self.target_feats)

    def compute(self) -> float:
        recon, target = self.features()
        if recon.shape[0] == 0:
            return float("nan")
        return mmd_poly(target.cpu().double().numpy(), recon.cpu().double().numpy(), degree=2, coef0=0) * 100

    def forward(self):
        pass
