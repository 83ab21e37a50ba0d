"""Mirror of the reference's `LPIPS` perceptual metric (model/metrics/lpips_gram.py) on the HIP path (csrc/ttv_lpips.hip).

Same submodule names and state-dict keys (`scaling_layer.shift/scale`, `net.slice1.0.weight` .. `net.slice5.28.bias`,
`lin0.model.1.weight` .. `lin4.model.1.weight`), same `forward(input, target) -> (lpips[B], gram[B])`.  The VGG16 trunk, both heads
and the input-gradient backward run in HIP kernels; gradients flow into `input` only (weights are frozen, as in the reference).

Differences from the reference, all deliberate:
  * weights never come from the network.  `LPIPS.from_file(path)` loads a state dict with the reference module's keys, and
    `lpips_state_dict(vgg16_path, lin_path)` composes one from torchvision's `vgg16-397923af.pth` and the LPIPS `vgg.pth`.
    `LPIPS()` alone holds uninitialised weights until one of these (or `load_state_dict`) fills them.
  * the lin layers always use eval semantics (no dropout).  The reference builds the module with `.eval()`; whether a trainer's
    `train()` later switches its dropouts back on depends on the Lightning version.  Here `train()` changes nothing.
  * inputs must be bf16 or fp32 CUDA tensors [B, 3, H, W] with H and W multiples of 16; anything else raises.

`LPIPS.frame_distances(recon_clips, target_clips)` is the evaluation path (EvalMetrics 'lpips'): per-frame values of whole frames
of CTHW clips, any H and W in 16 .. 2048 (the max-pools floor, as torch's), no tape, no autograd node.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Sequence

import torch
import torch.nn as nn

from ... import _lib

CHNS = [64, 128, 256, 512, 512]
# torchvision vgg16().features: (index, kind); conv layers carry weight + bias
VGG_FEATURES = [(0, "conv", 3, 64), (1, "relu"), (2, "conv", 64, 64), (3, "relu"), (4, "pool"),
                (5, "conv", 64, 128), (6, "relu"), (7, "conv", 128, 128), (8, "relu"), (9, "pool"),
                (10, "conv", 128, 256), (11, "relu"), (12, "conv", 256, 256), (13, "relu"), (14, "conv", 256, 256), (15, "relu"),
                (16, "pool"),
                (17, "conv", 256, 512), (18, "relu"), (19, "conv", 512, 512), (20, "relu"), (21, "conv", 512, 512), (22, "relu"),
                (23, "pool"),
                (24, "conv", 512, 512), (25, "relu"), (26, "conv", 512, 512), (27, "relu"), (28, "conv", 512, 512), (29, "relu")]
SLICES = [(0, 4), (4, 9), (9, 16), (16, 23), (23, 30)]
CONV_INDICES = [f[0] for f in VGG_FEATURES if f[1] == "conv"]
EVAL_WORKSPACE_BYTES = 1 << 30      # default budget of frame_distances: 127 bf16 frame pairs of 128 x 128 in one pass
EVAL_MAX_FRAMES = 2048              # frames of one pass at most (ttv_lpips_eval_workspace_bytes)


def _slice_of(index: int) -> int:
    for k, (a, b) in enumerate(SLICES):
        if a <= index < b:
            return k + 1
    raise ValueError(index)


class ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor([-0.030, -0.088, -0.188])[None, :, None, None])
        self.register_buffer("scale", torch.tensor([0.458, 0.448, 0.450])[None, :, None, None])


class NetLinLayer(nn.Module):
    """The reference's 1x1 conv head layer with its Dropout slot (keys `model.1.weight`); applied without dropout."""

    def __init__(self, chn_in: int, chn_out: int = 1, use_dropout: bool = True):
        super().__init__()
        layers = [nn.Dropout()] if use_dropout else []
        layers += [nn.Conv2d(chn_in, chn_out, 1, stride=1, padding=0, bias=False)]
        self.model = nn.Sequential(*layers)


class Vgg16Features(nn.Module):
    """VGG16 features[0:30] split into the reference's slice1 .. slice5 (module names are the torchvision indices)."""

    def __init__(self):
        super().__init__()
        for k in range(5):
            setattr(self, f"slice{k + 1}", nn.Sequential())
        for f in VGG_FEATURES:
            if f[1] == "conv":
                m = nn.Conv2d(f[2], f[3], kernel_size=3, padding=1)
            elif f[1] == "relu":
                m = nn.ReLU(inplace=True)
            else:
                m = nn.MaxPool2d(kernel_size=2, stride=2)
            getattr(self, f"slice{_slice_of(f[0])}").add_module(str(f[0]), m)

    def convs(self):
        return [getattr(self, f"slice{_slice_of(i)}")._modules[str(i)] for i in CONV_INDICES]


def lpips_state_dict(vgg16_path: str, lin_path: str) -> Dict[str, torch.Tensor]:
    """A state dict with the reference LPIPS keys from the two upstream files: torchvision's VGG16 checkpoint
    (`features.{i}.weight/bias`) and the LPIPS lin weights (`lin{k}.model.1.weight`).  Files are read with torch.load on the CPU."""
    vgg = torch.load(vgg16_path, map_location="cpu", weights_only=True)
    lin = torch.load(lin_path, map_location="cpu", weights_only=True)
    out: Dict[str, torch.Tensor] = OrderedDict()
    out["scaling_layer.shift"] = torch.tensor([-0.030, -0.088, -0.188])[None, :, None, None]
    out["scaling_layer.scale"] = torch.tensor([0.458, 0.448, 0.450])[None, :, None, None]
    for i in CONV_INDICES:
        for p in ("weight", "bias"):
            src = f"features.{i}.{p}"
            if src not in vgg:
                raise KeyError(f"{vgg16_path}: no '{src}' (expected torchvision's vgg16 state dict)")
            out[f"net.slice{_slice_of(i)}.{i}.{p}"] = vgg[src].float()
    for k in range(5):
        src = f"lin{k}.model.1.weight"
        if src not in lin:
            raise KeyError(f"{lin_path}: no '{src}' (expected the LPIPS vgg.pth lin weights)")
        out[src] = lin[src].float()
    return out


def _pack_images(w: torch.Tensor, dtype: torch.dtype, mfma: bool):
    """Forward and dgrad weight images of one 3x3 conv (include/titok_hip.h, ttv_lpips_weights)."""
    cout, cin = w.shape[0], w.shape[1]
    fwd = w.permute(2, 3, 1, 0).reshape(9, cin, cout)                 # [t][ci][co]
    dgr = w.flip(2, 3).permute(2, 3, 0, 1).reshape(9, cout, cin)      # [t][co][ci] = W[co][ci][2-kh][2-kw]
    if mfma:
        fwd = fwd.reshape(9, cin // 32, 32, cout).permute(1, 0, 3, 2)  # [ci/32][t][co][32]
        dgr = dgr.reshape(9, cout // 32, 32, cin).permute(1, 0, 3, 2)  # [co/32][t][ci][32]
    return fwd.to(dtype).contiguous(), dgr.to(dtype).contiguous()


class _Pack:
    def __init__(self, convs, lins, dtype, device):
        self.keep = []
        self.w = _lib.LpipsWeights()
        for l, conv in enumerate(convs):
            w = conv.weight.detach().to(device, torch.float32)
            mfma = dtype == torch.bfloat16 and w.shape[1] % 32 == 0 and w.shape[0] % 64 == 0
            fwd, dgr = _pack_images(w, dtype, mfma)
            b = conv.bias.detach().to(device, torch.float32).contiguous()
            self.keep += [fwd, dgr, b]
            self.w.w[l], self.w.wd[l], self.w.b[l] = fwd.data_ptr(), dgr.data_ptr(), b.data_ptr()
        for k, lin in enumerate(lins):
            v = lin.model[-1].weight.detach().to(device, torch.float32).reshape(-1).contiguous()
            self.keep.append(v)
            self.w.lin[k] = v.data_ptr()


def _check_input(x: torch.Tensor, what: str):
    _lib.require_gpu(x, what)
    _lib.dtype_code(x.dtype)
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"{what}: expected [B, 3, H, W], got {tuple(x.shape)}")
    H, W = x.shape[2], x.shape[3]
    if H < 16 or W < 16 or H % 16 or W % 16:
        raise ValueError(f"{what}: {H} x {W} images; H and W must be multiples of 16 (at least 16)")


def _alloc_bytes(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


class _LpipsFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inp, target, pack, want_gram):
        n, _, H, W = inp.shape
        dt = _lib.dtype_code(inp.dtype)
        L = _lib.lib()
        x = inp.contiguous()
        y = target.to(inp.dtype).contiguous()
        tape = _alloc_bytes(L.ttv_lpips_tape_bytes(n, H, W, dt), inp.device)
        ws_bytes = L.ttv_lpips_workspace_bytes(n, H, W, dt)
        ws = _alloc_bytes(ws_bytes, inp.device)
        lp = torch.empty(n, dtype=torch.float32, device=inp.device)
        gr = torch.empty(n, dtype=torch.float32, device=inp.device) if want_gram else None
        _lib.check(L.ttv_lpips_forward(_lib.C.byref(pack.w), x.data_ptr(), y.data_ptr(), n, H, W, dt, lp.data_ptr(), _lib.ptr(gr),
                                       tape.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(inp.device)), "ttv_lpips_forward")
        if gr is None:
            gr = torch.zeros(n, dtype=torch.float32, device=inp.device)
        del ws
        if ctx.needs_input_grad[0]:
            ctx.pack, ctx.tape, ctx.shape, ctx.dt, ctx.want_gram = pack, tape, (n, H, W), dt, want_gram
            ctx.in_dtype = inp.dtype
        if not want_gram:
            ctx.mark_non_differentiable(gr)
        return lp, gr

    @staticmethod
    def backward(ctx, g_lp, g_gr):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        n, H, W = ctx.shape
        L = _lib.lib()
        dev = ctx.tape.device
        g_lp = (torch.zeros(n, device=dev) if g_lp is None else g_lp).float().contiguous()
        use_gram = ctx.want_gram and g_gr is not None
        g_gr = g_gr.float().contiguous() if use_gram else None
        ws = _alloc_bytes(L.ttv_lpips_workspace_bytes(n, H, W, ctx.dt), dev)
        dx = torch.empty((n, 3, H, W), dtype=ctx.in_dtype, device=dev)
        _lib.check(L.ttv_lpips_backward(_lib.C.byref(ctx.pack.w), ctx.tape.data_ptr(), n, H, W, ctx.dt, g_lp.data_ptr(), _lib.ptr(g_gr),
                                        dx.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)), "ttv_lpips_backward")
        return dx, None, None, None


class LPIPS(nn.Module):
    """Learned perceptual metric (reference LPIPS(use_dropout=True).eval()), HIP forward and input-gradient backward."""

    def __init__(self, use_dropout: bool = True):
        super().__init__()
        self.scaling_layer = ScalingLayer()
        self.chns = list(CHNS)
        self.net = Vgg16Features()
        for k, c in enumerate(CHNS):
            setattr(self, f"lin{k}", NetLinLayer(c, use_dropout=use_dropout))
        for p in self.parameters():
            p.requires_grad = False
        self.compute_gram = True
        self._pack_cache = None
        self._eval_ws = None       # frame_distances: the workspace, kept between calls and grown as needed

    @classmethod
    def from_file(cls, path: str) -> "LPIPS":
        """An LPIPS whose weights come from `path`: a state dict with the reference module's keys (what
        `torch.save(LPIPS().state_dict(), path)` writes in the reference's environment, or `lpips_state_dict(...)` saved)."""
        m = cls()
        m.load_state_dict(torch.load(path, map_location="cpu", weights_only=True), strict=True)
        return m.eval()

    def _pack(self, dtype, device):
        convs = self.net.convs()
        lins = [getattr(self, f"lin{k}") for k in range(5)]
        params = [p for c in convs for p in (c.weight, c.bias)] + [l.model[-1].weight for l in lins]
        key = (dtype, str(device), tuple((p.data_ptr(), p._version) for p in params))
        if self._pack_cache is None or self._pack_cache[0] != key:
            self._pack_cache = (key, _Pack(convs, lins, dtype, device))
        return self._pack_cache[1]

    def forward(self, input: torch.Tensor, target: torch.Tensor, compute_gram: bool = None):
        """(lpips[B], gram[B]) in fp32.  `compute_gram=False` skips the Gram term (returned as zeros, no gradient)."""
        _check_input(input, "LPIPS input")
        _check_input(target, "LPIPS target")
        if input.shape != target.shape:
            raise ValueError(f"LPIPS: input {tuple(input.shape)} and target {tuple(target.shape)} differ")
        want_gram = self.compute_gram if compute_gram is None else bool(compute_gram)
        pack = self._pack(input.dtype, input.device)
        return _LpipsFunction.apply(input, target.detach(), pack, want_gram)

    @staticmethod
    def _check_clips(recon_clips, target_clips):
        """Shape rules first (ValueError), then device and dtype (TypeError); nothing is launched before all clips pass."""
        if len(recon_clips) == 0 or len(recon_clips) != len(target_clips):
            raise ValueError(f"LPIPS.frame_distances: {len(recon_clips)} reconstruction and {len(target_clips)} target clips")
        for i, (r, t) in enumerate(zip(recon_clips, target_clips)):
            if r.dim() != 4 or r.shape[0] != 3 or r.shape[1] < 1 or r.shape != t.shape:
                raise ValueError(f"LPIPS.frame_distances: clip {i}: expected a [3, T, H, W] pair of one shape, got {tuple(r.shape)} "
                                 f"and {tuple(t.shape)}")
            H, W = r.shape[2], r.shape[3]
            if H < 16 or W < 16 or H > 2048 or W > 2048:
                raise ValueError(f"LPIPS.frame_distances: clip {i}: {H} x {W} frames; H and W must lie in 16 .. 2048")
        r0 = recon_clips[0]
        for i, (r, t) in enumerate(zip(recon_clips, target_clips)):
            if not (r.is_cuda and t.is_cuda) or r.device != r0.device or t.device != r0.device:
                raise TypeError(f"LPIPS.frame_distances: clip {i} is on {r.device} / {t.device}; the clips of a call must be on one GPU "
                                f"(there is no CPU path)")
            if r.dtype != r0.dtype or r.dtype not in (torch.bfloat16, torch.float32):
                raise TypeError(f"LPIPS.frame_distances: clip {i} is {r.dtype}; reconstructions must all be bf16 or all fp32")

    @torch.no_grad()
    def frame_distances(self, recon_clips: Sequence[torch.Tensor], target_clips: Sequence[torch.Tensor], clamp_recon: bool = True,
                        workspace_bytes: int = EVAL_WORKSPACE_BYTES, acc: torch.Tensor = None) -> torch.Tensor:
        """Per-frame LPIPS of whole frames: fp32 [sum of T], in clip then frame order.  Clips are [3, T, H, W] pairs, bf16 or fp32,
        H and W anything in 16 .. 2048; a target is cast to its reconstruction's dtype.  With `clamp_recon` the reconstruction is
        clamped to [-1, 1] (in the kernel that reads it), the target never.  Each frame pair is a batch entry of its own of
        `forward`'s network with floor max-pools; no tape, no autograd node, no host sync.
        Clips are grouped by (H, W), one call of ttv_lpips_eval_accumulate per group, and a group is worked through in passes of as
        many frames as `workspace_bytes` holds (at least one frame, whatever the budget).  The workspace is kept on the module.
        `acc` (double [2] on the device, optional) gets += (sum of the values, frame count); within a group the values are added
        in frame order by one thread, the groups in the order their first clips appear."""
        self._check_clips(recon_clips, target_clips)
        dev, dtype = recon_clips[0].device, recon_clips[0].dtype
        dt, L = _lib.dtype_code(dtype), _lib.lib()
        rs = [r.detach().contiguous() for r in recon_clips]
        ts = [t.detach().to(dtype).contiguous() for t in target_clips]
        groups: Dict[tuple, list] = OrderedDict()
        for i, r in enumerate(rs):
            groups.setdefault((r.shape[2], r.shape[3]), []).append(i)
        if acc is not None and not (acc.is_cuda and acc.device == dev and acc.dtype == torch.float64 and acc.numel() == 2
                                    and acc.is_contiguous()):
            raise TypeError("LPIPS.frame_distances: acc must be a contiguous float64 [2] on the clips' device")
        nbytes = {}
        for (H, W), idx in groups.items():
            frames = min(sum(rs[i].shape[1] for i in idx), EVAL_MAX_FRAMES)
            whole, one = L.ttv_lpips_eval_workspace_bytes(frames, H, W, dt), L.ttv_lpips_eval_workspace_bytes(1, H, W, dt)
            if whole < 0 or one < 0:
                _lib.check(1, "ttv_lpips_eval_workspace_bytes")
            nbytes[(H, W)] = whole if whole <= workspace_bytes else max(int(workspace_bytes), one)
        need = max(nbytes.values())
        if self._eval_ws is None or self._eval_ws.device != dev or self._eval_ws.numel() < need:
            self._eval_ws = _alloc_bytes(need, dev)
        pack = self._pack(dtype, dev)
        starts, total = [], 0
        for r in rs:
            starts.append(total)
            total += r.shape[1]
        out = torch.empty(total, dtype=torch.float32, device=dev)
        single = len(groups) == 1
        for (H, W), idx in groups.items():
            r, t = [rs[i] for i in idx], [ts[i] for i in idx]
            frames = (_lib.C.c_int32 * len(idx))(*[int(c.shape[1]) for c in r])
            vals = out if single else torch.empty(sum(frames), dtype=torch.float32, device=dev)
            _lib.check(L.ttv_lpips_eval_accumulate(_lib.C.byref(pack.w), _lib.ptr_array(r), _lib.ptr_array(t), frames, len(idx), H, W, dt,
                                                   int(bool(clamp_recon)), vals.data_ptr(), _lib.ptr(acc), self._eval_ws.data_ptr(),
                                                   nbytes[(H, W)], _lib.stream_ptr(dev)),
                       "ttv_lpips_eval_accumulate")
            if not single:
                o = 0
                for i, n in zip(idx, frames):
                    out[starts[i]:starts[i] + n] = vals[o:o + n]
                    o += n
        return out
