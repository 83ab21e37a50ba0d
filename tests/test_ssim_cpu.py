"""SSIM of EvalMetrics without a GPU: the config surface, the C-ABI argument checks, and the float64 restatement of the reference's
metric that tests/test_hip_ssim.py compares the kernels against.

The reference (model/metrics/eval_metrics.py:20-21,32-37) feeds each clip as x.clamp(-1, 1), CTHW -> TCHW, to torchmetrics'
StructuralSimilarityIndexMeasure(data_range=2).  torchmetrics is not available here, so its `_ssim_update` with those defaults is
restated below (reflect-pad by 5, grouped conv2d with the 11 x 11 Gaussian window, crop 5) and pinned two independent ways.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from scipy.ndimage import correlate1d

from titok_video_amd import _lib
from titok_video_amd.model.metrics.eval_metrics import EvalMetrics

C1, C2 = (0.01 * 2) ** 2, (0.03 * 2) ** 2


def gaussian_taps() -> torch.Tensor:
    """torchmetrics' _gaussian(11, 1.5): int(3.5 * 1.5 + 0.5) * 2 + 1 = 11 taps, normalised to sum 1 (float64)."""
    dist = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-((dist / 1.5) ** 2) / 2)
    return g / g.sum()


def ssim_frames(recon: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """Per-frame SSIM of one [C,T,H,W] clip pair in float64, as the reference computes it: recon clamped to [-1, 1], frames as the
    batch (CTHW -> TCHW), reflect-pad 5, 'valid' grouped conv2d with g^T g, the index, crop 5 from every side, mean per frame."""
    x = recon.double().clamp(-1, 1).transpose(0, 1)
    y = target.double().transpose(0, 1)
    c = x.shape[1]
    g = gaussian_taps()
    k = torch.outer(g, g).expand(c, 1, 11, 11)
    xp, yp = F.pad(x, (5, 5, 5, 5), mode="reflect"), F.pad(y, (5, 5, 5, 5), mode="reflect")
    out = F.conv2d(torch.cat([xp, yp, xp * xp, yp * yp, xp * yp]), k, groups=c)
    mx, my, exx, eyy, exy = out.split(x.shape[0])
    sxx = (exx - mx * mx).clamp(min=0)
    syy = (eyy - my * my).clamp(min=0)
    sxy = exy - mx * my
    idx = ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))
    return idx[..., 5:-5, 5:-5].reshape(x.shape[0], -1).mean(-1)


def ssim_metric(recon, target) -> float:
    """The metric state over a list of clips: sum of per-frame values / number of frames."""
    f = torch.cat([ssim_frames(r, t) for r, t in zip(recon, target)])
    return float(f.sum() / f.numel())


def _cfg(names):
    return SimpleNamespace(training=SimpleNamespace(eval=SimpleNamespace(log_metrics=list(names))))


def _separable_frames(recon: torch.Tensor, target: torch.Tensor) -> np.ndarray:
    """An independent restatement: scipy correlate1d along W then H with the same taps, the valid region cut out directly."""
    x = np.clip(recon.double().numpy(), -1, 1)
    y = target.double().numpy()
    g = gaussian_taps().numpy()

    def filt(a):
        return correlate1d(correlate1d(a, g, axis=3, mode="constant"), g, axis=2, mode="constant")[:, :, 5:-5, 5:-5]

    mx, my, exx, eyy, exy = (filt(a) for a in (x, y, x * x, y * y, x * y))
    sxx = np.maximum(exx - mx * mx, 0)
    syy = np.maximum(eyy - my * my, 0)
    sxy = exy - mx * my
    idx = ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))
    return idx.mean(axis=(0, 2, 3))          # [C,T,h,w] -> per frame


def test_ssim_is_accepted_in_config_order():
    m = EvalMetrics(_cfg(["ssim", "psnr"]))
    assert m.names == ["ssim", "psnr"]
    assert EvalMetrics(_cfg(["psnr", "ssim"])).names == ["psnr", "ssim"]
    assert EvalMetrics().names == ["psnr"]
    assert m.compute() == {}


@pytest.mark.parametrize("other", ["fvd", "jedi"])
def test_network_metrics_still_raise(other):
    with pytest.raises(NotImplementedError, match="psnr, ssim"):
        EvalMetrics(_cfg(["ssim", "psnr", other]))


def test_restatement_matches_a_separable_filter():
    g = torch.Generator().manual_seed(11)
    for shape in [(3, 2, 16, 24), (1, 3, 11, 11), (3, 2, 40, 13), (2, 1, 23, 31)]:
        target = torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1
        recon = target + 0.4 * torch.randn(shape, generator=g, dtype=torch.float64)       # some values leave [-1, 1]
        a = ssim_frames(recon, target).numpy()
        b = _separable_frames(recon, target)
        assert a.shape == (shape[1],)
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-12)


@pytest.mark.parametrize("a,b", [(0.3, -0.2), (-0.7, -0.7), (1.0, 0.0), (0.05, 0.9)])
def test_restatement_matches_the_closed_form_on_constant_frames(a, b):
    x = torch.full((3, 2, 17, 14), a, dtype=torch.float64)
    y = torch.full((3, 2, 17, 14), b, dtype=torch.float64)
    want = (2 * a * b + C1) / (a * a + b * b + C1)
    np.testing.assert_allclose(ssim_frames(x, y).numpy(), [want, want], rtol=0, atol=1e-12)


def test_cabi_refuses_bad_shapes_without_touching_the_gpu():
    h = _lib.lib()
    dims = (C.c_int32 * 8)(3, 16, 128, 128, 3, 4, 16, 24)
    # 16 frames x 4 x 4 tiles of 32 x 32 outputs (118 x 118 valid) + 4 frames x 1 tile, one double per tile
    assert h.ttv_ssim_workspace_bytes(dims, 2) == (16 * 16 + 4) * 8
    assert h.ttv_ssim_workspace_bytes(dims, 0) == 0
    for bad in [(3, 4, 10, 24), (3, 4, 24, 10), (0, 4, 24, 24), (3, 0, 24, 24)]:
        d = (C.c_int32 * 4)(*bad)
        assert h.ttv_ssim_workspace_bytes(d, 1) == -1
        assert b"ssim" in h.ttv_error_string()
    assert h.ttv_ssim_workspace_bytes((C.c_int32 * 4)(3, 4, 10, 24), 1) == -1 and b"H >= 11" in h.ttv_error_string()
    many = (C.c_int32 * (4 * 65))(*([3, 1, 16, 16] * 65))
    assert h.ttv_ssim_workspace_bytes(many, 65) == -1 and b"at most 64" in h.ttv_error_string()
    ptrs = (C.c_void_p * 1)(16)
    d = (C.c_int32 * 4)(3, 4, 16, 24)
    acc = C.c_void_p(64)
    assert h.ttv_ssim_accumulate(None, ptrs, d, 1, _lib.TTV_F32, 1, acc, C.c_void_p(128), 64, None) == 1
    assert b"null" in h.ttv_error_string()
    assert h.ttv_ssim_accumulate(ptrs, ptrs, d, 1, _lib.TTV_F32, 1, acc, C.c_void_p(128), 24, None) == 1
    assert b"workspace" in h.ttv_error_string()
    assert h.ttv_ssim_accumulate(ptrs, ptrs, d, 1, 7, 1, acc, C.c_void_p(128), 64, None) == 1
    assert b"dtype" in h.ttv_error_string()
    assert h.ttv_ssim_accumulate(ptrs, ptrs, many, 65, _lib.TTV_F32, 1, acc, C.c_void_p(128), 1 << 20, None) == 1
