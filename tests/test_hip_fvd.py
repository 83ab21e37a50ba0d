"""FVD on the GPU (csrc/ttv_i3d.hip through model/metrics/fvd.py): the preprocessing against torch's F.interpolate, each convolution
shape of I3D and each max-pool against float64, the whole detector against the float64 restatement (tests/i3d_ref.py), batch
independence and determinism, and EvalMetrics end to end."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import i3d_ref as R
from titok_video_amd import _lib
from titok_video_amd.model.metrics import fvd
from titok_video_amd.model.metrics.eval_metrics import EvalMetrics
from titok_video_amd.synthetic import seeded_i3d_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CLIP_SHAPES = [(1, 128, 128), (2, 168, 136), (3, 96, 160), (8, 300, 260), (16, 128, 128), (17, 96, 160)]


@pytest.fixture(scope="module")
def state():
    return seeded_i3d_state(3)


@pytest.fixture(scope="module")
def detector(state):
    return fvd.I3D(state)


def _clips(shapes, seed, dtype=torch.float32, spread=1.2):
    g = torch.Generator().manual_seed(seed)
    return [((torch.rand((3,) + s, generator=g) * 2 - 1) * spread).to(dtype) for s in shapes]


def _torch_prep(clip, clamp):
    x = clip.float()
    if clamp:
        x = x.clamp(-1, 1)
    x = F.interpolate(x[None], size=(x.shape[0], 224, 224), mode="trilinear", align_corners=False)
    x = torch.cat([x, x[:, :, -1:].repeat(1, 1, 10 - x.shape[2], 1, 1)], dim=2)
    return x[0]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("clamp", [0, 1])
def test_preprocess_matches_torch_interpolate(dtype, clamp):
    clips = _clips(CLIP_SHAPES, 5, dtype)
    dev = [c.to(DEV) for c in clips]
    out = torch.full((len(clips), 10, 224, 224, 3), float("nan"), device=DEV)
    dims = (C.c_int32 * (4 * len(clips)))(*[int(d) for c in clips for d in c.shape])
    rc = _lib.lib().ttv_fvd_preprocess(_lib.ptr_array(dev), dims, len(clips), _lib.dtype_code(dtype), clamp, out.data_ptr(),
                                       _lib.stream_ptr(torch.device(DEV)))
    _lib.check(rc, "ttv_fvd_preprocess")
    got = out.cpu()
    for i, c in enumerate(clips):
        want = _torch_prep(c, clamp).permute(1, 2, 3, 0)
        err = float((got[i] - want).abs().max())
        assert err <= 1e-6, f"clip {tuple(c.shape)}: {err}"


def _layer_shapes():
    """(name, N, T, H, W, Cin, Cout, k, stride) of every distinct convolution shape of the network, plus the logits as a conv."""
    dims = {"Conv3d_1a_7x7": (10, 224), "Conv3d_2b_1x1": (5, 56), "Conv3d_2c_3x3": (5, 56)}
    for name in fvd.INCEPTION:
        dims[name] = (5, 28) if name.startswith("Mixed_3") else (3, 14) if name.startswith("Mixed_4") else (2, 7)
    seen, out = set(), []
    for unit, cin, cout, k in fvd.CONV_SPECS:
        t, h = dims.get(unit.split(".")[0], (2, 7))
        stride = 2 if unit == "Conv3d_1a_7x7" else 1
        key = (t, h, cin, cout, k, stride)
        if key in seen:
            continue
        seen.add(key)
        out.append((unit, 1 if unit == "Conv3d_1a_7x7" else 2, t, h, h, cin, cout, k, stride))
    return out


@pytest.mark.parametrize("shape", _layer_shapes(), ids=lambda s: s[0])
def test_conv3d_each_layer_shape(shape):
    name, N, T, H, W, cin, cout, k, stride = shape
    g = torch.Generator().manual_seed(sum(map(ord, name)) + k)
    x = torch.rand(N, cin, T, H, W, generator=g, dtype=torch.float64)
    if name != "Conv3d_1a_7x7":
        x = x * (torch.rand(x.shape, generator=g, dtype=torch.float64) > 0.4)     # post-ReLU-like: many zeros
    else:
        x = x * 2 - 1
    w = torch.randn(cout, cin, k, k, k, generator=g, dtype=torch.float64) * (2.0 / (cin * k ** 3)) ** 0.5
    scale = 0.5 + torch.rand(cout, generator=g, dtype=torch.float64)
    shift = 0.1 * torch.randn(cout, generator=g, dtype=torch.float64)
    relu = name != "logits"
    x32, w32, s32, b32 = x.float(), w.float(), scale.float(), shift.float()
    pre = R.conv3d(x32.double(), w32.double(), stride)
    ref = pre * s32.double().view(1, -1, 1, 1, 1) + b32.double().view(1, -1, 1, 1, 1)
    if relu:
        ref = ref.clamp_min(0)
    mag = R.conv3d(x32.double().abs(), w32.double().abs(), stride) * s32.double().abs().view(1, -1, 1, 1, 1)
    ldc, off = cout + 12, 8
    To, Ho, Wo = pre.shape[2:]
    y = torch.full((N, To, Ho, Wo, ldc), float("nan"), device=DEV)
    xd = x32.permute(0, 2, 3, 4, 1).contiguous().to(DEV)
    img = w32.permute(2, 3, 4, 1, 0).reshape(-1, cout).contiguous().to(DEV)
    sd, bd = s32.to(DEV), b32.to(DEV)
    rc = _lib.lib().ttv_i3d_conv3d(xd.data_ptr(), N, T, H, W, cin, k, stride, img.data_ptr(), sd.data_ptr(), bd.data_ptr(), cout,
                                   int(relu), y.data_ptr(), ldc, off, _lib.stream_ptr(torch.device(DEV)))
    _lib.check(rc, "ttv_i3d_conv3d")
    y = y.cpu()
    assert torch.isnan(y[..., :off]).all() and torch.isnan(y[..., off + cout:]).all(), "channels outside the slice were written"
    got = y[..., off:off + cout].double().permute(0, 4, 1, 2, 3)
    err = (got - ref).abs()
    bound = 1e-6 * mag + 1e-7 * b32.double().abs().view(1, -1, 1, 1, 1)
    worst = float((err / bound.clamp_min(1e-30)).max())
    assert worst <= 1.0, f"{name}: error {float(err.max()):.3e}, worst error / bound {worst:.3f}"


POOLS = [("MaxPool3d_2a_3x3", 5, 112, 64, (1, 3, 3), (1, 2, 2)), ("MaxPool3d_3a_3x3", 5, 56, 192, (1, 3, 3), (1, 2, 2)),
         ("MaxPool3d_4a_3x3", 5, 28, 480, (3, 3, 3), (2, 2, 2)), ("MaxPool3d_5a_2x2", 3, 14, 832, (2, 2, 2), (2, 2, 2)),
         ("b3a", 3, 14, 512, (3, 3, 3), (1, 1, 1))]


@pytest.mark.parametrize("pool", POOLS, ids=lambda p: p[0])
def test_maxpool3d_exact(pool):
    name, T, H, Cc, k, s = pool
    g = torch.Generator().manual_seed(7)
    x = torch.rand(2, Cc, T, H, H, generator=g)
    ref = R.maxpool3d(x.double(), k, s).float()
    y = torch.full((2,) + tuple(ref.shape[2:]) + (Cc,), float("nan"), device=DEV)
    xd = x.permute(0, 2, 3, 4, 1).contiguous().to(DEV)
    rc = _lib.lib().ttv_i3d_maxpool3d(xd.data_ptr(), 2, T, H, H, Cc, *k, *s, y.data_ptr(), _lib.stream_ptr(torch.device(DEV)))
    _lib.check(rc, "ttv_i3d_maxpool3d")
    assert torch.equal(y.cpu().permute(0, 4, 1, 2, 3), ref)


def test_detector_against_float64(state, detector):
    clips = _clips([(16, 128, 128), (3, 96, 160), (8, 168, 136)], 21)
    feats = detector.features([([c.to(DEV) for c in clips], False)]).cpu().double()
    worst = 0.0
    for i, c in enumerate(clips):
        ref = R.features(R.preprocess(c)[None], state)[0]
        rel = float((feats[i] - ref).abs().max() / ref.abs().max())
        worst = max(worst, rel)
        assert rel <= 1e-4, f"clip {i}: max |f - f64| / max |f64| = {rel:.3e}"
    print(f"\nI3D features vs float64: worst max|f - f64| / max|f64| = {worst:.3e}")


def test_batch_independence_and_determinism(detector):
    recon = _clips([(16, 128, 128)] * 70, 31, torch.bfloat16)
    target = _clips([(16, 128, 128)] * 70, 32, torch.bfloat16, spread=1.0)
    rd, td = [c.to(DEV) for c in recon], [c.to(DEV) for c in target]
    runs = []
    for _ in range(2):
        m = fvd.FVDCalculator(detector=detector)
        m.update_clips(rd, td, clamp_recon=True)
        runs.append(tuple(t.cpu() for t in m.features()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two runs differ"
    for i in (0, 33, 69):
        alone = fvd.FVDCalculator(detector=detector)
        alone.update_clips([rd[i]], [td[i]], clamp_recon=True)
        fa, ra = alone.features()
        assert torch.equal(fa.cpu()[0], runs[0][0][i]) and torch.equal(ra.cpu()[0], runs[0][1][i]), f"clip {i} alone differs"


def _cfg(names):
    return SimpleNamespace(training=SimpleNamespace(eval=SimpleNamespace(log_metrics=names)))


def test_eval_metrics_end_to_end(state, detector):
    recon = [c.to(DEV) for c in _clips([(16, 128, 128), (8, 96, 160), (3, 128, 128), (5, 168, 136)], 41, torch.bfloat16)]
    target = [c.to(DEV) for c in _clips([(16, 128, 128), (8, 96, 160), (3, 128, 128), (5, 168, 136)], 42, torch.bfloat16, 1.0)]
    with_fvd = EvalMetrics(_cfg(["ssim", "psnr", "fvd"]), fvd_detector=detector)
    plain = EvalMetrics(_cfg(["ssim", "psnr"]))
    for m in (with_fvd, plain):
        m.update(recon[:2], target[:2])
        m.update(recon[2:], target[2:])
    a, b = with_fvd.compute(), plain.compute()
    assert list(a) == ["eval/ssim", "eval/psnr", "eval/fvd"]
    assert a["eval/ssim"] == b["eval/ssim"] and a["eval/psnr"] == b["eval/psnr"]
    fake, real = with_fvd._fvd.features()
    assert fake.shape == (4, 400) and fake.is_cuda
    want = fvd.frechet_distance(fake.cpu().double().numpy(), real.cpu().double().numpy())
    assert abs(a["eval/fvd"] - want) <= 1e-9 * abs(want)
    # the reconstruction is clamped, the target is not: the features of clip 0 are the detector's on those inputs
    direct = detector.features([([recon[0]], True), ([target[0]], False)]).cpu()
    assert torch.equal(direct[0], fake.cpu()[0]) and torch.equal(direct[1], real.cpu()[0])
    assert not any(k.startswith("_fvd") or "detector" in k for k in with_fvd.state_dict())
    with_fvd.reset()
    assert with_fvd._fvd.features()[0].shape[0] == 0 and np.isnan(with_fvd.compute()["eval/fvd"])
    after = with_fvd.compute()
    assert after["eval/psnr"] == float("inf") and np.isnan(after["eval/ssim"])
