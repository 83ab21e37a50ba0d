"""FID / IS / MMD on the GPU (csrc/ttv_inception.hip through model/metrics/metrics.py): the preprocessing against torch's
F.interpolate, every distinct convolution geometry of Inception-v3 and the two pools against float64, the whole network against the
float64 restatement (tests/inception_ref.py) with the restatement in fp32 on the CPU as the yardstick, batch independence and
determinism, and EvalMetrics / MetricCalculator end to end."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import inception_ref as R
from titok_video_amd import _lib
from titok_video_amd.model.metrics import metrics as M
from titok_video_amd.model.metrics.eval_metrics import EvalMetrics
from titok_video_amd.synthetic import seeded_inception_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def state():
    return seeded_inception_state(R.NETWORK_STATE_SEED)


@pytest.fixture(scope="module")
def extractor(state):
    return M.InceptionV3(state)


def _stream():
    return _lib.stream_ptr(torch.device(DEV))


# ---- preprocess -------------------------------------------------------------------------------------------------------------
PREP_SHAPES = [(128, 128), (96, 160), (300, 260), (1, 7), (299, 299)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("clamp", [0, 1])
def test_preprocess_matches_torch_interpolate(dtype, clamp):
    frames = R.seeded_frames(PREP_SHAPES, 5, dtype)
    # the second image is a frame of a clip, read in place through its channel stride
    clip = torch.zeros(3, 3, *PREP_SHAPES[1], dtype=dtype)
    clip[:, 1] = frames[1]
    dev = [f.to(DEV) for f in frames]
    dev[1] = clip.to(DEV)[:, 1]
    out = torch.full((len(frames), 299, 299, 3), float("nan"), device=DEV)
    dims = (C.c_int64 * (3 * len(dev)))(*[v for d in dev for v in (d.shape[1], d.shape[2], d.stride(0))])
    rc = _lib.lib().ttv_inception_preprocess(_lib.ptr_array(dev), dims, len(dev), _lib.dtype_code(dtype), clamp, out.data_ptr(), _stream())
    _lib.check(rc, "ttv_inception_preprocess")
    got = out.cpu()
    for i, f in enumerate(frames):
        x = f.float().clamp(-1, 1) if clamp else f.float()
        want = F.interpolate(x[None], size=(299, 299), mode="bilinear", align_corners=True)[0].permute(1, 2, 0)
        err = float((got[i] - want).abs().max())
        print(f"frame {tuple(f.shape)} {dtype} clamp {clamp}: max error {err:.3e}")
        assert err <= 1e-6, f"frame {tuple(f.shape)}: {err}"


# ---- every distinct convolution geometry ------------------------------------------------------------------------------------
def _conv_cases():
    """(name, H, W, Cin, Cout, k, s, p) of every distinct convolution geometry of the 94 units at a small non-square size: the
    35- and 17-stage units (and the stem's after the first) at 9 x 11, which the stride-2 units take to 4 x 5, the 8-stage units
    at 5 x 6, the stem's first unit (the scalar loader) at its true 299 x 299."""
    seen, out = set(), []
    for name, cin, cout, k, s, p in M.UNIT_SPECS:
        if name == "Conv2d_1a_3x3":
            H, W = 299, 299
        elif name.startswith(("Mixed_7b", "Mixed_7c")):
            H, W = 5, 6
        else:
            H, W = 9, 11
        key = (H, W, cin, cout, k, s, p)
        if key not in seen:
            seen.add(key)
            out.append((name,) + key)
    return out


CONV_CASES = _conv_cases()


def test_conv_cases_cover_the_network():
    geoms = {c[3:] for c in CONV_CASES}
    assert geoms == {(cin, cout, k, s, p) for _n, cin, cout, k, s, p in M.UNIT_SPECS}
    kernels = {c[5] for c in CONV_CASES}
    assert kernels == {(1, 1), (3, 3), (5, 5), (1, 7), (7, 1), (1, 3), (3, 1)}
    assert max(c[3] * c[5][0] * c[5][1] for c in CONV_CASES) == 4032          # the largest K
    assert {c[4] % 64 for c in CONV_CASES} >= {0, 16, 32, 48}                 # tail tiles of every width


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: c[0])
def test_conv2d_each_geometry(case):
    name, H, W, cin, cout, k, s, p = case
    N = 3
    g = torch.Generator().manual_seed(sum(map(ord, name)) + 7 * k[0] + k[1])
    x = torch.rand(N, cin, H, W, generator=g, dtype=torch.float64)
    if name != "Conv2d_1a_3x3":
        x = x * (torch.rand(x.shape, generator=g, dtype=torch.float64) > 0.4)     # post-ReLU-like: many zeros
    else:
        x = x * 2.4 - 1.2
    w = torch.randn(cout, cin, *k, generator=g, dtype=torch.float64) * (2.0 / (cin * k[0] * k[1])) ** 0.5
    scale = 0.5 + torch.rand(cout, generator=g, dtype=torch.float64)
    shift = 0.1 * torch.randn(cout, generator=g, dtype=torch.float64)
    x32, w32, s32, b32 = x.float(), w.float(), scale.float(), shift.float()
    pre = R.conv2d(x32.double(), w32.double(), s, p)
    ref = (pre * s32.double().view(1, -1, 1, 1) + b32.double().view(1, -1, 1, 1)).clamp_min(0)
    mag = R.conv2d(x32.double().abs(), w32.double().abs(), s, p) * s32.double().abs().view(1, -1, 1, 1)
    Ho, Wo = pre.shape[2:]
    assert (Ho, Wo) == (M.conv_out(H, k[0], s[0], p[0]), M.conv_out(W, k[1], s[1], p[1]))
    ldc, off = cout + 12, 8
    y = torch.full((N, Ho, Wo, ldc), float("nan"), device=DEV)
    xd = x32.permute(0, 2, 3, 1).contiguous().to(DEV)
    img = w32.permute(2, 3, 1, 0).reshape(-1, cout).contiguous().to(DEV)
    sd, bd = s32.to(DEV), b32.to(DEV)
    rc = _lib.lib().ttv_inception_conv2d(xd.data_ptr(), N, H, W, cin, k[0], k[1], s[0], s[1], p[0], p[1], img.data_ptr(), sd.data_ptr(),
                                         bd.data_ptr(), cout, 1, y.data_ptr(), ldc, off, _stream())
    _lib.check(rc, "ttv_inception_conv2d")
    y = y.cpu()
    assert torch.isnan(y[..., :off]).all() and torch.isnan(y[..., off + cout:]).all(), "channels outside the slice were written"
    got = y[..., off:off + cout].double().permute(0, 3, 1, 2)
    assert not torch.isnan(got).any(), "channels of the slice were not written"
    err = (got - ref).abs()
    bound = 1e-6 * mag + 1e-7 * b32.double().abs().view(1, -1, 1, 1)
    worst = float((err / bound.clamp_min(1e-30)).max())
    print(f"{name}: max error {float(err.max()):.3e}, worst error / bound {worst:.3f}")
    assert worst <= 1.0, f"{name}: error {float(err.max()):.3e}, worst error / bound {worst:.3f}"


# ---- pools ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(9, 11, 288), (17, 17, 768)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", ["avg3", "max3s2"])
def test_pools(shape, mode):
    H, W, Cc = shape
    N = 3
    g = torch.Generator().manual_seed(7)
    x = torch.rand(N, Cc, H, W, generator=g) * (torch.rand(N, Cc, H, W, generator=g) > 0.4)      # post-ReLU-like
    ref = (R.avgpool3(x.double()) if mode == "avg3" else R.maxpool3s2(x.double())).float()
    Ho, Wo = ref.shape[2:]
    ldc, off = Cc + 12, 8
    y = torch.full((N, Ho, Wo, ldc), float("nan"), device=DEV)
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    code = _lib.TTV_INCEPTION_POOL_AVG3 if mode == "avg3" else _lib.TTV_INCEPTION_POOL_MAX3S2
    rc = _lib.lib().ttv_inception_pool2d(xd.data_ptr(), N, H, W, Cc, code, y.data_ptr(), ldc, off, _stream())
    _lib.check(rc, "ttv_inception_pool2d")
    y = y.cpu()
    assert torch.isnan(y[..., :off]).all() and torch.isnan(y[..., off + Cc:]).all(), "channels outside the slice were written"
    got = y[..., off:off + Cc].permute(0, 3, 1, 2)
    if mode == "max3s2":
        assert torch.equal(got, ref)
    else:
        ulp = torch.from_numpy(np.spacing(ref.abs().clamp_min(torch.finfo(torch.float32).tiny).numpy()))
        worst = float(((got - ref).abs() / ulp).max())
        print(f"avg3 {shape}: worst error {worst:.2f} ulp")
        assert worst <= 4.0


# ---- whole network ----------------------------------------------------------------------------------------------------------
def _rel(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max())


def test_network_against_float64(state, extractor):
    """max|f - f64| / max|f64| per frame for acts and probs: the HIP path's figure is held to 4 x the worst figure of the same
    arithmetic in torch fp32 on the CPU (both fp32, different summation orders).
    Measured (MI355X): acts 3.6e-7 .. 3.9e-7 on HIP against 1.9e-7 .. 2.0e-7 for the CPU fp32 run, probs 1.3e-6 .. 2.1e-6
    against 0.6e-6 .. 1.5e-6."""
    frames = R.seeded_frames(R.NETWORK_FRAME_SHAPES, R.NETWORK_FRAME_SEED)
    a64, p64 = R.features(torch.stack([R.preprocess(f) for f in frames]), state)
    a32, p32 = R.features(torch.stack([R.preprocess(f, dtype=torch.float32) for f in frames]), state, torch.float32)
    acts, probs = extractor.features([([f.to(DEV) for f in frames], False)])
    acts, probs = acts.cpu(), probs.cpu()
    assert acts.shape == (3, 2048) and probs.shape == (3, 1000) and acts.dtype == probs.dtype == torch.float32
    cpu = [(_rel(a32[i], a64[i]), _rel(p32[i], p64[i])) for i in range(3)]
    hip = [(_rel(acts[i], a64[i]), _rel(probs[i], p64[i])) for i in range(3)]
    yard_a, yard_p = max(c[0] for c in cpu), max(c[1] for c in cpu)
    for i in range(3):
        print(f"frame {i}: acts HIP {hip[i][0]:.3e} (CPU fp32 {cpu[i][0]:.3e}), probs HIP {hip[i][1]:.3e} (CPU fp32 {cpu[i][1]:.3e})")
    print(f"yardstick: acts {yard_a:.3e}, probs {yard_p:.3e}; HIP worst: acts {max(h[0] for h in hip):.3e}, probs {max(h[1] for h in hip):.3e}")
    for i in range(3):
        assert hip[i][0] <= 4 * yard_a, f"frame {i}: acts {hip[i][0]:.3e} > 4 x {yard_a:.3e}"
        assert hip[i][1] <= 4 * yard_p, f"frame {i}: probs {hip[i][1]:.3e} > 4 x {yard_p:.3e}"
    only_acts, none = extractor.features([([f.to(DEV) for f in frames], False)], want_probs=False)
    assert none is None and torch.equal(only_acts.cpu(), acts)


def test_batch_independence_and_determinism(extractor):
    gen = [f.to(DEV) for f in R.seeded_frames([(64, 80)] * 35, 31, torch.bfloat16)]
    real = [f.to(DEV) for f in R.seeded_frames([(64, 80)] * 35, 32, torch.bfloat16, spread=1.0)]
    groups = [(gen, True), (real, False)]       # 70 frames: a launch of 64 and one of 6
    runs = [tuple(t.cpu() for t in extractor.features(groups)) for _ in range(2)]
    assert runs[0][0].shape == (70, 2048) and runs[0][1].shape == (70, 1000)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two runs differ"
    flat = [(f, True) for f in gen] + [(f, False) for f in real]
    for i in (0, 33, 69):
        a, p = extractor.features([([flat[i][0]], flat[i][1])])
        assert torch.equal(a.cpu()[0], runs[0][0][i]) and torch.equal(p.cpu()[0], runs[0][1][i]), f"frame {i} alone differs"


# ---- end to end -------------------------------------------------------------------------------------------------------------
def _cfg(names):
    return SimpleNamespace(training=SimpleNamespace(eval=SimpleNamespace(log_metrics=names)))


def _clips(shapes, seed, dtype, spread):
    g = torch.Generator().manual_seed(seed)
    return [((torch.rand((3,) + s, generator=g) * 2 - 1) * spread).to(dtype).to(DEV) for s in shapes]


def _close(a, b):
    return abs(a - b) <= 1e-9 * abs(b)


def test_eval_metrics_end_to_end(extractor):
    shapes = [(4, 128, 128), (2, 96, 160), (3, 128, 128), (1, 168, 136)]
    recon, target = _clips(shapes, 41, torch.bfloat16, 1.2), _clips(shapes, 42, torch.bfloat16, 1.0)
    full = EvalMetrics(_cfg(["ssim", "psnr", "fid", "is", "mmd"]), inception_weights=extractor)
    plain = EvalMetrics(_cfg(["ssim", "psnr"]))
    for m in (full, plain):
        m.update(recon[:2], target[:2])
        m.update(recon[2:], target[2:])
    a, b = full.compute(), plain.compute()
    assert list(a) == ["eval/ssim", "eval/psnr", "eval/fid", "eval/is", "eval/mmd"]
    assert a["eval/ssim"] == b["eval/ssim"] and a["eval/psnr"] == b["eval/psnr"]
    real, fake, probs = full._inception.features()
    assert real.shape == fake.shape == (10, 2048) and probs.shape == (10, 1000) and fake.is_cuda and probs.is_cuda
    want = {"eval/fid": M.calculate_fid(real.cpu().double().numpy(), fake.cpu().double().numpy()),
            "eval/is": M.compute_inception_score(probs.cpu().double().numpy()),
            "eval/mmd": M.mmd_poly(real.cpu().double().numpy(), fake.cpu().double().numpy(), degree=2, coef0=0) * 100}
    for k, v in want.items():
        print(f"{k}: {a[k]!r}")
        assert np.isfinite(v) and _close(a[k], v), (k, a[k], v)
    # the reconstruction is clamped, the target is not: frame 0's features are the extractor's on those inputs
    da, dp = extractor.features([([recon[0][:, 0]], True), ([target[0][:, 0]], False)])
    assert torch.equal(da[0], fake[0]) and torch.equal(da[1], real[0]) and torch.equal(dp[0], probs[0])
    unclamped, _ = extractor.features([([recon[0][:, 0]], False)], want_probs=False)
    assert not torch.equal(unclamped[0], fake[0])
    assert len(full.state_dict()) == 0
    # MetricCalculator on the same frames (it does not clamp: the reconstructions are clamped for it) reports the same numbers
    mc = M.MetricCalculator(("fid", "is", "mmd"), inception_weights=extractor)
    frames_r = [c[:, t] for c in target for t in range(c.shape[1])]
    frames_g = [c.clamp(-1, 1)[:, t] for c in recon for t in range(c.shape[1])]
    mc(frames_r[:7], frames_g[:7])
    mc(frames_r[7:], frames_g[7:])
    out = mc.gather()
    assert list(out) == ["eval/fid", "eval/mmd", "eval/is"]
    for k in out:
        assert _close(out[k], a[k]), (k, out[k], a[k])
    mc.reset()
    assert all(np.isnan(v) for v in mc.gather().values())
    full.reset()
    assert all(t.shape[0] == 0 for t in full._inception.features())
    after = full.compute()
    assert all(np.isnan(after[f"eval/{k}"]) for k in ("fid", "is", "mmd"))
    assert after["eval/psnr"] == float("inf") and np.isnan(after["eval/ssim"])


def test_single_image_gives_nan_fid(extractor):
    one = M.MetricCalculator(("fid", "mmd"), inception_weights=extractor)
    r, g = R.seeded_frames([(64, 64), (64, 64)], 51)
    one([r.to(DEV)], [g.to(DEV)])
    out = one.gather()
    assert np.isnan(out["eval/fid"]) and np.isfinite(out["eval/mmd"])
