"""FVD without a GPU: the Fréchet distance and the restated preprocessing against the reference's own values
(tests/golden/fvd_kat.npz), the float64 restatement of I3D (tests/i3d_ref.py) against torch and against numpy loops, the TF-SAME
table, the EvalMetrics config surface, i3d_state_dict, and the C-ABI argument checks."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import i3d_ref as R
from titok_video_amd import _lib
from titok_video_amd.model.metrics import fvd
from titok_video_amd.model.metrics.eval_metrics import EvalMetrics
from titok_video_amd.synthetic import seeded_i3d_state

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fvd_kat.npz")


@pytest.fixture(scope="module")
def kat():
    return dict(np.load(GOLDEN))


def _feature_sets(kat, i):
    n, same = (int(v) for v in kat["feat_sets"][i])
    g = np.random.default_rng(int(kat["feat_seed"]) + i)
    fake = g.standard_normal((n, 400)) * (1.0 + 0.5 * g.random(400)) + 0.3
    real = fake.copy() if same else g.standard_normal((n, 400)) * (1.0 + 0.5 * g.random(400))
    return fake, real


def test_frechet_distance_matches_reference(kat):
    with np.errstate(invalid="ignore", divide="ignore"):
        for i, want in enumerate(kat["fvd"]):
            got = fvd.frechet_distance(*_feature_sets(kat, i))
            assert abs(got - want) <= 1e-9 * max(abs(want), 1.0), (i, got, want)


def test_preprocess_matches_reference_fingerprints(kat):
    """The restated preprocessing (tests/i3d_ref.py) gives the reference's detector inputs: 3 resampled frames (the size
    argument is C, not T), the last repeated to 10, the reconstruction clamped."""
    stride = int(kat["sample_stride"])
    for i, shp in enumerate(kat["clip_shapes"]):
        g = torch.Generator().manual_seed(int(kat["clip_seed"]) + i)
        shape = (3,) + tuple(int(d) for d in shp)
        recon = (torch.rand(shape, generator=g) * 2 - 1) * 1.2
        target = torch.rand(shape, generator=g) * 2 - 1
        for which, clip, clamp in (("fake", recon, True), ("real", target, False)):
            x = R.preprocess(clip, clamp)
            assert tuple(kat[f"{which}{i}_shape"]) == (3, 10, 224, 224) == tuple(x.shape)
            n = x.numel()
            assert abs(float(x.sum()) - float(kat[f"{which}{i}_sum"])) <= 1e-6 * n
            assert abs(float((x * x).sum()) - float(kat[f"{which}{i}_sumsq"])) <= 1e-6 * n
            np.testing.assert_allclose(x.reshape(-1)[::stride].numpy(), kat[f"{which}{i}_sample"], rtol=0, atol=1e-6)


def test_same_pad_table():
    # stage: (n, k, s) -> (out, front, back), the table of the issue / the architecture
    cases = {"Conv3d_1a T/H": ((10, 7, 2), (5, 2, 3)), "Conv3d_1a H": ((224, 7, 2), (112, 2, 3)),
             "MaxPool3d_2a T": ((5, 1, 1), (5, 0, 0)), "MaxPool3d_2a H": ((112, 3, 2), (56, 0, 1)),
             "Conv3d_2c": ((56, 3, 1), (56, 1, 1)), "MaxPool3d_3a H": ((56, 3, 2), (28, 0, 1)),
             "MaxPool3d_4a T": ((5, 3, 2), (3, 1, 1)), "MaxPool3d_4a H": ((28, 3, 2), (14, 0, 1)),
             "MaxPool3d_5a T": ((3, 2, 2), (2, 0, 1)), "MaxPool3d_5a H": ((14, 2, 2), (7, 0, 0)),
             "b3a": ((7, 3, 1), (7, 1, 1)), "1x1": ((14, 1, 1), (14, 0, 0))}
    for name, (args, want) in cases.items():
        assert fvd.same_pad(*args) == want, name


def test_architecture_size():
    assert len(fvd.CONV_SPECS) == 58
    n = sum(int(np.prod(s)) for k, s in fvd.canonical_shapes().items() if k.endswith("conv3d.weight"))
    assert abs(n - 12.68e6) < 0.005e6     # convolution weights
    assert fvd.CONV_SPECS[-1] == ("logits", 1024, 400, 1)


def test_restatement_matches_torch_conv3d_and_pool():
    g = torch.Generator().manual_seed(0)
    for T, H, W, k, s in [(10, 23, 19, 7, 2), (5, 9, 8, 3, 1), (3, 7, 7, 1, 1), (4, 6, 5, 3, 2)]:
        x = torch.randn(2, 5, T, H, W, generator=g, dtype=torch.float64)
        w = torch.randn(4, 5, k, k, k, generator=g, dtype=torch.float64)
        pads = []
        for n in (W, H, T):
            _, f, b = fvd.same_pad(n, k, s)
            pads += [f, b]
        want = F.conv3d(F.pad(x, pads), w, stride=s)
        torch.testing.assert_close(R.conv3d(x, w, s), want, rtol=1e-12, atol=1e-12)
    x = torch.rand(2, 3, 5, 9, 9, generator=g, dtype=torch.float64)
    for k, s in [((1, 3, 3), (1, 2, 2)), ((3, 3, 3), (2, 2, 2)), ((2, 2, 2), (2, 2, 2)), ((3, 3, 3), (1, 1, 1))]:
        pads = []
        for n, kk, ss in reversed(list(zip(x.shape[2:], k, s))):
            _, f, b = fvd.same_pad(n, kk, ss)
            pads += [f, b]
        assert torch.equal(R.maxpool3d(x, k, s), F.max_pool3d(F.pad(x, pads, value=-float("inf")), k, s))
        assert torch.equal(R.maxpool3d(x, k, s), F.max_pool3d(F.pad(x, pads, value=0.0), k, s))   # x >= 0: zero padding agrees


def test_restatement_matches_numpy_loops():
    g = torch.Generator().manual_seed(1)
    for T, H, W, k, s in [(3, 5, 4, 3, 1), (5, 6, 7, 7, 2), (2, 3, 3, 1, 1)]:
        x = torch.randn(1, 2, T, H, W, generator=g, dtype=torch.float64)
        w = torch.randn(3, 2, k, k, k, generator=g, dtype=torch.float64)
        np.testing.assert_allclose(R.conv3d(x, w, s).numpy(), R.conv3d_loop(x.numpy(), w.numpy(), s), rtol=1e-12, atol=1e-12)
    x = torch.rand(1, 2, 5, 6, 7, generator=g, dtype=torch.float64)
    for k, s in [((1, 3, 3), (1, 2, 2)), ((3, 3, 3), (2, 2, 2)), ((2, 2, 2), (2, 2, 2)), ((3, 3, 3), (1, 1, 1))]:
        np.testing.assert_array_equal(R.maxpool3d(x, k, s).numpy(), R.maxpool3d_loop(x.numpy(), k, s))


def test_restated_preprocess_matches_torch_interpolate():
    g = torch.Generator().manual_seed(2)
    for shape in [(3, 1, 40, 50), (3, 7, 230, 100), (3, 17, 96, 160)]:
        x = torch.rand(shape, generator=g) * 2.4 - 1.2
        want = F.interpolate(x.clamp(-1, 1)[None], size=(3, 224, 224), mode="trilinear", align_corners=False)[0].double()
        got = R.preprocess(x, clamp=True)
        torch.testing.assert_close(got[:, :3], want, rtol=0, atol=1e-6)     # torch blends in the input's fp32
        assert torch.equal(got[:, 3:], got[:, 2:3].expand(-1, 7, -1, -1))


# ---- config surface ---------------------------------------------------------------------------------------------------------
def _cfg(names, detector=None):
    ev = SimpleNamespace(log_metrics=names)
    if detector is not None:
        ev.fvd_detector = detector
    return SimpleNamespace(training=SimpleNamespace(eval=ev))


@pytest.fixture(scope="module")
def state_path(tmp_path_factory):
    p = tmp_path_factory.mktemp("i3d") / "i3d_state.pt"
    torch.save(seeded_i3d_state(4), p)
    return str(p)


def test_fvd_without_detector_still_raises():
    with pytest.raises(NotImplementedError, match="psnr, ssim"):
        EvalMetrics(_cfg(["ssim", "psnr", "fvd"]))
    with pytest.raises(ValueError, match="fvd_detector"):
        fvd.FVDCalculator()


def test_fvd_with_detector_accepted_in_config_order(state_path):
    m = EvalMetrics(_cfg(["fvd", "ssim", "psnr"], state_path))
    assert m.names == ["fvd", "ssim", "psnr"] and m._fvd is not None
    m2 = EvalMetrics(_cfg(["psnr", "fvd"]), fvd_detector=state_path)
    assert m2.names == ["psnr", "fvd"]
    assert not any("fvd" in k or "detector" in k for k in m.state_dict())
    with pytest.raises(NotImplementedError, match="psnr, ssim"):
        EvalMetrics(_cfg(["psnr", "fvd", "jedi"], state_path))


# ---- i3d_state_dict ---------------------------------------------------------------------------------------------------------
class _Unit(nn.Module):
    def __init__(self, cin, cout, k, bias=False, bn=True, bn_scale=True):
        super().__init__()
        self.conv3d = nn.Conv3d(cin, cout, k, bias=bias)
        if bn:
            self.bn = nn.BatchNorm3d(cout, eps=1e-3, affine=bn_scale)
            if not bn_scale:      # TF's BatchNorm: a shift (beta) and no scale
                self.bn.register_parameter("bias", nn.Parameter(torch.zeros(cout)))


class _Restated(nn.Module):
    """A module with the canonical names (or other names), only to be scripted into an archive."""

    def __init__(self, rename=False, bn_scale=True):
        super().__init__()
        units = nn.ModuleDict() if not rename else nn.ModuleList()
        for unit, cin, cout, k in fvd.CONV_SPECS:
            u = _Unit(cin, cout, k, bias=unit == "logits", bn=unit != "logits", bn_scale=bn_scale)
            if rename:
                units.append(u)
            else:
                units[unit.replace(".", "__")] = u
        self.units = units

    def forward(self, x):
        return x


def _fill(mod, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in mod.state_dict().items():
            if t.is_floating_point():
                t.copy_(torch.rand(t.shape, generator=g) + 0.5 if "running_var" in name else torch.randn(t.shape, generator=g))


def _canonical_of(mod):
    sd = {}
    for (unit, *_), u in zip(fvd.CONV_SPECS, mod.units.values() if isinstance(mod.units, nn.ModuleDict) else mod.units):
        for k, v in u.state_dict().items():
            if "num_batches" not in k:
                sd[f"{unit}.{k}"] = v
    return sd


def test_state_dict_round_trip(tmp_path):
    sd = seeded_i3d_state(1)
    p = tmp_path / "sd.pt"
    torch.save(sd, p)
    got = fvd.i3d_state_dict(p)
    assert list(got) == list(sd) and all(torch.equal(got[k], sd[k]) for k in sd)


@pytest.mark.parametrize("rename", [False, True])
def test_torchscript_archives_map(tmp_path, rename):
    mod = _Restated(rename=rename)
    _fill(mod, 5)
    want = _canonical_of(mod)
    p = tmp_path / "i3d_torchscript.pt"
    torch.jit.script(mod).save(str(p))
    got = fvd.i3d_state_dict(p)
    if not rename:    # names map through the common prefix, with the "__" of ModuleDict keys unlike the canonical ".": by shape
        pass
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_torchscript_archive_with_canonical_names(tmp_path):
    class Wrap(nn.Module):
        def __init__(self):
            super().__init__()
            self.net = nn.Module()
            for unit, cin, cout, k in fvd.CONV_SPECS:
                parent = self.net
                parts = unit.split(".")
                for part in parts[:-1]:
                    if not hasattr(parent, part):
                        parent.add_module(part, nn.Module())
                    parent = getattr(parent, part)
                parent.add_module(parts[-1], _Unit(cin, cout, k, bias=unit == "logits", bn=unit != "logits"))

        def forward(self, x):
            return x
    mod = Wrap()
    _fill(mod, 6)
    p = tmp_path / "named.pt"
    torch.jit.script(mod).save(str(p))
    got = fvd.i3d_state_dict(p)
    sd = {k[len("net."):]: v for k, v in mod.state_dict().items() if "num_batches" not in k}
    assert set(got) == set(sd)
    assert all(torch.equal(got[k], sd[k]) for k in sd)


def test_wrong_shape_is_refused(tmp_path):
    sd = seeded_i3d_state(2)
    sd["Mixed_4c.b1b.conv3d.weight"] = torch.zeros(224, 112, 3, 3, 1)
    p = tmp_path / "bad.pt"
    torch.save(sd, p)
    with pytest.raises(ValueError, match="Mixed_4c.b1b.conv3d.weight"):
        fvd.i3d_state_dict(p)
    mod = _Restated(rename=True)
    mod.units[10] = _Unit(192, 128, 1)       # Mixed_3c.b1a expects 256 -> 128
    p2 = tmp_path / "bad_ts.pt"
    torch.jit.script(mod).save(str(p2))
    with pytest.raises(ValueError, match="Mixed_3c.b1a.conv3d.weight"):
        fvd.i3d_state_dict(p2)


def test_missing_bn_scale_means_one(tmp_path):
    mod = _Restated(rename=True, bn_scale=False)
    _fill(mod, 7)
    p = tmp_path / "noscale.pt"
    torch.jit.script(mod).save(str(p))
    got = fvd.i3d_state_dict(p)
    assert "Conv3d_1a_7x7.bn.weight" not in got and "Conv3d_1a_7x7.bn.bias" in got
    _, scale, shift = fvd.fold_unit(got, "Conv3d_1a_7x7")
    var, mean, beta = (got[f"Conv3d_1a_7x7.bn.{k}"].double() for k in ("running_var", "running_mean", "bias"))
    want = 1.0 / torch.sqrt(var + 1e-3)
    assert torch.equal(scale, want.float()) and torch.equal(shift, (beta - mean * want).float())


# ---- C-ABI argument checks (no GPU touched: every call fails before a launch) -----------------------------------------------
@pytest.fixture(scope="module")
def handle():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


def test_cabi_argument_checks(handle):
    assert handle.ttv_i3d_workspace_bytes(0) == -1
    assert handle.ttv_i3d_workspace_bytes(_lib.TTV_MAX_CLIPS_PER_LAUNCH + 1) == -1
    assert handle.ttv_i3d_workspace_bytes(1) > 0
    fake = 1 << 20     # never dereferenced: every call below fails its argument checks first
    dims = (C.c_int32 * 4)(3, 4, 32, 32)
    clips = (C.c_void_p * 1)(fake)
    assert handle.ttv_fvd_preprocess(clips, dims, 0, _lib.TTV_F32, 0, fake, None) == 1
    assert handle.ttv_fvd_preprocess(clips, dims, 1, 7, 0, fake, None) == 1
    assert handle.ttv_fvd_preprocess(clips, (C.c_int32 * 4)(4, 4, 32, 32), 1, _lib.TTV_F32, 0, fake, None) == 1
    assert handle.ttv_fvd_preprocess(clips, dims, 1, _lib.TTV_F32, 0, None, None) == 1
    w = _lib.I3dWeights()
    assert handle.ttv_i3d_features(C.byref(w), fake, 1, fake, fake, 1 << 40, None) == 1       # weights missing
    for i in range(_lib.TTV_I3D_CONVS):
        w.w[i] = w.scale[i] = w.shift[i] = fake
    assert handle.ttv_i3d_features(C.byref(w), fake, 0, fake, fake, 1 << 40, None) == 1       # n = 0
    assert handle.ttv_i3d_features(C.byref(w), fake, 1, fake, fake, 16, None) == 1            # workspace too small
    assert handle.ttv_i3d_features(C.byref(w), fake + 4, 1, fake, fake, 1 << 40, None) == 1   # misaligned input
    args = [fake, 1, 4, 8, 8, 16]
    assert handle.ttv_i3d_conv3d(*args, 5, 1, fake, None, None, 16, 1, fake, 16, 0, None) == 1   # kernel size 5
    assert handle.ttv_i3d_conv3d(*args, 3, 3, fake, None, None, 16, 1, fake, 16, 0, None) == 1   # stride 3
    assert handle.ttv_i3d_conv3d(*args, 3, 1, fake, None, None, 18, 1, fake, 18, 0, None) == 1   # Cout % 4
    assert handle.ttv_i3d_conv3d(*args, 3, 1, fake, None, None, 16, 1, fake, 20, 8, None) == 1   # slice past ldc
    assert handle.ttv_i3d_conv3d(*args, 3, 1, None, None, None, 16, 1, fake, 16, 0, None) == 1   # null weights
    assert handle.ttv_i3d_maxpool3d(fake, 1, 4, 8, 8, 16, 3, 3, 3, 4, 1, 1, fake, None) == 1      # stride > window
    assert handle.ttv_i3d_maxpool3d(fake, 1, 4, 8, 8, 0, 3, 3, 3, 1, 1, 1, fake, None) == 1       # C = 0
    assert handle.ttv_i3d_maxpool3d(None, 1, 4, 8, 8, 16, 3, 3, 3, 1, 1, 1, fake, None) == 1
    assert b"i3d" in handle.ttv_error_string()
