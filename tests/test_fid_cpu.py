"""FID / IS / MMD without a GPU: the statistics against the reference's own values (tests/golden/fid_kat.npz), the architecture
table, inception_state_dict, the EvalMetrics / MetricCalculator surface, the header against the ctypes structs, the C-ABI argument
checks, the float64 restatement of Inception-v3 (tests/inception_ref.py) against explicit loops, and the seeded data of the GPU
tests (non-degenerate features)."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import inception_ref as R
from titok_video_amd import _lib
from titok_video_amd.model.metrics import metrics as M
from titok_video_amd.model.metrics.eval_metrics import EvalMetrics
from titok_video_amd.synthetic import seeded_inception_state

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "fid_kat.npz")
HEADER = os.path.join(HERE, "..", "include", "titok_hip.h")


@pytest.fixture(scope="module")
def kat():
    return dict(np.load(GOLDEN))


# the two recipes of tests/golden/make_golden_fid.py
def _feature_sets(kat, i):
    n, same = (int(v) for v in kat["feat_cases"][i])
    rng = np.random.default_rng(int(kat["seed"]) + i)
    dim = int(kat["dim"])
    real = rng.standard_normal((n, dim)) * (1.0 + 0.5 * rng.random(dim))
    fake = real.copy() if same else 0.8 * rng.standard_normal((n, dim)) + 0.3
    return real, fake, bool(same)


def _prob_sets(kat, i):
    n, spread = int(kat["prob_cases"][i][0]), float(kat["prob_cases"][i][1])
    rng = np.random.default_rng(int(kat["seed"]) + 100 + i)
    z = spread * rng.standard_normal((n, int(kat["classes"])))
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


# ---- statistics -------------------------------------------------------------------------------------------------------------
def test_fid_matches_reference(kat):
    assert sorted(int(c[0]) for c in kat["feat_cases"]) == [2, 37, 37, 300] and int(kat["dim"]) == 48
    for i, want in enumerate(kat["fid"]):
        real, fake, same = _feature_sets(kat, i)
        got = M.calculate_fid(real, fake)
        if same:
            assert abs(got) <= 1e-6 and abs(want) <= 1e-6, (i, got, want)
        else:
            assert abs(got - want) <= 1e-6 * abs(want), (i, got, want)      # sqrtm is involved
        mu1, s1 = M.calculate_activation_statistics(real)
        mu2, s2 = M.calculate_activation_statistics(fake)
        assert M.calculate_frechet_distance(mu1, s1, mu2, s2) == got
    assert sum(int(c[1]) for c in kat["feat_cases"]) == 1     # one identical pair


def test_fid_takes_float32_tensors_and_needs_two_images(kat):
    real, fake, _ = _feature_sets(kat, 1)
    r32, f32 = torch.from_numpy(real).float(), torch.from_numpy(fake).float()
    assert M.calculate_fid(r32, f32) == M.calculate_fid(r32.double().numpy(), f32.double().numpy())
    assert np.isnan(M.calculate_fid(real[:1], fake[:1]))
    with pytest.raises(ValueError, match="different sizes"):
        M.calculate_frechet_distance(np.zeros(3), np.eye(3), np.zeros(4), np.eye(4))


def test_mmd_and_inception_score_match_reference(kat):
    for i, want in enumerate(kat["mmd"]):
        real, fake, _ = _feature_sets(kat, i)
        got = M.mmd_poly(real, fake, degree=2, coef0=0)
        assert abs(got - want) <= 1e-9 * max(abs(want), 1e-300), (i, got, want)
    assert [int(c[0]) for c in kat["prob_cases"]] == [1, 37, 300] and int(kat["classes"]) == 10
    for i, want in enumerate(kat["inception_score"]):
        got = M.compute_inception_score(_prob_sets(kat, i))
        assert abs(got - want) <= 1e-9 * abs(want), (i, got, want)
    p = _prob_sets(kat, 1)
    assert abs(M.compute_inception_score(np.repeat(p[:1], 5, 0)) - 1.0) <= 1e-12     # one distribution: no information


# ---- architecture -----------------------------------------------------------------------------------------------------------
def test_architecture_table():
    specs = M.UNIT_SPECS
    assert len(specs) == 94 == _lib.TTV_INCEPTION_UNITS and len({s[0] for s in specs}) == 94
    blocks = M.blocks()
    assert list(blocks) == ["Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e", "Mixed_7a",
                            "Mixed_7b", "Mixed_7c"]
    width = M.STEM[-1][2]
    for name, b in blocks.items():
        assert b["cin"] == width, f"{name} takes {b['cin']} channels, the block before gives {width}"
        width = b["cout"]
    assert width == 2048 == _lib.TTV_INCEPTION_FEATURES
    assert [b["cout"] for b in blocks.values()] == [256, 288, 288, 768, 768, 768, 768, 768, 1280, 2048, 2048]
    for (_, _, cout, *_), (_, cin, *_) in zip(M.STEM, M.STEM[1:]):
        assert cout == cin
    s = M.spatial_sizes()
    stages = ["input", "Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3", "maxpool1", "Conv2d_3b_1x1", "Conv2d_4a_3x3", "maxpool2",
              "Mixed_5d", "Mixed_6a", "Mixed_7a"]
    assert [s[k] for k in stages] == [299, 149, 147, 147, 73, 73, 71, 35, 35, 17, 8]
    assert s["Mixed_6e"] == 17 and s["Mixed_7c"] == 8
    # a unit inside a block keeps the size unless it is one of the stride-2 units of Mixed_6a / Mixed_7a; 1 x 7 pads (0, 3) and so on
    for name, _cin, _cout, k, st, p in specs:
        if st == (1, 1) and "." in name:
            assert (2 * p[0] == k[0] - 1) and (2 * p[1] == k[1] - 1), name
    strided = [n for n, *_r in specs if _r[3] == (2, 2)]
    assert strided == ["Conv2d_1a_3x3", "Mixed_6a.branch3x3", "Mixed_6a.branch3x3dbl_3", "Mixed_7a.branch3x3_2", "Mixed_7a.branch7x7x3_4"]
    n = sum(int(np.prod(v)) for key, v in M.canonical_shapes().items() if key.endswith("conv.weight"))
    assert abs(n - 21.75e6) < 0.01e6       # convolution weights of the trunk


# ---- loader -----------------------------------------------------------------------------------------------------------------
def test_state_dict_round_trip_and_refusals(tmp_path):
    sd = seeded_inception_state(1)
    p = tmp_path / "inception.pt"
    extra = dict(sd)
    extra["AuxLogits.conv0.conv.weight"] = torch.zeros(128, 768, 1, 1)
    extra["AuxLogits.fc.bias"] = torch.zeros(1000)
    extra["Conv2d_1a_3x3.bn.num_batches_tracked"] = torch.tensor(7)
    torch.save(extra, p)
    got = M.inception_state_dict(p)
    assert list(got) == list(sd) == list(M.canonical_shapes())
    assert all(torch.equal(got[k], sd[k]) and got[k].dtype == torch.float32 for k in sd)
    got2 = M.inception_state_dict({k: v.double() for k, v in extra.items()})
    assert all(torch.equal(got2[k], sd[k]) and got2[k].dtype == torch.float32 for k in sd)
    missing = dict(sd)
    del missing["Mixed_6c.branch7x7dbl_3.bn.running_var"]
    with pytest.raises(ValueError, match="Mixed_6c.branch7x7dbl_3.bn.running_var"):
        M.inception_state_dict(missing)
    bad = dict(sd)
    bad["Mixed_6c.branch7x7_2.conv.weight"] = torch.zeros(160, 160, 7, 1)      # (1, 7) expected
    with pytest.raises(ValueError, match="Mixed_6c.branch7x7_2.conv.weight"):
        M.inception_state_dict(bad)
    torch.save(bad, p)
    with pytest.raises(ValueError, match="Mixed_6c.branch7x7_2.conv.weight"):
        M.InceptionV3.from_file(p)


def test_fold_unit_rounds_once():
    sd = seeded_inception_state(2)
    unit = "Mixed_7a.branch7x7x3_2"
    img, scale, shift = M.fold_unit(sd, unit)
    w = sd[f"{unit}.conv.weight"]
    assert img.shape == (7 * 192, 192) and torch.equal(img[3 * 192 + 5, 9], w[9, 5, 0, 3])     # K = (dh kW + dw) Cin + ci
    g, b, m, v = (sd[f"{unit}.bn.{k}"].double() for k in ("weight", "bias", "running_mean", "running_var"))
    want = g / torch.sqrt(v + 1e-3)
    assert torch.equal(scale, want.float()) and torch.equal(shift, (b - m * want).float())


# ---- config surface ---------------------------------------------------------------------------------------------------------
def _cfg(names, weights=None):
    ev = SimpleNamespace(log_metrics=names)
    if weights is not None:
        ev.inception_weights = weights
    return SimpleNamespace(training=SimpleNamespace(eval=ev))


@pytest.fixture(scope="module")
def state_path(tmp_path_factory):
    p = tmp_path_factory.mktemp("inception") / "inception_state.pt"
    torch.save(seeded_inception_state(4), p)
    return str(p)


def test_eval_metrics_surface(state_path):
    for name in ("fid", "is", "mmd"):
        with pytest.raises(NotImplementedError, match="psnr, ssim"):
            EvalMetrics(_cfg(["ssim", "psnr", name]))
    m = EvalMetrics(_cfg(["fid", "ssim", "is", "psnr", "mmd"], state_path))
    assert m.names == ["fid", "ssim", "is", "psnr", "mmd"] and m._inception is not None
    assert m._inception.want_acts and m._inception.want_probs
    assert len(m.state_dict()) == 0
    m2 = EvalMetrics(_cfg(["psnr", "is"]), inception_weights=M.inception_state_dict(state_path))
    assert m2.names == ["psnr", "is"] and not m2._inception.want_acts and m2._inception.want_probs
    ext = M.InceptionV3.from_file(state_path)
    m3 = EvalMetrics(_cfg(["mmd", "fid"]), inception_weights=ext)
    assert m3._inception.extractor is ext and not m3._inception.want_probs
    assert all(np.isnan(v) for v in m3.compute().values()) and list(m3.compute()) == ["eval/mmd", "eval/fid"]
    with pytest.raises(NotImplementedError, match="psnr, ssim"):
        EvalMetrics(_cfg(["psnr", "fid", "fvd"], state_path))


def test_metric_calculator_surface(state_path):
    with pytest.raises(ValueError, match="inception_weights"):
        M.MetricCalculator(("fid", "is", "mmd"))
    for name in ("ssim", "psnr"):
        with pytest.raises(NotImplementedError, match="EvalMetrics"):
            M.MetricCalculator(("fid", name), inception_weights=state_path)
    with pytest.raises(NotImplementedError, match="EvalMetrics"):
        M.MetricCalculator()          # the reference's default asks for 'ssim' and 'psnr'
    mc = M.MetricCalculator(("is", "fid", "mmd"), log_prefix="val", inception_weights=state_path)
    assert len(mc.state_dict()) == 0
    out = mc.gather()
    assert list(out) == ["val/fid", "val/mmd", "val/is"] and all(np.isnan(v) for v in out.values())
    with pytest.raises(RuntimeError, match="no CPU path"):
        mc([torch.zeros(3, 32, 32)], [torch.zeros(3, 32, 32)])
    mc.reset()


# ---- header and C ABI -------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_agree():
    src = open(HEADER).read()
    for name in ("UNITS", "FEATURES", "CLASSES", "INPUT", "POOL_AVG3", "POOL_MAX3S2"):
        value = int(re.search(r"#define TTV_INCEPTION_%s (\d+)" % name, src).group(1))
        assert value == getattr(_lib, f"TTV_INCEPTION_{name}"), name
    for struct, cls in (("ttv_inception_unit", _lib.InceptionUnit), ("ttv_inception_weights", _lib.InceptionWeights)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, flags=re.S).group(1)
        fields = [re.sub(r"\[.*\]", "", d.split()[-1].lstrip("*")) for d in (s.strip() for s in body.split(";")) if d]
        assert fields == [f[0] for f in cls._fields_], struct
    assert C.sizeof(_lib.InceptionUnit) == 3 * 8
    assert C.sizeof(_lib.InceptionWeights) == (3 * 94 + 2) * 8
    for sym in ("ttv_inception_workspace_bytes", "ttv_inception_preprocess", "ttv_inception_features", "ttv_inception_conv2d",
                "ttv_inception_pool2d"):
        decl = re.search(r"\b%s\((.*?)\);" % sym, src, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SYMBOLS[sym][1]), sym


@pytest.fixture(scope="module")
def handle():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


def test_cabi_argument_checks(handle):
    assert handle.ttv_inception_workspace_bytes(0) == -1
    assert handle.ttv_inception_workspace_bytes(_lib.TTV_MAX_CLIPS_PER_LAUNCH + 1) == -1
    one = handle.ttv_inception_workspace_bytes(1)
    assert one >= (2 * 147 * 147 * 64 + 2 * 35 * 35 * 96 + 35 * 35 * 288) * 4
    assert handle.ttv_inception_workspace_bytes(64) <= 64 * one
    fake = 1 << 20     # never dereferenced: every call below fails its argument checks first
    imgs = (C.c_void_p * 1)(fake)
    dims = (C.c_int64 * 3)(32, 48, 32 * 48)
    pre = handle.ttv_inception_preprocess
    assert pre(imgs, dims, 0, _lib.TTV_F32, 0, fake, None) == 1
    assert pre(imgs, dims, 65, _lib.TTV_F32, 0, fake, None) == 1
    assert pre(imgs, dims, 1, 7, 0, fake, None) == 1
    assert pre(imgs, dims, 1, _lib.TTV_F32, 0, None, None) == 1
    assert pre(imgs, (C.c_int64 * 3)(0, 48, 48), 1, _lib.TTV_F32, 0, fake, None) == 1
    assert pre(imgs, (C.c_int64 * 3)(32, 48, 100), 1, _lib.TTV_F32, 0, fake, None) == 1          # channels would overlap
    assert pre((C.c_void_p * 1)(None), dims, 1, _lib.TTV_F32, 0, fake, None) == 1
    assert b"inception preprocess" in handle.ttv_error_string()
    w = _lib.InceptionWeights()
    feat = handle.ttv_inception_features
    assert feat(C.byref(w), fake, 1, fake, fake, fake, 1 << 40, None) == 1            # weights missing
    for i in range(_lib.TTV_INCEPTION_UNITS):
        w.unit[i].w = w.unit[i].scale = w.unit[i].shift = fake
    assert feat(C.byref(w), fake, 1, fake, fake, fake, 1 << 40, None) == 1            # probs wanted, fc missing
    assert b"fc" in handle.ttv_error_string()
    assert feat(C.byref(w), fake, 0, fake, None, fake, 1 << 40, None) == 1            # n = 0
    assert feat(C.byref(w), fake, 1, fake, None, fake, 16, None) == 1                 # workspace too small
    assert b"workspace" in handle.ttv_error_string()
    assert feat(C.byref(w), fake + 4, 1, fake, None, fake, 1 << 40, None) == 1        # misaligned input
    assert feat(C.byref(w), fake, 1, None, None, fake, 1 << 40, None) == 1            # null acts
    w.unit[40].w = fake + 4
    assert feat(C.byref(w), fake, 1, fake, None, fake, 1 << 40, None) == 1            # misaligned weight image
    assert feat(None, fake, 1, fake, None, fake, 1 << 40, None) == 1
    conv = handle.ttv_inception_conv2d
    x = [fake, 1, 8, 8, 16]

    def c(kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, wp=fake, cout=16, y=fake, ldc=16, off=0, xs=x):
        return conv(*xs, kh, kw, sh, sw, ph, pw, wp, None, None, cout, 1, y, ldc, off, None)
    assert c(kh=8) == 1 and c(kw=0) == 1
    assert c(sh=3) == 1 and c(sw=0) == 1
    assert c(ph=3) == 1 and c(pw=-1) == 1
    assert c(kh=7, kw=7, ph=0, pw=0, xs=[fake, 1, 5, 8, 16]) == 1      # the kernel does not fit
    assert c(cout=18, ldc=18) == 1
    assert c(ldc=20, off=8) == 1
    assert c(wp=None) == 1 and c(y=None) == 1 and c(xs=[None, 1, 8, 8, 16]) == 1
    assert c(xs=[fake + 4, 1, 8, 8, 16]) == 1
    assert c(xs=[fake, 0, 8, 8, 16]) == 1
    assert b"inception conv2d" in handle.ttv_error_string()
    pool = handle.ttv_inception_pool2d
    assert pool(fake, 1, 8, 8, 16, 2, fake, 16, 0, None) == 1                          # mode
    assert pool(fake, 1, 2, 8, 16, _lib.TTV_INCEPTION_POOL_MAX3S2, fake, 16, 0, None) == 1
    assert pool(fake, 1, 8, 8, 16, _lib.TTV_INCEPTION_POOL_AVG3, fake, 20, 8, None) == 1
    assert pool(fake, 1, 8, 8, 0, _lib.TTV_INCEPTION_POOL_AVG3, fake, 16, 0, None) == 1
    assert pool(None, 1, 8, 8, 16, _lib.TTV_INCEPTION_POOL_AVG3, fake, 16, 0, None) == 1
    assert b"inception pool2d" in handle.ttv_error_string()


# ---- the restatement --------------------------------------------------------------------------------------------------------
def test_restatement_matches_loops():
    g = torch.Generator().manual_seed(1)
    for H, W, k, s, p in [(5, 6, (3, 3), (1, 1), (1, 1)), (9, 11, (3, 3), (2, 2), (0, 0)), (5, 7, (1, 7), (1, 1), (0, 3)),
                          (7, 5, (7, 1), (1, 1), (3, 0)), (6, 5, (5, 5), (1, 1), (2, 2)), (4, 5, (1, 3), (1, 1), (0, 1)),
                          (4, 5, (3, 1), (1, 1), (1, 0)), (4, 3, (1, 1), (1, 1), (0, 0))]:
        x = torch.randn(2, 3, H, W, generator=g, dtype=torch.float64)
        w = torch.randn(4, 3, *k, generator=g, dtype=torch.float64)
        got = R.conv2d(x, w, s, p)
        assert got.shape[2:] == (M.conv_out(H, k[0], s[0], p[0]), M.conv_out(W, k[1], s[1], p[1]))
        np.testing.assert_allclose(got.numpy(), R.conv2d_loop(x.numpy(), w.numpy(), s, p), rtol=1e-12, atol=1e-12)
    x = torch.randn(2, 3, 9, 11, generator=g, dtype=torch.float64)
    np.testing.assert_allclose(R.avgpool3(x).numpy(), R.avgpool3_loop(x.numpy()), rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(R.maxpool3s2(x).numpy(), R.maxpool3s2_loop(x.numpy()))
    assert R.maxpool3s2(x).shape[2:] == (4, 5)
    # the corner of the padded average divides by 9 although 4 cells are inside
    np.testing.assert_allclose(float(R.avgpool3(torch.ones(1, 1, 4, 4, dtype=torch.float64))[0, 0, 0, 0]), 4 / 9, rtol=1e-15)


def test_restated_preprocess_matches_torch_upsample():
    g = torch.Generator().manual_seed(2)
    up = torch.nn.Upsample(size=(299, 299), mode="bilinear", align_corners=True)
    for shape in [(3, 40, 50), (3, 300, 260), (3, 1, 7), (3, 299, 299)]:
        x = torch.rand(shape, generator=g) * 2.4 - 1.2
        for clamp in (False, True):
            want = up((x.clamp(-1, 1) if clamp else x)[None])[0].double()
            torch.testing.assert_close(R.preprocess(x, clamp), want, rtol=0, atol=1e-6)      # torch blends in the input's fp32
    assert torch.equal(R.preprocess(x), x.double())      # 299 -> 299 is the identity


def test_seeded_network_data_is_not_degenerate():
    """What the GPU tests' whole-network comparison rests on: with the seeded weights and frames no frame has more than half of its
    2048 acts at zero, and no frame's largest softmax probability exceeds 0.5 (float64)."""
    sd = seeded_inception_state(R.NETWORK_STATE_SEED)
    frames = R.seeded_frames(R.NETWORK_FRAME_SHAPES, R.NETWORK_FRAME_SEED)
    acts, probs = R.features(torch.stack([R.preprocess(f) for f in frames]), sd)
    assert acts.shape == (3, 2048) and probs.shape == (3, 1000) and acts.dtype == torch.float64
    torch.testing.assert_close(probs.sum(1), torch.ones(3, dtype=torch.float64), rtol=1e-12, atol=0)
    for i in range(3):
        zeros, pmax = int((acts[i] == 0).sum()), float(probs[i].max())
        print(f"frame {i}: {zeros} of 2048 acts are zero, largest probability {pmax:.4f}")
        assert zeros <= 1024 and pmax <= 0.5
    assert float((acts[0] - acts[1]).abs().max()) > 1e-3       # the frames differ
