"""CPU checks of the LPIPS / Gram perceptual terms: the float64 restatement (tests/lpips_ref.py) against the reference's own fp32
outputs (tests/golden/lpips_kat.npz), the crop selection of the mirror's perceptual_preprocess, weight-file composition, the
constructor guard, trainer checkpoints and the C-ABI exports.  No GPU."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_ref as R  # noqa: E402

from titok_video_amd import _lib  # noqa: E402
from titok_video_amd import checkpoint as CK  # noqa: E402
from titok_video_amd.model.losses import ReconstructionLoss  # noqa: E402
from titok_video_amd.model.metrics.lpips_gram import LPIPS, lpips_state_dict  # noqa: E402
from titok_video_amd.model.titok import TiTok  # noqa: E402
from titok_video_amd.synthetic import seeded_lpips_state  # noqa: E402

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FP32_VALUE = 1e-5      # restatement vs the reference's fp32 run: measured <= 1.6e-7 (values), <= 1.2e-6 (gradients)
FP32_GRAD = 1e-5


def fixture():
    return np.load(os.path.join(G, "lpips_kat.npz"))


def loss_config(d, perceptual_weight=1.0, gram_weight=None, disc_weight=0.0, weights=None):
    losses = SimpleNamespace(disc_weight=disc_weight, perceptual_weight=perceptual_weight,
                             gram_weight=float(d["gram_weight"]) if gram_weight is None else gram_weight,
                             perceptual_samples_per_step=int(d["samples"]), perceptual_sampling_size=128)
    if weights is not None:
        losses.perceptual_weights = weights
    return SimpleNamespace(
        tokenizer=SimpleNamespace(model=SimpleNamespace(patch_size=[4, 8, 8], fsq_levels=[7, 5, 5, 5, 5], encoder_size="tiny",
                                                        decoder_size="tiny"), losses=losses),
        discriminator=SimpleNamespace(model=SimpleNamespace(patch_size=[4, 8, 8], model_size="tiny"),
                                      losses=SimpleNamespace(gp_weight=0.1, gp_noise=0.1, centering_weight=0.01)),
        training=SimpleNamespace(main=SimpleNamespace(torch_compile=False, max_steps=10)))


def pair_result(sd, x, y, **kw):
    x = x.double().requires_grad_(True)
    lp, gr = R.lpips_gram(sd, x, y.double(), **kw)
    (gx,) = torch.autograd.grad(lp.sum(), x, retain_graph=True)
    (gg,) = torch.autograd.grad(gr.sum(), x)
    return lp.detach(), gr.detach(), gx[0], gg[0]


def pair_errors(d, i, res):
    lp, gr, gx, gg = res
    return (max(R.rel_err(lp, d[f"pair{i}_lpips"]), R.rel_err(gr, d[f"pair{i}_gram"])),
            max(R.rel_err(gx, d[f"pair{i}_dlpips"]), R.rel_err(R.project(gg, 100 + i, int(d["proj"])), d[f"pair{i}_dgram_proj"])))


def test_restatement_matches_reference_fixture():
    d = fixture()
    sd = seeded_lpips_state(int(d["weight_seed"]))
    for i, (x, y) in enumerate(R.pair_inputs(d)):
        assert abs(float(x.double().abs().sum()) - float(d[f"pair{i}_input_fp"])) < 1e-6 * float(d[f"pair{i}_input_fp"])
        ev, eg = pair_errors(d, i, pair_result(sd, x, y))
        assert ev < FP32_VALUE and eg < FP32_GRAD, (i, ev, eg)


@pytest.mark.parametrize("variant", ["flip", "halo_shift"])
def test_checker_rejects_wrong_restatements(variant):
    """A flipped 3x3 kernel or a one-pixel halo shift must fail the same bounds on every pair (the gradient discriminates)."""
    d = fixture()
    sd = seeded_lpips_state(int(d["weight_seed"]))
    for i, (x, y) in enumerate(R.pair_inputs(d)):
        ev, eg = pair_errors(d, i, pair_result(sd, x, y, **{variant: True}))
        assert eg > 100 * FP32_GRAD, (variant, i, ev, eg)


def frames_of(target, recon):
    tf, rf = [], []
    for t, r in zip(target, recon):
        tf += t.unbind(1)
        rf += r.unbind(1)
    return tf, rf


def test_preprocess_picks_the_reference_frames_and_offsets():
    d = fixture()
    mod = ReconstructionLoss(loss_config(d), perceptual_weights=seeded_lpips_state(int(d["weight_seed"])))
    target, recon = R.clip_inputs(d)
    for i, (t, r) in enumerate(zip(target, recon)):
        np.testing.assert_allclose([float(t.double().abs().sum()), float(r.double().abs().sum())], d[f"clip{i}_fp"], rtol=1e-6)
    import random
    random.seed(int(d["rseed"]))
    with R.RandomLog() as log:
        rc, tc = mod.perceptual_preprocess(*frames_of(target, recon))
    np.testing.assert_array_equal(log.array(), d["random_log"])
    assert rc.shape == (int(d["samples"]) + 1, 3, 128, 128) and tc.shape == rc.shape
    for name, c in (("recon", rc), ("target", tc)):
        c = c.double()
        fp = np.stack([c.flatten(1).sum(1).numpy(), c.square().flatten(1).sum(1).numpy()], axis=1)
        np.testing.assert_allclose(fp, d[f"crops_{name}_fp"], rtol=1e-5, atol=1e-3)


def test_generator_perceptual_terms_restated_match_reference():
    """The mirror's crops fed to the float64 restatement give the reference's loss dictionary and d total / d recon."""
    d = fixture()
    sd = seeded_lpips_state(int(d["weight_seed"]))
    mod = ReconstructionLoss(loss_config(d), perceptual_weights=sd)
    target, recon = R.clip_inputs(d)
    recon = [r.double().requires_grad_(True) for r in recon]
    target = [t.double() for t in target]
    import random
    random.seed(int(d["rseed"]))
    rc, tc = mod.perceptual_preprocess(*frames_of(target, recon))
    lp, gr = R.lpips_gram(sd, rc, tc)
    l1 = torch.stack([(t - r).abs().mean() for t, r in zip(target, recon)]).mean()
    gw = float(d["gram_weight"])
    total = l1 + lp.mean() + gw * gr.mean()
    for name, v in (("recon_loss", l1), ("perceptual_loss", lp.mean()), ("gram_loss", gr.mean()), ("total_loss", total)):
        assert R.rel_err(v.detach().reshape(1), np.asarray(d["gen_" + name]).reshape(1)) < FP32_VALUE, name
    # The Gram gradient is ill-conditioned in fp32 (G0 - G1 cancels): the same restatement run in fp32 moves the projections by
    # up to 1.1e-2 of their largest value from float64, so the reference's fp32 gradient is held to 3e-2 / 1e-2 (norm).
    grads = torch.autograd.grad(total, recon)
    for i, g in enumerate(grads):
        assert R.rel_err(R.project(g, 200 + i, int(d["proj"])), d[f"clip{i}_dtotal_proj"]) < 3e-2, i
        assert abs(float(g.norm()) - float(d[f"clip{i}_dtotal_norm"])) < 1e-2 * float(d[f"clip{i}_dtotal_norm"])


def test_lpips_state_dict_composes_upstream_files(tmp_path):
    ref = seeded_lpips_state(3)
    vgg = {}
    for k, v in ref.items():
        if k.startswith("net."):
            _, _, idx, p = k.split(".")
            vgg[f"features.{idx}.{p}"] = v
    vgg["classifier.0.weight"] = torch.zeros(2, 2)                          # torchvision's file carries the classifier too
    lin = {k: v for k, v in ref.items() if k.startswith("lin")}
    torch.save(vgg, tmp_path / "vgg16.pth")
    torch.save(lin, tmp_path / "vgg.pth")
    sd = lpips_state_dict(str(tmp_path / "vgg16.pth"), str(tmp_path / "vgg.pth"))
    assert list(sd.keys()) == list(ref.keys()) == list(LPIPS().state_dict().keys())
    for k in ref:
        assert torch.equal(sd[k], ref[k]), k
    torch.save(sd, tmp_path / "lpips.pth")
    m = LPIPS.from_file(str(tmp_path / "lpips.pth"))
    assert all(not p.requires_grad for p in m.parameters())
    d = fixture()
    mod = ReconstructionLoss(loss_config(d, weights=str(tmp_path / "lpips.pth")))   # the config key
    assert torch.equal(mod.perceptual_model.net.slice5._modules["28"].bias, ref["net.slice5.28.bias"])
    del vgg["features.28.bias"]
    torch.save(vgg, tmp_path / "vgg16.pth")
    with pytest.raises(KeyError, match="features.28.bias"):
        lpips_state_dict(str(tmp_path / "vgg16.pth"), str(tmp_path / "vgg.pth"))


def test_guard_without_weights_names_the_key():
    d = fixture()
    for pw, gw in ((1.0, 0.0), (0.0, 0.5)):
        with pytest.raises(NotImplementedError, match="tokenizer.losses.perceptual_weights"):
            ReconstructionLoss(loss_config(d, perceptual_weight=pw, gram_weight=gw))
    assert not hasattr(ReconstructionLoss(loss_config(d, perceptual_weight=0.0, gram_weight=0.0)), "perceptual_model")


def test_trainer_checkpoint_leaves_out_the_perceptual_model():
    d = fixture()
    cfg = loss_config(d, disc_weight=0.4)
    lm = ReconstructionLoss(cfg, perceptual_weights=seeded_lpips_state(1))
    assert any(k.startswith("perceptual_model.") for k in lm.state_dict())
    out = CK.trainer_state_dict(TiTok(cfg), lm)
    assert out and not any("perceptual_model" in k for k in out)
    assert any(k.startswith("loss_module.disc_model.") for k in out)


def test_cabi_exports_lpips_symbols():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    h = _lib.lib()
    for name in ("ttv_lpips_tape_bytes", "ttv_lpips_workspace_bytes", "ttv_lpips_forward", "ttv_lpips_backward",
                 "ttv_lpips_conv_workspace_bytes", "ttv_lpips_conv3x3", "ttv_lpips_maxpool", "ttv_lpips_maxpool_backward"):
        assert name in _lib.SYMBOLS
        getattr(h, name)
    # host-side shape rules (no device work): bad shapes / dtypes give -1
    assert h.ttv_lpips_tape_bytes(2, 128, 128, _lib.TTV_BF16) > 2 * 2 * 128 * 128 * 64 * 2
    assert h.ttv_lpips_workspace_bytes(2, 128, 128, _lib.TTV_F32) > 0
    assert h.ttv_lpips_tape_bytes(2, 120, 128, _lib.TTV_BF16) == -1
    assert h.ttv_lpips_tape_bytes(2, 128, 128, 7) == -1
    assert h.ttv_lpips_tape_bytes(0, 128, 128, _lib.TTV_BF16) == -1
    assert _lib.C.sizeof(_lib.LpipsWeights) == 8 * (13 * 3 + 5)
