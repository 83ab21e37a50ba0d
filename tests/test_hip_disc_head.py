"""`ttv_disc_head` (csrc/ttv_disc.hip) through `DiscHead` on the MI355X against the float64 torch restatement of
tests/disc_head_ref.py, values and `autograd.grad`, and the reported keys of `ReconstructionLoss` on both routes.  `-m gpu`.

THE BOUND is counted in tests/disc_head_ref.py from the kernel's rounding steps (logit sums of 4 values, the softplus / square of
every clip, means over at most 67 clips - the issue's ceiling of 268 fp32 terms is 67 clips x 4 tokens - and the weighted total); it
comes to about 1e-6 relative for fp32 inputs and is printed per case.  Grid: n in {1, 3, 5, 67} (67: more than one wave, a multiple
of nothing), generator and discriminator mode, the penalty (4 groups) on and off, centering on and off, fp32 and bf16 inputs, one
tensor and two.  Inputs hold real - fake beyond +-20 on both sides (both softplus branches and their derivatives) and equal logits."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import disc_head_ref as HR  # noqa: E402

from titok_video_amd import _lib  # noqa: E402
from titok_video_amd.model.losses import ReconstructionLoss  # noqa: E402
from titok_video_amd.model.losses.loss_module import DiscHead  # noqa: E402
from titok_video_amd.synthetic import seeded_tower_state, synthetic_clips  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R = 4
GP_SCALE, CENTER = 0.1 / 0.1 ** 2, 0.01
SLOT = {"total": 0, "loss": 1, "logits_relative": 2, "r1_penalty": 3, "r2_penalty": 4, "centering_loss": 5}


def run_head(x, mode, n, gp_scale, center, two):
    """x: CPU [G, n, R] -> (terms on the CPU, gradient shaped like x) through DiscHead and autograd.grad."""
    code = _lib.TTV_DISC_HEAD_GENERATOR if mode == "generator" else _lib.TTV_DISC_HEAD_DISCRIMINATOR
    G = x.shape[0]
    if two:
        a = x[:G // 2].reshape(-1, 1).to(DEV).requires_grad_(True)
        b = x[G // 2:].reshape(-1, 1).to(DEV).requires_grad_(True)
        total, terms = DiscHead.apply(code, n, R, gp_scale, center, a, b)
        ga, gb = torch.autograd.grad(total * 2.0, [a, b])                  # an upstream gradient other than 1 (a power of two: exact)
        assert ga.dtype == x.dtype and ga.shape == a.shape and gb.shape == b.shape
        grad = torch.cat([ga, gb]).double().cpu().reshape(x.shape) / 2.0
    else:
        a = x.reshape(-1, 1).to(DEV).requires_grad_(True)
        total, terms = DiscHead.apply(code, n, R, gp_scale, center, a, None)
        (ga,) = torch.autograd.grad(total, [a])
        assert ga.dtype == x.dtype and ga.shape == a.shape
        grad = ga.double().cpu().reshape(x.shape)
    assert total.requires_grad and not terms.requires_grad and terms.shape == (8,) and terms.dtype == torch.float32
    assert float(total) == float(terms[0])
    return terms.double().cpu(), grad


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("n", [1, 3, 5, 67])
def test_terms_and_gradient_against_float64(n, dt):
    dtype = {"f32": torch.float32, "bf16": torch.bfloat16}[dt]
    cases = [("generator", 2, 0.0, 0.0)]
    cases += [("discriminator", G, GP_SCALE if G == 4 else 0.0, c) for G in (2, 4) for c in (0.0, CENTER)]
    worst = 0.0
    for mode, G, gp_scale, center in cases:
        x = HR.head_inputs(G, n, R, dtype, seed=100 * n + G)
        want, tol, want_grad, grad_tol = HR.head_ref(x, mode, n, R, gp_scale, center, dtype)
        if n >= 2:
            m = x.double().mean(-1)
            assert float((m[0] - m[1]).max()) > 20 and float((m[0] - m[1]).min()) < -20
        for two in (False, True):
            terms, grad = run_head(x, mode, n, gp_scale, center, two)
            for name, slot in SLOT.items():
                if name in want:
                    err = abs(float(terms[slot]) - want[name])
                    if name == "total":
                        worst = max(worst, tol[name] / abs(want[name]))
                    assert err <= tol[name], (mode, G, center, two, name, float(terms[slot]), want[name], err, tol[name])
                else:
                    assert float(terms[slot]) == 0.0, (mode, G, center, name)
            excess = (grad - want_grad).abs() - grad_tol
            assert float(excess.max()) <= 0.0, (mode, G, center, two, float(excess.max()), float(want_grad.abs().max()))
            if mode == "generator":
                assert float(grad.abs().max()) > 0
    print(f"n {n} {dt}: the largest relative bound of a total {worst:.2e}")


def test_entry_point_refuses_bad_arguments():
    t = torch.zeros(8, dtype=torch.float32, device=DEV)
    x = torch.zeros(64, dtype=torch.float32, device=DEV)
    g = torch.zeros(64, dtype=torch.float32, device=DEV)
    s = _lib.stream_ptr(torch.device(DEV))
    call = lambda mode, G, n, dt: _lib.lib().ttv_disc_head(x.data_ptr(), None, mode, G, n, R, dt, 1.0, 0.0, t.data_ptr(), g.data_ptr(), s)
    assert call(_lib.TTV_DISC_HEAD_DISCRIMINATOR, 4, 4, _lib.TTV_F32) == 0
    for bad in ((2, 2, 4, _lib.TTV_F32), (_lib.TTV_DISC_HEAD_GENERATOR, 4, 4, _lib.TTV_F32), (1, 3, 4, _lib.TTV_F32), (1, 2, 0, _lib.TTV_F32), (1, 2, 4, 7)):
        assert call(*bad) != 0, bad
    torch.cuda.synchronize()


def _config(gp_weight, centering_weight):
    return SimpleNamespace(
        tokenizer=SimpleNamespace(losses=SimpleNamespace(disc_weight=0.1, perceptual_weight=0.0, gram_weight=0.0, perceptual_samples_per_step=24,
                                                         perceptual_sampling_size=128)),
        discriminator=SimpleNamespace(model=SimpleNamespace(patch_size=[4, 8, 8], model_size="tiny"),
                                      losses=SimpleNamespace(gp_weight=gp_weight, gp_noise=0.1, centering_weight=centering_weight)),
        training=SimpleNamespace(main=SimpleNamespace(torch_compile=False, max_steps=1000)))


def test_reported_keys_equal_the_eager_route_for_each_weight_configuration(monkeypatch):
    shapes = [(4, 16, 16), (4, 8, 24)]
    target = synthetic_clips(shapes, seed=3, dtype=torch.float32, device=DEV)
    recon = [(t * 0.9).contiguous() for t in target]
    sd = seeded_tower_state("encoder", "tiny", (4, 8, 8), 3, 1, seed=5)
    for gp_weight in (0.0, 0.1):
        for centering in (0.0, 0.01):
            keys = {}
            for route in ("1", "0"):
                monkeypatch.setenv("TTV_DISC_FUSED", route)
                mod = ReconstructionLoss(_config(gp_weight, centering))
                mod.disc_model.load_state_dict(sd, strict=True)
                mod = mod.to(DEV, torch.float32)
                _, gen = mod(target, recon)
                _, disc = mod(target, recon, disc_forward=True)
                for v in list(gen.values()) + list(disc.values()):
                    assert v.dim() == 0 and not v.requires_grad and bool(torch.isfinite(v))
                keys[route] = (list(gen), list(disc))
            assert keys["1"] == keys["0"], (gp_weight, centering, keys)
            assert ("disc/r1_penalty" in keys["1"][1]) == (gp_weight > 0) and ("disc/centering_loss" in keys["1"][1]) == (centering > 0)
