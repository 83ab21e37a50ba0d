"""`ReconstructionLoss` at the tests/golden/loss_kat.npz configuration with the fused discriminator-step route (TTV_DISC_FUSED, the
default) against the eager route (TTV_DISC_FUSED=0) on the same noise, and one `gan_training_step` whose noise the kernel draws.
`-m gpu`.  fp32: the towers are the same launches on both routes, so the two differ by the head's arithmetic alone: totals and every
term agree to the bound tests/disc_head_ref.py counts for the head (evaluated on the logits of this batch), and each is within it
of the float64 restatement; discriminator parameter gradients agree to the tolerance tests/test_hip_loss.py holds them to against
torch (2e-2 per large tensor, 5e-3 over all)."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import disc_head_ref as HR  # noqa: E402

from titok_video_amd.model.losses import ReconstructionLoss  # noqa: E402
from titok_video_amd.synthetic import seeded_tower_state, synthetic_clips  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def loss_config(d):
    return SimpleNamespace(
        tokenizer=SimpleNamespace(losses=SimpleNamespace(disc_weight=float(d["disc_weight"]), perceptual_weight=0.0, gram_weight=0.0,
                                                         perceptual_samples_per_step=24, perceptual_sampling_size=128)),
        discriminator=SimpleNamespace(model=SimpleNamespace(patch_size=[4, 8, 8], model_size="tiny"),
                                      losses=SimpleNamespace(gp_weight=float(d["gp_weight"]), gp_noise=float(d["gp_noise"]),
                                                             centering_weight=float(d["centering_weight"]))),
        training=SimpleNamespace(main=SimpleNamespace(torch_compile=False, max_steps=1000)))


def rel(a, b):
    a, b = a.double().cpu().flatten(), b.double().cpu().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def test_fused_route_against_the_eager_route_fp32(monkeypatch):
    d = np.load(os.path.join(G, "loss_kat.npz"))
    shapes = [tuple(int(v) for v in s) for s in d["shapes"]]
    to = lambda xs: [x.to(DEV, torch.float32) for x in xs]
    target = to(synthetic_clips(shapes, seed=int(d["clip_seed"])))
    recon = to([torch.from_numpy(d[f"recon{i}"]) for i in range(len(shapes))])
    noise = to([torch.from_numpy(d[f"noise{i}"]) for i in range(len(shapes))])
    sd = seeded_tower_state("encoder", "tiny", (4, 8, 8), 3, 1, seed=int(d["disc_seed"]))
    mod = ReconstructionLoss(loss_config(d))
    mod.disc_model.load_state_dict(sd, strict=True)
    mod = mod.to(DEV, torch.float32)
    n = len(shapes)
    out = {}
    for route in ("1", "0"):
        monkeypatch.setenv("TTV_DISC_FUSED", route)
        mod.zero_grad(set_to_none=True)
        rec = [r.clone().requires_grad_(True) for r in recon]
        g_tot, g_parts = mod(target, rec)
        g_tot.backward()
        d_tot, d_parts = mod(target, recon, disc_forward=True, gp_noise_tensors=noise)
        d_tot.backward()
        out[route] = dict(g_tot=float(g_tot), g_parts={k: float(v) for k, v in g_parts.items()}, d_tot=float(d_tot),
                          d_parts={k: float(v) for k, v in d_parts.items()}, drecon=[r.grad.clone() for r in rec],
                          grads={k: p.grad.clone() for k, p in mod.disc_model.named_parameters()})
    fused, eager = out["1"], out["0"]
    assert list(fused["g_parts"]) == list(eager["g_parts"]) and list(fused["d_parts"]) == list(eager["d_parts"])
    # the head's bound on this batch's logits: the per-token outputs of the packed call the step makes
    with torch.no_grad():
        noisy = [t + z for t, z in zip(target, noise)] + [r + z for r, z in zip(recon, noise)]
    per_token = mod._disc_per_token(target + recon + noisy).detach().cpu()
    scale = float(d["gp_weight"]) / float(d["gp_noise"]) ** 2
    want, tol, _g, _gt = HR.head_ref(per_token, "discriminator", n, 4, scale, float(d["centering_weight"]), torch.float32)
    names = {"disc/d_loss": "loss", "disc/logits_relative": "logits_relative", "disc/r1_penalty": "r1_penalty", "disc/r2_penalty": "r2_penalty",
             "disc/centering_loss": "centering_loss", "disc/total_loss": "total"}
    assert set(names) == set(fused["d_parts"])
    for key, name in names.items():
        print(f"{key}: fused {fused['d_parts'][key]:.9g} eager {eager['d_parts'][key]:.9g} float64 {want[name]:.9g} bound {tol[name]:.3g}")
        assert abs(fused["d_parts"][key] - want[name]) <= tol[name], key
        assert abs(fused["d_parts"][key] - eager["d_parts"][key]) <= tol[name], key
    assert abs(fused["d_tot"] - eager["d_tot"]) <= tol["total"] and fused["d_tot"] == fused["d_parts"]["disc/total_loss"]
    want_g, tol_g, _g, _gt = HR.head_ref(per_token[:2 * n * 4], "generator", n, 4, 0.0, 0.0, torch.float32)
    for key in ("gen/g_loss",):
        print(f"{key}: fused {fused['g_parts'][key]:.9g} eager {eager['g_parts'][key]:.9g} float64 {want_g['loss']:.9g} bound {tol_g['loss']:.3g}")
        assert abs(fused["g_parts"][key] - eager["g_parts"][key]) <= tol_g["loss"]
    w = float(d["disc_weight"])
    assert abs(fused["g_tot"] - eager["g_tot"]) <= w * tol_g["loss"] + 1e-6 + 2.0 ** -23 * abs(eager["g_tot"])
    # the L1 term is the same launch on both routes; its blocks meet in one atomicAdd, so two runs agree to the order of that sum only
    # (the bar tests/test_hip_backward.py holds the kernel to in fp32)
    assert abs(fused["g_parts"]["gen/recon_loss"] - eager["g_parts"]["gen/recon_loss"]) < 1e-6
    for a, b in zip(fused["drecon"], eager["drecon"]):
        assert rel(a, b) < 2e-3
    num = den = 0.0
    for k, r in eager["grads"].items():
        g = fused["grads"][k]
        num += float((g.double() - r.double()).pow(2).sum())
        den += float(r.double().pow(2).sum())
        if r.numel() >= 4096:
            assert rel(g, r) < 2e-2, (k, rel(g, r))
    assert (num / den) ** 0.5 < 5e-3


def test_gan_training_step_with_generated_noise():
    from titok_video_amd.model.titok import TiTok
    from titok_video_amd.synthetic import seeded_titok_state
    from titok_video_amd.train import gan_training_step, make_discriminator_optimizer, make_optimizer
    d = np.load(os.path.join(G, "loss_kat.npz"))
    cfg = SimpleNamespace(tokenizer=SimpleNamespace(model=SimpleNamespace(patch_size=[4, 8, 8], fsq_levels=[7, 5, 5, 5, 5],
                                                                          encoder_size="tiny", decoder_size="tiny")))
    torch.manual_seed(11)
    model = TiTok(cfg)
    model.load_state_dict(seeded_titok_state(0))
    model = model.to(DEV, torch.bfloat16).train()
    lm = ReconstructionLoss(loss_config(d))
    lm.disc_model.load_state_dict(seeded_tower_state("encoder", "tiny", (4, 8, 8), 3, 1, seed=77))
    lm = lm.to(DEV, torch.bfloat16).train()
    shapes, counts = [(4, 16, 16), (8, 32, 48), (4, 8, 24)], [2, 5, 3]
    clips = synthetic_clips(shapes, seed=9, dtype=torch.bfloat16, device=DEV)
    opt_g, opt_d = make_optimizer(model), make_discriminator_optimizer(lm)
    loss_dict, _idx = gan_training_step(model, lm, clips, counts, opt_g, opt_d)
    assert lm.__dict__.get("_gp_draw") == 1                          # the step drew its noise in the kernel, once
    for k in ("gen/recon_loss", "gen/g_loss", "gen/total_loss", "disc/d_loss", "disc/logits_relative", "disc/r1_penalty", "disc/r2_penalty",
              "disc/centering_loss", "disc/total_loss"):
        assert k in loss_dict and bool(torch.isfinite(loss_dict[k]).all()), k
    assert float(loss_dict["disc/r1_penalty"]) > 0 and float(loss_dict["disc/r2_penalty"]) > 0
