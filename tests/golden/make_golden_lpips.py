"""Golden fixture for the LPIPS / Gram perceptual terms: runs the REFERENCE's own code (model/metrics/lpips_gram.py LPIPS and
model/losses/loss_module.py ReconstructionLoss with perceptual_weight = 1, gram_weight > 0, disc_weight = 0) on the CPU in fp32.

Run in the build container only (needs the reference checkout):   python tests/golden/make_golden_lpips.py

torchvision is not installed, so stand-ins are put in place before import:
  * torchvision.models.vgg16(pretrained=...) returns an object whose `.features` is the VGG16 features architecture (13 3x3
    convolutions with bias, ReLU, 2x2/2 max-pools, torchvision's indices 0 .. 30);
  * torchvision.transforms.v2.functional.resize(x, size=s, interpolation=BICUBIC, antialias=False) is torchvision's tensor resize:
    short edge -> s, long edge int(s * long / short), F.interpolate(mode="bicubic", align_corners=False).
LPIPS.load_from_pretrained (a network download) is bypassed; the weights come from titok_video_amd.synthetic.seeded_lpips_state
(He-normal convolutions, |N(0,1)| / C lin weights) and only its seed is stored.  flash_attn / xformers as in make_golden.py.

Inputs are not stored: they are re-drawn from the seeds below (a fingerprint of each is stored).  Recorded (fp32, CPU):
  * LPIPS on two 128 x 128 pairs and one 48 x 80 pair: lpips[B], gram[B], d sum(lpips) / d input (full), and d sum(gram) / d input
    as projections on seeded random vectors (PROJ per image).
  * ReconstructionLoss generator step on ragged clips (one with H < 128: forced resize; one 168 x 136) under random.seed(RSEED):
    the loss dictionary, the log of every random.random / random.randrange call preprocess made, a fingerprint (sum, sum of
    squares) of every crop, and d total / d recon per clip as projections on seeded random vectors plus its norm.
"""
from __future__ import annotations

import os
import random
import sys
import types
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (sets sys.path for the reference and this repo)

WEIGHT_SEED = 11
INPUT_SEED = 5
PAIR_SHAPES = [(128, 128), (128, 128), (48, 80)]
CLIP_SHAPES = [(3, 3, 168, 136), (3, 2, 96, 160), (3, 2, 128, 128)]
CLIP_SEED = 9
RSEED = 1234
SAMPLES = 4          # perceptual_samples_per_step -> 5 crops
GRAM_WEIGHT = 0.5
PROJ = 6


def vgg_features():
    layers, cin = [], 3
    for v in [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"]:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    return nn.Sequential(*layers)


def tv_resize(x, size, interpolation=None, antialias=False):
    H, W = x.shape[-2:]
    short, long = (W, H) if W <= H else (H, W)
    new_short, new_long = size, int(size * long / short)
    new_w, new_h = (new_short, new_long) if W <= H else (new_long, new_short)
    return F.interpolate(x[None], size=(new_h, new_w), mode="bicubic", align_corners=False)[0]


def install_lpips_standins():
    tv = types.ModuleType("torchvision")
    models = types.ModuleType("torchvision.models")
    models.vgg16 = lambda pretrained=True, **kw: SimpleNamespace(features=vgg_features())
    tvt = types.ModuleType("torchvision.transforms")
    v2 = types.ModuleType("torchvision.transforms.v2")
    v2.functional = SimpleNamespace(resize=tv_resize)
    tvf = types.ModuleType("torchvision.transforms.functional")
    tvf.InterpolationMode = SimpleNamespace(BICUBIC="bicubic")
    tvt.v2, tvt.functional = v2, tvf
    tv.models, tv.transforms = models, tvt
    for name, mod in [("torchvision", tv), ("torchvision.models", models), ("torchvision.transforms", tvt),
                      ("torchvision.transforms.v2", v2), ("torchvision.transforms.functional", tvf)]:
        sys.modules[name] = mod


def loss_config():
    return SimpleNamespace(
        tokenizer=SimpleNamespace(losses=SimpleNamespace(disc_weight=0.0, perceptual_weight=1.0, gram_weight=GRAM_WEIGHT,
                                                         perceptual_samples_per_step=SAMPLES, perceptual_sampling_size=128)),
        discriminator=SimpleNamespace(model=SimpleNamespace(patch_size=[4, 8, 8], model_size="tiny"),
                                      losses=SimpleNamespace(gp_weight=0.1, gp_noise=0.1, centering_weight=0.01)),
        training=SimpleNamespace(main=SimpleNamespace(torch_compile=False, max_steps=1000)))


def projections(shape, seed, k=PROJ):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((k,) + tuple(shape), generator=g, dtype=torch.float64)


def project(grad, seed):
    v = projections(grad.shape, seed)
    return (v * grad.double()[None]).flatten(1).sum(1).numpy()


def main():
    torch.set_num_threads(16)
    MG.install_standins()
    install_lpips_standins()
    from titok_video_amd.synthetic import seeded_lpips_state
    import model.metrics.lpips_gram as RL
    RL.LPIPS.load_from_pretrained = lambda self, name="vgg_lpips": None
    from model.losses.loss_module import ReconstructionLoss

    sd = seeded_lpips_state(WEIGHT_SEED)
    lp = RL.LPIPS().eval()
    lp.load_state_dict(sd, strict=True)
    out = {"weight_seed": np.int64(WEIGHT_SEED), "input_seed": np.int64(INPUT_SEED), "pair_shapes": np.array(PAIR_SHAPES, np.int32),
           "clip_shapes": np.array(CLIP_SHAPES, np.int32), "clip_seed": np.int64(CLIP_SEED), "rseed": np.int64(RSEED),
           "samples": np.int64(SAMPLES), "gram_weight": np.float64(GRAM_WEIGHT), "proj": np.int64(PROJ)}

    # ---- LPIPS pairs ----
    g = torch.Generator().manual_seed(INPUT_SEED)
    for i, (H, W) in enumerate(PAIR_SHAPES):
        y = torch.rand((1, 3, H, W), generator=g) * 2 - 1
        x = (0.7 * y + 0.3 * (torch.rand((1, 3, H, W), generator=g) * 2 - 1)).requires_grad_(True)
        out[f"pair{i}_input_fp"] = np.float64(x.detach().double().abs().sum())     # inputs are re-drawn from the seed by the tests
        l, gr = lp(x, y)
        (gx,) = torch.autograd.grad(l.sum(), x, retain_graph=True)
        (gg,) = torch.autograd.grad(gr.sum(), x)
        out[f"pair{i}_lpips"], out[f"pair{i}_gram"] = MG.np32(l.detach()), MG.np32(gr.detach())
        out[f"pair{i}_dlpips"] = MG.np32(gx[0])
        out[f"pair{i}_dgram_proj"] = project(gg[0], 100 + i)
        out[f"pair{i}_dgram_norm"] = np.float64(gg.double().norm())

    # ---- ReconstructionLoss generator step ----
    mod = ReconstructionLoss(loss_config())
    mod.perceptual_model.load_state_dict(sd, strict=True)
    g = torch.Generator().manual_seed(CLIP_SEED)
    target = [torch.rand(s, generator=g) * 2 - 1 for s in CLIP_SHAPES]
    recon = [(1.1 * t + 0.2 * torch.randn(t.shape, generator=g)).requires_grad_(True) for t in target]   # some values outside [-1, 1]
    for i, (t, r) in enumerate(zip(target, recon)):
        out[f"clip{i}_fp"] = np.array([float(t.double().abs().sum()), float(r.detach().double().abs().sum())])
    log = []
    real_random, real_randrange = random.random, random.randrange

    def rec_random():
        v = real_random()
        log.append((0.0, 0.0, v))
        return v

    def rec_randrange(a, b):
        v = real_randrange(a, b)
        log.append((float(a), float(b), float(v)))
        return v

    crops = {}
    real_pre = mod.perceptual_preprocess

    def rec_pre(target_frames, recon_frames):
        r, t = real_pre(target_frames, recon_frames)
        crops["recon"], crops["target"] = r.detach(), t.detach()
        return r, t

    mod.perceptual_preprocess = rec_pre
    random.seed(RSEED)
    random.random, random.randrange = rec_random, rec_randrange
    try:
        tot, d = mod(target, recon)
    finally:
        random.random, random.randrange = real_random, real_randrange
    out["random_log"] = np.array(log, dtype=np.float64)
    for k in ("recon", "target"):
        c = crops[k].double()
        out[f"crops_{k}_fp"] = np.stack([c.flatten(1).sum(1).numpy(), c.square().flatten(1).sum(1).numpy()], axis=1)
    out["gen_total"] = MG.np32(tot.detach())
    out["gen_keys"] = np.array(list(d.keys()))
    for k, v in d.items():
        out["gen_" + k.split("/")[1]] = MG.np32(v)
    grads = torch.autograd.grad(tot, recon)
    for i, gr in enumerate(grads):
        out[f"clip{i}_dtotal_proj"] = project(gr, 200 + i)
        out[f"clip{i}_dtotal_norm"] = np.float64(gr.double().norm())
    MG.save("lpips_kat.npz", **out)


if __name__ == "__main__":
    main()
