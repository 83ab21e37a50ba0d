"""GPU tests of the LPIPS / Gram perceptual terms (csrc/ttv_lpips.hip, model/metrics/lpips_gram.py, ReconstructionLoss).

Single operations against float64 on the network's layer shapes (inputs and weights are bf16-representable, so one float64 result
is the reference for both dtypes), stray-write checks on NaN-padded outputs, max-pool tie routing, the whole module and the
generator step against the reference's own outputs (tests/golden/lpips_kat.npz), bit-reproducibility, and one training step."""
import os
import random
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_ref as R  # noqa: E402

from titok_video_amd import _lib  # noqa: E402
from titok_video_amd.model.losses import ReconstructionLoss  # noqa: E402
from titok_video_amd.model.metrics.lpips_gram import LPIPS, _pack_images  # noqa: E402
from titok_video_amd.synthetic import seeded_lpips_state  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (Cin, Cout, n, H, W): every layer shape of the network at its stage of a 128 x 128 crop, the split-K stages at n = 50, and the
# 48 x 80 / 16 x 16 / 160 x 160 crops' odd stages (3 x 5, 1 x 1, 80 x 80)
CONV_CASES = [(3, 64, 7, 128, 128), (64, 64, 7, 128, 128), (64, 128, 7, 64, 64), (128, 128, 7, 64, 64), (128, 256, 7, 32, 32),
              (256, 256, 7, 32, 32), (256, 512, 7, 16, 16), (512, 512, 7, 16, 16), (512, 512, 50, 8, 8), (64, 64, 1, 48, 80),
              (512, 512, 1, 3, 5), (512, 512, 50, 1, 1), (128, 128, 1, 80, 80), (64, 64, 1, 16, 16), (256, 256, 50, 4, 4)]


def bf16_exact(t):
    return t.to(torch.bfloat16).double()


def bound_check(out, ref, dtype, what):
    """Elementwise: bf16 |out - ref| <= 8e-3 |ref| + 2e-3 max|ref| (one bf16 rounding of the output plus fp32 accumulation);
    fp32 <= 1e-5 |ref| + 2e-5 max|ref|.  Returns the worst ratio err / bound (< 1 passes)."""
    out, ref = out.double().cpu(), ref.double().cpu()
    assert torch.isfinite(out).all(), what
    rel, ab = (8e-3, 2e-3) if dtype == torch.bfloat16 else (1e-5, 2e-5)
    bound = rel * ref.abs() + ab * ref.abs().max().clamp_min(1e-30)
    worst = float(((out - ref).abs() / bound).max())
    assert worst < 1.0, f"{what}: worst err / bound = {worst:.3f}"
    return worst


def run_conv(x_nhwc, w, b, mode, h_nhwc, dtype, transpose=False):
    """ttv_lpips_conv3x3 on NHWC x with the forward (or dgrad) image of w [Cout_fwd, Cin_fwd, 3, 3]; output in a NaN-padded
    buffer whose padding is checked."""
    N, H, W, Cin = x_nhwc.shape
    Cout = w.shape[1] if transpose else w.shape[0]
    mfma = dtype == torch.bfloat16 and Cin % 32 == 0 and Cout % 64 == 0
    fwd, dgr = _pack_images(w.float().to(DEV), dtype, mfma)
    img = dgr if transpose else fwd
    L = _lib.lib()
    dt = _lib.dtype_code(dtype)
    x = x_nhwc.to(DEV, dtype).contiguous()
    h = h_nhwc.to(DEV, dtype).contiguous() if h_nhwc is not None else None
    bias = b.to(DEV, torch.float32).contiguous() if b is not None else None
    total = N * H * W * Cout
    buf = torch.full((total + 256,), float("nan"), device=DEV, dtype=dtype)
    y = buf[:total]
    wsb = L.ttv_lpips_conv_workspace_bytes(N, H, W, Cin, Cout, dt)
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=DEV)
    _lib.check(L.ttv_lpips_conv3x3(x.data_ptr(), N, H, W, Cin, Cout, img.data_ptr(), _lib.ptr(bias), mode, _lib.ptr(h), y.data_ptr(), dt,
                                   ws.data_ptr(), ws.numel(), _lib.stream_ptr(DEV)), "ttv_lpips_conv3x3")
    torch.cuda.synchronize()
    assert torch.isnan(buf[total:].float()).all(), "stray write past the output"
    return y.view(N, H, W, Cout).float().cpu()


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv3x3_forward_and_dgrad_against_float64(case):
    Cin, Cout, n, H, W = case
    g = torch.Generator().manual_seed(hash(case) % 1000)
    x = bf16_exact(torch.randn((n, Cin, H, W), generator=g).relu_() if Cin > 3 else torch.randn((n, Cin, H, W), generator=g))
    w = bf16_exact(torch.randn((Cout, Cin, 3, 3), generator=g) * (2.0 / (9 * Cin)) ** 0.5)
    b = 0.05 * torch.randn((Cout,), generator=g, dtype=torch.float64)
    ref = torch.relu(F.conv2d(x, w, b, padding=1))
    xh = x.permute(0, 2, 3, 1)
    for dtype in (torch.float32, torch.bfloat16):
        out = run_conv(xh, w, b.float(), 0, None, dtype)
        bound_check(out, ref.permute(0, 2, 3, 1), dtype, f"forward {case} {dtype}")
    # dgrad: dy [n, Cout, H, W] -> dx = conv_transpose(dy, w) [n, Cin, H, W], masked by h > 0 (mode 1) or raw (mode 2)
    dy = bf16_exact(torch.randn((n, Cout, H, W), generator=g))
    dx = F.conv_transpose2d(dy, w, padding=1)
    hmask = bf16_exact(torch.randn((n, Cin, H, W), generator=g))
    dyh = dy.permute(0, 2, 3, 1)
    for dtype in (torch.float32, torch.bfloat16):
        out = run_conv(dyh, w, None, 2, None, dtype, transpose=True)
        bound_check(out, dx.permute(0, 2, 3, 1), dtype, f"dgrad {case} {dtype}")
        out = run_conv(dyh, w, None, 1, hmask.permute(0, 2, 3, 1), dtype, transpose=True)
        bound_check(out, (dx * (hmask > 0)).permute(0, 2, 3, 1), dtype, f"dgrad masked {case} {dtype}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_maxpool_and_tie_routing(dtype):
    g = torch.Generator().manual_seed(3)
    n, H, W, C = 3, 16, 24, 64
    h = bf16_exact(torch.randn((n, C, H, W), generator=g)).relu()
    # ties: whole windows of one positive value, windows with two equal maxima at different positions, all-zero windows
    h[:, :8, 0:2, 0:2] = 0.5
    h[:, 8:16, 2:4, 2:4] = torch.tensor([[0.25, 0.75], [0.75, 0.5]], dtype=torch.float64)
    h[:, 16:24, 4:6, 4:6] = 0.0
    dy = bf16_exact(torch.randn((n, C, H // 2, W // 2), generator=g))
    add = torch.randn((n, C, H, W), generator=g)
    hr = h.clone().requires_grad_(True)
    pooled = F.max_pool2d(hr, 2, 2)                       # CPU max_pool2d routes to the first maximum
    (routed,) = torch.autograd.grad(pooled, hr, dy)
    ref_dx = (routed + add.double()) * (h > 0)
    L = _lib.lib()
    dt = _lib.dtype_code(dtype)
    hd = h.permute(0, 2, 3, 1).to(DEV, dtype).contiguous()
    y = torch.full((n * (H // 2) * (W // 2) * C + 64,), float("nan"), device=DEV, dtype=dtype)
    _lib.check(L.ttv_lpips_maxpool(hd.data_ptr(), n, H, W, C, y.data_ptr(), dt, _lib.stream_ptr(DEV)), "maxpool")
    dyd = dy.permute(0, 2, 3, 1).to(DEV, dtype).contiguous()
    addd = add.permute(0, 2, 3, 1).to(DEV).contiguous()
    dx = torch.full((n * H * W * C + 64,), float("nan"), device=DEV, dtype=dtype)
    _lib.check(L.ttv_lpips_maxpool_backward(dyd.data_ptr(), addd.data_ptr(), hd.data_ptr(), n, H, W, C, dx.data_ptr(), dt,
                                            _lib.stream_ptr(DEV)), "maxpool backward")
    torch.cuda.synchronize()
    npool = n * (H // 2) * (W // 2) * C
    assert torch.isnan(y[npool:].float()).all() and torch.isnan(dx[n * H * W * C:].float()).all()
    assert torch.equal(y[:npool].view(n, H // 2, W // 2, C).double().cpu(), pooled.detach().permute(0, 2, 3, 1))
    got = dx[:n * H * W * C].view(n, H, W, C).double().cpu()
    bound_check(got, ref_dx.permute(0, 2, 3, 1), dtype, "maxpool backward")
    # the tie windows, without the added term: only the first maximum (row-major) receives the pooled gradient
    _lib.check(L.ttv_lpips_maxpool_backward(dyd.data_ptr(), None, hd.data_ptr(), n, H, W, C, dx.data_ptr(), dt, _lib.stream_ptr(DEV)),
               "maxpool backward")
    got = dx[:n * H * W * C].view(n, H, W, C).double().cpu()
    assert torch.equal(got[:, 0, 0, :8], dyd[:, 0, 0, :8].double().cpu())
    assert (got[:, 1, 0, :8] == 0).all() and (got[:, 0, 1, :8] == 0).all() and (got[:, 1, 1, :8] == 0).all()
    assert torch.equal(got[:, 2, 3, 8:16], dyd[:, 1, 1, 8:16].double().cpu())
    assert (got[:, 3, 2, 8:16] == 0).all()                                 # the second 0.75 in row-major order
    assert (got[:, 4:6, 4:6, 16:24] == 0).all()                            # all-zero windows: masked


def fixture():
    return np.load(os.path.join(G, "lpips_kat.npz"))


def lpips_module(d, dtype):
    m = LPIPS()
    m.load_state_dict(seeded_lpips_state(int(d["weight_seed"])), strict=True)
    return m.to(DEV).eval()


def test_lpips_fp32_matches_reference_fixture():
    d = fixture()
    m = lpips_module(d, torch.float32)
    for i, (x, y) in enumerate(R.pair_inputs(d)):
        xg = x.to(DEV).requires_grad_(True)
        lp, gr = m(xg, y.to(DEV))
        (gx,) = torch.autograd.grad(lp.sum(), xg, retain_graph=True)
        (gg,) = torch.autograd.grad(gr.sum(), xg)
        e = (R.rel_err(lp, d[f"pair{i}_lpips"]), R.rel_err(gr, d[f"pair{i}_gram"]), R.rel_err(gx[0], d[f"pair{i}_dlpips"]),
             R.rel_err(R.project(gg[0], 100 + i, int(d["proj"])), d[f"pair{i}_dgram_proj"]))
        print(f"pair {i}: lpips {e[0]:.2e} gram {e[1]:.2e} dlpips {e[2]:.2e} dgram {e[3]:.2e}")
        # measured worst: values 2.2e-7, d lpips 4.3e-4, d gram 1.2e-3 (the reference's own fp32 gradient is the yardstick)
        assert e[0] < 1e-5 and e[1] < 1e-5 and e[2] < 1e-3 and e[3] < 1e-2, (i, e)


def test_lpips_bf16_against_float64_per_image_and_block():
    """bf16 trunk vs the float64 restatement on the same (bf16-rounded) crops: per image, and per 16 x 16 block of the gradient."""
    d = fixture()
    sd = seeded_lpips_state(int(d["weight_seed"]))
    m = lpips_module(d, torch.bfloat16)
    g = torch.Generator().manual_seed(8)
    y = torch.rand((7, 3, 128, 128), generator=g) * 2 - 1
    x = (0.7 * y + 0.3 * (torch.rand(y.shape, generator=g) * 2 - 1)).to(torch.bfloat16)
    y = y.to(torch.bfloat16)
    xg = x.to(DEV).requires_grad_(True)
    lp, _ = m(xg, y.to(DEV), compute_gram=False)
    (gx,) = torch.autograd.grad(lp.sum(), xg)
    xr = x.double().requires_grad_(True)
    rl, _ = R.lpips_gram(sd, xr, y.double())
    (rg,) = torch.autograd.grad(rl.sum(), xr)
    img_err = float(((lp.double().cpu() - rl.detach()).abs() / rl.detach().abs()).max())
    gx = gx.double().cpu()
    blk = (gx - rg).abs().unfold(2, 16, 16).unfold(3, 16, 16).amax((-1, -2))
    scale = rg.abs().unfold(2, 16, 16).unfold(3, 16, 16).amax((-1, -2))
    blk_err = float((blk / rg.abs().amax((1, 2, 3), keepdim=True)).max())
    glob = float((gx - rg).norm() / rg.norm())
    print(f"bf16 lpips per-image rel {img_err:.3e}; grad per-block {blk_err:.3e} (of image max), global {glob:.3e}; "
          f"blocks with scale > 0: {int((scale > 0).sum())}")
    # measured on an MI355X: 4.1e-4 per image, 0.141 per block, 5.2e-2 global
    assert img_err < 5e-3 and blk_err < 0.25 and glob < 0.15


def test_lpips_batch_is_independent_and_bit_reproducible():
    d = fixture()
    m32 = lpips_module(d, torch.float32)
    g = torch.Generator().manual_seed(9)
    y = (torch.rand((50, 3, 128, 128), generator=g) * 2 - 1).to(DEV)
    x = (0.7 * y + 0.3 * (torch.rand(y.shape, generator=g) * 2 - 1).to(DEV))
    with torch.no_grad():
        lp32, gr32 = m32(x, y)
        one, _ = m32(x[7:8], y[7:8])
    assert abs(float(one[0]) - float(lp32[7])) <= 1e-6 * abs(float(lp32[7]))
    xb, yb = x.to(torch.bfloat16), y.to(torch.bfloat16)
    outs = []
    for _ in range(2):
        xg = xb.clone().requires_grad_(True)
        lp, gr = m32(xg, yb)
        (gx,) = torch.autograd.grad(lp.sum() + 1e-3 * gr.sum(), xg)
        outs.append((lp, gr, gx))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b), "two identical calls differ"
    rel = float(((outs[0][0] - lp32).abs() / lp32.abs()).max())
    grel = float(((outs[0][1] - gr32).abs() / gr32.abs()).max())
    print(f"n=50 bf16 vs fp32 lpips per-image rel {rel:.3e}, gram {grel:.3e}")
    assert rel < 5e-3 and grel < 2e-2                                     # measured: 4.0e-4, 4.2e-3


def test_generator_step_fp32_matches_reference_fixture():
    d = fixture()
    cfg = SimpleNamespace(
        tokenizer=SimpleNamespace(losses=SimpleNamespace(disc_weight=0.0, perceptual_weight=1.0, gram_weight=float(d["gram_weight"]),
                                                         perceptual_samples_per_step=int(d["samples"]), perceptual_sampling_size=128)),
        discriminator=SimpleNamespace(model=SimpleNamespace(patch_size=[4, 8, 8], model_size="tiny"),
                                      losses=SimpleNamespace(gp_weight=0.1, gp_noise=0.1, centering_weight=0.01)),
        training=SimpleNamespace(main=SimpleNamespace(torch_compile=False, max_steps=10)))
    mod = ReconstructionLoss(cfg, perceptual_weights=seeded_lpips_state(int(d["weight_seed"]))).to(DEV)
    target, recon = R.clip_inputs(d)
    target = [t.to(DEV) for t in target]
    recon = [r.to(DEV).requires_grad_(True) for r in recon]
    random.seed(int(d["rseed"]))
    with R.RandomLog() as log:
        total, ld = mod(target, recon)
    np.testing.assert_array_equal(log.array(), d["random_log"])
    assert list(ld.keys()) == list(d["gen_keys"])
    for k in ld:
        name = k.split("/")[1]
        tol = 1e-3 if name in ("gram_loss", "total_loss") else 1e-4
        assert R.rel_err(ld[k].reshape(1), np.asarray(d["gen_" + name]).reshape(1)) < tol, name
    grads = torch.autograd.grad(total, recon)
    for i, g in enumerate(grads):
        pe = R.rel_err(R.project(g, 200 + i, int(d["proj"])), d[f"clip{i}_dtotal_proj"])
        ne = abs(float(g.norm()) - float(d[f"clip{i}_dtotal_norm"])) / float(d[f"clip{i}_dtotal_norm"])
        print(f"clip {i}: projection {pe:.2e}, norm {ne:.2e}")
        assert pe < 3e-2 and ne < 1e-3, (i, pe, ne)                       # measured worst 6.8e-3 / 2.3e-5 (fp32 Gram: test_lpips_cpu)


def test_unsupported_inputs_are_refused():
    d = fixture()
    m = lpips_module(d, torch.float32)
    x = torch.zeros((1, 3, 32, 32), device=DEV)
    with pytest.raises(TypeError):
        m(x.half(), x.half())
    with pytest.raises(ValueError):
        m(torch.zeros((1, 3, 40, 32), device=DEV), torch.zeros((1, 3, 40, 32), device=DEV))


def test_gan_training_step_with_perceptual_term():
    from titok_video_amd.model.titok import TiTok
    from titok_video_amd.synthetic import seeded_titok_state, seeded_tower_state, synthetic_clips
    from titok_video_amd.train import gan_training_step, make_discriminator_optimizer, make_optimizer
    cfg = SimpleNamespace(
        tokenizer=SimpleNamespace(model=SimpleNamespace(patch_size=[4, 8, 8], fsq_levels=[7, 5, 5, 5, 5], encoder_size="tiny",
                                                        decoder_size="tiny"),
                                  losses=SimpleNamespace(disc_weight=0.4, perceptual_weight=1.0, gram_weight=0.0,
                                                         perceptual_samples_per_step=24, perceptual_sampling_size=128)),
        discriminator=SimpleNamespace(model=SimpleNamespace(patch_size=[4, 8, 8], model_size="tiny"),
                                      losses=SimpleNamespace(gp_weight=0.1, gp_noise=0.1, centering_weight=0.01)),
        training=SimpleNamespace(main=SimpleNamespace(torch_compile=False, max_steps=1000)))
    m = TiTok(cfg)
    m.load_state_dict(seeded_titok_state(0))
    m = m.to(DEV, torch.bfloat16).train()
    lm = ReconstructionLoss(cfg, perceptual_weights=seeded_lpips_state(2))
    lm.disc_model.load_state_dict(seeded_tower_state("encoder", "tiny", (4, 8, 8), 3, 1, seed=77))
    lm = lm.to(DEV, torch.bfloat16).train()
    clips = synthetic_clips([(8, 128, 128), (8, 128, 128)], seed=1, dtype=torch.bfloat16, device=DEV)
    og, od = make_optimizer(m), make_discriminator_optimizer(lm)
    random.seed(0)
    ld, _ = gan_training_step(m, lm, clips, [128, 128], og, od)
    torch.cuda.synchronize()
    assert "gen/perceptual_loss" in ld and np.isfinite(float(ld["gen/perceptual_loss"])) and float(ld["gen/perceptual_loss"]) > 0
    assert all(p.grad is None or torch.isfinite(p.grad.float()).all() for p in m.parameters())
    assert any(p.grad is not None and float(p.grad.float().abs().sum()) > 0 for p in m.parameters())
