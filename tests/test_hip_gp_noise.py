"""`ttv_gp_noise_add` (csrc/ttv_disc.hip) through `ReconstructionLoss.gp_noise_add` on the MI355X: generate mode element by element
against the numpy restatement of tests/gp_noise_ref.py, the same s for both sums, determinism and stream separation, the
statistics of one 2^20-element draw, and given mode against torch._foreach_add bit for bit.  `-m gpu`.

THE BOUND of generate mode, fp32, per element, counted from the device functions the kernel calls (OpenCL's bounds, which the
device library's logf / sqrtf / sincospif are built to): u_a and u_b are exact; logf 3 ulp; times -2 exact; sqrtf halves its
argument's error (1.5) and adds 3: r within 4.5 ulp; sincospif of the exact 2 u_b 4 ulp; the product r * cos half an ulp: the normal
within 9 ulp; s = n * gp_noise half an ulp more: |s - s_64| <= 10 * 2^-23 |s_64| (9.5 rounded up, which also covers the second-order
part).  The sum is rounded once: half an ulp at the value rounded, <= 2^-24 (|ref| + E).  bf16: every element within one bf16 step of
s plus one of the sum, and at most 0.5 % of the elements differ at all from the restatement's own bf16 chain (a cap, not a
measurement; tests/test_gp_noise_cpu.py holds a float32 evaluation of the formulas to a tenth of it)."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gp_noise_ref as GR  # noqa: E402

from titok_video_amd.model.losses import ReconstructionLoss  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"bf16": torch.bfloat16, "f32": torch.float32}
SHAPES = [(3, 4, 8, 8), (3, 1, 5, 7), (3, 4, 16, 24)]          # numel 768, 105 (odd: a tail, and the next clip's offset is rounded up), 4608
GP_NOISE = 0.01


def module(gp_noise=GP_NOISE):
    cfg = SimpleNamespace(
        tokenizer=SimpleNamespace(losses=SimpleNamespace(disc_weight=0.0, perceptual_weight=0.0, gram_weight=0.0, perceptual_samples_per_step=24,
                                                         perceptual_sampling_size=128)),
        discriminator=SimpleNamespace(model=SimpleNamespace(patch_size=[4, 8, 8], model_size="tiny"),
                                      losses=SimpleNamespace(gp_weight=0.1, gp_noise=gp_noise, centering_weight=0.01)),
        training=SimpleNamespace(main=SimpleNamespace(torch_compile=False, max_steps=1000)))
    return ReconstructionLoss(cfg)


def clips(dt, seed):
    """real, fake on the CPU: multiples of 2^-4 in [-1, 1], a quarter of them zero (there out = s itself)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(2):
        out.append([(torch.randint(-16, 17, s, generator=g) * (torch.rand(s, generator=g) > 0.25)).to(DT[dt]) / 16 for s in SHAPES])
    return out


def on_gpu(xs):
    return [x.to(DEV) for x in xs]


def f64(t):
    return t.detach().double().cpu().numpy().reshape(-1)


def bf16_step(x):
    _m, e = np.frexp(np.abs(x))
    return np.ldexp(1.0, np.maximum(e, -125) - 8)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_generate_mode_against_the_restatement(dt):
    real, fake = clips(dt, seed=1)
    torch.manual_seed(1234567890123)
    mod = module()
    mod.__dict__["_gp_draw"] = 5
    out_real, out_fake = mod.gp_noise_add(on_gpu(real), on_gpu(fake))
    assert mod.__dict__["_gp_draw"] == 6
    offs, _ = GR.clip_offsets([r.numel() for r in real])
    differ = count = 0
    for clean, out in ((real, out_real), (fake, out_fake)):
        for c, o, off in zip(clean, out, offs):
            assert o.shape == c.shape and o.dtype == c.dtype and o.data_ptr() % 16 == 0
            s64, ref64, s_chain, out_chain = GR.noisy(f64(c), off, 1234567890123, 5, GP_NOISE, dt)
            got = f64(o)
            if dt == "f32":
                E = 10 * 2.0 ** -23 * np.abs(s64)
                tol = E + 2.0 ** -24 * (np.abs(ref64) + E)
            else:
                tol = bf16_step(s64) + bf16_step(ref64)
                differ += int((got != out_chain).sum())
                count += got.size
            worst = float((np.abs(got - ref64) / tol).max())
            print(f"{dt} clip {tuple(c.shape)}: max |error| / bound {worst:.3f}")
            assert worst <= 1.0
    if dt == "bf16":
        print(f"bf16: {differ} of {count} elements differ from the restatement's bf16 chain")
        assert differ <= 0.005 * count
    # the same s in both sums: where real is 0 the output IS s, and the other output must be the one rounding of fake + s (and the
    # other way round); where both are 0 - both sums exact - the two outputs are identical
    for r, f, a, b in zip(real, fake, out_real, out_fake):
        a, b = a.cpu(), b.cpu()
        zr, zf = r == 0, f == 0
        assert int(zr.sum()) > 10 and int(zf.sum()) > 10 and int((zr & zf).sum()) > 2
        assert torch.equal(b[zr], (f[zr] + a[zr]))
        assert torch.equal(a[zf], (r[zf] + b[zf]))
        assert torch.equal((a - r)[zr & zf], (b - f)[zr & zf])


def test_determinism_and_stream_separation():
    real, fake = [on_gpu(x) for x in clips("bf16", seed=2)]
    runs = []
    for seed in (77, 77, 78):
        torch.manual_seed(seed)
        mod = module()                                             # a fresh module starts at draw 0
        first = [t.clone() for t in mod.gp_noise_add(real, fake)[0]]
        second = [t.clone() for t in mod.gp_noise_add(real, fake)[0]]
        runs.append((first, second))
    same = lambda xs, ys: all(torch.equal(x, y) for x, y in zip(xs, ys))
    assert same(runs[0][0], runs[1][0]) and same(runs[0][1], runs[1][1])          # manual_seed + a fresh module reproduce two steps
    assert not same(runs[0][0], runs[0][1])                                        # the next draw differs
    assert not same(runs[0][0], runs[2][0])                                        # another seed differs
    torch.manual_seed(77)
    mod = module()
    mod.__dict__["_gp_draw"] = 1
    assert same(mod.gp_noise_add(real, fake)[0], runs[0][1])                       # same seed and same draw: the same bits


def test_statistics_of_one_draw():
    """One call generates N = 2^20 elements (gp_noise 1 and zeros: the output is the normal itself, fp32).  Fixed seed, so the outcome
    is deterministic: mean within 5 / sqrt(N), variance within 1 %, Kolmogorov distance to the normal below 3 / sqrt(N), lanes 0 / 1
    and 2 / 3 (the cos and sin of one Box-Muller pair) correlated below 5 / sqrt(N)."""
    N = 1 << 20
    torch.manual_seed(2024)
    mod = module(gp_noise=1.0)
    zeros = [torch.zeros(N, dtype=torch.float32, device=DEV)]
    x = mod.gp_noise_add(zeros, zeros)[0][0].double().cpu()
    assert bool(torch.isfinite(x).all())
    assert abs(float(x.mean())) < 5 / N ** 0.5
    assert abs(float(x.var()) - 1.0) < 0.01
    xs = torch.sort(x).values
    cdf = 0.5 * (1.0 + torch.erf(xs / 2.0 ** 0.5))
    i = torch.arange(1, N + 1, dtype=torch.float64)
    ks = float(torch.maximum((i / N - cdf).abs(), (cdf - (i - 1) / N).abs()).max())
    lanes = x.view(-1, 4)
    c01 = float(torch.corrcoef(torch.stack([lanes[:, 0], lanes[:, 1]]))[0, 1])
    c23 = float(torch.corrcoef(torch.stack([lanes[:, 2], lanes[:, 3]]))[0, 1])
    print(f"mean {float(x.mean()):.2e} var {float(x.var()):.5f} KS {ks:.2e} (3/sqrt(N) = {3 / N ** 0.5:.2e}) corr {c01:.2e} {c23:.2e}")
    assert ks < 3 / N ** 0.5
    assert abs(c01) < 5 / N ** 0.5 and abs(c23) < 5 / N ** 0.5


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_given_mode_equals_foreach_add_bit_for_bit(dt):
    g = torch.Generator().manual_seed(3)
    shapes = SHAPES + [(3, 2, 40, 40)]                              # 9600 elements: more than one chunk
    real = [torch.randn(s, generator=g).to(DT[dt]).to(DEV) for s in shapes]
    fake = [torch.randn(s, generator=g).to(DT[dt]).to(DEV) for s in shapes]
    noise = [(0.3 * torch.randn(s, generator=g)).to(DT[dt]).to(DEV) for s in shapes]
    # a clip that is not 16-byte aligned takes the element-by-element path
    base = torch.randn(105 + 1, generator=g).to(DT[dt]).to(DEV)
    real[1] = base[1:].view(SHAPES[1])
    assert real[1].data_ptr() % 16 != 0 and real[1].is_contiguous()
    mod = module()
    out_real, out_fake = mod.gp_noise_add(real, fake, noise)
    assert mod.__dict__.get("_gp_draw", 0) == 0                     # a given noise consumes no draw
    for got, want in zip(out_real + out_fake, list(torch._foreach_add(real, noise)) + list(torch._foreach_add(fake, noise))):
        assert got.dtype == want.dtype and torch.equal(got, want)
