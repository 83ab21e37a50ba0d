"""Every training step reads the weights the step before it wrote.  `-m gpu`.

The towers keep derived copies of their weights (`_Tower._packed`: permuted, folded and panel-packed images, compute-dtype copies, the
backward's W^T copies, the decoder's layer-0 constant block) and the L2 quantiser keeps its codebook norms, all under a key made of the
parameters' version counters.  An optimizer that writes the parameters with a kernel has to bump those counters, or step k+1 computes
with what step 0's weights implied.  Two HIP runs with the same stale copies agree with each other, so nothing here compares a run
with a run: after every step the live model is held to a TWIN (tests/twin.py), a newly constructed module that loaded the live weights
and has never seen a step, and once to the float64 oracle, so that a twin wrong in the same way does not pass either.

Shapes: the suite's smallest training batch.  lr = 1e-2: AdamW moves every element by about lr per step, order one against seeded
weights of about width^-0.5 = 1/16, so a stale copy shows far above rounding (profiles/step_reads_new_weights.txt has the figures
with and without the version bump).

Rows: optimizer = HipAdamW's host path, its device path (`hip_capturable=True`), torch's AdamW as `TTV_HIP_ADAMW=0` builds it (fused:
one multi-tensor kernel, which does NOT bump the counters either - `train._make_adamw` gives it a step post-hook that does) and torch's foreach
AdamW, which bumps them itself: the control that passes with and without the bumps of this package and shows the twin harness sound.
Parameters / compute = fp32 / fp32, bf16 / bf16 and fp32 masters with bf16 clips (the reference's bf16-mixed mode: `TiTok`
supports it, the towers compute in the clips' dtype)."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from twin import fresh_twin, twin_optimizer  # noqa: E402

from oracle import titok_oracle as O  # noqa: E402
from titok_video_amd import _lib  # noqa: E402
from titok_video_amd.model.losses import ReconstructionLoss  # noqa: E402
from titok_video_amd.model.titok import TiTok  # noqa: E402
from titok_video_amd.optim import HipAdamW  # noqa: E402
from titok_video_amd.synthetic import seeded_titok_state, seeded_tower_state, synthetic_clips  # noqa: E402
from titok_video_amd.train import (GraphedTrainingStep, gan_training_step, make_discriminator_optimizer, make_optimizer,  # noqa: E402
                                   training_step)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES, COUNTS = [(4, 16, 16), (8, 32, 48), (4, 8, 24)], [2, 5, 3]
LEVELS = [7, 5, 5, 5, 5]
STEPS, LR = 3, 1e-2

# (parameter dtype, clip = compute dtype)
DTYPES = {"fp32": (torch.float32, torch.float32), "bf16": (torch.bfloat16, torch.bfloat16), "fp32w_bf16": (torch.float32, torch.bfloat16)}
OPTIMIZERS = ["hip_host", "hip_device", "torch", "torch_foreach"]

# gradients of twin and live model, relative Frobenius norm per tensor.  fp32: the project's own figure (tests/test_hip_backward.py).
# bf16 compute: the two sides differ only in the order of fp32 atomic sums before one rounding to bf16, which moves an element by at
# most one bf16 step, 2^-8 relative; the margin is a factor of two.
GRAD_BOUND = {torch.float32: 2e-3, torch.bfloat16: 2.0 ** -7}
LOSS_BOUND = 1e-4           # loss scalars, relative (tests/test_hip_vq.py)


def titok_config(kind="fsq"):
    if kind == "fsq":
        m = SimpleNamespace(patch_size=[4, 8, 8], fsq_levels=LEVELS, encoder_size="tiny", decoder_size="tiny")
    else:
        m = SimpleNamespace(patch_size=[4, 8, 8], fsq_levels=None, quantizer="l2", codebook_size=512, token_size=32, encoder_size="tiny",
                            decoder_size="tiny")
    return SimpleNamespace(tokenizer=SimpleNamespace(model=m))


def build_fsq():
    return TiTok(titok_config("fsq"))


def build_l2():
    return TiTok(titok_config("l2"))


def loss_config():
    return SimpleNamespace(
        tokenizer=SimpleNamespace(losses=SimpleNamespace(disc_weight=1.0, perceptual_weight=0.0, gram_weight=0.0, perceptual_samples_per_step=24,
                                                         perceptual_sampling_size=128)),
        discriminator=SimpleNamespace(model=SimpleNamespace(patch_size=[4, 8, 8], model_size="tiny"),
                                      losses=SimpleNamespace(gp_weight=0.1, gp_noise=0.1, centering_weight=0.01)),
        training=SimpleNamespace(main=SimpleNamespace(torch_compile=False, max_steps=1000)))


def build_loss():
    return ReconstructionLoss(loss_config())


def live_fsq(param_dtype):
    m = build_fsq()
    m.load_state_dict(seeded_titok_state(0), strict=True)
    return m.to(DEV, param_dtype).train()


def optimizer_maker(which, monkeypatch, **kw):
    """make(model) -> the optimizer of row `which`.  The switch is read when make_optimizer runs, so it stays set for the test."""
    if which == "torch":
        monkeypatch.setenv("TTV_HIP_ADAMW", "0")
    else:
        monkeypatch.delenv("TTV_HIP_ADAMW", raising=False)

    def make(model):
        if which == "torch_foreach":          # make_optimizer's hyper-parameters on the implementation that bumps the version counters
            return torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=LR, betas=(0.5, 0.96), weight_decay=1e-4, foreach=True)
        opt = make_optimizer(model, lr=LR, hip_capturable=(which == "hip_device"), **kw)
        if which == "torch":
            assert type(opt) is torch.optim.AdamW and opt.defaults["fused"]
        else:
            assert type(opt) is HipAdamW and opt.device_path == (which == "hip_device")
        return opt
    return make


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


class Ledger:
    """Collects every comparison of a test, prints them (worst first) and asserts at the end, so that one run shows how far off
    every compared output is, not only the first."""

    def __init__(self, row):
        self.row, self.exact, self.bounded = row, [], []

    def equal(self, what, got, want):
        got, want = list(got), list(want)
        assert len(got) == len(want), what
        ok = all(g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w) for g, w in zip(got, want))
        worst = max((float((g.double() - w.double()).abs().max()) if g.numel() else 0.0) for g, w in zip(got, want))
        self.exact.append((what, ok, worst))

    def within(self, what, err, bound):
        self.bounded.append((what, float(err), float(bound)))

    def close(self):
        bad_exact = [e for e in self.exact if not e[1]]
        bad_bounded = [b for b in self.bounded if not b[1] <= b[2]]       # (NaN fails)
        ratio = max((b[1] / b[2] for b in self.bounded), default=0.0)
        worst_abs = max((e[2] for e in self.exact), default=0.0)
        print(f"TWIN {self.row}: {len(self.exact)} exact comparisons, {len(bad_exact)} differ (largest |difference| {worst_abs:.3g}); "
              f"{len(self.bounded)} bounded comparisons, {len(bad_bounded)} over, worst error / bound {ratio:.3g}")
        for what, _, worst in sorted(bad_exact, key=lambda e: -e[2])[:6]:
            print(f"    differs: {what} (max |difference| {worst:.3g})")
        for what, err, bound in sorted(bad_bounded, key=lambda b: -b[1] / b[2])[:6]:
            print(f"    over: {what} {err:.3g} > {bound:.3g}")
        assert not bad_exact and not bad_bounded, (self.row, [e[0] for e in bad_exact][:8], [(b[0], b[1]) for b in bad_bounded][:8])


# ------------------------------------------------------------------------------------------------ (a) the forward after each step
def forward_outputs(model, clips):
    """Everything (a) compares: the no-grad forward, encode, decode_indices, and the tape forward in both tape modes."""
    out = {}
    with torch.no_grad():
        recon, info = model(clips, COUNTS)
        out["recon"], out["indices"] = list(recon), [info["indices"]]
        out["encode codes"] = [model.encode(clips, COUNTS)[0]]
        out["decode_indices"] = list(model.decode_indices(info["indices"], SHAPES, COUNTS))
    was = model.encoder.activation_recompute
    for flag in (False, True):
        model.set_activation_recompute(flag)
        with torch.enable_grad():
            z = model.encoder.forward_z(clips, COUNTS)
            taped, _ = model(clips, COUNTS)
        assert z.requires_grad and taped[0].requires_grad          # the tape entries, not the inference ones
        out[f"tape z (recompute={flag})"] = [z.detach()]
        out[f"tape recon (recompute={flag})"] = [r.detach() for r in taped]
    model.set_activation_recompute(was)
    torch.cuda.synchronize()
    return {k: [t.clone() for t in v] for k, v in out.items()}


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("which", OPTIMIZERS)
def test_forward_after_each_step_is_a_fresh_twins(which, dt, monkeypatch):
    param_dtype, clip_dtype = DTYPES[dt]
    make = optimizer_maker(which, monkeypatch)
    clips = synthetic_clips(SHAPES, seed=31, dtype=clip_dtype, device=DEV)
    model = live_fsq(param_dtype)
    opt = make(model)
    # two independent twins agree bit for bit on every compared output (the forwards have no atomics): equality is a fair demand
    first, second = forward_outputs(fresh_twin(model, build_fsq), clips), forward_outputs(fresh_twin(model, build_fsq), clips)
    for k in first:
        assert all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(first[k], second[k])), f"two twins differ on {k}"
    led = Ledger(f"(a) {which} {dt}")
    for step in range(1, STEPS + 1):
        loss, _, _ = training_step(model, clips, COUNTS, opt)
        assert torch.isfinite(loss)
        got, want = forward_outputs(model, clips), forward_outputs(fresh_twin(model, build_fsq), clips)
        for k in want:
            led.equal(f"after step {step}: {k}", got[k], want[k])
    led.close()


# ------------------------------------------------------------------------------------------------ (b) the backward before each step
def loss_and_gradients(model, clips):
    """The loss of tests/test_hip_backward.py (L1 to half the clip + 0.1 mean z^2): (loss, {parameter: gradient}, clip gradients)."""
    leaves = [c.detach().clone().requires_grad_(True) for c in clips]
    for p in model.parameters():
        p.grad = None
    z = model.encoder.forward_z(leaves, COUNTS)
    codes, _ = model.quantize(z)
    recon = model.decode(codes.to(leaves[0].dtype), COUNTS, SHAPES)
    loss = sum((r.float() - 0.5 * c.detach().float()).abs().mean() for r, c in zip(recon, leaves)) + 0.1 * z.pow(2).mean()
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    for p in model.parameters():
        p.grad = None
    return loss.detach(), grads, [c.grad.detach().clone() for c in leaves]


def compare_gradients(led, when, live, twin, bound):
    (loss_a, grads_a, clips_a), (loss_b, grads_b, clips_b) = live, twin
    led.within(f"{when}: loss", abs(float(loss_a) - float(loss_b)) / abs(float(loss_b)), LOSS_BOUND)
    assert grads_a.keys() == grads_b.keys()
    for n in grads_b:
        led.within(f"{when}: d {n}", rel(grads_a[n], grads_b[n]), bound)
    for i, (a, b) in enumerate(zip(clips_a, clips_b)):
        led.within(f"{when}: d clip {i}", rel(a, b), bound)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("which", OPTIMIZERS)
def test_backward_before_each_step_is_a_fresh_twins(which, dt, monkeypatch):
    """The data-gradient GEMMs multiply by W^T copies the pack builds once (`_WeightPack.transposed`): this is the test that sees
    them."""
    param_dtype, clip_dtype = DTYPES[dt]
    make = optimizer_maker(which, monkeypatch)
    clips = synthetic_clips(SHAPES, seed=31, dtype=clip_dtype, device=DEV)
    model = live_fsq(param_dtype)
    opt = make(model)
    led = Ledger(f"(b) {which} {dt}")
    for step in range(STEPS + 1):          # before steps 1, 2, 3 and behind the last one
        compare_gradients(led, f"before step {step + 1}", loss_and_gradients(model, clips),
                          loss_and_gradients(fresh_twin(model, build_fsq), clips), GRAD_BOUND[clip_dtype])
        if step < STEPS:
            training_step(model, clips, COUNTS, opt)
    led.close()


# ------------------------------------------------------------------------------------------------ (c) against the oracle
def test_after_three_steps_the_towers_match_the_oracle_fp32():
    """A twin that was wrong in the same way as the live model would pass (a): after three HipAdamW steps the encoder's z and the
    decoder's output are those of the float64 oracle on `model.state_dict()`.  Tolerances of tests/test_hip_parity.py for the same
    outputs of an fp32 tower: 2e-3 absolute on the encoder's output tokens, 5e-3 * max(1, pixel scale) on the pixels."""
    clips = synthetic_clips(SHAPES, seed=31, dtype=torch.float32, device=DEV)
    model = live_fsq(torch.float32)
    opt = make_optimizer(model, lr=LR)
    assert type(opt) is HipAdamW
    for _ in range(STEPS):
        training_step(model, clips, COUNTS, opt)
    with torch.no_grad():
        z = model.encoder.forward_z(clips, COUNTS)
        codes, _ = model.encode(clips, COUNTS)
        recon = model.decode(codes, COUNTS, SHAPES)
    sd = {k: v.detach().double().cpu() for k, v in model.state_dict().items()}
    with torch.no_grad():
        z_ref = O.encoder_forward([c.double().cpu() for c in clips], COUNTS, sd, "tiny", prefix="encoder.")
        recon_ref = O.decoder_forward(codes.double().cpu(), COUNTS, SHAPES, sd, "tiny", prefix="decoder.")       # on the live codes
    z_err = float((z.double().cpu() - z_ref).abs().max())
    p_err = max(float((r.double().cpu() - rr).abs().max()) for r, rr in zip(recon, recon_ref))
    scale = max(float(rr.abs().max()) for rr in recon_ref)
    print(f"TWIN (c) hip_host fp32: max |z error| {z_err:.3g} (bound 2e-3), max pixel error {p_err:.3g} (bound {5e-3 * max(1.0, scale):.3g})")
    assert z_err < 2e-3 and p_err < 5e-3 * max(1.0, scale)


# ------------------------------------------------------------------------------------------------ (d) the L2 quantiser's norms
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("which", OPTIMIZERS)
def test_l2_codebook_norms_follow_the_trained_codebook(which, dt, monkeypatch):
    """`quantizer: l2` without EMA: the codebook (512 x 32) is a trained parameter and `L2Quantizer._cb` keeps its norms under the
    codebook's version.  The fixed z holds, besides random rows, the midpoints between each entry and its nearest neighbour in
    the start codebook: rows whose argmin a small error in either norm decides."""
    param_dtype, _ = DTYPES[dt]
    make = optimizer_maker(which, monkeypatch)
    clips = synthetic_clips(SHAPES, seed=31, dtype=param_dtype, device=DEV)
    sd0 = seeded_titok_state(3, token_size=32)
    cb0 = torch.randn(512, 32, generator=torch.Generator().manual_seed(9)) * 1.5
    model = build_l2()
    model.load_state_dict({**sd0, "quantize.codebook": cb0}, strict=True)
    model = model.to(DEV, param_dtype).train()
    opt = make(model)
    near = torch.cdist(cb0, cb0).fill_diagonal_(float("inf")).argmin(1)
    z = torch.cat([0.5 * (cb0 + cb0[near]), torch.randn(1024, 32, generator=torch.Generator().manual_seed(10)) * 1.5]).to(DEV, param_dtype)
    led = Ledger(f"(d) {which} {dt}")
    for step in range(1, STEPS + 1):
        training_step(model, clips, COUNTS, opt)
        idx = model.quantize.indices(z)
        led.equal(f"after step {step}: indices of the fixed z", [idx], [fresh_twin(model, build_l2).quantize.indices(z)])
        cb = model.quantize.codebook.detach().contiguous()
        norms = torch.empty(cb.shape[0], dtype=torch.float32, device=DEV)
        _lib.check(_lib.lib().ttv_vq_codebook_norms(cb.data_ptr(), _lib.dtype_code(cb.dtype), cb.shape[1], cb.shape[0], cb.shape[1],
                                                    norms.data_ptr(), _lib.stream_ptr(DEV)), "ttv_vq_codebook_norms")
        led.equal(f"after step {step}: cached norms", [model.quantize._cb(param_dtype)[1]], [norms])
    led.close()


# ------------------------------------------------------------------------------------------------ (e) the GAN step
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_gan_step_discriminator_reads_its_new_weights(dt):
    """Both optimizers HipAdamW.  The discriminator is a tower stepped by its own optimizer, and the generator step differentiates
    through it while it is frozen (tape forward + inputs-only backward: its W^T copies)."""
    param_dtype, _ = DTYPES[dt]
    clips = synthetic_clips(SHAPES, seed=9, dtype=param_dtype, device=DEV)
    fakes = [(0.5 * c + 0.25 * n) for c, n in zip(clips, synthetic_clips(SHAPES, seed=10, dtype=param_dtype, device=DEV))]
    model = live_fsq(param_dtype)
    lm = build_loss()
    lm.disc_model.load_state_dict(seeded_tower_state("encoder", "tiny", (4, 8, 8), 3, 1, seed=77), strict=True)
    lm = lm.to(DEV, param_dtype).train()
    opt_g = make_optimizer(model, lr=LR)
    opt_d = make_discriminator_optimizer(lm, lr=LR, disc_lr_ratio=1.0)
    assert type(opt_g) is HipAdamW and type(opt_d) is HipAdamW

    def generator_gradient(module):
        leaves = [f.detach().clone().requires_grad_(True) for f in fakes]
        loss, _ = module(target=clips, recon=leaves)
        loss.backward()
        torch.cuda.synchronize()
        module._set_disc_trainable(True)          # as the discriminator branch of a step leaves it
        return loss.detach(), [t.grad.detach().clone() for t in leaves]

    led = Ledger(f"(e) hip_host {dt}")
    for step in range(1, STEPS + 1):
        gan_training_step(model, lm, clips, COUNTS, opt_g, opt_d)
        twin = fresh_twin(lm, build_loss)
        with torch.no_grad():
            led.equal(f"after step {step}: disc_wrapper", [lm.disc_wrapper(clips)], [twin.disc_wrapper(clips)])
        (loss_a, grads_a), (loss_b, grads_b) = generator_gradient(lm), generator_gradient(twin)
        led.within(f"after step {step}: generator loss", abs(float(loss_a) - float(loss_b)) / abs(float(loss_b)), LOSS_BOUND)
        for i, (a, b) in enumerate(zip(grads_a, grads_b)):
            led.within(f"after step {step}: d loss / d recon {i}", rel(a, b), GRAD_BOUND[param_dtype])
    led.close()


# ------------------------------------------------------------------------------------------------ (f) the graphed step
@pytest.mark.parametrize("which", ["torch_capturable", "hip_capturable"])
def test_graphed_step_replays_read_the_weights_of_the_replay_before(which):
    """fp32 masters, bf16 clips, as the suite's other graphed tests.  Replay k's loss is the loss of an eager step on a twin of the
    state before that replay (twin optimizer loaded from `optimizer.state_dict()`, so the step counts agree), and behind the last
    replay an eager forward of the live model is a twin's."""
    flags = dict(capturable=True) if which == "torch_capturable" else dict(hip_capturable=True)
    clips = synthetic_clips(SHAPES, seed=31, dtype=torch.bfloat16, device=DEV)
    model = live_fsq(torch.float32)
    opt = make_optimizer(model, lr=LR, **flags)
    assert (type(opt) is HipAdamW) == (which == "hip_capturable")
    step = GraphedTrainingStep(model, opt, clips, COUNTS)
    led = Ledger(f"(f) {which}")
    for k in range(1, STEPS + 1):
        twin = fresh_twin(model, build_fsq)
        twin_opt = twin_optimizer(opt, lambda: make_optimizer(twin, lr=LR, **flags))
        want, _, want_idx = training_step(twin, clips, COUNTS, twin_opt)
        got, _, got_idx = step(clips)
        torch.cuda.synchronize()
        led.within(f"replay {k}: loss", abs(float(got) - float(want)) / abs(float(want)), LOSS_BOUND)
        led.equal(f"replay {k}: indices", [got_idx], [want_idx])
    with torch.no_grad():
        got, want = model(clips, COUNTS), fresh_twin(model, build_fsq)(clips, COUNTS)
    led.equal("behind the last replay: eager recon", got[0], want[0])
    led.equal("behind the last replay: eager indices", [got[1]["indices"]], [want[1]["indices"]])
    led.close()
