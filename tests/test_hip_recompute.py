"""Activation recompute of the training towers (TTV_TAPE_RECOMPUTE) against the stored tape (`-m gpu`).

The recompute tape keeps the layer boundaries and two layer slots; the backward rebuilds a layer's tape from its boundary with the very
kernels, launch arguments and inputs of the forward (csrc/ttv_train.hip, layer_forward_train).  So it must change no bit of anything
the stored path itself reproduces bit for bit.  The rule every test here applies:

  * the stored path runs TWICE; an output is *stable* if the two runs agree bit for bit.  In bf16 the stable set must contain every
    layer's to_qkv, out_proj, w12 and w3 gradient of both towers (tests/test_hip_backward_bf16.py documents them as bit-reproducible;
    if they are not, that is a finding about the stored path), and in both dtypes the forward's outputs z and the reconstructions;
  * under recompute every stable output is bit-identical to the stored run - except the outputs the backward sums with fp32 atomicAdd
    across blocks (csrc/ttv_bwd.hip: norm gains, biases, mask tokens, and the two token-width projections ttvk_outer_small reduces,
    encoder.proj_out.weight and decoder.proj_in.weight).  Two stored runs agree on most of those by chance (first MI355X run, tiny FULL
    bf16: 37 of 42 such outputs agreed, the 5 others differed between the two STORED runs; the recompute run then differed in
    decoder.proj_in.weight, which the two stored runs happened to agree on), so agreement of two runs does not show that a third
    would agree: two runs cannot tell them from reproducible outputs, the kernels' text can;
  * the atomically summed outputs, and every output that is not stable (the fp32 weight-gradient and attention-backward kernels use
    atomics too), are held to the bounds the stored path is held to: bf16, check_against_replay of tests/test_hip_backward_bf16.py (the
    float64 replay of the bf16 tape); fp32, 2e-3 relative per tensor against the float64 model (the bound of tests/test_hip_backward.py
    for the fp32 towers).

Model, inputs and linear losses are those of hip_grads in tests/test_hip_backward_bf16.py; the fp32 runs take the same bf16 numbers in
fp32.  Cases: the small size at SMALL (8 layers: both slots are reused three times; one sequence over 128 rows, one of 7), the tiny size
at FULL (K = 128 / 200 / 5) and at FIVE (half-item attention tables), the base size at SMALL (12 layers: both slots reused five times; the
bf16 bounds are the gap-relative ones of tests/gap_bounds.py).  The float64 references are the lru-cached ones of that module,
shared with its own tests when the suite runs in one process.
"""
import ctypes as C
import functools

import pytest
import torch

from tests.test_hip_backward_bf16 import CASES, LAYER_LINEARS, _inputs, check_against_replay, replay
from tests.test_hip_backward_shapes import _model, _rel, report
from titok_video_amd import _lib
from titok_video_amd.synthetic import synthetic_clips

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"bf16": torch.bfloat16, "f32": torch.float32}
F32_TOL = 2e-3          # tests/test_hip_backward.py: every fp32 gradient within 2e-3 relative (Frobenius) of the float64 model's


class TowerStep:
    """hip_grads of tests/test_hip_backward_bf16.py as an object: the model and its inputs stay on the device, run() repeats the step
    (encoder forward + backward under sum(wz * z), decoder forward + backward under sum(W * recon)) and outputs() brings everything
    the step computed to the host.  `flip`: the towers' activation_recompute is inverted between each forward and its backward."""

    def __init__(self, case, dtype, recompute, frozen_encoder=False):
        size, shapes, counts, wz, clips, codes, w = _inputs(case)
        self.case, self.shapes, self.counts = case, [tuple(s) for s in shapes], list(counts)
        model = _model(size, torch.bfloat16)              # the bf16 model's parameters ...
        self.model = (model.float() if dtype is torch.float32 else model).set_activation_recompute(recompute)      # ... also for fp32
        if frozen_encoder:
            for p in self.model.encoder.parameters():
                p.requires_grad_(False)
        self.clips = [c.to(DEV, dtype).requires_grad_(True) for c in clips]
        self.codes = codes.to(DEV, dtype).requires_grad_(True)
        self.wz, self.w = wz.to(DEV), [wc.to(DEV).float() for wc in w]
        self.z = self.rec = None

    def _flip(self):
        self.model.set_activation_recompute(not self.model.encoder.activation_recompute)

    def run(self, flip=False, decoder=True):
        for t in list(self.model.parameters()) + self.clips + [self.codes]:
            t.grad = None
        self.z = self.rec = None
        self.z = self.model.encoder.forward_z(self.clips, self.counts)
        loss = (self.z * self.wz).sum()
        if flip:
            self._flip()
        loss.backward()
        if flip:
            self._flip()
        if not decoder:
            return
        self.rec = self.model.decode(self.codes, self.counts, self.shapes)
        loss = sum((r.float() * wc).sum() for r, wc in zip(self.rec, self.w))
        if flip:
            self._flip()
        loss.backward()
        if flip:
            self._flip()

    def outputs(self):
        torch.cuda.synchronize()
        out = {"params": {n: p.grad.float().cpu() for n, p in self.model.named_parameters() if p.grad is not None},
               "clips": [c.grad.float().cpu() for c in self.clips], "z": self.z.detach().float().cpu()}
        if self.rec is not None:
            out["codes"] = self.codes.grad.float().cpu()
            out["recon"] = [r.detach().float().cpu() for r in self.rec]
        return out


def flat(out):
    """One name per tensor of a step's outputs."""
    d = {"param " + n: g for n, g in out["params"].items()}
    d.update({f"clip {i}": c for i, c in enumerate(out["clips"])})
    d["z"] = out["z"]
    if "codes" in out:
        d["codes"] = out["codes"]
        d.update({f"recon {i}": r for i, r in enumerate(out["recon"])})
    return d


@functools.lru_cache(maxsize=None)
def stored_twice_and_recompute(case, dt):
    """The step on the stored tape, twice, and on the recompute tape: computed once per (case, dtype) and read only."""
    runs = []
    for recompute in (False, False, True):
        step = TowerStep(case, DT[dt], recompute)
        step.run()
        runs.append(step.outputs())
    return tuple(runs)


def check_fp32(got, case, names, what):
    """The tensors `names` of an fp32 step within F32_TOL of the float64 model's (no rounding anywhere)."""
    ref, ref_clips, ref_codes = replay(case, False)
    worst = (0.0, "")
    for n in names:
        kind, _, rest = n.partition(" ")
        r = ref[rest] if kind == "param" else ref_clips[int(rest)] if kind == "clip" else ref_codes
        worst = max(worst, (_rel(flat(got)[n], r), n))
    report(f"{what}: worst of {len(names)} tensors against the float64 model {worst[0]:.2e} ({worst[1]})")
    assert worst[0] < F32_TOL, (what, worst)


def summed_with_atomics(name, t):
    """Gains, biases, mask tokens (vectors and [1, 1]) and the token-width projections: one fp32 atomicAdd per block and element."""
    return name.startswith("param ") and (t.dim() < 2 or min(t.shape) == 1 or name.endswith(("encoder.proj_out.weight", "decoder.proj_in.weight")))


def check_rule(case, dt, a, b, got, what):
    """The rule of the module docstring: a, b two stored runs, got the run under test."""
    fa, fb, fg = flat(a), flat(b), flat(got)
    assert set(fa) == set(fb) == set(fg), what
    stable = [n for n in fa if torch.equal(fa[n], fb[n])]
    unstable = sorted(set(fa) - set(stable))
    report(f"{what}: {len(stable)} of {len(fa)} outputs stable between two stored runs; not stable: {unstable[:6]}"
           + (f" and {len(unstable) - 6} more" if len(unstable) > 6 else ""))
    forward = [n for n in fa if n == "z" or n.startswith("recon")]
    assert not [n for n in forward if n not in stable], "the stored forward does not reproduce itself"
    if dt == "bf16":
        linears = [n for n in fa if n.startswith("param") and any(k in n for k in LAYER_LINEARS) and n.endswith("weight")]
        assert linears
        missing = [n for n in linears if n not in stable]
        assert not missing, f"stored bf16 path: layer weight gradients not bit-reproducible: {missing}"
    differ = [n for n in stable if not torch.equal(fg[n], fa[n])]
    by_chance = [n for n in differ if summed_with_atomics(n, fa[n])]
    if by_chance:
        report(f"{what}: atomically summed outputs on which the two stored runs agreed and this run does not: {by_chance}")
    differ = [n for n in differ if n not in by_chance]
    assert not differ, f"{what}: differs from the stored path where that path is bit-reproducible: {differ}"
    bounded = unstable + by_chance
    assert not [n for n in bounded if n in forward]
    if dt == "bf16":
        if bounded:
            check_against_replay(got, case, what)          # every bound of that module, the unstable outputs among them
    elif bounded:
        check_fp32(got, case, bounded, what)


# ---------------------------------------------------------------------------------------------- 1. gradients against the stored path
@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("case", ["tiny-full", "small", "tiny-five", "base"])      # base: 12 layers, both slots reused five times
def test_recompute_gradients_against_the_stored_tape(case, dt):
    a, b, got = stored_twice_and_recompute(case, dt)
    n_layers = {"tiny": 4, "small": 8, "base": 12}[CASES[case][0]]
    linears = [n for n in a["params"] if any(k in n for k in LAYER_LINEARS) and n.endswith("weight")]
    assert len(linears) == 2 * 4 * n_layers
    check_rule(case, dt, a, b, got, f"recompute {dt} {case}")


# ---------------------------------------------------------------------------------------------- 2. frozen discriminator route
@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("case", ["tiny-full", "small"])
def test_recompute_frozen_encoder_gives_the_stored_clip_gradients(case, dt):
    """grads == NULL (every parameter frozen, clips require grad: the generator step through the discriminator): ttv_encoder_backward_ex
    skips every weight gradient and reduction and still has to rebuild every layer's tape for the dX chain."""
    runs = []
    for recompute in (False, False, True):
        step = TowerStep(case, DT[dt], recompute, frozen_encoder=True)
        step.run(decoder=False)
        out = step.outputs()
        assert not [n for n in out["params"] if n.startswith("encoder.")], "a frozen encoder received parameter gradients"
        runs.append(out)
    a, b, got = runs
    stable = all(torch.equal(x, y) for x, y in zip(a["clips"], b["clips"]))
    report(f"frozen encoder {dt} {case}: clip gradients of two stored runs bit-equal: {stable}")
    assert torch.equal(a["z"], b["z"]) and torch.equal(got["z"], a["z"])
    if stable:
        assert all(torch.equal(x, y) for x, y in zip(got["clips"], a["clips"]))
    elif dt == "f32":
        check_fp32(got, case, [f"clip {i}" for i in range(len(got["clips"]))], f"frozen encoder f32 {case}")
    else:
        from oracle import titok_oracle as O
        from tests.blockwise import check_blockwise
        from tests.test_hip_backward_bf16 import CLIP_TOL, PATCH
        gp = torch.cat([O.patchify(c, PATCH) for c in got["clips"]])
        rp = torch.cat([O.patchify(c, PATCH) for c in replay(case, True)[1]])
        cu = [0]
        for s in CASES[case][1][0]:
            cu.append(cu[-1] + (s[0] // PATCH[0]) * (s[1] // PATCH[1]) * (s[2] // PATCH[2]))
        check_blockwise(gp, rp, cu, 1, CLIP_TOL[0], CLIP_TOL[1], f"frozen encoder bf16 {case} clip gradients")


# ---------------------------------------------------------------------------------------------- 3. a training step end to end
def _l1_in_fixed_order(recon, target):
    """train.l1_reconstruction_loss's definition (mean over clips of the clip's mean |recon - target|) by torch's reductions."""
    return torch.stack([(r.float() - t.float()).abs().mean() for r, t in zip(recon, target)]).mean()


def _train_three_steps(recompute):
    from titok_video_amd.optim import HipAdamW
    from titok_video_amd.train import make_optimizer, training_step
    shapes, counts = CASES["tiny-five"][1]
    torch.manual_seed(0)
    model = _model("tiny", torch.bfloat16).set_activation_recompute(recompute)
    opt = make_optimizer(model)
    assert isinstance(opt, HipAdamW)
    clips = synthetic_clips(shapes, seed=1, dtype=torch.bfloat16, device=DEV)
    seen = []
    hook = model.register_forward_hook(lambda mod, args, out: seen.append(_l1_in_fixed_order([r.detach() for r in out[0]], clips)))
    returned = []
    for _ in range(3):
        loss, _gnorm, _idx = training_step(model, clips, list(counts), opt)
        returned.append(float(loss))
    hook.remove()
    torch.cuda.synchronize()
    return [x.cpu() for x in seen], returned, {n: p.detach().float().cpu() for n, p in model.named_parameters()}


def test_recompute_training_steps_follow_the_stored_ones():
    """train.training_step (forward, L1, backward, clip, HipAdamW) three times on FIVE, recompute on against off, same seed.  Per step
    loss and per parameter after step 3: bit-equal where two stored runs are; otherwise no further from the first stored run than twice
    the distance between the two stored runs (max abs over the tensor; the factor because a third sample of a run-to-run-noisy quantity
    can fall outside two).

    The loss of a step is taken from the reconstruction that step produced (a forward hook on the model), summed by torch in a fixed
    order.  The scalar training_step returns is the same quantity summed by ttv_l1_loss with one fp32 atomicAdd per block: its last
    bits differ between runs whose reconstructions are bit-identical (first MI355X run, step 1, which no update precedes: 1.5869858,
    1.5869864 stored twice, 1.5869875 recompute - 2.8 times the distance of the two stored values, by the loss kernel's summation order
    alone).  Those scalars are printed, not judged."""
    (la, ra, pa), (lb, rb, pb), (lc, rc, pc) = _train_three_steps(False), _train_three_steps(False), _train_three_steps(True)
    assert len(la) == len(lb) == len(lc) == 3
    items = [(f"loss of step {i + 1}", la[i], lb[i], lc[i]) for i in range(3)] + [(n, pa[n], pb[n], pc[n]) for n in pa]
    bad, n_equal, worst = [], 0, (0.0, 0.0, "")
    for name, a, b, c in items:
        if torch.equal(a, b):
            n_equal += 1
            if not torch.equal(c, a):
                bad.append(f"{name}: stored runs bit-equal, recompute differs by {float((c - a).abs().max()):.3e}")
            continue
        spread, dist = float((a.double() - b.double()).abs().max()), float((c.double() - a.double()).abs().max())
        worst = max(worst, (dist / spread, spread, name))
        if not dist <= 2 * spread:
            bad.append(f"{name}: {dist:.3e} from the stored run, spread of two stored runs {spread:.3e}")
    report(f"training steps: {n_equal} of {len(items)} quantities bit-equal between two stored runs; losses {[float(x) for x in la]}; "
           f"worst distance / spread {worst[0]:.2f} (spread {worst[1]:.3e}, {worst[2]}); scalars returned by training_step: stored {ra}, "
           f"stored again {rb}, recompute {rc}")
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------- 4. HIP graph capture
class ModelStep:
    """Forward + backward of the tiny tokenizer as train.training_step runs them (TiTok.forward, L1 against the clips, backward),
    without the optimizer: the sequence train.GraphedTrainingStep records."""

    def __init__(self, recompute):
        shapes, counts = CASES["tiny-five"][1]
        self.counts = list(counts)
        self.model = _model("tiny", torch.bfloat16).set_activation_recompute(recompute)
        self.clips = synthetic_clips(shapes, seed=1, dtype=torch.bfloat16, device=DEV)
        self.recon = None

    def run(self):
        from titok_video_amd.train import l1_reconstruction_loss
        self.model.zero_grad(set_to_none=True)
        self.recon = None          # with the last output goes the last autograd graph, and with it the parameters' gradient accumulators
        self.recon, _ = self.model(self.clips, self.counts)
        l1_reconstruction_loss(self.recon, self.clips).backward()

    def outputs(self):
        torch.cuda.synchronize()
        out = {"param " + n: p.grad.float().cpu() for n, p in self.model.named_parameters()}
        out.update({f"recon {i}": r.detach().float().cpu() for i, r in enumerate(self.recon)})
        return out


def test_recompute_step_is_capturable_into_a_hip_graph():
    """After two eager steps, forward + backward of the tiny model on FIVE with recompute is captured once and replayed twice: the library
    allocates nothing, waits for nothing and reads nothing back.  The eager step runs twice (the stable set); each replay then has to
    give bit for bit every output that is stable and not summed with atomics - every weight matrix's gradient and the reconstructions,
    asserted to be among them.  The atomically summed ones (no float64 replay exists for this loss): the gradients are stored in bf16,
    and another order of an fp32 sum moves an element to a neighbouring bf16 number at most, unless the sum cancels to less than 2^-15
    of its terms - so a tensor is held to a relative Frobenius distance of one bf16 ulp, 2^-7, from the eager one."""
    # Every run on the capture stream, the eager ones too: autograd runs a leaf's gradient accumulator on the stream that was current
    # when the accumulator was made and keeps it while any graph that reaches it lives.  An eager step on another stream before the
    # capture would have the captured backward hop to that stream through events torch destroys before the capture ends.
    dev = torch.device(DEV)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        step = ModelStep(True)
        step.run()
        a = step.outputs()
        step.run()
        b = step.outputs()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step.run()
    exact = [n for n in a if torch.equal(a[n], b[n]) and not summed_with_atomics(n, a[n])]
    matrices = [n for n in a if n.startswith("param ") and not summed_with_atomics(n, a[n])]
    assert len(matrices) == 2 * (4 * 4 + 1) and not [n for n in matrices if n not in exact], "eager weight gradients not bit-reproducible"
    assert not [n for n in a if n.startswith("recon") and n not in exact]
    for k in (1, 2):
        for p in step.model.parameters():
            p.grad.zero_()                            # the replay has to write every one of them again
        graph.replay()
        got = step.outputs()
        assert set(got) == set(a)
        differ = [n for n in exact if not torch.equal(got[n], a[n])]
        assert not differ, f"graph replay {k}: differs from the eager step: {differ}"
        worst = max((_rel(got[n], a[n]), n) for n in a if n not in exact)
        report(f"graph replay {k} of the recompute step: {len(exact)} of {len(a)} outputs bit-equal to the eager step; worst of the "
               f"atomically summed ones {worst[0]:.2e} ({worst[1]})")
        assert worst[0] < 2.0 ** -7, worst


# ---------------------------------------------------------------------------------------------- 5. memory
def _tape_bytes(tower, shapes, counts, dtype, mode):
    plan = tower._plan([tuple(s) for s in shapes], list(counts), torch.device(DEV))
    dims = tower._dims(_lib.dtype_code(dtype))
    batch = plan.batch_for(tower.heads[0], tower.heads[1])
    n = int(_lib.lib().ttv_tower_tape_bytes_ex(C.byref(dims), C.byref(batch), mode))
    assert n > 0
    return n


def test_recompute_lowers_the_peak_by_the_tape_difference():
    """Forward + backward of the whole tokenizer (both tapes alive from the decoder's forward to its backward) on FIVE, tiny, bf16: the
    peak of torch's allocator drops by the two towers' tape difference, less 4 MiB per tower for the allocator's rounding."""
    from titok_video_amd.train import l1_reconstruction_loss
    shapes, counts = CASES["tiny-five"][1]
    model = _model("tiny", torch.bfloat16)
    clips = synthetic_clips(shapes, seed=1, dtype=torch.bfloat16, device=DEV)
    peaks = {}
    for recompute in (False, True, False, True):
        model.set_activation_recompute(recompute)
        for measured in (False, True):                # the first pass builds plans and weight packs
            model.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            recon, _ = model(clips, list(counts))
            l1_reconstruction_loss(recon, clips).backward()
            torch.cuda.synchronize()
            del recon
            if measured:
                peaks.setdefault(recompute, []).append(torch.cuda.max_memory_allocated() - base)
    saved = sum(_tape_bytes(t, shapes, counts, torch.bfloat16, _lib.TTV_TAPE_STORED)
                - _tape_bytes(t, shapes, counts, torch.bfloat16, _lib.TTV_TAPE_RECOMPUTE) for t in (model.encoder, model.decoder))
    report(f"peak above the resident bytes, tiny FIVE bf16: stored {peaks[False]}, recompute {peaks[True]}; tape difference {saved}")
    assert saved > 0
    assert max(peaks[True]) <= min(peaks[False]) - (saved - 2 * (4 << 20))


# ---------------------------------------------------------------------------------------------- 6. mode consistency
@pytest.mark.parametrize("forward_mode", [True, False], ids=["recompute-forward", "stored-forward"])
def test_backward_runs_in_the_mode_of_its_forward(forward_mode):
    """activation_recompute inverted between each forward and its backward: the backward still reads the tape its forward wrote."""
    a, b, _ = stored_twice_and_recompute("tiny-five", "bf16")
    step = TowerStep("tiny-five", torch.bfloat16, forward_mode)
    step.run(flip=True)
    assert step.model.encoder.activation_recompute is forward_mode
    check_rule("tiny-five", "bf16", a, b, step.outputs(), f"flag inverted before the backward, forward recompute={forward_mode}")
