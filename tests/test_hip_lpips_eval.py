"""GPU tests of the evaluation LPIPS (csrc/ttv_lpips.hip evaluation path, LPIPS.frame_distances, EvalMetrics 'lpips'): per-frame
values of whole frames whose sizes are not multiples of 16 against the float64 restatement (tests/lpips_eval_ref.py) and the
reference's own per-frame values (tests/golden/lpips_eval_kat.npz), in both dtypes; no frame reads a neighbouring image; the
reconstruction's clamp; passes and grouping; the metric's surface.  Seeded weights, `-m gpu`."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_eval_ref as E  # noqa: E402

from titok_video_amd import _lib  # noqa: E402
from titok_video_amd.model.metrics.eval_metrics import EvalMetrics  # noqa: E402
from titok_video_amd.model.metrics.lpips_gram import LPIPS  # noqa: E402
from titok_video_amd.synthetic import seeded_lpips_state  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IDS = ["x".join(map(str, s)) for s in E.SHAPES]
DTYPES = [torch.float32, torch.bfloat16]
_CACHE = {}


def state():
    if "sd" not in _CACHE:
        _CACHE["sd"] = seeded_lpips_state(E.WEIGHT_SEED)
    return _CACHE["sd"]


def pair(i):
    """The fixture's clip pair i (bf16-representable fp32, CPU), drawn once."""
    if ("pair", i) not in _CACHE:
        _CACHE[("pair", i)] = E.clip_pair(E.SHAPES[i], E.CLIP_SEED + i)
    return _CACHE[("pair", i)]


def ref64(i):
    """float64 per-frame values of clip pair i, computed once and left alone; the reference for both dtypes."""
    if ("ref", i) not in _CACHE:
        _CACHE[("ref", i)] = E.frame_values(state(), *pair(i))
    return _CACHE[("ref", i)]


@pytest.fixture(scope="module")
def model():
    m = LPIPS()
    m.load_state_dict(state(), strict=True)
    return m.to(DEV).eval()


def dev_pair(i, dtype):
    r, t = pair(i)
    return r.to(DEV, dtype), t.to(DEV, dtype)


def rel(got, ref):
    """Per-frame |got - ref| / |ref|, the worst frame."""
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    return float(((got - ref).abs() / ref.abs()).max())


def seq_sum(v):
    """The double sum of fp32 values added one by one in order, as the accumulator adds them."""
    s = 0.0
    for x in v.cpu().tolist():
        s += x
    return s


def raw_call(m, recons, targets, clamp=1, frames_per_pass=None):
    """ttv_lpips_eval_accumulate on clips of one frame size, with NaN-filled slack behind the per-frame values and behind the
    accumulator (checked to stay NaN).  Returns (values [frames] fp32, acc [2] double)."""
    L, dtype = _lib.lib(), recons[0].dtype
    dt = _lib.dtype_code(dtype)
    H, W = recons[0].shape[2:]
    total = sum(r.shape[1] for r in recons)
    nbytes = L.ttv_lpips_eval_workspace_bytes(frames_per_pass or total, H, W, dt)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    out = torch.full((total + 64,), float("nan"), device=DEV)
    acc = torch.full((2 + 6,), float("nan"), dtype=torch.float64, device=DEV)
    acc[:2] = 0
    frames = (_lib.C.c_int32 * len(recons))(*[int(r.shape[1]) for r in recons])
    pack = m._pack(dtype, recons[0].device)
    _lib.check(L.ttv_lpips_eval_accumulate(_lib.C.byref(pack.w), _lib.ptr_array(recons), _lib.ptr_array(targets), frames, len(recons), H, W,
                                           dt, clamp, out.data_ptr(), acc.data_ptr(), ws.data_ptr(), nbytes, _lib.stream_ptr(DEV)),
               "ttv_lpips_eval_accumulate")
    torch.cuda.synchronize()
    assert torch.isnan(out[total:]).all() and torch.isnan(acc[2:]).all(), "stray write past an output"
    return out[:total].clone(), acc[:2].clone()


@pytest.mark.parametrize("i", range(len(E.SHAPES)), ids=IDS)
def test_fp32_per_frame_against_float64_and_the_reference(model, i):
    """Exact-fp32 kernels: < 1e-5 relative per frame against float64 at every shape (the project's bound for this network), and
    against the reference's own fp32 per-frame values.  Measured on an MI355X: worst 1.7e-7 / 2.1e-7 over the seven shapes."""
    r, t = dev_pair(i, torch.float32)
    got, acc = raw_call(model, [r], [t])
    d = np.load(os.path.join(G, "lpips_eval_kat.npz"))
    e64, eref = rel(got, ref64(i)), rel(got, torch.from_numpy(d[f"clip{i}_lpips"]))
    print(f"{E.SHAPES[i]} fp32: rel to float64 {e64:.2e}, to the reference's fp32 {eref:.2e}")
    assert e64 < 1e-5 and eref < 1e-5
    assert torch.equal(model.frame_distances([r], [t]), got)
    assert float(acc[1]) == r.shape[1] and float(acc[0]) == seq_sum(got)     # added one by one, in frame order


@pytest.mark.parametrize("i", range(len(E.SHAPES)), ids=IDS)
def test_bf16_per_frame_against_float64(model, i):
    """bf16 MFMA path against float64 on the same (bf16-representable) clips.  Both edges >= 64: the project's per-image bound
    5e-3.  Smaller frames, where one stage-4 pixel carries a whole tap: twice the error of the CPU restatement that rounds every
    activation to bf16 (tests/lpips_eval_ref.py frame_values_bf16) at the same inputs, computed here; the factor 2 is for the
    kernel's fp32 summation order, which moves some roundings to the neighbouring bf16 value.  The bound never comes from the
    kernel's output.  Measured on an MI355X, kernel / CPU restatement (worst frame of the clip):
      (5,16,16) 9.83e-4 / 9.79e-4   (2,17,23) 2.76e-4 / 1.45e-4   (3,24,40) 1.31e-3 / 1.25e-3   (2,40,24) 2.19e-4 / 2.81e-4
      (1,16,520) 3.99e-4 / 3.64e-4;   (2,136,168) 4.73e-4 and (16,128,128) 5.73e-4 against the 5e-3."""
    r, t = dev_pair(i, torch.bfloat16)
    got, _ = raw_call(model, [r], [t])
    err = rel(got, ref64(i))
    T, H, W = E.SHAPES[i]
    if min(H, W) >= 64:
        bound, what = 5e-3, "per-image bound"
    else:
        cpu = rel(E.frame_values_bf16(state(), *pair(i)), ref64(i))
        bound, what = 2 * cpu, f"2 x CPU bf16 restatement ({cpu:.2e})"
    print(f"{E.SHAPES[i]} bf16: rel to float64 {err:.2e}; bound {bound:.2e} = {what}")
    assert err < bound
    assert torch.equal(model.frame_distances([r], [t]), got)


@pytest.mark.parametrize("i", [0, 1], ids=IDS[:2])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_a_frame_equal_to_its_target_is_exactly_zero(model, i, dtype):
    """Leak detector: frame t has recon == target (inside [-1, 1]) while its neighbours differ strongly; any tap that reads a
    neighbouring image of the stack makes frame t non-zero."""
    r0, t = dev_pair(i, dtype)
    assert float(t.abs().max()) <= 1.0
    r0 = (r0 + torch.where(t > 0, -1.0, 1.0).to(dtype))        # far from the target everywhere
    for k in range(r0.shape[1]):
        r = r0.clone()
        r[:, k] = t[:, k]
        got, _ = raw_call(model, [r], [t])
        assert float(got[k]) == 0.0, (k, got)
        assert (got[[j for j in range(r.shape[1]) if j != k]] > 1e-4).all()
    # two clips of one size in one call: the equal frames are the last of the first clip and the first of the second
    ra, rb = r0.clone(), r0.flip(1).contiguous()
    tb = t.flip(1).contiguous()
    ra[:, -1], rb[:, 0] = t[:, -1], tb[:, 0]
    got, _ = raw_call(model, [ra, rb], [t, tb])
    n = r0.shape[1]
    assert float(got[n - 1]) == 0.0 and float(got[n]) == 0.0
    assert (got[:n - 1] > 1e-4).all() and (got[n + 1:] > 1e-4).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_the_reconstruction_is_clamped_and_the_target_is_not(model, dtype):
    r, t = dev_pair(1, dtype)
    wild = (3 * r).contiguous()                                   # out to beyond +-3
    assert float(wild.abs().max()) > 3
    a = model.frame_distances([wild], [t])
    assert torch.equal(a, model.frame_distances([wild.clamp(-1, 1)], [t]))
    assert torch.equal(a, model.frame_distances([wild.clamp(-1, 1)], [t], clamp_recon=False))
    assert not torch.equal(a, model.frame_distances([wild], [t], clamp_recon=False))
    b = model.frame_distances([r], [wild])                        # a target out to +-3 stays as it is
    assert not torch.equal(b, model.frame_distances([r], [wild.clamp(-1, 1)]))
    # ... and the value is the unclamped target's: clamping it would move the value by far more than either dtype's error (bf16
    # keeps 8 significant bits, 2^-7 = 8e-3 per rounding)
    free = E.frame_values(state(), r.float().cpu(), wild.float().cpu())
    assert rel(E.frame_values(state(), r.float().cpu(), wild.float().cpu().clamp(-1, 1)), free) > 0.1
    assert rel(b, free) < (1e-5 if dtype == torch.float32 else 2e-2)


def test_passes_and_grouping(model):
    """A mixed list in one call, clip by clip, and with workspace budgets that force single-frame passes and passes that cut a
    clip: per-frame values within 1e-6 relative in fp32, identical bits on a rerun, the accumulator equal to the double sum."""
    shapes = [(2, 17, 23), (3, 24, 40), (2, 17, 23)]
    pairs = [E.clip_pair(s, 70 + k) for k, s in enumerate(shapes)]
    rs = [p[0].to(DEV) for p in pairs]
    ts = [p[1].to(DEV) for p in pairs]
    em = EvalMetrics(SimpleNamespace(training=SimpleNamespace(eval=SimpleNamespace(log_metrics=["lpips"]))), lpips_model=model)
    em.update(rs, ts)
    whole = model.frame_distances(rs, ts)
    assert whole.shape == (7,) and whole.dtype == torch.float32
    ref = torch.cat([E.frame_values(state(), *p) for p in pairs])
    assert rel(whole, ref) < 1e-5                                  # clip then frame order, whatever the grouping
    acc = em._lpips_acc.cpu()
    assert float(acc[1]) == 7.0
    assert abs(float(acc[0]) - float(whole.double().sum())) <= 1e-12 * float(whole.double().sum())
    assert abs(em.compute()["eval/lpips"] - float(whole.double().mean())) <= 1e-12
    assert torch.equal(whole, model.frame_distances(rs, ts)), "two identical calls differ"
    by_clip = torch.cat([model.frame_distances([r], [t]) for r, t in zip(rs, ts)])
    one = _lib.lib().ttv_lpips_eval_workspace_bytes(1, 24, 40, _lib.TTV_F32)
    single = model.frame_distances(rs, ts, workspace_bytes=1)      # below one frame's need: single-frame passes
    assert model._eval_ws.numel() >= one
    three = _lib.lib().ttv_lpips_eval_workspace_bytes(3, 17, 23, _lib.TTV_F32)
    cut, acc2 = raw_call(model, [rs[0], rs[2]], [ts[0], ts[2]], frames_per_pass=3)     # passes of 3 + 1 frames: the second clip is cut
    assert three < _lib.lib().ttv_lpips_eval_workspace_bytes(4, 17, 23, _lib.TTV_F32)
    for name, other in (("clip by clip", by_clip), ("single-frame passes", single)):
        assert rel(other, whole) < 1e-6, name
    assert rel(cut, whole[[0, 1, 5, 6]]) < 1e-6
    assert float(acc2[1]) == 4.0 and float(acc2[0]) == seq_sum(cut)
    # bf16: the same list, the same order (values may move in the last bits between pass sizes: split-K follows the stack's size)
    rb, tb = [r.to(torch.bfloat16) for r in rs], [t.to(torch.bfloat16) for t in ts]
    wb = model.frame_distances(rb, tb)
    assert torch.equal(wb, model.frame_distances(rb, tb))
    assert rel(model.frame_distances(rb, tb, workspace_bytes=1), wb) < 1e-3 and rel(wb, ref) < 2e-2


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_benchmark_clip_equals_the_loss_path_per_frame(model, dtype):
    """16 x 128 x 128 in one pass runs the loss path's kernels on the same stack in the same order: per-frame values equal
    LPIPS.forward on the 16 frame pairs to the project's batch-independence figure, 1e-6 relative (measured: identical bits)."""
    r, t = dev_pair(6, dtype)
    got = model.frame_distances([r], [t])
    with torch.no_grad():
        want, _ = model(r.clamp(-1, 1).permute(1, 0, 2, 3).contiguous(), t.permute(1, 0, 2, 3).contiguous(), compute_gram=False)
    print(f"{dtype}: frame_distances vs LPIPS.forward rel {rel(got, want):.2e}, equal bits {torch.equal(got, want)}")
    assert rel(got, want) <= 1e-6


def test_eval_metrics_surface_and_shared_weights(model):
    cfg = SimpleNamespace(training=SimpleNamespace(eval=SimpleNamespace(log_metrics=["psnr", "ssim", "lpips"])))
    r1, t1 = dev_pair(2, torch.bfloat16)
    r2, t2 = dev_pair(1, torch.bfloat16)
    with torch.no_grad():
        model(r1[:, 0, :16, :16][None].contiguous(), t1[:, 0, :16, :16][None].contiguous())      # the loss path packs the weights
    pack = model._pack_cache[1]
    em = EvalMetrics(cfg, lpips_model=model)
    assert em.compute() == {}
    em.update([r1, r2], [t1.float(), t2.float()])                 # targets are cast to the reconstruction's dtype
    assert model._pack_cache[1] is pack, "a second pack was built"
    out = em.compute()
    assert list(out) == ["eval/psnr", "eval/ssim", "eval/lpips"]
    want = model.frame_distances([r1, r2], [t1, t2]).double().mean()
    assert abs(out["eval/lpips"] - float(want)) <= 1e-12 and out["eval/lpips"] > 0
    plain = EvalMetrics(SimpleNamespace(training=SimpleNamespace(eval=SimpleNamespace(log_metrics=["psnr", "ssim"]))))
    plain.update([r1, r2], [t1, t2])
    assert {k: v for k, v in out.items() if k != "eval/lpips"} == plain.compute()
    em.update([r1], [t1])
    assert float(em._lpips_acc[1]) == 8.0
    em.reset()
    assert float(em._lpips_acc.abs().sum()) == 0.0
    assert np.isnan(em.compute()["eval/lpips"])
    em.update([r2], [t2])
    assert abs(em.compute()["eval/lpips"] - float(model.frame_distances([r2], [t2]).double().mean())) <= 1e-12
    assert not any("lpips" in k for k in em.state_dict())
    with pytest.raises(ValueError, match="15 x 16"):
        em.update([torch.zeros((3, 1, 15, 16), device=DEV)], [torch.zeros((3, 1, 15, 16), device=DEV)])
    with pytest.raises(TypeError):
        model.frame_distances([r1.half()], [t1.half()])


def test_validation_loop_carries_eval_lpips():
    from titok_video_amd.model.titok import TiTok
    from titok_video_amd.synthetic import seeded_titok_state, synthetic_clips
    from titok_video_amd.train import ValidationLoop
    cfg = SimpleNamespace(tokenizer=SimpleNamespace(model=SimpleNamespace(patch_size=[4, 8, 8], fsq_levels=[7, 5, 5, 5, 5],
                                                                           encoder_size="tiny", decoder_size="tiny")),
                          training=SimpleNamespace(eval=SimpleNamespace(log_metrics=["psnr", "lpips"])))
    tok = TiTok(cfg)
    tok.load_state_dict(seeded_titok_state(0), strict=True)
    tok = tok.to(DEV, torch.float32).eval()
    clips = synthetic_clips([(4, 16, 16), (4, 24, 40)], seed=3, dtype=torch.float32, device=DEV)
    metrics = EvalMetrics(cfg, lpips_weights=state())
    loop = ValidationLoop(tok, metrics, log_recon_num=0, eval_samples=2, random_recon=False)
    loop.start()
    loop.step({"video": clips, "fps": [8, 8], "token_counts": [3, 6]})
    out = loop.end()
    assert set(out) == {"eval/psnr", "eval/lpips"} and np.isfinite(out["eval/lpips"]) and out["eval/lpips"] > 0
    with torch.no_grad():
        recon = tok(clips, [3, 6])[0]
    want = metrics._lpips.frame_distances(recon, clips).double().mean()
    assert abs(out["eval/lpips"] - float(want)) <= 1e-9 * float(want)
    assert float(metrics._lpips_acc.abs().sum()) == 0.0              # end() reset the metrics
