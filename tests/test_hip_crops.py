"""ttv_lpips_crops_forward / ttv_lpips_crops_backward (csrc/ttv_crops.hip) on the MI355X, through the C ABI, against the float64
restatement of tests/crops_ref.py; then `ReconstructionLoss` with the fused crop path and with TTV_LPIPS_CROPS=0.

THE BOUND of every value comparison, per element, from the kernel's rounding steps (nothing here is tuned to what the kernel gives):
  * not resized: the crop is a copy and the gradient is g or 0: equality.
  * resized, forward: the kernel forms h_r = sum_k wx_k v_rk and out = sum_r wy_r h_r as two fmaf chains of four, so c = 4 + 4 = 8
    roundings lie on the path of every term: |fl(out) - sum| <= gamma_8 * S, S = sum |wy| |wx| |v| (gamma_n = n u / (1 - n u),
    u = 2^-24: c * 2^-24 * S with its second-order part).  The weights are the float32 weights themselves: src, floor and t are
    reproduced exactly, and the Keys polynomials are evaluated either operation by operation (crops_ref mode "f32") or as a
    compiler contracts them into fma (mode "f32c", exact too).  Which of the two the build uses is the compiler's choice; an
    output array must meet the bound against ONE of them in all its elements, and no slack is added for the choice.  Then one
    rounding to the clip dtype: half an ulp at the value rounded, which lies within E = gamma_8 S of the reference:
    half_ulp(|ref| + E) (= half an ulp at the reference except across a power of two).
  * resized, backward: the gather adds its terms with fmaf, n_x(x) column taps into a row sum and n_y(y) row taps into the result:
    c = n_x + n_y roundings, counted per pixel from the tap tables (crops_ref.backward's `n`), the same weights, the same final
    rounding.  The mask is exact.
No element of any output is left out: whole crops, whole clip gradients (zeros of unsampled frames and outside footprints included),
and guard bands around every destination.
"""
import os
import random
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crops_ref as CR  # noqa: E402
import lpips_ref as R  # noqa: E402

from titok_video_amd import _lib  # noqa: E402
from titok_video_amd.model.losses import PerceptualCrops, ReconstructionLoss, perceptual_crop_plan  # noqa: E402
from titok_video_amd.synthetic import seeded_lpips_state  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"bf16": torch.bfloat16, "f32": torch.float32}
GUARD = 64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def L():
    return _lib.lib()


def S():
    return _lib.stream_ptr(torch.device(DEV))


def make_clip(shape, dt, seed):
    """[3,T,H,W] in the dtype, CPU: normal with sigma 1.2 (40 % of the values outside [-1, 1]), with exact -1, +1 and their
    neighbours one ulp to either side planted at both ends of every frame's rows 0, 1 and H // 2."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn((3,) + tuple(shape), generator=g) * 1.2).to(DT[dt])
    one = torch.ones((), dtype=DT[dt])
    up, down = torch.nextafter(one, one * 2), torch.nextafter(one, one * 0)
    vals = torch.stack([one, -one, up, -up, down, -down])
    H, W = shape[1], shape[2]
    n = min(6, W)
    for row in (0, 1, H // 2):
        x[:, :, row, :n] = vals[:n]
        x[:, :, row, W - n:] = vals[:n].flip(0)
    return x


def guarded(numel, dt, fill=7.0):
    buf = torch.full((GUARD + numel + GUARD,), fill, dtype=DT[dt], device=DEV)
    return buf, buf[GUARD:GUARD + numel]


def guards_ok(buf, numel, fill=7.0):
    h = buf.float().cpu()
    return bool((h[:GUARD] == fill).all() and (h[GUARD + numel:] == fill).all())


def dims_of(clips):
    flat = [int(v) for c in clips for v in c.shape[1:]]
    return (_lib.i32 * len(flat))(*flat)


def table_of(rows):
    flat = [int(v) for r in rows for v in r]
    return (_lib.i32 * len(flat))(*flat)


def call_forward(recon, target, rows, size, dt, expect_rc=0, dtype_code=None, dst_off=0):
    """recon / target: device clips.  Returns (recon crops, target crops) on the device, after checking the guard bands; the error
    text of a refused call (whose destinations must be untouched)."""
    n = len(rows) * 3 * size * size
    rb, rv = guarded(n + dst_off, dt)
    tb, tv = guarded(n + dst_off, dt)
    rc = L().ttv_lpips_crops_forward(_lib.ptr_array(recon), _lib.ptr_array(target), dims_of(recon), len(recon), table_of(rows), len(rows), size,
                                     rv[dst_off:].data_ptr(), tv[dst_off:].data_ptr(), _lib.dtype_code(DT[dt]) if dtype_code is None else dtype_code, S())
    msg = L().ttv_error_string().decode()
    torch.cuda.synchronize()
    assert rc == expect_rc, msg
    assert guards_ok(rb, n + dst_off) and guards_ok(tb, n + dst_off), "written outside a destination"
    if rc != 0:
        assert (rv == 7.0).all() and (tv == 7.0).all(), "a refused call wrote to its destination"
        return msg
    return rv.view(len(rows), 3, size, size), tv.view(len(rows), 3, size, size)


def call_backward(recon, rows, size, g, dt, expect_rc=0, dtype_code=None, dst_off=0):
    bufs, views = zip(*[guarded(c.numel() + dst_off, dt) for c in recon])
    rc = L().ttv_lpips_crops_backward(_lib.ptr_array(recon), _lib.ptr_array([v[dst_off:] for v in views]), dims_of(recon), len(recon),
                                      table_of(rows), len(rows), size, g.data_ptr(), _lib.dtype_code(DT[dt]) if dtype_code is None else dtype_code, S())
    msg = L().ttv_error_string().decode()
    torch.cuda.synchronize()
    assert rc == expect_rc, msg
    for b, c in zip(bufs, recon):
        assert guards_ok(b, c.numel() + dst_off), "written outside a destination"
    if rc != 0:
        assert all(bool((v == 7.0).all()) for v in views), "a refused call wrote to its destination"
        return msg
    return [v.view(c.shape) for v, c in zip(views, recon)]


def row(clips, clip, frame, size, resized, oy, ox):
    """A table row; oy / ox: an origin, or "max"."""
    H, W = clips[clip].shape[2:]
    Hr, Wr = CR.resized_hw(H, W, size) if resized else (H, W)
    return (clip, frame, H, W, Hr, Wr, Hr - size if oy == "max" else oy, Wr - size if ox == "max" else ox)


# name -> (clip shapes (T, H, W), size, rows as (clip, frame, resized, oy, ox))
def scenarios():
    out = {
        "copy_origin_0_and_max": ([(2, 160, 144)], 128, [(0, 0, False, 0, 0), (0, 1, False, "max", "max")]),
        "down_168x136_to_158x128": ([(2, 168, 136)], 128, [(0, 1, True, 0, 0), (0, 0, True, "max", 0)]),
        "up_96x160_to_128x213": ([(3, 96, 160)], 128, [(0, 0, True, 0, 0), (0, 2, True, 0, "max")]),
        "up_64x64_to_128x128": ([(2, 64, 64)], 128, [(0, 1, True, 0, 0)]),
        "one_edge_below_s_t1": ([(1, 100, 200)], 128, [(0, 0, True, 0, 77)]),
        "s64": ([(2, 64, 48), (2, 80, 72)], 64, [(0, 0, True, 10, 0), (1, 1, False, 16, 8), (1, 0, True, 3, 0)]),
        "ragged_odd_widths": ([(2, 50, 70), (1, 45, 51), (3, 40, 56), (2, 32, 32)], 32,
                              [(0, 1, True, 0, 5), (0, 0, False, 9, 21), (1, 0, True, 0, 3), (2, 2, False, 8, 24), (2, 0, True, 0, 7),
                               (3, 1, False, 0, 0), (3, 0, True, 0, 0)]),
    }
    rng = random.Random(3)
    shapes = [(16, 40, 56)] * 3 + [(16, 36, 44)] * 2
    rows = []
    for c, (t, h, w) in enumerate(shapes):
        for f in range(t):
            resized = rng.random() < 0.5
            hr, wr = CR.resized_hw(h, w, 32) if resized else (h, w)
            rows.append((c, f, resized, rng.randrange(hr - 32 + 1), rng.randrange(wr - 32 + 1)))
    rng.shuffle(rows)
    out["80_crops_every_frame"] = (shapes, 32, rows)
    return out


SCENARIOS = scenarios()


def build(name, dt):
    shapes, size, spec = SCENARIOS[name]
    seed = sum(map(ord, name))
    recon = [make_clip(s, dt, seed + 2 * i) for i, s in enumerate(shapes)]
    target = [make_clip(s, dt, seed + 2 * i + 1) for i, s in enumerate(shapes)]
    rows = [row(recon, c, f, size, rs, oy, ox) for c, f, rs, oy, ox in spec]
    return recon, target, rows, size


TAP_MODES = ("f32", "f32c")


def within(got, refs_and_bounds):
    """(passes, worst error / bound): `got` meets its bound in every element against one of the (ref, tol) pairs."""
    ratios = []
    for ref, tol in refs_and_bounds:
        err = np.abs(got - ref)
        ratios.append(float((err / np.maximum(tol, 1e-300)).max()) if tol.any() else float(err.max()))
        if (err <= tol).all():
            return True, ratios[-1]
    return False, min(ratios)


def forward_bounds(frame64, geom, size, clamped, resized, dt):
    out = []
    for mode in TAP_MODES if resized else TAP_MODES[:1]:
        ref, Ssum, _Sw = CR.forward(frame64, geom, size, clamped, mode)
        E = CR.gamma(8) * Ssum
        out.append((ref, E + CR.half_ulp(np.abs(ref) + E, dt) if resized else np.zeros_like(ref)))
    return out


def backward_bounds(g64, x64, geom, size, resized, dt):
    out = []
    for mode in TAP_MODES if resized else TAP_MODES[:1]:
        dref, Ssum, _Sw, n = CR.backward(g64, x64, geom, size, mode)
        E = CR.gamma(n)[None] * Ssum
        out.append((dref, E + CR.half_ulp(np.abs(dref) + E, dt) if resized else np.zeros_like(dref)))
    return out


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_forward_and_backward_against_float64(name, dt):
    recon, target, rows, size = build(name, dt)
    assert name != "80_crops_every_frame" or len(rows) > _lib.TTV_MAX_CLIPS_PER_LAUNCH
    rd, td = [c.to(DEV) for c in recon], [c.to(DEV) for c in target]
    rc, tc = call_forward(rd, td, rows, size, dt)
    rc2, tc2 = call_forward(rd, td, rows, size, dt)
    assert torch.equal(rc, rc2) and torch.equal(tc, tc2), "two identical forward calls differ"
    g = (torch.randn(rc.shape, generator=torch.Generator().manual_seed(len(rows))) * 0.5).to(DT[dt])
    gd = g.to(DEV)
    grads = call_backward(rd, rows, size, gd, dt)
    grads2 = call_backward(rd, rows, size, gd, dt)
    assert all(torch.equal(a, b) for a, b in zip(grads, grads2)), "two identical backward calls differ"
    worst = {"fwd": 0.0, "bwd": 0.0, "torch_fwd": 0.0, "torch_bwd": 0.0}
    sampled = set()
    for k, (clip, frame, H, W, Hr, Wr, oy, ox) in enumerate(rows):
        geom, resized = (H, W, Hr, Wr, oy, ox), (Hr, Wr) != (H, W)
        sampled.add((clip, frame))
        for out, src, clamped in ((rc, recon, True), (tc, target, False)):
            ok, ratio = within(out[k].double().cpu().numpy(), forward_bounds(src[clip][:, frame].double().numpy(), geom, size, clamped, resized, dt))
            worst["fwd"] = max(worst["fwd"], ratio)
            assert ok, f"{name} {dt}: crop {k} forward: error / bound {ratio:.3f} (absolute error for a copy)"
        got = grads[clip][:, frame].double().cpu().numpy()
        ok, ratio = within(got, backward_bounds(g[k].double().numpy(), recon[clip][:, frame].double().numpy(), geom, size, resized, dt))
        worst["bwd"] = max(worst["bwd"], ratio)
        assert ok, f"{name} {dt}: crop {k} backward: error / bound {ratio:.3f} (absolute error for a copy)"
        assert not got[:, ~CR.touched(geom, size)].any(), f"{name} {dt}: crop {k}: gradient outside the window's footprint"
        # the eager path on the same device: equality where nothing is resampled, a distance for information where torch resamples
        if dt == "f32" or not resized:
            xe = rd[clip][:, frame].clone().requires_grad_(True)
            v, t = xe.clamp(-1, 1), td[clip][:, frame]
            if resized:
                v = F.interpolate(v[None], size=(Hr, Wr), mode="bicubic", align_corners=False)[0]
                t = F.interpolate(t[None], size=(Hr, Wr), mode="bicubic", align_corners=False)[0]
            v, t = v[:, oy:oy + size, ox:ox + size], t[:, oy:oy + size, ox:ox + size]
            (ge,) = torch.autograd.grad(v, xe, gd[k])
            if resized:
                worst["torch_fwd"] = max(worst["torch_fwd"], float((v.detach() - rc[k]).abs().max()), float((t - tc[k]).abs().max()))
                worst["torch_bwd"] = max(worst["torch_bwd"], float((ge - grads[clip][:, frame]).abs().max()))
            else:
                assert torch.equal(v.detach(), rc[k]) and torch.equal(t, tc[k]), f"{name} {dt}: crop {k} is not the eager copy"
                assert torch.equal(ge, grads[clip][:, frame]), f"{name} {dt}: crop {k}: gradient is not the eager one"
    for c, clip in enumerate(recon):
        for f in range(clip.shape[1]):
            if (c, f) not in sampled:
                assert not grads[c][:, f].any(), f"{name} {dt}: unsampled frame {f} of clip {c} is not zero"
    print(f"{name} {dt}: {len(rows)} crops; worst error / bound forward {worst['fwd']:.3f}, backward {worst['bwd']:.3f} (copies: absolute); "
          f"for information, max distance from torch's GPU fp32 F.interpolate {worst['torch_fwd']:.2e}, its autograd {worst['torch_bwd']:.2e}")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_mask_is_inclusive_at_plus_and_minus_one(dt):
    """Planted values: exactly +-1 pass the gradient, one ulp outside blocks it, in a copy crop where the gradient is g itself."""
    recon, target, rows, size = build("copy_origin_0_and_max", dt)
    rd = [c.to(DEV) for c in recon]
    g = torch.full((len(rows), 3, size, size), 0.5, dtype=DT[dt], device=DEV)
    grads = call_backward(rd, rows, size, g, dt)
    got = grads[0][:, 0, 0, :6].float().cpu()          # frame 0, window at the origin, row 0: 1, -1, 1 + ulp, -(1 + ulp), 1 - ulp, -(1 - ulp)
    assert got.tolist() == [[0.5, 0.5, 0.0, 0.0, 0.5, 0.5]] * 3


def test_refusals_launch_nothing():
    dt = "f32"
    recon, target, rows, size = build("s64", dt)
    rd, td = [c.to(DEV) for c in recon], [c.to(DEV) for c in target]
    g = torch.zeros((len(rows), 3, size, size), device=DEV)

    def both(bad_rows, word, **kw):
        for msg in (call_forward(rd, td, bad_rows, size, dt, expect_rc=1, **kw), call_backward(rd, bad_rows, size, g, dt, expect_rc=1, **kw)):
            assert word in msg, (word, msg)

    both(rows, "dtype", dtype_code=7)
    r = list(rows[1]); r[6] += 1                       # rows 17 .. 80 of 80
    both([rows[0], tuple(r)], "window")
    r = list(rows[1]); r[7] = -1
    both([rows[0], tuple(r)], "window")
    r = list(rows[0]); r[5] += 1                       # 64 x 48 -> 85 x 64, not 85 x 65
    both([tuple(r)], "resized")
    r = list(rows[0]); r[4], r[5] = 64, 64             # the long edge squeezed to s as well
    both([tuple(r)], "resized")
    both([rows[0], rows[1], rows[0]], "twice")
    both(rows, "aligned", dst_off=1)
    r = list(rows[1]); r[1] = 2
    both([tuple(r)], "frame")
    both([(0, 0, 64, 48, 64, 48, 0, 0)], "outside")    # not resized and smaller than s: no window fits
    rc, tc = call_forward(rd, td, rows, size, dt)      # and the same arguments, in order, are accepted
    assert not (rc == 7.0).all()


# ------------------------------------------------------------------------------------------------- the loss module, end to end
def loss_config(samples, gram_weight=0.0, disc_weight=0.0):
    return SimpleNamespace(
        tokenizer=SimpleNamespace(model=SimpleNamespace(patch_size=[4, 8, 8], fsq_levels=[7, 5, 5, 5, 5], encoder_size="tiny", decoder_size="tiny"),
                                  losses=SimpleNamespace(disc_weight=disc_weight, perceptual_weight=1.0, gram_weight=gram_weight,
                                                         perceptual_samples_per_step=samples, perceptual_sampling_size=128)),
        discriminator=SimpleNamespace(model=SimpleNamespace(patch_size=[4, 8, 8], model_size="tiny"),
                                      losses=SimpleNamespace(gp_weight=0.1, gp_noise=0.1, centering_weight=0.01)),
        training=SimpleNamespace(main=SimpleNamespace(torch_compile=False, max_steps=10)))


def float64_chain(sd, target, recon, plan_rows):
    """l1 + mean LPIPS of the crops_ref crops (float32-tap matrices, applied with torch in float64 so autograd gives d / d recon)."""
    rec = [r.double().cpu().requires_grad_(True) for r in recon]
    trg = [t.double().cpu() for t in target]
    rcs, tcs = [], []
    for clip, frame, H, W, Hr, Wr, oy, ox in plan_rows:
        (Ry, _a, _n), (Rx, _b, _m) = CR.operators((H, W, Hr, Wr, oy, ox), 128)
        Ry, Rx = torch.from_numpy(Ry), torch.from_numpy(Rx)
        rcs.append(Ry @ rec[clip][:, frame].clamp(-1, 1) @ Rx.T)
        tcs.append(Ry @ trg[clip][:, frame] @ Rx.T)
    lp, _gr = R.lpips_gram(sd, torch.stack(rcs), torch.stack(tcs))
    l1 = torch.stack([(t - r).abs().mean() for t, r in zip(trg, rec)]).mean()
    total = l1 + lp.mean()
    return l1.detach(), lp.mean().detach(), total.detach(), torch.autograd.grad(total, rec)


def run_paths(monkeypatch, mod, target, recon, rseed):
    out = {}
    for path in ("fused", "eager"):
        monkeypatch.setenv("TTV_LPIPS_CROPS", "1" if path == "fused" else "0")
        leaves = [r.detach().clone().requires_grad_(True) for r in recon]
        random.seed(rseed)
        with R.RandomLog() as log:
            total, ld = mod(target, leaves)
        grads = torch.autograd.grad(total, leaves)
        torch.cuda.synchronize()
        out[path] = (log.array(), ld, grads)
    monkeypatch.delenv("TTV_LPIPS_CROPS")
    return out


@pytest.mark.parametrize("case", ["fixture_f32", "batch5_bf16"])
def test_loss_module_fused_and_eager_against_the_float64_chain(case, monkeypatch):
    """Both crop paths draw the same numbers and are held - each on its own, not to each other - to the float64 chain crops_ref ->
    lpips_ref.lpips_gram: the crop bound above can not be carried through the VGG trunk's bf16 MFMA kernels by derivation, so the
    bounds are the ones tests/test_hip_lpips.py already holds ttv_lpips_forward / backward to (fp32, the generator-step fixture test:
    terms 1e-4, gradient projections 3e-2 and gradient norm 1e-3; bf16: perceptual term 5e-3, gradient 0.15 of its norm), which the crop
    path's own error (1e-6 in fp32, half a bf16 ulp of a crop pixel) does not widen.  The Gram term is off: its fp32 gradient is
    ill-conditioned (test_lpips_cpu) and has its own fixture test."""
    d = np.load(os.path.join(GOLDEN, "lpips_kat.npz"))
    sd = seeded_lpips_state(int(d["weight_seed"]))
    if case == "fixture_f32":
        dtype, (target, recon) = torch.float32, R.clip_inputs(d)
    else:
        dtype = torch.bfloat16
        shapes = [(3, 16, 128, 128), (3, 16, 168, 136), (3, 16, 128, 128), (3, 16, 168, 136), (3, 16, 128, 128)]
        g = torch.Generator().manual_seed(11)
        target = [(torch.rand(s, generator=g) * 2 - 1).to(dtype) for s in shapes]
        recon = [(1.1 * t.float() + 0.2 * torch.randn(t.shape, generator=g)).to(dtype) for t in target]
    mod = ReconstructionLoss(loss_config(int(d["samples"])), perceptual_weights=sd).to(DEV)
    td, rd = [t.to(DEV) for t in target], [r.to(DEV) for r in recon]
    res = run_paths(monkeypatch, mod, td, rd, int(d["rseed"]))
    np.testing.assert_array_equal(res["fused"][0], res["eager"][0])
    if case == "fixture_f32":
        np.testing.assert_array_equal(res["fused"][0], d["random_log"])
    owner = [(c, f) for c, t in enumerate(target) for f in range(t.shape[1])]
    random.seed(int(d["rseed"]))
    plan = perceptual_crop_plan([tuple(t.shape[2:]) for t in target for _ in range(t.shape[1])], 128, int(d["samples"]))
    l1, lp, total, ref_grads = float64_chain(sd, target, recon, CR.plan_table(owner, plan))
    term_tol = 1e-4 if dtype == torch.float32 else 5e-3
    for path in ("fused", "eager"):
        _log, ld, grads = res[path]
        assert list(ld.keys()) == ["gen/recon_loss", "gen/perceptual_loss", "gen/total_loss"]
        for key, ref in (("gen/recon_loss", l1), ("gen/perceptual_loss", lp), ("gen/total_loss", total)):
            e = abs(float(ld[key]) - float(ref)) / abs(float(ref))
            print(f"{case} {path}: {key} rel {e:.3e}")
            assert e < term_tol, (path, key, e)
        for i, (gq, gr) in enumerate(zip(grads, ref_grads)):
            glob = float((gq.double().cpu() - gr).norm() / gr.norm())
            if dtype == torch.float32:      # the two statistics, and their bounds, of test_generator_step_fp32_matches_reference_fixture
                pe = R.rel_err(R.project(gq, 200 + i, int(d["proj"])), R.project(gr, 200 + i, int(d["proj"])))
                ne = abs(float(gq.double().norm()) - float(gr.norm())) / float(gr.norm())
                print(f"{case} {path}: clip {i} gradient projection {pe:.3e}, norm {ne:.3e} (for information: largest element "
                      f"{R.rel_err(gq, gr):.3e} of the largest, difference norm {glob:.3e})")
                assert pe < 3e-2 and ne < 1e-3, (path, i, pe, ne)
            else:
                print(f"{case} {path}: clip {i} gradient difference norm {glob:.3e}")
                assert glob < 0.15, (path, i, glob)
    # the frames neither path sampled have the L1 gradient only: the two paths agree there bit for bit
    taken = {owner[p[0]] for p in plan}
    for c, (a, b) in enumerate(zip(res["fused"][2], res["eager"][2])):
        for f in range(a.shape[1]):
            if (c, f) not in taken:
                assert torch.equal(a[:, f], b[:, f]), (c, f)


def test_perceptual_crops_function_matches_preprocess_on_copies():
    """PerceptualCrops against perceptual_preprocess on clips that are never resized (160 x 144, resize_prob = 0): bit equality of
    the crops and of the gradients."""
    mod = ReconstructionLoss(loss_config(6), perceptual_weights=seeded_lpips_state(1)).to(DEV)
    for dt in ("f32", "bf16"):
        target = [make_clip((4, 160, 144), dt, 40 + i).to(DEV) for i in range(2)]
        recon = [make_clip((4, 160, 144), dt, 50 + i).to(DEV).requires_grad_(True) for i in range(2)]
        random.seed(5)
        rc, tc = mod.perceptual_crops(target, recon, resize_prob=0.0)
        assert isinstance(rc.grad_fn, PerceptualCrops._backward_cls) and not tc.requires_grad
        random.seed(5)
        tf, rf = [], []
        for t, r in zip(target, recon):
            tf += t.unbind(1)
            rf += r.unbind(1)
        re_, te = mod.perceptual_preprocess(tf, rf, resize_prob=0.0)
        assert rc.shape == (7, 3, 128, 128) and torch.equal(rc, re_) and torch.equal(tc, te)
        up = torch.randn_like(rc)
        ga = torch.autograd.grad(rc, recon, up)
        gb = torch.autograd.grad(re_, recon, up)
        assert all(torch.equal(a, b) for a, b in zip(ga, gb))


def test_gan_training_step_runs_on_the_fused_path(monkeypatch):
    from titok_video_amd.model.losses import loss_module as LM
    from titok_video_amd.model.titok import TiTok
    from titok_video_amd.synthetic import seeded_titok_state, seeded_tower_state, synthetic_clips
    from titok_video_amd.train import gan_training_step, make_discriminator_optimizer, make_optimizer
    calls = []
    real_apply = LM.PerceptualCrops.apply
    monkeypatch.setattr(LM.PerceptualCrops, "apply", lambda *a: calls.append(len(a[0])) or real_apply(*a))
    monkeypatch.setattr(LM.ReconstructionLoss, "perceptual_preprocess", lambda *a, **k: pytest.fail("the eager crop path ran"))
    cfg = loss_config(24, disc_weight=0.4)
    m = TiTok(cfg)
    m.load_state_dict(seeded_titok_state(0))
    m = m.to(DEV, torch.bfloat16).train()
    lm = ReconstructionLoss(cfg, perceptual_weights=seeded_lpips_state(2))
    lm.disc_model.load_state_dict(seeded_tower_state("encoder", "tiny", (4, 8, 8), 3, 1, seed=77))
    lm = lm.to(DEV, torch.bfloat16).train()
    clips = synthetic_clips([(8, 128, 128), (8, 168, 136)], seed=1, dtype=torch.bfloat16, device=DEV)
    og, od = make_optimizer(m), make_discriminator_optimizer(lm)
    random.seed(0)
    ld, _ = gan_training_step(m, lm, clips, [128, 128], og, od)
    torch.cuda.synchronize()
    assert calls == [16]                               # 16 frames in the batch, 24 asked for: every frame once
    assert np.isfinite(float(ld["gen/perceptual_loss"])) and float(ld["gen/perceptual_loss"]) > 0
    assert all(p.grad is None or torch.isfinite(p.grad.float()).all() for p in m.parameters())
    assert any(p.grad is not None and float(p.grad.float().abs().sum()) > 0 for p in m.parameters())


def test_crops_of_non_contiguous_and_mixed_dtype_clips_equal_the_eager_ones():
    """A reconstruction that is not contiguous and a target of another dtype go through the fused path (made contiguous, cast to the
    reconstruction's dtype) and give the crops the eager definition gives.  (fp16 clips never reach the crops: the L1 term refuses
    them first, as it did before.)"""
    mod = ReconstructionLoss(loss_config(6), perceptual_weights=seeded_lpips_state(1)).to(DEV)
    wide = make_clip((4, 160, 288), "f32", 62).to(DEV)
    recon = [wide[..., ::2]]
    target = [make_clip((4, 160, 144), "bf16", 63).to(DEV)]
    assert not recon[0].is_contiguous()
    random.seed(2)
    rc, tc = mod.perceptual_crops(target, recon, resize_prob=0.0)
    random.seed(2)
    re_, te = mod.perceptual_preprocess(list(target[0].float().unbind(1)), list(recon[0].unbind(1)), resize_prob=0.0)
    assert rc.dtype == torch.float32 and torch.equal(rc, re_) and torch.equal(tc, te)
    with pytest.raises(TypeError):
        mod([t.half() for t in target], [r.half() for r in recon])
