"""The bf16 tower backward against a float64 replay of its bf16 tape (`-m gpu`).

tests/test_hip_backward.py and tests/test_hip_backward_shapes.py hold the bf16 towers to the fp32 oracle, and so only to a cosine of
0.97 per parameter and a global error of 0.12 per tower: a bf16 forward differs from the oracle by bf16 noise compounded through the
KEEL layers.  Here the reference is tests/bf16_tape.py - the same model in float64, rounded to bf16 exactly where the HIP training path
stores bf16 - so what is left is the kernels' own arithmetic, and every parameter is held to it:

  * weight matrices: every 128 x 128 tile (the output tile of k_wgrad128_bf16 and of the batched split sum k_wgrad_reduce_multi) and
    globally; gains, biases, mask tokens: globally; input clips: per 64 patch rows ([P, 768] rows); codes: globally;
  * per tower, the global error over all parameters, reported next to the gap (the distance between the rounded replay and the
    unrounded float64 model).

The HIP gradients sit at 0.64 - 1.12 of the gap from the replay, not below half of it: the rounded tape is chaotic.  On the CPU, with
no kernel involved, input clips perturbed by 1e-6 relative (far below one bf16 ulp) move the replay's encoder gradients by 0.59 of
the gap, and the top layer's to_qkv gradient by 4 % - every bf16 rounding that flips changes the next one, and the attention backward
of the upper layers (dS = P (dP - delta), a cancellation) amplifies it.  Any fp32 summation order other than the kernels' own therefore
lands at about the gap, and the worst tile (a top-layer to_qkv, 7 %) is too wide for a tile 2 % off to show.  The bounds below are
still 2 - 4 times tighter than the cosine 0.97 / global 0.12 against the fp32 oracle, and they hold for every switch.

Losses are linear with fixed seeded weights (encoder sum(wz * z), decoder sum(W * recon), W bf16 numbers), so dL/d(output) is exact and
the same on both sides.  Batches: the tiny size at FULL (1152-row sequence, K = 128 / 200 / 5), the small size at SMALL, and the
reference's training batch - 5 clips of 16x128x128 with K = 128, which runs on half-item attention tables.

The base (12 layers) and large (24 layers) towers run on SMALL as well (test_tower_gradients_bf16_against_the_tape_replay only).  The
constants below are absolute and were measured at 4 and 8 layers, and the gap grows with depth, so these two cases are held to
R x the gap of each quantity instead (tests/gap_bounds.py: R and the measured ratios; tests/test_backward_sizes_cpu.py: what that
check can still see).  Towers, global / gap (ratio), the five cases side by side - first MI355X runs:
    tiny-full, small, tiny-five   0.64 - 1.12 of the gap (the figures above)
    base    encoder 1.81e-2 / 2.26e-2 (0.80)    decoder 1.62e-2 / 1.52e-2 (1.07)
    large   encoder 3.01e-2 / 2.94e-2 (1.03)    decoder 2.68e-2 / 2.30e-2 (1.17)

The A/B switches of the bf16 backward run in child processes (each is read once per process): TTV_WGRAD_BATCHED=0 is bit-identical;
TTV_GEGLU_BWD_ERF=1 is within the same bounds and not bit-equal; TTV_TAPE_Y_F32=1 and TTV_TRAIN_FUSED_NORMS=1 are within the same
bounds of the replay with unrounded KEEL sums.  Also: ttv_fsq_backward against the float64 autograd of the straight-through FSQ.

Bounds: set from the first MI355X run with a margin of about 2 (MEASURED lines).  Worst measured over all cases and switches: tile
7.1e-2 (decoder layer 3 to_qkv), weight matrix 4.9e-2 (encoder layer 3 to_qkv), gain / bias / mask token 0.13 (small decoder
mask_token), clips 3.9e-2 per 64 patch rows and 3.2e-2 whole, codes 2.8e-2, tower 3.0e-2 (encoder; gap 4.3e-2) and 2.3e-2 (decoder;
gap 2.1e-2).  TTV_WGRAD_BATCHED=0: all 32 layer weight gradients bit-identical.
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import pytest
import torch

from oracle import titok_oracle as O
from tests import bf16_tape as T
from tests import gap_bounds as G
from tests.blockwise import block_errors, check_blockwise, check_tiles, global_error, tile_errors
from tests.test_hip_backward_shapes import FULL, SMALL, _model, _state, report
from titok_video_amd import _lib
from titok_video_amd.synthetic import synthetic_clips

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = [7, 5, 5, 5, 5]
PATCH = (4, 8, 8)
FIVE = ([(16, 128, 128)] * 5, [128] * 5)          # the reference's 5-clip training batch
CASES = {"tiny-full": ("tiny", FULL), "small": ("small", SMALL), "tiny-five": ("tiny", FIVE), "base": ("base", SMALL), "large": ("large", SMALL)}
GAP_CASES = ("base", "large")    # 12 and 24 layers: held to R x the rounding gap of each quantity (tests/gap_bounds.py), not to the constants below

TILE_TOL = 0.14          # weight matrices, every 128 x 128 tile      (measured worst 7.0e-2)
W_GLOBAL_TOL = 0.1       # weight matrices, whole                     (4.9e-2)
VEC_TOL = 0.25           # gains, biases, mask tokens                 (0.13, the small decoder's mask token: one sum over every row)
CLIP_TOL = (0.25, 6e-2)  # input clips: per 64 patch rows, whole      (block: see the MEASURED lines; whole 3.2e-2)
CODE_TOL = 6e-2          # codes                                      (2.8e-2)
TOWER_TOL = 6e-2         # per tower, all parameters together         (3.0e-2)


def _inputs(case):
    size, (shapes, counts) = CASES[case]
    g = torch.Generator().manual_seed(11)
    wz = torch.randn(sum(counts), 5, generator=g)
    codes = O.fsq_indices_to_codes(torch.randint(0, 4375, (sum(counts),), generator=g, dtype=torch.int32), LEVELS)   # bf16 numbers
    w = [torch.randn((3,) + tuple(s), generator=g).to(torch.bfloat16) for s in shapes]
    clips = synthetic_clips(shapes, seed=8, dtype=torch.bfloat16)
    return size, shapes, counts, wz, clips, codes, w


def hip_grads(case):
    """bf16 HIP gradients of both towers under the linear losses: {"params": {name: fp32}, "clips": [fp32], "codes": fp32} on the CPU."""
    size, shapes, counts, wz, clips, codes, w = _inputs(case)
    model = _model(size, torch.bfloat16)
    cl = [c.to(DEV).requires_grad_(True) for c in clips]
    z = model.encoder.forward_z(cl, list(counts))
    (z * wz.to(DEV)).sum().backward()
    cd = codes.to(DEV, torch.bfloat16).requires_grad_(True)
    rec = model.decode(cd, list(counts), [tuple(s) for s in shapes])
    sum((r.float() * wc.to(DEV).float()).sum() for r, wc in zip(rec, w)).backward()
    torch.cuda.synchronize()
    return {"params": {n: p.grad.float().cpu() for n, p in model.named_parameters()},
            "clips": [c.grad.float().cpu() for c in cl], "codes": cd.grad.float().cpu()}


@functools.lru_cache(maxsize=None)
def replay(case, rounding=True, y_bf16=True):
    """float64 gradients of the same losses: the bf16 tape replay (rounding) or the plain float64 model (no rounding)."""
    size, shapes, counts, wz, clips, codes, w = _inputs(case)
    params = {k: v.to(torch.bfloat16) for k, v in _state(size).items()}       # the bf16 model's own parameters
    enc, enc_clips = T.encoder_grads(params, clips, counts, wz, size, rounding, y_bf16)
    dec, dec_codes = T.decoder_grads(params, codes, counts, shapes, w, size, rounding, y_bf16)
    return {**enc, **dec}, enc_clips, dec_codes


def _is_matrix(t):
    return t.dim() == 2 and min(t.shape) > 1


def check_against_replay(got, case, what, y_bf16=True):
    """Every bound of the module docstring; the failures are collected so that one run reports every value.  Returns the worst figures."""
    if case in GAP_CASES:
        return check_against_gaps(got, case, what, y_bf16)
    size, shapes, counts = CASES[case][0], CASES[case][1][0], CASES[case][1][1]
    ref, ref_clips, ref_codes = replay(case, True, y_bf16)
    exact = replay(case, False)[0]
    bad, worst = [], {"tile": (0.0, ""), "matrix": (0.0, ""), "vector": (0.0, "")}

    def note(key, v, name):
        worst[key] = max(worst[key], (v, name))
    for tower in ("encoder.", "decoder."):
        names = [n for n in ref if n.startswith(tower)]
        assert set(names) == {n for n in got["params"] if n.startswith(tower)}, tower
        for n in names:
            g, r = got["params"][n], ref[n]
            if _is_matrix(r):
                try:
                    wt, wg = check_tiles(g, r, TILE_TOL, W_GLOBAL_TOL, f"{what} {n}")
                except AssertionError as e:
                    bad.append(str(e))
                    wt, wg = float(tile_errors(g, r).max()), global_error(g, r)
                note("tile", wt, n)
                note("matrix", wg, n)
            else:
                e = global_error(g, r)
                note("vector", e, n)
                if not e < VEC_TOL:
                    bad.append(f"{what} {n}: relative error {e:.3e} >= {VEC_TOL:.1e}")
        glob = T.global_distance({n: got["params"][n] for n in names}, {n: ref[n] for n in names})
        gap = T.global_distance({n: ref[n] for n in names}, {n: exact[n] for n in names})
        worst[tower + "global"], worst[tower + "gap"] = glob, gap
        report(f"{what} {tower[:-1]}: global error over all parameters {glob:.3e}, gap {gap:.3e} (ratio {glob / gap:.3f})")
        if not glob < TOWER_TOL:
            bad.append(f"{what} {tower[:-1]}: global error {glob:.3e} >= {TOWER_TOL:.1e}")
    gp = torch.cat([O.patchify(c, PATCH) for c in got["clips"]])
    rp = torch.cat([O.patchify(c, PATCH) for c in ref_clips])
    cu = [0]
    for s in shapes:
        cu.append(cu[-1] + (s[0] // PATCH[0]) * (s[1] // PATCH[1]) * (s[2] // PATCH[2]))
    try:
        worst["clips"] = check_blockwise(gp, rp, cu, 1, CLIP_TOL[0], CLIP_TOL[1], f"{what} clip gradients")
    except AssertionError as e:
        bad.append(str(e))
        worst["clips"] = (float(block_errors(gp, rp, cu, 1).max()), global_error(gp, rp))
    worst["codes"] = global_error(got["codes"], ref_codes)
    if not worst["codes"] < CODE_TOL:
        bad.append(f"{what} code gradients: relative error {worst['codes']:.3e} >= {CODE_TOL:.1e}")
    report(f"{what}: worst tile {worst['tile'][0]:.3e} ({worst['tile'][1]}), worst matrix {worst['matrix'][0]:.3e} ({worst['matrix'][1]}), "
           f"worst gain / bias {worst['vector'][0]:.3e} ({worst['vector'][1]}), clips block {worst['clips'][0]:.3e} global "
           f"{worst['clips'][1]:.3e}, codes {worst['codes']:.3e}")
    assert not bad, "\n".join(bad)
    return worst


def _tower_references(case, tower, y_bf16=True, params=None):
    """One tower's float64 gradients and input gradients (the clips, or the codes in a one-element list), twice: the rounded replay and
    the unrounded model.  The large towers' are built here, one tower at a time from `params` (the bf16 state), and not kept (2.3 GB
    per tower and replay); the others come from the cached replay, under the cache keys of its other callers."""
    size, shapes, counts, wz, clips, codes, w = _inputs(case)
    out = []
    for rounding in (True, False):
        if params is None:
            grads, rclips, rcodes = replay(case, True, y_bf16) if rounding else replay(case, False)
            out += [{n: v for n, v in grads.items() if n.startswith(tower)}, rclips if tower == "encoder." else [rcodes]]
        elif tower == "encoder.":
            out += list(T.encoder_grads(params, clips, counts, wz, size, rounding, y_bf16))
        else:
            grads, dcodes = T.decoder_grads(params, codes, counts, shapes, w, size, rounding, y_bf16)
            out += [grads, [dcodes]]
    return out


def check_against_gaps(got, case, what, y_bf16=True):
    """check_against_replay for the GAP_CASES: every quantity within tests/gap_bounds.R x its own gap.  Reports per tower the global
    error, the gap and their ratio (the line of check_against_replay), the worst ratio of every class and the worst ratio per layer."""
    shapes = CASES[case][1][0]
    bad, out = [], {}
    params = {k: v.to(torch.bfloat16) for k, v in _state("large").items()} if CASES[case][0] == "large" else None
    for tower in ("encoder.", "decoder."):
        ref, ref_in, exact, exact_in = _tower_references(case, tower, y_bf16, params)
        mine = {n: g for n, g in got["params"].items() if n.startswith(tower)}
        b, worst, per_layer, (glob, gap) = G.check_tower(mine, ref, exact, f"{what} {tower[:-1]}")
        bad += b
        if tower == "encoder.":
            b, w_in = G.check_clips(got["clips"], ref_in, exact_in, shapes, what)
        else:
            b, w_in = G.check_codes(got["codes"], ref_in[0], exact_in[0], what)
        bad += b
        del ref, exact
        report(f"{what} {tower[:-1]}: global error over all parameters {glob:.3e}, gap {gap:.3e} (ratio {glob / gap:.3f})")
        report(f"{what} {tower[:-1]}: worst figure / gap per class: "
               + "; ".join(f"{c} {r:.2f} ({f:.3e} / {g:.3e}, {n})" for c, (r, f, g, n) in worst.items() if c != "tower") + "; "
               + "; ".join(f"{c} {r:.2f} ({f:.3e} / {g:.3e})" for c, (r, f, g) in w_in.items()))
        report(f"{what} {tower[:-1]}: worst ratio per layer: "
               + " ".join(f"{'tower' if k is None else k}:{v:.2f}" for k, v in sorted(per_layer.items(), key=lambda kv: -1 if kv[0] is None else kv[0])))
        out[tower + "global"], out[tower + "gap"] = glob, gap
        out.update({tower + c: v for c, v in list(worst.items()) + list(w_in.items())})
    assert not bad, "\n".join(bad)
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_tower_gradients_bf16_against_the_tape_replay(case):
    check_against_replay(hip_grads(case), case, f"bf16 {case}")


# ---------------------------------------------------------------------------------------------- A/B switches, child processes
_STEP = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from tests.test_hip_backward_bf16 import hip_grads
torch.save(hip_grads("tiny-full"), sys.argv[2])
"""


def _child_step(path, **env):
    """The tiny-full bf16 step in a fresh process with `env` set (each switch is read once per process)."""
    r = subprocess.run([sys.executable, "-c", _STEP, ROOT, str(path)], env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return torch.load(str(path))


@pytest.fixture(scope="module")
def default_step(tmp_path_factory):
    return _child_step(tmp_path_factory.mktemp("bf16_default") / "grads.pt")


LAYER_LINEARS = ("to_qkv", "out_proj", "w12", "w3")


def _bit_equal(a, b, names=None):
    return all(torch.equal(a["params"][n], b["params"][n]) for n in (names or a["params"]))


@pytest.mark.parametrize("switch", ["TTV_WGRAD_BATCHED=0", "TTV_GEGLU_BWD_ERF=1", "TTV_TAPE_Y_F32=1", "TTV_TRAIN_FUSED_NORMS=1"])
def test_backward_switches_against_the_default_and_the_replay(switch, default_step, tmp_path):
    key, val = switch.split("=")
    got = _child_step(tmp_path / "grads.pt", **{key: val})
    names = [n for n in got["params"] if any(k in n for k in LAYER_LINEARS) and n.endswith("weight")]
    if key == "TTV_WGRAD_BATCHED":
        # one summing launch for a layer's four weight gradients or one per gradient: same partial tiles, same order (ttv_bwd.hip:1059).
        # The layer linears are what WgradBatch sums; the gains / biases accumulate with fp32 atomics (order varies from run to run).
        assert len(names) == 32
        differ = [n for n in names if not torch.equal(got["params"][n], default_step["params"][n])]
        report(f"TTV_WGRAD_BATCHED=0: {len(names) - len(differ)} of {len(names)} layer weight gradients bit-identical; differ: {differ}")
        assert not differ, differ
        return
    assert not _bit_equal(got, default_step, names), f"{switch} did not change the computation"
    check_against_replay(got, "tiny-full", f"bf16 tiny-full {switch}", y_bf16=key == "TTV_GEGLU_BWD_ERF")


# ---------------------------------------------------------------------------------------------- ttv_fsq_backward
def _fsq_specials(levels):
    """Rows with z = 0, z deep in the tanh saturation and z on a rounding boundary (bound(z) = 0.5 exactly in float64)."""
    lv = torch.tensor(levels, dtype=torch.float32)
    half_l = (lv - 1) * (1 + 1e-3) / 2
    offset = torch.where(lv % 2 == 0, 0.5, 0.0)
    shift = (offset / half_l).atanh()
    edge = (((0.5 + offset) / half_l).double().atanh() - shift.double()).float()
    n = len(levels)
    mixed = torch.tensor([0.0, 20.0, -20.0, 0.0, 0.0])[:n]
    mixed[3:] = edge[3:]
    return torch.stack([mixed, edge, torch.zeros(n), torch.full((n,), 20.0), torch.full((n,), -20.0), -edge])


@pytest.mark.parametrize("levels", [LEVELS, [8, 8, 8, 6, 5]], ids=["7-5-5-5-5", "8-8-8-6-5"])
@pytest.mark.parametrize("rows", [1, 257, 5000])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_fsq_backward(levels, rows, dt):
    """ttv_fsq_backward against the float64 autograd of the FSQ bound with a straight-through round (O.fsq_bound, fsq.py:48-51, 78-90):
    dz = dcodes * half_l / half_width * (1 - tanh(z + shift)^2), elementwise; nothing written past the last row."""
    from titok_video_amd.model.quantizer.fsq import FSQ
    fsq = FSQ(levels)
    n = len(levels)
    g = torch.Generator().manual_seed(rows + 10 * n)
    z = torch.randn(rows, n, generator=g) * 2
    sp = _fsq_specials(levels)
    z[:min(rows, sp.shape[0])] = sp[:rows]
    dcodes = torch.randn(rows, n, generator=g).to(torch.bfloat16 if dt == "bf16" else torch.float32)
    z64 = z.double().requires_grad_(True)
    b = O.fsq_bound(z64, levels)
    q = b + (b.round() - b).detach()
    (q / (torch.tensor(levels) // 2)).backward(dcodes.double())
    ref = z64.grad
    zd, dcd = z.to(DEV), dcodes.to(DEV)
    dz = torch.full((rows + 1, n), float("nan"), device=DEV)
    _lib.check(_lib.lib().ttv_fsq_backward(C.byref(fsq.params), zd.data_ptr(), dcd.data_ptr(), _lib.dtype_code(dcodes.dtype), dz.data_ptr(),
                                           rows, _lib.stream_ptr(torch.device(DEV))), "fsq_backward")
    got = dz.cpu()
    assert bool(torch.isnan(got[rows]).all()), "written past the last row"
    got = got[:rows].double()
    # relative 1e-5, plus the fp32 rounding of 1 - tanh^2 near saturation: a few ulps of 1 times |dcodes| * half_l / half_width
    k = torch.tensor([fsq.params.half_l[c] / fsq.params.half_width[c] for c in range(n)], dtype=torch.float64)
    err = (got - ref).abs()
    assert bool((err <= 1e-5 * ref.abs() + 4e-7 * dcodes.double().abs() * k).all()), float((err / (ref.abs() + 1e-30)).max())
    assert bool((got[0, 1:3] == 0).all())                            # tanh(+-20) == +-1 in fp32: no slope left
    if rows >= 5:
        assert bool((got[3:5] == 0).all())
    if dt == "f32":            # the module path: FSQ.forward under autograd -> _FsqFn.backward -> the same kernel
        zr = zd.clone().requires_grad_(True)
        codes, idx = fsq(zr)
        codes.backward(dcd)
        assert torch.equal(zr.grad.cpu(), got.float())


def test_fsq_backward_zero_rows_is_a_no_op():
    from titok_video_amd.model.quantizer.fsq import FSQ
    fsq = FSQ(LEVELS)
    z = torch.zeros(4, 5, device=DEV)
    dcodes = torch.ones(4, 5, device=DEV)
    dz = torch.full((4, 5), float("nan"), device=DEV)
    s = _lib.stream_ptr(torch.device(DEV))
    _lib.check(_lib.lib().ttv_fsq_backward(C.byref(fsq.params), z.data_ptr(), dcodes.data_ptr(), _lib.dtype_code(torch.float32),
                                           dz.data_ptr(), 0, s), "fsq_backward rows=0")
    _lib.check(_lib.lib().ttv_fsq_backward(C.byref(fsq.params), None, None, _lib.dtype_code(torch.float32), None, 0, s), "fsq_backward null")
    torch.cuda.synchronize()
    assert bool(torch.isnan(dz).all())
