"""CPU checks of the evaluation LPIPS (EvalMetrics 'lpips'): the float64 per-frame restatement (tests/lpips_eval_ref.py) against the
reference's own fp32 per-frame values at frame sizes that are not multiples of 16 (tests/golden/lpips_eval_kat.npz), what the bf16
restatement measures, the EvalMetrics config surface, the shape refusals and the C-ABI argument checks.  No GPU."""
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

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FP32_VALUE = 1e-5      # the project's fp32-vs-float64 figure for this network (tests/test_lpips_cpu.py); measured here <= 2.4e-7
SMALL = [0, 1, 2, 3, 5]   # the fixture's clips with an edge below 64


def _cfg(names, **extra):
    return SimpleNamespace(training=SimpleNamespace(eval=SimpleNamespace(log_metrics=list(names), **extra)))


def test_restatement_matches_reference_fixture_per_frame():
    d = np.load(os.path.join(G, "lpips_eval_kat.npz"))
    assert d["shapes"].tolist() == [list(s) for s in E.SHAPES] and int(d["clip_seed"]) == E.CLIP_SEED
    sd = seeded_lpips_state(int(d["weight_seed"]))
    for i, (recon, target) in enumerate(E.fixture_pairs()):
        np.testing.assert_allclose(E.fingerprint(recon, target), d[f"clip{i}_fp"], rtol=1e-6)
        if i == 6:
            recon, target = recon[:, :4], target[:, :4]      # four frames of the 128 x 128 clip are enough here
        got = E.frame_values(sd, recon, target).numpy()
        want = d[f"clip{i}_lpips"].astype(np.float64)[:len(got)]
        rel = np.abs(got - want) / np.abs(want)
        print(f"clip {i} {E.SHAPES[i]}: per-frame rel {rel.max():.2e}")
        assert rel.max() < FP32_VALUE, (i, rel)


def test_restatement_clamps_the_reconstruction_only():
    sd = seeded_lpips_state(E.WEIGHT_SEED)
    recon, target = E.clip_pair((2, 17, 23), 3)
    assert float(recon.abs().max()) > 1.0
    a = E.frame_values(sd, recon, target)
    assert torch.equal(a, E.frame_values(sd, recon.clamp(-1, 1), target, clamp=False))
    assert not torch.equal(a, E.frame_values(sd, recon, target, clamp=False))
    # identical frames give exactly zero; the values are per frame (frame 1 does not move when frame 0 changes)
    same = E.frame_values(sd, torch.cat([target[:, :1], recon[:, 1:]], 1), target)
    assert float(same[0]) == 0.0 and float(same[1]) == float(a[1])


def test_bf16_restatement_error_at_the_small_shapes():
    """What bf16 storage alone costs where one stage-4 pixel carries a whole tap: the per-clip worst relative error of the bf16
    restatement against float64 on the same clips.  Measured: (5,16,16) 1.62e-3, (2,17,23) 6.08e-4, (3,24,40) 6.38e-4,
    (2,40,24) 5.19e-4, (1,16,520) 3.46e-4.  The GPU test sets its bound at twice these, computed there from the same inputs."""
    sd = seeded_lpips_state(E.WEIGHT_SEED)
    pairs = E.fixture_pairs()
    for i in SMALL:
        recon, target = pairs[i]                           # bf16-representable as drawn
        ref = E.frame_values(sd, recon, target)
        err = float(((E.frame_values_bf16(sd, recon, target) - ref).abs() / ref.abs()).max())
        print(f"clip {i} {E.SHAPES[i]}: bf16 restatement rel {err:.2e}")
        assert 0 < err < 2e-2      # bf16 has 8 significant bits: a per-frame sum of thousands of rounded terms stays well inside


def test_lpips_is_accepted_in_config_order_with_weights(tmp_path):
    sd = seeded_lpips_state(2)
    m = EvalMetrics(_cfg(["psnr", "ssim", "lpips"]), lpips_weights=sd)
    assert m.names == ["psnr", "ssim", "lpips"] and isinstance(m._lpips, LPIPS)
    assert torch.equal(m._lpips.net.slice5._modules["28"].bias, sd["net.slice5.28.bias"])
    assert m.compute() == {}
    # the weights are held outside the module tree: not in state_dict(), not moved or cast with the metrics
    assert list(m.state_dict().keys()) == [] and list(m.parameters()) == []
    torch.save(sd, tmp_path / "lpips.pth")
    by_key = EvalMetrics(_cfg(["lpips", "psnr"], lpips_weights=str(tmp_path / "lpips.pth")))
    assert by_key.names == ["lpips", "psnr"]
    assert torch.equal(by_key._lpips.lin4.model[-1].weight, sd["lin4.model.1.weight"])
    by_arg = EvalMetrics(_cfg(["lpips"]), lpips_weights=str(tmp_path / "lpips.pth"))
    assert torch.equal(by_arg._lpips.lin0.model[-1].weight, sd["lin0.model.1.weight"])
    shared = LPIPS()
    assert EvalMetrics(_cfg(["psnr", "lpips"]), lpips_model=shared)._lpips is shared
    assert EvalMetrics(_cfg(["psnr"]), lpips_weights=sd)._lpips is None      # not asked for: nothing is loaded


def test_lpips_without_weights_raises_the_unchanged_message():
    with pytest.raises(NotImplementedError, match="psnr, ssim"):
        EvalMetrics(_cfg(["ssim", "psnr", "lpips"]))
    with pytest.raises(NotImplementedError, match="metric 'lpips' is not built"):
        EvalMetrics(_cfg(["lpips"]))


def test_bad_clips_are_refused_before_any_launch():
    m = LPIPS()
    z = torch.zeros
    with pytest.raises(ValueError, match="15 x 16"):
        m.frame_distances([z(3, 2, 15, 16)], [z(3, 2, 15, 16)])
    with pytest.raises(ValueError, match="16 .. 2048"):
        m.frame_distances([z(3, 1, 16, 2056)], [z(3, 1, 16, 2056)])
    with pytest.raises(ValueError, match="one shape"):
        m.frame_distances([z(3, 2, 16, 24)], [z(3, 2, 24, 16)])
    with pytest.raises(ValueError, match="one shape"):
        m.frame_distances([z(1, 2, 16, 16)], [z(1, 2, 16, 16)])
    with pytest.raises(ValueError):
        m.frame_distances([z(3, 2, 16, 16)], [])
    with pytest.raises(TypeError, match="no CPU path"):
        m.frame_distances([z(3, 2, 16, 24)], [z(3, 2, 16, 24)])


def test_cabi_exports_and_argument_checks():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    h = _lib.lib()
    for name in ("ttv_lpips_eval_workspace_bytes", "ttv_lpips_eval_accumulate"):
        assert name in _lib.SYMBOLS
        getattr(h, name)
    BF, F32 = _lib.TTV_BF16, _lib.TTV_F32
    # two buffers of 2 x 16 frames x 128 x 128 x 64 bf16, the head partials and up to 32 MiB of split-K partials: far below the loss
    # path's tape for the same frames
    n = h.ttv_lpips_eval_workspace_bytes(16, 128, 128, BF)
    assert 2 * 2 * 16 * 128 * 128 * 64 * 2 < n < 2 * 2 * 16 * 128 * 128 * 64 * 2 + (33 << 20)
    assert n < h.ttv_lpips_tape_bytes(16, 128, 128, BF)
    assert h.ttv_lpips_eval_workspace_bytes(16, 128, 128, F32) > 2 * 2 * 16 * 128 * 128 * 64 * 4
    assert h.ttv_lpips_eval_workspace_bytes(2, 136, 168, BF) > 0 and h.ttv_lpips_eval_workspace_bytes(1, 17, 23, F32) > 0
    assert h.ttv_lpips_eval_workspace_bytes(1, 16, 16, BF) % 256 == 0
    for bad in ((1, 15, 16, BF), (1, 16, 2049, BF), (0, 16, 16, BF), (2049, 16, 16, BF), (1, 16, 16, 7)):
        assert h.ttv_lpips_eval_workspace_bytes(*bad) == -1, bad
    assert b"dtype 7" in h.ttv_error_string()
    # every argument error returns before any device work (there is no device here)
    w = _lib.LpipsWeights()
    one = (_lib.vp * 1)(256)
    frames = (_lib.C.c_int32 * 1)(2)
    args = lambda **k: [k.get("w", _lib.C.byref(w)), one, one, k.get("frames", frames), 1, k.get("H", 17), 23, k.get("dtype", BF), 1, 256, None,
                        k.get("ws", 256), 1 << 20, None]
    assert h.ttv_lpips_eval_accumulate(*args(w=None)) == 1 and b"null weights" in h.ttv_error_string()
    assert h.ttv_lpips_eval_accumulate(*args()) == 1 and b"null weight image" in h.ttv_error_string()
    for l in range(13):
        w.w[l] = w.wd[l] = w.b[l] = 256
    for k in range(5):
        w.lin[k] = 256
    assert h.ttv_lpips_eval_accumulate(*args(H=15)) == 1 and b"15 x 23" in h.ttv_error_string()
    assert h.ttv_lpips_eval_accumulate(*args(dtype=3)) == 1 and b"dtype" in h.ttv_error_string()
    assert h.ttv_lpips_eval_accumulate(*args(frames=(_lib.C.c_int32 * 1)(0))) == 1 and b"0 frames" in h.ttv_error_string()
    assert h.ttv_lpips_eval_accumulate(*args(ws=128)) == 1 and b"aligned" in h.ttv_error_string()
    a = args()
    a[12] = 4096                                                  # a workspace too small for one frame
    assert h.ttv_lpips_eval_accumulate(*a) == 1 and b"one 17 x 23 frame needs" in h.ttv_error_string()
    a = args()
    a[9] = None                                                   # neither per-frame values nor an accumulator
    assert h.ttv_lpips_eval_accumulate(*a) == 1 and b"null argument" in h.ttv_error_string()
