"""CPU checks of the loader's resampling stage: the float64 restatement (tests/resample_ref.py) against the aten fixture, the
properties of its weights, and `data.sample_chunks` against the constraints of the reference's `_video_process`."""
import math
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref as R  # noqa: E402

from titok_video_amd.data import ClipSampling, random_resized_crop_box, resized_hw, sample_chunks  # noqa: E402

KAT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample_kat.npz")


def test_restatement_matches_aten_fixture():
    """Pre-rounding values of the float64 restatement against torch-CPU fp32 F.interpolate(mode='bicubic', antialias=True) as
    tests/golden/make_golden_resample.py recorded it.  The generator printed 2.482e-05, 1.909e-04, 1.124e-04 and 1.661e-04 as the
    largest difference of the four cases (aten's fp32 weights and sums against float64, 0 .. 255 scale); the bound is four times the
    largest of them."""
    bound = 4 * 1.909e-04
    kat = np.load(KAT)
    assert list(kat["names"]) == ["down_2x", "down_1.37x_by_1.61x", "up_1.25x", "eval_window"]
    for k, name in enumerate(kat["names"]):
        frames, geom, want = kat[f"frames_{k}"], tuple(int(v) for v in kat[f"geom_{k}"]), kat[f"out_{k}"]
        assert frames.shape[0] == 2 and want.dtype == np.float32
        got = R.prerounding(frames, geom)
        d = float(np.abs(got - want.astype(np.float64)).max())
        print(f"{name}: max |restatement - fixture| = {d:.3e} (bound {bound:.3e})")
        assert got.shape == want.shape and d <= bound, name
    assert tuple(kat["geom_3"][5:7]) != (0, 0)          # the evaluation case really has a window origin


def test_fixture_is_what_this_torch_computes():
    """The stored results are aten's: recomputed with this torch build they agree to fp32 rounding of the sums."""
    kat = np.load(KAT)
    for k in range(4):
        now = R.torch_float_path(kat[f"frames_{k}"], kat[f"geom_{k}"])
        assert float(np.abs(now - kat[f"out_{k}"]).max()) <= 1e-3


@pytest.mark.parametrize("n_in,n_out", [(16, 8), (150, 128), (640, 168), (206, 128), (390, 100), (100, 125), (50, 100), (72, 72),
                                         (1024, 128), (333, 47), (131, 93)])
def test_weights(n_in, n_out):
    scale = n_in / n_out
    support = 2.0 * scale if scale >= 1.0 else 2.0
    taps = R.axis_taps(n_in, n_out)
    assert len(taps) == n_out
    for lo, w in taps:
        assert abs(w.sum() - 1.0) <= 1e-12
        assert 1 <= len(w) <= 2 * math.ceil(support) + 1
        assert 0 <= lo and lo + len(w) <= n_in
    if n_in == n_out:
        assert np.array_equal(R.axis_matrix(n_in, n_out), np.eye(n_in))


def test_identity_and_constant_frames():
    f = R.noise_frames(3, 2, 24, 40)
    assert np.array_equal(R.levels(f, R.train_geom(2, 24, 40, 24, 40)), f.transpose(3, 0, 1, 2).astype(np.int64))
    flipped = R.levels(f, R.train_geom(2, 24, 40, 24, 40, flip=1))
    assert np.array_equal(flipped, f.transpose(3, 0, 1, 2)[..., ::-1].astype(np.int64))
    for level in (0, 1, 127, 128, 254, 255):
        c = np.full((1, 30, 44, 3), level, dtype=np.uint8)
        for g in (R.train_geom(1, 30, 44, 16, 24), R.eval_geom(1, 30, 44, 16, 24), R.train_geom(1, 30, 44, 40, 55)):
            assert (R.levels(c, g) == level).all()


def test_normalisation_restatement_equals_torch():
    lv = np.arange(256)
    t = torch.arange(256, dtype=torch.uint8).to(torch.float32) / 127.5 - 1.0
    assert np.array_equal(R.normalise(lv, "f32"), t.numpy())
    assert np.array_equal(R.normalise(lv, "bf16"), t.to(torch.bfloat16).float().numpy())
    assert np.array_equal(R.decode_levels(R.normalise(lv, "bf16")), lv) and np.array_equal(R.decode_levels(R.normalise(lv, "f32")), lv)


SAMPLING = ClipSampling(min_grid=(8, 128, 128), max_grid=(16, 168, 168), fps_range=(3, 5), max_aspect_ratio=2.0, min_scale=0.25,
                        patch_size=(4, 8, 8))


def _sources(n=200, seed=11):
    rng = random.Random(seed)
    return [((rng.randrange(24, 97), rng.randrange(128, 361), rng.randrange(128, 641)), rng.randrange(3, 31)) for _ in range(n)]


@pytest.mark.parametrize("eval_mode", [False, True])
def test_sample_chunks_obey_the_reference_constraints(eval_mode):
    s, n_chunks = SAMPLING, 0
    for k, (in_grid, in_fps) in enumerate(_sources()):
        chunks = list(sample_chunks(random.Random(k), in_grid, in_fps, s, eval=eval_mode))
        again = list(sample_chunks(random.Random(k), in_grid, in_fps, s, eval=eval_mode))
        assert chunks == again                                   # the same seed yields the same chunks
        prev_end = -1
        for c in chunks:
            n_chunks += 1
            t, ho, wo = c["out"]
            assert all(d % p == 0 for d, p in zip(c["out"], s.patch_size))
            assert all(lo <= d <= hi for d, lo, hi in zip(c["out"], s.min_grid, s.max_grid))
            assert ho <= in_grid[1] and wo <= in_grid[2]
            # the reference rounds the width bounds to the lattice: "might be slightly over the max aspect ratio"
            assert wo <= int(ho * s.max_aspect_ratio) and wo >= min(int(ho / s.max_aspect_ratio) - s.patch_size[2] + 1, s.max_grid[2])
            assert s.fps_range[0] <= c["fps"] <= min(s.fps_range[1], in_fps)
            start, end = c["span"]
            assert start == prev_end + 1 and end <= in_grid[0] and end == start + int(t * (in_fps / c["fps"]))
            prev_end = end
            idx = c["indices"]
            assert len(idx) == t and idx[0] == start and idx[-1] == end - 1 and all(a <= b for a, b in zip(idx, idx[1:]))
            assert all(0 <= i < in_grid[0] for i in idx)
            top, left, bh, bw = c["box"]
            assert 0 <= top and 0 <= left and bh >= 1 and bw >= 1 and top + bh <= in_grid[1] and left + bw <= in_grid[2]
            g = c["geom"]
            assert g[0] == t and g[1:3] == (bh, bw) and g[7:9] == (ho, wo)
            assert g[5] >= 0 and g[6] >= 0 and g[5] + ho <= g[3] and g[6] + wo <= g[4]      # window inside the resized frame
            if eval_mode:
                assert (bh, bw) == tuple(in_grid[1:]) and g[9] == 0
                assert (g[3], g[4]) == resized_hw(in_grid[1], in_grid[2], max(ho, wo)) and min(g[3], g[4]) == max(ho, wo)
                assert g[5] == int(round((g[3] - ho) / 2.0)) and g[6] == int(round((g[4] - wo) / 2.0))
            else:
                assert g[3:9] == (ho, wo, 0, 0, ho, wo) and g[9] in (0, 1)
                # area share in [min_scale, 1] up to get_params' rounding of each side to an integer (half a pixel per side); the
                # central fallback takes the largest box of the ratio instead
                area = in_grid[1] * in_grid[2]
                lo_side = (math.sqrt(s.min_scale * area * wo / ho) - 0.5) * (math.sqrt(s.min_scale * area * ho / wo) - 0.5)
                fallback = bh == in_grid[1] or bw == in_grid[2]
                assert bh * bw <= area and (bh * bw >= lo_side or fallback)
                assert abs(bw / bh - wo / ho) <= (1.0 / bh + 1.0 / bw) * max(wo / ho, 1.0) * 1.01      # fixed ratio up to that rounding
    assert n_chunks >= 200


def test_sources_below_the_minimum_yield_nothing():
    s = SAMPLING
    assert list(sample_chunks(random.Random(0), (7, 256, 256), 24, s)) == []       # fewer frames than min_grid
    assert list(sample_chunks(random.Random(0), (48, 120, 256), 24, s)) == []      # lower than min_grid
    assert list(sample_chunks(random.Random(0), (48, 256, 127), 24, s)) == []      # narrower than min_grid
    assert list(sample_chunks(random.Random(0), (48, 256, 256), 2, s)) == []       # below min_fps
    assert list(sample_chunks(random.Random(0), (200, 256, 256), 24, s)) != []     # the control: same frame, enough frames


def test_draw_order_is_the_reference_s():
    """The four randrange draws of a chunk, in the reference's order, then the crop's: replayed by hand from the same seed."""
    s, in_grid, in_fps = SAMPLING, (60, 240, 320), 12
    c = next(sample_chunks(random.Random(5), in_grid, in_fps, s))
    rng = random.Random(5)
    n = rng.randrange(8, 17, 4)
    fps = rng.randrange(3, 6, 1)
    ho = rng.randrange(128, min(168, 240) + 1, 8)
    err = int(ho / 2.0) % 8
    wo = rng.randrange(max(128, int(ho / 2.0) - err), min(168, 320, int(ho * 2.0)) + 1, 8)
    box = random_resized_crop_box(rng, 240, 320, (0.25, 1.0), wo / ho)
    flip = 1 if rng.random() < 0.5 else 0
    assert (c["out"], c["fps"], c["box"], c["geom"][9]) == ((n, ho, wo), fps, box, flip)
    assert c["indices"] == np.linspace(0, int(n * (in_fps / fps)) - 1, n, dtype=int).tolist()


def test_clip_sampling_from_config():
    from types import SimpleNamespace as NS
    cfg = NS(training=NS(sampling=NS(min_grid=[8, 128, 128], max_grid=[16, 168, 168], fps_range=[3, 5], max_aspect_ratio=2, token_range=[1, 128])),
             tokenizer=NS(model=NS(patch_size=[4, 8, 8])))
    s = ClipSampling.from_config(cfg)
    assert s == SAMPLING                                  # min_scale absent (configs/tiny.yaml): the value of tiny_csv.yaml
    with pytest.raises(ValueError):
        ClipSampling(min_grid=(8, 130, 128))


def test_float_path_against_native_uint8_path(capsys):
    """Prints (does not assert) how far torch's native uint8 antialias kernel - fixed-point weights, the intermediate image rounded
    and clamped to uint8 between the passes - is from the float path this repository implements, for INTEGRATION.md."""
    import torch.nn.functional as F
    probe = torch.zeros(1, 3, 8, 8, dtype=torch.uint8)
    try:
        F.interpolate(probe, size=(4, 4), mode="bicubic", antialias=True)
    except (RuntimeError, NotImplementedError):
        pytest.skip("this torch build has no native uint8 antialias path")
    with capsys.disabled():
        for name, frames in (("smooth", R.smooth_frames(1, 1, 256, 320)), ("noise", R.noise_frames(1, 1, 256, 320))):
            geom = R.train_geom(1, 256, 320, 152, 168)
            ref = R.levels(frames, geom)
            x = torch.from_numpy(frames).permute(0, 3, 1, 2).contiguous()
            nat = F.interpolate(x, size=(152, 168), mode="bicubic", antialias=True).permute(1, 0, 2, 3).numpy().astype(np.int64)
            d = np.abs(nat - ref)
            print(f"\nfloat path vs native uint8 path, {name} 256 x 320 -> 152 x 168: {float((d > 0).mean()):.4f} of the pixels differ, "
                  f"largest difference {int(d.max())} levels")
