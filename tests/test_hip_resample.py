"""ttv_clip_resample_u8 (crop box + antialiased bicubic resize + flip + normalisation, one launch per batch) on the MI355X, through
the C ABI, against the float64 restatement of tests/resample_ref.py; then `data.resample_clip` and `ShardBatchLoader(sampling=...)`.

THE RULE of every comparison (`check_clip`).  The kernel stores level / 127.5 - 1 of an integer level 0 .. 255; levels are decoded
from the output (`round((out + 1) * 127.5)`, exact in both dtypes) and compared with the restatement's:
  * a decoded level may differ from the restatement's only by one,
  * and only at pixels whose float64 pre-rounding value lies within `tau` of a half-integer, where tau = 4 * max |torch-CPU fp32
    F.interpolate(antialias=True) - float64| on that same case: four times the error aten's own fp32 kernel shows there.  tau
    comes from torch on the CPU, never from the kernel under test;
  * the share of differing pixels per case is at most 2e-3: four times the worst share torch's own fp32 path shows against float64
    on uniform noise (5.0e-4 over six shapes between 130 x 150 and 360 x 640 going to 128 .. 168).  Noise is the worst content
    for ties (bicubic overshoot everywhere, no flat regions), so every case here is noise;
  * everywhere else the output is bit-equal to the restated normalisation of the restatement's level in the clip's dtype (and at
    the differing pixels to the normalisation of the level it decoded to).
"""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref as R  # noqa: E402

from titok_video_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"bf16": torch.bfloat16, "f32": torch.float32}
SHARE_CAP = 2e-3
GUARD = 256            # elements before and after every destination
SRC_FRONT = 19         # poisoned bytes before every source: its first byte sits at an odd address
SRC_TAIL = 64          # poisoned bytes behind every source


def L():
    return _lib.lib()


def S():
    return _lib.stream_ptr(torch.device(DEV))


# (name, geometry).  The kernel's output tile is 16 rows x 64 columns and a thread stores 4 columns: Wo in {64, 128} sits on the
# tile, 72 / 100 / 80 are multiples of 4 off it, 70 / 93 / 125 are not multiples of 4; Ho likewise around 16.
SINGLE_CASES = [
    ("down_2x", R.train_geom(2, 128, 144, 64, 72)),
    ("down_1.37x_by_1.61x", R.train_geom(2, 175, 206, 128, 128)),
    ("down_3.9x", R.train_geom(2, 312, 390, 80, 100)),
    ("up_1.25x", R.train_geom(2, 80, 100, 100, 125)),
    ("up_2x", R.train_geom(2, 40, 50, 80, 100)),
    ("identity", R.train_geom(2, 64, 72, 64, 72)),
    ("eval_window", R.eval_geom(2, 150, 233, 96, 128)),
    ("flip_odd_ws", R.train_geom(2, 90, 131, 66, 93, flip=1)),
    ("flip_down_2x", R.train_geom(2, 100, 144, 50, 72, flip=1)),
    ("off_tile_both", R.train_geom(2, 77, 91, 50, 70)),
    ("t1", R.train_geom(1, 77, 91, 33, 41)),
    ("t16", R.train_geom(16, 96, 120, 64, 80)),
]


def mixed_cases(n=64, seed=7):
    rng, out = random.Random(seed), []
    for i in range(n):
        t = rng.choice([1, 2, 4])
        hs, ws = rng.randrange(20, 91), rng.randrange(20, 91)
        ho, wo = rng.randrange(16, 73), rng.randrange(16, 73)
        if i % 3 == 2 and ho <= hs and wo <= ws:
            g = R.eval_geom(t, hs, ws, ho, wo)
        else:
            g = R.train_geom(t, hs, ws, ho, wo, flip=rng.randrange(2))
        out.append((f"mixed_{i}", g))
    return out


def run_call(frames_list, geoms, dt, poison=0xA5, expect_rc=0):
    """One ttv_clip_resample_u8 call.  Every source lies in its own buffer between poisoned bytes, every destination between guard
    bands.  Returns the outputs (CPU, float32 view of the stored values) after checking that the bands are untouched."""
    srcs, bufs, dsts = [], [], []
    for f, g in zip(frames_list, geoms):
        n = f.size
        host = np.full(SRC_FRONT + n + SRC_TAIL, poison, dtype=np.uint8)
        host[SRC_FRONT:SRC_FRONT + n] = f.reshape(-1)
        buf = torch.from_numpy(host).to(DEV)
        bufs.append(buf)
        srcs.append(buf[SRC_FRONT:SRC_FRONT + n])
        n_out = 3 * g[0] * g[7] * g[8]
        d = torch.full((GUARD + n_out + GUARD,), 7.0, dtype=DT[dt], device=DEV)
        dsts.append(d)
    flat = [int(v) for g in geoms for v in g]
    arr = (_lib.i32 * len(flat))(*flat)
    dst_views = [d[GUARD:GUARD + 3 * g[0] * g[7] * g[8]] for d, g in zip(dsts, geoms)]
    rc = L().ttv_clip_resample_u8(_lib.ptr_array(srcs), _lib.ptr_array(dst_views), arr, len(geoms), _lib.dtype_code(DT[dt]), S())
    torch.cuda.synchronize()
    assert rc == expect_rc, L().ttv_error_string()
    outs = []
    for d, g in zip(dsts, geoms):
        h = d.float().cpu().numpy()
        n_out = 3 * g[0] * g[7] * g[8]
        assert (h[:GUARD] == 7.0).all() and (h[GUARD + n_out:] == 7.0).all(), "written outside the destination"
        outs.append(h[GUARD:GUARD + n_out].reshape(3, g[0], g[7], g[8]))
    return outs


def check_clip(name, dt, out, frames, geom):
    """THE RULE of the module docstring for one clip; prints the figures before it asserts."""
    pre = R.prerounding(frames, geom)
    ref = np.clip(np.rint(pre), 0, 255).astype(np.int64)
    tau = 4.0 * float(np.abs(R.torch_float_path(frames, geom).astype(np.float64) - pre).max())
    dec = R.decode_levels(out)
    diff = dec != ref
    share = float(diff.mean())
    worst_tie = float(R.tie_distance(pre)[diff].max()) if diff.any() else 0.0
    print(f"{name} {dt}: geom {tuple(geom)} tau {tau:.3e}  differing levels {int(diff.sum())} of {diff.size} (share {share:.2e}), "
          f"largest step {int(np.abs(dec - ref).max())}, largest tie distance among them {worst_tie:.3e}")
    assert np.abs(dec - ref).max() <= 1, f"{name}: a level is off by more than one"
    assert worst_tie <= tau, f"{name}: a level differs {worst_tie:.3e} away from a half-integer, tau = {tau:.3e}"
    assert share <= SHARE_CAP, f"{name}: {share:.2e} of the levels differ"
    assert np.array_equal(out, R.normalise(dec, dt)), f"{name}: output is not the normalisation of a level"


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("case", SINGLE_CASES, ids=[c[0] for c in SINGLE_CASES])
def test_levels_against_float64(case, dt):
    name, geom = case
    frames = R.noise_frames(sum(geom), *geom[:3])
    out, = run_call([frames], [geom], dt)
    check_clip(name, dt, out, frames, geom)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_64_mixed_clips_in_one_call(dt):
    cases = mixed_cases()
    assert len(cases) == _lib.TTV_MAX_CLIPS_PER_LAUNCH
    frames = [R.noise_frames(1000 + i, *g[:3]) for i, (_n, g) in enumerate(cases)]
    outs = run_call(frames, [g for _n, g in cases], dt)
    for (name, g), f, o in zip(cases, frames, outs):
        check_clip(name, dt, o, f, g)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_result_does_not_depend_on_what_surrounds_the_source(dt):
    """The bytes before and behind each source array are poisoned with two different values: a read outside the array that
    reaches a result would show as a difference."""
    cases = [c for c in SINGLE_CASES if c[0] in ("down_2x", "flip_odd_ws", "eval_window", "off_tile_both", "t1")]
    frames = [R.noise_frames(sum(g), *g[:3]) for _n, g in cases]
    a = run_call(frames, [g for _n, g in cases], dt, poison=0x00)
    b = run_call(frames, [g for _n, g in cases], dt, poison=0xFF)
    for (name, _g), x, y in zip(cases, a, b):
        assert np.array_equal(x, y), name


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_identity_geometry_equals_clip_from_u8(dt):
    for t, h, w in [(2, 64, 72), (4, 16, 16), (1, 50, 70)]:
        frames = R.noise_frames(t * h + w, t, h, w)
        frames.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
        out, = run_call([frames], [R.train_geom(t, h, w, h, w)], dt)
        d8 = torch.from_numpy(frames).to(DEV)
        ref = torch.empty((3, t, h, w), dtype=DT[dt], device=DEV)
        _lib.check(L().ttv_clip_from_u8(d8.data_ptr(), t, h, w, ref.data_ptr(), _lib.dtype_code(DT[dt]), S()), "clip_from_u8")
        assert np.array_equal(out, ref.float().cpu().numpy()), (t, h, w)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("level", [0, 1, 127, 128, 254, 255])
def test_constant_frames_keep_their_level(level, dt):
    """Normalised weights sum to 1: a flat frame stays flat, exactly, through every geometry (also the clamps at 0 and 255)."""
    cases = SINGLE_CASES + mixed_cases(16, seed=3)
    geoms = [g for _n, g in cases]
    frames = [np.full((g[0], g[1], g[2], 3), level, dtype=np.uint8) for g in geoms]
    outs = run_call(frames, geoms, dt)
    want = R.normalise(np.array(level), dt)
    for (name, _g), o in zip(cases, outs):
        assert (o == want).all(), f"{name}: level {level} became {np.unique(R.decode_levels(o))}"


def test_argument_errors_launch_nothing():
    g = R.train_geom(1, 32, 32, 16, 16)
    f = R.noise_frames(0, 1, 32, 32)
    src = torch.from_numpy(f).to(DEV)
    dst = torch.full((3 * 16 * 16 + 8,), 7.0, dtype=torch.float32, device=DEV)

    def call(geoms, n=None, dtype=_lib.TTV_F32, dst_off=0, refused=True):
        n = len(geoms) if n is None else n
        flat = [int(v) for gg in geoms for v in gg]
        arr = (_lib.i32 * len(flat))(*flat)
        rc = L().ttv_clip_resample_u8(_lib.ptr_array([src] * len(geoms)), _lib.ptr_array([dst[dst_off:]] * len(geoms)), arr, n, dtype, S())
        msg = L().ttv_error_string().decode()
        torch.cuda.synchronize()
        assert not refused or (dst == 7.0).all(), "a refused call wrote to its destination"
        return rc, msg

    rc, msg = call([g] * 65)
    assert rc == 1 and "65" in msg and "clips" in msg
    rc, msg = call([(1, 32, 32, 3, 16, 0, 0, 3, 16, 0)])                 # 32 -> 3 rows: scale 10.7
    assert rc == 1 and "scale" in msg
    rc, msg = call([(1, 32, 32, 16, 16, 1, 0, 16, 16, 0)])               # window rows 1 .. 17 of 16
    assert rc == 1 and "window" in msg
    rc, msg = call([(1, 32, 32, 16, 16, 0, 4, 16, 13, 0)])               # window columns 4 .. 17 of 16
    assert rc == 1 and "window" in msg
    rc, msg = call([g], dst_off=1)                                       # 4 bytes off a 16-byte boundary
    assert rc == 1 and "aligned" in msg
    rc, msg = call([g], dtype=7)
    assert rc == 1 and "dtype" in msg
    rc, msg = call([g], refused=False)                                   # and the same arguments, in order, are accepted
    assert rc == 0 and not (dst[:3 * 16 * 16] == 7.0).any() and (dst[3 * 16 * 16:] == 7.0).all()


# ------------------------------------------------------------------------------------- resample_clip and the loader, end to end
def test_resample_clip_wrapper():
    from titok_video_amd.data import resample_clip
    frames = R.noise_frames(5, 4, 90, 131)
    d = torch.from_numpy(frames).to(DEV)
    box = (7, 20, 66, 99)
    crop = np.ascontiguousarray(frames[:, 7:73, 20:119])
    for dt in ("bf16", "f32"):
        out = resample_clip(d, (48, 72), box=box, flip=True, dtype=DT[dt])
        torch.cuda.synchronize()
        assert out.shape == (3, 4, 48, 72) and out.dtype == DT[dt]
        check_clip("resample_clip train", dt, out.float().cpu().numpy(), crop, R.train_geom(4, 66, 99, 48, 72, flip=1))
        out = resample_clip(d, (48, 72), eval=True, dtype=DT[dt])
        torch.cuda.synchronize()
        check_clip("resample_clip eval", dt, out.float().cpu().numpy(), frames, R.eval_geom(4, 90, 131, 48, 72))
    with pytest.raises(RuntimeError, match="no CPU path"):
        resample_clip(torch.from_numpy(frames), (48, 72))
    with pytest.raises(ValueError):
        resample_clip(d, (48, 72), box=(0, 0, 91, 10))


SAMPLING_KW = dict(min_grid=(8, 128, 128), max_grid=(16, 168, 168), fps_range=(3, 5), max_aspect_ratio=2.0, min_scale=0.25, patch_size=(4, 8, 8))
SEQ_LEN = 6144
N_BATCHES = 2


def _loader_child(paths, eval_mode, dt, q):
    """Fresh process (the loader forks its workers before the first GPU call): a host-side run (crop boxes + geometry), two device
    runs with the same seed, and one TiTok forward on the first device batch."""
    try:
        from types import SimpleNamespace
        from titok_video_amd.data import ClipSampling
        from titok_video_amd.loader import ShardBatchLoader
        kw = dict(patch=(4, 8, 8), token_range=(1, 128), seq_len=SEQ_LEN, seed=3, workers=2, epochs=1, drop_last=False,
                  sampling=ClipSampling(**SAMPLING_KW), eval=eval_mode)
        host, dev1, dev2 = (ShardBatchLoader(paths, **kw).start() for _ in range(3))
        assert host.workers == 2
        raw = []
        for b in host.raw_batches():
            raw.append({"frames": [f.numpy() for f in b["frames"]], "geom": b["geom"], "__key__": b["__key__"], "fps": b["fps"],
                        "token_counts": b["token_counts"]})
            if len(raw) == N_BATCHES:
                break
        host.close()
        runs = []
        first = None
        for ld in (dev1, dev2):
            got = []
            for b in ld.batches(DEV, DT[dt]):
                if first is None:
                    first = b
                got.append({"video": [c.float().cpu().numpy() for c in b["video"]], "geom": b["geom"], "__key__": b["__key__"],
                            "fps": b["fps"], "token_counts": b["token_counts"].tolist(), "dtypes": {str(c.dtype) for c in b["video"]}})
                if len(got) == N_BATCHES:
                    break
            runs.append(got)
            ld.close()
        from titok_video_amd.model.titok import TiTok
        from titok_video_amd.synthetic import seeded_titok_state
        cfg = SimpleNamespace(tokenizer=SimpleNamespace(model=SimpleNamespace(
            patch_size=[4, 8, 8], fsq_levels=[7, 5, 5, 5, 5], encoder_size="tiny", decoder_size="tiny")))
        model = TiTok(cfg)
        model.load_state_dict(seeded_titok_state(0), strict=True)
        model = model.to(DEV, DT[dt]).eval()
        with torch.no_grad():
            recon, out = model(first["video"], first["token_counts"].tolist())
        torch.cuda.synchronize()
        fwd = {"shapes": [tuple(r.shape) for r in recon], "finite": all(bool(torch.isfinite(r.float()).all()) for r in recon),
               "n_idx": int(out["indices"].numel())}
        q.put(("ok", raw, runs, fwd, dev1.skipped))
    except BaseException:
        import traceback
        q.put(("error", traceback.format_exc()))


@pytest.mark.parametrize("eval_mode,dt", [(False, "bf16"), (True, "f32")], ids=["train-bf16", "eval-f32"])
def test_loader_with_sampling_end_to_end(tmp_path, eval_mode, dt):
    import torch.multiprocessing as mp
    from titok_video_amd.shards import write_synthetic_video_shards
    paths = write_synthetic_video_shards(str(tmp_path), 2, 8, seed=2)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_loader_child, args=(paths, eval_mode, dt, q))
    p.start()
    res = q.get(timeout=300)
    p.join(timeout=60)
    assert res[0] == "ok", res[1]
    _ok, raw, runs, fwd, skipped = res
    assert skipped == 0 and len(raw) == N_BATCHES and len(runs[0]) == N_BATCHES and len(runs[1]) == N_BATCHES
    for hb, b1, b2 in zip(raw, runs[0], runs[1]):
        assert hb["geom"] == b1["geom"] == b2["geom"] and hb["__key__"] == b1["__key__"] == b2["__key__"]
        assert hb["token_counts"] == b1["token_counts"] and hb["fps"] == b1["fps"]
        assert b1["dtypes"] == {str(DT[dt])}
        packed = 0
        for k, (frames, geom, clip, again) in enumerate(zip(hb["frames"], hb["geom"], b1["video"], b2["video"])):
            t, ho, wo = geom[0], geom[7], geom[8]
            assert clip.shape == (3, t, ho, wo) and frames.shape == (t, geom[1], geom[2], 3)
            assert t % 4 == 0 and ho % 8 == 0 and wo % 8 == 0 and 8 <= t <= 16 and 128 <= ho <= 168 and 128 <= wo <= 168
            packed += (t // 4) * (ho // 8) * (wo // 8) + b1["token_counts"][k]
            assert np.array_equal(clip, again), "two runs with the same seed differ"
            check_clip(f"loader {hb['__key__'][k]}", dt, clip, np.ascontiguousarray(frames), geom)
        assert packed <= SEQ_LEN
    if not eval_mode:
        flips = [g[9] for hb in raw for g in hb["geom"]]
        assert 0 in flips and 1 in flips
    else:
        assert all(g[9] == 0 for hb in raw for g in hb["geom"]) and any(g[5] or g[6] for hb in raw for g in hb["geom"])
    assert fwd["finite"] and fwd["shapes"] == [c.shape for c in runs[0][0]["video"]] and fwd["n_idx"] == sum(runs[0][0]["token_counts"])


def _plain_loader_child(paths, dt, q):
    try:
        from titok_video_amd.loader import ShardBatchLoader
        ld = ShardBatchLoader(paths, patch=(4, 8, 8), token_range=(1, 16), seq_len=160, seed=1, workers=2, epochs=1, drop_last=False).start()
        out = {}
        for b in ld.batches(DEV, DT[dt]):
            assert "geom" not in b
            for k, c in zip(b["__key__"], b["video"]):
                out[k] = c.float().cpu().numpy()
        ld.close()
        q.put(("ok", out))
    except BaseException:
        import traceback
        q.put(("error", traceback.format_exc()))


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_loader_without_sampling_is_unchanged(tmp_path, dt):
    """Without `sampling=` the loader yields the clips the host-side reader computes (shards.shard_samples: u8 / 127.5 - 1 in torch),
    bit for bit: the path the parent commit has."""
    import torch.multiprocessing as mp
    from titok_video_amd.shards import shard_samples, write_synthetic_shards
    paths = write_synthetic_shards(str(tmp_path), 2, 4, min_grid=(4, 16, 16), max_grid=(8, 32, 32), seed=5)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_plain_loader_child, args=(paths, dt, q))
    p.start()
    res = q.get(timeout=300)
    p.join(timeout=60)
    assert res[0] == "ok", res[1]
    want = {s["__key__"]: s["video"].float().numpy() for s in shard_samples(paths, dtype=DT[dt])}
    assert set(res[1]) == set(want) and len(want) == 8
    for k, v in want.items():
        assert np.array_equal(res[1][k], v), k
