"""The definition of the Y'CbCr 4:2:0 path (include/titok_hip.h) held on the CPU: the coefficient tables of tests/yuv_ref.py against
exact fractions, the closures that keep greys grey, the upsampling weights, a frame worked by hand, the integer ranges, the round trip
of every colour, and the argument checks of `video.YUV420Frames`.  No GPU."""
import os
import sys
from fractions import Fraction as Fr
from math import floor

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yuv_ref as YR  # noqa: E402

from titok_video_amd import video as V  # noqa: E402

MATRICES = {"bt601": (Fr(299, 1000), Fr(114, 1000)), "bt709": (Fr(2126, 10000), Fr(722, 10000))}
RANGES = ("limited", "full")
TABLES = [(m, r) for m in MATRICES for r in RANGES]


def half_up(x):
    return floor(x + Fr(1, 2))


@pytest.mark.parametrize("matrix,rng", TABLES)
def test_coefficients_are_the_rounded_fractions(matrix, rng):
    kr, kb = MATRICES[matrix]
    kg = 1 - kr - kb
    sy, sc = (Fr(255, 219), Fr(255, 224)) if rng == "limited" else (Fr(1), Fr(1))
    ys, cs = 1 / sy, 1 / sc
    k = YR.Coef(matrix, rng)
    assert k.y0 == (16 if rng == "limited" else 0)
    assert k.to_rgb() == (half_up(sy * 4096), half_up(2 * (1 - kr) * sc * 4096), -half_up(2 * (1 - kb) * kb / kg * sc * 4096),
                          -half_up(2 * (1 - kr) * kr / kg * sc * 4096), half_up(2 * (1 - kb) * sc * 4096))
    ytot, yr, yb = half_up(ys * 65536), half_up(kr * ys * 65536), half_up(kb * ys * 65536)
    ub = half_up(cs * 32768)
    ur, vb = -half_up(kr / (2 * (1 - kb)) * cs * 65536), -half_up(kb / (2 * (1 - kr)) * cs * 65536)
    assert k.from_rgb() == ((yr, ytot - yr - yb, yb), (ur, -(ur + ub), ub), (ub, -(ub + vb), vb))
    # the closures: the luma row sums to ytot and each chroma row to 0
    assert sum(k.from_rgb()[0]) == ytot and sum(k.from_rgb()[1]) == 0 and sum(k.from_rgb()[2]) == 0
    assert k.gu < 0 and k.gv < 0 and k.ur < 0 and k.ug < 0 and k.vg < 0 and k.vb < 0


@pytest.mark.parametrize("siting", ["left", "center"])
@pytest.mark.parametrize("matrix,rng", TABLES)
def test_every_grey_has_chroma_128(matrix, rng, siting):
    for H, W in ((4, 4), (3, 5), (1, 1)):
        g = np.arange(256, dtype=np.uint8)
        levels = np.broadcast_to(g[:, None, None, None], (256, H, W, 3))
        (y, u, v), _ = YR.planes_from_levels(levels, matrix, rng, siting)
        assert (u == 128).all() and (v == 128).all()
        assert (np.diff(y[:, 0, 0].astype(int)) >= 0).all() and (y == y[:, :1, :1]).all()


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3, 7, 8])
def test_upsampling_weights_sum_to_four_per_axis(n, center):
    """Per axis 4, so 16 per sample, for both parities and at the clamped ends; the indices stay inside the plane."""
    n_c = (n + 1) // 2
    p = np.arange(n)
    a, b, wa, wb = YR.taps(p, n_c, center)
    assert ((wa + wb) == 4).all() and (wa >= 0).all() and (wb >= 0).all()
    assert (a >= 0).all() and (b <= n_c - 1).all() and (a <= b).all()
    ones = np.ones((n_c, n_c), dtype=np.uint8)
    for siting in ("left", "center"):
        assert (YR.chroma16(ones, p, p, siting) == 16).all()


def test_a_4x4_frame_worked_by_hand():
    u = np.array([[100, 200], [50, 150]], dtype=np.uint8)
    p = np.arange(4)
    c = YR.chroma16(u, p, p, "center")
    # (0,0): both axes clamp to sample 0.  (1,1): rows 0,1 at 3,1 and columns 0,1 at 3,1.  (2,1): rows 0,1 at 1,3.  (3,3): clamped to sample (1,1).
    assert c[0, 0] == 1600 and c[1, 1] == 3 * (3 * 100 + 200) + (3 * 50 + 150) == 1800
    assert c[2, 1] == (3 * 100 + 200) + 3 * (3 * 50 + 150) == 1400 and c[3, 3] == 2400
    left = YR.chroma16(u, p, p, "left")
    # odd columns average two samples, even columns take their own; column 3 has no sample to its right
    assert left[1, 1] == 3 * (2 * 100 + 2 * 200) + (2 * 50 + 2 * 150) == 2200
    assert left[1, 2] == 3 * 4 * 200 + 4 * 150 == 3000 and left[1, 3] == 3000 and left[2, 0] == 4 * 100 + 3 * 4 * 50 == 1000
    # one pixel through to its level: BT.601 full range, Y = 100, the same plane as U and V, pixel (1, 1) under 'center'
    k = YR.Coef("bt601", "full")
    assert k.ky == 4096 and k.y0 == 0
    y = np.full((4, 4), 100, dtype=np.uint8)
    n = YR.source_n(y, u, u, [1], [1], k, "center")[0, 0]
    d = 1800 - 2048
    assert list(n) == [6553600 + k.rv * d, 6553600 + (k.gu + k.gv) * d, 6553600 + k.bu * d]
    assert list(YR.level_of_n(n)) == [(int(v) + 32768) >> 16 for v in n] and YR.level_of_n(n)[0] < 100 < YR.level_of_n(n)[1]
    assert YR.unit_from_n(np.array([0, YR.N_MAX]), "f32").tolist() == [-1.0, 1.0]


@pytest.mark.parametrize("siting", ["left", "center"])
def test_a_constant_chroma_plane_upsamples_to_16_times_the_constant(siting):
    for H, W in ((1, 1), (5, 7), (6, 8)):
        for value in (0, 1, 128, 255):
            plane = np.full(((H + 1) // 2, (W + 1) // 2), value, dtype=np.uint8)
            assert (YR.chroma16(plane, np.arange(H), np.arange(W), siting) == 16 * value).all()


@pytest.mark.parametrize("matrix,rng", TABLES)
def test_n_fits_int32_and_the_clamp_holds_it_below_2_24(matrix, rng):
    k = YR.Coef(matrix, rng)
    Y, U, Vv = np.meshgrid([0, 255], [0, 4080], [0, 4080], indexing="ij")
    raw = YR.n_unclamped(k, Y, U, Vv)
    assert np.abs(raw).max() < 2 ** 31
    # the terms of the sums as well: each product alone
    assert 16 * k.ky * 255 < 2 ** 31 and max(abs(c) for c in k.to_rgb()[1:]) * 2048 < 2 ** 31
    n = YR.n_of(k, Y, U, Vv)
    assert n.min() == 0 and n.max() == 255 * 65536 < 2 ** 24


@pytest.mark.parametrize("matrix", list(MATRICES))
def test_full_range_chroma_reaches_256_before_the_clamp(matrix):
    levels = np.array([[[[0, 0, 255]]], [[[255, 0, 0]]]], dtype=np.uint8)         # blue, red: frames of 1 x 1
    for siting in ("left", "center"):
        (y, u, v), (u_raw, v_raw) = YR.planes_from_levels(levels, matrix, "full", siting)
        assert u_raw[0, 0, 0] == 256 and v_raw[1, 0, 0] == 256
        assert u[0, 0, 0] == 255 and v[1, 0, 0] == 255


@pytest.mark.parametrize("matrix,rng", TABLES)
def test_round_trip_of_all_colours(matrix, rng):
    """Every (R, G, B) as a constant frame: levels -> planes -> source level.  A constant frame's chroma sample is that of one pixel and
    upsamples to 16 x itself (tested above), so a frame of 1 x 1 per colour stands for any size."""
    k = YR.Coef(matrix, rng)
    g, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    worst, worst_grey = 0, 0
    for r in range(256):
        levels = np.stack([np.full(65536, r), g.reshape(-1), b.reshape(-1)], axis=-1).astype(np.uint8).reshape(65536, 1, 1, 3)
        (y, u, v), _ = YR.planes_from_levels(levels, matrix, rng, "left")
        back = YR.level_of_n(YR.n_of(k, y.reshape(-1), 16 * u.reshape(-1).astype(np.int64), 16 * v.reshape(-1).astype(np.int64)))
        err = np.abs(back - levels.reshape(65536, 3).astype(np.int64))
        worst = max(worst, int(err.max()))
        worst_grey = max(worst_grey, int(err[r * 256 + r].max()))
    print(f"{matrix} {rng}: worst error {worst} levels, greys {worst_grey}")
    assert worst <= (2 if rng == "limited" else 1)
    assert worst_grey <= (1 if rng == "limited" else 0)


# ---- YUV420Frames: argument checks (host tensors: what is checked before the device) -----------------------------------------------------
def planes(T=2, H=5, W=7):
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    z = lambda *s: torch.zeros(s, dtype=torch.uint8)  # noqa: E731
    return z(T, H, W), z(T, Hc, Wc), z(T, Hc, Wc), z(T, Hc, Wc, 2)


def test_yuv420frames_refuses_bad_arguments():
    y, u, v, uv = planes()
    bad = [
        dict(y=y), dict(y=y, u=u), dict(y=y, u=u, v=v, uv=uv), dict(y=y, uv=uv, vu=uv),                   # which chroma
        dict(y=y, u=u, v=v, matrix="bt2020"), dict(y=y, u=u, v=v, range="tv"), dict(y=y, u=u, v=v, siting="top"),
        dict(y=y.float(), u=u, v=v), dict(y=y[0], u=u, v=v), dict(y=y, u=u.to(torch.int8), v=v),          # dtypes, ranks
        dict(y=y, u=u[:, :2], v=v), dict(y=y, u=u, v=v[:, :, :3]), dict(y=y, uv=uv[:, :, :3]), dict(y=y, uv=uv[..., :1]),
        dict(y=y.transpose(1, 2).contiguous().transpose(1, 2), u=u, v=v),                                 # luma columns not adjacent
        dict(y=y, u=torch.zeros((2, 3, 8), dtype=torch.uint8)[:, :, ::2], v=v),                           # chroma columns not adjacent
        dict(y=y, u=u, v=torch.zeros((2, 3, 6), dtype=torch.uint8)[:, :, :4]),                            # u and v pitched differently
        dict(y=y, vu=torch.zeros((2, 3, 4, 4), dtype=torch.uint8)[..., :2]),                              # pairs 4 bytes apart
        dict(y=y[:1].expand(2, 5, 7), u=u, v=v),                                                          # frames on top of each other
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            V.YUV420Frames(**kw)
    # everything in order but on the host: there is no CPU path
    for kw in (dict(u=u, v=v), dict(uv=uv), dict(vu=uv)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            V.YUV420Frames(y, **kw)
    with pytest.raises(ValueError):
        V.YUV420Frames.empty(2, 4, 4, layout="yv12", device="cpu")
    with pytest.raises(ValueError):
        V.YUV420Frames.empty(2, 0, 4, device="cpu")


def test_yuv420frames_accepts_pitched_views_up_to_the_device_check():
    """A decoder surface: rows of 16 bytes holding 7, frames of 8 rows holding 5, NV12 chroma below the luma.  Only the device is wrong."""
    surface = torch.zeros((2, 12, 16), dtype=torch.uint8)
    y, uv = surface[:, :5, :7], surface[:, 8:11, :8].unflatten(2, (4, 2))
    assert uv.shape == (2, 3, 4, 2) and uv.stride() == (192, 16, 2, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        V.YUV420Frames(y, uv=uv)
