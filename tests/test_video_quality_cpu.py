"""Per-frame quality of whole videos without a GPU: the numpy restatement (tests/quality_ref.py) pinned by hand and against
independent formulations, the arithmetic of `video.VideoQuality` on injected sums, every Python ValueError, and every refusal of
the C entry points, which return before anything touches the GPU."""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import pytest
import torch
from scipy.ndimage import correlate1d

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quality_ref as QR  # noqa: E402
from test_ssim_cpu import gaussian_taps  # noqa: E402

from titok_video_amd import _lib  # noqa: E402
from titok_video_amd import video as V  # noqa: E402


# ---- the restatement: squared error ----------------------------------------------------------------------------------------------------
def test_sse_by_hand_on_a_2x2_rgb_frame():
    a = np.array([[[[0, 10, 255], [3, 3, 3]], [[7, 0, 100], [255, 255, 0]]]], dtype=np.uint8)
    b = np.array([[[[255, 10, 0], [0, 4, 3]], [[7, 2, 90], [254, 0, 0]]]], dtype=np.uint8)
    # R: 255^2 + 3^2 + 0 + 1 ; G: 0 + 1 + 2^2 + 255^2 ; B: 255^2 + 0 + 10^2 + 0
    assert QR.sse_rgb(a, b) == [[65025 + 9 + 1, 1 + 4 + 65025, 65025 + 100]]
    two = np.concatenate([b, a, b])
    assert QR.sse_rgb(np.concatenate([a, a]), two, b_stride=1) == [[65035, 65030, 65125], [0, 0, 0]]
    assert QR.sse_rgb(np.concatenate([a, a]), two, b_stride=2) == [[65035, 65030, 65125], [65035, 65030, 65125]]


def test_sse_by_hand_on_a_4x4_420_frame():
    ya, yb = np.zeros((1, 4, 4), np.uint8), np.zeros((1, 4, 4), np.uint8)
    ya[0, 0, 0], ya[0, 3, 3], yb[0, 3, 3], yb[0, 1, 2] = 200, 5, 9, 1
    ua, ub = np.array([[[1, 2], [3, 4]]], np.uint8), np.array([[[4, 2], [3, 0]]], np.uint8)
    va, vb = np.full((1, 2, 2), 128, np.uint8), np.full((1, 2, 2), 126, np.uint8)
    assert QR.sse_planes((ya, ua, va), (yb, ub, vb)) == [[200 * 200 + 16 + 1, 9 + 16, 4 * 4]]


def test_a_264x256_frame_of_0_against_255_is_beyond_32_bits():
    """The condition the GPU overflow case rests on: one component of one frame pair exceeds what a 32-bit sum holds."""
    a, b = np.zeros((1, 264, 256, 3), np.uint8), np.full((1, 264, 256, 3), 255, np.uint8)
    want = 67584 * 65025
    assert want > 1 << 32
    assert QR.sse_rgb(a, b) == [[want, want, want]]


# ---- the restatement: SSIM -------------------------------------------------------------------------------------------------------------
def test_taps_are_the_evaluation_loops():
    np.testing.assert_allclose(QR.gaussian_taps(), gaussian_taps().numpy(), rtol=0, atol=1e-16)      # two exp() implementations
    assert abs(QR.gaussian_taps().sum() - 1) < 1e-15


def _separable(a, b):
    x, y, g = a.astype(np.float64), b.astype(np.float64), QR.gaussian_taps()

    def filt(p):
        return correlate1d(correlate1d(p, g, axis=1, mode="constant"), g, axis=0, mode="constant")[5:-5, 5:-5]

    mx, my, exx, eyy, exy = (filt(p) for p in (x, y, x * x, y * y, x * y))
    sxx, syy, sxy = np.maximum(exx - mx * mx, 0), np.maximum(eyy - my * my, 0), exy - mx * my
    return float((((2 * mx * my + QR.C1) * (2 * sxy + QR.C2)) / ((mx * mx + my * my + QR.C1) * (sxx + syy + QR.C2))).mean())


def test_ssim_matches_a_separable_filter():
    rng = np.random.default_rng(5)
    for shape in [(11, 11), (12, 43), (43, 44), (23, 17)]:
        a = rng.integers(0, 256, shape, dtype=np.uint8)
        b = np.clip(a.astype(np.int64) + rng.integers(-40, 41, shape), 0, 255).astype(np.uint8)
        assert abs(QR.plane_ssim(a, b) - _separable(a, b)) < 1e-12


@pytest.mark.parametrize("a,b", [(0, 255), (255, 255), (17, 200), (128, 127), (0, 0)])
def test_ssim_of_constant_planes_is_the_closed_form(a, b):
    want = (2 * a * b + QR.C1) / (a * a + b * b + QR.C1)
    got = QR.plane_ssim(np.full((14, 19), a, np.uint8), np.full((14, 19), b, np.uint8))
    assert abs(got - want) < 1e-12


def test_ssim_of_one_window_summed_by_hand():
    rng = np.random.default_rng(9)
    a, b = rng.integers(0, 256, (11, 11), dtype=np.uint8), rng.integers(0, 256, (11, 11), dtype=np.uint8)
    g = QR.gaussian_taps()
    mx = my = exx = eyy = exy = 0.0
    for i in range(11):
        for j in range(11):
            wgt, x, y = g[i] * g[j], float(a[i, j]), float(b[i, j])
            mx, my, exx, eyy, exy = mx + wgt * x, my + wgt * y, exx + wgt * x * x, eyy + wgt * y * y, exy + wgt * x * y
    sxx, syy, sxy = max(exx - mx * mx, 0.0), max(eyy - my * my, 0.0), exy - mx * my
    want = ((2 * mx * my + QR.C1) * (2 * sxy + QR.C2)) / ((mx * mx + my * my + QR.C1) * (sxx + syy + QR.C2))
    assert abs(QR.plane_ssim(a, b) - want) < 1e-12
    assert QR.ssim_rgb(np.stack([a, a, b], -1)[None], np.stack([b, a, b], -1)[None]).shape == (1, 3)


# ---- VideoQuality on injected sums ------------------------------------------------------------------------------------------------------
def injected(yuv):
    q = V.VideoQuality(4, 6, yuv420=yuv)
    q.t0 = 3
    q.sse = [[24, 0, 6], [240, 12, 6], [240, 0, 0]]
    q.ssim = [[0.5, 1.0, 0.25], [0.25, 1.0, 0.75], [0.75, 1.0, 0.5]]
    return q


def test_components_and_elements():
    rgb, yuv = V.VideoQuality(5, 7), V.VideoQuality(5, 7, yuv420=True)
    assert rgb.components == ("r", "g", "b") and rgb.elements == (35, 35, 35)
    assert yuv.components == ("y", "u", "v") and yuv.elements == (35, 12, 12)
    with pytest.raises(ValueError):
        rgb.psnr()                                              # nothing finished
    with pytest.raises(ValueError):
        rgb.finish()                                            # nothing measured
    with pytest.raises(ValueError):
        V.VideoQuality(0, 7)


def test_psnr_per_frame_overall_and_pooled():
    q = injected(False)
    db = lambda sse, n: 10 * math.log10(65025 * n / sse)        # noqa: E731
    p = q.psnr()
    assert p[0] == [db(24, 24), math.inf, db(6, 24)] and p[1] == [db(240, 24), db(12, 24), db(6, 24)] and p[2][1:] == [math.inf, math.inf]
    assert q.psnr_overall() == [db(504, 72), db(12, 72), db(12, 72)]
    assert q.psnr_pooled() == db(528, 216)
    assert q.ssim_mean() == [0.5, 1.0, 0.5]
    q.sse = [[0, 0, 0]]
    assert q.psnr_pooled() == math.inf and q.psnr_overall() == [math.inf] * 3


def test_pooled_psnr_of_420_weights_y_u_v_as_4_1_1():
    q = injected(True)
    assert q.elements == (24, 6, 6)
    assert q.psnr_pooled() == 10 * math.log10(65025 * 3 * 36 / 528)
    # the same mean squared error in every plane: the pooled value is that of any plane, and the weights of the planes' mean squared
    # errors are their sample counts, 4 : 1 : 1
    q.sse = [[4 * 50, 50, 50]]
    assert q.psnr_pooled() == pytest.approx(q.psnr()[0][0]) and q.psnr()[0][0] == pytest.approx(q.psnr()[0][1])
    mse = [200 / 24, 10 / 6, 70 / 6]
    q.sse = [[200, 10, 70]]
    assert q.psnr_pooled() == pytest.approx(10 * math.log10(65025 / ((4 * mse[0] + mse[1] + mse[2]) / 6)))


def test_worst_frame_and_as_dict():
    q = injected(False)
    assert q.worst_frame() == 4 and q.worst_frame(1) == 4 and q.worst_frame(2) == 3       # the first of equals, on the timeline
    d = json.loads(json.dumps(q.as_dict()))
    assert d["components"] == ["r", "g", "b"] and d["elements"] == [24, 24, 24] and d["t0"] == 3 and d["frames"] == 3
    assert d["sse"] == q.sse and d["ssim"] == q.ssim and d["psnr"][0][1] is None and d["psnr"][1][1] == q.psnr()[1][1]
    assert d["psnr_pooled"] == q.psnr_pooled() and d["ssim_mean"] == [0.5, 1.0, 0.5] and d["worst_frame"] == [4, 4, 3]
    q.ssim = None
    assert q.ssim_mean() is None and json.loads(json.dumps(q.as_dict()))["ssim"] is None


# ---- Python refusals -----------------------------------------------------------------------------------------------------------------------
def fake_yuv(T, H, W, **kw):
    """A YUV420Frames whose planes are host tensors (the constructor refuses those): enough for the checks that come before the GPU."""
    f = object.__new__(V.YUV420Frames)
    f.__dict__.update(dict(y=torch.zeros((T, H, W), dtype=torch.uint8), shape=(T, H, W), matrix="bt709", range="limited", siting="left",
                           layout="i420", device=torch.device("cpu")))
    f.__dict__.update(kw)
    return f


@pytest.mark.parametrize("fn", [V.frame_sse, V.frame_ssim])
def test_frame_functions_raise_value_errors(fn):
    rgb = torch.zeros((3, 24, 32, 3), dtype=torch.uint8)
    for a, b, stride in [(rgb, fake_yuv(3, 24, 32), 1), (fake_yuv(3, 24, 32), rgb, 1),                    # mixed kinds
                         (rgb, torch.zeros((3, 24, 30, 3), dtype=torch.uint8), 1),                       # different H x W
                         (rgb, torch.zeros((3, 26, 32, 3), dtype=torch.uint8), 1),
                         (fake_yuv(3, 24, 32), fake_yuv(3, 24, 34), 1),
                         (rgb, torch.zeros((4, 24, 32, 3), dtype=torch.uint8), 2),                       # b too short: 5 frames needed
                         (fake_yuv(2, 24, 32), fake_yuv(3, 24, 32), 3),
                         (rgb, rgb, 0),                                                                  # b_stride
                         (fake_yuv(1, 24, 32), fake_yuv(1, 24, 32, matrix="bt601"), 1),                  # colour descriptions
                         (fake_yuv(1, 24, 32), fake_yuv(1, 24, 32, range="full"), 1),
                         (fake_yuv(1, 24, 32), fake_yuv(1, 24, 32, siting="center"), 1),
                         (rgb.float(), rgb, 1), (rgb, rgb[..., :2], 1), (rgb[:, :, ::2], rgb[:, :, ::2], 1)]:  # dtype, shape, layout
        with pytest.raises(ValueError):
            fn(a, b, stride)
    with pytest.raises(RuntimeError, match="no CPU path"):                                               # host tensors, as everywhere
        fn(rgb, rgb)


def test_frame_ssim_needs_whole_windows():
    with pytest.raises(ValueError, match="at least 11"):
        V.frame_ssim(torch.zeros((1, 10, 32, 3), dtype=torch.uint8), torch.zeros((1, 10, 32, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="at least 21"):
        V.frame_ssim(fake_yuv(1, 32, 20), fake_yuv(1, 32, 20))


def test_update_raises_value_errors():
    q = V.VideoQuality(24, 32)
    rgb = torch.zeros((4, 24, 32, 3), dtype=torch.uint8)
    for dec, src, t0, stride in [(rgb, fake_yuv(4, 24, 32), 0, 1), (rgb, torch.zeros((4, 24, 30, 3), dtype=torch.uint8), 0, 1),
                                 (rgb, rgb, 4, 1), (rgb, rgb, 2, 2), (rgb, rgb, -1, 1), (rgb, rgb, 0, 0), (rgb, rgb, 2, 1), (rgb, "frames", 0, 1)]:
        with pytest.raises(ValueError):
            q.update(dec, src, t0, stride)
    with pytest.raises(ValueError):
        V.VideoQuality(24, 32, yuv420=True).update(fake_yuv(4, 24, 32), rgb, 0)


# ---- C refusals ------------------------------------------------------------------------------------------------------------------------------
def desc(H, W, step=1, **kw):
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    d = dict(y=1 << 20, u=2 << 20, v=(2 << 20) + 1 if step == 2 else 3 << 20, y_frame=H * W, c_frame=Hc * Wc * step, y_pitch=W,
             c_pitch=Wc * step, c_step=step, matrix=1, range=0, siting=0)
    d.update(kw)
    return _lib.Yuv420(**d)


def test_cabi_refuses_bad_arguments_without_touching_the_gpu():
    h = _lib.lib()
    A, B, OUT, WORK = C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20), C.c_void_p(4 << 20)
    big = 1 << 30

    def rgb(fn, a=A, b=B, n=2, stride=1, H=24, W=32, out=OUT, work=WORK, nbytes=big):
        if fn == "sse":
            return h.ttv_video_frame_sse_u8(a, b, n, stride, H, W, out, None)
        return h.ttv_video_frame_ssim_u8(a, b, n, stride, H, W, out, work, nbytes, None)

    def yuv(fn, a=None, b=None, n=2, stride=1, H=24, W=32, out=OUT, work=WORK, nbytes=big, null_a=False, null_b=False):
        a = desc(H, W) if a is None else a
        b = desc(H, W, 2) if b is None else b
        pa, pb = (None if null_a else C.byref(a)), (None if null_b else C.byref(b))
        if fn == "sse":
            return h.ttv_video_frame_sse_yuv420(pa, pb, n, stride, H, W, out, None)
        return h.ttv_video_frame_ssim_yuv420(pa, pb, n, stride, H, W, out, work, nbytes, None)

    def refused(rc, word):
        assert rc == 1 and word in h.ttv_error_string(), (rc, h.ttv_error_string())

    for fn in ("sse", "ssim"):
        for call in (rgb, yuv):
            assert call(fn, n=0) == 0                                    # passes the checks, does nothing
            refused(call(fn, n=-1), b"n = -1")
            refused(call(fn, stride=0), b"b_stride 0")
            refused(call(fn, out=None), b"null")
            refused(call(fn, out=C.c_void_p((3 << 20) + 4)), b"8-byte")
        refused(rgb(fn, a=None), b"null")
        refused(rgb(fn, b=None), b"null")
        refused(yuv(fn, null_a=True), b"null frame description (a)")
        refused(yuv(fn, null_b=True), b"null frame description (b)")
        refused(yuv(fn, a=desc(24, 32, u=None)), b"null plane (a)")
        refused(yuv(fn, b=desc(24, 32, y=None)), b"null plane (b)")
        refused(yuv(fn, a=desc(24, 32, c_step=3)), b"c_step 3")
        refused(yuv(fn, a=desc(24, 32, y_pitch=31)), b"pitches")
        refused(yuv(fn, b=desc(24, 32, 2, c_pitch=31)), b"pitches")
        refused(yuv(fn, a=desc(24, 32, y_frame=24 * 32 - 1)), b"frame strides")
        refused(yuv(fn, b=desc(24, 32, 2, c_frame=11 * 32 + 30)), b"frame strides")
        assert yuv(fn, n=0, b=desc(24, 32, 2, c_frame=11 * 32 + 31)) == 0   # a frame's samples end at its last U byte
    # sizes: any H, W >= 1 for the sums; whole windows in every plane for SSIM
    refused(rgb("sse", H=0), b"at least 1")
    refused(yuv("sse", W=0), b"at least 1")
    assert rgb("sse", n=0, H=1, W=1) == 0 and yuv("sse", n=0, H=1, W=1) == 0
    refused(rgb("ssim", H=10), b"at least 11")
    refused(rgb("ssim", W=10), b"at least 11")
    refused(yuv("ssim", H=20), b"at least 21")
    refused(yuv("ssim", W=20), b"at least 21")
    assert rgb("ssim", n=0, H=11, W=11) == 0 and yuv("ssim", n=0, H=21, W=21) == 0
    # workspace: 2 frames x 3 planes of one tile each
    need = h.ttv_video_frame_ssim_workspace_bytes(2, 24, 32, 0)
    assert need == 2 * 3 * 8 == h.ttv_video_frame_ssim_workspace_bytes(2, 24, 32, 1)
    for call in (rgb, yuv):
        refused(call("ssim", nbytes=need - 8), b"workspace")
        refused(call("ssim", work=None), b"null")
        refused(call("ssim", work=C.c_void_p((4 << 20) + 4)), b"8-byte")


def test_workspace_bytes_is_deterministic_and_monotone():
    h = _lib.lib()
    f = h.ttv_video_frame_ssim_workspace_bytes
    assert f(0, 64, 64, 0) == 0 and f(0, 64, 64, 1) == 0
    # 256 x 256: 246 x 246 windows = 8 x 8 tiles per plane; 4:2:0 chroma 128 x 128: 118 x 118 = 4 x 4
    assert f(1, 256, 256, 0) == 3 * 64 * 8 and f(1, 256, 256, 1) == (64 + 2 * 16) * 8
    assert f(1, 43, 44, 0) == 3 * 2 * 2 * 8 and f(1, 42, 42, 0) == 3 * 8 and f(1, 45, 87, 1) == (2 * 3 + 2 * 2) * 8
    for yuv, (H, W) in ((0, (37, 45)), (1, (45, 87))):
        sizes = [f(n, H, W, yuv) for n in range(0, 9)]
        assert sizes == [f(n, H, W, yuv) for n in range(0, 9)]
        assert all(b - a == sizes[1] > 0 for a, b in zip(sizes, sizes[1:]))
    for bad in ((-1, 64, 64, 0), (1, 10, 64, 0), (1, 64, 10, 0), (1, 20, 64, 1), (1, 64, 20, 1)):
        assert f(*bad) == -1 and b"video_frame_ssim_workspace_bytes" in h.ttv_error_string()
