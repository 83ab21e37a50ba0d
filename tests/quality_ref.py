"""The numpy restatement of the per-frame quality measures of whole videos (include/titok_hip.h: ttv_video_frame_sse_*,
ttv_video_frame_ssim_*): what tests/test_hip_video_quality.py holds the kernels to, and what tests/test_video_quality_cpu.py pins by hand.

A plane is a 2-D uint8 array.  An RGB frame gives the planes f[..., 0], f[..., 1], f[..., 2]; a 4:2:0 frame the triple (y, u, v) with
chroma of ceil(H / 2) x ceil(W / 2).  Frame j of `a` meets frame j * b_stride of `b`."""
import numpy as np

C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2


def gaussian_taps() -> np.ndarray:
    """The 11-tap Gaussian, sigma 1.5, normalised to sum 1 (float64): gaussian_taps() of tests/test_ssim_cpu.py in numpy."""
    d = np.arange(11, dtype=np.float64) - 5
    g = np.exp(-((d / 1.5) ** 2) / 2)
    return g / g.sum()


def plane_sse(a: np.ndarray, b: np.ndarray) -> int:
    """sum (a - b)^2 over a plane pair as a Python int: int64 differences, and a sum that cannot overflow."""
    assert a.shape == b.shape and a.dtype == b.dtype == np.uint8
    d = a.astype(np.int64) - b.astype(np.int64)
    return int(sum(int(v) for v in (d * d).sum(axis=-1).reshape(-1)))


def rgb_planes(frame: np.ndarray):
    assert frame.ndim == 3 and frame.shape[-1] == 3
    return [frame[..., c] for c in range(3)]


def sse_rgb(a: np.ndarray, b: np.ndarray, b_stride: int = 1):
    """[n][3] Python ints for uint8 [n,H,W,3] against uint8 [.,H,W,3]."""
    return [[plane_sse(pa, pb) for pa, pb in zip(rgb_planes(a[j]), rgb_planes(b[j * b_stride]))] for j in range(a.shape[0])]


def sse_planes(a, b, b_stride: int = 1):
    """[n][3] Python ints for plane triples (y [n,H,W], u, v [n,Hc,Wc]) against such triples."""
    return [[plane_sse(pa[j], pb[j * b_stride]) for pa, pb in zip(a, b)] for j in range(a[0].shape[0])]


def plane_ssim(a: np.ndarray, b: np.ndarray) -> float:
    """Mean SSIM over the (h - 10)(w - 10) windows wholly inside a plane pair, float64, on the levels 0 .. 255.  Every window is
    formed directly as a weighted sum over its 11 x 11 samples (no padding anywhere)."""
    assert a.shape == b.shape and a.ndim == 2 and min(a.shape) >= 11
    x, y = a.astype(np.float64), b.astype(np.float64)
    g = gaussian_taps()
    h, w = a.shape

    def filt(p):
        rows = sum(g[k] * p[:, k:k + w - 10] for k in range(11))
        return sum(g[k] * rows[k:k + h - 10, :] for k in range(11))

    mx, my, exx, eyy, exy = (filt(p) for p in (x, y, x * x, y * y, x * y))
    sxx = np.maximum(exx - mx * mx, 0)
    syy = np.maximum(eyy - my * my, 0)
    sxy = exy - mx * my
    idx = ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))
    assert idx.shape == (h - 10, w - 10)
    return float(idx.mean())


def ssim_rgb(a: np.ndarray, b: np.ndarray, b_stride: int = 1) -> np.ndarray:
    return np.array([[plane_ssim(pa, pb) for pa, pb in zip(rgb_planes(a[j]), rgb_planes(b[j * b_stride]))] for j in range(a.shape[0])])


def ssim_planes(a, b, b_stride: int = 1) -> np.ndarray:
    return np.array([[plane_ssim(pa[j], pb[j * b_stride]) for pa, pb in zip(a, b)] for j in range(a[0].shape[0])])
