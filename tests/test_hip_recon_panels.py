"""`ttv_recon_panels_u8` (csrc/ttv_panels.hip) on the MI355X against the numpy restatement of tests/recon_panels_ref.py, through
ctypes and through `train.recon_panels`.  Element-exact: the value is defined bit for bit, so no byte may differ.  `-m gpu`.

Shapes: 1x8x8 (one block, the 16-byte path), 2x16x24 (W a multiple of 8 but not of 16), 3x11x13 (the element-wise path: odd W, row
starts at odd byte offsets, and a panel that starts 3 bytes off a word), two clips of different shapes in one call (one per path),
65 clips (one more than a launch takes).  Every panel lies in a buffer filled with a canary and one row longer than the panel."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import recon_panels_ref as PR  # noqa: E402

from titok_video_amd import _lib  # noqa: E402
from titok_video_amd.train import recon_panels  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 0xA5
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def raw_panels(targets, recons, lead=0):
    """The C entry point on device clips [3,T,H,W]; every panel in its own canary-filled buffer, `lead` bytes in and one row short of
    its end.  Returns the panels (numpy) after checking that the bytes around them still hold the canary."""
    dt = recons[0].dtype
    bufs, outs = [], []
    for x in recons:
        _, T, H, W = x.shape
        n = T * 3 * H * 2 * W
        b = torch.full((lead + n + 2 * W,), CANARY, dtype=torch.uint8, device=DEV)
        bufs.append((b, n))
        outs.append(b.data_ptr() + lead)
    dims = (C.c_int32 * (3 * len(recons)))(*[int(d) for x in recons for d in x.shape[1:]])
    rc = _lib.lib().ttv_recon_panels_u8(_lib.ptr_array(targets), _lib.ptr_array(recons), dims, len(recons), _lib.dtype_code(dt),
                                        (C.c_void_p * len(outs))(*outs), _lib.stream_ptr(torch.device(DEV)))
    _lib.check(rc, "ttv_recon_panels_u8")
    torch.cuda.synchronize()
    got = []
    for (b, n), x in zip(bufs, recons):
        h = b.cpu().numpy()
        assert (h[:lead] == CANARY).all() and (h[lead + n:] == CANARY).all(), "bytes outside the panel were written"
        got.append(h[lead:lead + n].reshape(x.shape[1], 3, x.shape[2], 2 * x.shape[3]))
    return got


def expected(targets, recons):
    return [PR.panel(y.float().cpu().numpy(), x.float().cpu().numpy()) for y, x in zip(targets, recons)]


def make_pair(shape, dtype, seed):
    """A target inside [-1, 1] with exact +-1 planted, a reconstruction with a good share beyond +-1 and 1.5, -3, +-inf planted."""
    g = torch.Generator().manual_seed(seed)
    T, H, W = shape
    y = (torch.rand(3, T, H, W, generator=g) * 2 - 1)
    x = torch.randn(3, T, H, W, generator=g) * 1.2
    yf, xf = y.view(-1), x.view(-1)
    yf[0], yf[-1], yf[yf.numel() // 2] = 1.0, -1.0, 1.0
    for k, v in enumerate((1.5, -3.0, float("inf"), float("-inf"), 1.0, -1.0)):
        xf[(k * 37 + 5) % xf.numel()] = v
    return y.to(dtype).to(DEV), x.to(dtype).to(DEV)


def assert_equal(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.uint8 and g.shape == w.shape, (what, i, g.shape, w.shape)
        bad = int((g != w).sum())
        assert bad == 0, f"{what}: clip {i}: {bad} of {w.size} bytes differ"


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("shape", [(1, 8, 8), (2, 16, 24), (3, 11, 13)])
def test_single_clip_is_exact(shape, dt):
    y, x = make_pair(shape, DTYPES[dt], seed=sum(shape))
    want = expected([y], [x])
    assert want[0][..., shape[2]:].min() == 0 and want[0][..., shape[2]:].max() == 255      # the clamp's ends are in the panel
    assert_equal(raw_panels([y], [x]), want, f"{shape} {dt}")
    if shape[2] % 8:
        assert_equal(raw_panels([y], [x], lead=3), want, f"{shape} {dt}, panel 3 bytes off a word")
    else:
        assert_equal(raw_panels([y], [x], lead=4), want, f"{shape} {dt}, panel off the 8-byte grid")


@pytest.mark.parametrize("dt", list(DTYPES))
def test_two_shapes_in_one_call_and_the_host_function(dt):
    pairs = [make_pair(s, DTYPES[dt], seed=k) for k, s in enumerate([(2, 16, 24), (3, 11, 13)])]
    ys, xs = [p[0] for p in pairs], [p[1] for p in pairs]
    want = expected(ys, xs)
    raw = raw_panels(ys, xs)
    assert_equal(raw, want, f"two shapes {dt}")
    host = recon_panels(ys, xs)
    assert_equal(host, raw, f"recon_panels {dt}")
    assert all(h.shape == (x.shape[1], 3, x.shape[2], 2 * x.shape[3]) for h, x in zip(host, xs))


@pytest.mark.parametrize("dt", list(DTYPES))
def test_65_clips_cross_the_launch_limit(dt):
    assert _lib.TTV_MAX_CLIPS_PER_LAUNCH == 64
    pairs = [make_pair((1, 8, 8), DTYPES[dt], seed=100 + k) for k in range(65)]
    ys, xs = [p[0] for p in pairs], [p[1] for p in pairs]
    want = expected(ys, xs)
    assert_equal(raw_panels(ys, xs), want, f"65 clips {dt}")
    assert_equal(recon_panels(ys, xs), want, f"recon_panels, 65 clips {dt}")


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("W", [8, 7])
def test_integer_edges_in_both_halves(W, dt):
    edges = PR.integer_edges()
    rows = -(-edges.size // W)
    flat = np.full(rows * W, np.float32(1.0), dtype=np.float32)
    flat[:edges.size] = edges
    clip = torch.from_numpy(np.broadcast_to(flat.reshape(1, 1, rows, W), (3, 1, rows, W)).copy()).to(DTYPES[dt]).to(DEV)
    other = clip.flip(2).contiguous()
    want = expected([clip, other], [other, clip])
    assert len(set(want[0][..., :W].reshape(-1).tolist())) == 256 or dt == "bf16"      # every level, from either side of its edge
    assert_equal(raw_panels([clip, other], [other, clip]), want, f"edges W={W} {dt}")


def test_nan_and_targets_outside_the_range_take_the_documented_values():
    y = torch.tensor([-1.5, 3.0, float("nan"), float("inf"), float("-inf"), -1.0, 1.0, 0.0]).repeat(3, 1, 8, 1).contiguous().to(DEV)
    x = torch.tensor([float("nan"), 7.0, -7.0, 0.0, -0.0, 1.0, -1.0, 0.5]).repeat(3, 1, 8, 1).contiguous().to(DEV)
    (got,) = raw_panels([y], [x])
    assert got[0, 0, 0].tolist() == [0, 255, 0, 255, 0, 0, 255, 127] + [0, 255, 0, 127, 127, 255, 0, 191]
    assert_equal([got], expected([y], [x]), "documented values")


def test_entry_point_refuses_bad_arguments():
    y, x = make_pair((1, 8, 8), torch.float32, seed=1)
    out = torch.zeros(3 * 8 * 16, dtype=torch.uint8, device=DEV)
    s = _lib.stream_ptr(torch.device(DEV))

    def call(dims, dt, out_ptr):
        return _lib.lib().ttv_recon_panels_u8(_lib.ptr_array([y]), _lib.ptr_array([x]), (C.c_int32 * 3)(*dims), 1, dt,
                                              (C.c_void_p * 1)(out_ptr), s)
    assert call((1, 8, 8), _lib.TTV_F32, out.data_ptr()) == 0
    for bad in (((0, 8, 8), _lib.TTV_F32, out.data_ptr()), ((1, 8, 8), 7, out.data_ptr()), ((1, 8, 8), _lib.TTV_F32, None),
                ((65536, 65536, 8), _lib.TTV_F32, out.data_ptr())):
        assert call(*bad) != 0, bad
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="no CPU path"):
        recon_panels([y.cpu()], [x.cpu()])
