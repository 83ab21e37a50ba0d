"""Y'CbCr 4:2:0 frames in and out on the MI355X: `ttv_video_tiles_yuv420`, `ttv_video_blend_yuv420` and `ttv_video_tile_sse_yuv420`
(csrc/ttv_video.hip) through the C ABI, bit for bit or integer for integer against the numpy restatement of tests/yuv_ref.py, with the
untouched RGB kernels as a second yardstick, and `video.VideoTokenizer` end to end on `YUV420Frames`.  `-m gpu`.

Planes live in host-packed byte buffers (`Surface`): any pitch, any lead, padding of a chosen byte, so that the same buffers serve as
pitched inputs and as canary-filled outputs."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rate_ref as RR  # noqa: E402
import video_ref as VR  # noqa: E402
import yuv_ref as YR  # noqa: E402

from titok_video_amd import _lib  # noqa: E402
from titok_video_amd import video as V  # noqa: E402
from titok_video_amd.model.titok import TiTok  # noqa: E402
from titok_video_amd.synthetic import seeded_titok_state  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
CANARY_U8, CANARY_F, GUARD = 0xA5, 77.0, 64
# (layout, matrix, range, siting): every value of each, every layout with both sitings
COMBOS = [("i420", "bt709", "limited", "left"), ("nv12", "bt601", "full", "center"), ("nv21", "bt709", "full", "left"),
          ("i420", "bt601", "limited", "center"), ("nv12", "bt709", "limited", "left"), ("nv21", "bt601", "limited", "center")]


def S():
    return _lib.stream_ptr(torch.device(DEV))


def both(video, tile, overlap, patch, stride=1):
    plan, ref = V.TilePlan(video, tile, overlap, patch, stride), VR.Plan(video, tile, overlap, patch, stride)
    assert plan.tile == ref.tile and list(plan.origins) == ref.origins
    return plan, ref


def random_planes(T, H, W, seed):
    r = np.random.default_rng(seed)
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    y, u, v = (r.integers(0, 256, s, dtype=np.uint8) for s in ((T, H, W), (T, Hc, Wc), (T, Hc, Wc)))
    y.reshape(-1)[:2], u.reshape(-1)[:2], v.reshape(-1)[:2] = (0, 255), (255, 0), (0, 255)
    return y, u, v


class Surface:
    """y, u, v (numpy uint8 [T,H,W], [T,Hc,Wc] x 2) packed into byte buffers as `layout` with `y_pad` / `c_pad` bytes after each row, a
    few bytes after each frame when padded, `lead` bytes in front and GUARD bytes behind; everything that is no sample is `fill`."""

    def __init__(self, y, u, v, layout, y_pad=0, c_pad=0, lead=0, fill=0):
        self.T, self.H, self.W = y.shape
        self.Hc, self.Wc = u.shape[1:]
        self.layout, self.lead, self.step = layout, lead, 1 if layout == "i420" else 2
        self.y_pitch, self.c_pitch = self.W + y_pad, self.step * self.Wc + c_pad
        self.y_frame = self.H * self.y_pitch + (5 if y_pad else 0)
        self.c_frame = self.Hc * self.c_pitch + (3 if c_pad else 0)
        ybuf = np.full(lead + self.T * self.y_frame + GUARD, fill, dtype=np.uint8)
        self.y_view(ybuf)[...] = y
        if layout == "i420":
            ubuf, vbuf = (np.full(lead + self.T * self.c_frame + GUARD, fill, dtype=np.uint8) for _ in range(2))
            self.c_view(ubuf, 0)[...] = u
            self.c_view(vbuf, 0)[...] = v
            self.host = [ybuf, ubuf, vbuf]
        else:
            cbuf = np.full(lead + self.T * self.c_frame + GUARD, fill, dtype=np.uint8)
            self.c_view(cbuf, 0 if layout == "nv12" else 1)[...] = u
            self.c_view(cbuf, 1 if layout == "nv12" else 0)[...] = v
            self.host = [ybuf, cbuf]
        self.dev = [torch.from_numpy(b).to(DEV) for b in self.host]

    def y_view(self, buf):
        return np.lib.stride_tricks.as_strided(buf[self.lead:], (self.T, self.H, self.W), (self.y_frame, self.y_pitch, 1))

    def c_view(self, buf, at):
        return np.lib.stride_tricks.as_strided(buf[self.lead + at:], (self.T, self.Hc, self.Wc), (self.c_frame, self.c_pitch, self.step))

    def pointers(self):
        y = self.dev[0].data_ptr() + self.lead
        if self.layout == "i420":
            return y, self.dev[1].data_ptr() + self.lead, self.dev[2].data_ptr() + self.lead
        c = self.dev[1].data_ptr() + self.lead
        return (y, c, c + 1) if self.layout == "nv12" else (y, c + 1, c)

    def desc(self, m, r, s, **override):
        y, u, v = self.pointers()
        kw = dict(y=y, u=u, v=v, y_frame=self.y_frame, c_frame=self.c_frame, y_pitch=self.y_pitch, c_pitch=self.c_pitch, c_step=self.step,
                  matrix=_lib.YUV_MATRIX[m], range=_lib.YUV_RANGE[r], siting=_lib.YUV_SITING[s])
        kw.update(override)
        return _lib.Yuv420(**kw)

    def frames(self, matrix, rng, siting):
        """The same planes as strided views of the device buffers: what wrapping a decoder surface looks like."""
        y = self.dev[0][self.lead:].as_strided((self.T, self.H, self.W), (self.y_frame, self.y_pitch, 1))
        kw = dict(matrix=matrix, range=rng, siting=siting)
        cs = (self.T, self.Hc, self.Wc)
        if self.layout == "i420":
            u, v = (self.dev[k][self.lead:].as_strided(cs, (self.c_frame, self.c_pitch, 1)) for k in (1, 2))
            return V.YUV420Frames(y, u=u, v=v, **kw)
        pair = self.dev[1][self.lead:].as_strided(cs + (2,), (self.c_frame, self.c_pitch, 2, 1))
        return V.YUV420Frames(y, uv=pair, **kw) if self.layout == "nv12" else V.YUV420Frames(y, vu=pair, **kw)

    def download(self):
        return [d.cpu().numpy() for d in self.dev]


def same_bits(got, want, what):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert bad == 0, f"{what}: {bad} of {want.size} elements differ"


# ---- gather -----------------------------------------------------------------------------------------------------------------------------
def raw_gather(desc, plan, begin, end, dt, cplan=None, out_shift=0, dtype_code=None, null_out=False):
    n = (end - begin) * 3 * plan.tile[0] * plan.tile[1] * plan.tile[2]
    buf = torch.full((max(n, 0) + 2 * GUARD,), CANARY_F, dtype=DTYPES[dt], device=DEV)
    cp = plan.c_plan() if cplan is None else cplan
    rc = _lib.lib().ttv_video_tiles_yuv420(None if desc is None else C.byref(desc), C.byref(cp), begin, end,
                                           None if null_out else buf.data_ptr() + GUARD * buf.element_size() + out_shift,
                                           _lib.dtype_code(DTYPES[dt]) if dtype_code is None else dtype_code, S())
    torch.cuda.synchronize()
    h = buf.float().cpu().numpy()
    if rc != 0:
        assert (h == CANARY_F).all(), "a refused call wrote something"
        return rc, None
    assert (h[:GUARD] == CANARY_F).all() and (h[GUARD + n:] == CANARY_F).all(), "elements outside the tiles were written"
    return rc, h[GUARD:GUARD + n].reshape((end - begin, 3) + plan.tile)


GATHER = {
    "every axis shorter than the tile, odd H and W": ((3, 13, 19), (4, 16, 24), (2, 8, 8), (4, 8, 8), 1),
    "T and H shorter, two tiles along W": ((3, 13, 19), (4, 16, 16), (0, 0, 4), (4, 8, 8), 1),
    "odd strides: origins on odd rows and columns": ((5, 40, 45), (4, 16, 16), (0, 3, 3), (4, 8, 8), 1),
    "Wt no multiple of 8": ((5, 21, 27), (4, 16, 12), (0, 8, 4), (4, 8, 4), 1),
    "frame stride 2": ((7, 20, 24), (4, 16, 16), (2, 4, 4), (4, 8, 8), 2),
}


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("case", list(GATHER))
def test_gather_is_exact(case, dt):
    video, tile, overlap, patch, stride = GATHER[case]
    plan, ref = both(video, tile, overlap, patch, stride)
    if "odd strides" in case:
        assert any(o % 2 for o in plan.origins[1]) and any(o % 2 for o in plan.origins[2])
    y, u, v = random_planes(*video, seed=sum(video))
    for layout, matrix, rng, siting in COMBOS:
        want = YR.gather(y, u, v, ref, 0, plan.n_tiles, dt, matrix, rng, siting)
        assert want.min() == -1.0 and want.max() == 1.0
        what = f"{case} {dt} {layout} {matrix} {rng} {siting}"
        # tight planes on the allocation's grid; then pitched planes one and three bytes off the 4-byte grid, padding of 0 and of 255
        for y_pad, c_pad, lead, fill in ((0, 0, 0, 0), (5, 3, 1, 0), (5, 3, 3, 255)):
            surf = Surface(y, u, v, layout, y_pad, c_pad, lead, fill)
            rc, got = raw_gather(surf.desc(matrix, rng, siting), plan, 0, plan.n_tiles, dt)
            assert rc == 0, _lib.lib().ttv_error_string()
            same_bits(got, want, f"{what}, pads {y_pad} {c_pad}, lead {lead}, padding {fill}")
        same_bits(V.gather_tiles(surf.frames(matrix, rng, siting), plan, 1, plan.n_tiles, DTYPES[dt]).float().cpu().numpy(), want[1:],
                  f"gather_tiles of pitched views, {what}")


@pytest.mark.parametrize("dt,combo", [("f32", COMBOS[0]), ("bf16", COMBOS[1])])
def test_gather_of_every_chroma_pair(dt, combo):
    """512 x 512: the chroma planes hold every (U, V) pair once, Y sweeps 0 .. 255 along both axes."""
    layout, matrix, rng, siting = combo
    plan, ref = both((1, 512, 512), (1, 128, 128), (0, 16, 16), (1, 8, 8))
    yy, xx = np.meshgrid(np.arange(512), np.arange(512), indexing="ij")
    y = ((7 * xx + 13 * yy) & 255).astype(np.uint8)[None]
    vv, uu = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    u, v = uu.astype(np.uint8)[None], vv.astype(np.uint8)[None]
    want = YR.gather(y, u, v, ref, 0, plan.n_tiles, dt, matrix, rng, siting)
    rc, got = raw_gather(Surface(y, u, v, layout).desc(matrix, rng, siting), plan, 0, plan.n_tiles, dt)
    assert rc == 0
    same_bits(got, want, f"every chroma pair, {dt} {combo}")


def test_gather_refuses_bad_arguments():
    plan, _ = both((5, 21, 27), (4, 16, 16), (0, 8, 4), (4, 8, 8))
    y, u, v = random_planes(5, 21, 27, seed=1)
    for layout in ("i420", "nv12"):
        surf = Surface(y, u, v, layout, 5, 3, 1)
        d = lambda **kw: surf.desc("bt709", "limited", "left", **kw)  # noqa: E731
        assert raw_gather(d(), plan, 0, 2, "bf16")[0] == 0
        assert raw_gather(d(), plan, 3, 3, "bf16")[0] == 0                           # an empty range is no error and no launch
        bad = [dict(y=None), dict(u=None), dict(v=None), dict(c_step=0), dict(c_step=3), dict(matrix=2), dict(matrix=-1), dict(range=2),
               dict(range=-1), dict(siting=2), dict(siting=-1), dict(y_pitch=26), dict(c_pitch=surf.step * 14 - 1),
               dict(y_frame=20 * surf.y_pitch + 26), dict(c_frame=10 * surf.c_pitch + surf.step * 13)]
        for kw in bad:
            assert raw_gather(d(**kw), plan, 0, 2, "bf16")[0] == 1, kw
            assert b"video_tiles_yuv420" in _lib.lib().ttv_error_string()
        # the least strides that are in order
        assert raw_gather(d(y_frame=20 * surf.y_pitch + 27, c_frame=10 * surf.c_pitch + surf.step * 13 + 1), plan, 0, 1, "bf16")[0] == 0
    assert raw_gather(None, plan, 0, 2, "bf16")[0] == 1
    assert raw_gather(d(), plan, 0, 2, "bf16", dtype_code=7)[0] == 1
    assert raw_gather(d(), plan, 0, 2, "bf16", null_out=True)[0] == 1
    assert raw_gather(d(), plan, 0, 2, "bf16", out_shift=2)[0] == 1                 # a destination off the 16-byte grid
    assert raw_gather(d(), plan, 0, plan.n_tiles + 1, "bf16")[0] == 1 and raw_gather(d(), plan, -1, 2, "bf16")[0] == 1
    for field, value in (("count", (2, 5, 3)), ("overlap", (0, 9, 4)), ("overlap", (0, -1, 4)), ("tile", (4, 0, 16))):
        cp = plan.c_plan()
        setattr(cp, field, (_lib.i32 * 3)(*value))
        assert raw_gather(d(), plan, 0, 2, "bf16", cplan=cp)[0] == 1, (field, value)
    cp = plan.c_plan()
    cp.frame_stride = 0
    assert raw_gather(d(), plan, 0, 2, "bf16", cplan=cp)[0] == 1
    with pytest.raises(ValueError):
        V.gather_tiles(surf.frames("bt709", "limited", "left"), V.TilePlan((5, 21, 28), (4, 16, 16), (0, 8, 4), (4, 8, 8)))
    with pytest.raises(RuntimeError):
        V.YUV420Frames(torch.zeros((1, 2, 2), dtype=torch.uint8), u=torch.zeros((1, 1, 1), dtype=torch.uint8), v=torch.zeros((1, 1, 1), dtype=torch.uint8))


# ---- blend ------------------------------------------------------------------------------------------------------------------------------
def random_tiles(plan, dt, seed, nans=True):
    """Per tile U(-1.5, 1.5) with exact +-1, +-1.5, 0, +-inf and NaNs planted; device tensors, one allocation each."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(plan.n_tiles):
        x = torch.rand((3,) + plan.tile, generator=g) * 3.0 - 1.5
        f = x.view(-1)
        for j, v in enumerate((1.0, -1.0, 1.5, -1.5, 0.0)):
            f[(j * 53 + 7 * k + 1) % f.numel()] = v
        if nans:
            for j, v in enumerate((float("nan"), float("inf"), float("-inf"), float("nan"))):
                f[(11 * k + 3 + 97 * j) % f.numel()] = v
        out.append(x.to(DTYPES[dt]).to(DEV))
    return out


def raw_blend(tiles, plan, t0, t1, surf, combo, dtype_code=None, null_table=False, **override):
    """The C entry point into the planes of `surf` (device buffers, canary-filled).  Returns rc."""
    ptrs = [0 if t is None else t.data_ptr() for t in tiles]
    host = (C.c_void_p * len(ptrs))(*ptrs)
    table = torch.tensor(ptrs, dtype=torch.int64).to(DEV)
    dt = next(t.dtype for t in tiles if t is not None)
    cp, d = plan.c_plan(), surf.desc(*combo[1:], **override)
    rc = _lib.lib().ttv_video_blend_yuv420(None if null_table else host, table.data_ptr(), C.byref(cp), t0, t1,
                                           _lib.dtype_code(dt) if dtype_code is None else dtype_code, C.byref(d), S())
    torch.cuda.synchronize()
    return rc


def canary_surface(n, H, W, layout, y_pad, c_pad, lead):
    z = lambda *s: np.zeros(s, dtype=np.uint8)  # noqa: E731
    surf = Surface(z(n, H, W), z(n, (H + 1) // 2, (W + 1) // 2), z(n, (H + 1) // 2, (W + 1) // 2), layout, y_pad, c_pad, lead, CANARY_U8)
    for d in surf.dev:
        d.fill_(CANARY_U8)
    return surf


def check_blend(tiles, plan, t0, t1, what, combos=COMBOS):
    """The planes against yuv_ref's conversion of what the RGB kernel returns for the same tiles, every buffer byte compared: the
    padding, the bytes before and behind and between the frames keep their canary."""
    rgb = V.blend_tiles(tiles, plan, t0, t1).cpu().numpy()
    n, H, W = rgb.shape[:3]
    for layout, matrix, rng, siting in combos:
        (y, u, v), _ = YR.planes_from_levels(rgb, matrix, rng, siting)
        for y_pad, c_pad, lead in ((0, 0, 0), (5, 3, 1), (2, 6, 3)):
            surf = canary_surface(n, H, W, layout, y_pad, c_pad, lead)
            rc = raw_blend(tiles, plan, t0, t1, surf, (layout, matrix, rng, siting))
            assert rc == 0, _lib.lib().ttv_error_string()
            want = Surface(y, u, v, layout, y_pad, c_pad, lead, CANARY_U8).host
            first = surf.download()
            for name, g, w in zip(("luma", "chroma", "chroma v"), first, want):
                bad = int((g != w).sum())
                assert bad == 0, f"{what} {layout} {matrix} {rng} {siting}, pads {y_pad} {c_pad}, lead {lead}: {bad} {name} bytes differ"
        rc = raw_blend(tiles, plan, t0, t1, surf, (layout, matrix, rng, siting))      # the same call again, onto its own result
        assert rc == 0 and all((a == b).all() for a, b in zip(first, surf.download())), f"{what}: two identical calls differ"
    return rgb


BLEND = {
    "odd sizes, every axis overlapped": ((5, 37, 45), (4, 16, 24), (2, 8, 8), (4, 8, 8)),
    "triple cover on all three": ((15, 30, 30), (8, 16, 16), (2, 4, 4), (4, 8, 8)),
    "H = 1": ((4, 1, 30), (4, 8, 16), (0, 0, 4), (4, 8, 8)),
    "W = 1": ((4, 30, 1), (4, 16, 8), (0, 4, 0), (4, 8, 8)),
    "H = W = 2, a single padded tile": ((3, 2, 2), (4, 8, 8), (0, 0, 0), (4, 8, 8)),
    "rows of several blocks, odd W": ((2, 6, 531), (2, 8, 64), (0, 0, 8), (2, 8, 8)),
    "rows of 65 to 128 groups of four, odd H": ((2, 5, 300), (2, 8, 64), (0, 0, 8), (2, 8, 8)),
    "W a multiple of 4, Wt not of 8": ((5, 21, 28), (4, 16, 12), (0, 8, 4), (4, 8, 4)),
}


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("case", list(BLEND))
def test_blend_is_exact(case, dt):
    video, tile, overlap, patch = BLEND[case]
    plan, _ = both(video, tile, overlap, patch)
    if "triple" in case:
        assert plan.origins[0] == [0, 6, 7] and plan.origins[1] == [0, 12, 14]
    tiles = random_tiles(plan, dt, seed=len(case))
    rgb = check_blend(tiles, plan, 0, plan.timeline[0], f"{case} {dt}")
    assert rgb.size < 4096 or (rgb.min() == 0 and rgb.max() == 255)
    layout, matrix, rng, siting = COMBOS[1]
    (y, u, v), _ = YR.planes_from_levels(rgb, matrix, rng, siting)
    out = V.blend_tiles(tiles, plan, out=V.YUV420Frames.empty(video[0], video[1], video[2], layout, DEV, matrix, rng, siting))
    assert out.layout == layout and (out.y.cpu().numpy() == y).all() and (out.u.cpu().numpy() == u).all() and (out.v.cpu().numpy() == v).all()


@pytest.mark.parametrize("dt", list(DTYPES))
def test_blend_of_a_frame_range_with_null_tiles(dt):
    plan, _ = both((20, 40, 56), (8, 32, 32), (4, 8, 8), (4, 8, 8))
    assert plan.origins[0] == [0, 4, 8, 12] and plan.tiles_per_layer == 4
    tiles = random_tiles(plan, dt, seed=9)
    part = [None] * 4 + tiles[4:12] + [None] * 4              # frames [9, 12) lie in layers 1 and 2 only
    rgb = check_blend(part, plan, 9, 12, f"frames [9, 12) {dt}", COMBOS[:2])
    assert (rgb == V.blend_tiles(tiles, plan).cpu().numpy()[9:12]).all()
    out = V.blend_tiles(part, plan, 9, 12, out="nv12")
    (y, u, v), _ = YR.planes_from_levels(rgb, "bt709", "limited", "left")
    assert out.shape == (3, 40, 56) and (out.y.cpu().numpy() == y).all() and (out.u.cpu().numpy() == u).all() and (out.v.cpu().numpy() == v).all()
    surf = canary_surface(3, 40, 56, "i420", 0, 0, 0)
    for hole in (4, 11):                                       # a covering tile that is NULL: the error, and nothing launched
        broken = list(part)
        broken[hole] = None
        assert raw_blend(broken, plan, 9, 12, surf, COMBOS[0]) == 1 and b"NULL" in _lib.lib().ttv_error_string()
    assert raw_blend(part, plan, 7, 10, surf, COMBOS[0]) == 1 and raw_blend(part, plan, 9, 13, canary_surface(4, 40, 56, "i420", 0, 0, 0), COMBOS[0]) == 1
    assert all((d.cpu().numpy() == CANARY_U8).all() for d in surf.dev), "a refused call wrote something"


def test_blend_refuses_bad_arguments():
    plan, _ = both((5, 21, 27), (4, 16, 16), (0, 8, 4), (4, 8, 8))
    tiles = random_tiles(plan, "f32", seed=2, nans=False)
    n = plan.timeline[0]
    for layout in ("i420", "nv21"):
        combo = (layout, "bt601", "full", "center")
        surf = canary_surface(n, 21, 27, layout, 5, 3, 1)
        bad = [dict(y=None), dict(u=None), dict(v=None), dict(c_step=0), dict(c_step=4), dict(matrix=2), dict(range=2), dict(siting=2),
               dict(y_pitch=26), dict(c_pitch=surf.step * 14 - 1), dict(y_frame=20 * surf.y_pitch + 26),
               dict(c_frame=10 * surf.c_pitch + surf.step * 13)]
        for kw in bad:
            assert raw_blend(tiles, plan, 0, n, surf, combo, **kw) == 1, kw
            assert b"video_blend_yuv420" in _lib.lib().ttv_error_string()
        for t0, t1 in ((-1, 3), (0, n + 1), (4, 3)):
            assert raw_blend(tiles, plan, t0, t1, surf, combo) == 1, (t0, t1)
        assert raw_blend(tiles, plan, 0, n, surf, combo, dtype_code=5) == 1
        assert raw_blend(tiles, plan, 0, n, surf, combo, null_table=True) == 1
        cp_bad = V.TilePlan((5, 21, 27), (4, 16, 16), (0, 8, 4), (4, 8, 8))
        cp_bad.counts = (2, 3, 2)
        assert raw_blend(tiles, cp_bad, 0, n, surf, combo) == 1
        assert raw_blend(tiles, plan, 2, 2, surf, combo) == 0                         # an empty range is no error and no launch
        assert all((d.cpu().numpy() == CANARY_U8).all() for d in surf.dev), "a refused call wrote something"
        assert raw_blend(tiles, plan, 0, n, surf, combo) == 0
    with pytest.raises(ValueError):
        V.blend_tiles(tiles, plan, out="yuy2")
    with pytest.raises(ValueError):
        V.blend_tiles(tiles, plan, out=V.YUV420Frames.empty(n, 21, 28, "i420", DEV))
    with pytest.raises(ValueError):
        V.blend_tiles(tiles, plan, 1, n, out=V.YUV420Frames.empty(n, 21, 27, "i420", DEV))


# ---- squared error ----------------------------------------------------------------------------------------------------------------------
def raw_sse(desc, plan, begin, end, recon, dtype_code=None, null=(), shift=0):
    n = end - begin
    buf = torch.full((n + 2,), 0x5A5A5A5A5A5A5A5, dtype=torch.int64, device=DEV)
    ptrs = [0 if t is None else t.data_ptr() for t in recon]
    host = (C.c_void_p * max(len(ptrs), 1))(*ptrs)
    table = torch.tensor(ptrs if ptrs else [0], dtype=torch.int64).to(DEV)
    dt = next((t.dtype for t in recon if t is not None), torch.float32)
    cp = plan.c_plan()
    rc = _lib.lib().ttv_video_tile_sse_yuv420(None if desc is None else C.byref(desc), C.byref(cp), begin, end, None if "host" in null else host,
                                              None if "table" in null else table.data_ptr(), _lib.dtype_code(dt) if dtype_code is None else dtype_code,
                                              None if "sse" in null else buf.data_ptr() + 8 + shift, S())
    torch.cuda.synchronize()
    h = buf.cpu().tolist()
    if rc != 0:
        assert all(x == 0x5A5A5A5A5A5A5A5 for x in h), "a refused call wrote something"
        return rc, None
    assert h[0] == h[-1] == 0x5A5A5A5A5A5A5A5, "sums outside the range were written"
    return rc, h[1:-1]


SSE = {
    "stride 1, odd sizes": ((5, 37, 45), (4, 16, 24), (2, 8, 8), (4, 8, 8), 1),
    "stride 2, every axis shorter than the tile": ((5, 13, 19), (4, 16, 24), (2, 8, 8), (4, 8, 8), 2),
    "Wt no multiple of 8, odd origins": ((5, 21, 27), (4, 16, 12), (0, 3, 3), (4, 8, 4), 1),
}


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("case", list(SSE))
def test_tile_sse_is_exact(case, dt):
    video, tile, overlap, patch, stride = SSE[case]
    plan, ref = both(video, tile, overlap, patch, stride)
    y, u, v = random_planes(*video, seed=len(case))
    recon = random_tiles(plan, dt, seed=5)
    host = [t.float().cpu().numpy() for t in recon]
    for layout, matrix, rng, siting in COMBOS[:4]:
        levels = YR.source_levels(y, u, v, matrix, rng, siting)
        want = [RR.tile_sse(levels, ref, k, host[k]) for k in range(plan.n_tiles)]
        surf = Surface(y, u, v, layout, 5, 3, 1, 255)
        rc, got = raw_sse(surf.desc(matrix, rng, siting), plan, 0, plan.n_tiles, recon)       # onto garbage: written, not accumulated
        assert rc == 0 and got == want, f"{case} {dt} {layout} {matrix} {rng} {siting}"
        frames = surf.frames(matrix, rng, siting)
        assert V.tile_sse(frames, plan, recon[1:], 1).tolist() == want[1:]
        # the second yardstick: the RGB kernel on the video of source levels
        rgb = torch.from_numpy(levels).to(DEV)
        assert V.tile_sse(rgb, plan, recon).tolist() == want
        # a reconstruction whose levels are the source levels costs nothing
        exact = list(V.gather_tiles(rgb, plan, dtype=torch.float32).unbind(0))
        assert V.tile_sse(frames, plan, exact).tolist() == [0] * plan.n_tiles


def test_tile_sse_refuses_bad_arguments():
    plan, _ = both((5, 21, 27), (4, 16, 16), (0, 8, 4), (4, 8, 8))
    y, u, v = random_planes(5, 21, 27, seed=1)
    surf = Surface(y, u, v, "nv12", 5, 3, 1)
    recon = random_tiles(plan, "bf16", seed=4)[:3]
    d = lambda **kw: surf.desc("bt709", "limited", "left", **kw)  # noqa: E731
    assert raw_sse(d(), plan, 0, 3, recon)[0] == 0 and raw_sse(d(), plan, 2, 2, [])[0] == 0
    bad = [dict(y=None), dict(u=None), dict(v=None), dict(c_step=3), dict(matrix=2), dict(range=2), dict(siting=2), dict(y_pitch=26),
           dict(c_pitch=27), dict(y_frame=20 * surf.y_pitch + 26), dict(c_frame=10 * surf.c_pitch + 26)]
    for kw in bad:
        assert raw_sse(d(**kw), plan, 0, 3, recon)[0] == 1, kw
        assert b"video_tile_sse_yuv420" in _lib.lib().ttv_error_string()
    assert raw_sse(None, plan, 0, 3, recon)[0] == 1
    assert raw_sse(d(), plan, 0, 3, recon, dtype_code=9)[0] == 1
    for null in ("host", "table", "sse"):
        assert raw_sse(d(), plan, 0, 3, recon, null=(null,))[0] == 1
    assert raw_sse(d(), plan, 0, 3, recon, shift=4)[0] == 1
    assert raw_sse(d(), plan, 0, 3, recon[:2] + [None])[0] == 1
    assert raw_sse(d(), plan, -1, 2, recon)[0] == 1 and raw_sse(d(), plan, plan.n_tiles - 2, plan.n_tiles + 1, recon)[0] == 1
    with pytest.raises(ValueError):
        V.tile_sse(surf.frames("bt709", "limited", "left"), plan, recon[:2], 0, 3)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
VIDEO, TILE, OVERLAP, PATCH, K, SEQ = (20, 40, 56), (8, 32, 32), (4, 8, 8), (4, 8, 8), 8, 200
BATCHES = ((0, 5), (5, 10), (10, 15), (15, 16))               # 32 patches + at most 8 tokens a tile under 200 rows
LADDER = (2, 4, 8)


def tiny_model():
    m = SimpleNamespace(patch_size=list(PATCH), fsq_levels=[7, 5, 5, 5, 5], encoder_size="tiny", decoder_size="tiny")
    model = TiTok(SimpleNamespace(tokenizer=SimpleNamespace(model=m)))
    missing, unexpected = model.load_state_dict(seeded_titok_state(0), strict=False)
    assert not unexpected and all(k.startswith("quantize.") for k in missing)
    return model.to(DEV, torch.bfloat16).eval()


@pytest.fixture(scope="module")
def round_trip():
    model = tiny_model()
    y, u, v = random_planes(*VIDEO, seed=77)
    frames = Surface(y, u, v, "nv12", 8, 8, 0).frames("bt709", "limited", "left")
    vt = V.VideoTokenizer(model, tile=TILE, overlap=OVERLAP, tokens_per_tile=K, seq_len=SEQ, dtype=torch.bfloat16, depth=2)
    tok = vt.encode_video(frames, fps=24.0)
    out = vt.decode_video(tok, output="i420")
    torch.cuda.synchronize()
    return model, frames, vt, tok, out


def test_encode_equals_the_steps_done_by_hand(round_trip):
    model, frames, vt, tok, _ = round_trip
    plan = V.TilePlan(VIDEO, TILE, OVERLAP, PATCH)
    assert plan.n_tiles == 16
    with torch.no_grad():
        idx = torch.cat([model.encode(list(V.gather_tiles(frames, plan, a, b, torch.bfloat16).unbind(0)), [K] * (b - a))[1]["indices"]
                         for a, b in BATCHES])
    assert tok.counts == [K] * 16 and tok.fps == 24.0 and (tok.video, tok.tile, tok.frame_stride) == (VIDEO, TILE, 1)
    assert torch.equal(tok.indices.cpu(), idx.to(torch.int32).cpu())
    again = vt.encode_video(frames, fps=24.0, frame_stride=3)
    assert again.plan().timeline == (7, 40, 56) and again.fps == 8.0 and len(again.counts) == 4


def test_allocated_counts_equal_the_steps_done_by_hand(round_trip):
    model, frames, vt, _, _ = round_trip
    plan = V.TilePlan(VIDEO, TILE, OVERLAP, PATCH)
    sums, indices = [], []
    with torch.no_grad():
        for count in LADDER:
            part_s, part_i = [], []
            for a, b in BATCHES:
                recon, info = model(list(V.gather_tiles(frames, plan, a, b, torch.bfloat16).unbind(0)), [count] * (b - a))
                part_s.append(V.tile_sse(frames, plan, recon, a, b))
                part_i.append(info["indices"].to(torch.int32))
            sums.append(torch.cat(part_s).tolist())
            indices.append(torch.cat(part_i).view(16, count).cpu())
    sse = [[sums[l][j] for l in range(len(LADDER))] for j in range(16)]
    table = vt.rate_distortion(frames, LADDER)
    assert table.sse == sse and table.elements == [plan.tile_elements(j) for j in range(16)]
    quality = sorted(q for row in table.psnr() for q in row)
    target = quality[len(quality) // 2]
    for kw, counts in ((dict(target_psnr=target), RR.allocate_target(LADDER, sse, table.elements, target)),
                       (dict(total_tokens=70), RR.allocate_budget(LADDER, sse, 70))):
        tok = vt.encode_video(frames, ladder=LADDER, **kw)
        assert tok.counts == list(counts)
        want = torch.cat([indices[LADDER.index(k)][j] for j, k in enumerate(counts)])
        assert torch.equal(tok.indices.cpu(), want)


def test_decode_into_planes_equals_the_conversion_of_the_rgb_frames(round_trip):
    _, _, vt, tok, out = round_trip
    rgb = vt.decode_video(tok).cpu().numpy()
    assert len(np.unique(rgb)) > 32
    (y, u, v), _ = YR.planes_from_levels(rgb, "bt709", "limited", "left")
    assert isinstance(out, V.YUV420Frames) and out.layout == "i420" and out.shape == VIDEO
    assert (out.y.cpu().numpy() == y).all() and (out.u.cpu().numpy() == u).all() and (out.v.cpu().numpy() == v).all()
    # into planes of the caller's, another layout and colour description
    mine = V.YUV420Frames.empty(*VIDEO, layout="nv21", device=DEV, matrix="bt601", range="full", siting="center")
    assert vt.decode_video(tok, output=mine) is mine
    (y, u, v), _ = YR.planes_from_levels(rgb, "bt601", "full", "center")
    assert (mine.y.cpu().numpy() == y).all() and (mine.u.cpu().numpy() == u).all() and (mine.v.cpu().numpy() == v).all()
    with pytest.raises(ValueError):
        vt.decode_video(tok, output="rgb24")
    with pytest.raises(ValueError):
        next(vt.decode_video_iter(tok, output=V.YUV420Frames.empty(19, 40, 56, device=DEV)))


def test_iter_ranges_concatenate_to_the_planes(round_trip):
    _, _, vt, tok, out = round_trip
    at, parts = 0, []
    for t0, part in vt.decode_video_iter(tok, output="i420"):
        assert t0 == at and isinstance(part, V.YUV420Frames) and part.shape[1:] == VIDEO[1:]
        at += part.shape[0]
        parts.append(part)
    assert at == VIDEO[0] and [p.shape[0] for p in parts] == [4, 4, 4, 8]
    for plane in ("y", "u", "v"):
        assert torch.equal(torch.cat([getattr(p, plane) for p in parts]), getattr(out, plane))


def test_an_rgb_video_still_gives_its_bytes(round_trip):
    """The RGB path, unchanged arguments, against the restatement of tests/video_ref.py around the public model calls."""
    model, _, vt, _, _ = round_trip
    g = torch.Generator().manual_seed(77)
    frames = torch.randint(0, 256, VIDEO + (3,), generator=g, dtype=torch.uint8)
    tok = vt.encode_video(frames.to(DEV), fps=24.0)
    out = vt.decode_video(tok)
    ref = VR.Plan(VIDEO, TILE, OVERLAP, PATCH)
    cut = VR.gather(frames.numpy(), ref, 0, 16, "bf16")
    with torch.no_grad():
        idx = torch.cat([model.encode([torch.from_numpy(cut[k]).to(torch.bfloat16).to(DEV) for k in range(a, b)], [K] * (b - a))[1]["indices"]
                         for a, b in BATCHES])
        recon = []
        for layer in range(4):
            recon += model.decode_indices(idx[layer * 4 * K:(layer + 1) * 4 * K], [TILE] * 4, [K] * 4)
    assert torch.equal(tok.indices.cpu(), idx.to(torch.int32).cpu())
    assert out.dtype == torch.uint8 and (out.cpu().numpy() == VR.blend([r.float().cpu().numpy() for r in recon], ref)).all()
