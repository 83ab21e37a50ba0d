"""tests/recon_panels_ref.py against the reference's own expression (train.py:141-142), typed out here with torch on the CPU: for
targets inside [-1, 1] and arbitrary reconstructions the two give the same bytes.  No GPU."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import recon_panels_ref as PR  # noqa: E402


def reference_expression(y: torch.Tensor, x: torch.Tensor) -> np.ndarray:
    merged_video = torch.cat((y, x.clamp(-1, 1)), dim=-1).permute(1, 0, 2, 3).cpu().float().numpy()
    return ((merged_video + 1) / 2 * 255).astype(np.uint8)


def restated(y: torch.Tensor, x: torch.Tensor) -> np.ndarray:
    return PR.panel(y.float().numpy(), x.float().numpy())


def test_random_clips_fp32_and_bf16():
    g = torch.Generator().manual_seed(7)
    for dtype in (torch.float32, torch.bfloat16):
        for T, H, W in ((1, 8, 8), (3, 11, 13), (2, 16, 24)):
            y = (torch.rand(3, T, H, W, generator=g) * 2 - 1).to(dtype)
            x = (torch.randn(3, T, H, W, generator=g) * 1.2).to(dtype)          # a good share beyond +-1
            got, want = restated(y, x), reference_expression(y, x)
            assert got.dtype == np.uint8 and got.shape == (T, 3, H, 2 * W)
            assert np.array_equal(got, want), (dtype, T, H, W)
            assert int((x.float().abs() > 1).sum()) > 0


def test_planted_integer_edges_and_ends():
    edges = PR.integer_edges()
    assert edges.size >= 256 * 3 and edges.min() == -1.0 and edges.max() == 1.0
    # the sweep holds both sides of the crossings: the level steps inside it
    lv = PR.levels(edges)
    assert lv.min() == 0 and lv.max() == 255 and len(set(lv.tolist())) == 256
    n = edges.size
    W = 8
    rows = -(-n // W)
    flat = np.full(rows * W, np.float32(1.0), dtype=np.float32)
    flat[:n] = edges
    clip = torch.from_numpy(np.broadcast_to(flat.reshape(1, 1, rows, W), (3, 1, rows, W)).copy())
    for dtype in (torch.float32, torch.bfloat16):
        c = clip.to(dtype)
        # in both halves: as the target, and as the reconstruction
        assert np.array_equal(restated(c, c.flip(2)), reference_expression(c, c.flip(2))), dtype
    assert PR.levels(np.array([-1.0, 1.0], dtype=np.float32)).tolist() == [0, 255]


def test_each_step_is_rounded_to_float32():
    """(v + 1) / 2 * 255 in float32 is not v * 127.5 + 127.5: the restatement follows the reference's grouping."""
    edges = PR.integer_edges()
    folded = np.trunc(np.clip(edges * np.float32(127.5) + np.float32(127.5), 0, 255)).astype(np.uint8)
    assert int((folded != PR.levels(edges)).sum()) > 0


def test_definitions_outside_the_reference_domain():
    inf = np.float32(np.inf)
    v = np.array([-1.5, -3.0, 1.5, 3.0, -inf, inf, np.nan, -0.0], dtype=np.float32)
    assert PR.levels(v).tolist() == [0, 0, 255, 255, 0, 255, 0, 127]
    # the reconstruction is clamped first: beyond +-1 and +-inf land on the ends, NaN on 0
    assert PR.levels(PR.clamp(v)).tolist() == [0, 0, 255, 255, 0, 255, 0, 127]
