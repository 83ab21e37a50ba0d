"""The gap-relative checker of the base and large bf16 tower gradients (tests/gap_bounds.py) must be able to see a wrong tile, a
dropped K edge and a dropped pass of a row kernel - with the bounds it ships (CPU, no GPU).

"got" is the unrounded float64 model's encoder gradient at the base size on SMALL (175 rows), the reference the rounded replay of the
bf16 tape: by construction one gap away from it, about where the HIP gradients sit.  The checker has to accept that and to reject it
with one error planted:

  (a) one interior 128 x 128 tile of layer 6's w12 gradient (32 x 6 tiles) scaled by 1.5 - a wrong split or tile of k_wgrad128_bf16;
  (b) the last 64 columns of a [1024, 2752] matrix zeroed (the 64-wide K edge of the large tower's w3: 2752 = 21 x 128 + 64), on a
      synthetic pair whose rounding gap is the base encoder's median matrix gap;
  (c) the last 256 entries of a gain's gradient zeroed: the last `f += 256` pass of the row kernels over d (the third at 768, the fourth
      at the large tower's 1024).

Each planted error is well above R x gap: (a) puts the tile at 0.50 against a bound of 3.0 x 3.1e-2 = 9.4e-2, (b) the 22 edge tiles at
1.0 against 3.0 x 2.5e-2, (c) the gain at 0.52 against 2.8 x 2.4e-2.  Resolution of the tile check (printed as MEASURED): the tile of
(a) is rejected from a scale of 1.10 on - a tile 10 % off shows, one 5 % off does not."""
import functools

import torch

from tests import bf16_tape as T
from tests import gap_bounds as G
from tests.blockwise import tile_errors

SMALL = ([(8, 64, 64), (4, 16, 16)], [40, 3])        # tests/test_hip_backward_shapes.SMALL
W12 = "encoder.model_layers.ffd_layer.6.w12.weight"
GAIN = "encoder.model_layers.ffd_layer.6.norm.weight"
TILE = (slice(15 * 128, 16 * 128), slice(3 * 128, 4 * 128))      # tile (15, 3) of 32 x 6


@functools.lru_cache(maxsize=None)
def _base_encoder():
    """(rounded replay, unrounded model): float64 gradients of the base encoder on SMALL under the linear loss of
    tests/test_hip_backward_bf16.py.  Read only."""
    from titok_video_amd.synthetic import seeded_titok_state, synthetic_clips
    shapes, counts = SMALL
    wz = torch.randn(sum(counts), 5, generator=torch.Generator().manual_seed(11))
    clips = synthetic_clips(shapes, seed=8, dtype=torch.bfloat16)
    state = seeded_titok_state(3, encoder_size="base", decoder_size="base", gain=3.0)
    params = {k: v.to(torch.bfloat16) for k, v in state.items() if k.startswith("encoder.")}
    ref, _ = T.encoder_grads(params, clips, counts, wz, "base", True)
    exact, _ = T.encoder_grads(params, clips, counts, wz, "base", False)
    return ref, exact


def _planted(name, plant):
    ref, exact = _base_encoder()
    got = dict(exact)
    got[name] = exact[name].clone()
    plant(got[name])
    return G.check_tower(got, ref, exact, "planted")[0]


def test_the_unplanted_gradients_are_accepted():
    ref, exact = _base_encoder()
    assert W12 in ref and tuple(ref[W12].shape) == (4096, 768) and tuple(ref[GAIN].shape) == (768,)
    bad, worst, per_layer, (glob, gap) = G.check_tower(dict(exact), ref, exact, "unplanted")
    print("MEASURED base encoder, model against replay: tower", f"{glob:.3e} gap {gap:.3e};",
          "; ".join(f"{c} worst ratio {r:.2f} ({f:.3e} / {g:.3e}, {n})" for c, (r, f, g, n) in worst.items()), flush=True)
    assert not bad, "\n".join(bad)
    assert set(per_layer) == set(range(12)) | {None}


def test_a_scaled_interior_tile_is_rejected():
    """(a), and the smallest scale of that tile the check rejects (1.10 with R["tile"] = 3.0)."""
    ref, exact = _base_encoder()
    bad = _planted(W12, lambda g: g[TILE].mul_(1.5))
    assert any(W12 in b and "tile" in b for b in bad), bad
    # resolution: the scale from which this tile alone exceeds R x the matrix's worst-tile gap
    bound = G.R["tile"] * G.tower_gaps(ref, exact)["tile"][W12]
    r, e = ref[W12][TILE], exact[W12][TILE]
    scale = next(s / 100 for s in range(100, 400) if float((s / 100 * e - r).norm() / r.norm()) > bound)
    print(f"MEASURED resolution of the tile check: tile (15, 3) of {W12} is rejected from a scale of {scale:.2f} (bound {bound:.3e}, "
          f"tile error unscaled {float((e - r).norm() / r.norm()):.3e})", flush=True)
    assert scale <= 1.5


def test_a_dropped_k_edge_is_rejected():
    """(b): synthetic [1024, 2752] pair, rounding gap = the base encoder's median matrix gap."""
    ref, exact = _base_encoder()
    gap = min(G.tower_gaps(ref, exact)["matrix"].values())          # floored at the median: the smallest is the median
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1024, 2752, generator=g, dtype=torch.float64)
    r = x + gap * torch.randn(1024, 2752, generator=g, dtype=torch.float64)          # the "rounded replay"
    got = r + gap * torch.randn(1024, 2752, generator=g, dtype=torch.float64)        # a third summation order, one gap away
    name = "synthetic.w3.weight"
    assert not G.check_tower({name: got}, {name: r}, {name: x}, "synthetic")[0]
    cut = got.clone()
    cut[:, 2688:] = 0
    bad = G.check_tower({name: cut}, {name: r}, {name: x}, "synthetic")[0]
    assert any("tile" in b for b in bad), bad
    err = tile_errors(cut, r)
    assert float(err[:, :21].max()) < G.R["tile"] * gap * 1.5 and float(err[:, 21].min()) > 0.99      # only the edge column is off


def test_a_dropped_pass_over_the_width_is_rejected():
    """(c)."""
    bad = _planted(GAIN, lambda g: g[512:].zero_())
    assert any(GAIN in b and "vector" in b for b in bad), bad


def test_r_is_twice_a_measured_ratio_that_needed_no_absorbing():
    """The convention of tests/gap_bounds.py, asserted: no recorded HIP / gap ratio reaches ABSORB_LIMIT (a larger one is a finding to
    localise, not a number to double), and every R is about twice (1.9 - 2.1 times) the ratio recorded for its class."""
    assert set(G.R) == set(G.MEASURED_WORST)
    for c, m in G.MEASURED_WORST.items():
        assert m < G.ABSORB_LIMIT, (c, m)
        assert 1.9 * m <= G.R[c] <= 2.1 * m, (c, m, G.R[c])
