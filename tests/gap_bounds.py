"""Bounds for the bf16 tower gradients stated in units of the rounding gap (CPU, no GPU; imported by
tests/test_hip_backward_bf16.py, checked by tests/test_backward_sizes_cpu.py).

tests/test_hip_backward_bf16.py holds the tiny (4 layers) and small (8 layers) towers to absolute constants measured at those depths.
The distance it measures - HIP gradient against the float64 replay of the bf16 tape - sits at about one *gap*, the distance between
that replay and the unrounded float64 model, because the rounded tape is chaotic (that module's docstring); and the gap grows with
depth.  For the base (12 layers) and large (24 layers) towers every quantity is therefore held to R x its own gap, both sides of which
come from the CPU alone:

  class         quantity                                                   gap
  matrix        a weight matrix's gradient, whole                          ||replay - model|| / ||model|| of that matrix
  tile          its worst 128 x 128 tile (tests/blockwise.tile_errors)     the worst tile of replay against model, same matrix
  vector        a gain, bias or mask token                                 as matrix
  clip_block    input-clip gradient per 64 patch rows                      the same block of replay against model
  clips, codes  input-clip / code gradient, whole                          as matrix
  tower         all parameters of a tower together                         bf16_tape.global_distance(replay, model)

A gap below the median gap of its class (in that tower and case) is raised to the median: a tile or gain whose two CPU replays happen
to agree says nothing about how far a third summation order lands.

R per class: about twice the worst HIP / gap ratio of the first MI355X run of the base and large towers on SMALL (175 rows), the
margin convention of tests/test_hip_backward_bf16.py; the measured ratios stand next to each R.  A ratio above ABSORB_LIMIT is not to
be absorbed into R: the tiny and small towers sit at 0.64 - 1.12 of their gap, and twice the worst of those is where "chaotic at
about one gap" stops being an explanation."""
import re
import statistics

import torch

from oracle import titok_oracle as O
from tests import bf16_tape as T
from tests.blockwise import block_errors, global_error, tile_errors

#                      measured worst figure / gap: base encoder, base decoder, large encoder, large decoder
R = {
    "matrix": 2.5,      # 1.08, 1.16, 1.19, 1.23 (large decoder, layer 11 to_qkv)
    "tile": 3.0,        # 1.06, 1.38, 1.44, 1.47 (large decoder, layer 10 to_qkv: tile 0.180 against a gap of 0.123)
    "vector": 2.8,      # 1.09, 1.37, 1.38 (large encoder, mask_token), 1.32
    "clip_block": 2.0,  # 1.01, -, 1.02, -
    "clips": 2.0,       # 0.84, -, 0.99, -
    "codes": 2.0,       # -, 0.95, -, 1.01
    "tower": 2.3,       # 0.80, 1.07, 1.03, 1.17 (tiny and small: 0.64 - 1.12)
}
MEASURED_WORST = {"matrix": 1.23, "tile": 1.47, "vector": 1.38, "clip_block": 1.02, "clips": 0.99, "codes": 1.01, "tower": 1.17}
# (tests/test_backward_sizes_cpu.py holds every figure of MEASURED_WORST under ABSORB_LIMIT and every R at about twice its figure)
# Worst ratio per layer grows slowly with depth: base encoder 0.84 (layer 0) -> 1.09 (layer 10), base decoder 1.06 -> 1.38 (layer 9),
# large encoder 1.07 -> 1.44 (layer 22), large decoder 1.15 -> 1.47 (layer 10).  Nothing reaches ABSORB_LIMIT.
ABSORB_LIMIT = 2.24
PATCH = (4, 8, 8)


def is_matrix(t) -> bool:
    return t.dim() == 2 and min(t.shape) > 1


def layer_of(name: str):
    """Layer index of a tower parameter (the post-norms `*_post_ln.{i}` follow layer i + 1), None for the tower's own parameters."""
    m = re.search(r"\.(attn_layer|ffd_layer|attn_post_ln|ffd_post_ln)\.(\d+)\.", name)
    if not m:
        return None
    return int(m.group(2)) + (1 if m.group(1).endswith("post_ln") else 0)


def floored(gaps: dict) -> dict:
    """Every gap of one class, raised to the class's median."""
    if not gaps:
        return {}
    med = statistics.median(gaps.values())
    return {k: max(v, med) for k, v in gaps.items()}


def tower_gaps(ref: dict, exact: dict) -> dict:
    """{"matrix" | "tile" | "vector": {name: floored gap}, "tower": gap} of one tower: ref the rounded replay's gradients, exact the
    unrounded model's."""
    g = {"matrix": {}, "tile": {}, "vector": {}}
    for n, r in ref.items():
        if is_matrix(r):
            g["matrix"][n] = global_error(r, exact[n])
            g["tile"][n] = float(tile_errors(r, exact[n]).max())
        else:
            g["vector"][n] = global_error(r, exact[n])
    out = {k: floored(v) for k, v in g.items()}
    out["tower"] = T.global_distance(ref, exact)
    return out


def check_tower(got: dict, ref: dict, exact: dict, what: str, R: dict = R):
    """One tower's parameter gradients `got` against the rounded replay `ref`, every figure held to R x its gap (tower_gaps).
    Returns (failures, worst, per_layer, tower): failures a list of messages (empty: accepted); worst {class: (ratio, figure, gap,
    name)} the largest figure / gap ratio of each class; per_layer {layer index or None: worst ratio of any class}; tower (global
    error, gap)."""
    assert set(got) == set(ref) == set(exact), what
    gaps = tower_gaps(ref, exact)
    bad, worst, per_layer = [], {}, {}

    def hold(cls, name, fig, gap):
        ratio = fig / gap
        worst[cls] = max(worst.get(cls, (0.0, 0.0, 0.0, "")), (ratio, fig, gap, name))
        if cls != "tower":
            per_layer[layer_of(name)] = max(per_layer.get(layer_of(name), 0.0), ratio)
        if not fig <= R[cls] * gap:            # also catches a NaN figure
            bad.append(f"{what} {name}: {cls} error {fig:.3e} > {R[cls]} x gap {gap:.3e} (ratio {ratio:.2f})")

    for n, r in ref.items():
        g = got[n]
        if not bool(torch.isfinite(g.double()).all()):
            bad.append(f"{what} {n}: non-finite values")
            continue
        if is_matrix(r):
            hold("matrix", n, global_error(g, r), gaps["matrix"][n])
            hold("tile", n, float(tile_errors(g, r).max()), gaps["tile"][n])
        else:
            hold("vector", n, global_error(g, r), gaps["vector"][n])
    glob = T.global_distance(got, ref)
    hold("tower", what, glob, gaps["tower"])
    return bad, worst, per_layer, (glob, gaps["tower"])


def _patch_rows(clips):
    return torch.cat([O.patchify(c, PATCH) for c in clips])


def check_clips(got, ref, exact, shapes, what: str, R: dict = R):
    """Input-clip gradients (lists of [3, T, H, W]) per 64 patch rows and whole.  Returns (failures, {class: (ratio, figure, gap)})."""
    gp, rp, ep = _patch_rows(got), _patch_rows(ref), _patch_rows(exact)
    cu = [0]
    for s in shapes:
        cu.append(cu[-1] + (s[0] // PATCH[0]) * (s[1] // PATCH[1]) * (s[2] // PATCH[2]))
    bad = []
    if not bool(torch.isfinite(gp.double()).all()):
        return [f"{what} clip gradients: non-finite values"], {}
    fig = block_errors(gp, rp, cu, 1).flatten()
    gap = block_errors(rp, ep, cu, 1).flatten()
    gap = gap.clamp_min(float(gap.median()))
    ratio = fig / gap
    b = int(ratio.argmax())
    worst = {"clip_block": (float(ratio[b]), float(fig[b]), float(gap[b]))}
    if not float(ratio[b]) <= R["clip_block"]:
        bad.append(f"{what} clip gradients: block {b}: error {float(fig[b]):.3e} > {R['clip_block']} x gap {float(gap[b]):.3e}")
    whole, wgap = global_error(gp, rp), global_error(rp, ep)
    worst["clips"] = (whole / wgap, whole, wgap)
    if not whole <= R["clips"] * wgap:
        bad.append(f"{what} clip gradients: error {whole:.3e} > {R['clips']} x gap {wgap:.3e}")
    return bad, worst


def check_codes(got, ref, exact, what: str, R: dict = R):
    fig, gap = global_error(got, ref), global_error(ref, exact)
    bad = [] if fig <= R["codes"] * gap else [f"{what} code gradients: error {fig:.3e} > {R['codes']} x gap {gap:.3e}"]
    return bad, {"codes": (fig / gap, fig, gap)}
