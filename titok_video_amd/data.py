"""Synthetic clip stream + token-budget dynamic batching.

The reference's loaders decode real videos (decord, WebDataset shards: out of scope).  What the hot path sees from them is
a stream of batch dicts built by `_dynamic_batching` (reference dataset/video_dataset.py:130-172): clips of varying
(T,H,W) are appended, each with a latent-token count drawn from `token_range`, until adding the next clip would push the
packed sequence length  sum(grid_size + token_count)  past the budget (`train_seq_len` 6144 / `eval_seq_len` 4096,
configs/tiny.yaml:65-66); the batch is then emitted as
    {'video': [C,T,H,W tensors], 'fps': [...], '__key__': [...], 'token_counts': int32 tensor [B]}.
This module produces the same dicts from seeded synthetic clips, with rank-disjoint sharding for data parallelism
(the reference has no node split - SURVEY.md R4).

It also restates the front of the reference's loader, `_video_process` (video_dataset.py:38-127): `ClipSampling` holds the keys of
`training.sampling` it reads, `sample_chunks` makes its draws (chunk length, frame rate, output grid, crop box, flip) and returns the
geometry that `ttv_clip_resample_u8` executes on the device, and `resample_clip` is that call for one clip.
"""
from __future__ import annotations

import math
import random
from dataclasses import dataclass
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch


def sample_clip_shape(rng: random.Random, min_grid: Sequence[int], max_grid: Sequence[int], patch: Sequence[int],
                      max_aspect_ratio: float = 2.0) -> Tuple[int, int, int]:
    """(T,H,W) on the patch lattice inside [min_grid, max_grid] with max(H,W)/min(H,W) <= max_aspect_ratio
    (the sampling ranges of configs/tiny.yaml:56-62)."""
    for _ in range(1000):
        shape = tuple(rng.randrange(lo // p, hi // p + 1) * p for lo, hi, p in zip(min_grid, max_grid, patch))
        if max(shape[1], shape[2]) <= max_aspect_ratio * min(shape[1], shape[2]):
            return shape
    raise RuntimeError("no clip shape satisfies the sampling constraints")


class SyntheticClipStream:
    """Infinite (or `length`-bounded) stream of {'video', 'fps', '__key__'} samples.  Sample i belongs to rank i % world_size."""

    def __init__(self, min_grid=(8, 128, 128), max_grid=(16, 168, 168), patch=(4, 8, 8), fps_range=(3, 5), max_aspect_ratio=2.0,
                 dtype=torch.bfloat16, device="cpu", seed: int = 0, rank: int = 0, world_size: int = 1, length: Optional[int] = None):
        self.min_grid, self.max_grid, self.patch = tuple(min_grid), tuple(max_grid), tuple(patch)
        self.fps_range, self.max_aspect_ratio = tuple(fps_range), max_aspect_ratio
        self.dtype, self.device, self.seed, self.rank, self.world_size, self.length = dtype, device, seed, rank, world_size, length

    def __iter__(self) -> Iterator[Dict]:
        i = self.rank
        while self.length is None or i < self.length:
            rng = random.Random((self.seed << 20) + i)               # per-sample seed: any rank can regenerate any sample
            shape = sample_clip_shape(rng, self.min_grid, self.max_grid, self.patch, self.max_aspect_ratio)
            g = torch.Generator(device="cpu").manual_seed((self.seed << 20) + i)
            video = torch.rand((3, *shape), generator=g, dtype=torch.float32) * 2.0 - 1.0     # [-1, 1] (video_dataset.py:118-119)
            yield {"video": video.to(device=self.device, dtype=self.dtype), "fps": rng.uniform(*self.fps_range), "__key__": f"synthetic_{i:08d}"}
            i += self.world_size


@dataclass(frozen=True)
class ClipSampling:
    """The keys of `training.sampling` that `_video_process` reads, plus the tokenizer's `patch_size` (all grids are (T, H, W)).
    `min_scale` is the least share of the frame's area a training crop sees; upstream only configs/tiny_csv.yaml sets it (0.25)
    although both dataset files read it, so `from_config` falls back to that value when the key is absent."""
    min_grid: Tuple[int, int, int] = (8, 128, 128)
    max_grid: Tuple[int, int, int] = (16, 168, 168)
    fps_range: Tuple[int, int] = (3, 5)
    max_aspect_ratio: float = 2.0
    min_scale: float = 0.25
    patch_size: Tuple[int, int, int] = (4, 8, 8)

    def __post_init__(self):
        for name in ("min_grid", "max_grid", "fps_range", "patch_size"):
            object.__setattr__(self, name, tuple(int(v) for v in getattr(self, name)))
        if not (all(d % p == 0 for d, p in zip(self.min_grid, self.patch_size)) and all(d % p == 0 for d, p in zip(self.max_grid, self.patch_size))):
            raise ValueError("dimensions in min_grid and max_grid must be evenly divisible by their respective patch size")
        if not 0.0 < self.min_scale <= 1.0:
            raise ValueError(f"min_scale = {self.min_scale} must lie in (0, 1]")

    @classmethod
    def from_config(cls, config) -> "ClipSampling":
        cs = config.training.sampling
        return cls(min_grid=tuple(cs.min_grid), max_grid=tuple(cs.max_grid), fps_range=tuple(cs.fps_range),
                   max_aspect_ratio=float(cs.max_aspect_ratio), min_scale=float(getattr(cs, "min_scale", 0.25)),
                   patch_size=tuple(config.tokenizer.model.patch_size))


def resized_hw(h: int, w: int, size: int) -> Tuple[int, int]:
    """torchvision Resize(size=int): the short edge becomes `size`, the long edge int(size * long / short) (the rule
    model/losses/loss_module.py `_resized_hw` also restates)."""
    if w <= h:
        return int(size * h / w), size
    return size, int(size * w / h)


def random_resized_crop_box(rng: random.Random, height: int, width: int, scale: Tuple[float, float], ratio: float) -> Tuple[int, int, int, int]:
    """(top, left, h, w) as torchvision's RandomResizedCrop.get_params draws it at a FIXED aspect ratio (ratio = (r, r), what the
    reference passes): ten attempts of an area share uniform in `scale`, w = round(sqrt(area * r)), h = round(sqrt(area / r)), accepted
    when the box fits, with uniform integer offsets; then the central fallback (the largest box of that ratio)."""
    area = height * width
    for _ in range(10):
        target = area * rng.uniform(scale[0], scale[1])
        w = int(round(math.sqrt(target * ratio)))
        h = int(round(math.sqrt(target / ratio)))
        if 0 < w <= width and 0 < h <= height:
            return rng.randrange(0, height - h + 1), rng.randrange(0, width - w + 1), h, w
    in_ratio = float(width) / float(height)
    if in_ratio < ratio:
        w, h = width, int(round(width / ratio))
    elif in_ratio > ratio:
        h, w = height, int(round(height * ratio))
    else:
        w, h = width, height
    return (height - h) // 2, (width - w) // 2, h, w


def sample_chunks(rng: random.Random, in_grid: Sequence[int], in_fps: int, sampling: ClipSampling, eval: bool = False) -> Iterator[Dict]:
    """The chunks `_video_process` cuts out of one decoded video of `in_grid` = (frames, H, W) at `in_fps` (video_dataset.py:66-125).

    Same accept test (every dimension >= min_grid, in_fps >= min_fps), same `while` loop, the same four `randrange` draws in the same
    order from `rng` (chunk frames, chunk fps, chunk height, chunk width), `np.linspace(start, end - 1, n, dtype=int)` frame indices and
    `start = end + 1`.  Then the transform's own draws, from the same `rng`: training = RandomResizedCrop.get_params
    (`random_resized_crop_box`) and the flip coin; evaluation draws nothing.  torchvision draws those from torch's global generator
    and is not installed here: this matches its DISTRIBUTION, not its draws.  A `randrange` over an empty range (a grid the source
    cannot satisfy) ends the video, as the reference's `except` does.

    Yields {'indices': frame indices, 'fps', 'span': (start, end), 'out': (T, Ho, Wo), 'box': (top, left, h, w) of the source region
    to hand to the kernel (the crop in training, the whole frame in evaluation), 'geom': (T, h, w, Hr, Wr, oy, ox, Ho, Wo, flip) as
    ttv_clip_resample_u8 takes it for that region}."""
    min_grid, max_grid, patch = sampling.min_grid, sampling.max_grid, sampling.patch_size
    min_fps, max_fps = sampling.fps_range
    mar = sampling.max_aspect_ratio
    in_grid = [int(v) for v in in_grid]
    in_fps = int(in_fps)
    if not (all(x >= y for x, y in zip(in_grid, min_grid)) and in_fps >= min_fps):
        return
    start = 0
    while True:
        try:
            n = rng.randrange(min_grid[0], max_grid[0] + 1, patch[0])
            fps = rng.randrange(min_fps, min(max_fps, in_fps) + 1, 1)
            end = start + int(n * (in_fps / fps))
            if in_grid[0] < end:
                return
            ho = rng.randrange(min_grid[1], min(max_grid[1], in_grid[1]) + 1, patch[1])
            width_error = int(ho / mar) % patch[2]
            min_w = max(min_grid[2], int(ho / mar) - width_error)
            max_w = min(max_grid[2], in_grid[2], int(ho * mar))
            wo = rng.randrange(min_w, max_w + 1, patch[2])
        except ValueError:
            return
        indices = np.linspace(start, end - 1, n, dtype=int).tolist()
        if eval:
            hr, wr = resized_hw(in_grid[1], in_grid[2], max(ho, wo))
            box = (0, 0, in_grid[1], in_grid[2])
            geom = (n, in_grid[1], in_grid[2], hr, wr, int(round((hr - ho) / 2.0)), int(round((wr - wo) / 2.0)), ho, wo, 0)
        else:
            box = random_resized_crop_box(rng, in_grid[1], in_grid[2], (sampling.min_scale, 1.0), wo / ho)
            flip = 1 if rng.random() < 0.5 else 0
            geom = (n, box[2], box[3], ho, wo, 0, 0, ho, wo, flip)
        yield {"indices": indices, "fps": fps, "span": (start, end), "out": (n, ho, wo), "box": box, "geom": geom}
        start = end + 1


def resample_geoms(frames: Sequence[torch.Tensor], geoms: Sequence[Sequence[int]], dtype: torch.dtype, stream: int) -> List[torch.Tensor]:
    """ttv_clip_resample_u8 on device uint8 arrays [T,h,w,3] (contiguous) with their geometries, TTV_MAX_CLIPS_PER_LAUNCH clips per
    call: the clips [3,T,Ho,Wo] in `dtype`, allocated on the current stream's device."""
    from . import _lib
    code = _lib.dtype_code(dtype)
    clips = [torch.empty((3, int(g[0]), int(g[7]), int(g[8])), dtype=dtype, device=f.device) for f, g in zip(frames, geoms)]
    step = _lib.TTV_MAX_CLIPS_PER_LAUNCH
    for c0 in range(0, len(clips), step):
        flat = [int(v) for g in geoms[c0:c0 + step] for v in g]
        arr = (_lib.i32 * len(flat))(*flat)
        n = len(clips[c0:c0 + step])
        _lib.check(_lib.lib().ttv_clip_resample_u8(_lib.ptr_array(frames[c0:c0 + step]), _lib.ptr_array(clips[c0:c0 + step]), arr, n, code, stream), "ttv_clip_resample_u8")
    return clips


def resample_clip(frames_u8: torch.Tensor, out_hw: Tuple[int, int], box: Optional[Tuple[int, int, int, int]] = None, flip: bool = False,
                  eval: bool = False, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """One clip through ttv_clip_resample_u8, for users with their own loader: decoded frames uint8 [T,H,W,3] on the GPU -> [3,T,Ho,Wo] in
    `dtype`, [-1, 1].  Training form (default): the `box` = (top, left, h, w) of the frame (the whole frame when None) is resized to
    `out_hw` with the antialiased bicubic filter and mirrored when `flip`.  eval=True: Resize(max(out_hw)) + CenterCrop(out_hw) of the
    whole frame.  Runs on the current stream; there is no CPU path."""
    from . import _lib
    _lib.require_gpu(frames_u8, "resample_clip")
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
        raise ValueError(f"resample_clip: frames must be uint8 [T,H,W,3], got {frames_u8.dtype} {tuple(frames_u8.shape)}")
    t, h, w, _ = frames_u8.shape
    ho, wo = int(out_hw[0]), int(out_hw[1])
    if eval:
        if box is not None or flip:
            raise ValueError("resample_clip: the evaluation form takes neither a crop box nor a flip")
        hr, wr = resized_hw(h, w, max(ho, wo))
        src, geom = frames_u8, (t, h, w, hr, wr, int(round((hr - ho) / 2.0)), int(round((wr - wo) / 2.0)), ho, wo, 0)
    else:
        top, left, bh, bw = (0, 0, h, w) if box is None else (int(v) for v in box)
        if not (0 <= top and 0 <= left and bh > 0 and bw > 0 and top + bh <= h and left + bw <= w):
            raise ValueError(f"resample_clip: box {box} lies outside the {h} x {w} frame")
        src, geom = frames_u8[:, top:top + bh, left:left + bw], (t, bh, bw, ho, wo, 0, 0, ho, wo, int(bool(flip)))
    src = src.contiguous()
    with torch.cuda.device(frames_u8.device):
        return resample_geoms([src], [geom], dtype, _lib.stream_ptr(frames_u8.device))[0]


def dynamic_batches(samples, patch: Sequence[int], token_range: Sequence[int], max_seq_len: int, seed: int = 0,
                    max_grid: Optional[Sequence[int]] = None, device=None, drop_last: bool = False) -> Iterator[Dict]:
    """Token-budget batching with the reference's policy (video_dataset.py:130-172): never exceed `max_seq_len` packed rows.
    drop_last: the reference never emits the clips left over when the stream ends (its generator only yields when the NEXT clip
    would overflow the budget); True reproduces that, False (default, inference / tests) also emits the trailing partial batch."""
    if max_grid is not None and math.prod(x // y for x, y in zip(max_grid, patch)) + token_range[1] > max_seq_len:
        raise ValueError("max_grid/patch + token_range[1] must fit in max_seq_len")
    rng = random.Random(seed)
    chunk: List[Dict] = []
    counts: List[int] = []
    cur = 0
    for sample in samples:
        grid = math.prod(x // y for x, y in zip(sample["video"].shape[1:], patch))
        k = rng.randrange(token_range[0], token_range[1] + 1)
        if cur + grid + k > max_seq_len and chunk:
            yield _collate(chunk, counts, device)
            chunk, counts, cur = [], [], 0
        cur += grid + k
        chunk.append(sample)
        counts.append(k)
    if chunk and not drop_last:
        yield _collate(chunk, counts, device)


_control_groups: Dict = {}       # rank tuple of the data group (None = the world) -> gloo group


def _group_key(process_group):
    import torch.distributed as dist
    return None if process_group is None else tuple(dist.get_process_group_ranks(process_group))


def setup_control_group(process_group=None, force: bool = False):
    """COLLECTIVE over the WORLD: create (once) the CPU-side gloo group that carries the 8-byte control collectives of
    `process_group`.  `dist.new_group` must be entered by every rank of the default group, also by ranks outside `process_group`
    and by ranks that never iterate `equal_steps` (an evaluation-only rank) - so a program with sub-groups or such ranks calls this
    on every rank right after `init_process_group`.  When every rank of the world trains over the default group, `equal_steps`
    calls it lazily at its first step, which is then the same collective.  Cached by the group's RANK TUPLE (not `id()`, which a
    new group can reuse after the old one is collected); `drop_control_groups()` forgets them (call it before
    `destroy_process_group`)."""
    import torch.distributed as dist
    if dist.get_backend(process_group) == "gloo" and not force:
        return process_group
    key = _group_key(process_group)
    g = _control_groups.get(key)
    if g is None:
        g = _control_groups[key] = dist.new_group(ranks=list(key) if key is not None else None, backend="gloo")
    return g


def drop_control_groups() -> None:
    _control_groups.clear()


def _control_group(process_group=None, force: bool = False):
    """Under RCCL a flag all-reduce lives on the GPU and reading it back (`flag.item()`) drains everything the rank has queued - one
    host synchronisation per training step.  Control decisions go through gloo instead (`setup_control_group`): the host blocks for
    the other ranks' hosts only, the GPU queues stay full.  gloo groups are returned as they are."""
    return setup_control_group(process_group, force)


def equal_steps(batches: Iterator[Dict], process_group=None, _force_control_group: bool = False) -> Iterator[Dict]:
    """Data-parallel training loop guard: yield this rank's batches only while EVERY rank still has one.  Token-budget batching
    gives the ranks different numbers of batches for the same number of clips; the per-step gradient all-reduce must be entered
    by all ranks or by none, so the epoch ends (collectively) when the first rank runs out - one 8-byte all-reduce per step, on a
    CPU-side control group (no GPU synchronisation: `_control_group`)."""
    import torch.distributed as dist
    it = iter(batches)
    on = dist.is_available() and dist.is_initialized()
    ctl = _control_group(process_group, _force_control_group) if on else None
    while True:
        nxt = next(it, None)
        if on:
            flag = torch.tensor([0 if nxt is None else 1], dtype=torch.int64)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=ctl)
            if int(flag.item()) == 0:
                return
        elif nxt is None:
            return
        yield nxt


def _collate(chunk: List[Dict], counts: List[int], device) -> Dict:
    out = {k: [c[k] for c in chunk] for k in chunk[0].keys()}
    out["token_counts"] = torch.tensor(counts, dtype=torch.int32, device=device if device is not None else "cpu")
    return out
