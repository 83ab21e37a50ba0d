#!/usr/bin/env python3
"""The two logging paths of the trainer against what the reference runs in their place, in one process on one GPU:

  recon_panels      train.recon_panels (ttv_recon_panels_u8 + one uint8 device-to-host copy) against the reference's eager expression
                    (train.py:141-142: cat / clamp / permute / .cpu().float().numpy(), then the numpy pass), per clip as the reference
                    runs it; 16 clips of 16 x 128 x 128 bf16.  Wall time per call (both end on the host), and the launch alone by
                    HIP events with its bytes over time - rotating over working sets larger than the Infinity Cache (an HBM
                    rate), and on one set (cache-warm).
  grad_norm_dict    train.grad_norm_dict over the tiny tokenizer's parameters - through optimizer.param_grad_norms() (gradients
                    re-read) and from the sums of a clip_and_step(want_param_norms=True) that has just run - against a loop of
                    p.grad.norm(2) per parameter with one .cpu() of the stacked norms (Lightning's grad_norm).
  norms launch      ttv_opt_param_norms alone on a chunk table of the base configs' size (20 480 chunks).
  ema update        ttv_opt_ema_update (ema.WeightEMA.update: fp32 shadows += w (parameter - shadow), one launch) alone, by HIP events, on
                    the tiny tokenizer's parameter list (rotating over working sets larger than the Infinity Cache, as a training step
                    between two updates leaves it) and on the base-size table, fp32 and bf16 parameters: us and the GB/s they imply
                    at 12 / 10 bytes per element - against the eager form on fp32 tensors in the same run,
                    torch._foreach_mul_(shadows, decay) + torch._foreach_add_(shadows, params, alpha=1 - decay).
  ema exchange      ttv_opt_ema_exchange on the same tables: apply (backup = p, p = cast shadow: 16 / 10 bytes per element) and
                    restore (p = backup: 8 / 4 bytes per element).

Reported, not gated.  GPU box only; writes what it prints to the file given as the first argument, if any."""
import ctypes as C
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from titok_video_amd import _lib  # noqa: E402
from titok_video_amd.model.titok import TiTok  # noqa: E402
from titok_video_amd.optim import HipAdamW  # noqa: E402
from titok_video_amd.synthetic import seeded_titok_state  # noqa: E402
from titok_video_amd.train import grad_norm_dict, recon_panels  # noqa: E402

DEV = "cuda:0"
SHAPE, CLIPS, WARMUP, ITERS = (3, 16, 128, 128), 16, 3, 20
SETS = 8                      # working sets of the rotated panel launch: 8 x 75.5 MB = 576 MiB
BIG_CHUNKS = 20480            # chunks of 8192 elements in ~168 M parameters: the base-size tower pair
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def wall(fn):
    """µs per call, host clock, the device idle before and after (every fn here ends with its result on the host)."""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ITERS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / ITERS


def events(fn, iters=ITERS):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def eager_panels(target, recon):
    out = []
    for y, x in zip(target, recon):
        merged = torch.cat((y, x.clamp(-1, 1)), dim=-1).permute(1, 0, 2, 3).cpu().float().numpy()
        out.append(((merged + 1) / 2 * 255).astype(np.uint8))
    return out


def bench_panels():
    g = torch.Generator(device=DEV).manual_seed(0)
    target = [(torch.rand(SHAPE, generator=g, device=DEV) * 2 - 1).to(torch.bfloat16) for _ in range(CLIPS)]
    recon = [(t.float() + 0.3 * torch.randn(SHAPE, generator=g, device=DEV)).to(torch.bfloat16) for t in target]
    same = all(np.array_equal(a, b) for a, b in zip(recon_panels(target, recon), eager_panels(target, recon)))
    us_hip, us_eager = wall(lambda: recon_panels(target, recon)), wall(lambda: eager_panels(target, recon))
    n = 2 * target[0].numel()
    nbytes = CLIPS * (2 * 2 * target[0].numel() + n)
    stream = _lib.stream_ptr(torch.device(DEV))
    dims = (C.c_int32 * (3 * CLIPS))(*(list(SHAPE[1:]) * CLIPS))
    # the launch alone, twice: on ONE working set (75.5 MB: it stays in the 256 MiB Infinity Cache between launches), and rotating
    # over SETS working sets (more than twice the cache: every launch reads and writes HBM)
    sets = []
    for k in range(SETS):
        t = target if k == 0 else [x.clone() for x in target]
        r = recon if k == 0 else [x.clone() for x in recon]
        out = torch.empty(CLIPS * n, dtype=torch.uint8, device=DEV)
        sets.append((t, r, out, _lib.ptr_array(t), _lib.ptr_array(r), (C.c_void_p * CLIPS)(*[out.data_ptr() + j * n for j in range(CLIPS)])))
    turn = [0]

    def launch(rotate):
        _, _, _, tp, rp, op = sets[turn[0] % SETS if rotate else 0]
        turn[0] += 1
        _lib.check(_lib.lib().ttv_recon_panels_u8(tp, rp, dims, CLIPS, _lib.TTV_BF16, op, stream), "ttv_recon_panels_u8")
    us_warm, us_hbm = events(lambda: launch(False)), events(lambda: launch(True))
    say(f"recon_panels  {CLIPS} x {SHAPE} bf16: HIP {us_hip:9.1f} us per call, eager expression {us_eager:9.1f} us per call "
        f"({us_eager / us_hip:.1f}x), same bytes: {same}")
    say(f"              the launch alone, {nbytes / 1e6:.1f} MB read + written: {us_hbm:7.1f} us = {nbytes / us_hbm / 1e6:.2f} TB/s rotating over "
        f"{SETS} working sets ({SETS * nbytes / 2 ** 20:.0f} MiB, from HBM); {us_warm:7.1f} us = {nbytes / us_warm / 1e6:.2f} TB/s on one set (cache-warm)")


def eager_grad_norms(module):
    norms = {f"grad_2.0_norm/{name}": p.grad.data.norm(2) for name, p in module.named_parameters() if p.grad is not None}
    host = torch.stack(list(norms.values())).cpu()
    out = dict(zip(norms, host.tolist()))
    out["grad_2.0_norm_total"] = float(host.norm(2))
    return out


def bench_norms():
    cfg = SimpleNamespace(tokenizer=SimpleNamespace(model=SimpleNamespace(patch_size=[4, 8, 8], fsq_levels=[7, 5, 5, 5, 5], encoder_size="tiny",
                                                                          decoder_size="tiny")))
    model = TiTok(cfg)
    model.load_state_dict(seeded_titok_state(0), strict=True)
    model = model.to(DEV, torch.bfloat16)
    g = torch.Generator(device=DEV).manual_seed(1)
    params = [p for p in model.parameters() if p.requires_grad]
    for p in params:
        p.grad = torch.randn(p.shape, generator=g, device=DEV).to(p.dtype)
    opt = HipAdamW(params, lr=0.0)
    a, b = grad_norm_dict(model, opt), eager_grad_norms(model)
    worst = max(abs(a[k] - b[k]) / max(abs(b[k]), 1e-30) for k in b)
    us_fresh = wall(lambda: grad_norm_dict(model, opt))

    def stepped():
        opt.clip_and_step(1.0, want_param_norms=True)
        return grad_norm_dict(model, opt, reuse=True)
    us_step_with = wall(stepped)
    us_step_without = wall(lambda: (opt.clip_and_step(1.0), torch.cuda.synchronize()))
    us_eager = wall(lambda: eager_grad_norms(model))
    say(f"grad_norm_dict {len(params)} parameters, {sum(p.numel() for p in params) / 1e6:.2f} M elements bf16: largest relative "
        f"difference from the eager loop (whose norms are rounded to bf16) {worst:.1e}")
    say(f"              grad_norm_dict (takes the norms itself) {us_fresh:9.1f} us; eager p.grad.norm(2) loop + one copy {us_eager:9.1f} us "
        f"({us_eager / us_fresh:.1f}x)")
    say(f"              clip_and_step(want_param_norms=True) + grad_norm_dict(reuse=True) {us_step_with:9.1f} us; clip_and_step alone + sync {us_step_without:9.1f} us: "
        f"the log adds {us_step_with - us_step_without:.1f} us to a step")


def bench_norms_launch_at_base_size():
    """ttv_opt_param_norms alone on a table the size of the base configs': BIG_CHUNKS chunks over 300 entries, the largest holding
    a tenth of them.  The bucket total is one lane's chain over all chunks: this is what that costs."""
    n_entries = 300
    big = BIG_CHUNKS // 10
    per = (BIG_CHUNKS - big) // (n_entries - 1)
    owners = [0] * big
    for e in range(1, n_entries):
        owners += [e] * per
    owners += [n_entries - 1] * (BIG_CHUNKS - len(owners))
    chunks = torch.tensor([[e, 0] for e in owners], dtype=torch.int32, device=DEV)
    partials = torch.rand(BIG_CHUNKS, device=DEV) * 8192
    norms = torch.empty(n_entries + 1, device=DEV)
    stream = _lib.stream_ptr(torch.device(DEV))
    us = events(lambda: _lib.check(_lib.lib().ttv_opt_param_norms(chunks.data_ptr(), chunks.data_ptr(), BIG_CHUNKS, n_entries, partials.data_ptr(),
                                                                  norms.data_ptr(), stream), "ttv_opt_param_norms"))
    want = float(partials.double().sum().sqrt())
    say(f"ttv_opt_param_norms alone, {BIG_CHUNKS} chunks ({BIG_CHUNKS * 8192 / 1e6:.0f} M elements) over {n_entries} entries, the largest {big} chunks: "
        f"{us:7.1f} us per launch (bucket norm {float(norms[-1]):.6g}, float64 {want:.6g})")


def ema_tables(sizes, dtype, sets):
    """`sets` independent working sets over tensors of `sizes` elements: parameters of `dtype`, fp32 shadows, backups of `dtype`, each
    family carved from one flat buffer (every tensor starts on a 16-byte boundary), with the device entry table and chunk list."""
    offs, total = [], 0
    for n in sizes:
        offs.append(total)
        total += (n + 7) // 8 * 8
    chunk_words = [i | (first << 32) for i, n in enumerate(sizes) for first in range(0, n, 8192)]
    chunks = torch.tensor(chunk_words, dtype=torch.int64).to(DEV)
    out = []
    for _ in range(sets):
        p = (torch.randn(total, device=DEV) * 0.5).to(dtype)
        sh = p.float() + 0.01
        bk = torch.empty_like(p)
        words = []
        for n, o in zip(sizes, offs):
            words += [p.data_ptr() + o * p.element_size(), 0, sh.data_ptr() + 4 * o, bk.data_ptr() + o * p.element_size(), n]
        out.append({"p": p, "shadow": sh, "backup": bk, "table": torch.tensor(words, dtype=torch.int64).to(DEV),
                    "views": [(p[o:o + n], sh[o:o + n]) for n, o in zip(sizes, offs)]})
    return out, chunks, len(chunk_words)


def bench_ema():
    """ttv_opt_ema_update / ttv_opt_ema_exchange alone and the eager foreach form, at the tiny tokenizer's table and at base size."""
    cfg = SimpleNamespace(tokenizer=SimpleNamespace(model=SimpleNamespace(patch_size=[4, 8, 8], fsq_levels=[7, 5, 5, 5, 5], encoder_size="tiny",
                                                                          decoder_size="tiny")))
    tiny = [p.numel() for p in TiTok(cfg).parameters()]
    n_entries, big = 300, BIG_CHUNKS // 10
    per = (BIG_CHUNKS - big) // (n_entries - 1)
    base = [big * 8192] + [per * 8192] * (n_entries - 2) + [(BIG_CHUNKS - big - per * (n_entries - 2)) * 8192]
    lib, stream, decay = _lib.lib(), _lib.stream_ptr(torch.device(DEV)), 0.9999
    for name, sizes in (("tiny tokenizer", tiny), ("base size", base)):
        elements = sum(sizes)
        for dtype in (torch.float32, torch.bfloat16):
            item = 4 if dtype == torch.float32 else 2
            # the working sets together exceed twice the 256 MiB Infinity Cache: every launch reads and writes HBM
            sets = max(1, -(-(2 * 256 * 2 ** 20) // (elements * (8 + item))))
            tabs, chunks, n_chunks = ema_tables(sizes, dtype, sets)
            code, turn = _lib.dtype_code(dtype), [0]
            iters = 10 * ITERS if sets > 1 else ITERS          # launches of tens of microseconds: a longer window

            def pick():
                turn[0] += 1
                return tabs[turn[0] % sets]

            def update():
                t = pick()
                _lib.check(lib.ttv_opt_ema_update(t["table"].data_ptr(), chunks.data_ptr(), n_chunks, code, 1.0 - decay, stream), "ttv_opt_ema_update")

            def exchange(mode):
                t = pick()
                _lib.check(lib.ttv_opt_ema_exchange(t["table"].data_ptr(), chunks.data_ptr(), n_chunks, code, mode, stream), "ttv_opt_ema_exchange")
            tag = f"{name}, {'fp32' if item == 4 else 'bf16'} parameters: {len(sizes)} tensors, {elements / 1e6:.2f} M elements, {n_chunks} chunks, {sets} working set(s), {iters} launches timed"
            us = events(update, iters)
            say(f"ema update    {tag}: {us:8.1f} us per launch = {elements * (8 + item) / us / 1e3:7.1f} GB/s at {8 + item} bytes per element")
            us0 = events(lambda: exchange(0), iters)
            us1 = events(lambda: exchange(1), iters)
            say(f"ema exchange  {tag}: apply {us0:8.1f} us = {elements * (4 + 3 * item) / us0 / 1e3:7.1f} GB/s at {4 + 3 * item} bytes per element; "
                f"restore {us1:8.1f} us = {elements * 2 * item / us1 / 1e3:7.1f} GB/s at {2 * item}")
            if dtype == torch.float32:
                def eager():
                    t = pick()
                    shadows, params = [v[1] for v in t["views"]], [v[0] for v in t["views"]]
                    torch._foreach_mul_(shadows, decay)
                    torch._foreach_add_(shadows, params, alpha=1.0 - decay)
                us_e = events(eager, iters)
                say(f"ema eager     {tag}: _foreach_mul_ + _foreach_add_ {us_e:8.1f} us per update ({us_e / us:.2f}x the launch; it moves "
                    f"{elements * 20 / 1e6:.0f} MB: {elements * 20 / us_e / 1e3:7.1f} GB/s at 20 bytes per element)")
            del tabs
            torch.cuda.empty_cache()


if __name__ == "__main__":
    say(f"device: {torch.cuda.get_device_name(0)}; wall times over {ITERS} calls after {WARMUP}")
    bench_panels()
    bench_norms()
    bench_norms_launch_at_base_size()
    bench_ema()
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(LINES) + "\n")
