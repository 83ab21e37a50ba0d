#!/usr/bin/env python3
"""JEDiMetric.update on 32 clip pairs of 3 x 16 x 128 x 128, bf16 (the benchmark batch), with seeded ViT-L/16 + probe weights: ms per
update (HIP events around a window of updates, after a warm-up) and the network's algorithmic FLOPs (24 (24 N d^2 + 4 N^2 d) per
clip, N = 1568, d = 1024) over that time as a fraction of the bf16 dense MFMA peak; a per-phase breakdown timed with the single-op
entry points at the update's shapes (GEMMs by shape, attention, LayerNorm, pooler, preprocess); and the same network restated in
torch (F.linear, F.scaled_dot_product_attention, F.layer_norm, F.gelu under bf16 autocast) on the same preprocessed rows, timed in the
same process.  Prints the relative L2 difference of the two feature sets.  GPU box only."""
import ctypes as C
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from titok_video_amd import _lib  # noqa: E402
from titok_video_amd.model.metrics import jedi as J  # noqa: E402
from titok_video_amd.synthetic import seeded_probe_state, seeded_vjepa_state, synthetic_clips  # noqa: E402

DEV = "cuda:0"
BF16_PEAK = 2.5e15
SHAPE, PAIRS, WARMUP, ITERS = (16, 128, 128), 32, 1, 3
N, D, H, DEPTH = J.TOKENS, J.WIDTH, J.HEADS, J.DEPTH


def timed(fn, iters=ITERS, warmup=WARMUP):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters   # ms


def torch_features(rows, enc, probe):
    """The network in torch eager, bf16 autocast: rows [n * 1568, 1536] bf16 -> [n, 1024] fp32."""
    n = rows.shape[0] // N
    with torch.autocast("cuda", dtype=torch.bfloat16):
        x = F.linear(rows, enc["pw"], enc["pb"]).float() + enc["pos"].repeat(n, 1)
        for L in enc["layers"]:
            h = F.layer_norm(x, (D,), L[0], L[1], 1e-6)
            qkv = F.linear(h, L[2], L[3]).view(n, N, 3, H, 64).permute(2, 0, 3, 1, 4)
            a = F.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2]).transpose(1, 2).reshape(n * N, D)
            x = x + F.linear(a, L[4], L[5])
            h = F.layer_norm(x, (D,), L[6], L[7], 1e-6)
            x = x + F.linear(F.gelu(F.linear(h, L[8], L[9])), L[10], L[11])
        y = F.layer_norm(x, (D,), enc["nw"], enc["nb"], 1e-6)
        h = F.layer_norm(y, (D,), probe["n1w"], probe["n1b"], 1e-5)
        kv = F.linear(h, probe["kvw"], probe["kvb"]).view(n, N, 2, H, 64).permute(2, 0, 3, 1, 4)
        q = F.linear(probe["qt"], probe["qw"], probe["qb"]).view(1, 1, H, 64).transpose(1, 2).expand(n, -1, -1, -1)
        a = F.scaled_dot_product_attention(q, kv[0], kv[1]).transpose(1, 2).reshape(n, D)
        z = probe["qt"] + F.linear(a, probe["pw"], probe["pb"])
        z = z + F.linear(F.gelu(F.linear(F.layer_norm(z, (D,), probe["n2w"], probe["n2b"], 1e-5), probe["f1w"], probe["f1b"])),
                         probe["f2w"], probe["f2b"])
    return z.float()


def main():
    torch.manual_seed(0)
    enc_sd, probe_sd = J.vjepa_state_dict(seeded_vjepa_state(DEPTH, 0)), J.probe_state_dict(seeded_probe_state(1))
    metric = J.JEDiMetric(weights=J.VJEPA(enc_sd, probe_sd))
    recon = synthetic_clips([SHAPE] * PAIRS, seed=1, dtype=torch.bfloat16, device=DEV)
    target = synthetic_clips([SHAPE] * PAIRS, seed=2, dtype=torch.bfloat16, device=DEV)
    metric.update_clips(recon, target)        # weights upload
    torch.cuda.synchronize()
    flop = 2 * PAIRS * DEPTH * (24 * N * D * D + 4 * N * N * D)
    ms = timed(lambda: metric.update_clips(recon, target))
    print(f"HIP: {ms:.2f} ms per update of {PAIRS} pairs, {flop / 1e12:.1f} TFLOP algorithmic -> {flop / (ms * 1e-3) / 1e12:.0f} TFLOP/s, "
          f"{flop / (ms * 1e-3) / BF16_PEAK:.3f} of the bf16 dense peak", flush=True)

    # ---- per phase, at the update's shapes (64 clips) ----
    m, n = metric.model, 2 * PAIRS
    M = n * N
    s = _lib.stream_ptr(DEV)
    lib = _lib.lib()
    x, ws = m._buffers(n)
    t = m.table
    L0 = m._layers[0]
    a16 = torch.randn(M, 4 * D, device=DEV).to(torch.bfloat16)
    r32 = torch.randn(M, D, device=DEV)
    y16 = torch.empty(M, 4 * D, dtype=torch.bfloat16, device=DEV)

    def lin(w, b, Nn, K, epi, resid=None, rows=0, ldy=None):
        return lambda: lib.ttv_vjepa_linear(a16.data_ptr(), K, w, K, b, M, Nn, K, epi, resid, Nn if resid else 0, rows,
                                            (r32 if epi == _lib.TTV_VJEPA_EPI_RESID else y16).data_ptr(), ldy or Nn, s)

    phases = []
    ph = [("preprocess", 1, lambda: m.preprocess(recon + target, x), 0),
          ("gemm patch 1024x1536 +pos", 1, lin(t.patch_w, t.patch_b, D, 1536, 2, t.pos_embed, N), 2 * M * D * 1536),
          ("gemm qkv 3072x1024", DEPTH, lin(L0.qkv_w, L0.qkv_b, 3 * D, D, 0), 2 * M * 3 * D * D),
          ("gemm proj 1024x1024 +res", DEPTH, lin(L0.proj_w, L0.proj_b, D, D, 2, r32.data_ptr()), 2 * M * D * D),
          ("gemm fc1 4096x1024 +gelu", DEPTH, lin(L0.fc1_w, L0.fc1_b, 4 * D, D, 1), 2 * M * 4 * D * D),
          ("gemm fc2 1024x4096 +res", DEPTH, lin(L0.fc2_w, L0.fc2_b, D, 4 * D, 2, r32.data_ptr()), 2 * M * 4 * D * D),
          ("gemm pooler kv 2048x1024", 1, lin(t.pool_kv_w, t.pool_kv_b, 2 * D, D, 0), 2 * M * 2 * D * D),
          ("layernorm", 2 * DEPTH + 1, lambda: lib.ttv_vjepa_layernorm(r32.data_ptr(), D, M, D, L0.norm1_w, L0.norm1_b, C.c_float(1e-6), None,
                                                                       None, C.c_float(0), None, 0, y16.data_ptr(), D, s), 0)]
    tab = torch.tensor([[c, qb * 128, h, 0] for c in range(n) for h in range(H) for qb in range(13)], dtype=torch.int32, device=DEV)
    cu = torch.arange(n + 1, dtype=torch.int32, device=DEV) * N
    ph.append(("attention 1568 x 16 heads", DEPTH, lambda: lib.ttv_attention(a16.data_ptr(), 4 * D, y16.data_ptr(), D, cu.data_ptr(),
                                                                             tab.data_ptr(), tab.shape[0], H, H, 64, 0, _lib.TTV_BF16, s),
               4 * M * N * D))
    ph.append(("pooler attention", 1, lambda: lib.ttv_vjepa_pool_attention(t.pool_q, a16.data_ptr(), n, N, y16.data_ptr(), s), 0))
    total = 0.0
    for name, times, fn, fl in ph:
        one = timed(fn, iters=5)
        total += one * times
        frac = f", {fl / (one * 1e-3) / BF16_PEAK:.3f} of peak" if fl else ""
        print(f"  {name:28s} {one:8.3f} ms x {times:2d} = {one * times:8.2f} ms{frac}", flush=True)
    print(f"  sum of phases {total:.2f} ms (update {ms:.2f} ms)", flush=True)

    # ---- torch eager restatement on the same rows ----
    bf = lambda k: enc_sd[k].to(DEV, torch.bfloat16)
    enc = {"pw": bf("patch_embed.proj.weight").reshape(D, -1), "pb": bf("patch_embed.proj.bias"),
           "pos": enc_sd["pos_embed"].reshape(N, D).to(DEV), "nw": enc_sd["norm.weight"].to(DEV), "nb": enc_sd["norm.bias"].to(DEV),
           "layers": [[enc_sd[f"blocks.{i}.{k}"].to(DEV) for k in ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias",
                                                                  "attn.proj.weight", "attn.proj.bias", "norm2.weight", "norm2.bias",
                                                                  "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")]
                      for i in range(DEPTH)]}
    for Ls in enc["layers"]:
        for j in (2, 3, 4, 5, 8, 9, 10, 11):
            Ls[j] = Ls[j].to(torch.bfloat16)
    p = "pooler.cross_attention_block."
    pg = lambda k, b16=True: probe_sd[p + k].to(DEV, torch.bfloat16 if b16 else torch.float32)
    probe = {"qt": probe_sd["pooler.query_tokens"].reshape(1, D).to(DEV), "qw": pg("xattn.q.weight"), "qb": pg("xattn.q.bias"),
             "n1w": pg("norm1.weight", False), "n1b": pg("norm1.bias", False), "kvw": pg("xattn.kv.weight"), "kvb": pg("xattn.kv.bias"),
             "pw": pg("xattn.proj.weight"), "pb": pg("xattn.proj.bias"), "n2w": pg("norm2.weight", False), "n2b": pg("norm2.bias", False),
             "f1w": pg("mlp.fc1.weight"), "f1b": pg("mlp.fc1.bias"), "f2w": pg("mlp.fc2.weight"), "f2b": pg("mlp.fc2.bias")}
    m.preprocess(recon + target, x)
    rows = x[:M].clone()
    with torch.no_grad():
        ft = torch_features(rows, enc, probe)
        ms_t = timed(lambda: torch_features(rows, enc, probe))
    fh = m.features([recon, target])
    rel = ((fh.double() - ft.double()).norm(dim=1) / ft.double().norm(dim=1)).max().item()
    print(f"torch bf16 eager: {ms_t:.2f} ms per update ({flop / (ms_t * 1e-3) / BF16_PEAK:.3f} of peak);  HIP / torch time {ms / ms_t:.3f};  "
          f"max relative L2 difference of the features {rel:.2e}", flush=True)


if __name__ == "__main__":
    main()
