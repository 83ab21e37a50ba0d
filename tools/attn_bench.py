#!/usr/bin/env python3
"""Attention kernel alone at the benchmark shape (32 sequences x 1152 rows, 4 q-heads / 2 kv-heads, head_dim 64): launch time by
torch events over back-to-back launches, TFLOP/s against the MFMA peak, and the error against an fp64 reference on two sequences.
GPU box only.    python tools/attn_bench.py [spread ...]   (spread = std of the score exponents; default 1.5 6)
PV8=1 adds the opt-in e4m3 P.V kernel (ttv_attention_pv8) as three rows - its V pre-pass alone, the attention launch alone, the two
back to back - and ROUNDS=n repeats the whole variant list n times in this process (alternations of one box, same inputs)."""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from titok_video_amd import _lib  # noqa: E402
from titok_video_amd.plan import BatchPlan  # noqa: E402

DEV = torch.device("cuda:0")
lib = _lib.lib()
ST = _lib.stream_ptr(DEV)
B, HQ, HKV, D = int(os.environ.get("B", "32")), int(os.environ.get("HQ", "4")), int(os.environ.get("HKV", "2")), 64
CLIP = tuple(int(v) for v in os.environ.get("CLIP", "16,128,128").split(","))
KTOK = int(os.environ.get("K", "128"))
plan = BatchPlan([CLIP] * B, [KTOK] * B, (4, 8, 8), DEV)
L, S = plan.total_rows, plan.total_rows // B
dm, g = HQ * D, HKV * D
ld = 2 * dm + 2 * g
table = plan.attention_table(HQ, HKV)
table64 = plan.attention_table64(HQ, HKV)
W64 = 1 << 20          # tool-local marker: run ttv_attention64 (the 64-rows-per-wave kernel)
PV8_QUANT, PV8_ATTN = 1 << 21, 1 << 22      # tool-local markers: ttv_quant_v_pv8 / ttv_attention_pv8 (either or both)
pv8_image = torch.empty(max(int(lib.ttv_attention_pv8_bytes(L, B, HKV)), 16), dtype=torch.uint8, device=DEV)
C_EXP = 0.125 * 1.4426950408889634


def reference(qkv, seqs, prescaled):
    out = {}
    for b in seqs:
        x = qkv[b * S:(b + 1) * S].double()
        q, gate, k, v = x[:, :dm], x[:, dm:2 * dm], x[:, 2 * dm:2 * dm + g], x[:, 2 * dm + g:]
        o = torch.empty(S, dm, dtype=torch.float64, device=DEV)
        for hh in range(HQ):
            kv = hh // (HQ // HKV)
            s = q[:, hh * D:(hh + 1) * D] @ k[:, kv * D:(kv + 1) * D].T
            p = torch.softmax(s * (math.log(2.0) if prescaled else 0.125), dim=-1)
            o[:, hh * D:(hh + 1) * D] = p @ v[:, kv * D:(kv + 1) * D]
        out[b] = o * torch.sigmoid(gate)
    return out


def run(dtype, flags, qkv, iters=30):
    out = torch.empty(L, dm, dtype=dtype, device=DEV)
    code = _lib.dtype_code(dtype)

    def call():
        if flags & (PV8_QUANT | PV8_ATTN):
            if flags & PV8_QUANT:
                _lib.check(lib.ttv_quant_v_pv8(qkv.data_ptr(), ld, plan.cu_dev.data_ptr(), B, L, HQ, HKV, pv8_image.data_ptr(), ST), "quant_v_pv8")
            if flags & PV8_ATTN:
                _lib.check(lib.ttv_attention_pv8(qkv.data_ptr(), ld, out.data_ptr(), dm, plan.cu_dev.data_ptr(), table.data_ptr(), table.shape[0],
                                                 HQ, HKV, D, 1 | 4, pv8_image.data_ptr(), ST), "attention_pv8")
            return
        if flags & W64:
            _lib.check(lib.ttv_attention64(qkv.data_ptr(), ld, out.data_ptr(), dm, plan.cu_dev.data_ptr(), table64.data_ptr(),
                                           table64.shape[0], HQ, HKV, D, flags & ~W64, code, ST), "attention64")
            return
        _lib.check(lib.ttv_attention(qkv.data_ptr(), ld, out.data_ptr(), dm, plan.cu_dev.data_ptr(), table.data_ptr(), table.shape[0],
                                     HQ, HKV, D, flags, code, ST), "attention")
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters, out


spreads = [float(a) for a in sys.argv[1:]] or [1.5, 6.0]
flops = B * 4.0 * S * S * dm
print(f"shape: {B} x {S} rows, {HQ}/{HKV} heads, table {table.shape[0]} entries (w64: {table64.shape[0]} workgroups), {flops / 1e9:.1f} GFLOP per launch")
for spread in spreads:
    gen = torch.Generator(device="cpu").manual_seed(7)
    base = torch.randn(L, ld, generator=gen)
    if os.environ.get("ZERO", "0") == "1":      # clock probe: all-zero operands draw less power, the part holds a higher clock (rule 25)
        base.zero_()
    # score exponent std = |q||k| terms: q, k ~ N(0, a^2) -> q.k std = 8 a^2; exponent = q.k * C_EXP
    a = math.sqrt(spread / (8.0 * C_EXP))
    base[:, :dm] *= a
    base[:, 2 * dm:2 * dm + g] *= a
    all_full = 8 if not bool((table[:, 3] > 0).any()) else 0
    variants = [(torch.bfloat16, "bf16 gate", 1, False), (torch.bfloat16, "bf16 gate+qscaled", 1 | 4, True)]
    if os.environ.get("W64", "0") == "1":
        variants.append((torch.bfloat16, "bf16 gate+qscaled w64", 1 | 4 | W64, True))
    if all_full:
        variants.append((torch.bfloat16, "bf16 gate+qscaled swp", 1 | 4 | 8, True))        # k_attn_swp (round 5, the default for such tables)
        if os.environ.get("PIPE", "0") == "1":
            variants.append((torch.bfloat16, "bf16 gate+qscaled pipe", 1 | 4 | 8 | 16, True))
    if os.environ.get("FP32", "0") == "1":
        variants.append((torch.float32, "fp32 gate", 1, False))
    if os.environ.get("PV8", "0") == "1":
        variants += [(torch.bfloat16, "pv8 V pre-pass alone", PV8_QUANT, True), (torch.bfloat16, "pv8 pre-pass + attention", PV8_QUANT | PV8_ATTN, True),
                     (torch.bfloat16, "pv8 attention alone", PV8_ATTN, True)]       # (alone: on the image the row above left)
    for dtype, name, flags, pre in variants * int(os.environ.get("ROUNDS", "1")):
        x = base.clone()
        if pre:
            x[:, :dm] *= C_EXP
        qkv = x.to(DEV, dtype).contiguous()
        us, out = run(dtype, flags, qkv, iters=30 if dtype == torch.bfloat16 else 8)
        if flags & PV8_QUANT and not flags & PV8_ATTN:
            print(f"spread {spread:4.1f} {name:24s} {us:8.1f} us", flush=True)
            continue
        ref = reference(qkv, (0, B - 1), pre)
        err = max(float((out[b * S:(b + 1) * S].double() - r).abs().max()) for b, r in ref.items())
        rel = max(float((out[b * S:(b + 1) * S].double() - r).norm() / r.norm()) for b, r in ref.items())
        peak = 2500.0 if dtype == torch.bfloat16 else 157.3
        print(f"spread {spread:4.1f} {name:24s} {us:8.1f} us  {flops / us / 1e6:8.1f} TFLOP/s = {flops / us / 1e6 / peak:.3f} of peak   "
              f"max abs err {err:.2e}  rel {rel:.2e}", flush=True)
