"""Seeded inputs and float64 references of tests/test_hip_fp8_blocks.py, built on the CPU (no GPU needed:
tests/test_mx_cases_cpu.py evaluates the no-floored-tile condition and the expected tile heights on the same inputs the GPU tests
launch).

The fp8 GEMMs (`ttv_linear_fp8` row-scaled, `ttv_linear_fp8_mx` block-scaled) take quantised operands, so a case IS its quantised
operands: x and w are drawn here, quantised here (oracle/fp8_oracle.py for MX; `rows_quantize` below restates
ttv_quant_rows_fp8: scale = max|row| / 448, e4m3 round to nearest even) and the GPU test uploads these bytes.  The reference is the
float64 product of the dequantised operands with the row factors and the float64 epilogue on top (exact erf GELU, the rotary of
oracle/titok_oracle.py apply_rotary restated in float64).

Shapes: the smallest that reach each kernel variant.  The token-tile height follows ttv_gemm.hip gemm_token_tile (`token_tile`
restates it; every case names the height it expects, so a changed rule fails loudly):

  store / residual   (4097, 2048, 768): 16 feature tiles x 33 token tiles = 528 > 512 slots -> 160-token tiles, last tile 97 rows,
                     6 k-tiles (the MX scale prefetch runs); M = 300 and M = 1 at the same N, K -> 128-token tiles
  qkv + rotary       d = 768, g = 256 (N = 2048), K = 768: M = 4097 (160) and M = 300 (128); the rotary table belongs to QKV_PLANS
  GEGLU              N = I = 2048, K = 768: M = 2049 (32 x 17 = 544 blocks -> 160, last tile 129 rows), M = 300 and M = 1 (128)
  long K (MX only)   (129, 768, 2048), store and residual: 16 k-tiles = four scale dwords per lane

The layer restatement at the end (mx_layer_weights / mx_stack / encoder_front) also serves the plain bf16 wide layer: with the quantiser
off, bf16 weights and the fold switch it is what tests/wide_cases.py compares the truncated towers with.
"""
import functools
from typing import NamedTuple

import torch

from oracle import fp8_oracle as F
from oracle import titok_oracle as O
from tests import forward_cases as FC

ALPHA = 24.0          # the residual case's alpha (what a 12-layer KEEL tower passes)
D_MODEL, GQA = 768, 256


class Case(NamedTuple):
    flavour: str      # "rows" (ttv_linear_fp8) | "mx" (ttv_linear_fp8_mx)
    epi: str          # "store" | "qkv" | "geglu" | "resid"
    M: int
    N: int
    K: int
    tile: int         # expected token-tile height


EPI_CODE = {"store": 0, "qkv": 1, "geglu": 2, "resid": 3}
GEMM_CASES = (
    [Case(f, "store", M, 2048, 768, t) for f in ("rows", "mx") for M, t in ((4097, 160), (300, 128), (1, 128))]
    + [Case("mx", "resid", M, 2048, 768, t) for M, t in ((4097, 160), (300, 128), (1, 128))]
    + [Case(f, "qkv", M, 2048, 768, t) for f in ("rows", "mx") for M, t in ((4097, 160), (300, 128))]
    + [Case(f, "geglu", M, 2048, 768, t) for f in ("rows", "mx") for M, t in ((2049, 160), (300, 128), (1, 128))]
    + [Case("mx", e, 129, 768, 2048, 128) for e in ("store", "resid")]
)
# clips whose packed rows give the M of the qkv cases (the kernel's rotary table comes from a BatchPlan)
QKV_PLANS = {4097: ([(16, 128, 128)] * 3 + [(16, 64, 64)], [128] * 3 + [385]), 300: ([(16, 64, 64)], [44])}
# the GEGLU producer of part B: the two tile heights of part A's MX cases and the smallest launch there is
GEGLU_Q_CASES = [Case("mx", "geglu", 2049, 2048, 768, 160), Case("mx", "geglu", 300, 2048, 768, 128), Case("mx", "geglu", 1, 256, 128, 128)]


def case_id(c: Case) -> str:
    return f"{c.flavour}-{c.epi}-{c.M}x{c.N}x{c.K}"


def cdiv(a, b):
    return -(-a // b)


def token_tile(M: int, N: int, epi: str) -> int:
    """ttv_gemm.hip gemm_token_tile restated: rounds of 512 resident blocks x tile height; 160 where that saves a round."""
    nf = cdiv(N, 64 if epi == "geglu" else 128)
    cost = {t: cdiv(nf * cdiv(M, t), 512) * t for t in (128, 160)}
    return 160 if cost[160] < cost[128] else 128


def planted(M: int):
    """forward_cases.planted_rows where the matrix has room for them; a one-row launch carries none."""
    return FC.planted_rows(M) if M >= 32 else {}


def rows_quantize(x):
    """ttv_quant_rows_fp8 without the norm: (e4m3 bytes [rows, K], fp32 scale per row = max|row| / 448, 1 for an all-zero row)."""
    xf = x.float()
    amax = xf.abs().amax(1)
    sc = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    return (xf / sc[:, None]).to(torch.float8_e4m3fn).view(torch.uint8), sc


def rows_dequantize(q, sc):
    return q.view(torch.float8_e4m3fn).double() * sc.double()[:, None]


def rotary64(x, cos, sin):
    """oracle/titok_oracle.py apply_rotary in float64 (that function computes in float32 whatever it is given): x [L, H * 64], the first
    cos.shape[1] (re, im) pairs of every 64-wide head are rotated, the rest stay."""
    L, R = x.shape[0], cos.shape[1]
    p = x.double().reshape(L, -1, 32, 2).clone()
    c, s = cos.double()[:, None, :], sin.double()[:, None, :]
    re, im = p[..., :R, 0].clone(), p[..., :R, 1].clone()
    p[..., :R, 0] = re * c - im * s
    p[..., :R, 1] = re * s + im * c
    return p.reshape(L, -1)


def qkv_rope_table(M: int):
    shapes, counts = QKV_PLANS[M]
    grids = [[v // p for v, p in zip(s, FC.PATCH)] for s in shapes]
    cos, sin = O.rope_table(grids, counts)
    assert cos.shape[0] == M, (cos.shape, M)
    return cos, sin


def _seed(c: Case) -> int:
    return 7 * c.M + 3 * c.N + c.K + 1000 * EPI_CODE[c.epi] + (500 if c.flavour == "mx" else 0)


def _spread(g, r, K):
    """Block maxima spread over 2^+-6 per (row, block of 32)."""
    return torch.exp2(torch.randint(-6, 7, (r, K // 32), generator=g).float()).repeat_interleave(32, 1)


@functools.lru_cache(maxsize=4)
def operands(c: Case):
    """The quantised operands of one case (CPU tensors): x / w as drawn (bf16, rows planted in x before quantisation), xq / wq e4m3
    bytes, MX: xe / we E8M0 [rows, K / 32] and the fp32 row factors xrs (None in the residual case) / wrs; row-scaled: xs / ws;
    resid (bf16) in the residual case; `planted` {row: kind}."""
    g = torch.Generator().manual_seed(_seed(c))
    wrows = 2 * c.N if c.epi == "geglu" else c.N
    pl = planted(c.M)
    out = {"planted": pl}
    if c.flavour == "mx":
        x = FC.plant(torch.randn(c.M, c.K, generator=g) * _spread(g, c.M, c.K), pl).to(torch.bfloat16)
        w = (torch.randn(wrows, c.K, generator=g) * _spread(g, wrows, c.K) * c.K ** -0.5).to(torch.bfloat16)
        out["xq"], out["xe"], _ = F.mx_quantize(x)
        out["wq"], out["we"], out["wrs"] = F.mx_quantize(w, True)
        out["xrs"] = None if c.epi == "resid" else (0.5 + torch.rand(c.M, generator=g))
    else:
        x = FC.plant(torch.randn(c.M, c.K, generator=g) * torch.rand(c.M, 1, generator=g) * 5, pl).to(torch.bfloat16)
        w = (torch.randn(wrows, c.K, generator=g) * c.K ** -0.5).to(torch.bfloat16)
        out["xq"], out["xs"] = rows_quantize(x)
        out["wq"], out["ws"] = rows_quantize(w)
    out["x"], out["w"] = x, w
    if c.epi == "resid":
        # alpha * resid ~ 100 next to a product of a few hundred: neither term drowns the other
        out["resid"] = (torch.randn(c.M, c.N, generator=g) * 4.0).to(torch.bfloat16)
    return out


def accumulator(c: Case):
    """float64 [M, w rows]: the product of the dequantised operands with both row factors - what the kernel hands its epilogue."""
    o = operands(c)
    if c.flavour == "mx":
        xd = F.mx_dequantize(o["xq"], o["xe"], o["xrs"])
        wd = F.mx_dequantize(o["wq"], o["we"], o["wrs"])
    else:
        xd, wd = rows_dequantize(o["xq"], o["xs"]), rows_dequantize(o["wq"], o["ws"])
    return xd @ wd.T


@functools.lru_cache(maxsize=2)
def reference(c: Case):
    """float64 [M, N]: `accumulator` through the case's float64 epilogue."""
    u = accumulator(c)
    if c.epi == "store":
        return u
    if c.epi == "resid":
        return ALPHA * operands(c)["resid"].double() + u
    if c.epi == "geglu":
        return torch.nn.functional.gelu(u[:, c.N:]) * u[:, :c.N]        # float64, exact erf
    cos, sin = qkv_rope_table(c.M)
    d, gq = D_MODEL, GQA
    assert c.N == 2 * d + 2 * gq
    return torch.cat([rotary64(u[:, :d], cos, sin), u[:, d:2 * d], rotary64(u[:, 2 * d:2 * d + gq], cos, sin), u[:, 2 * d + gq:]], 1)


def floored_tiles(ref, planted_rows, rows: int = 16, cols: int = 64):
    """First rows of the 16 x 64 tiles of `ref` that are under the floor of blockwise.block_errors with the planted rows taken out -
    except tiles that hold planted rows only (those are measured by check_rows).  A case is valid when this is empty."""
    from tests.blockwise import floored_blocks
    r = ref.clone()
    r[list(planted_rows)] = 0.0
    low = floored_blocks(r, [0, r.shape[0]], r.shape[1] // cols, rows).any(1)
    return [rows * t for t in torch.nonzero(low).flatten().tolist()
            if not all(row in planted_rows for row in range(rows * t, min(rows * t + rows, r.shape[0])))]


# ---------------------------------------------------------------------------------------------- part B: the post-norm producer
NORM_WIDTHS = [128, 256, 768, 1024]
NORM_ROWS = [1, 7, 131]
NORM_EPS = 1e-5
POW2_ROW, POW2_A = 6, 5      # row 6 (where there is one): every element +-2^5, so mean(x^2) + eps rounds to 2^10 and rstd is exactly 2^-5


def norm_inputs(rows: int, width: int, gains: str):
    """x fp32 [rows, width] and gain fp32 [width] of one post-norm case.  Rows whose 32-element blocks lie 1e-4 .. 1e4 apart; row 3
    all-zero, row 5 with an all-zero block, row 6 every element +-2^5 (each where the case has that row).
    gains "pow2": 448 * 2^k with k per block in -6 .. 5 - with row 6 the stored values are exactly +-448 * 2^k, so every block maximum
    / 448 is an exact power of two (the "keeps its exponent" branch of the scale rule); "random": 1 +- 0.1."""
    g = torch.Generator().manual_seed(rows * 31 + width + (1 if gains == "pow2" else 0))
    x = torch.randn(rows, width, generator=g) * torch.exp(4 * torch.randn(rows, width // 32, generator=g)).repeat_interleave(32, 1)
    if rows > 3:
        x[3] = 0
    if rows > 5:
        x[5, 32:64] = 0
    if rows > POW2_ROW:
        x[POW2_ROW] = 2.0 ** POW2_A * (2 * torch.randint(0, 2, (width,), generator=g).float() - 1)
    if gains == "pow2":
        gain = 448.0 * torch.exp2(torch.randint(-6, 6, (width // 32,), generator=g).float()).repeat_interleave(32)
    else:
        gain = 1 + 0.1 * torch.randn(width, generator=g)
    return x, gain


def norm_stored(x, gain, out_dtype=torch.bfloat16):
    """k_rmsnorm's row as stored, in its own arithmetic (fp32: sum of squares / width + eps, 1 / sqrt, x * rstd * gain, one rounding).
    Used on the CPU for the power-of-two row only; the GPU test takes the plain launch's output as the twin."""
    xf = x.float()
    rstd = 1.0 / torch.sqrt(xf.pow(2).sum(1, keepdim=True) / xf.shape[1] + NORM_EPS)
    return (xf * rstd * gain.float()).to(out_dtype)


# ---------------------------------------------------------------------------------------------- part D: run_layer_mx restated in float64
def _mx(t):
    """F.mx_dequantize(F.mx_quantize(t)): the values a block-scaled e4m3 activation operand stands for, float64."""
    q, e, _ = F.mx_quantize(t)
    return F.mx_dequantize(q, e)


def _norm64(t, gain=None, eps=O.RMS_EPS):
    y = t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + eps)
    return y if gain is None else y * gain


def identity(t):
    return t


def bf16_round(t):
    return t.to(torch.bfloat16).double()


def mx_layer_weights(sd, prefix, layers, width, quant: bool, last_plain: bool, bf16_all: bool = False, fold: bool = True):
    """Per layer the four float64 weights run_layer_mx multiplies by: W' = to_qkv * pre_ln gain with the q rows times
    head_dim^-0.5 * log2(e), w12 * ffd_norm gain, out_proj, w3 - formed in fp32 as the weight pack forms them (blocks.py f8_mx), then
    quant: the values of their block-scaled images with row factors (tests/test_hip_fp8_blocks.py pins those images to the pack's);
    the last layer under `last_plain` (the encoder's, which runs off the MX path on its latent rows): rounded to bf16 instead - the
    folded weights to_qkv_pn / w12_pn and the plain out_proj / w3.  quant False: W' itself (the oracle's stack, re-associated).
    bf16_all (the plain bf16 wide layer, tests/wide_cases.py): every layer's weights rounded to bf16, no image anywhere.  fold False
    (TTV_FOLD_NORMS=0): the gains stay out of the weights - to_qkv with the q factor on its q rows (to_qkv_qs) and w12 as they are,
    the gains under "g_qkv" / "g_w12" for the stand-alone norms."""
    out = []
    for i in range(layers):
        ap, fp = f"{prefix}attn_layer.{i}.", f"{prefix}ffd_layer.{i}."
        gq, gf = sd[ap + "pre_ln.weight"].float(), sd[fp + "norm.weight"].float()
        wqkv = sd[ap + "to_qkv.weight"].float() * gq[None, :] if fold else sd[ap + "to_qkv.weight"].float().clone()
        wqkv[:width] *= FC.C_EXP
        w = {"qkv": wqkv, "wo": sd[ap + "out_proj.weight"].float(), "w12": sd[fp + "w12.weight"].float() * gf[None, :] if fold else sd[fp + "w12.weight"].float(),
             "w3": sd[fp + "w3.weight"].float()}
        plain = bf16_all or (last_plain and i == layers - 1)
        if (quant or bf16_all) and plain:
            w = {k: v.to(torch.bfloat16).double() for k, v in w.items()}
        elif quant:
            w = {k: F.mx_dequantize(*F.mx_quantize(v, True)) for k, v in w.items()}
        else:
            w = {k: v.double() for k, v in w.items()}
        w["plain"] = plain or not quant
        if not fold:
            w["g_qkv"], w["g_w12"] = gq.double(), gf.double()
        out.append(w)
    return out


def mx_stack(x, weights, sd, prefix, layers, heads, cos, sin, cu, rnd, alpha=None):
    """run_layer_mx (csrc/ttv_api.hip) layer by layer in float64: every linear on mx(operand) x image, rstd applied AFTER the product,
    the q factor inside the image and the softmax 2^(q . k), layer 0 without post-norms.  `rnd` (identity or bf16_round) stands at each
    point where the HIP path stores bf16; the ttv_api.hip line of the launch that stores is named.
    With plain weights (mx_layer_weights quant False or bf16_all) this is the plain bf16 wide layer of run_layers: prenorm_proj's
    folded route (the statistic is that of x as it stands - under bf16_round the stored row, which is what k_row_rstd reads and what
    k_rmsnorm's next_rstd is taken from) and keel_tail.  Weights without the fold ("g_qkv" / "g_w12" present): the stand-alone pre-norm
    writes the normalised copy xn (one more store), then the plain weight.  alpha: what keel_alpha sees for layers >= 1 (the module's
    2 x its full depth, whatever depth runs); None: 2 x layers."""
    from tests.blockwise import attention_forward_reference
    hq, hkv = heads
    d = x.shape[1]
    g = d // hq * hkv
    a_keel = 2.0 * layers if alpha is None else float(alpha)
    for i, w in enumerate(weights):
        q8 = identity if w["plain"] else _mx
        alpha = 1.0 if i == 0 else a_keel
        if "g_qkv" in w:
            u = rnd(_norm64(x, w["g_qkv"])) @ w["qkv"].T                                 # prenorm_proj, no fold: ws.xn
        else:
            rstd = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + O.RMS_EPS)
            u = (q8(x) @ w["qkv"].T) * rstd
        qkv = rnd(torch.cat([rotary64(u[:, :d], cos, sin), u[:, d:2 * d], rotary64(u[:, 2 * d:2 * d + g], cos, sin), u[:, 2 * d + g:]], 1))  # :138 ws.qkv
        ao = rnd(attention_forward_reference(qkv, cu, hq, hkv, c_exp=FC.C_EXP)[1])       # :142 / :147 the gated output, before its quantisation
        x = rnd(alpha * x + q8(ao) @ w["wo"].T)                                          # :151 in place on ws.x
        if i > 0:
            x = rnd(_norm64(x, sd[f"{prefix}attn_post_ln.{i - 1}.weight"].double()))     # :153
        if "g_w12" in w:
            u = rnd(_norm64(x, w["g_w12"])) @ w["w12"].T
        else:
            rstd = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + O.RMS_EPS)
            u = (q8(x) @ w["w12"].T) * rstd
        inner = u.shape[1] // 2
        h = rnd(torch.nn.functional.gelu(u[:, inner:]) * u[:, :inner])                   # :165 h, before its quantisation
        x = rnd(alpha * x + q8(h) @ w["w3"].T)                                           # :168 in place on ws.x
        if i > 0:
            x = rnd(_norm64(x, sd[f"{prefix}ffd_post_ln.{i - 1}.weight"].double()))      # :172
    return x


def encoder_front(videos, token_counts, sd, size="base", rnd=identity, patch=FC.PATCH, prefix="encoder."):
    """The oracle's encoder up to the stack, float64: (x [L, width], cos, sin, cu_seqlens, latent-row mask)."""
    width, _layers, heads = O.model_dims(size)
    grids, sizes, counts, cu, mask = O.batch_metadata([v.shape[1:] for v in videos], token_counts, patch)
    cos, sin = O.rope_table(grids, counts, width // heads[0])
    D = lambda name: sd[prefix + name].double()
    mt = D("mask_token")
    p = torch.cat([O.patchify(v.double(), patch) for v in videos], 0)
    p = rnd(rnd(p @ D("proj_in.weight").T + D("proj_in.bias")) + mt)              # :752 the GEMM's store (Linear output in dtype, + mask_token)
    x = torch.zeros(mask.shape[0], width, dtype=torch.float64)
    x[mask] = rnd(_norm64(mt.expand(-1, width), D("ln_pre_t.weight")))            # :756
    x[~mask] = rnd(_norm64(p, D("ln_pre_p.weight")))                              # :753
    return x, cos, sin, cu, mask


def mx_encoder_forward(videos, token_counts, sd, size="base", rnd=identity, quant=True, patch=FC.PATCH, prefix="encoder."):
    """oracle encoder_forward with the stack replaced by mx_stack (the last layer on plain weights), float64.  Returns z [sum K, C]."""
    width, layers, heads = O.model_dims(size)
    x, cos, sin, cu, mask = encoder_front(videos, token_counts, sd, size, rnd, patch, prefix)
    D = lambda name: sd[prefix + name].double()
    w = mx_layer_weights(sd, prefix + "model_layers.", layers, width, quant, last_plain=True)
    x = mx_stack(x, w, sd, prefix + "model_layers.", layers, heads, cos, sin, cu, rnd)
    t = rnd(_norm64(x[mask], D("ln_post.weight")))                                # :761 k_enc_tail: ln_post output in dtype, z stays fp32
    return t @ D("proj_out.weight").T + D("proj_out.bias")


def mx_decoder_forward(tokens, token_counts, pixel_grids, sd, size="base", rnd=identity, quant=True, patch=FC.PATCH, prefix="decoder."):
    """oracle decoder_forward with mx_stack, float64.  Returns the patch rows [sum P, C * pt * ph * pw] in the oracle's (pt, ph, pw, c)
    order (before unpatchify: rows to measure in 64-row blocks) and the patch count of every clip."""
    width, layers, heads = O.model_dims(size)
    grids, sizes, counts, cu, mask = O.batch_metadata(pixel_grids, token_counts, patch)
    cos, sin = O.rope_table(grids, counts, width // heads[0])
    D = lambda name: sd[prefix + name].double()
    mt = D("mask_token")
    h = rnd(rnd(tokens.double() @ D("proj_in.weight").T + D("proj_in.bias")) + mt)    # :829 k_dec_embed
    x = torch.zeros(mask.shape[0], width, dtype=torch.float64)
    x[mask] = rnd(_norm64(h, D("ln_pre_t.weight")))                               # :829
    x[~mask] = rnd(_norm64(mt.expand(-1, width), D("ln_pre_p.weight")))           # :830
    w = mx_layer_weights(sd, prefix + "model_layers.", layers, width, quant, last_plain=False)
    x = mx_stack(x, w, sd, prefix + "model_layers.", layers, heads, cos, sin, cu, rnd)
    p = rnd(_norm64(x[~mask], D("ln_post.weight")))                               # :842
    return rnd(p @ D("proj_out.weight").T + D("proj_out.bias")), sizes            # :852
