"""Seeded inputs, float64 references and reference-only rounding models of tests/test_hip_wide_layer.py, built on the CPU (no GPU
needed: tests/test_wide_cases_cpu.py evaluates their conditions on the same inputs the GPU tests launch).

The layer under test is the plain bf16 layer of the towers of width 512 / 768 / 1024 ("small" / "base" / "large"; run_layers with
gen_ok in csrc/ttv_api.hip): the pre-norm gain folded into to_qkv_pn / w12_pn, the row statistic rsqrt(mean(x^2) + eps) multiplying the
GEMM's accumulator rows (GemmArgs.row_scale), the statistic from k_row_rstd or from the KEEL post-norm's next_rstd, the residual sums
stored in place on x.  tests/mx_cases.py mx_stack with the quantiser off and bf16 weights IS that layer in float64; it is used, not copied.

Rows: row r of every activation operand is scaled by 2^((r % 7) - 3), so neighbouring rows' statistics lie a factor of two apart and a
statistic read one row off is a 2 x error in that row.  Planted rows (x 100, x 1e-3, all-zero; `planted`): the first three rows, the
last row of the first token tile of each height (127, 159, 255), three in the middle and the last three.

Shapes: the smallest that reach every tile edge.  M = 129 / 161 / 257 leave a one-row last tile under a full 128- / 160- / 256-token
tile; 300 and 1 025 are ragged under several tiles; M = 1 is the smallest launch.  inner = 1376 (width 512) is no multiple of 64: the
GEGLU kernel's last feature tile is ragged, the 256 x 256 kernel (128 GEGLU features per tile) cannot take it and neither 2752."""
import functools
from typing import NamedTuple

import torch

from oracle import titok_oracle as O
from tests import forward_cases as FC
from tests import mx_cases as MC

EPS = O.RMS_EPS
WIDTHS = [512, 768, 1024]
SIZE = {512: "small", 768: "base", 1024: "large"}
GQA = {512: 128, 768: 256, 1024: 256}
INNER = {512: 1376, 768: 2048, 1024: 2752}
MS = [1, 129, 161, 257, 300, 1025]
TILES = (128, 160, 256)                    # token-tile heights of k_gemm_bf16_dma<.., 4>, <.., 5> and k_gemm_bf16_t256
KINDS = [100.0, 1e-3, 0.0]
# clips whose packed rows give M (the rotary table of the to_qkv epilogue comes from a BatchPlan); patches of (4, 8, 8) pixels
QKV_PLANS = {1: ([(4, 8, 8)], [0]), 129: ([(4, 64, 128)], [1]), 161: ([(4, 64, 128)], [33]), 257: ([(4, 128, 128)], [1]),
             300: ([(16, 64, 64)], [44]), 1025: ([(16, 128, 128)], [1])}


def row_factors(rows: int):
    return torch.exp2((torch.arange(rows) % 7 - 3).float())


def planted(M: int):
    """{row: kind}: rows 0, 1, 2; the last row of the first token tile of every height that is not the launch's last rows anyway;
    M // 2 .. M // 2 + 2; M - 3 .. M - 1.  The kinds rotate group by group.  A launch under 32 rows carries none."""
    if M < 32:
        return {}
    out = {}
    groups = [[0, 1, 2], [M // 2, M // 2 + 1, M // 2 + 2], [M - 3, M - 2, M - 1]]
    for n, rows in enumerate(groups):
        for i, r in enumerate(rows):
            out[r] = KINDS[(i + n) % 3]
    for n, t in enumerate(TILES):
        if t - 1 < M - 3:
            assert t - 1 not in out
            out[t - 1] = KINDS[n % 3]
    return out


def scaled_rows(g, rows, width, plant=True):
    """bf16 [rows, width]: N(0, 1) x 2^((r % 7) - 3) per row, the planted rows on top."""
    x = torch.randn(rows, width, generator=g) * row_factors(rows)[:, None]
    return FC.plant(x, planted(rows) if plant else {}).to(torch.bfloat16)


def rstd64(x, eps=EPS):
    """float64 rsqrt(mean(x^2) + eps) per row."""
    return torch.rsqrt(x.double().pow(2).mean(-1) + eps)


def rstd_bound(width: int) -> float:
    """Relative bound of an fp32 row statistic: `width` fp32 additions by the project's rule (sqrt(width) x 2^-24, twice: the 2 x of
    tests/test_hip_ops.py assert_tiles with f32_terms) plus the division by width, the eps addition, the square root and the reciprocal."""
    return (2.0 * width ** 0.5 + 4.0) * 2.0 ** -24


# ---------------------------------------------------------------------------------------------- A: the row-scaled GEMMs
class Case(NamedTuple):
    epi: str          # "store" | "qkv" | "geglu"
    width: int        # K = d_model
    M: int


EPI_CODE = {"store": 0, "qkv": 1, "geglu": 2}
GEMM_CASES = [Case(e, w, M) for e in ("store", "qkv", "geglu") for w in WIDTHS for M in MS]
PADDED_LDY = {Case("store", 512, 300), Case("qkv", 768, 161), Case("geglu", 512, 257)}      # ldy = N + 8, one case per epilogue


def case_id(c: Case) -> str:
    return f"{c.epi}-{c.width}-M{c.M}"


def out_features(c: Case) -> int:
    return {"store": c.width, "qkv": 2 * c.width + 2 * GQA[c.width], "geglu": INNER[c.width]}[c.epi]


def t256_takes(c: Case) -> bool:
    """launch() of ttv_gemm.hip: the 256 x 256 kernel serves N % 256 == 0 (GEGLU: N % 128 == 0), K % 64 == 0, K >= 128."""
    return out_features(c) % (128 if c.epi == "geglu" else 256) == 0


def pad64(t):
    """[M, N] with zero columns appended up to a multiple of 64: N = 1376 ends in a 32-column tile, which is then measured on its own
    like a ragged last row tile (zeros add to neither the error nor the norm)."""
    return torch.nn.functional.pad(t, (0, -t.shape[1] % 64))


def qkv_rope_table(M: int):
    shapes, counts = QKV_PLANS[M]
    grids = [[v // p for v, p in zip(s, FC.PATCH)] for s in shapes]
    cos, sin = O.rope_table(grids, counts)
    assert cos.shape[0] == M, (cos.shape, M)
    return cos, sin


def qkv_blocks(width: int):
    """Column ranges q | gate | k | v of a to_qkv output: q and k take the rotary branch of the epilogue, gate and v the plain one."""
    d, g = width, GQA[width]
    return {"q": (0, d), "gate": (d, 2 * d), "k": (2 * d, 2 * d + g), "v": (2 * d + g, 2 * d + 2 * g)}


@functools.lru_cache(maxsize=4)
def operands(c: Case):
    """x bf16 [M, K] (scaled rows, planted), w bf16 [N or 2N, K], row_scale fp32 [M] = the statistic of x (1 / sqrt(eps) for an
    all-zero row), planted {row: kind}."""
    g = torch.Generator().manual_seed(11 * c.M + c.width + 1000 * EPI_CODE[c.epi])
    N, K = out_features(c), c.width
    x = scaled_rows(g, c.M, K)
    w = (torch.randn(2 * N if c.epi == "geglu" else N, K, generator=g) * K ** -0.5).to(torch.bfloat16)
    return {"x": x, "w": w, "row_scale": rstd64(x).float(), "planted": planted(c.M)}


@functools.lru_cache(maxsize=2)
def reference(c: Case):
    """float64 [M, N]: (x @ W^T) * row_scale[:, None] through the float64 epilogue (rotary of the oracle restated in float64, exact erf
    GELU)."""
    o = operands(c)
    u = (o["x"].double() @ o["w"].double().T) * o["row_scale"].double()[:, None]
    if c.epi == "store":
        return u
    if c.epi == "geglu":
        N = out_features(c)
        return torch.nn.functional.gelu(u[:, N:]) * u[:, :N]
    cos, sin = qkv_rope_table(c.M)
    b = qkv_blocks(c.width)
    return torch.cat([MC.rotary64(u[:, slice(*b["q"])], cos, sin), u[:, slice(*b["gate"])], MC.rotary64(u[:, slice(*b["k"])], cos, sin),
                      u[:, slice(*b["v"])]], 1)


# ---------------------------------------------------------------------------------------------- B: the two producers of the statistic
STAT_ROWS = [1, 3, 4, 5, 130]              # k_row_rstd and k_rmsnorm take four rows per block
STAT_PADDED = (5, 768)                     # (rows, width) of the case whose ldx is width + 8 with NaN in the padding columns
ZERO_ROW = 2


def stat_inputs(rows: int, width: int):
    """fp32 [rows, width] for ttv_row_rstd (the bf16 case rounds it): scaled rows, row 2 all-zero where there is one."""
    g = torch.Generator().manual_seed(rows * 37 + width)
    x = torch.randn(rows, width, generator=g) * row_factors(rows)[:, None]
    if rows > ZERO_ROW:
        x[ZERO_ROW] = 0
    return x


def norm_inputs(rows: int, width: int):
    """x bf16 [rows, width] and gain fp32 [width] of the in-place post-norm.  Row 0 is +-4 throughout and every gain lies in
    [1.001, 1.003]: the unrounded output of row 0 is +-gain (1 - 3e-7), every element of which bf16 stores as +-1 - the statistic of
    the stored row (1 - 5e-6) and that of the unrounded row (about 0.998) lie 2e-3 apart, a thousand times `rstd_bound`.  (Random rows
    alone would not do: their roundings cancel to a few 1e-5.)  Other rows: scaled rows, row 2 all-zero where there is one."""
    g = torch.Generator().manual_seed(rows * 41 + width)
    x = torch.randn(rows, width, generator=g) * row_factors(rows)[:, None]
    x[0] = 4.0 * (2 * torch.randint(0, 2, (width,), generator=g).float() - 1)
    if rows > ZERO_ROW:
        x[ZERO_ROW] = 0
    gain = 1.001 + 0.002 * torch.rand(width, generator=g)
    return x.to(torch.bfloat16), gain


def norm_unrounded(x, gain):
    """float64 RMSNorm(x) * gain before its store."""
    xd = x.double()
    return xd * rstd64(xd)[:, None] * gain.double()


# ---------------------------------------------------------------------------------------------- C: the residual GEMM in place
RESID_NK = [(512, 512), (512, 1376), (768, 768), (768, 2048), (1024, 2752)]
RESID_M = [129, 161, 257]


def resid_alphas(N: int):
    """alpha of layer 0 and of every later layer (2 x the tower's depth)."""
    return [1.0, 2.0 * O.model_dims(SIZE[N])[1]]


@functools.lru_cache(maxsize=4)
def resid_operands(N: int, K: int, M: int, alpha: float):
    """x bf16 [M, K] of size alpha (so that alpha * resid and the product are of one size: neither drowns the other), w bf16 [N, K],
    resid bf16 [M, N]; float64 reference alpha * resid + x @ W^T."""
    g = torch.Generator().manual_seed(N + 3 * K + 7 * M + int(alpha))
    x = (torch.randn(M, K, generator=g) * alpha).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16)
    r = torch.randn(M, N, generator=g).to(torch.bfloat16)
    return x, w, r, alpha * r.double() + x.double() @ w.double().T


# ---------------------------------------------------------------------------------------------- D: the layer
LAYER_BATCHES = {"even": ([(4, 16, 16), (8, 16, 24), (4, 32, 16)], [128, 128, 128]),          # 408 rows
                 "ragged": ([(8, 32, 48), (4, 16, 16), (16, 64, 64)], [5, 1, 17])}             # 331 rows: sequences of 53, 5 and 273
CLIP_SEED, WEIGHT_SEED, WEIGHT_GAIN = 13, 1003, 3.0
PREFIX = "encoder."


@functools.lru_cache(maxsize=3)
def tower_state(size: str):
    """fp32 state dict of a seeded encoder of `size` (keys without prefix)."""
    from titok_video_amd.synthetic import seeded_tower_state
    return seeded_tower_state("encoder", size, FC.PATCH, 3, 5, WEIGHT_SEED, WEIGHT_GAIN)


def held_state(size: str):
    """What the bf16 module holds, as fp32, under the encoder's prefix."""
    return {PREFIX + k: v.to(torch.bfloat16).float() for k, v in tower_state(size).items()}


def layer_clips(batch: str):
    from titok_video_amd.synthetic import synthetic_clips
    return [c.to(torch.bfloat16) for c in synthetic_clips(LAYER_BATCHES[batch][0], seed=CLIP_SEED)]


def encoder_stack(size: str, batch: str, layers: int, rnd=MC.identity, fold: bool = True, bf16_weights: bool = True, sd=None, clips=None):
    """The encoder's front and its first `layers` layers in float64 on every row (the all-rows encoder): x [L, width] as the stack
    leaves it in ws.x, and the latent-row mask.  alpha is what keel_alpha sees: ttv_tower_dims.alpha = 2 x the module's FULL depth,
    which a module truncated through `num_layers` keeps.  rnd = MC.bf16_round: one bf16 store wherever the HIP path stores (the
    front's sums and norms, qkv, the gated attention output, each residual sum, each post-norm, h and - fold False - the normalised
    copy xn); the statistic of a folded pre-norm is then that of the stored row."""
    width, full, heads = O.model_dims(size)
    sd = held_state(size) if sd is None else sd
    clips = layer_clips(batch) if clips is None else clips
    counts = LAYER_BATCHES[batch][1]
    x, cos, sin, cu, mask = MC.encoder_front([c.double() for c in clips], counts, sd, size, rnd, FC.PATCH, PREFIX)
    pre = PREFIX + "model_layers."
    w = MC.mx_layer_weights(sd, pre, layers, width, quant=False, last_plain=False, bf16_all=bf16_weights, fold=fold)
    return MC.mx_stack(x, w, sd, pre, layers, heads, cos, sin, cu, rnd, alpha=2.0 * full), mask


def encoder_z(x, mask, sd, rnd=MC.identity):
    """The encoder's tail on the stack's output: z [sum K, C]."""
    D = lambda name: sd[PREFIX + name].double()
    return rnd(MC._norm64(x[mask], D("ln_post.weight"))) @ D("proj_out.weight").T + D("proj_out.bias")
