"""The encoder's last layer under TTV_ENC_LATENT_LAST queries its latent rows only, so its to_qkv needs q and gate for the latent token
tiles alone: with one geometry for every clip, K and P multiples of 128 and the width-256 bf16 kernels, k_qkv256 runs over a tile list
with a panel floor (GemmArgs.panel_lo) - every panel for the latent tiles, the k | v panels only for the patch tiles - in one launch.
Against the switch-off run (ttv_debug_set bit 23, same process): the k | v columns of every row and the q | gate columns of the latent
rows bit for bit, the q | gate columns of the patch rows never written (the pattern the workspace was filled with survives), and the
encoder's outputs bit for bit.  `-m gpu`.

The last layer's to_qkv output is read out of the tower's workspace after a forward of ONE layer (`num_layers` set to 1 on the module:
layer 0 is then the last layer, and nothing in front of it has written ws.qkv).  Workspace layout (ttv_api.hip, carve): x, xn [L, d],
qkv [L, 2d+2g], each rounded up to 256 bytes.

Shapes: the smallest at which the item map can go wrong - case A, 3 clips of 8x64x64 with K = 128 (one latent and one patch tile per
clip: period 2, run 1, 48 items, one per block); case B, 2 clips of 8x64x128 with K = 256 (period 4, run 2: 64 items); case C, 36 clips
of case B's geometry (1 152 items: 288 blocks of 4, the launch code's aligned split - a latent tile is shared by three blocks that
start at panels 0, 4 and 8); case D, 48 clips of 8x128x256 with K = 128 (period 9, run 1; 2 112 items are more than 512 blocks of 4, so
the 512 blocks walk 4.1 items each: ranges start inside a tile, cross tiles and meet the floor in their middle).  K = 32 and a batch of two geometries take the plain sequence."""
from types import SimpleNamespace

import pytest
import torch

from titok_video_amd import _lib
from titok_video_amd.model.titok import TiTok
from titok_video_amd.plan import BatchPlan, NativeBatchPlan, get_plan
from titok_video_amd.synthetic import seeded_titok_state, synthetic_clips

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
LEVELS = [7, 5, 5, 5, 5]
OFF = _lib.DBG_ENC_LAST_QKV_ALL
CASES = {"A": ([(8, 64, 64)] * 3, [128] * 3), "B": ([(8, 64, 128)] * 2, [256] * 2), "C": ([(8, 64, 128)] * 36, [256] * 36),
         "D": ([(8, 128, 256)] * 48, [128] * 48)}
FALLBACKS = {"k32": ([(8, 64, 64)] * 3, [32] * 3), "two_geometries": ([(8, 64, 64), (8, 64, 128)], [128, 128])}
PATTERN = 0x7f7f


@pytest.fixture(autouse=True)
def full_items(monkeypatch):
    monkeypatch.setenv("TTV_ATTN_SPLIT", "0")        # tables of full items at these small batches too (what the benchmark batch gets)
    yield
    _lib.lib().ttv_debug_set(0)


def build_model(seed=0):
    cfg = SimpleNamespace(tokenizer=SimpleNamespace(model=SimpleNamespace(patch_size=[4, 8, 8], fsq_levels=LEVELS, encoder_size="tiny",
                                                                          decoder_size="tiny")))
    m = TiTok(cfg)
    m.load_state_dict(seeded_titok_state(seed), strict=True)
    return m.to(DEV, BF).eval()


def encode(model, clips, counts, bits):
    """(indices, codes, bounded, z) of the encoder with its FSQ tail under the given debug bits."""
    _lib.lib().ttv_debug_set(bits)
    try:
        with torch.no_grad():
            res = model.encoder.run(clips, counts, None, model.quantize.params, want_z=True, want_bounded=True)
        torch.cuda.synchronize()
    finally:
        _lib.lib().ttv_debug_set(0)
    return tuple(res[k].clone() for k in ("indices", "codes", "bounded", "z"))


def same_outputs(a, b):
    return all(torch.equal(x.view(torch.int16) if x.dtype == BF else x, y.view(torch.int16) if y.dtype == BF else y) for x, y in zip(a, b))


def qkv_view(enc, shapes, counts):
    """(workspace, qkv view [L, 2d+2g], plan) of the encoder's workspace on the current stream."""
    plan = get_plan(shapes, counts, enc.patch, torch.device(DEV))
    ws = enc._workspace(enc._dims(_lib.dtype_code(BF)), plan, torch.device(DEV))
    L, d, g = plan.total_rows, enc.width, enc.heads[1] * 64
    nq = 2 * d + 2 * g
    a256 = lambda v: (v + 255) // 256 * 256
    o_qkv = 2 * a256(L * d * 2)
    return ws, ws[o_qkv:o_qkv + L * nq * 2].view(BF).view(L, nq), plan


def one_layer_runs(model, shapes, counts, seed):
    """The last layer alone (a tower of one layer), switch off and on, over a workspace pre-filled with the pattern."""
    enc = model.encoder
    clips = synthetic_clips(shapes, seed=seed, dtype=BF, device=DEV)
    enc.num_layers = 1
    try:
        ws, qkv, plan = qkv_view(enc, shapes, counts)
        out = {}
        for name, bits in (("off", OFF), ("on", 0)):
            ws.fill_(PATTERN & 0xff)
            outs = encode(model, clips, counts, bits)
            out[name] = (qkv.clone().view(torch.int16), outs)
    finally:
        enc.num_layers = len(enc.model_layers.attn_layer)
        enc.invalidate_packs()           # (a pack built meanwhile carries one layer)
    return out, plan


@pytest.mark.parametrize("case", sorted(CASES))
def test_last_to_qkv_skips_the_patch_rows_q_and_gate_and_keeps_every_other_bit(case):
    shapes, counts = CASES[case]
    model = build_model()
    out, plan = one_layer_runs(model, shapes, counts, seed=31)
    (qkv_off, outs_off), (qkv_on, outs_on) = out["off"], out["on"]
    d = model.encoder.width
    cu = plan.cu_seqlens
    assert not bool((qkv_off == PATTERN).all(1).any()), "the switch-off to_qkv left a row unwritten"
    assert torch.equal(qkv_on[:, 2 * d:], qkv_off[:, 2 * d:]), "k | v columns differ"
    for b, k in enumerate(counts):
        lat, pat = slice(cu[b], cu[b] + k), slice(cu[b] + k, cu[b + 1])
        assert torch.equal(qkv_on[lat], qkv_off[lat]), f"clip {b}: latent rows of to_qkv differ"
        assert bool((qkv_on[pat, :2 * d] == PATTERN).all()), f"clip {b}: q | gate of a patch row was written"
    assert same_outputs(outs_on, outs_off), "the one-layer encoder's outputs differ"


@pytest.mark.parametrize("case", sorted(CASES))
def test_whole_encoder_same_indices_codes_and_bounded_z(case):
    shapes, counts = CASES[case]
    model = build_model()
    clips = synthetic_clips(shapes, seed=21, dtype=BF, device=DEV)
    on, off = encode(model, clips, counts, 0), encode(model, clips, counts, OFF)
    assert bool(torch.isfinite(on[2]).all()) and bool(torch.isfinite(on[3]).all())
    assert same_outputs(on, off), "indices, codes, bounded or z differ between the switch on and off"


@pytest.mark.parametrize("case", sorted(FALLBACKS))
def test_fallback_geometries_take_the_plain_sequence(case):
    shapes, counts = FALLBACKS[case]
    model = build_model()
    out, plan = one_layer_runs(model, shapes, counts, seed=33)
    (qkv_off, outs_off), (qkv_on, outs_on) = out["off"], out["on"]
    d = model.encoder.width
    assert not bool((qkv_on[:, :2 * d] == PATTERN).all(1).any()), "a row's q | gate was skipped at a geometry that cannot take the tile list"
    assert torch.equal(qkv_on, qkv_off)
    assert same_outputs(outs_on, outs_off)


@pytest.mark.parametrize("case", sorted(CASES) + sorted(FALLBACKS))
def test_both_planners_make_the_same_promise(case):
    """ttv_batch.tokens_per_clip: K when every clip has K latent tokens and the same patch count, else 0 - from plan.py and from the
    library's own planner."""
    shapes, counts = {**CASES, **FALLBACKS}[case]
    expect = counts[0] if case != "two_geometries" else 0
    for cls in (BatchPlan, NativeBatchPlan):
        plan = cls(shapes, counts, (4, 8, 8), torch.device(DEV))
        assert plan.batch_for(4, 2).tokens_per_clip == expect, cls.__name__
    torch.cuda.synchronize()


# ---- the encoder's front in one kernel: ttv_patch_embed_norm against ttv_patch_gather + ttv_linear + ttv_rmsnorm ----
# Shapes: one full tile and a clip change inside a tile (3 clips of 128 patches); more than one block with a ragged end, 384 + 64
# patches of two geometries (the last block holds 64 of its 128 rows); a call that stops inside a tile (rows < P); and two clips of the
# benchmark's geometry (four frame groups, 16 x 16 patches each: every term of the patch address is exercised).
EMBED_CASES = {"three_tiles": ([(8, 64, 64)] * 3, [128] * 3, None),
               "ragged_two_geometries": ([(8, 64, 96), (8, 64, 96), (8, 32, 64)], [32, 5, 17], None),
               "stops_inside_a_tile": ([(8, 64, 96), (8, 64, 96), (8, 32, 64)], [32, 5, 17], 411),
               "benchmark_clips": ([(16, 128, 128)] * 2, [128] * 2, None)}
WIDTH, PATCH, CH = 256, (4, 8, 8), 3
PD = CH * PATCH[0] * PATCH[1] * PATCH[2]


def bf16_ulp(x):
    """One unit in the last place of the bf16 values in x (8 significant bits), as float64; the smallest normal's for zero."""
    a = x.double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


@pytest.fixture(scope="module")
def embed_weights():
    g = torch.Generator().manual_seed(77)
    w = (torch.randn(WIDTH, PD, generator=g) * PD ** -0.5).to(DEV, BF)
    bias = (torch.randn(WIDTH, generator=g) * 0.1).to(DEV, BF)
    mask = torch.full((1,), 0.0625 * 1.37, device=DEV)
    gain = (1.0 + 0.2 * torch.randn(WIDTH, generator=g)).to(DEV)
    return w, bias, mask, gain


@pytest.fixture(scope="module")
def embed_runs(embed_weights):
    """Per case, computed once: (sequence's x, kernel's x, float64 replay of the rows written, their packed rows, the plan)."""
    w, bias, mask, gain = embed_weights
    lib, S, bf = _lib.lib(), _lib.stream_ptr(torch.device(DEV)), _lib.TTV_BF16
    out = {}
    for name, (shapes, counts, rows) in EMBED_CASES.items():
        plan = get_plan(shapes, counts, PATCH, torch.device(DEV))
        plan.use_on_current_stream()
        clips = synthetic_clips(shapes, seed=55, dtype=BF, device=DEV)
        L, P = plan.total_rows, plan.sum_patches
        M = P if rows is None else rows
        desc, prow, rseq = plan.clip_desc_dev, plan.patch_rows_dev, plan.table(5, L)
        pa = torch.empty(P, PD, device=DEV, dtype=BF)
        pb = torch.empty(P, WIDTH, device=DEV, dtype=BF)
        xs = [torch.full((L + 128, WIDTH), PATTERN, device=DEV, dtype=torch.int16).view(BF) for _ in range(2)]
        _lib.check(lib.ttv_patch_gather(_lib.ptr_array(clips), desc.data_ptr(), 0, len(clips), *PATCH, CH, pa.data_ptr(), PD, bf, max(plan.grid_sizes), S), "gather")
        _lib.check(lib.ttv_linear(pa.data_ptr(), PD, w.data_ptr(), PD, bias.data_ptr(), mask.data_ptr(), pb.data_ptr(), WIDTH, M, WIDTH, PD, bf, S), "linear")
        _lib.check(lib.ttv_rmsnorm(pb.data_ptr(), bf, WIDTH, None, xs[0].data_ptr(), bf, WIDTH, prow.data_ptr(), gain.data_ptr(), M, WIDTH, 1e-5, S), "rmsnorm")
        _lib.check(lib.ttv_patch_embed_norm(_lib.ptr_array(clips), desc.data_ptr(), prow.data_ptr(), rseq.data_ptr(), len(clips), *PATCH, CH, w.data_ptr(), PD,
                                            bias.data_ptr(), mask.data_ptr(), gain.data_ptr(), 1e-5, xs[1].data_ptr(), WIDTH, M, WIDTH, bf, S), "patch_embed_norm")
        torch.cuda.synchronize()
        # float64 replay: float64 sums of the bf16 inputs, the two bf16 roundings of the stored sum, a float64 norm
        s = pa[:M].cpu().double() @ w.cpu().double().T + bias.cpu().double()
        y = (s.to(BF).float() + mask.cpu().to(BF).float()).to(BF).double()
        ref = y / torch.sqrt((y * y).mean(1, keepdim=True) + 1e-5) * gain.cpu().double()
        out[name] = (xs[0].cpu(), xs[1].cpu(), ref, prow.cpu().long()[:M], plan)
    return out


@pytest.mark.parametrize("case", sorted(EMBED_CASES))
def test_patch_embed_norm_is_the_three_call_sequence_within_one_ulp(case, embed_runs):
    seq, new, ref, rows, _ = embed_runs[case]
    a, b = seq[rows].double(), new[rows].double()
    assert bool(torch.isfinite(b).all())
    differing = int((seq[rows].view(torch.int16) != new[rows].view(torch.int16)).sum())
    worst_pair = float(((a - b).abs() / bf16_ulp(a)).max())
    err_seq, err_new = float(((a - ref).abs() / bf16_ulp(ref)).max()), float(((b - ref).abs() / bf16_ulp(ref)).max())
    print(f"MEASURED {case}: {differing} of {a.numel()} elements differ from the sequence, worst {worst_pair:.2f} ulp; "
          f"worst error against float64: sequence {err_seq:.3f} ulp, kernel {err_new:.3f} ulp")
    assert worst_pair <= 1.0, "an element is more than one bf16 ulp from the sequence's value"
    assert err_new <= err_seq + 1.0, "the kernel's worst error against float64 exceeds the sequence's by more than one bf16 ulp"
    # the kernel keeps the GEMM's k order and sums the row statistic in the row kernel's order: the same bits, so that is what is held
    assert differing == 0, "the kernel's rows are not the sequence's bits"


@pytest.mark.parametrize("case", sorted(EMBED_CASES))
def test_patch_embed_norm_writes_the_rows_it_was_given_and_no_other(case, embed_runs):
    seq, new, _, rows, plan = embed_runs[case]
    untouched = torch.ones(new.shape[0], dtype=torch.bool)
    untouched[rows] = False
    assert int(untouched.sum()) >= 128 + plan.sum_tokens
    assert bool((new[untouched].view(torch.int16) == PATTERN).all()), "a row that is not one of the call's patch rows was written"
    assert not bool((new[rows].view(torch.int16) == PATTERN).all(1).any()), "a patch row of the call was not written"
    assert torch.equal(seq[untouched].view(torch.int16), new[untouched].view(torch.int16))


FRONT_CASES = {**{k: CASES[k] for k in ("A", "B")}, "benchmark_clips": ([(16, 128, 128)] * 8, [128] * 8),
               "two_geometries": FALLBACKS["two_geometries"]}


@pytest.mark.parametrize("case", sorted(FRONT_CASES))
def test_whole_encoder_with_the_fused_front_changes_no_bit(case):
    """ttv_encoder_forward with k_patch_embed256 against the gathering GEMM + row kernel (ttv_debug_set bit 24): indices, codes, bounded
    values and z bit for bit - a row of x that differed in one place would move tokens across FSQ boundaries four layers later."""
    shapes, counts = FRONT_CASES[case]
    model = build_model()
    clips = synthetic_clips(shapes, seed=23, dtype=BF, device=DEV)
    on, off = encode(model, clips, counts, 0), encode(model, clips, counts, _lib.DBG_PATCH_EMBED_UNFUSED)
    assert same_outputs(on, off), "indices, codes, bounded or z differ between the fused and the unfused front"
