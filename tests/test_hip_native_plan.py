"""TTV_NATIVE_PLAN=1 on the GPU: the plan the library builds (csrc/ttv_plan_host.cpp + the fill kernel of csrc/ttv_plan.hip) against
BatchPlan on the same device - every device table downloaded and compared exactly - and the towers, a training step and the
two-stream pipeline under either plan, bit for bit.  No tolerance anywhere.  `-m gpu`."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from titok_video_amd import _lib
from titok_video_amd import plan as P
from titok_video_amd.model.titok import TiTok
from titok_video_amd.synthetic import seeded_titok_state, synthetic_clips

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATCH = (4, 8, 8)
RAGGED = ([(16, 128, 128), (8, 64, 96), (4, 8, 8), (12, 96, 128)], [128, 0, 1, 37])
TABLE_CASES = {
    "ragged": RAGGED,
    "latent_blocks": ([(4, 128, 128), (8, 64, 64)], [256, 130]),
    "k600": ([(8, 64, 64)], [600]),
    "one_clip": ([(16, 128, 128)], [128]),
}
CANARY = 0x5A5A5A5A


def build(dtype, train=False):
    cfg = SimpleNamespace(tokenizer=SimpleNamespace(model=SimpleNamespace(
        patch_size=list(PATCH), fsq_levels=[7, 5, 5, 5, 5], encoder_size="tiny", decoder_size="tiny")))
    m = TiTok(cfg)
    m.load_state_dict(seeded_titok_state(0), strict=True)
    m = m.to(DEV, dtype)
    return m.train() if train else m.eval()


@pytest.fixture(autouse=True)
def _fresh_plans(monkeypatch):
    for name in ("TTV_NATIVE_PLAN", "TTV_ATTN_SPLIT", "TTV_ATTN_TAIL_DIV", "TTV_BWD_XCD", "TTV_ROPE_IDS"):
        monkeypatch.delenv(name, raising=False)
    P._plan_cache.clear()
    yield
    torch.cuda.synchronize()
    P._plan_cache.clear()


def _assert_same_tables(nat, ref, heads=((4, 2),)):
    """Every device table of a NativeBatchPlan against BatchPlan's (any device), downloaded."""
    torch.cuda.synchronize()
    assert (nat.cu_seqlens, nat.grids, nat.grid_sizes, nat.total_rows, nat.sum_tokens, nat.sum_patches, nat.max_seqlen, nat.n_rope_ids,
            nat.n_blocks64) == (ref.cu_seqlens, ref.grids, ref.grid_sizes, ref.total_rows, ref.sum_tokens, ref.sum_patches, ref.max_seqlen,
                                ref.n_rope_ids, ref.n_blocks64)
    L, B = ref.total_rows, len(ref.grids)
    for i, n in enumerate((B + 1, ref.sum_tokens, ref.sum_patches, 8 * B, 2 * ref.n_blocks64, L, 2 * L)):
        assert torch.equal(nat.table(i, n).cpu(), ref.table(i, n).cpu()), ("cu_seqlens", "latent_rows", "patch_rows", "clip_desc", "blocks64",
                                                                              "row_seq", "rope_ids")[i]
    assert torch.equal(nat.rope_cs.cpu().view(torch.int32), ref.rope_cs.cpu().view(torch.int32)), "rope_cs"
    for hq, hkv in heads:
        a, b = nat.batch_for(hq, hkv), ref.batch_for(hq, hkv)
        torch.cuda.synchronize()
        for f in ("n_clips", "total_rows", "sum_tokens", "sum_patches", "max_patches_per_clip", "n_qblocks", "n_blocks64", "qblocks_all_full",
                  "n_qblocks_latent", "n_qblocks_patch"):
            assert getattr(a, f) == getattr(b, f), f
        assert not a.items64 and a.n_items64 == 0 and a.qblocks_paired == 0
        assert bool(a.rope_ids) == bool(b.rope_ids) and bool(a.rope_base) == bool(b.rope_base)
        assert torch.equal(nat.attention_table(hq, hkv).cpu(), ref.attention_table(hq, hkv).cpu())
        assert torch.equal(nat.attention_table_l0(hq, hkv).cpu(), ref.attention_table_l0(hq, hkv).cpu())
        for mine, theirs, there in ((nat.attention_table_latent, ref.attention_table_latent, b.qblocks_latent),
                                    (nat.attention_table_patch, ref.attention_table_patch, b.qblocks_patch)):
            if there:
                assert torch.equal(mine(hq, hkv).cpu(), theirs(hq, hkv).cpu())
            else:
                assert mine(hq, hkv) is None


@pytest.mark.parametrize("name", list(TABLE_CASES))
def test_device_tables_equal_batchplan_and_nothing_else_is_written(name):
    shapes, counts = TABLE_CASES[name]
    ref = P.BatchPlan(shapes, counts, PATCH, torch.device(DEV))
    _assert_same_tables(P.NativeBatchPlan(shapes, counts, PATCH, torch.device(DEV)), ref, heads=((4, 2), (12, 4)))

    # the library's calls on buffers of the test: canary words between, behind and around every table stay as they were
    lib, n = _lib.lib(), len(shapes)
    dims, cnt, pt = P._i32s([v for g in shapes for v in g]), P._i32s(counts), P._i32s(PATCH)
    sz = _lib.PlanSizes()
    _lib.check(lib.ttv_plan_rows_sizes(dims, cnt, n, pt, C.byref(sz)), "sizes")
    host = torch.empty(int(sz.host_words), dtype=torch.int32).pin_memory()
    _lib.check(lib.ttv_plan_rows_fill(dims, cnt, n, pt, 1, host.data_ptr(), host.numel()), "fill")
    pad = 64
    seg = torch.full((int(sz.dev_words) + 2 * pad,), CANARY, dtype=torch.int32, device=DEV)
    L = int(sz.total_rows)
    cs = torch.full(((L + 2) * 64,), CANARY, dtype=torch.int32, device=DEV)
    bc, bs = P._rope_base_device(64, 3, int(sz.n_rope_ids), DEV)
    batch = _lib.Batch()
    _lib.check(lib.ttv_plan_rows_build(C.byref(sz), host.data_ptr(), seg.data_ptr() + 4 * pad, bc.data_ptr(), bs.data_ptr(), bc.shape[1],
                                       cs.data_ptr() + 4 * 64, None, C.byref(batch), _lib.stream_ptr(torch.device(DEV))), "build")
    torch.cuda.synchronize()
    assert batch.rope_ids is None and batch.rope_base is None and batch.qblocks is None and batch.n_qblocks == 0
    assert batch.cu_seqlens == seg.data_ptr() + 4 * pad + 4 * sz.off_cu_seqlens and batch.rope_cs == cs.data_ptr() + 4 * 64
    got = seg.cpu().numpy()
    assert (got[:pad] == CANARY).all() and (got[pad + int(sz.dev_words):] == CANARY).all()
    body = got[pad: pad + int(sz.dev_words)]
    assert np.array_equal(body[:int(sz.host_words)], host.numpy()), "the host segment arrives unchanged"
    tables = ((sz.off_latent_rows, ref.sum_tokens, 1), (sz.off_patch_rows, ref.sum_patches, 2), (sz.off_row_seq, L, 5), (sz.off_rope_ids, 2 * L, 6))
    untouched = np.ones(int(sz.dev_words), dtype=bool)
    untouched[:int(sz.host_words)] = False
    for off, words, i in tables:
        assert np.array_equal(body[off: off + words], ref.table(i, words).cpu().numpy())
        untouched[off: off + words] = False
    assert (body[untouched] == CANARY).all(), "a word between the device tables was written"
    got_cs = cs.cpu().numpy()
    assert (got_cs[:64] == CANARY).all() and (got_cs[(L + 1) * 64:] == CANARY).all()
    assert np.array_equal(got_cs[64: (L + 1) * 64], ref.rope_cs.cpu().view(torch.int32).numpy().reshape(-1))

    az = _lib.PlanAttn()
    cu = P._i32s(ref.cu_seqlens)
    _lib.check(lib.ttv_plan_attn_sizes(cu, cnt, n, 4, 2, -1, 0, C.byref(az)), "attn sizes")
    htab = torch.empty(int(az.words), dtype=torch.int32).pin_memory()
    _lib.check(lib.ttv_plan_attn_fill(cu, cnt, n, 4, 2, -1, 0, htab.data_ptr(), htab.numel()), "attn fill")
    dtab = torch.full((int(az.words) + 2 * pad,), CANARY, dtype=torch.int32, device=DEV)
    _lib.check(lib.ttv_plan_attn_set(C.byref(az), htab.data_ptr(), dtab.data_ptr() + 4 * pad, C.byref(batch), _lib.stream_ptr(torch.device(DEV))), "attn set")
    torch.cuda.synchronize()
    got = dtab.cpu().numpy()
    assert (got[:pad] == CANARY).all() and (got[pad + int(az.words):] == CANARY).all()
    assert np.array_equal(got[pad + az.off_qblocks: pad + az.off_qblocks + 4 * az.n_qblocks].reshape(-1, 4), ref.attention_table(4, 2).cpu().numpy())
    assert batch.n_qblocks == az.n_qblocks and batch.qblocks == dtab.data_ptr() + 4 * pad + 4 * az.off_qblocks


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_tower_forward_is_bit_equal_under_either_plan(dtype, monkeypatch):
    shapes, counts = RAGGED
    model = build(dtype)
    clips = synthetic_clips(shapes, seed=31, dtype=dtype, device=DEV)
    outs = []
    for flag in (None, "1"):
        if flag:
            monkeypatch.setenv("TTV_NATIVE_PLAN", flag)          # read when get_plan is called
        P._plan_cache.clear()
        plan = P.get_plan(shapes, counts, PATCH, torch.device(DEV))
        assert type(plan) is (P.NativeBatchPlan if flag else P.BatchPlan)
        with torch.no_grad():
            recon, out = model(clips, counts)
        torch.cuda.synchronize()
        assert P.get_plan(shapes, counts, PATCH, torch.device(DEV)) is plan
        outs.append(([r.clone() for r in recon], out["indices"].clone()))
    assert outs[0][1].numel() == sum(counts) and torch.equal(outs[0][1], outs[1][1])
    for a, b in zip(outs[0][0], outs[1][0]):
        assert torch.equal(a, b)


def test_training_step_is_bit_equal_under_either_plan(monkeypatch):
    """One training_step on a 3-clip ragged batch from identical weights under each plan.

    The step's loss scalar is NOT a bit-reproducible function of its inputs: the loss kernel ends every block in a float atomicAdd on
    the scalar (csrc/ttv_bwd.hip k_l1_loss).  Measured on an MI355X with this batch: six evaluations of the kernel on ONE reconstruction
    gave the bit patterns 1070250664, ...659, ...662, ...667, ...667, ...667, and three steps under BatchPlan the losses ...659, ...668,
    ...666 (three under the library's plan: ...660, ...666, ...668); 72 of the 76 gradient tensors differ between two steps under
    BatchPlan.  So the loss is compared where it is a function of the plan: the reconstruction the loss is taken of is bit-equal in
    every pixel, and so is the loss of it in the package's deterministic host evaluation; the kernel's scalar and the gradients are
    compared bit for bit whenever they are reproducible under BatchPlan itself (checked first: two steps, and for the scalar eight more
    evaluations of the kernel on one reconstruction, all agree), otherwise the test says why and compares every table the two plans hand
    to the kernels."""
    from titok_video_amd import train
    shapes, counts = [(8, 64, 96), (4, 16, 16), (12, 96, 128)], [37, 1, 128]
    clips = synthetic_clips(shapes, seed=41, dtype=torch.float32, device=DEV)
    host_clips = [c.cpu() for c in clips]
    l1 = train.l1_reconstruction_loss
    seen = []

    def capturing_l1(recon, target):
        seen.append([r.detach().clone() for r in recon])
        return l1(recon, target)
    monkeypatch.setattr(train, "l1_reconstruction_loss", capturing_l1)

    def step():
        P._plan_cache.clear()
        model = build(torch.float32, train=True)
        loss, _gnorm, idx = train.training_step(model, clips, counts, train.make_optimizer(model))
        torch.cuda.synchronize()
        recon = seen.pop()
        assert not seen
        host_loss = l1([r.cpu() for r in recon], host_clips)          # plain torch on the host: the same bits for the same reconstruction
        return dict(loss=loss.clone(), idx=idx.clone(), recon=recon, host_loss=host_loss,
                    grads={n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})

    first, again = step(), step()
    monkeypatch.setenv("TTV_NATIVE_PLAN", "1")
    native = step()
    plan = next(iter(P._plan_cache.values()))
    assert type(plan) is P.NativeBatchPlan
    assert torch.equal(first["idx"], native["idx"]) and first["idx"].numel() == sum(counts)
    for a, b in zip(first["recon"], native["recon"]):
        assert torch.equal(a, b), "the training forward's reconstruction differs between the plans"
    assert torch.equal(first["host_loss"].view(torch.int32), native["host_loss"].view(torch.int32))
    bits = [int(r["loss"].view(torch.int32).item()) for r in (first, again, native)]
    # reproducible = two steps under BatchPlan AND eight more evaluations of the loss kernel on the first step's reconstruction agree
    # (two values that merely coincide once say little: the kernel's spread here is a handful of bit patterns)
    repeats = [int(l1(first["recon"], clips).view(torch.int32).item()) for _ in range(8)]
    print(f"loss bits: BatchPlan {bits[0]}, BatchPlan again {bits[1]}, library plan {bits[2]}; the kernel eight more times on one reconstruction: {repeats}")
    loss_reproducible = len(set(bits[:2] + repeats)) == 1
    if loss_reproducible:
        assert bits[2] == bits[0], (float(first["loss"]), float(native["loss"]))
    else:
        print("the loss scalar is not reproducible under BatchPlan (float atomics in the loss kernel): compared through the "
              "reconstruction and its host evaluation above")
    unequal = [n for n in first["grads"] if not torch.equal(first["grads"][n], again["grads"][n])]
    if not unequal:
        assert sorted(first["grads"]) == sorted(native["grads"])
        for n in first["grads"]:
            assert torch.equal(first["grads"][n], native["grads"][n]), n
    else:
        print(f"gradients are not reproducible run to run under BatchPlan ({len(unequal)} of {len(first['grads'])} tensors, e.g. {unequal[0]}): "
              "float atomics in the backward")
    if not loss_reproducible or unequal:
        # what cannot be compared through the step's own outputs is compared through what the plans hand to the kernels
        _assert_same_tables(plan, P.BatchPlan(shapes, counts, PATCH, torch.device(DEV)))


def _ten_batches():
    rng = np.random.RandomState(3)
    shapes = [(16, 128, 128), (8, 64, 96), (16, 64, 64), (4, 128, 96), (12, 96, 128), (4, 8, 8)]
    out = []
    for i in range(10):
        n = 2 + i % 4
        out.append(([shapes[j] for j in rng.randint(0, len(shapes), n)], [int(k) for k in rng.choice([0, 1, 37, 64, 128, 130], n)]))
    return out


@pytest.mark.parametrize("slots", [3, 16])
def test_staging_slots_are_not_rewritten_before_their_copy_ran(slots, monkeypatch):
    """Ten plans (twenty segments) back to back behind ~50 ms of queued work, with no synchronisation in between: more than the ring
    holds.  With 3 slots the host must wait for the oldest copy before it reuses a slot; with 16 the ring grows instead."""
    monkeypatch.setattr(P, "_STAGE_MAX_SLOTS", slots)
    monkeypatch.setattr(P, "_stage_rings", {})
    batches = _ten_batches()
    refs = [P.BatchPlan(s, c, PATCH, torch.device(DEV)) for s, c in batches]
    a = torch.randn(8192, 8192, device=DEV)
    torch.cuda.synchronize()
    for _ in range(5):
        a = (a @ a).clamp_(-1, 1)                                  # the copies queue up behind this
    plans = []
    for s, c in batches:
        p = P.NativeBatchPlan(s, c, PATCH, torch.device(DEV))
        p.batch_for(4, 2)
        plans.append(p)
    assert len(P._stage_rings[DEV].slots) <= slots
    for p, r in zip(plans, refs):
        _assert_same_tables(p, r)


def test_forward_pipeline_under_the_native_plan(monkeypatch):
    from titok_video_amd.pipeline import ForwardPipeline
    monkeypatch.setenv("TTV_NATIVE_PLAN", "1")
    model = build(torch.bfloat16)
    kinds = [([(8, 64, 96), (4, 8, 8), (4, 16, 16)], [37, 1, 0]), ([(12, 96, 128), (4, 16, 16)], [128, 5])]
    batches = [(synthetic_clips(kinds[i % 2][0], seed=60 + i, dtype=torch.bfloat16, device=DEV), kinds[i % 2][1]) for i in range(6)]
    with torch.no_grad():
        ref = [model(c, k) for c, k in batches]
    torch.cuda.synchronize()
    assert all(type(p) is P.NativeBatchPlan for p in P._plan_cache.values()) and len(P._plan_cache) == 2
    P._plan_cache.clear()                                          # the pipeline's streams build the plans themselves
    pipe = ForwardPipeline(model, depth=2)
    tickets = [pipe.submit(c, k) for c, k in batches]
    outs = [pipe.result(t) for t in tickets]
    torch.cuda.synchronize()
    assert all(type(p) is P.NativeBatchPlan for p in P._plan_cache.values()) and len(P._plan_cache) == 2
    for (r0, o0), (r1, o1) in zip(ref, outs):
        assert torch.equal(o0["indices"], o1["indices"])
        for x, y in zip(r0, r1):
            assert torch.equal(x, y)
