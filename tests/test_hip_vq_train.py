"""The L2 quantiser's training kernels (csrc/ttv_vq_train.hip) on the MI355X against the numpy restatement of tests/vq_train_ref.py:
the per-entry statistics bit for bit, the commitment loss and its gradient, the EMA update with the restart of dead entries, the
refreshed argmin cache, the state dict, three training steps of a tiny TiTok, and a captured graph.  `-m gpu`.

Shapes are the smallest at which the kernels can go wrong: C = 7 (no vector fits a row), N = 1000 (a last block of 8 entries in the
statistics, of 40 in the update), rows 1 / 257 / 4099 (one partial block, a wave's quarter of 65 rows, 65 commitment blocks), the two
workload codebooks, and index patterns with one chain of all rows, empty entries between 0 and N - 1, and fewer rows than entries.
Indices fed to the C entries are built on the host, so no case depends on an argmin tie.

Every bound is a count of float32 roundings (u = 2^-24) against float64, written at the assertion or in vq_train_ref."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vq_train_ref as R  # noqa: E402

from titok_video_amd import _lib  # noqa: E402
from titok_video_amd.model.quantizer.vq_l2 import L2Quantizer  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = R.U
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
CODEBOOKS = [(64, 8), (1000, 7), (8192, 32), (16384, 64)]
ROWS = [1, 257, 4099]


def patterns(rows, n, rng):
    out = {"uniform": rng.integers(0, n, rows), "one": np.full(rows, n // 3), "ends": np.where(np.arange(rows) % 2 == 0, 0, n - 1)}
    if rows < n:
        out["distinct"] = rng.permutation(n)[:rows]          # fewer rows than entries, no entry twice
    return {k: v.astype(np.int32) for k, v in out.items()}


def rows_of(rows, c, dtype, seed):
    """z on the device in `dtype` and the same values as float32 on the host."""
    z = (torch.randn(rows, c, generator=torch.Generator().manual_seed(seed)) * 2).to(DT[dtype])
    return z.to(DEV), z.float().numpy()


def one_rounding(x, dtype):
    """Half a step of the output format at x = m 2^e (0.5 <= |m| < 1): float32 has 24 significant bits (2^(e - 25)), bf16 has 8
    (2^(e - 9)); a bf16 result went through float32 first, which adds float32's half step."""
    _m, e = np.frexp(np.asarray(x, np.float64))
    f32 = np.ldexp(1.0, e - 25)
    return f32 if dtype == "f32" else np.ldexp(1.0, e - 9) + f32


def workspace(rows, n):
    nbytes = int(_lib.lib().ttv_vq_train_workspace_bytes(rows, n))
    return torch.empty(nbytes // 8, dtype=torch.int64, device=DEV), nbytes


def hip_stats(z, idx, n, cluster_size=None, t=0.0, seed=0, step=None, rank=0, world=1):
    rows, c = z.shape
    stats = torch.full((n * (2 * c + 1),), float("nan"), dtype=torch.float32, device=DEV)      # the kernel writes every element
    ws, nbytes = workspace(rows, n)
    _lib.check(_lib.lib().ttv_vq_ema_stats(z.data_ptr(), _lib.dtype_code(z.dtype), c, idx.data_ptr(), rows, n, c, _lib.ptr(cluster_size), t, seed,
                                           _lib.ptr(step), rank, world, stats.data_ptr(), ws.data_ptr(), nbytes, _lib.stream_ptr(z.device)),
               "ttv_vq_ema_stats")
    torch.cuda.synchronize()
    s = stats.cpu().numpy()
    return s[:n], s[n:n + n * c].reshape(n, c), s[n + n * c:].reshape(n, c)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("n,c", CODEBOOKS)
def test_stats_are_the_restatement_bit_for_bit(n, c, rows, dtype):
    z, z32 = rows_of(rows, c, dtype, seed=rows + n)
    for name, idx in patterns(rows, n, np.random.default_rng(n + rows)).items():
        it = torch.from_numpy(idx).to(DEV)
        count, s, cand = hip_stats(z, it, n)
        ref_count, ref_s = R.stats_f32(z32, idx, n)
        assert np.array_equal(count, np.bincount(idx, minlength=n).astype(np.float32)), name
        assert np.array_equal(s.view(np.uint32), ref_s.view(np.uint32)), name        # same order of additions: same bits
        assert not cand.any(), name                                                  # no restarts asked for
        again = hip_stats(z, it, n)
        assert np.array_equal(again[1].view(np.uint32), s.view(np.uint32)) and np.array_equal(again[0], count), name


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_stats_write_the_drawn_row_for_dead_entries(dtype):
    n, c, rows, t, seed, step = 1000, 7, 257, 1.0, 0x1234567890ABCDEF, (5 << 32) + 3
    z, z32 = rows_of(rows, c, dtype, seed=4)
    idx = np.random.default_rng(0).integers(0, n, rows).astype(np.int32)
    cs = np.random.default_rng(1).random(n).astype(np.float32) * 2          # about half below t
    step_t = torch.tensor([step], dtype=torch.int64, device=DEV)
    for rank, world in [(0, 1), (0, 2), (1, 2)]:
        _, _, cand = hip_stats(z, torch.from_numpy(idx).to(DEV), n, torch.from_numpy(cs).to(DEV), t, seed, step_t, rank, world)
        assert np.array_equal(cand.view(np.uint32), R.candidates(z32, cs, t, seed, step, rank, world).view(np.uint32))
    assert int(step_t.item()) == step


def hip_commit(z, cbd, idx):
    rows, c = z.shape
    loss = torch.zeros(1, dtype=torch.float32, device=DEV)
    ws, nbytes = workspace(rows, cbd.shape[0])
    _lib.check(_lib.lib().ttv_vq_commit_forward(z.data_ptr(), _lib.dtype_code(z.dtype), c, cbd.data_ptr(), c, idx.data_ptr(), rows, cbd.shape[0], c,
                                                loss.data_ptr(), ws.data_ptr(), nbytes, _lib.stream_ptr(z.device)), "ttv_vq_commit_forward")
    return loss


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("n,c", CODEBOOKS)
def test_commitment_loss_and_gradient(n, c, rows, dtype):
    z, z32 = rows_of(rows, c, dtype, seed=3 * rows + n)
    cb, cb32 = rows_of(n, c, dtype, seed=n)
    g, g32 = rows_of(rows, c, dtype, seed=7)
    beta = 0.25
    for name, idx in patterns(rows, n, np.random.default_rng(rows)).items():
        it = torch.from_numpy(idx).to(DEV)
        loss = hip_commit(z, cb, it)
        e32 = cb32[idx]
        ref = R.commit_loss(z32, e32)
        got = float(loss.item())
        # every term is >= 0, so sum |terms| is the loss itself: depth roundings on the longest path of the kernel's own order
        assert abs(got - ref) <= R.commit_loss_depth(rows, c) * U * ref * 1.01, (name, got, ref)
        assert torch.equal(hip_commit(z, cb, it), loss), name
        e = cb[it.long()].contiguous()
        dz = torch.empty_like(z)
        scale = 2.0 * beta / (rows * c)
        _lib.check(_lib.lib().ttv_vq_commit_backward(g.data_ptr(), c, z.data_ptr(), c, e.data_ptr(), c, _lib.dtype_code(z.dtype), rows, c, scale,
                                                     dz.data_ptr(), c, _lib.stream_ptr(DEV)), "ttv_vq_commit_backward")
        x = R.commit_grad(g32, z32, e32, beta)
        # formed in float64 (three operations on |g| + |term|: 3 * 2^-53), rounded once to float32; bf16 rows: once more, to 8 bits
        one = one_rounding(x, dtype) + 3 * 2.0 ** -53 * (np.abs(g32) + np.abs(x - g32))
        assert (np.abs(dz.float().cpu().numpy().astype(np.float64) - x) <= one).all(), name


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_module_injects_the_commitment_gradient(dtype):
    n, c, rows, beta = 1000, 7, 257, 0.5
    cb0 = torch.randn(n, c, generator=torch.Generator().manual_seed(2))
    z, z32 = rows_of(rows, c, dtype, seed=11)
    for b in (beta, 0.0):
        vq = L2Quantizer(cb0, commitment_weight=b).to(DEV)
        zz = z.clone().requires_grad_(True)
        codes, info = vq(zz)
        codes.sum().backward()
        e = vq.lookup(info["indices"], DT[dtype])
        assert torch.equal(codes.detach(), e)                    # the straight-through value is the entry itself
        if b == 0.0:
            assert "commit_loss" not in info and torch.equal(zz.grad, torch.ones_like(zz))
            assert vq.codebook.grad is not None
            continue
        e32 = e.float().cpu().numpy()
        assert info["commit_loss"].dtype == torch.float32 and info["commit_loss"].dim() == 0 and not info["commit_loss"].requires_grad
        ref = R.commit_loss(z32, e32)
        assert abs(float(info["commit_loss"]) - ref) <= R.commit_loss_depth(rows, c) * U * ref * 1.01
        x = R.commit_grad(np.ones_like(z32), z32, e32, b)
        one = one_rounding(x, dtype) + 3 * 2.0 ** -53 * (1 + np.abs(x - 1))
        assert (np.abs(zz.grad.float().cpu().numpy().astype(np.float64) - x) <= one).all()


# ---- the update -----------------------------------------------------------------------------------------------------------------------------
def ema_module(n, c, t, seed=0, decay=0.9, some_dead=True):
    g = torch.Generator().manual_seed(n + c)
    vq = L2Quantizer(torch.randn(n, c, generator=g), codebook_update="ema", decay=decay, eps=1e-5, dead_code_threshold=t, seed=seed)
    cs = torch.rand(n, generator=g) * 3 + (0.0 if some_dead else t)
    vq.cluster_size.copy_(cs)
    vq.embed_avg.copy_(torch.randn(n, c, generator=g) * cs[:, None])
    vq.ema_step.fill_(6)
    return vq.to(DEV).train()


def state_np(vq):
    return {k: v.detach().cpu().numpy().copy() for k, v in vq.state_dict().items()}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("n,c", CODEBOOKS)
def test_update_against_the_restatement(n, c, rows, dtype):
    t, seed, decay = 1.0, 77, 0.9
    vq = ema_module(n, c, t, seed, decay)
    before = state_np(vq)
    z, z32 = rows_of(rows, c, dtype, seed=rows + c)
    idx = vq.indices(z)
    count, s, cand = hip_stats(z, idx, n, vq.cluster_size, t, seed, vq.ema_step)          # the kernel's own statistics
    assert np.array_equal(count, np.bincount(idx.cpu().numpy(), minlength=n).astype(np.float32))
    codes, info = vq(z)
    torch.cuda.synchronize()
    assert torch.equal(info["indices"], idx) and torch.equal(codes, torch.from_numpy(before["codebook"]).to(DT[dtype])[idx.long().cpu()].to(DEV))
    after = state_np(vq)
    cs_r, ea_r, cb_r, dead, total_r, sm_r = R.update_f64(before["cluster_size"], before["embed_avg"], count, s, cand, decay, 1e-5, t)
    b_cs, b_ea, b_total, rel_sm, b_cb = R.update_bounds(before["cluster_size"], before["embed_avg"], count, s, decay, 1e-5, t)
    live = ~dead
    assert dead.any() and live.any()
    assert (np.abs(after["cluster_size"] - cs_r) <= b_cs)[live].all()
    assert (np.abs(after["embed_avg"] - ea_r) <= b_ea)[live].all()
    assert (np.abs(after["codebook"] - cb_r) <= b_cb)[live].all()
    # restarted entries hold exactly the drawn row, t and t * row
    row = R.draw(seed, 6, n, 1, rows)[1]
    assert np.array_equal(after["codebook"][dead].view(np.uint32), z32[row[dead]].view(np.uint32))
    assert (after["cluster_size"][dead] == np.float32(t)).all()
    assert np.array_equal(after["embed_avg"][dead], (np.float32(t) * z32[row[dead]]).astype(np.float32))
    assert after["ema_step"].tolist() == [7]
    # the float32 restatement with the kernel's operation sequence gives the same bits except where numpy's fmaf (vq_train_ref.fma32)
    # rounds twice: one float32 step (2 u) on a moving average.  The codebook row carries that step from embed_avg (2 u) and from
    # cluster_size into cs + eps (2 u); a total that moved by at most 2 u of itself enters the denominator and the product (4 u); and
    # each of the six roundings on the way (cs + eps, the fmaf of the denominator twice over in numpy, the division, the product, the last division) can then fall the
    # other way by one step (12 u): 20 u.  Restarted rows are exact (asserted above).
    cs32, ea32, cb32, _, _, _ = R.update_f32(before["cluster_size"], before["embed_avg"], count, s, cand, decay, 1e-5, t)
    assert (np.abs(after["embed_avg"] - ea32) <= 2 * U * np.abs(ea32) + 1e-45).all()
    assert (np.abs(after["cluster_size"] - cs32) <= 2 * U * np.abs(cs32)).all()
    assert (np.abs(after["codebook"] - cb32) <= 20 * U * np.abs(cb32) + 1e-45)[live].all()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_first_step_redraws_every_entry_from_data(dtype):
    n, c, rows = 1000, 7, 257
    vq = L2Quantizer(torch.randn(n, c), codebook_update="ema", dead_code_threshold=1.0, seed=3).to(DEV).train()
    z, z32 = rows_of(rows, c, dtype, seed=5)
    vq(z)
    row = R.draw(3, 0, n, 1, rows)[1]
    assert np.array_equal(vq.codebook.detach().cpu().numpy().view(np.uint32), z32[row].view(np.uint32))
    assert (vq.cluster_size == 1.0).all() and vq.ema_step.tolist() == [1]
    assert len(set(row.tolist())) > rows // 2                  # the draw spreads over the rows


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("n,c,rows", [(64, 8, 257), (1000, 7, 4099), (16384, 64, 4099)])
def test_the_next_argmin_reads_the_updated_codebook(n, c, rows, dtype):
    vq = ema_module(n, c, 1.0, seed=5)
    z, _ = rows_of(rows, c, dtype, seed=1)
    z2, _ = rows_of(rows, c, dtype, seed=2)
    vq(z)
    got = vq.indices(z2)
    fresh = L2Quantizer(vq.codebook.detach().clone()).to(DEV)
    assert torch.equal(got, fresh.indices(z2))                 # fails if the compute-dtype copy or the norms are stale
    cbd, norms = vq._norms
    fcbd, fnorms = fresh._cb(DT[dtype])
    assert torch.equal(cbd, fcbd)
    # the kernel forms ||c||^2 with the fmaf chain of k_vq_norms: c roundings of a sum of squares
    assert ((norms - fnorms).abs() <= c * U * fnorms).all()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_state_dict_round_trip_continues_bit_for_bit(dtype):
    n, c, rows = 1000, 7, 257
    vq = ema_module(n, c, 1.0, seed=9)
    z, _ = rows_of(rows, c, dtype, seed=8)
    vq(z)
    other = L2Quantizer(torch.zeros(n, c), codebook_update="ema", decay=0.9, eps=1e-5, dead_code_threshold=1.0, seed=9).to(DEV).train()
    other.load_state_dict(vq.state_dict(), strict=True)
    vq(z)
    other(z)
    a, b = state_np(vq), state_np(other)
    assert a["ema_step"].tolist() == [8]
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---- through the model ----------------------------------------------------------------------------------------------------------------------
def tiny_cfg(**extra):
    return SimpleNamespace(tokenizer=SimpleNamespace(model=SimpleNamespace(
        patch_size=[4, 8, 8], fsq_levels=None, quantizer="l2", codebook_size=256, token_size=8, encoder_size="tiny", decoder_size="tiny", **extra)))


def test_three_training_steps_of_a_tiny_model():
    from titok_video_amd.model.titok import TiTok
    from titok_video_amd.synthetic import synthetic_clips
    from titok_video_amd.train import make_optimizer, training_step
    shapes, counts = [(4, 16, 16), (8, 32, 48), (4, 8, 24)], [6, 9, 3]
    clips = synthetic_clips(shapes, seed=21, dtype=torch.float32, device=DEV)
    torch.manual_seed(0)
    model = TiTok(tiny_cfg(commitment_weight=0.25, codebook_update="ema", dead_code_threshold=1.0)).to(DEV).train()
    vq = model.quantize
    opt = make_optimizer(model)
    assert all(p is not vq.codebook for g in opt.param_groups for p in g["params"])
    seen = []
    hook = vq.register_forward_hook(lambda mod, inp, out: seen.append((inp[0].detach().clone(), out[0].detach().clone(), out[1])))
    start = state_np(vq)
    for _ in range(3):
        loss, _, _ = training_step(model, clips, counts, opt)
        assert torch.isfinite(loss)
    hook.remove()
    assert len(seen) == 3
    for z, codes, info in seen:
        assert "commit_loss" in info
        z32, e32 = z.float().cpu().numpy(), codes.float().cpu().numpy()          # the value of codes is the selected entry
        ref = R.commit_loss(z32, e32)
        assert abs(float(info["commit_loss"]) - ref) <= R.commit_loss_depth(z.shape[0], 8) * U * ref * 1.01
    after = state_np(vq)
    assert after["ema_step"].tolist() == [3]
    for k in ("codebook", "cluster_size", "embed_avg"):
        assert not np.array_equal(start[k], after[k]), k
    # eval() and no_grad leave the state alone
    model.eval()
    model(clips, counts)
    model.train()
    with torch.no_grad():
        model(clips, counts)
    for k, v in state_np(vq).items():
        assert np.array_equal(v, after[k]), k
    # without the keys: the same three steps, no buffers, the codebook trained by the optimizer
    torch.manual_seed(0)
    plain = TiTok(tiny_cfg()).to(DEV).train()
    opt = make_optimizer(plain)
    assert any(p is plain.quantize.codebook for g in opt.param_groups for p in g["params"])
    for _ in range(3):
        loss, _, _ = training_step(plain, clips, counts, opt)
        assert torch.isfinite(loss)
    assert list(plain.quantize.buffers()) == [] and list(plain.quantize.state_dict()) == ["codebook"]


def test_trainer_checkpoint_keeps_the_buffers(tmp_path):
    from titok_video_amd.model.titok import TiTok
    model = TiTok(tiny_cfg(codebook_update="ema", dead_code_threshold=1.0)).to(DEV).train()
    z, _ = rows_of(257, 8, "f32", seed=1)
    model.quantize(z)
    from titok_video_amd.checkpoint import load_checkpoint, save_checkpoint
    path = str(tmp_path / "vq.ckpt")
    save_checkpoint(path, model, global_step=1)
    other = TiTok(tiny_cfg(codebook_update="ema", dead_code_threshold=1.0, codebook_seed=5)).to(DEV)
    assert load_checkpoint(path, other, strict=True) == 1
    for k, v in state_np(model.quantize).items():
        assert np.array_equal(v, state_np(other.quantize)[k]), k


def test_captured_graph_replays_the_update():
    n, c, rows = 1000, 7, 257
    za, _ = rows_of(rows, c, "bf16", seed=1)
    zb, _ = rows_of(rows, c, "bf16", seed=2)
    eager = ema_module(n, c, 1.0, seed=4)
    eager(za)
    eager(zb)
    vq = ema_module(n, c, 1.0, seed=4)
    static = za.clone()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        vq.eval()
        vq(static)                                             # warm-up without an update: builds the argmin cache
        vq.train()
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):                 # one stream, one chain of launches
        codes, info = vq(static)
    assert vq.ema_step.tolist() == [6]                         # capture runs nothing
    for zz in (za, zb):
        static.copy_(zz)
        graph.replay()
    torch.cuda.synchronize()
    a, b = state_np(eager), state_np(vq)
    assert b["ema_step"].tolist() == [8]                       # the step counter lives on the device
    for k in a:
        assert np.array_equal(a[k], b[k]), k
