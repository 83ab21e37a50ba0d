"""The L2 quantiser's training pieces without a GPU: the numpy restatement (tests/vq_train_ref.py) against float64, the module's
arguments, buffers and state-dict keys, the config keys of TiTok, the argument checks of the new C entries through the loaded library,
and the one all-reduce of the flat count | sum | cand buffer on two gloo ranks."""
import ctypes as C
import os
import socket
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vq_train_ref as R  # noqa: E402

from titok_video_amd import _lib  # noqa: E402
from titok_video_amd.model.quantizer.vq_l2 import L2Quantizer  # noqa: E402

U = R.U


def _case(rows=700, n=37, c=5, seed=0, collapse=False):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((rows, c)).astype(np.float32) * 3
    idx = np.zeros(rows, np.int64) if collapse else rng.integers(0, n, rows)
    return z, idx


@pytest.mark.parametrize("collapse", [False, True])
def test_float32_stats_against_float64(collapse):
    z, idx = _case(collapse=collapse)
    count, s32 = R.stats_f32(z, idx, 37)
    s64 = R.stats_f64(z, idx, 37)
    absum = R.stats_f64(np.abs(z), idx, 37)
    assert np.array_equal(count, np.bincount(idx, minlength=37))
    # count[n] additions per element, each rounding a partial sum that is at most sum |z|
    assert (np.abs(s32.astype(np.float64) - s64) <= count[:, None] * U * absum).all()
    # np.add.at adds in ascending row order: an explicit loop gives the same bits
    loop = np.zeros_like(s32)
    for r in range(len(idx)):
        loop[idx[r]] = (loop[idx[r]] + z[r]).astype(np.float32)
    assert np.array_equal(loop, s32)


def _state(n=37, c=5, seed=1):
    rng = np.random.default_rng(seed)
    cs = (rng.random(n) * 4).astype(np.float32)
    cs[::7] = 0.0
    ea = rng.standard_normal((n, c)).astype(np.float32) * cs[:, None]
    return cs, ea


@pytest.mark.parametrize("t", [0.0, 0.5])
def test_update_restatement_against_float64(t):
    z, idx = _case()
    cs0, ea0 = _state()
    count, s = R.stats_f32(z, idx, 37)
    cand = R.candidates(z, cs0, t, seed=5, step=3)
    cs, ea, cb, dead, total, sm = R.update_f32(cs0, ea0, count, s, cand, 0.99, 1e-5, t)
    cs_r, ea_r, cb_r, dead_r, total_r, sm_r = R.update_f64(cs0, ea0, count, s, cand, 0.99, 1e-5, t)
    # the rounding steps are counted in vq_train_ref.update_bounds: 2 per moving average, n additions for the total, 4 for smoothed
    # plus what it carries in, 1 for the division
    b_cs, b_ea, b_total, rel_sm, b_cb = R.update_bounds(cs0, ea0, count, s, 0.99, 1e-5, t)
    assert np.array_equal(dead, dead_r) and np.array_equal(dead, cs0 < np.float32(t)) and (dead[::7].all() if t > 0 else not dead.any())
    live = ~dead
    assert (np.abs(cs - cs_r) <= b_cs)[live].all() and (cs[dead] == np.float32(t)).all()
    assert (np.abs(ea - ea_r) <= b_ea)[live].all()
    assert abs(float(total) - total_r) <= b_total
    assert (np.abs(sm - sm_r) <= rel_sm * sm_r).all()
    assert (np.abs(cb - cb_r) <= b_cb)[live].all()
    # restarted entries: exactly the drawn row, t and t * row
    rk, row = R.draw(5, 3, 37, 1, len(z))
    assert (rk == 0).all()
    assert np.array_equal(cb[dead], z[row[dead]]) and np.array_equal(ea[dead], (np.float32(t) * z[row[dead]]).astype(np.float32))
    # sum smoothed = total: exact in exact arithmetic (sum (cs + eps) = total + n eps); each float32 term is within rel_sm of its float64
    # value and the float32 total within b_total of the float64 one (the sum below is taken in float64)
    assert abs(sm.astype(np.float64).sum() - float(total)) <= rel_sm.max() * total_r + b_total + 1e-12 * total_r


def test_entry_without_rows_only_decays():
    cs0, ea0 = _state()
    n = len(cs0)
    zeros = np.zeros_like(ea0)
    cs, ea, cb, dead, total, sm = R.update_f32(cs0, ea0, np.zeros(n), zeros, zeros, 0.9, 1e-5, 0.0)
    assert not dead.any()
    assert np.array_equal(cs, (np.float32(0.9) * cs0).astype(np.float32))
    assert np.array_equal(ea, (np.float32(0.9) * ea0).astype(np.float32))


def test_draw_is_keyed_by_seed_step_and_entry():
    a = R.draw(7, 0, 64, 2, 100)
    assert all(not np.array_equal(x, y) for x, y in zip(a, R.draw(8, 0, 64, 2, 100)))
    assert all(not np.array_equal(x, y) for x, y in zip(a, R.draw(7, 1, 64, 2, 100)))
    assert set(a[0].tolist()) == {0, 1} and a[1].max() < 100 and len(set(a[1].tolist())) > 32
    # the entry is the counter: a longer table starts with the shorter one
    assert np.array_equal(R.draw(7, 0, 128, 2, 100)[1][:64], a[1])


# ---- the module on the host ---------------------------------------------------------------------------------------------------------------
def test_defaults_have_no_buffers_and_the_same_keys():
    vq = L2Quantizer(torch.randn(16, 4))
    assert list(vq.state_dict().keys()) == ["codebook"]
    assert list(vq.buffers()) == [] and vq.codebook.requires_grad
    assert [n for n, _ in vq.named_parameters()] == ["codebook"]


def test_ema_adds_three_buffers_and_freezes_the_codebook():
    cb = torch.randn(16, 4)
    vq = L2Quantizer(cb, codebook_update="ema", dead_code_threshold=1.0)
    assert list(vq.state_dict().keys()) == ["codebook", "cluster_size", "embed_avg", "ema_step"]
    assert not vq.codebook.requires_grad
    assert vq.cluster_size.dtype == torch.float32 and vq.cluster_size.shape == (16,) and not vq.cluster_size.any()
    assert torch.equal(vq.embed_avg, cb) and vq.embed_avg.dtype == torch.float32
    assert vq.ema_step.dtype == torch.int64 and vq.ema_step.tolist() == [0]
    fresh = L2Quantizer(torch.zeros(16, 4), codebook_update="ema")
    fresh.load_state_dict(vq.state_dict(), strict=True)
    assert torch.equal(fresh.codebook, vq.codebook)


@pytest.mark.parametrize("kw", [dict(decay=0.0), dict(decay=1.0), dict(decay=1.5), dict(commitment_weight=-0.1),
                                dict(dead_code_threshold=-1.0), dict(codebook_update="kmeans"), dict(eps=0.0), dict(eps=-1e-5)])
def test_bad_arguments_raise(kw):
    with pytest.raises(ValueError):
        L2Quantizer(torch.randn(8, 4), **kw)


def _cfg(**extra):
    return SimpleNamespace(tokenizer=SimpleNamespace(model=SimpleNamespace(
        patch_size=[4, 8, 8], fsq_levels=None, quantizer="l2", codebook_size=32, token_size=8, encoder_size="tiny", decoder_size="tiny", **extra)))


def test_titok_reads_the_keys():
    from titok_video_amd.model.titok import TiTok
    from titok_video_amd.train import make_optimizer
    plain = TiTok(_cfg())
    q = plain.quantize
    assert (q.commitment_weight, q.codebook_update, q.dead_code_threshold) == (0.0, "grad", 0.0) and list(q.buffers()) == []
    assert "quantize.codebook" in plain.state_dict() and not any("cluster_size" in k for k in plain.state_dict())
    m = TiTok(_cfg(commitment_weight=0.25, codebook_update="ema", codebook_decay=0.8, codebook_eps=1e-4, dead_code_threshold=1.5, codebook_seed=11))
    q = m.quantize
    assert (q.commitment_weight, q.codebook_update, q.decay, q.eps, q.dead_code_threshold, q.seed) == (0.25, "ema", 0.8, 1e-4, 1.5, 11)
    assert {"quantize.codebook", "quantize.cluster_size", "quantize.embed_avg", "quantize.ema_step"} <= set(m.state_dict())
    assert torch.equal(m.quantize.codebook, TiTok(_cfg(codebook_seed=11)).quantize.codebook)
    opt = make_optimizer(m)
    assert all(p is not q.codebook for g in opt.param_groups for p in g["params"])


# ---- the C entries refuse bad arguments without a GPU --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handle():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


def test_cabi_argument_checks(handle):
    err = lambda: handle.ttv_error_string().decode()
    p, odd = C.c_void_p(256), C.c_void_p(260)
    big = 1 << 30
    assert handle.ttv_vq_train_workspace_bytes(0, 8) == -1 and "rows" in err()
    assert handle.ttv_vq_train_workspace_bytes(4099, 1000) >= 4 * (3 * 4099 + 1001)
    f = handle.ttv_vq_commit_forward
    assert f(None, 0, 8, p, 8, p, 4, 16, 8, p, p, big, None) == 1 and "null" in err()
    assert f(odd, 0, 8, p, 8, p, 4, 16, 8, p, p, big, None) == 1 and "aligned" in err()
    assert f(p, 2, 8, p, 8, p, 4, 16, 8, p, p, big, None) == 1 and "dtype" in err()
    assert f(p, 0, 8, p, 8, p, 4, 16, 65, p, p, big, None) == 1 and "dim" in err()
    assert f(p, 0, 8, p, 8, p, 4, 16, 8, p, p, 8, None) == 1 and "workspace" in err()
    assert f(p, 0, 8, p, 8, p, 1 << 24, 16, 8, p, p, big, None) == 1 and "rows" in err()
    b = handle.ttv_vq_commit_backward
    assert b(p, 8, p, 8, None, 8, 0, 4, 8, 0.1, p, 8, None) == 1 and "null" in err()
    assert b(p, 8, p, 8, odd, 8, 0, 4, 8, 0.1, p, 8, None) == 1 and "aligned" in err()
    assert b(p, 4, p, 8, p, 8, 0, 4, 8, 0.1, p, 8, None) == 1 and "leading" in err()
    s = handle.ttv_vq_ema_stats
    assert s(p, 0, 8, None, 4, 16, 8, None, 0.0, 0, None, 0, 1, p, p, big, None) == 1 and "null" in err()
    assert s(odd, 0, 8, p, 4, 16, 8, None, 0.0, 0, None, 0, 1, p, p, big, None) == 1 and "aligned" in err()
    assert s(p, 0, 8, p, 4, 16, 8, None, 0.0, 0, None, 2, 2, p, p, big, None) == 1 and "rank" in err()
    assert s(p, 0, 8, p, 4, 16, 8, p, 1.0, 0, None, 0, 1, p, p, big, None) == 1 and "step" in err()
    assert s(p, 0, 8, p, 1 << 24, 16, 8, None, 0.0, 0, None, 0, 1, p, p, big, None) == 1 and "2^24" in err()
    u = handle.ttv_vq_ema_update
    assert u(p, p, p, p, p, 0, p, None, 16, 8, 0.99, 0.01, 1e-5, 0.0, p, big, None) == 1 and "null" in err()
    assert u(p, p, p, p, p, 0, p, odd, 16, 8, 0.99, 0.01, 1e-5, 0.0, p, big, None) == 1 and "aligned" in err()
    assert u(p, p, p, p, p, 0, p, p, 16, 8, 1.0, 0.01, 1e-5, 0.0, p, big, None) == 1 and "decay" in err()
    assert u(p, p, p, p, p, 0, p, p, 16, 8, 0.99, 0.01, 0.0, 0.0, p, big, None) == 1 and "eps" in err()
    assert u(p, p, p, p, C.c_void_p(512), 1, p, p, 16, 8, 0.99, 0.01, 1e-5, 0.0, p, big, None) == 1 and "itself" in err()
    assert u(p, p, p, p, p, 0, p, p, 16, 8, 0.99, 0.01, 1e-5, 0.0, p, 16, None) == 1 and "workspace" in err()


def test_gpu_only():
    vq = L2Quantizer(torch.randn(8, 4), commitment_weight=0.5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        vq(torch.randn(3, 4))


# ---- two gloo ranks: one all-reduce of count | sum | cand ---------------------------------------------------------------------------------
N_DP, C_DP, T_DP, SEED_DP, STEP_DP = 24, 6, 1.0, 9, 4


def _dp_rows(rank):
    rng = np.random.default_rng(100 + rank)
    rows = 50 + 13 * rank                                   # ranks hold different numbers of rows
    return rng.standard_normal((rows, C_DP)).astype(np.float32), rng.integers(0, N_DP, rows)


def _dp_cluster_size():
    cs = np.full(N_DP, 2.0, np.float32)
    cs[::3] = 0.25                                          # dead at t = 1: the same on every rank
    return cs


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        z, idx = _dp_rows(rank)
        count, s = R.stats_f32(z, idx, N_DP)
        cand = R.candidates(z, _dp_cluster_size(), T_DP, SEED_DP, STEP_DP, rank, world)
        buf = torch.from_numpy(R.flat_stats(count, s, cand))
        vq = L2Quantizer(torch.zeros(N_DP, C_DP), codebook_update="ema", dead_code_threshold=T_DP, seed=SEED_DP)
        assert vq._world() == (rank, world)
        vq.reduce_stats(buf)
        q.put((rank, buf.numpy().copy()))
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks_reduce_the_flat_buffer():
    import torch.multiprocessing as mp
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert np.array_equal(res[0], res[1])                    # every rank applies the same update
    buf = res[0]
    zs, idxs = zip(*[_dp_rows(r) for r in range(world)])
    count = buf[:N_DP]
    assert np.array_equal(count, np.bincount(np.concatenate(idxs), minlength=N_DP).astype(np.float32))
    s = buf[N_DP:N_DP + N_DP * C_DP].reshape(N_DP, C_DP)
    parts = [R.stats_f32(z, i, N_DP)[1] for z, i in zip(zs, idxs)]
    assert np.array_equal(s, (parts[0] + parts[1]).astype(np.float32))
    # cand: the drawn row of the rank the draw named, exactly (the other rank adds zeros)
    cand = buf[N_DP + N_DP * C_DP:].reshape(N_DP, C_DP)
    dead = _dp_cluster_size() < T_DP
    rk = R.draw(SEED_DP, STEP_DP, N_DP, world, 1)[0]
    assert set(rk[dead].tolist()) == {0, 1}, "the case must restart from both ranks"
    for n in range(N_DP):
        if dead[n]:
            z = zs[rk[n]]
            row = R.draw(SEED_DP, STEP_DP, N_DP, world, len(z))[1][n]
            assert np.array_equal(cand[n], z[row])
        else:
            assert not cand[n].any()
