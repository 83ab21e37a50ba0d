"""JEDi's feature extractor on the GPU (ttv_vjepa.hip) against float64 restatements: the preprocessing, each GEMM epilogue at the
network's shapes, LayerNorm, both attentions, the 2-layer and the full 24-layer tower with the pooler (tests/vjepa_ref.py), batch
independence, determinism and EvalMetrics end to end."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import vjepa_ref as R
from titok_video_amd import _lib
from titok_video_amd.model.metrics import jedi as J
from titok_video_amd.synthetic import seeded_probe_state, seeded_vjepa_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D, TOK, KIN = 1024, 1568, 1536


def _stream():
    return _lib.stream_ptr(DEV)


def _clips(shapes, dtype, seed, scale=1.3):
    g = torch.Generator().manual_seed(seed)
    return [((torch.rand((3,) + tuple(s), generator=g) * 2 - 1) * scale).to(DEV, dtype) for s in shapes]


def _rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm(dim=-1) / b.norm(dim=-1)).max().item()


@pytest.fixture(scope="module")
def model2():
    return J.VJEPA(J.vjepa_state_dict(seeded_vjepa_state(2, 3)), J.probe_state_dict(seeded_probe_state(4))).to(DEV)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_preprocess_matches_interpolate(dtype):
    shapes = [(1, 64, 64), (3, 128, 128), (8, 168, 168), (16, 300, 300), (5, 224, 224)]
    clips = _clips(shapes, dtype, 11)
    out = torch.empty(len(clips) * TOK, KIN, dtype=torch.bfloat16, device=DEV)
    J.VJEPA.preprocess(None, clips, out)
    torch.cuda.synchronize()
    for i, c in enumerate(clips):
        ref = R.patch_rows(R.preprocess(c.float()))                      # torch's F.interpolate on the device, fp32
        got = out[i * TOK:(i + 1) * TOK].float()
        exact = got == ref.to(torch.bfloat16).float()
        # the same fp32 value rounded to bf16, but for values whose fp32 sum lands on the other side of a bf16 rounding boundary
        # (fp32 summation order, a few fp32 ulps of the taps' magnitude): those may differ by one bf16 ulp
        ulp = 2.0 ** (torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -30))) - 7)
        assert ((got - ref).abs() <= ulp * 1.0001 + 4e-6).all(), f"clip {i}: more than one bf16 ulp off"
        assert exact.float().mean().item() > 0.999, f"clip {i}: {1 - exact.float().mean().item():.2e} of values differ from bf16(ref)"


def test_preprocess_refuses_bad_shapes():
    m = J.VJEPA.preprocess
    out = torch.empty(TOK, KIN, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="square"):
        m(None, [torch.zeros(3, 4, 64, 96, device=DEV)], out)
    with pytest.raises(ValueError, match="17 frames"):
        m(None, [torch.zeros(3, 17, 64, 64, device=DEV)], out)


LINEARS = [("patch", D, KIN, _lib.TTV_VJEPA_EPI_RESID), ("qkv", 3 * D, D, _lib.TTV_VJEPA_EPI_STORE),
           ("fc1", 4 * D, D, _lib.TTV_VJEPA_EPI_GELU), ("proj", D, D, _lib.TTV_VJEPA_EPI_RESID),
           ("fc2", D, 4 * D, _lib.TTV_VJEPA_EPI_RESID), ("kv", 2 * D, D, _lib.TTV_VJEPA_EPI_STORE)]


@pytest.mark.parametrize("M", [TOK, 3 * TOK])
@pytest.mark.parametrize("name,N,K,epi", LINEARS, ids=[l[0] for l in LINEARS])
def test_linear_epilogues(name, N, K, epi, M):
    g = torch.Generator(device=DEV).manual_seed(N + K + M)
    x = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV, generator=g) * K ** -0.5).to(torch.bfloat16)
    b = (torch.randn(N, device=DEV, generator=g) * 0.1).to(torch.bfloat16)
    acc = x.double() @ w.double().T + b.double()
    rows = TOK if name == "patch" else 0
    if epi == _lib.TTV_VJEPA_EPI_RESID:
        resid = torch.randn(rows or M, N, device=DEV, generator=g)
        y = resid.clone() if not rows else torch.empty(M, N, device=DEV)
        rc = _lib.lib().ttv_vjepa_linear(x.data_ptr(), K, w.data_ptr(), K, b.data_ptr(), M, N, K, epi, resid.data_ptr(), N, rows,
                                         y.data_ptr(), N, _stream())
        _lib.check(rc, "ttv_vjepa_linear")
        r = resid.double().repeat(M // TOK, 1) if rows else resid.double()
        tol = acc.abs() * 2.0 ** -8 + 1e-4
        assert ((y.double() - r - acc).abs() <= tol).all()
    else:
        y = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
        rc = _lib.lib().ttv_vjepa_linear(x.data_ptr(), K, w.data_ptr(), K, b.data_ptr(), M, N, K, epi, None, 0, 0, y.data_ptr(), N, _stream())
        _lib.check(rc, "ttv_vjepa_linear")
        ref = F.gelu(acc) if epi == _lib.TTV_VJEPA_EPI_GELU else acc
        tol = ref.abs() * 2.0 ** -7 + 2e-3
        assert ((y.double() - ref).abs() <= tol).all()


@pytest.mark.parametrize("dual", [False, True])
def test_layernorm(dual):
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(777, D, device=DEV, generator=g) * 3 + 0.5
    w1, b1, w2, b2 = (1 + 0.1 * torch.randn(D, device=DEV, generator=g), 0.1 * torch.randn(D, device=DEV, generator=g),
                      1 + 0.1 * torch.randn(D, device=DEV, generator=g), 0.1 * torch.randn(D, device=DEV, generator=g))
    y32 = torch.empty_like(x)
    y16 = torch.empty(777, D, dtype=torch.bfloat16, device=DEV)
    rc = _lib.lib().ttv_vjepa_layernorm(x.data_ptr(), D, 777, D, w1.data_ptr(), b1.data_ptr(), 1e-6, w2.data_ptr() if dual else None,
                                        b2.data_ptr() if dual else None, 1e-5, y32.data_ptr(), D, y16.data_ptr(), D, _stream())
    _lib.check(rc, "ttv_vjepa_layernorm")
    r1 = R.layer_norm(x.double(), w1.double(), b1.double(), 1e-6)
    assert (y32.double() - r1).abs().max().item() < 1e-5
    r2 = R.layer_norm(r1, w2.double(), b2.double(), 1e-5) if dual else r1
    assert ((y16.double() - r2).abs() <= r2.abs() * 2.0 ** -8 + 1e-5).all()


def test_pool_attention():
    n = 3
    g = torch.Generator(device=DEV).manual_seed(6)
    q = torch.randn(D, device=DEV, generator=g).to(torch.bfloat16)
    kv = torch.randn(n * TOK, 2 * D, device=DEV, generator=g).to(torch.bfloat16)
    out = torch.empty(n, D, dtype=torch.bfloat16, device=DEV)
    _lib.check(_lib.lib().ttv_vjepa_pool_attention(q.data_ptr(), kv.data_ptr(), n, TOK, out.data_ptr(), _stream()), "pool attention")
    for c in range(n):
        k, v = kv[c * TOK:(c + 1) * TOK].double().chunk(2, -1)
        ref = R.mha(q.double()[None], k, v, 16)[0]
        assert ((out[c].double() - ref).abs() <= ref.abs() * 2.0 ** -7 + 1e-3).all()


def test_attention_1568_rows_16_heads():
    """ttv_attention as the encoder calls it: no gate, q_heads == kv_heads == 16, q | unused | k | v rows of 4096."""
    n = 2
    g = torch.Generator(device=DEV).manual_seed(7)
    qkv = torch.randn(n * TOK, 4 * D, device=DEV, generator=g).to(torch.bfloat16)
    tab = torch.tensor([[s, qb * 128, h, 0] for s in range(n) for h in range(16) for qb in range(13)], dtype=torch.int32, device=DEV)
    cu = torch.tensor([i * TOK for i in range(n + 1)], dtype=torch.int32, device=DEV)
    out = torch.empty(n * TOK, D, dtype=torch.bfloat16, device=DEV)
    rc = _lib.lib().ttv_attention(qkv.data_ptr(), 4 * D, out.data_ptr(), D, cu.data_ptr(), tab.data_ptr(), tab.shape[0], 16, 16, 64, 0,
                                  _lib.TTV_BF16, _stream())
    _lib.check(rc, "ttv_attention")
    for s in range(n):
        rows = qkv[s * TOK:(s + 1) * TOK].double()
        ref = R.mha(rows[:, :D], rows[:, 2 * D:3 * D], rows[:, 3 * D:], 16)
        err = (out[s * TOK:(s + 1) * TOK].double() - ref).abs().max().item()
        assert err < 2e-2 * ref.abs().max().item()


def _ref_feats(clips, enc, probe, finetuned=True, bf16=True):
    return torch.stack([R.features(c, enc, probe, finetuned, bf16=bf16) for c in clips])


def test_two_layer_tower_and_pooler(model2):
    clips = _clips([(16, 128, 128), (5, 96, 96), (16, 224, 224)], torch.bfloat16, 21)
    got = model2.features([clips])
    ref = _ref_feats(clips, model2.host, model2.probe)
    e_replay = _rel_l2(got, ref)
    e_f64 = _rel_l2(got, _ref_feats(clips, model2.host, model2.probe, bf16=False))
    print(f"\n2-layer tower + pooler: relative L2 per feature vector {e_replay:.3e} vs the bf16-point replay, {e_f64:.3e} vs float64")
    assert e_replay < 2e-2 and e_f64 < 2e-2


def test_not_finetuned(model2):
    clips = _clips([(8, 128, 128), (16, 64, 64)], torch.float32, 22)
    got = model2.features([clips], finetuned=False)
    ref = _ref_feats(clips, model2.host, None, finetuned=False)
    e = _rel_l2(got, ref)
    print(f"\nfinetuned=False: relative L2 {e:.3e}")
    assert e < 2e-2


def test_batch_independence_and_determinism(model2):
    clips = _clips([(16, 128, 128)] * 32, torch.bfloat16, 23)
    alone = model2.features([clips[:1]])
    batch = model2.features([clips[1:16], clips[:1], clips[16:]])
    again = model2.features([clips[1:16], clips[:1], clips[16:]])
    assert torch.equal(alone[0], batch[15])
    assert torch.equal(batch, again)


def test_full_vit_large_with_pooler():
    m = J.VJEPA(J.vjepa_state_dict(seeded_vjepa_state(24, 8)), J.probe_state_dict(seeded_probe_state(9))).to(DEV)
    clips = _clips([(16, 128, 128), (9, 224, 224)], torch.bfloat16, 24)
    got = m.features([clips])
    e_replay = _rel_l2(got, _ref_feats(clips, m.host, m.probe))
    e_f64 = _rel_l2(got, _ref_feats(clips, m.host, m.probe, bf16=False))
    print(f"\nViT-L/16 x 24 + pooler: relative L2 per feature vector {e_replay:.3e} vs the bf16-point replay, {e_f64:.3e} vs float64")
    assert e_replay < 2e-2 and e_f64 < 2e-2


def test_eval_metrics_end_to_end():
    from titok_video_amd.model.metrics.eval_metrics import EvalMetrics

    enc, probe = seeded_vjepa_state(2, 12), seeded_probe_state(13)
    cfg = SimpleNamespace(training=SimpleNamespace(eval=SimpleNamespace(log_metrics=["psnr", "jedi"], jedi_jepa_model="vit_large")))
    em = EvalMetrics(cfg, jedi_weights=enc, jedi_probe=probe)
    assert not any("jedi" in k or "pooler" in k or "blocks" in k for k in em.state_dict())
    target = _clips([(8, 64, 64)] * 5, torch.bfloat16, 30, scale=1.0)
    g = torch.Generator(device=DEV).manual_seed(31)
    recon = [(t.float() + 0.3 * torch.randn(t.shape, device=DEV, generator=g)).to(torch.bfloat16) for t in target]
    em.update(recon, target)
    out = em.compute()
    rf = _ref_feats([r.clamp(-1, 1) for r in recon], J.vjepa_state_dict(enc), J.probe_state_dict(probe))
    tf = _ref_feats(target, J.vjepa_state_dict(enc), J.probe_state_dict(probe))
    ref = J.mmd_poly(tf.cpu().numpy(), rf.cpu().numpy()) * 100
    print(f"\nEvalMetrics jedi {out['eval/jedi']:.6g}, restatement {ref:.6g}")
    assert math.isfinite(out["eval/jedi"]) and abs(out["eval/jedi"] - ref) <= 0.05 * abs(ref) + 1e-6
    em.reset()
    assert math.isnan(em.compute()["eval/jedi"])
