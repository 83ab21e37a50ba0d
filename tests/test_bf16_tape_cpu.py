"""tests/bf16_tape.py, the float64 replay of the bf16 training tape (no GPU):

  * rounding off, it IS the oracle's model: output and every gradient equal the oracle's float64 autograd to 1e-10 (with the oracle's
    three fp32-computing primitives - rmsnorm, apply_rotary, attention_varlen - evaluated in float64), and the oracle as it stands to
    fp32 precision;
  * rounding on, the values at its F points are bf16 numbers;
  * the gap - the global distance between the rounded replay's gradients and the unrounded ones - is what the GPU tests
    (tests/test_hip_backward_bf16.py) hold the HIP backward to half of."""
import pytest
import torch

from oracle import titok_oracle as O
from tests import bf16_tape as T
from titok_video_amd.synthetic import seeded_titok_state, synthetic_clips

SHAPES, COUNTS = [(4, 16, 16), (8, 32, 48), (4, 8, 24)], [2, 5, 3]


def _bf16_state():
    return {k: v.to(torch.bfloat16) for k, v in seeded_titok_state(0).items()}


def _inputs():
    g = torch.Generator().manual_seed(4)
    wz = torch.randn(sum(COUNTS), 5, generator=g, dtype=torch.float64)
    clips = [c.to(torch.bfloat16) for c in synthetic_clips(SHAPES, seed=8)]
    codes = O.fsq_indices_to_codes(torch.randint(0, 4375, (sum(COUNTS),), generator=g, dtype=torch.int32), [7, 5, 5, 5, 5])
    w = [torch.randn((3,) + s, generator=g).to(torch.bfloat16) for s in SHAPES]
    return wz, clips, codes, w


@pytest.fixture
def float64_oracle(monkeypatch):
    """The oracle with rmsnorm / apply_rotary / attention_varlen computing in float64 (they cast to fp32 by definition)."""
    monkeypatch.setattr(O, "rmsnorm", lambda x, w, eps=O.RMS_EPS: T.rmsnorm64(x, w.to(x.dtype), eps))
    monkeypatch.setattr(O, "apply_rotary", lambda x, c, s: T.rotate64(x, c.to(x.dtype), s.to(x.dtype)))
    monkeypatch.setattr(O, "attention_varlen", lambda q, k, v, cu: T._Attention64.apply(q, k, v, cu, False))
    return O


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-300))


def _oracle_encoder(sd, clips, wz):
    p = T._leaves(sd, "encoder.")
    cl = [c.double().requires_grad_(True) for c in clips]
    z = O.encoder_forward(cl, COUNTS, p, "tiny", (4, 8, 8), prefix="encoder.")
    (z * wz).sum().backward()
    return z.detach(), {k: v.grad for k, v in p.items()}, [c.grad for c in cl]


def _oracle_decoder(sd, codes, w):
    p = T._leaves(sd, "decoder.")
    cd = codes.double().requires_grad_(True)
    recon = O.titok_decode(cd, COUNTS, SHAPES, p)
    sum((c * wc.double()).sum() for c, wc in zip(recon, w)).backward()
    return [c.detach() for c in recon], {k: v.grad for k, v in p.items()}, cd.grad


def _replay_encoder(sd, clips, wz, **kw):
    got, gclips = T.encoder_grads(sd, clips, COUNTS, wz, **kw)
    p = T._leaves(sd, "encoder.")
    with torch.no_grad():
        z = T.encoder_replay([c.double() for c in clips], COUNTS, p, r=T.Rounding(kw.get("rounding", True)))
    return z, got, gclips


def test_unrounded_replay_is_the_float64_oracle(float64_oracle):
    sd = _bf16_state()
    wz, clips, codes, w = _inputs()
    z_ref, ref, ref_clips = _oracle_encoder(sd, clips, wz)
    z, got, gclips = _replay_encoder(sd, clips, wz, rounding=False)
    assert _rel(z, z_ref) < 1e-10
    assert set(got) == set(ref) and len(ref) == 4 * 6 + 3 * 2 + 8
    for k in ref:
        assert _rel(got[k], ref[k]) < 1e-10, (k, _rel(got[k], ref[k]))
    for a, b in zip(gclips, ref_clips):
        assert _rel(a, b) < 1e-10
    rec_ref, ref, ref_codes = _oracle_decoder(sd, codes, w)
    got, gcodes = T.decoder_grads(sd, codes, COUNTS, SHAPES, w, rounding=False)
    with torch.no_grad():
        rec = T.decoder_replay(codes.double(), COUNTS, SHAPES, T._leaves(sd, "decoder."), r=T.Rounding(False))
    for a, b in zip(rec, rec_ref):
        assert _rel(a, b) < 1e-10
    for k in ref:
        assert _rel(got[k], ref[k]) < 1e-10, (k, _rel(got[k], ref[k]))
    assert _rel(gcodes, ref_codes) < 1e-10


def test_unrounded_replay_matches_the_oracle_as_it_stands():
    """The same comparison against the unpatched oracle (fp32 norms, rotary and attention): fp32 precision."""
    sd = _bf16_state()
    wz, clips, codes, w = _inputs()
    z_ref, ref, _ = _oracle_encoder(sd, clips, wz)
    z, got, _ = _replay_encoder(sd, clips, wz, rounding=False)
    assert _rel(z, z_ref) < 1e-5
    assert T.global_distance(got, ref) < 1e-5
    _, ref, _ = _oracle_decoder(sd, codes, w)
    got, _ = T.decoder_grads(sd, codes, COUNTS, SHAPES, w, rounding=False)
    assert T.global_distance(got, ref) < 1e-5


def _is_bf16(x):
    return torch.equal(x, x.to(torch.bfloat16).double())


def test_rounded_replay_holds_bf16_values_at_its_tape_points():
    sd = _bf16_state()
    wz, clips, codes, w = _inputs()
    rec = {}
    T.encoder_grads(sd, clips, COUNTS, wz, record=rec)
    for name in ("pe", "X0", "l0.xn1", "l0.qkvg", "l1.a", "l1.ag", "l2.y1", "l2.x1", "l3.u", "l3.h", "l3.y2", "l3.X", "n"):
        assert rec[name].dtype == torch.float64 and _is_bf16(rec[name]), name
        assert not torch.equal(rec[name], torch.zeros_like(rec[name])), name
    assert rec["l3.h"].shape[1] == 704 and rec["l3.u"].shape[1] == 1408
    rec = {}
    T.decoder_grads(sd, codes, COUNTS, SHAPES, w, record=rec)
    for name in ("hpre", "X0", "l1.qkvg", "l3.X", "pn", "recon"):
        assert _is_bf16(rec[name]), name
    rec = {}
    T.encoder_grads(sd, clips, COUNTS, wz, y_bf16=False, record=rec)        # TTV_TAPE_Y_F32 / TTV_TRAIN_FUSED_NORMS: no y1 / y2 rounding
    assert "l1.y1" not in rec and "l1.y2" not in rec and _is_bf16(rec["l1.x1"])


def test_rounding_changes_the_gradients_by_the_gap():
    """The gap of both towers: far above the 1e-10 of the unrounded replay, far below the 0.12 the bf16 tower checks allowed."""
    sd = _bf16_state()
    wz, clips, codes, w = _inputs()
    exact, _ = T.encoder_grads(sd, clips, COUNTS, wz, rounding=False)
    rounded, _ = T.encoder_grads(sd, clips, COUNTS, wz)
    keep_y, _ = T.encoder_grads(sd, clips, COUNTS, wz, y_bf16=False)
    gap_e, gap_ey = T.global_distance(rounded, exact), T.global_distance(keep_y, exact)
    exact, _ = T.decoder_grads(sd, codes, COUNTS, SHAPES, w, rounding=False)
    rounded, _ = T.decoder_grads(sd, codes, COUNTS, SHAPES, w)
    gap_d = T.global_distance(rounded, exact)
    print(f"bf16 tape gap (rounded replay vs float64): encoder {gap_e:.3e} (y unrounded {gap_ey:.3e}), decoder {gap_d:.3e}")
    for gap in (gap_e, gap_ey, gap_d):
        assert 1e-3 < gap < 0.1
