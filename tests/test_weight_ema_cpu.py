"""Host side of `WeightEMA` (titok_video_amd/ema.py): the bound of tests/weight_ema_ref.py is valid and it bites, the decay schedule,
the argument checks of the two C entries, the checkpoint layout, and the capture guard.  No GPU."""
import ctypes as C
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import weight_ema_ref as R  # noqa: E402

from titok_video_amd import _lib  # noqa: E402
from titok_video_amd.checkpoint import load_checkpoint, save_checkpoint  # noqa: E402
from titok_video_amd.ema import ShadowState, WeightEMA  # noqa: E402

MAGNITUDES = [2.0 ** e for e in range(-20, 5, 4)]          # 2^-20 ... 2^4


def cases():
    """(tag, p, s) as float32 arrays: every magnitude, p close to s (a few ulp, a relative 1e-3) and far from it (independent, of the
    other sign, of another magnitude), p an fp32 or a bf16 value."""
    rng = np.random.default_rng(0)
    n = 4096
    for m in MAGNITUDES:
        s = (rng.standard_normal(n) * m).astype(np.float32)
        yield f"{m:g} ulps", np.nextafter(s, np.float32(np.inf)).astype(np.float32), s
        yield f"{m:g} close", (s * np.float32(1.001)).astype(np.float32), s
        yield f"{m:g} independent", (rng.standard_normal(n) * m).astype(np.float32), s
        yield f"{m:g} opposite", (-s * np.float32(1.5)).astype(np.float32), s
        yield f"{m:g} larger", (rng.standard_normal(n) * m * 256).astype(np.float32), s
        yield f"{m:g} smaller", (rng.standard_normal(n) * m / 256).astype(np.float32), s
        pb = torch.from_numpy(rng.standard_normal(n).astype(np.float32) * np.float32(m)).to(torch.bfloat16).float().numpy()
        yield f"{m:g} bf16", pb, s


def emulate(p, s, w, fma=False):
    """The kernel's three operations in float32 numpy (fma=True: product and sum rounded once, through float64 - the product of two
    floats is exact there)."""
    wf = np.float32(w)
    d = (p - s).astype(np.float32)
    if fma:
        return (s.astype(np.float64) + wf.astype(np.float64) * d.astype(np.float64)).astype(np.float32)
    return (s + (wf * d).astype(np.float32)).astype(np.float32)


@pytest.mark.parametrize("w", R.W_GRID)
def test_the_bound_holds_for_a_float32_emulation(w):
    worst = 0.0
    for tag, p, s in cases():
        for fma in (False, True):
            got = emulate(p, s, w, fma)
            fails, frac = R.check(p.astype(np.float64), s.astype(np.float64), got.astype(np.float64), w, f"w {w} {tag} fma {fma}")
            assert not fails, fails
            worst = max(worst, frac)
    print(f"w = {w!r}: largest error {worst:.3f} of its bound")
    assert 0.0 < worst <= 1.0


def test_the_bound_rejects_a_bf16_shadow_and_a_result_four_ulp_off():
    rng = np.random.default_rng(1)
    n = 4096
    for w in (1.0 - 0.9999, 1.0 - 0.999):
        for m in MAGNITUDES:
            s = torch.from_numpy((rng.standard_normal(n) * m).astype(np.float32)).to(torch.bfloat16).float().numpy()
            p = (s * np.float32(1.25)).astype(np.float32)
            # a shadow kept in bf16: the increment w |p - s| = w |s| / 4 is below half a bf16 ulp (2^-9 |s| at least), the shadow stands still
            kept = torch.from_numpy(emulate(p, s, w)).to(torch.bfloat16).float().numpy()
            assert np.array_equal(kept, s)
            live = s != 0
            outside = np.abs(kept.astype(np.float64) - R.replay(p.astype(np.float64), s.astype(np.float64), w)) > R.bound(p.astype(np.float64), s.astype(np.float64), w)
            assert outside[live].all(), (w, m)
            # the float32 result moved by 4 ulp: more than 3.5 u |s*| off, the bound is u |s*| (1 + 3 w / 4) + 2^-125
            good = emulate(p, s, w)
            moved = good.copy()
            for _ in range(4):
                moved = np.nextafter(moved, np.float32(np.inf)).astype(np.float32)
            fails, _ = R.check(p.astype(np.float64), s.astype(np.float64), moved.astype(np.float64), w)
            assert fails, (w, m)
            err = np.abs(moved.astype(np.float64) - R.replay(p.astype(np.float64), s.astype(np.float64), w))
            assert (err > R.bound(p.astype(np.float64), s.astype(np.float64), w))[live].all(), (w, m)


class _Tiny(torch.nn.Module):
    """Two floating parameters (one frozen), one integer parameter and a buffer."""

    def __init__(self, dtype=torch.float32):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        self.a = torch.nn.Parameter(torch.randn(5, 3, generator=g).to(dtype))
        self.b = torch.nn.Parameter(torch.randn(7, generator=g).to(dtype), requires_grad=False)
        self.steps = torch.nn.Parameter(torch.arange(4), requires_grad=False)
        self.register_buffer("stat", torch.randn(2, generator=g))


@pytest.mark.parametrize("warmup", [True, False])
def test_decay_at_is_the_formula_in_double(warmup):
    for decay in (0.9999, 0.999, 0.5, 0.0, 1.0):
        st = ShadowState(_Tiny(), decay=decay, warmup=warmup)
        for t in (0, 1, 9, 10, 10 ** 4):
            want = min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay
            got = st.decay_at(t)
            assert isinstance(got, float) and got == want, (decay, t, got, want)
    assert ShadowState(_Tiny(), 0.9999, True).decay_at(0) == 0.1 and ShadowState(_Tiny(), 0.9999, True).decay_at(10 ** 6) == 0.9999
    for bad in (-0.1, 1.0001, float("nan")):
        with pytest.raises(ValueError, match="decay"):
            ShadowState(_Tiny(), decay=bad)


def test_shadows_are_exact_fp32_copies_of_the_floating_parameters():
    for dtype in (torch.float32, torch.bfloat16):
        m = _Tiny(dtype)
        st = ShadowState(m)
        assert list(st.shadow) == ["a", "b"] and all(v.dtype == torch.float32 for v in st.shadow.values())
        assert torch.equal(st.shadow["a"], m.a.detach().float()) and torch.equal(st.shadow["b"], m.b.detach().float())
        assert st.shadow["a"].data_ptr() != m.a.data_ptr()
        sd = st.model_state_dict()
        assert list(sd) == list(m.state_dict()) and all(sd[k].dtype == v.dtype for k, v in m.state_dict().items())
        st.shadow["a"].add_(1.0)
        sd = st.model_state_dict()
        assert torch.equal(sd["a"], (m.a.detach().float() + 1.0).to(dtype)) and torch.equal(sd["stat"], m.stat) and torch.equal(sd["steps"], m.steps)
        st.num_updates = 5
        st.reset()
        assert st.num_updates == 0 and torch.equal(st.shadow["a"], m.a.detach().float())


def test_state_dict_round_trip_is_strict():
    m = _Tiny()
    st = ShadowState(m, decay=0.999, warmup=False)
    st.shadow["a"].mul_(0.5)
    st.num_updates = 7
    sd = st.state_dict()
    assert list(sd) == ["decay", "warmup", "num_updates", "shadow"] and isinstance(sd["shadow"], OrderedDict) and list(sd["shadow"]) == ["a", "b"]
    other = ShadowState(_Tiny(), decay=0.5, warmup=True)
    other.load_state_dict(sd)
    assert (other.decay, other.warmup, other.num_updates) == (0.999, False, 7)
    assert all(torch.equal(other.shadow[k], st.shadow[k]) and other.shadow[k].data_ptr() != st.shadow[k].data_ptr() for k in st.shadow)
    was = {k: v.clone() for k, v in other.shadow.items()}
    for broken, err in (({"a": sd["shadow"]["a"]}, KeyError),
                        ({"a": sd["shadow"]["a"], "b": sd["shadow"]["b"], "c": sd["shadow"]["b"]}, KeyError),
                        ({"a": sd["shadow"]["a"].t().contiguous(), "b": sd["shadow"]["b"]}, ValueError)):
        with pytest.raises(err):
            other.load_state_dict({**sd, "shadow": OrderedDict(broken)})
        assert all(torch.equal(other.shadow[k], was[k]) for k in was), "a refused load changes nothing"


@pytest.fixture(scope="module")
def handle():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


def test_cabi_argument_checks(handle):
    err = lambda: handle.ttv_error_string().decode()          # noqa: E731
    fake = C.c_void_p(4096)          # never dereferenced: every call below returns before a launch
    for dtype in (_lib.TTV_F32, _lib.TTV_BF16):
        assert handle.ttv_opt_ema_update(None, None, 0, dtype, 0.5, None) == 0
        assert handle.ttv_opt_ema_exchange(None, None, 0, dtype, 0, None) == 0
        assert handle.ttv_opt_ema_exchange(None, None, 0, dtype, 1, None) == 0
    assert handle.ttv_opt_ema_update(fake, fake, 3, 7, 0.5, None) == 1 and "opt_ema_update" in err() and "dtype 7" in err()
    assert handle.ttv_opt_ema_exchange(fake, fake, 3, 7, 0, None) == 1 and "opt_ema_exchange" in err() and "dtype 7" in err()
    assert handle.ttv_opt_ema_exchange(fake, fake, 3, _lib.TTV_F32, 2, None) == 1 and "mode 2" in err()
    assert handle.ttv_opt_ema_exchange(fake, fake, 3, _lib.TTV_BF16, -1, None) == 1 and "mode -1" in err()
    assert handle.ttv_opt_ema_update(None, fake, 3, _lib.TTV_F32, 0.5, None) == 1 and "null" in err()
    assert handle.ttv_opt_ema_update(fake, None, 3, _lib.TTV_F32, 0.5, None) == 1 and "null" in err()
    assert handle.ttv_opt_ema_exchange(None, fake, 3, _lib.TTV_F32, 0, None) == 1 and "null" in err()
    assert handle.ttv_opt_ema_update(fake, fake, -1, _lib.TTV_F32, 0.5, None) == 1
    assert handle.ttv_opt_ema_exchange(fake, fake, -1, _lib.TTV_F32, 0, None) == 1


def test_checkpoint_keeps_the_reference_entries_and_round_trips_the_average(tmp_path):
    m = _Tiny()
    st = ShadowState(m, decay=0.999, warmup=False)
    st.shadow["a"].mul_(0.25)
    st.num_updates = 11
    plain, with_ema = str(tmp_path / "plain.ckpt"), str(tmp_path / "ema.ckpt")
    save_checkpoint(plain, m, global_step=42)
    save_checkpoint(with_ema, m, global_step=42, ema=st)
    a, b = torch.load(plain, weights_only=False), torch.load(with_ema, weights_only=False)
    assert list(a) == ["state_dict", "global_step"] and list(b) == ["state_dict", "global_step", "weight_ema"]
    assert a["global_step"] == b["global_step"] == 42 and list(a["state_dict"]) == list(b["state_dict"])
    for k, v in a["state_dict"].items():
        w = b["state_dict"][k]
        assert v.dtype == w.dtype and v.shape == w.shape and v.numpy().tobytes() == w.numpy().tobytes(), k
    saved = b["weight_ema"]
    assert (saved["decay"], saved["warmup"], saved["num_updates"]) == (0.999, False, 11)
    assert all(v.device.type == "cpu" and v.dtype == torch.float32 for v in saved["shadow"].values())
    # into a fresh model and a fresh average
    m2 = _Tiny()
    with torch.no_grad():
        m2.a.zero_()
    st2 = ShadowState(m2, decay=0.5, warmup=True)
    assert load_checkpoint(with_ema, m2, strict=True, ema=st2) == 42
    assert torch.equal(m2.a, m.a) and (st2.decay, st2.warmup, st2.num_updates) == (0.999, False, 11)
    assert all(torch.equal(st2.shadow[k], st.shadow[k]) for k in st.shadow)
    # a file without the entry: the average restarts from the loaded weights
    st2.num_updates = 3
    assert load_checkpoint(plain, m2, strict=True, ema=st2) == 42
    assert st2.num_updates == 0 and torch.equal(st2.shadow["a"], m.a.detach()) and torch.equal(st2.shadow["b"], m.b.detach())
    # and without an average given the file loads as before
    assert load_checkpoint(with_ema, _Tiny(), strict=True) == 42


def test_make_weight_ema_reads_the_config_and_stays_off_by_default():
    from types import SimpleNamespace
    from titok_video_amd.train import make_weight_ema
    m = _Tiny()
    for cfg in (SimpleNamespace(), SimpleNamespace(training=SimpleNamespace()), SimpleNamespace(training=SimpleNamespace(main=SimpleNamespace())),
                SimpleNamespace(training=SimpleNamespace(main=SimpleNamespace(ema_decay=0.0))),
                SimpleNamespace(training=SimpleNamespace(main=SimpleNamespace(ema_decay=None))),
                {"training": {"main": {"max_steps": 10}}}):
        assert make_weight_ema(m, cfg) is None
    with pytest.raises(RuntimeError, match="GPU only"):          # asked for: built, and a model on the host has no EMA path
        make_weight_ema(m, SimpleNamespace(training=SimpleNamespace(main=SimpleNamespace(ema_decay=0.999))))


def test_no_cpu_path_and_the_capture_guard(monkeypatch):
    m = _Tiny()
    with pytest.raises(RuntimeError, match="GPU only"):
        WeightEMA(m)
    # the guard is the first thing update() does: an instance with the host half only (no tables - WeightEMA() itself refuses a model
    # on the host), a library that must not be reached, and a stream that claims to be capturing
    ema = object.__new__(WeightEMA)
    ShadowState.__init__(ema, m, decay=0.9999, warmup=True)
    ema._applied = False

    def no_library():
        raise AssertionError("update() reached the library while the stream was capturing")
    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    was = {k: v.clone() for k, v in ema.shadow.items()}
    with pytest.raises(RuntimeError, match="capturing"):
        ema.update()
    assert ema.num_updates == 0 and all(torch.equal(ema.shadow[k], was[k]) for k in was)
