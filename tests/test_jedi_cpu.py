"""JEDi without a GPU: mmd_poly against sklearn's kernel formula and the reference's golden values, the identity path against the
direct one, the V-JEPA / probe state-dict loaders and their refusals, the shape refusals, the EvalMetrics surface, the C-ABI argument
checks, and the float64 restatement (tests/vjepa_ref.py) against explicit loops at a small width."""
import ctypes as C
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import vjepa_ref as R
from titok_video_amd import _lib
from titok_video_amd.model.metrics import jedi as J
from titok_video_amd.model.metrics.eval_metrics import EvalMetrics
from titok_video_amd.synthetic import seeded_probe_state, seeded_vjepa_state

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KAT = os.path.join(HERE, "golden", "jedi_kat.npz")


def _sklearn_formula(X, Y, degree=2, gamma=None, coef0=0):
    """sklearn.metrics.pairwise.polynomial_kernel's definition, in float64: K = (gamma X Y^T + coef0)^degree, gamma = 1 / d."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    g = 1.0 / X.shape[1] if gamma is None else gamma
    k = lambda a, b: (g * (a @ b.T) + coef0) ** degree
    return k(X, X).mean() + k(Y, Y).mean() - 2 * k(X, Y).mean()


@pytest.mark.parametrize("n,m,d", [(1, 1, 8), (2, 5, 16), (37, 37, 1024), (300, 120, 64)])
def test_mmd_poly_matches_kernel_formula(n, m, d):
    rng = np.random.default_rng(n + m + d)
    X, Y = rng.standard_normal((n, d)), 0.7 * rng.standard_normal((m, d)) + 0.2
    want = _sklearn_formula(X, Y)
    assert abs(J.mmd_poly(X, Y) - want) <= 1e-10 * abs(want)
    scale = _sklearn_formula(X, np.zeros_like(X))          # mean K(X, X): the size of the terms that cancel for identical sets
    assert abs(J.mmd_poly(X, X)) <= 1e-12 * scale


def test_identity_path_matches_direct_path():
    rng = np.random.default_rng(3)
    X, Y = rng.standard_normal((50, 32)), rng.standard_normal((70, 32)) * 1.1
    ident = J.mmd_poly(X, Y, degree=2, gamma=0.3, coef0=0)
    direct = J.mmd_poly(X, Y, degree=2, gamma=0.3, coef0=1e-300)     # any coef0 != 0 takes the direct kernel means
    assert abs(ident - direct) <= 1e-10 * abs(direct)
    want3 = _sklearn_formula(X, Y, degree=3, coef0=1.0)
    assert abs(J.mmd_poly(X, Y, degree=3, coef0=1.0) - want3) <= 1e-10 * abs(want3)


def test_mmd_poly_matches_reference_golden():
    kat = np.load(KAT)
    seed, dim = int(kat["seed"]), int(kat["dim"])

    def sets(i, n, dtype, same):
        rng = np.random.default_rng(seed + i)
        X = rng.standard_normal((n, dim)).astype(dtype)
        Y = X.copy() if same else (0.8 * rng.standard_normal((n, dim)) + 0.3).astype(dtype)
        return X, Y

    for i, (n, dt, same, want) in enumerate(zip(kat["n"], kat["dtype"], kat["same"], kat["mmd"])):
        X, Y = sets(i, int(n), str(dt), bool(same))
        got = J.mmd_poly(X, Y)
        # the reference runs sklearn in the features' dtype (float32 sets: float32 arithmetic); here always float64
        scale = _sklearn_formula(X, np.zeros_like(X))
        tol = (1e-5 if str(dt) == "float32" else 1e-10) * scale
        assert abs(got - want) <= tol, (i, got, want)
    for j, ((n, deg, c0), want) in enumerate(zip(kat["extra_cases"], kat["extra_mmd"])):
        X, Y = sets(100 + j, int(n), "float64", False)
        assert abs(J.mmd_poly(X, Y, degree=int(deg), coef0=float(c0)) - want) <= 1e-10 * abs(want)


def test_state_dict_loaders_nested_and_prefixed(tmp_path):
    enc, probe = seeded_vjepa_state(2, 0), seeded_probe_state(1)
    p1 = tmp_path / "vitl16.pth.tar"
    torch.save({"encoder": {"module.backbone." + k: v * 0 for k, v in enc.items()},
                "target_encoder": {"module.backbone." + k: v for k, v in enc.items()}, "epoch": 300}, p1)
    p2 = tmp_path / "ssv2-probe.pth.tar"
    cls = {"module." + k: v for k, v in probe.items()}
    cls["module.linear.weight"], cls["module.linear.bias"] = torch.zeros(174, 1024), torch.zeros(174)
    torch.save({"classifier": cls, "opt": {}}, p2)
    e, p = J.vjepa_state_dict(p1), J.probe_state_dict(p2)
    assert list(e) == list(J.encoder_shapes(2)) and all(torch.equal(e[k], enc[k]) for k in e)     # target_encoder wins
    assert list(p) == list(J.probe_shapes()) and all(torch.equal(p[k], probe[k]) for k in p)
    p3 = tmp_path / "encoder_only.pth.tar"
    torch.save({"encoder": {"module." + k: v for k, v in enc.items()}}, p3)
    assert all(torch.equal(J.vjepa_state_dict(p3)[k], enc[k]) for k in e)
    p4 = tmp_path / "flat.pt"
    torch.save(enc, p4)
    assert list(J.vjepa_state_dict(p4)) == list(e)
    q = J.pooler_query(p)
    assert q.dtype == torch.bfloat16 and q.shape == (1024,)


def test_loader_refusals():
    enc = seeded_vjepa_state(1, 0)
    with pytest.raises(ValueError, match="pos_embed"):
        J.vjepa_state_dict({k: v for k, v in enc.items() if k != "pos_embed"})
    bad = dict(enc)
    bad["blocks.0.mlp.fc1.weight"] = torch.zeros(4096, 1000)
    with pytest.raises(ValueError, match="blocks.0.mlp.fc1.weight"):
        J.vjepa_state_dict(bad)
    with pytest.raises(ValueError, match="blocks.0.attn.proj.bias"):
        J.vjepa_state_dict({k: v for k, v in enc.items() if k != "blocks.0.attn.proj.bias"})
    huge = dict(enc)
    huge["pos_embed"] = torch.zeros(1, 1568, 1280)
    with pytest.raises(NotImplementedError, match="head_dim 80"):
        J.vjepa_state_dict(huge)
    probe = seeded_probe_state(0)
    del probe["pooler.cross_attention_block.xattn.kv.bias"]
    with pytest.raises(ValueError, match="xattn.kv.bias"):
        J.probe_state_dict(probe)
    with pytest.raises(NotImplementedError, match="vit_huge"):
        J.JEDiMetric(model_name="vit_huge", weights=enc, probe=seeded_probe_state(0))
    with pytest.raises(ValueError, match="jedi_weights"):
        J.JEDiMetric()


class _Dev:
    """Stand-in for a device tensor (shape / dtype / is_cuda only): the shape checks run before anything touches a GPU."""

    def __init__(self, *shape, dtype=torch.bfloat16):
        self.shape, self.dtype, self.is_cuda = torch.Size(shape), dtype, True

    def dim(self):
        return len(self.shape)


def test_shape_refusals_before_any_launch():
    with pytest.raises(ValueError, match="square"):
        J.check_clips([_Dev(3, 4, 64, 96)])
    with pytest.raises(ValueError, match="17 frames"):
        J.check_clips([_Dev(3, 17, 64, 64)])
    J.check_clips([_Dev(3, 16, 64, 64), _Dev(3, 1, 300, 300)])
    metric = J.JEDiMetric(weights=J.VJEPA(J.vjepa_state_dict(seeded_vjepa_state(1, 0)), J.probe_state_dict(seeded_probe_state(1))))
    with pytest.raises(ValueError, match="square"):
        metric.update_clips([_Dev(3, 16, 64, 64), _Dev(3, 8, 64, 32)], [_Dev(3, 16, 64, 64), _Dev(3, 8, 64, 64)])
    assert metric.model.device is None          # nothing was uploaded or launched


def _cfg(names, **extra):
    return SimpleNamespace(training=SimpleNamespace(eval=SimpleNamespace(log_metrics=names, **extra)))


def test_eval_metrics_surface():
    with pytest.raises(NotImplementedError, match="psnr, ssim"):
        EvalMetrics(_cfg(["ssim", "psnr", "jedi"]))
    with pytest.raises(NotImplementedError, match="psnr, ssim"):
        EvalMetrics(_cfg(["psnr", "jedi"], jedi_jepa_model="vit_large"))
    enc, probe = seeded_vjepa_state(1, 0), seeded_probe_state(1)
    m = EvalMetrics(_cfg(["jedi", "psnr"], jedi_jepa_model="vit_large"), jedi_weights=enc, jedi_probe=probe)
    assert m.names == ["jedi", "psnr"] and m._jedi is not None and m._jedi.finetuned
    assert len(m.state_dict()) == 0
    m2 = EvalMetrics(_cfg(["psnr", "jedi"], jedi_weights=enc, jedi_probe=probe))
    assert m2._jedi is not None
    with pytest.raises(NotImplementedError, match="vit_huge"):
        EvalMetrics(_cfg(["jedi"], jedi_jepa_model="vit_huge"), jedi_weights=enc, jedi_probe=probe)
    with pytest.raises(ValueError, match="jedi_probe"):
        EvalMetrics(_cfg(["jedi"]), jedi_weights=enc)
    assert math.isnan(m._jedi.compute())


@pytest.fixture(scope="module")
def handle():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


def test_cabi_structs_mirror_header():
    src = open(os.path.join(ROOT, "include", "titok_hip.h")).read()
    for struct, cls in [("ttv_vjepa_layer", _lib.VjepaLayer), ("ttv_vjepa_weights", _lib.VjepaWeights)]:
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                decl = re.sub(r"^(const\s+)?(struct\s+)?[A-Za-z_0-9]+\s*\*?\s*", "", decl, count=1)
                fields += [re.sub(r"[\*\s]|\[.*\]", "", part) for part in decl.split(",")]
        assert fields == [f[0] for f in cls._fields_], struct
    assert C.sizeof(_lib.VjepaLayer) == 12 * 8 and C.sizeof(_lib.VjepaWeights) == 16 + 20 * 8


def test_cabi_argument_checks(handle):
    err = lambda: handle.ttv_error_string().decode()
    p = C.c_void_p(256)
    assert handle.ttv_vjepa_workspace_bytes(0) == -1 and "clips" in err()
    assert handle.ttv_vjepa_workspace_bytes(65) == -1
    assert handle.ttv_vjepa_workspace_bytes(1) > 1568 * 1024 * 4
    ptrs = (C.c_void_p * 1)(256)
    assert handle.ttv_jedi_preprocess(ptrs, (C.c_int32 * 4)(3, 4, 64, 96), 1, _lib.TTV_BF16, p, None) == 1 and "square" in err()
    assert handle.ttv_jedi_preprocess(ptrs, (C.c_int32 * 4)(3, 17, 64, 64), 1, _lib.TTV_BF16, p, None) == 1 and "17 frames" in err()
    assert handle.ttv_jedi_preprocess(ptrs, (C.c_int32 * 4)(3, 4, 64, 64), 0, _lib.TTV_BF16, p, None) == 1
    w = _lib.VjepaWeights(width=1280, heads=16, depth=24)
    assert handle.ttv_vjepa_features(C.byref(w), p, 1, p, 1, p, 1 << 30, None) == 1 and "head_dim 80" in err()
    assert handle.ttv_vjepa_linear(p, 1024, p, 1024, p, 16, 1000, 1024, 0, None, 0, 0, p, 1024, None) == 1 and "multiple of 128" in err()
    assert handle.ttv_vjepa_linear(p, 1024, p, 1024, p, 16, 1024, 1024, 2, None, 0, 0, p, 1024, None) == 1 and "resid" in err()
    assert handle.ttv_vjepa_linear(p, 1024, p, 1024, p, 16, 1024, 1024, 7, None, 0, 0, p, 1024, None) == 1 and "epilogue" in err()
    assert handle.ttv_vjepa_layernorm(p, 768, 4, 768, p, p, 1e-6, None, None, 0.0, None, 0, p, 768, None) == 1 and "width" in err()
    assert handle.ttv_vjepa_pool_attention(p, p, 0, 1568, p, None) == 1 and "clips" in err()


# ---- the restatement against explicit loops at a small width ----------------------------------------------------------------

def _loop_ln(x, w, b, eps):
    out = torch.empty_like(x)
    for i in range(x.shape[0]):
        mu = sum(float(v) for v in x[i]) / x.shape[1]
        var = sum((float(v) - mu) ** 2 for v in x[i]) / x.shape[1]
        for j in range(x.shape[1]):
            out[i, j] = (float(x[i, j]) - mu) / math.sqrt(var + eps) * float(w[j]) + float(b[j])
    return out


def _loop_mha(q, k, v, heads):
    n, d = q.shape
    hd = d // heads
    out = torch.zeros(n, d, dtype=q.dtype)
    for h in range(heads):
        sl = slice(h * hd, (h + 1) * hd)
        for i in range(n):
            s = [float(q[i, sl] @ k[j, sl]) / math.sqrt(hd) for j in range(k.shape[0])]
            mx = max(s)
            e = [math.exp(t - mx) for t in s]
            tot = sum(e)
            for j in range(k.shape[0]):
                out[i, sl] += e[j] / tot * v[j, sl]
    return out


def _loop_gelu(x):
    return torch.tensor([[0.5 * float(v) * (1 + math.erf(float(v) / math.sqrt(2))) for v in r] for r in x], dtype=x.dtype)


def _rand(shape, key, g):
    if "norm" in key and key.endswith("weight"):
        return 1 + 0.1 * torch.randn(shape, generator=g, dtype=torch.float64)
    return torch.randn(shape, generator=g, dtype=torch.float64) * (shape[-1] ** -0.5 if len(shape) >= 2 else 0.3)


def test_restatement_matches_explicit_loops():
    g = torch.Generator().manual_seed(0)
    d, heads, depth, tokens = 16, 4, 2, 12
    rows = torch.randn(tokens, 3 * 2 * 16 * 16, generator=g, dtype=torch.float64)
    enc = {k: _rand(s, k, g) for k, s in J.encoder_shapes(depth, d).items()}
    enc["patch_embed.proj.weight"] *= 0.05
    enc["pos_embed"] = enc["pos_embed"][:, :tokens]
    probe = {k: _rand(s, k, g) for k, s in J.probe_shapes(d).items()}
    y = R.encoder(rows, enc, heads=heads, bf16=False)
    x = rows @ enc["patch_embed.proj.weight"].reshape(d, -1).T + enc["patch_embed.proj.bias"] + enc["pos_embed"][0]
    for i in range(depth):
        p = f"blocks.{i}."
        h = _loop_ln(x, enc[p + "norm1.weight"], enc[p + "norm1.bias"], 1e-6)
        qkv = h @ enc[p + "attn.qkv.weight"].T + enc[p + "attn.qkv.bias"]
        a = _loop_mha(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], heads)
        x = x + a @ enc[p + "attn.proj.weight"].T + enc[p + "attn.proj.bias"]
        h = _loop_ln(x, enc[p + "norm2.weight"], enc[p + "norm2.bias"], 1e-6)
        f = _loop_gelu(h @ enc[p + "mlp.fc1.weight"].T + enc[p + "mlp.fc1.bias"])
        x = x + f @ enc[p + "mlp.fc2.weight"].T + enc[p + "mlp.fc2.bias"]
    want = _loop_ln(x, enc["norm.weight"], enc["norm.bias"], 1e-6)
    assert torch.allclose(y, want, rtol=1e-10, atol=1e-10)
    c = "pooler.cross_attention_block."
    qt = probe["pooler.query_tokens"].reshape(1, d)
    h = _loop_ln(want, probe[c + "norm1.weight"], probe[c + "norm1.bias"], 1e-5)
    q = qt @ probe[c + "xattn.q.weight"].T + probe[c + "xattn.q.bias"]
    kv = h @ probe[c + "xattn.kv.weight"].T + probe[c + "xattn.kv.bias"]
    z = qt + _loop_mha(q, kv[:, :d], kv[:, d:], heads) @ probe[c + "xattn.proj.weight"].T + probe[c + "xattn.proj.bias"]
    f = _loop_ln(z, probe[c + "norm2.weight"], probe[c + "norm2.bias"], 1e-5) @ probe[c + "mlp.fc1.weight"].T + probe[c + "mlp.fc1.bias"]
    z = z + _loop_gelu(f) @ probe[c + "mlp.fc2.weight"].T + probe[c + "mlp.fc2.bias"]
    assert torch.allclose(R.pooler(y, probe, heads=heads, bf16=False), z[0], rtol=1e-10, atol=1e-10)


def test_restated_preprocess_and_patch_order():
    g = torch.Generator().manual_seed(4)
    clip = torch.rand(3, 5, 40, 40, generator=g) * 2.6 - 1.3
    v = R.preprocess(clip)
    assert v.shape == (3, 16, 224, 224)
    assert torch.equal(v[:, 5:], v[:, 4:5].expand(-1, 11, -1, -1))            # the last frame repeated
    x = (clip.clamp(-1, 1) + 1) / 2
    up = F.interpolate(x.permute(1, 0, 2, 3), size=(224, 224), mode="bicubic", align_corners=False)
    mean = torch.tensor(R.MEAN)[None, :, None, None]
    std = torch.tensor(R.STD)[None, :, None, None]
    assert torch.equal(v[:, :5], ((up - mean) / std).permute(1, 0, 2, 3))
    rows = R.patch_rows(v)
    assert rows.shape == (1568, 1536)
    # token (t, h, w) = (3, 5, 7), column (c, kt, kh, kw) = (2, 1, 9, 4) is pixel (c, 2 t + kt, 16 h + kh, 16 w + kw)
    assert rows[(3 * 14 + 5) * 14 + 7, ((2 * 2 + 1) * 16 + 9) * 16 + 4] == v[2, 7, 89, 116]
    # and the rows times the flattened Conv3d weight are the Conv3d (kernel = stride = (2, 16, 16)) in (t, h, w) token order
    w = torch.randn(8, 3, 2, 16, 16, generator=g, dtype=torch.float64)
    conv = F.conv3d(v[None].double(), w, stride=(2, 16, 16))[0].reshape(8, -1).T
    assert torch.allclose(rows.double() @ w.reshape(8, -1).T, conv, rtol=1e-10, atol=1e-9)
