"""Float64 replay of the bf16 training tape (CPU, no GPU; imported by tests/test_hip_backward_bf16.py, pinned by
tests/test_bf16_tape_cpu.py).

The bf16 training step (csrc/ttv_train.hip) stores its forward tape and its activation gradients in bf16 and accumulates in fp32.
Compared with a float64 autograd of the model, its gradients legitimately differ by that rounding, compounded through the KEEL layers -
which is why the per-tower bf16 checks could only ask for a cosine of 0.97.  This module restates the encoder and the decoder in float64
autograd and rounds to bf16 at exactly the points where the HIP path stores bf16, so that what remains between the two is the kernels'
own arithmetic (fp32 summation order, the attention backward's internal bf16 P / dS, the fast GELU forms, the final bf16 gradient):

  * F(x): rounded to bf16 going forward, the gradient passes straight through - a tape value the backward reads;
  * B(x): identity going forward, the incoming gradient rounded to bf16 - a gradient buffer the backward keeps in bf16.

Every other value (the residual-stream gradient, the norm-gain and bias sums, z, dz, the decoder's d(hpre)) is fp32 on the HIP side and
float64 here.  Each F / B cites the ttv_train.hip line (or the kernel) that stores the value.  Attention and its backward run in float64
per (sequence, kv-head) like tests/blockwise.attention_reference; GELU is exact erf; RMSNorm and the rotary embedding are the oracle's
definitions in float64 (the oracle's own rmsnorm / apply_rotary / attention_varlen compute in fp32 whatever their inputs).

The encoder's last layer runs on the latent rows only on the HIP side (latent_tail); that is the same function (the loss does not read
the patch rows of its output), so the replay runs it on every row."""
import torch
import torch.nn.functional as F

from oracle import titok_oracle as O

BF16 = torch.bfloat16


class _Fwd(torch.autograd.Function):
    """F: bf16 value forward, straight-through gradient."""
    @staticmethod
    def forward(ctx, x):
        return x.to(BF16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


class _Bwd(torch.autograd.Function):
    """B: identity forward, bf16-rounded gradient."""
    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return g.to(BF16).to(g.dtype)


class Rounding:
    """Where the replay rounds.  on=False: a plain float64 autograd of the model (no rounding anywhere).  y_bf16=False: the KEEL sums
    y1 / y2 stay unrounded (TTV_TAPE_Y_F32=1 or TTV_TRAIN_FUSED_NORMS=1, ttv_train.hip:30-33).  `record`: a dict that receives the
    forward value of every named F point (for the CPU tests)."""

    def __init__(self, on: bool = True, y_bf16: bool = True, record=None):
        self.on, self.y_bf16, self.record = on, on and y_bf16, record

    def F(self, x, name=None):
        out = _Fwd.apply(x) if self.on else x
        if self.record is not None and name:
            self.record[name] = out.detach()
        return out

    def B(self, x):
        return _Bwd.apply(x) if self.on else x

    def FB(self, x, name=None):
        return self.B(self.F(x, name))


def rmsnorm64(x, w, eps: float = O.RMS_EPS):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w


def rotate64(x, cos, sin):
    """O.apply_rotary in float64: x [L, H, D]; the first cos.shape[-1] (x[2j], x[2j+1]) pairs of each head rotated."""
    pairs = x.unflatten(-1, (-1, 2))
    R = cos.shape[-1]
    re, im = pairs[..., :R, 0], pairs[..., :R, 1]
    c, s = cos.unsqueeze(1), sin.unsqueeze(1)
    rot = torch.stack((re * c - im * s, re * s + im * c), -1)
    return torch.cat((rot, pairs[..., R:, :]), -2).flatten(-2)


class _Attention64(torch.autograd.Function):
    """Non-causal per-sequence softmax(q k^T / 8) v with GQA on [L, H, 64] float64 operands.  The backward is FlashAttention-2's, per
    (sequence, kv-head) so that a 5-clip batch of 1152-row sequences stays at a few 10 MB: dS = P * (dP - delta) with delta = rowsum(dO * O)
    taken from the output as the tape stores it (`tape_bf16`: rounded to bf16 - the HIP backward reads the stored a, ttv_bwd.hip
    k_gate_bwd; the exact output otherwise, which makes this the exact gradient)."""

    @staticmethod
    def forward(ctx, q, k, v, cu, tape_bf16=False):
        hq, hkv = q.shape[1], k.shape[1]
        rep = hq // hkv
        out = torch.zeros_like(q)
        for b in range(len(cu) - 1):
            s, e = int(cu[b]), int(cu[b + 1])
            for h in range(hkv):
                p = torch.softmax(q[s:e, h * rep:(h + 1) * rep].transpose(0, 1) @ k[s:e, h].T * 0.125, -1)
                out[s:e, h * rep:(h + 1) * rep] = (p @ v[s:e, h]).transpose(0, 1)
        o_tape = out.to(BF16).to(out.dtype) if tape_bf16 else out
        ctx.save_for_backward(q, k, v, o_tape)
        ctx.cu = cu
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, o = ctx.saved_tensors
        hq, hkv = q.shape[1], k.shape[1]
        rep = hq // hkv
        dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
        delta = (dout * o).sum(-1)                                      # [L, hq]
        for b in range(len(ctx.cu) - 1):
            s, e = int(ctx.cu[b]), int(ctx.cu[b + 1])
            for h in range(hkv):
                hs = slice(h * rep, (h + 1) * rep)
                qq, kk, vv = q[s:e, hs].transpose(0, 1), k[s:e, h], v[s:e, h]          # [rep, n, 64], [n, 64]
                do = dout[s:e, hs].transpose(0, 1)
                p = torch.softmax(qq @ kk.T * 0.125, -1)                                # [rep, n, n]
                ds = p * (do @ vv.T - delta[s:e, hs].T.unsqueeze(-1))
                dq[s:e, hs] = (ds @ kk * 0.125).transpose(0, 1)
                dk[s:e, h] = (ds.transpose(1, 2) @ qq * 0.125).sum(0)
                dv[s:e, h] = (p.transpose(1, 2) @ do).sum(0)
        return dq, dk, dv, None, None


def layers_replay(x, p, prefix, layers, heads, cos, sin, cu, r: Rounding):
    """layers_forward_train (ttv_train.hip:139-237) on X[0] -> X[layers]; the backward's bf16 buffers from layers_backward (:291-409)."""
    hq, hkv = heads
    d = x.shape[1]
    g = hkv * 64
    alpha = 2 * layers
    for i in range(layers):
        ap, fp = f"{prefix}attn_layer.{i}.", f"{prefix}ffd_layer.{i}."
        t = f"l{i}."
        xn1 = r.FB(rmsnorm64(x, p[ap + "pre_ln.weight"]), t + "xn1")             # F :158 xn1 ; B :377 dxn1 (g_d2)
        qkv = r.B(xn1 @ p[ap + "to_qkv.weight"].T)                               # B :370-374 dq / dk / dv (un-rotated) and dgate (g_nq)
        q, gate, k, v = qkv.split([d, d, g, g], -1)
        q = rotate64(q.unflatten(-1, (hq, 64)), cos, sin)                        # EPI_QKV_ROPE: rotary on the fp32 accumulator (:160-162)
        k = rotate64(k.unflatten(-1, (hkv, 64)), cos, sin)
        qkvg = r.F(torch.cat((q.flatten(-2), gate, k.flatten(-2), v), -1), t + "qkvg")   # F :162 qkvg
        q, gate, k, v = qkvg.split([d, d, g, g], -1)
        a = _Attention64.apply(q.unflatten(-1, (hq, 64)), k.unflatten(-1, (hkv, 64)), v.unflatten(-1, (hkv, 64)), cu, r.on)
        a = r.FB(a.flatten(-2), t + "a")                                         # F :172 a (also delta's O) ; B :370 da (gate backward)
        ag = r.FB(a * torch.sigmoid(gate), t + "ag")                             # F :172 ag from the rounded a ; B :355 dag (g_d2)
        o = r.B(ag @ p[ap + "out_proj.weight"].T)                                # B :350-352 do (g_do)
        if i == 0:
            x1 = r.F(x + o, t + "x1")                                            # F :190-192 x1 = X0 + ag Wo^T
        else:
            y1 = alpha * x + o
            if r.y_bf16:
                y1 = r.F(y1, t + "y1")                                           # F :198 y1 (tape_y_dtype)
            x1 = r.F(rmsnorm64(y1, p[f"{prefix}attn_post_ln.{i - 1}.weight"]), t + "x1")   # F :199 x1
        xn2 = r.FB(rmsnorm64(x1, p[fp + "norm.weight"]), t + "xn2")              # F :202 xn2 ; B :345 dxn2 (g_d2)
        u = r.FB(xn2 @ p[fp + "w12.weight"].T, t + "u")                          # F :205-207 u (EPI_GEGLU resid) ; B :342 du (g_2i)
        ux, ug = u.chunk(2, -1)
        h = r.FB(F.gelu(ug) * ux, t + "h")                                       # F :205-207 h from the stored u ; B :340 dh (g_i)
        f = r.B(h @ p[fp + "w3.weight"].T)                                       # B :332 / :394-396 df (the w3 product only)
        if i == 0:
            x = r.F(x1 + f, t + "X")                                             # F :214-216 X[1]
        else:
            y2 = alpha * x1 + f
            if r.y_bf16:
                y2 = r.F(y2, t + "y2")                                           # F :226 y2 (tape_y_dtype)
            x = r.F(rmsnorm64(y2, p[f"{prefix}ffd_post_ln.{i - 1}.weight"]), t + "X")   # F :227 X[i + 1]
    return x


def _rows(mask, latent, patch):
    """The packed [L, d] rows from the latent and the patch rows (latent first in every clip: O.batch_metadata)."""
    lat, pat = mask.nonzero().squeeze(1), (~mask).nonzero().squeeze(1)
    x = torch.zeros(mask.shape[0], latent.shape[1], dtype=latent.dtype)
    return x.index_put((lat,), latent).index_put((pat,), patch)


def encoder_replay(clips, counts, p, size="tiny", patch=(4, 8, 8), r: Rounding = None, prefix="encoder."):
    """z [sum(K), C] of O.encoder_forward with the bf16 tape's rounding (ttv_encoder_forward_train / ttv_encoder_backward)."""
    r = r or Rounding()
    width, layers, heads = O.model_dims(size)
    grids, sizes, counts, cu, mask = O.batch_metadata([c.shape[1:] for c in clips], counts, patch)
    cos, sin = O.rope_table(grids, counts, width // heads[0])
    mt = p[prefix + "mask_token"]
    patches = torch.cat([O.patchify(c, patch) for c in clips], 0)
    lin = r.F(patches @ p[prefix + "proj_in.weight"].T + p[prefix + "proj_in.bias"])   # Linear output rounded before + mask_token
    pe = r.FB(lin + mt, "pe")                                    # (ttv_gemm.hip epilogue) ; F :442-444 pe ; B :489 dpe (g_d)
    xt = rmsnorm64(mt.expand(-1, width), p[prefix + "ln_pre_t.weight"]).expand(int(mask.sum()), width)   # :446 constant latent rows
    xp = rmsnorm64(pe, p[prefix + "ln_pre_p.weight"])            # :445
    x = r.F(_rows(mask, xt, xp), "X0")                           # F X[0]
    x = layers_replay(x, p, prefix + "model_layers.", layers, heads, cos, sin, cu, r)
    n = r.FB(rmsnorm64(x[mask], p[prefix + "ln_post.weight"]), "n")   # F :448 / :476 n ; B :479 dn (g_d2)
    return n @ p[prefix + "proj_out.weight"].T + p[prefix + "proj_out.bias"]   # z: fp32 (:448), dz fp32


def decoder_replay(codes, counts, pixel_grids, p, size="tiny", patch=(4, 8, 8), r: Rounding = None, prefix="decoder.", out_channels=3):
    """Clips of O.decoder_forward with the bf16 tape's rounding (ttv_decoder_forward_train / ttv_decoder_backward)."""
    r = r or Rounding()
    width, layers, heads = O.model_dims(size)
    grids, sizes, counts, cu, mask = O.batch_metadata(pixel_grids, counts, patch)
    cos, sin = O.rope_table(grids, counts, width // heads[0])
    mt = p[prefix + "mask_token"]
    lin = r.F(codes @ p[prefix + "proj_in.weight"].T + p[prefix + "proj_in.bias"])   # k_dec_embed: Linear output rounded, then
    hpre = r.F(lin + mt, "hpre")                                 # + mask_token rounded: F :514 hpre ; d(hpre) fp32 (:552 small_f32)
    xt = rmsnorm64(hpre, p[prefix + "ln_pre_t.weight"])
    xp = rmsnorm64(mt.expand(-1, width), p[prefix + "ln_pre_p.weight"]).expand(int((~mask).sum()), width)   # :515 constant patch rows
    x = r.F(_rows(mask, xt, xp), "X0")                           # F X[0]
    x = layers_replay(x, p, prefix + "model_layers.", layers, heads, cos, sin, cu, r)
    pn = r.FB(rmsnorm64(x[~mask], p[prefix + "ln_post.weight"]), "pn")   # F :517 pn ; B :543 dpn (g_d2)
    out = r.FB(pn @ p[prefix + "proj_out.weight"].T + p[prefix + "proj_out.bias"], "recon")   # F :518-521 clips ; B: dclips arrive in bf16
    return [O.unpatchify(c, g, patch, out_channels) for c, g in zip(torch.split(out, sizes, 0), grids)]


def _leaves(params, prefix):
    return {k: v.detach().double().clone().requires_grad_(True) for k, v in params.items() if k.startswith(prefix)}


def encoder_grads(params, clips, counts, wz, size="tiny", rounding=True, y_bf16=True, record=None):
    """float64 gradients of the linear loss sum(wz * z) w.r.t. every `encoder.*` parameter and the clips (dict, list)."""
    p = _leaves(params, "encoder.")
    cl = [c.detach().double().clone().requires_grad_(True) for c in clips]
    z = encoder_replay(cl, list(counts), p, size, r=Rounding(rounding, y_bf16, record))
    (z * wz.double()).sum().backward()
    return {k: v.grad for k, v in p.items()}, [c.grad for c in cl]


def decoder_grads(params, codes, counts, shapes, w, size="tiny", rounding=True, y_bf16=True, record=None):
    """float64 gradients of the linear loss sum_c sum(w_c * recon_c) w.r.t. every `decoder.*` parameter and the codes (dict, tensor)."""
    p = _leaves(params, "decoder.")
    cd = codes.detach().double().clone().requires_grad_(True)
    recon = decoder_replay(cd, list(counts), [tuple(s) for s in shapes], p, size, r=Rounding(rounding, y_bf16, record))
    sum((c * wc.double()).sum() for c, wc in zip(recon, w)).backward()
    return {k: v.grad for k, v in p.items()}, cd.grad


def global_distance(got, ref) -> float:
    """||got - ref|| / ||ref|| over all entries of two gradient dicts together."""
    num = sum(float((got[k].double() - ref[k].double()).pow(2).sum()) for k in ref)
    den = sum(float(ref[k].double().pow(2).sum()) for k in ref)
    return (num / den) ** 0.5
