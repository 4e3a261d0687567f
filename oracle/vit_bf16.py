"""Rounding-matched twin of the HIP ViT plan (daliid_amd/csrc/vit_plan.hip): the forward and an EXPLICIT backward of one transformer
block, of the head (final LayerNorm on the cls rows) and of the token tail, in fp32 on the CPU, rounding to bf16 where the kernels store bf16.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  With ``rounding=False`` the backward is plain calculus and equals autograd through
oracle/vit.py to fp32 roundoff (tests/test_vit_twin_cpu.py); with ``rounding=True`` it follows the plan's launch sequence:

  forward   patches, pe, x0, h1, qkv, att, x_mid, h2, pre1, act1, x_out stored in bf16; LayerNorm mean / rstd and the attention lse in fp32;
            weights as P.to(bf16); the attention probabilities normalised in fp32, rounded to bf16 for P V;
            x_mid = x + s * (acc + bias), x_out = x_mid + s * (acc + bias), one rounding each.
  backward  t1, t2, t3 and dx stored in bf16; GELU' taken at the stored bf16 pre1; P recomputed from the stored lse, rounded to bf16 for dV;
            dS = P (dP - D) scale rounded to bf16, D = rowsum(dO o) on the stored o; the DropPath copy s * d rounded to bf16 (only when the
            plan runs with DropPath factors); weight, bias and LayerNorm gradients summed in fp32 from those stored values.

Every function consumes STORED tensors (a dict of fp32 tensors holding the plan's own values, or this file's forward), so a test can hand it
the plan's own forward tensors and incoming gradient: errors do not chain from block to block.

``defect`` switches in ONE deliberate wiring mistake, for the sensitivity table of tests/test_vit_twin_cpu.py:
  "bias_rows"   the four linears' bias gradients omit the last 4 token rows
  "ln1_x_mid"   LN1's backward reads x_mid instead of x_in
  "ln2_rstd"    LN2's backward uses n1's saved rstd
  "pos_token0"  the pos_embed gradient omits token 0
(factors taken from the neighbouring block, or exchanged between the two branches, are mistakes of the CALLER: it passes other factors.)
"""
import math

import torch
import torch.nn.functional as F

bf16 = torch.bfloat16
LN_EPS = 1e-6
BLOCK_PARAMS = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
                "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")


def _q(rounding):
    return (lambda t: t.to(bf16).float()) if rounding else (lambda t: t)


def _rows(s, T):
    """per-sample factors [B] -> per-row column [B*T, 1]; None stays None"""
    return None if s is None else s.float().repeat_interleave(T).unsqueeze(1)


def _heads(t, B, T, H, part, n_parts):
    """[B*T, n_parts*C] -> [B, H, T, 64] of one part (vit_pytorch.py:155 layout)"""
    return t.reshape(B, T, n_parts, H, -1)[:, :, part].permute(0, 2, 1, 3)


def _unheads(t):
    """[B, H, T, 64] -> [B*T, C]"""
    B, H, T, D = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * T, H * D)


def _ln_fwd(x, gamma, beta, Q):
    mean = x.mean(1)
    rstd = 1.0 / torch.sqrt(((x - mean[:, None]) ** 2).mean(1) + LN_EPS)
    return Q((x - mean[:, None]) * rstd[:, None] * gamma + beta), mean, rstd


def _ln_bwd(g, x, gamma, mean, rstd, add, Q):
    """layernorm_bwd_kernel: dgamma = sum g xhat, dbeta = sum g (fp32); dx = rstd (g gamma - mean_c - xhat mean_c(g gamma xhat)) + add, stored once"""
    xh = (x - mean[:, None]) * rstd[:, None]
    dgamma, dbeta = (g * xh).sum(0), g.sum(0)
    gh = g * gamma
    s1, s2 = gh.mean(1, keepdim=True), (gh * xh).mean(1, keepdim=True)
    o = rstd[:, None] * (gh - s1 - xh * s2)
    if add is not None:
        o = o + add
    return Q(o), dgamma, dbeta


def _gelu_grad(v):
    return 0.5 * torch.erfc(-v / math.sqrt(2.0)) + v * torch.exp(-0.5 * v * v) / math.sqrt(2 * math.pi)


def forward_block(x_in, p, heads, B, s_att=None, s_mlp=None, rounding=True):
    """one block of the plan's forward (run_block) on x_in [B*T, C] -> dict of its stored tensors (x_out among them)"""
    Q = _q(rounding)
    W = lambda k: Q(p[k])
    rows, C = x_in.shape
    T = rows // B
    t = {"x_in": x_in}
    t["h1"], t["n1.mean"], t["n1.rstd"] = _ln_fwd(x_in, p["norm1.weight"], p["norm1.bias"], Q)
    t["qkv"] = Q(t["h1"] @ W("attn.qkv.weight").t() + p["attn.qkv.bias"])
    q, k, v = (_heads(t["qkv"], B, T, heads, i, 3) for i in range(3))
    S = 0.125 * (q @ k.transpose(-1, -2))
    t["lse"] = torch.logsumexp(S, -1)                                           # [B, H, T]
    t["att"] = Q(_unheads(Q(torch.exp(S - t["lse"][..., None])) @ v))
    ra, rm = _rows(s_att, T), _rows(s_mlp, T)
    br = t["att"] @ W("attn.proj.weight").t() + p["attn.proj.bias"]
    t["x_mid"] = Q(x_in + (br if ra is None else br * ra))
    t["h2"], t["n2.mean"], t["n2.rstd"] = _ln_fwd(t["x_mid"], p["norm2.weight"], p["norm2.bias"], Q)
    pre = t["h2"] @ W("mlp.fc1.weight").t() + p["mlp.fc1.bias"]
    t["pre1"], t["act1"] = Q(pre), Q(F.gelu(pre))
    br = t["act1"] @ W("mlp.fc2.weight").t() + p["mlp.fc2.bias"]
    t["x_out"] = Q(t["x_mid"] + (br if rm is None else br * rm))
    return t


def attention_backward(qkv, o, d_o, lse, B, T, heads, Q):
    """attention_bwd_dq / _dkv kernels: qkv [B*T, 3C], o and d_o [B*T, C], lse [B, H, T] -> d_qkv [B*T, 3C]"""
    q, k, v = (_heads(qkv, B, T, heads, i, 3) for i in range(3))
    dO, oh = _heads(d_o, B, T, heads, 0, 1), _heads(o, B, T, heads, 0, 1)
    P = torch.exp(0.125 * (q @ k.transpose(-1, -2)) - lse[..., None])
    D = (dO * oh).sum(-1, keepdim=True)
    dS = Q(P * (dO @ v.transpose(-1, -2) - D) * 0.125)
    dq, dk, dv = dS @ k, dS.transpose(-1, -2) @ q, Q(P).transpose(-1, -2) @ dO
    return Q(torch.stack([_unheads(dq), _unheads(dk), _unheads(dv)], 1).reshape(B * T, -1))


def backward_block(t, p, d_out, heads, B, s_att=None, s_mlp=None, rounding=True, defect=None):
    """One block of the plan's backward from its stored forward tensors t, its parameters p and the incoming gradient d_out [B*T, C] (= d x_out).
    s_att / s_mlp [B]: the DropPath factors the backward applies (None: the plan ran without DropPath and makes no scaled copy).
    -> (d x_in, {name: gradient} of the 12 parameters)"""
    Q = _q(rounding)
    W = lambda k: Q(p[k])
    rows = d_out.shape[0]
    T = rows // B
    keep = rows - 4 if defect == "bias_rows" else rows
    g = {}

    def lin(name, x, dy):
        g[name + ".weight"], g[name + ".bias"] = dy.t() @ x, dy[:keep].sum(0)
        return dy @ W(name + ".weight")

    # x_out = x_mid + s_mlp * fc2(gelu(fc1(LN2(x_mid))))
    d_br = d_out if s_mlp is None else Q(_rows(s_mlp, T) * d_out)
    t1 = Q(lin("mlp.fc2", t["act1"], d_br) * _gelu_grad(t["pre1"]))                                  # d_pre1
    t2 = Q(lin("mlp.fc1", t["h2"], t1))                                                              # d_h2
    rstd2 = t["n1.rstd"] if defect == "ln2_rstd" else t["n2.rstd"]
    t3, g["norm2.weight"], g["norm2.bias"] = _ln_bwd(t2, t["x_mid"], p["norm2.weight"], t["n2.mean"], rstd2, d_out, Q)      # d_x_mid
    # x_mid = x_in + s_att * proj(attn(qkv(LN1(x_in))))
    d_br = t3 if s_att is None else Q(_rows(s_att, T) * t3)
    t1 = Q(lin("attn.proj", t["att"], d_br))                                                         # d_att
    t2 = attention_backward(t["qkv"], t["att"], t1, t["lse"], B, T, heads, Q)                        # d_qkv
    t1 = Q(lin("attn.qkv", t["h1"], t2))                                                             # d_h1
    x1 = t["x_mid"] if defect == "ln1_x_mid" else t["x_in"]
    dx, g["norm1.weight"], g["norm1.bias"] = _ln_bwd(t1, x1, p["norm1.weight"], t["n1.mean"], t["n1.rstd"], t3, Q)
    return dx, g


def forward_tokens(images, sd, patch, stride, rounding=True):
    """patchify, the patch embedding and assemble_tokens -> dict(patches [B*np, 3 ps ps], pe [B*np, C], x0 [B*T, C])"""
    Q = _q(rounding)
    B = images.shape[0]
    patches = Q(F.unfold(images, patch, stride=stride).transpose(1, 2).reshape(-1, 3 * patch * patch))
    wp = sd["base.patch_embed.proj.weight"]
    C = wp.shape[0]
    pe = Q(patches @ Q(wp.reshape(C, -1)).t() + sd["base.patch_embed.proj.bias"])
    x0 = Q(torch.cat((sd["base.cls_token"].reshape(1, 1, C).expand(B, 1, C), pe.reshape(B, -1, C)), 1) + sd["base.pos_embed"].reshape(1, -1, C))
    return {"patches": patches, "pe": pe, "x0": x0.reshape(-1, C)}


def backward_tokens(d_x0, patches, B, patch, defect=None):
    """the token tail from d_x0 [B*T, C] (stored bf16 values): pos_embed / cls_token gradients are sums over the samples in ascending order,
    the patch rows are copied, and their weight / bias gradients are fp32 sums -> {name: gradient}"""
    C = d_x0.shape[1]
    d = d_x0.reshape(B, -1, C)
    dpos = torch.zeros(d.shape[1], C)
    for b in range(B):
        dpos = dpos + d[b]
    dpe = d[:, 1:].reshape(-1, C)
    g = {"base.cls_token": dpos[0].clone().reshape(1, 1, C), "base.pos_embed": dpos.reshape(1, -1, C),
         "base.patch_embed.proj.weight": (dpe.t() @ patches).reshape(C, 3, patch, patch), "base.patch_embed.proj.bias": dpe.sum(0)}
    if defect == "pos_token0":
        g["base.pos_embed"] = g["base.pos_embed"].clone()
        g["base.pos_embed"][0, 0] = 0
    return g


def forward_head(x_last, sd, B):
    """cls rows of the last block's output and the final LayerNorm on them (fp32 output, the plan's y32 path)"""
    C = x_last.shape[1]
    cls_rows = x_last.reshape(B, -1, C)[:, 0]
    gf, mean, rstd = _ln_fwd(cls_rows, sd["base.norm.weight"], sd["base.norm.bias"], lambda v: v)
    return {"cls_rows": cls_rows, "gf": gf, "fin.mean": mean, "fin.rstd": rstd}


def backward_head(d_gf, h, sd, B, T, rounding=True):
    """final LayerNorm backward from the fp32 gradient of gf (the plan's g32 path), scattered to token 0 of a zero token gradient"""
    Q = _q(rounding)
    dcls, dg, db = _ln_bwd(d_gf, h["cls_rows"], sd["base.norm.weight"], h["fin.mean"], h["fin.rstd"], None, Q)
    d = torch.zeros(B, T, dcls.shape[1])
    d[:, 0] = dcls
    return d.reshape(B * T, -1), {"base.norm.weight": dg, "base.norm.bias": db}


def block_params(sd, i):
    return {k: sd["base.blocks.%d.%s" % (i, k)] for k in BLOCK_PARAMS}


def forward_backward(sd, images, d_gf, heads, patch, stride, scales=None, rounding=True, defect=None, bwd_scales=None):
    """The whole chain on the CPU: forward to the cls feature gf (before the neck), backward from d_gf -> (gf, {name: gradient}, [d x_in per block]).
    scales [2*depth, B] or None; bwd_scales: what the backward applies instead (a caller's wiring mistake); defect = (kind, block or None)."""
    B = images.shape[0]
    depth = 0
    while "base.blocks.%d.norm1.weight" % depth in sd:
        depth += 1
    tok = forward_tokens(images, sd, patch, stride, rounding)
    T = tok["x0"].shape[0] // B
    x, ts = tok["x0"], []
    sc = lambda s, j: None if s is None else s[j]
    for i in range(depth):
        ts.append(forward_block(x, block_params(sd, i), heads, B, sc(scales, 2 * i), sc(scales, 2 * i + 1), rounding))
        x = ts[-1]["x_out"]
    h = forward_head(x, sd, B)
    d, grads = backward_head(d_gf, h, sd, B, T, rounding)
    bs = scales if bwd_scales is None else bwd_scales
    kind, where = defect if defect else (None, None)
    dxs = [None] * depth
    for i in range(depth - 1, -1, -1):
        d, g = backward_block(ts[i], block_params(sd, i), d, heads, B, sc(bs, 2 * i), sc(bs, 2 * i + 1), rounding, kind if where == i else None)
        dxs[i] = d
        grads.update({"base.blocks.%d.%s" % (i, k): v for k, v in g.items()})
    grads.update(backward_tokens(d, tok["patches"], B, patch, kind if where is None else None))
    return h["gf"], grads, dxs
