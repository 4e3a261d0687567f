"""A short fp32 torch restatement of ``build_transformer.forward`` (make_models.py:184-205) over ``TransReID.forward_features``
(vit_pytorch.py:375-408) with the two options of ``Attention`` that the small backbones use (vit_pytorch.py:139-164): ``qkv_bias=False`` (no
``attn.qkv.bias`` in the state dict) and ``qk_scale`` (the scale that replaces ``head_dim ** -0.5``).  For the tests only, written from reading
vit_pytorch.py:139-185 and :375-408 in this project's own words; tests/test_vit_small_cpu.py pins it to the reference's own outputs
(tests/golden/vit_small.npz).  Differentiable, so it also serves as the training reference for a bias-less qkv at head_dim 64.

  * forward        the post-neck feature (and the pre-neck cls feature) of build_transformer
  * seeded_state   the per-key seeded weights tests/golden/make_vit_small_golden.py loads into the reference's models
  * FACTORY_PARAMS the two small factories' parameter lists (names and defaults), restated as data from vit_pytorch.py:461 and :470
"""
import torch
import torch.nn.functional as F

# (name, default) in the reference's order; both factories end in **kwargs
FACTORY_PARAMS = {
    "vit_small_patch16_224_TransReID": (("img_size", (256, 128)), ("stride_size", 16), ("drop_rate", 0.0), ("attn_drop_rate", 0.0),
                                        ("drop_path_rate", 0.1), ("camera", 0), ("view", 0), ("local_feature", False), ("sie_xishu", 1.5)),
    "deit_small_patch16_224_TransReID": (("img_size", (256, 128)), ("stride_size", 16), ("drop_path_rate", 0.1), ("drop_rate", 0.0),
                                         ("attn_drop_rate", 0.0), ("camera", 0), ("view", 0), ("local_feature", False), ("sie_xishu", 1.5)),
}
TRANSFORMER_TYPES = ("vit_base_patch16_224_TransReID", "deit_base_patch16_224_TransReID", "vit_small_patch16_224_TransReID",
                     "deit_small_patch16_224_TransReID")             # make_models.py:392-397


def block(sd, p, t, num_heads, qk_scale=None, eps=1e-6):
    """vit_pytorch.py:166-184 with Attention (:139-164): pre-LN residual block; ``attn.qkv.bias`` is used if the state dict has one"""
    B, N, dim = t.shape
    hd = dim // num_heads
    scale = qk_scale or hd ** -0.5                                  # :145
    h = F.layer_norm(t, (dim,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
    qkv = F.linear(h, sd[p + "attn.qkv.weight"], sd.get(p + "attn.qkv.bias")).reshape(B, N, 3, num_heads, hd).permute(2, 0, 3, 1, 4)
    attn = ((qkv[0] @ qkv[1].transpose(-2, -1)) * scale).softmax(dim=-1)
    h = (attn @ qkv[2]).transpose(1, 2).reshape(B, N, dim)
    t = t + F.linear(h, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
    h = F.layer_norm(t, (dim,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
    return t + F.linear(F.gelu(F.linear(h, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])), sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])


def forward(sd, x, num_heads, stride, qk_scale=None, training=False, bn_eps=1e-5):
    """-> (feat, global_feat): the BatchNorm1d neck's output and the cls feature after the final LayerNorm.  ``training``: the neck uses the
    batch's statistics (biased variance), as nn.BatchNorm1d does in train mode; the running statistics are not updated here."""
    g = lambda k: sd["base." + k]
    t = F.conv2d(x, g("patch_embed.proj.weight"), g("patch_embed.proj.bias"), stride=stride).flatten(2).transpose(1, 2)
    t = torch.cat((g("cls_token").expand(x.shape[0], -1, -1), t), dim=1) + g("pos_embed")
    depth = 0
    while "base.blocks.%d.norm1.weight" % depth in sd:
        t = block(sd, "base.blocks.%d." % depth, t, num_heads, qk_scale)
        depth += 1
    gf = F.layer_norm(t[:, 0], (t.shape[-1],), g("norm.weight"), g("norm.bias"), 1e-6)
    if training:
        mean, var = gf.mean(0), gf.var(0, unbiased=False)
    else:
        mean, var = sd["bottleneck.running_mean"], sd["bottleneck.running_var"]
    return (gf - mean) * torch.rsqrt(var + bn_eps) * sd["bottleneck.weight"] + sd["bottleneck.bias"], gf


def _is_norm_weight(k):
    return (k.endswith(("norm1.weight", "norm2.weight", "norm.weight")) or k in ("b1.1.weight", "b2.1.weight")
            or (k.startswith("bottleneck") and k.endswith(".weight")))


def parse_shape(s):
    return tuple(int(v) for v in s.strip("()").split(",") if v.strip())


def seeded_state(keys, shapes, qkv_std=0.02):
    """key i gets a generator seeded 1000 + i (make_vit_long_golden.gen_vit_state's recipe, the JPM norms and necks counted as norms);
    ``attn.qkv.weight`` at std ``qkv_std``: at 0.02 the attention is nearly uniform and a wrong scale hides"""
    sd = {}
    for i, (k, shp) in enumerate(zip(keys, shapes)):
        shape = parse_shape(shp) if isinstance(shp, str) else tuple(shp)
        gg = torch.Generator().manual_seed(1000 + i)
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.zeros((), dtype=torch.long)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(shape, generator=gg)
        elif _is_norm_weight(k):
            sd[k] = 1.0 + 0.1 * torch.randn(shape, generator=gg)
        else:
            sd[k] = (qkv_std if k.endswith("attn.qkv.weight") else 0.02) * torch.randn(shape, generator=gg)
    return sd


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp(min=1e-30))
