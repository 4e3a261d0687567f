"""Plain torch restatements (fp32 CPU) of what the JPM / SIE additions compute, for the tests only, written from the reference's line
numbers in this project's own words (as oracle/vit.py is; no reference text is copied):

  * token_map        shuffle_unit (make_models.py:8-25) + the four consecutive runs (make_models.py:323-349), on token indices
  * sie_index        which sie_embed row a sample uses (vit_pytorch.py:382-389)
  * tokens           patch embedding + cls + pos_embed + sie_xishu * sie_embed[index] (vit_pytorch.py:375-391)
  * block            pre-LN residual block (vit_pytorch.py:139-184)
  * local_features   forward_features with local_feature=True: blocks[:-1], no final norm (vit_pytorch.py:393-396)
  * jpm_head         the five necks and the concatenation (make_models.py:351-377)
  * jpm_forward      build_transformer_local.forward in eval mode (make_models.py:314-377)
  * seeded_state     the per-key seeded weights the golden generator loads into the reference model (only seeds are stored)
"""
import torch
import torch.nn.functional as F


def token_map(n_patches, shift, groups, divide=4, rearrange=True):
    """-> (list of `divide` runs of 1-based patch indices, full shuffled list).  Raises ValueError where the reference's view() raises."""
    order = list(range(1, n_patches + 1))
    if rearrange:
        order = order[shift - 1:] + order[:shift - 1]              # features[:, shift:] then features[:, 1:shift]
        if len(order) % groups:
            order = order + [order[-2]]                             # x[:, -2:-1] appended once
        if len(order) % groups:
            raise ValueError("cannot view %d tokens as %d groups" % (len(order), groups))
        per = len(order) // groups
        order = [order[g * per + j] for j in range(per) for g in range(groups)]      # [groups][per] -> [per][groups]
    L = n_patches // divide
    return [order[i * L:(i + 1) * L] for i in range(divide)], order


def sie_index(cam, view, cam_num, view_num):
    cam = None if cam is None else torch.as_tensor(cam, dtype=torch.long)
    view = None if view is None else torch.as_tensor(view, dtype=torch.long)
    if cam_num > 1 and view_num > 1:
        return cam * view_num + view
    if cam_num > 1:
        return cam
    if view_num > 1:
        return view
    return None


def tokens(sd, x, stride, idx=None, coef=0.0, prefix="base."):
    g = lambda k: sd[prefix + k]
    t = F.conv2d(x, g("patch_embed.proj.weight"), g("patch_embed.proj.bias"), stride=stride).flatten(2).transpose(1, 2)
    t = torch.cat((g("cls_token").expand(x.shape[0], -1, -1), t), dim=1) + g("pos_embed")
    if idx is not None:
        t = t + coef * g("sie_embed")[idx]                          # [B, 1, C] broadcast over the tokens
    return t


def block(sd, p, t, num_heads, eps=1e-6):
    B, N, dim = t.shape
    hd = dim // num_heads
    h = F.layer_norm(t, (dim,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
    qkv = F.linear(h, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"]).reshape(B, N, 3, num_heads, hd).permute(2, 0, 3, 1, 4)
    attn = ((qkv[0] @ qkv[1].transpose(-2, -1)) * hd ** -0.5).softmax(dim=-1)
    h = (attn @ qkv[2]).transpose(1, 2).reshape(B, N, dim)
    t = t + F.linear(h, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
    h = F.layer_norm(t, (dim,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
    return t + F.linear(F.gelu(F.linear(h, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])), sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])


def _depth(sd, prefix="base."):
    d = 0
    while prefix + "blocks.%d.norm1.weight" % d in sd:
        d += 1
    return d


def local_features(sd, x, num_heads, stride, idx=None, coef=0.0):
    t = tokens(sd, x, stride, idx, coef)
    for i in range(_depth(sd) - 1):
        t = block(sd, "base.blocks.%d." % i, t, num_heads)
    return t


def jpm_head(feats, sd, after, eps=1e-5):
    """feats: [global, l1, l2, l3, l4], each [B, C]."""
    out = []
    for i, f in enumerate(feats):
        name = "bottleneck_%d" % i if i else "bottleneck"
        if after:
            f = (f - sd[name + ".running_mean"]) * torch.rsqrt(sd[name + ".running_var"] + eps) * sd[name + ".weight"] + sd[name + ".bias"]
        out.append(f / 4 if i else f)
    return torch.cat(out, dim=1)


def jpm_forward(sd, x, num_heads, stride, shift, groups, rearrange, after, idx=None, coef=0.0, eps=1e-6):
    feats = local_features(sd, x, num_heads, stride, idx, coef)
    dim = feats.shape[-1]
    norm = lambda t, p: F.layer_norm(t, (dim,), sd[p + "weight"], sd[p + "bias"], eps)
    out = [norm(block(sd, "b1.0.", feats, num_heads), "b1.1.")[:, 0]]
    runs, _ = token_map(feats.shape[1] - 1, shift, groups, 4, rearrange)
    for run in runs:
        seq = torch.cat((feats[:, 0:1], feats[:, run]), dim=1)
        out.append(norm(block(sd, "b2.0.", seq, num_heads), "b2.1.")[:, 0])
    return jpm_head(out, sd, after)


def _is_norm_weight(k):
    return (k.endswith(("norm1.weight", "norm2.weight", "norm.weight")) or k in ("b1.1.weight", "b2.1.weight")
            or (k.startswith("bottleneck") and k.endswith(".weight")))


def parse_shape(s):
    return tuple(int(v) for v in s.strip("()").split(",") if v.strip())


def seeded_state(keys, shapes):
    """key i gets a generator seeded 1000 + i (the scheme of tests/test_gpu_vit.py::_golden_state, extended to the JPM / SIE keys)."""
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
            sd[k] = 0.02 * torch.randn(shape, generator=gg)
    return sd


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp(min=1e-30))
