"""Evaluation past 256 tokens: the chunked attention forward (attention_fwd_long_kernel: key chunks of 256 under an online softmax), the
eval-only plan it allows (up to 1024 tokens), and the Python surface on top (TransReID at 384x128 / stride 12 = 311 tokens and at
256x256 / stride 16 = 257, JPM + SIE, extractFeatures / validate), plus the position-embedding resize a checkpoint of another size needs.

Kernel tests compare with torch CPU fp32 attention on the same bf16 qkv, by the criteria of tests/test_gpu_vit_ops.py::test_attention_fwd_bwd:
output |err| <= 2^-7 |ref| + 4e-3 max|ref|, lse rtol = atol = 1e-4.  Model tests use the bounds of the same comparisons at <= 256 tokens."""
import os
import types

import numpy as np
import pytest
import torch

from conftest import load_golden

bf16 = torch.bfloat16
gpu = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def close(got, ref, rel=2.0 ** -7, abs_frac=4e-3):
    got, ref = got.float().cpu(), ref.float()
    err = (got - ref).abs()
    tol = rel * ref.abs() + abs_frac * ref.abs().max()
    assert (err <= tol).all(), "max err %.4g (ref scale %.4g), worst err / tol %.3f" % (float(err.max()), float(ref.abs().max()), float((err / tol).max()))


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp(min=1e-30))


def _qkv(B, T, H, seed=None):
    g = torch.Generator().manual_seed(B * 1000 + T + H if seed is None else seed)
    return torch.randn(B * T, 3 * H * 64, generator=g)


def _ref_attention(qkv, B, T, H):
    """fp32 attention and row log-sum-exp on the bf16-rounded qkv (vit_pytorch.py:155 layout), scale 0.125"""
    t = qkv.to(bf16).float().reshape(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (t[0] @ t[1].transpose(-2, -1)) * 0.125
    out = (s.softmax(dim=-1) @ t[2]).transpose(1, 2).reshape(B * T, H * 64)
    return out, torch.logsumexp(s, dim=-1).reshape(B * H, T)


def _check(fn, qkv, B, T, H):
    ref, ref_lse = _ref_attention(qkv, B, T, H)
    out, lse = fn(qkv.to(bf16).cuda(), B, T, H, 0.125)
    assert out.shape == (B * T, H * 64) and lse.shape == (B * H, T)
    close(out, ref)
    np.testing.assert_allclose(lse.cpu().numpy(), ref_lse.numpy(), rtol=1e-4, atol=1e-4)


# (2, 257, 2): one key in the second chunk, one query in the third query block (seven idle waves); 272 / 273: a tile edge in the second chunk;
# (2, 311, 12): 384x128 at stride 12; (3, 385, 2): one query in the fourth query block, three sequences adjacent in memory; 512 / 513: a chunk
# edge; (2, 577, 4): 384x384 at stride 16; (1, 1024, 2): the cap, four full chunks
@gpu
@pytest.mark.parametrize("B,T,H", [(2, 257, 2), (1, 272, 1), (2, 273, 2), (2, 311, 12), (3, 385, 2), (2, 512, 2), (2, 513, 2), (2, 577, 4), (1, 1024, 2)])
def test_attention_fwd_past_256_tokens(B, T, H):
    _need_gpu()
    from daliid_amd import ops_vit
    _check(ops_vit.attention_fwd, _qkv(B, T, H), B, T, H)


# the running maximum has to move in both directions: keys of the last chunk (rows >= 512) times 4 -> every row's maximum moves there and
# everything accumulated before is scaled down; keys of the first tile times 4 -> the first chunk dominates and alpha = 1 afterwards
@gpu
@pytest.mark.parametrize("which", ["last_chunk", "first_tile"])
def test_attention_fwd_long_rescales_in_both_directions(which):
    _need_gpu()
    from daliid_amd import ops_vit
    B, T, H = 2, 513, 2
    C = H * 64
    qkv = _qkv(B, T, H).reshape(B, T, 3 * C).clone()
    if which == "last_chunk":
        qkv[:, 512:, C:2 * C] *= 4
    else:
        qkv[:, :16, C:2 * C] *= 4
    _check(ops_vit.attention_fwd, qkv.reshape(B * T, 3 * C), B, T, H)


# the chunked kernel on its own below its routing threshold: one chunk, idle waves (T = 1: one live query of 128), a tile edge, 197, a full chunk
@gpu
@pytest.mark.parametrize("T", [1, 16, 17, 197, 256])
def test_attention_fwd_long_one_chunk(T):
    _need_gpu()
    from daliid_amd import ops_vit
    _check(ops_vit.attention_fwd_long, _qkv(2, T, 4), 2, T, 4)


@gpu
def test_attention_fwd_long_without_lse_is_bitwise_the_same():
    _need_gpu()
    from daliid_amd import ops_vit
    B, T, H = 2, 311, 2
    qkv = _qkv(B, T, H).to(bf16).cuda()
    out, lse = ops_vit.attention_fwd_long(qkv, B, T, H)
    out2, none = ops_vit.attention_fwd_long(qkv, B, T, H, with_lse=False)
    assert none is None and lse is not None
    assert torch.equal(out.view(torch.int16), out2.view(torch.int16))


@gpu
def test_attention_limits_are_refused_without_a_launch():
    _need_gpu()
    from daliid_amd import _lib, ops_vit
    H = 1
    qkv = torch.zeros(1025, 3 * 64, dtype=bf16, device="cuda")
    for fn in (ops_vit.attention_fwd, ops_vit.attention_fwd_long):
        with pytest.raises(_lib.DaliError, match="1025 tokens exceed the limit of 1024"):
            fn(qkv, 1, 1025, H)
        assert "1025 tokens exceed the limit of 1024" in _lib.last_error()
    # the backward keeps its limit
    q = torch.zeros(257, 3 * 64, dtype=bf16, device="cuda")
    o = torch.zeros(257, 64, dtype=bf16, device="cuda")
    lse = torch.zeros(1, 257, device="cuda")
    with pytest.raises(_lib.DaliError, match="256"):
        ops_vit.attention_bwd(q, o, o, lse, 1, 257, H)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------- the small model
def _perturbed_small_net():
    from daliid_amd import vit_pytorch as V
    net = V.ViTNeckNet(img_size=(160, 128), patch_size=16, stride_size=8, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4.0, num_classes=10, seed=3)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for p in net.parameters():
            p.add_((0.05 * torch.randn(p.shape, generator=g)).to(p.device))
    net.mark_weights_changed()
    return net, g


@pytest.fixture(scope="module")
def small():
    """19 x 15 + 1 = 286 tokens; parameters perturbed as tests/test_gpu_vit.py::test_small_vit_forward_backward_vs_oracle does; batch 3.
    The eval output is computed once and shared (the later tests compare against it bit for bit)."""
    _need_gpu()
    net, g = _perturbed_small_net()
    assert net.num_tokens == 286
    x = torch.randn(3, 3, 160, 128, generator=g)
    net.eval()
    with torch.no_grad():
        y = net(x.cuda()).clone()
        gf = net.global_feat(x.cuda()).clone()
    return types.SimpleNamespace(net=net, x=x, y=y, gf=gf)


@gpu
def test_small_model_286_tokens_eval_vs_oracle(small):
    from oracle import vit as OV
    sd = {k: v.detach().cpu() for k, v in small.net.state_dict().items()}
    with torch.no_grad():
        ref = OV.build_transformer_forward(sd, small.x, num_heads=2, patch=16, stride=8, training=False)
        ref_gf = OV.transreid_forward(sd, small.x, 2, 16, 8, prefix="base.")
    e_y, e_gf = rel_l2(small.y.cpu(), ref), rel_l2(small.gf.cpu(), ref_gf)
    print("286 tokens, eval: post-neck feat rel-L2 %.3e, global_feat rel-L2 %.3e" % (e_y, e_gf))
    assert e_y < 3e-2 and e_gf < 3e-2


@gpu
def test_training_past_256_tokens_is_refused_and_the_model_stays_usable(small):
    from daliid_amd import _lib
    net = small.net
    net.train()
    try:
        with pytest.raises(_lib.DaliError, match=r"256 tokens.*\.eval\(\).*torch\.no_grad\(\)"):
            net(small.x.cuda())
        # the plan refuses too, before any launch: the train-mode forward without autograd, and the backward entries
        with torch.no_grad(), pytest.raises(_lib.DaliError, match="training needs at most 256 tokens \\(this plan has 286\\); eval mode only"):
            net(small.x.cuda())
        plan = net._plan(3)
        d = torch.zeros(3, 128, device="cuda")
        for rc in (_lib.lib().dali_vit_backward(plan.h, _lib.stream_ptr(), _lib.ptr(d)),
                   _lib.lib().dali_vit_backward_stages(plan.h, _lib.stream_ptr(), _lib.ptr(d), 0, 0)):
            assert rc == -4 and "training needs at most 256 tokens (this plan has 286); eval mode only" in _lib.last_error()
    finally:
        net.eval()
    with torch.no_grad():
        assert torch.equal(net(small.x.cuda()), small.y)


@gpu
def test_local_tokens_past_256_tokens():
    """local_feature=True at 286 tokens: blocks[:-1], all tokens, no final norm -- against the oracle's block on the same weights"""
    _need_gpu()
    from daliid_amd import vit_pytorch as V
    import vit_jpm_ref as R
    net = V.ViTNeckNet(img_size=(160, 128), patch_size=16, stride_size=8, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4.0, num_classes=10, seed=3,
                       local_feature=True).eval()
    x = torch.randn(2, 3, 160, 128, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        tok = net.local_tokens(x.cuda()).cpu()
        ref = R.local_features({k: v.detach().cpu() for k, v in net.state_dict().items()}, x, 2, 8)
    assert tok.shape == ref.shape == (2, 286, 128)
    assert rel_l2(tok, ref) < 3e-2


@gpu
def test_extract_features_and_validate_past_256_tokens(small):
    from daliid_amd import getFeatures, ops_eval, validateModels
    net = small.net.eval()
    images = torch.randn(10, 3, 160, 128, generator=torch.Generator().manual_seed(21))
    records = np.array([["img%02d" % i, str(i % 4), str(i % 3), "person"] for i in range(10)])
    getFeatures.set_image_loader(lambda paths, h, w, turb=None: images[[int(p[3:]) for p in paths]])
    try:
        fvs = getFeatures.extractFeatures(records[:5], 160, 128, net, 2, gpu_index=0, keep_on_device=True, verbose=False)        # batches of 2, 2, 1
        with torch.no_grad():
            direct = torch.cat([net(images[b:b + 2].cuda()) for b in (0, 2)] + [net(images[4:5].cuda())], 0)
        assert fvs.shape == (5, 128) and torch.equal(fvs, direct)
        validator = validateModels.validationManager.getValidator("Market")
        validator.setParameters(160, 128, False, 0)
        cmc, mAP, distmat = validator.validate(records[:4], records[4:], net)
        with torch.no_grad():
            fq, fg = net(images[:4].cuda()), net(images[4:].cuda())
        want = ops_eval.pairdist(fq.contiguous(), fg.contiguous(), metric="cosine", precision=validator.precision, normalize=True)
        assert tuple(distmat.shape) == (4, 6) and torch.equal(distmat, want) and 0.0 <= mAP <= 1.0
    finally:
        getFeatures.set_image_loader(None)


# ------------------------------------------------------------------------------------------------------------------- the reference's outputs
def _cfg(size, stride, jpm=False, sie_cam=False, sie_view=False, coef=3.0, neck_feat="after", pretrain=("none", "")):
    return types.SimpleNamespace(
        MODEL=types.SimpleNamespace(NAME="transformer", JPM=jpm, LAST_STRIDE=1, PRETRAIN_PATH=pretrain[1], PRETRAIN_CHOICE=pretrain[0], COS_LAYER=False,
                                    NECK="bnneck", TRANSFORMER_TYPE="vit_base_patch16_224_TransReID", SIE_CAMERA=sie_cam, SIE_VIEW=sie_view,
                                    SIE_COE=coef, STRIDE_SIZE=stride, DROP_PATH=0.0, DROP_OUT=0.0, ATT_DROP_RATE=0.0, ID_LOSS_TYPE="softmax",
                                    RE_ARRANGE=jpm, SHUFFLE_GROUP=2, SHIFT_NUM=5, DEVIDE_LENGTH=4),
        TEST=types.SimpleNamespace(NECK_FEAT=neck_feat), INPUT=types.SimpleNamespace(SIZE_TRAIN=size))


def _gen_vit_state(keys, shapes):
    """the per-key seeded weights tests/golden/make_vit_long_golden.py loaded into the reference model (make_golden.gen_vit's recipe)"""
    sd = {}
    for i, (k, shp) in enumerate(zip(keys, shapes)):
        shape = tuple(int(v) for v in shp.strip("()").split(",") if v.strip())
        gg = torch.Generator().manual_seed(1000 + i)
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.zeros((), dtype=torch.long)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(shape, generator=gg)
        elif k.endswith("norm1.weight") or k.endswith("norm2.weight") or k.endswith("norm.weight") or k == "bottleneck.weight":
            sd[k] = 1.0 + 0.1 * torch.randn(shape, generator=gg)
        else:
            sd[k] = 0.02 * torch.randn(shape, generator=gg)
    return sd


# 384x128 at stride 12: 31 x 10 + 1 = 311 tokens; 256x256 at stride 16 (the vehicle size): 16 x 16 + 1 = 257
@gpu
@pytest.mark.parametrize("name,tokens", [("s12", 311), ("v16", 257)])
def test_full_vit_b16_past_256_tokens_matches_reference_outputs(name, tokens):
    _need_gpu()
    from daliid_amd import make_models
    z = load_golden("vit_long.npz")
    H, W, stride = (int(v) for v in z[name + "/geom"])
    keys, shapes = [str(k) for k in z[name + "/keys"]], [str(s) for s in z[name + "/shapes"]]
    model = make_models.make_model(_cfg((H, W), stride), 10, 0, 0)
    assert model.num_tokens == tokens
    assert list(model.state_dict().keys()) == keys                                   # the reference's keys, same order
    for (k, v), shp in zip(model.state_dict().items(), shapes):
        assert str(tuple(v.shape)) == shp, k
    model.load_state_dict(_gen_vit_state(keys, shapes))
    model.eval()
    x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(77))
    with torch.no_grad():
        y = model(x.cuda()).cpu()
        gf = model.global_feat(x.cuda()).cpu()
    e_gf, e_y = rel_l2(gf, torch.from_numpy(z[name + "/global_feat"])), rel_l2(y, torch.from_numpy(z[name + "/y_eval"]))
    print("ViT-B/16 at %dx%d stride %d (%d tokens), eval: global_feat rel-L2 %.3e, post-neck feat rel-L2 %.3e" % (H, W, stride, tokens, e_gf, e_y))
    assert e_gf < 2e-2 and e_y < 2e-2


@gpu
def test_jpm_with_sie_at_384x128_stride_12_matches_reference_outputs():
    """310 patches, four runs of 77 (+ cls = 78 tokens: the regular kernel, not the short one); depth 2, 3 cameras x 2 views"""
    _need_gpu()
    from daliid_amd import make_models
    import vit_jpm_ref as R
    z = load_golden("vit_long.npz")
    H, W, stride, depth, cams, views, seed = (int(v) for v in z["jpm/geom"])
    keys, shapes = [str(k) for k in z["jpm/keys"]], [str(s) for s in z["jpm/shapes"]]
    model = make_models.make_model(_cfg((H, W), stride, True, True, True, float(z["jpm/coef"]), str(z["jpm/neck_feat"])), 10, cams, views, depth=depth)
    assert model.token_map.shape == (4, 77)
    assert list(model.state_dict().keys()) == keys
    for (k, v), shp in zip(model.state_dict().items(), shapes):
        assert str(tuple(v.shape)) == shp, k
    model.load_state_dict(R.seeded_state(keys, shapes))
    model.eval()
    x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(seed))
    with torch.no_grad():
        y = model(x.cuda(), cam_label=z["jpm/cam"], view_label=z["jpm/view"]).cpu()
    ref = torch.from_numpy(z["jpm/y"])
    assert y.shape == ref.shape == (2, 3840)
    errs = [R.rel_l2(y[:, i * 768:(i + 1) * 768], ref[:, i * 768:(i + 1) * 768]) for i in range(5)]
    print("JPM + SIE at 384x128 / 12: rel-L2 of (global, l1, l2, l3, l4) vs the fp32 reference: %s" % " ".join("%.3e" % e for e in errs))
    assert max(errs) < 2e-2, errs


# ------------------------------------------------------------------------------------------------------------------- checkpoints of another size
def test_resize_pos_embed_matches_the_reference():
    """host-side torch: needs no GPU and no library"""
    from daliid_amd import vit_pytorch as V
    z = load_golden("vit_long.npz")
    pos = torch.randn(1, 1 + 14 * 14, 16, generator=torch.Generator().manual_seed(int(z["resize/seed"])))
    for h, w in ((31, 10), (16, 16)):
        got = V.resize_pos_embed(pos, torch.zeros(1, 1 + h * w, 16), h, w)
        ref = torch.from_numpy(z["resize/%dx%d" % (h, w)])
        assert got.shape == ref.shape == (1, 1 + h * w, 16)
        assert torch.equal(got[:, 0], pos[:, 0])                                      # the cls row is kept
        assert float((got - ref).abs().max()) <= 1e-6
    with pytest.raises(ValueError):
        V.resize_pos_embed(pos[:, :-1], torch.zeros(1, 311, 16), 31, 10)              # 195 patch tokens are no square grid


@gpu
def test_load_param_resizes_pos_embed_and_skips_the_head(tmp_path):
    _need_gpu()
    from daliid_amd import vit_pytorch as V
    kw = dict(patch_size=16, embed_dim=128, depth=1, num_heads=2, qkv_bias=True, num_classes=10)
    src = V.TransReID(img_size=(224, 224), stride_size=16, seed=11, **kw)
    dst = V.TransReID(img_size=(384, 128), stride_size=12, seed=12, **kw)
    saved = {k: v.detach().cpu().clone() for k, v in src.state_dict().items()}
    assert saved["pos_embed"].shape == (1, 197, 128) and dst.state_dict()["pos_embed"].shape == (1, 311, 128)
    saved["head.weight"] = torch.randn(10, 128)
    path = str(tmp_path / "vit_224.pth")
    torch.save({"model": saved}, path)                                                # wrapped, as the public ViT checkpoints are
    before = {k: v.detach().cpu().clone() for k, v in dst.state_dict().items()}
    assert dst.load_param(path) == []
    after = {k: v.detach().cpu() for k, v in dst.state_dict().items()}
    assert "head.weight" not in after and set(after) == set(before)
    assert torch.equal(after["pos_embed"], V.resize_pos_embed(saved["pos_embed"], before["pos_embed"], 31, 10))
    for k in after:
        if k != "pos_embed":
            assert torch.equal(after[k], saved[k]), k
    assert not torch.equal(after["blocks.0.attn.qkv.weight"], before["blocks.0.attn.qkv.weight"])          # the two seeds did differ
    # an old checkpoint with a 2-D patch projection
    flat = dict(saved)
    flat["patch_embed.proj.weight"] = 2.0 * saved["patch_embed.proj.weight"].reshape(128, -1)
    torch.save(flat, path)
    assert dst.load_param(path) == []
    assert torch.equal(dst.state_dict()["patch_embed.proj.weight"].cpu(), 2.0 * saved["patch_embed.proj.weight"])
    dst.eval()
    with torch.no_grad():                                                             # the loaded weights reach the plan: 311 tokens, eval forward
        f = dst(torch.randn(2, 3, 384, 128, generator=torch.Generator().manual_seed(13)).cuda())
    assert f.shape == (2, 128) and bool(torch.isfinite(f).all())


def test_imagenet_pretrain_choice_without_a_local_file_is_still_refused():
    from daliid_amd import make_models
    cfg = _cfg((384, 128), 12, pretrain=("imagenet", os.path.join("no", "such", "jx_vit_base_p16_224.pth")))
    with pytest.raises(NotImplementedError, match="needs a file fetched from the network"):
        make_models.make_model(cfg, 10, 0, 0)


@gpu
def test_imagenet_pretrain_choice_loads_a_local_file(tmp_path):
    _need_gpu()
    from daliid_amd import make_models, vit_pytorch as V
    pos = torch.randn(1, 197, 768, generator=torch.Generator().manual_seed(14))
    cls = torch.randn(1, 1, 768, generator=torch.Generator().manual_seed(15))
    path = str(tmp_path / "jx_vit_base_p16_224.pth")
    torch.save({"pos_embed": pos, "cls_token": cls, "head.bias": torch.zeros(1000)}, path)
    model = make_models.make_model(_cfg((384, 128), 12, pretrain=("imagenet", path)), 10, 0, 0, depth=1)
    assert torch.equal(model.base.cls_token.detach().cpu(), cls)
    assert torch.equal(model.base.pos_embed.detach().cpu(), V.resize_pos_embed(pos, torch.zeros(1, 311, 768), 31, 10))
