"""TransReID's two small backbones (make_models.py:392-397) on the HIP plan: DeiT-Small (dim 384, 6 heads of 64; evaluates and trains) and
ViT-Small (dim 768, 8 heads of 96, no qkv bias, scale 768 ** -0.5; evaluation only, on the chunked head-dim-96 attention forward).

Reference outputs: tests/golden/vit_small.npz (the reference's own models on the CPU, tests/golden/make_vit_small_golden.py), bound rel-L2 < 2e-2,
this project's bound for that comparison (tests/test_gpu_vit_long.py).  Training: the bounds of tests/test_gpu_vit.py::
test_small_vit_forward_backward_vs_oracle (feature 3e-2, gradients 8e-2, base.norm.* 2e-3 absolute)."""
import ctypes
import types

import numpy as np
import pytest
import torch

from conftest import load_golden
import vit_small_ref as R

pytestmark = pytest.mark.gpu
VS, DS = "vit_small_patch16_224_TransReID", "deit_small_patch16_224_TransReID"
LIMIT = -4                  # DALI_ERR_LIMIT


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _cfg(name, size, stride, jpm=False, sie=False, coef=3.0, neck_feat="after"):
    return types.SimpleNamespace(
        MODEL=types.SimpleNamespace(NAME="transformer", JPM=jpm, LAST_STRIDE=1, PRETRAIN_PATH="", PRETRAIN_CHOICE="none", COS_LAYER=False,
                                    NECK="bnneck", TRANSFORMER_TYPE=name, SIE_CAMERA=sie, SIE_VIEW=sie, SIE_COE=coef, STRIDE_SIZE=stride,
                                    DROP_PATH=0.0, DROP_OUT=0.0, ATT_DROP_RATE=0.0, ID_LOSS_TYPE="softmax", RE_ARRANGE=jpm, SHUFFLE_GROUP=2,
                                    SHIFT_NUM=5, DEVIDE_LENGTH=4),
        TEST=types.SimpleNamespace(NECK_FEAT=neck_feat), INPUT=types.SimpleNamespace(SIZE_TRAIN=size))


def _keys_and_shapes(model, z, pre):
    keys, shapes = [str(k) for k in z[pre + "keys"]], [str(s) for s in z[pre + "shapes"]]
    assert list(model.state_dict().keys()) == keys                                   # the reference's keys, same order
    for (k, v), shp in zip(model.state_dict().items(), shapes):
        assert str(tuple(v.shape)) == shp, k
    return keys, shapes


# vs16: 129 tokens (one key in the second chunk of 128); vs12: 311 tokens; ds16: DeiT-Small, 129 tokens on the head-dim-64 kernels
@pytest.mark.parametrize("name,typ,tokens", [("vs16", VS, 129), ("vs12", VS, 311), ("ds16", DS, 129)])
def test_small_backbones_match_reference_outputs(name, typ, tokens):
    _need_gpu()
    from daliid_amd import make_models
    z = load_golden("vit_small.npz")
    H, W, stride = (int(v) for v in z[name + "/geom"])
    model = make_models.make_model(_cfg(typ, (H, W), stride), 10, 0, 0)
    assert model.num_tokens == tokens
    keys, shapes = _keys_and_shapes(model, z, name + "/")
    if typ == VS:
        assert not any(k.endswith("attn.qkv.bias") for k in keys) and model.in_planes == 768
        assert tuple(model.state_dict()["base.blocks.0.mlp.fc1.weight"].shape) == (2304, 768)
    else:
        assert model.in_planes == 384 and all(tuple(v.shape) == (384,) for k, v in model.state_dict().items() if k.startswith("bottleneck.") and v.dim())
    model.load_state_dict(R.seeded_state(keys, shapes, float(z["qkv_std"]) if typ == VS else 0.02))
    model.eval()
    x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(int(z["x_seed"])))
    with torch.no_grad():
        y = model(x.cuda()).cpu()
        gf = model.global_feat(x.cuda()).cpu()
    e_gf, e_y = R.rel_l2(gf, torch.from_numpy(z[name + "/global_feat"])), R.rel_l2(y, torch.from_numpy(z[name + "/y_eval"]))
    print("%s at %dx%d stride %d (%d tokens), eval: global_feat rel-L2 %.3e, post-neck feat rel-L2 %.3e" % (typ, H, W, stride, tokens, e_gf, e_y))
    assert e_gf < 2e-2 and e_y < 2e-2


def test_vit_small_jpm_with_sie_matches_reference_outputs():
    """128 patches, four runs of 32 (+ cls = 33 tokens) through the head-dim-96 kernel; depth 2, 3 cameras x 2 views, 'after'"""
    _need_gpu()
    from daliid_amd import make_models
    z = load_golden("vit_small.npz")
    H, W, stride, depth, cams, views, seed = (int(v) for v in z["vsjpm/geom"])
    model = make_models.make_model(_cfg(VS, (H, W), stride, True, True, float(z["vsjpm/coef"]), str(z["vsjpm/neck_feat"])), 10, cams, views, depth=depth)
    assert model.token_map.shape == (4, 32)
    keys, shapes = _keys_and_shapes(model, z, "vsjpm/")
    assert not any(k.endswith("attn.qkv.bias") for k in keys) and "b2.0.attn.qkv.weight" in keys
    model.load_state_dict(R.seeded_state(keys, shapes, float(z["qkv_std"])))
    model.eval()
    x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(seed))
    with torch.no_grad():
        y = model(x.cuda(), cam_label=z["vsjpm/cam"], view_label=z["vsjpm/view"]).cpu()
    ref = torch.from_numpy(z["vsjpm/y"])
    assert y.shape == ref.shape == (2, 3840)
    errs = [R.rel_l2(y[:, i * 768:(i + 1) * 768], ref[:, i * 768:(i + 1) * 768]) for i in range(5)]
    print("ViT-Small JPM + SIE at 256x128 / 16: rel-L2 of (global, l1, l2, l3, l4) vs the fp32 reference: %s" % " ".join("%.3e" % e for e in errs))
    assert max(errs) < 2e-2, errs


def test_jpm_with_deit_small_is_refused():
    _need_gpu()
    from daliid_amd import make_models
    with pytest.raises(NotImplementedError, match=r"768-wide necks.*make_models\.py:229.*first forward"):
        make_models.make_model(_cfg(DS, (256, 128), 16, jpm=True), 10, 0, 0, depth=2)


def _perturb(net, seed=4):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in net.parameters():
            p.add_((0.05 * torch.randn(p.shape, generator=g)).to(p.device))
    net.mark_weights_changed()
    return g


def _train_and_compare(net, ref_fn, x, w):
    """the comparison of tests/test_gpu_vit.py::test_small_vit_forward_backward_vs_oracle, with its bounds; ref_fn(sd, training) -> feat"""
    pnames = {n for n, _ in net.named_parameters()}
    sd = {k: v.detach().cpu().clone().requires_grad_(k in pnames) for k, v in net.state_dict().items()}
    ref = ref_fn(sd, True)
    (ref * w).sum().backward()
    net.train()
    y = net(x.cuda())
    (y * w.cuda()).sum().backward()
    e = R.rel_l2(y.detach().cpu(), ref.detach())
    print("train-mode feat rel-L2 %.3e" % e)
    assert e < 3e-2
    worst, bad = ("", 0.0), []
    for name, p in net.named_parameters():
        if name.startswith("base.fc.") or name == "bottleneck.bias":
            continue                                   # unused head (zero gradient) / frozen neck bias
        r = R.rel_l2(p.grad.cpu(), sd[name].grad)
        if r > worst[1]:
            worst = (name, r)
        if name.startswith("base.norm."):              # ~0 in exact arithmetic under a train-mode BatchNorm: on the scale of the other gradients
            assert float((p.grad.cpu() - sd[name].grad).abs().max()) < 2e-3, name
            continue
        if r >= 8e-2:
            bad.append((name, r, float(p.grad.abs().max()), float(sd[name].grad.abs().max())))
    print("worst gradient rel-L2 %.3e at %s" % (worst[1], worst[0]))
    assert not bad, bad
    assert float(net.base.fc.weight.grad.abs().max()) == 0.0
    net.eval()
    with torch.no_grad():
        e2 = R.rel_l2(net(x.cuda()).cpu(), ref_fn({k: v.cpu() for k, v in net.state_dict().items()}, False))
    print("eval-mode feat rel-L2 %.3e" % e2)
    assert e2 < 3e-2, e2


def test_deit_small_width_trains_vs_oracle():
    """C = 384, H = 6: linears at N = 384 / 1152 / 1536 and K = 384 / 1536, LayerNorm and neck at 384; 7 x 3 + 1 = 22 tokens, B = 6"""
    _need_gpu()
    from daliid_amd import vit_pytorch as V
    from oracle import vit as OV
    net = V.ViTNeckNet(img_size=(96, 48), patch_size=16, stride_size=12, embed_dim=384, depth=2, num_heads=6, mlp_ratio=4.0, num_classes=10, seed=3)
    assert net.num_tokens == 22
    g = _perturb(net)
    x, w = torch.randn(6, 3, 96, 48, generator=g), torch.randn(6, 384, generator=g)
    _train_and_compare(net, lambda sd, training: OV.build_transformer_forward(sd, x, num_heads=6, patch=16, stride=12, training=training), x, w)


def test_biasless_qkv_and_a_set_scale_train_at_head_dim_64():
    _need_gpu()
    from daliid_amd import vit_pytorch as V
    net = V.ViTNeckNet(img_size=(64, 32), patch_size=16, stride_size=16, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4.0, num_classes=10, seed=3,
                       qkv_bias=False, qk_scale=0.2)
    names = [n for n, _ in net.named_parameters()]
    assert not any(n.endswith("attn.qkv.bias") for n in names) and "base.blocks.1.attn.qkv.weight" in names
    assert not any(k.endswith("attn.qkv.bias") for k in net.state_dict())
    g = _perturb(net)
    x, w = torch.randn(6, 3, 64, 32, generator=g), torch.randn(6, 128, generator=g)
    _train_and_compare(net, lambda sd, training: R.forward(sd, x, 2, 16, qk_scale=0.2, training=training)[0], x, w)
    # the scale is really the set one: the head width's own scale (0.125) gives another feature
    with torch.no_grad():
        sd = {k: v.cpu() for k, v in net.state_dict().items()}
        shift = R.rel_l2(R.forward(sd, x, 2, 16, qk_scale=None, training=True)[0], R.forward(sd, x, 2, 16, qk_scale=0.2, training=True)[0])
    print("scale 0.125 instead of 0.2 moves the train-mode feature by %.3f rel-L2" % shift)
    assert shift > 5e-2                                # above the 3e-2 bound: a plan that ignored qk_scale would not pass


# ------------------------------------------------------------------------------------------------------------------- head_dim 96: eval only
def _hd96_net(heads=2):
    from daliid_amd import vit_pytorch as V
    net = V.ViTNeckNet(img_size=(64, 48), patch_size=16, stride_size=8, embed_dim=192, depth=2, num_heads=heads, mlp_ratio=4.0, num_classes=10, seed=3,
                       qkv_bias=False, qk_scale=192 ** -0.5)
    _perturb(net)
    return net


@pytest.fixture(scope="module")
def small96():
    """7 x 5 + 1 = 36 tokens, two heads of 96; the eval output is computed once and shared (the later tests compare with it bit for bit)"""
    _need_gpu()
    net = _hd96_net()
    assert net.num_tokens == 36 and net.head_dim == 96
    x = torch.randn(3, 3, 64, 48, generator=torch.Generator().manual_seed(6))
    net.eval()
    with torch.no_grad():
        y = net(x.cuda()).clone()
    return types.SimpleNamespace(net=net, x=x, y=y)


def test_small_head_dim_96_model_eval_vs_restatement(small96):
    sd = {k: v.detach().cpu() for k, v in small96.net.state_dict().items()}
    with torch.no_grad():
        ref, _ = R.forward(sd, small96.x, 2, 8, qk_scale=192 ** -0.5)
    e = R.rel_l2(small96.y.cpu(), ref)
    print("36 tokens, head_dim 96, eval: post-neck feat rel-L2 %.3e" % e)
    assert e < 3e-2


def test_training_at_head_dim_96_is_refused_and_the_model_stays_usable(small96):
    from daliid_amd import _lib
    net, msg = small96.net, "training needs head_dim 64 (this plan has 96); eval mode only"
    net.train()
    try:
        with pytest.raises(_lib.DaliError, match=r"head_dim 64.*\.eval\(\).*torch\.no_grad\(\)"):
            net(small96.x.cuda())
        # the plan refuses too, before any launch: the train-mode forward without autograd, and the backward entries
        with torch.no_grad(), pytest.raises(_lib.DaliError, match="training needs head_dim 64 \\(this plan has 96\\); eval mode only"):
            net(small96.x.cuda())
        plan = net._plan(3)
        x, feat, d = small96.x.cuda().contiguous(), torch.empty(3, 192, device="cuda"), torch.zeros(3, 192, device="cuda")
        rc = _lib.lib().dali_vit_forward_ex(plan.h, _lib.stream_ptr(), _lib.ptr(x), None, 1, _lib.ptr(feat), None, None)
        assert rc == LIMIT and msg in _lib.last_error()
        for rc in (_lib.lib().dali_vit_backward(plan.h, _lib.stream_ptr(), _lib.ptr(d)),
                   _lib.lib().dali_vit_backward_stages(plan.h, _lib.stream_ptr(), _lib.ptr(d), 0, 0)):
            assert rc == LIMIT and msg in _lib.last_error()
        # none of the backward's buffers: a trainable twin (three heads of 64, everything else equal) needs a larger arena
        twin = _hd96_net(heads=3)
        assert plan.arena_bytes < twin._plan(3).arena_bytes and plan.param_elems == twin._plan(3).param_elems
    finally:
        net.eval()
    with torch.no_grad():
        assert torch.equal(net(small96.x.cuda()), small96.y)


def test_other_head_widths_are_refused_at_create():
    _need_gpu()
    from daliid_amd import _lib
    from daliid_amd.vit_pytorch import _VitCfg
    h, cfg = ctypes.c_void_p(), _VitCfg(2, 64, 48, 16, 16, 160, 2, 2, 640, 10)              # dim 160, 2 heads: head_dim 80
    rc = _lib.lib().dali_vit_create(_lib.ctx(0), ctypes.byref(cfg), ctypes.byref(h))
    assert rc != 0 and not h.value
    err = _lib.last_error()
    assert "dim=160" in err and "heads=2" in err and "64 or 96" in err


def test_extract_features_and_validate_at_head_dim_96(small96):
    from daliid_amd import getFeatures, ops_eval, validateModels
    net = small96.net.eval()
    images = torch.randn(10, 3, 64, 48, generator=torch.Generator().manual_seed(21))
    records = np.array([["img%02d" % i, str(i % 4), str(i % 3), "person"] for i in range(10)])
    getFeatures.set_image_loader(lambda paths, h, w, turb=None: images[[int(p[3:]) for p in paths]])
    try:
        fvs = getFeatures.extractFeatures(records[:5], 64, 48, net, 2, gpu_index=0, keep_on_device=True, verbose=False)          # batches of 2, 2, 1
        with torch.no_grad():
            direct = torch.cat([net(images[b:b + 2].cuda()) for b in (0, 2)] + [net(images[4:5].cuda())], 0)
        assert fvs.shape == (5, 192) and torch.equal(fvs, direct)
        validator = validateModels.validationManager.getValidator("Market")
        validator.setParameters(64, 48, False, 0)
        cmc, mAP, distmat = validator.validate(records[:4], records[4:], net)
        with torch.no_grad():
            fq, fg = net(images[:4].cuda()), net(images[4:].cuda())
        want = ops_eval.pairdist(fq.contiguous(), fg.contiguous(), metric="cosine", precision=validator.precision, normalize=True)
        assert tuple(distmat.shape) == (4, 6) and torch.equal(distmat, want) and 0.0 <= mAP <= 1.0
    finally:
        getFeatures.set_image_loader(None)
