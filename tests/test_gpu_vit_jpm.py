"""GPU: TransReID's JPM local branch and SIE embeddings on the ViT plan.  Kernels (jpm_gather, assemble_tokens_sie, sie_grad,
attention_fwd_short, jpm_head) against torch on the same inputs; the models against outputs of the REFERENCE's own build_transformer_local /
build_transformer (tests/golden/vit_jpm.npz: weights re-seeded per key, only outputs stored).

Measured on an MI355X (rel-L2 of the 768-wide slices against the fp32 reference, bound 2e-2): case A 1.12e-2 .. 1.16e-2, B 9.5e-3 .. 9.7e-3,
C 6.8e-3 .. 7.2e-3; local_feature tokens 4.6e-3; SIE train step: feature 9.1e-3 (bound 3e-2), sie_embed.grad 1.5e-2 (bound 8e-2).  The table is in
docs/experiments.md, "JPM local branch and SIE embeddings"."""
import types

import numpy as np
import pytest
import torch

from conftest import load_golden
import vit_jpm_ref as R

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
NAME = "vit_base_patch16_224_TransReID"


def close(got, ref, rel=2.0 ** -7, abs_frac=4e-3):
    """tests/test_gpu_vit_ops.py::close"""
    got, ref = got.float().cpu(), ref.float()
    err = (got - ref).abs()
    tol = rel * ref.abs() + abs_frac * ref.abs().max()
    assert (err <= tol).all(), "max err %.4g (ref scale %.4g)" % (float(err.max()), float(ref.abs().max()))


@pytest.fixture(scope="module")
def V():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from daliid_amd import ops_vit
    return ops_vit


@pytest.fixture(scope="module")
def z():
    return load_golden("vit_jpm.npz")


def _cfg(size, stride, jpm, sie_cam=False, sie_view=False, coef=3.0, neck_feat="after", groups=2, shift=5, rearrange=True):
    return types.SimpleNamespace(
        MODEL=types.SimpleNamespace(NAME="transformer", JPM=jpm, LAST_STRIDE=1, PRETRAIN_PATH="", PRETRAIN_CHOICE="none", COS_LAYER=False,
                                    NECK="bnneck", TRANSFORMER_TYPE=NAME, SIE_CAMERA=sie_cam, SIE_VIEW=sie_view, SIE_COE=coef, STRIDE_SIZE=stride,
                                    DROP_PATH=0.0, DROP_OUT=0.0, ATT_DROP_RATE=0.0, ID_LOSS_TYPE="softmax", RE_ARRANGE=rearrange,
                                    SHUFFLE_GROUP=groups, SHIFT_NUM=shift, DEVIDE_LENGTH=4),
        TEST=types.SimpleNamespace(NECK_FEAT=neck_feat), INPUT=types.SimpleNamespace(SIZE_TRAIN=size))


# ---------------------------------------------------------------------------------------------------------------- kernels
def _maps(z):
    from daliid_amd.make_models import jpm_token_map
    out = []
    for k in z.files:
        if k.startswith("shuffle/") and k != "shuffle/raises":
            n, groups, shift = (int(v) for v in k.split("/")[1].split("_"))
            out.append((n, jpm_token_map(n, shift, groups, 4, True), z[k]))
    out.append((128, jpm_token_map(128, 5, 2, 4, False), None))
    return out


@pytest.mark.parametrize("C", [64, 768])
def test_jpm_gather_bit_exact(V, z, C):
    """Integer-valued bf16 tokens, every stored shuffle plus rearrange=False; B = 3.  The padded duplicate of shuffle_unit always lands behind the
    four runs (position n of the shuffled order), so no map of jpm_token_map holds a token twice: the duplicate is checked on the reference's
    whole shuffled order of n = 9 (10 entries, token 3 twice) handed to the kernel as a [2][5] map."""
    B = 3
    g = torch.Generator().manual_seed(C)
    extra = [(9, z["shuffle/9_2_5"].reshape(2, 5).astype(np.int32), z["shuffle/9_2_5"])]
    for n, m, order in _maps(z) + extra:
        T = n + 1
        G, L = m.shape
        feat = torch.randint(-100, 101, (B, T, C), generator=g).to(bf16)
        out = V.jpm_gather(feat.reshape(B * T, C).cuda(), torch.from_numpy(m).cuda(), B, T).cpu().reshape(G, B, 1 + L, C)
        mt = torch.from_numpy(m.astype(np.int64))
        for gi in range(G):
            assert torch.equal(out[gi, :, 0], feat[:, 0]), (n, gi)                       # cls in row 0 of every sequence
            assert torch.equal(out[gi, :, 1:], feat[:, mt[gi]]), (n, gi)
        used = set(m.reshape(-1).tolist())
        assert 0 not in used and max(used) <= n
        if n == 210 and order is not None and G == 4:
            assert m.shape == (4, 52) and not set(order[208:].tolist()) & used         # the last two of the shuffled order are dropped
        if G == 2:
            assert sorted(m.reshape(-1).tolist()).count(3) == 2                          # the duplicate is present twice
            assert torch.equal(out[1, :, 1 + 0], feat[:, 3]) and torch.equal(out[1, :, 1 + 4], feat[:, 3])      # 5,1,6,2,7 | 3,8,4,9,3
    with pytest.raises(Exception):
        V.jpm_gather(torch.zeros(4, 12, dtype=bf16).cuda(), torch.ones(1, 1, dtype=torch.int32).cuda(), 1, 4)       # C % 8 != 0


@pytest.mark.parametrize("cams,views", [(6, 0), (3, 2)])
def test_assemble_tokens_sie(V, cams, views):
    B, T, C, coef = 5, 13, 64, 3.0
    g = torch.Generator().manual_seed(cams * 10 + views)
    n_sie = cams * views if views else cams
    pe = torch.randn(B * (T - 1), C, generator=g).to(bf16)
    cls, pos, sie = torch.randn(C, generator=g), torch.randn(T, C, generator=g), torch.randn(n_sie, C, generator=g)
    cam = torch.randint(0, cams, (B,), generator=g)
    view = torch.randint(0, views, (B,), generator=g) if views else None
    idx = R.sie_index(cam, view, cams, views)
    base = torch.cat((cls.expand(B, 1, C), pe.float().reshape(B, T - 1, C)), 1) + pos
    ref = base + coef * sie[idx][:, None, :]
    x = V.assemble_tokens_sie(pe.cuda(), cls.cuda(), pos.cuda(), sie.cuda(), idx.to(torch.int32).cuda(), coef, B, T)
    close(x, ref.reshape(B * T, C), abs_frac=1e-6)
    assert float((ref - base).abs().max()) > 0.5                                        # the term is not lost in the tolerance
    # one out-of-range index adds nothing to its row (and is never dereferenced)
    for bad in (n_sie, -1, 1 << 30):
        idx2 = idx.clone(); idx2[2] = bad
        ref2 = ref.clone(); ref2[2] = base[2]
        x2 = V.assemble_tokens_sie(pe.cuda(), cls.cuda(), pos.cuda(), sie.cuda(), idx2.to(torch.int32).cuda(), coef, B, T)
        close(x2, ref2.reshape(B * T, C), abs_frac=1e-6)
        assert torch.equal(x2.cpu().reshape(B, T, C)[2], V.assemble_tokens(pe.cuda(), cls.cuda(), pos.cuda(), B, T).cpu().reshape(B, T, C)[2])


@pytest.mark.parametrize("T", [5, 13])
def test_sie_grad(V, T):
    B, C, n_sie, coef = 7, 64, 6, 3.0
    idx = torch.tensor([2, 0, 2, 5, 0, 2, 1], dtype=torch.int32)
    dx = torch.randn(B * T, C, generator=torch.Generator().manual_seed(T)).to(bf16)
    ref = torch.zeros(n_sie, C, dtype=torch.float64)
    ref.index_add_(0, idx.long(), dx.double().reshape(B, T, C).sum(1))
    ref *= coef
    got = V.sie_grad(dx.cuda(), idx.cuda(), n_sie, coef, B, T)
    again = V.sie_grad(dx.cuda(), idx.cuda(), n_sie, coef, B, T)
    np.testing.assert_allclose(got.cpu().numpy(), ref.numpy(), rtol=1e-5, atol=1e-5)
    assert torch.equal(got, again)                                                       # fixed order: bit-identical run to run
    assert float(got[3].abs().max()) == 0.0 and float(got[4].abs().max()) == 0.0         # rows no sample uses
    assert float(got[2].abs().max()) > 0.0


@pytest.mark.parametrize("B,T,H", [(8, 3, 2), (4, 33, 12), (3, 50, 2), (2, 53, 12), (2, 64, 1)])
def test_attention_fwd_short(V, B, T, H):
    """test_attention_fwd_bwd's forward and lse checks, same tolerances, on the 4-tile instance."""
    g = torch.Generator().manual_seed(B * 1000 + T + H)
    C = H * 64
    qkv = torch.randn(B * T, 3 * C, generator=g).to(bf16)
    t = qkv.float().reshape(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)                       # vit_pytorch.py:155
    q, k, v = t[0], t[1], t[2]
    s = (q @ k.transpose(-2, -1)) * 0.125
    out = (s.softmax(dim=-1) @ v).transpose(1, 2).reshape(B * T, C)
    ok, lse = V.attention_fwd_short(qkv.cuda(), B, T, H)
    close(ok, out, abs_frac=4e-3)
    np.testing.assert_allclose(lse.cpu().numpy(), torch.logsumexp(s, dim=-1).reshape(B * H, T).numpy(), rtol=1e-4, atol=1e-4)
    o13, lse13 = V.attention_fwd(qkv.cuda(), B, T, H)
    print("attention_fwd_short (%d, %d, %d): bitwise equal to attention_fwd: out %s, lse %s" % (B, T, H, torch.equal(ok, o13), torch.equal(lse, lse13)))


def test_attention_fwd_short_refuses_65_tokens(V):
    from daliid_amd._lib import DaliError
    with pytest.raises(DaliError):
        V.attention_fwd_short(torch.zeros(65, 192, dtype=bf16).cuda(), 1, 65, 1)


@pytest.mark.parametrize("after", [True, False])
def test_jpm_head(V, after):
    B, C = 3, 768
    g = torch.Generator().manual_seed(11)
    glob, loc = torch.randn(B, C, generator=g), torch.randn(4 * B, C, generator=g)
    gamma, beta = 1.0 + 0.1 * torch.randn(5, C, generator=g), 0.1 * torch.randn(5, C, generator=g)
    rm, rv = 0.5 * torch.randn(5, C, generator=g), 0.5 + torch.rand(5, C, generator=g)
    sd = {}
    for i in range(5):
        name = "bottleneck_%d" % i if i else "bottleneck"
        sd.update({name + ".weight": gamma[i], name + ".bias": beta[i], name + ".running_mean": rm[i], name + ".running_var": rv[i]})
    ref = R.jpm_head([glob] + [loc[i * B:(i + 1) * B] for i in range(4)], sd, after)
    necks = tuple(t.cuda() for t in (gamma, beta, rm, rv)) if after else None
    got = V.jpm_head(glob.cuda(), loc.cuda(), necks).cpu()
    assert got.shape == (B, 5 * C)
    if after:
        np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-5, atol=1e-6)
    else:
        assert torch.equal(got, ref)                                                     # 0.25 is exact


# ---------------------------------------------------------------------------------------------------------------- models
def _case_model(z, name, jpm=True):
    from daliid_amd import make_models
    keys, shapes = [str(k) for k in z[name + "/keys"]], [str(s) for s in z[name + "/shapes"]]
    if name == "train":
        H, W, stride, depth, cams, views, coef, neck = 48, 48, 16, 2, 3, 2, 3.0, "after"
    else:
        H, W, stride, depth, cams, views, _ = (int(v) for v in z[name + "/geom"])
        coef, neck = float(z[name + "/coef"]), str(z[name + "/neck_feat"])
    model = make_models.make_model(_cfg((H, W), stride, jpm, cams > 1, views > 1, coef, neck), 10, cams, views, depth=depth)
    assert list(model.state_dict().keys()) == keys                                       # the reference's keys, same order
    for (k, v), shp in zip(model.state_dict().items(), shapes):
        assert str(tuple(v.shape)) == shp, k
    model.load_state_dict(R.seeded_state(keys, shapes))
    return model


@pytest.mark.parametrize("name,n_keys", [("A", 210), ("B", 211), ("C", 91)])
def test_jpm_model_matches_reference_outputs(z, name, n_keys):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    assert len(z[name + "/keys"]) == n_keys
    model = _case_model(z, name).eval()
    H, W, seed = int(z[name + "/geom"][0]), int(z[name + "/geom"][1]), int(z[name + "/geom"][6])
    x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(seed))
    cam, view = (z[name + "/cam"] if len(z[name + "/cam"]) else None), (z[name + "/view"] if len(z[name + "/view"]) else None)
    with torch.no_grad():
        y = model(x.cuda(), cam_label=cam, view_label=view).cpu()
    ref = torch.from_numpy(z[name + "/y"])
    assert y.shape == ref.shape == (2, 3840)
    errs = [R.rel_l2(y[:, i * 768:(i + 1) * 768], ref[:, i * 768:(i + 1) * 768]) for i in range(5)]
    print("JPM case %s: rel-L2 of (global, l1, l2, l3, l4) vs the fp32 reference: %s" % (name, " ".join("%.3e" % e for e in errs)))
    assert max(errs) < 2e-2, errs


def test_jpm_global_slice_is_the_plain_model_bit_for_bit():
    """b1 = a copy of the last block + final norm on the same B*T rows through the same kernels: with the plain model's weights in base.*, b1.* and
    the neck, the first 768 columns equal the plain model's output exactly."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from daliid_amd import make_models
    plain = make_models.make_model(_cfg((256, 128), 16, False), 10, 0, 0, seed=5)
    jpm = make_models.make_model(_cfg((256, 128), 16, True), 10, 0, 0, seed=6)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        plain.bottleneck.running_mean.copy_(0.3 * torch.randn(768, generator=g))
        plain.bottleneck.running_var.copy_(0.5 + torch.rand(768, generator=g))
        plain.bottleneck.weight.copy_(1.0 + 0.1 * torch.randn(768, generator=g))
        plain.bottleneck.bias.copy_(0.1 * torch.randn(768, generator=g))
        for p in plain.base.parameters():
            p.add_((0.02 * torch.randn(p.shape, generator=g)).to(p.device))
    plain.mark_weights_changed()
    src, sd = plain.state_dict(), dict(jpm.state_dict())
    for k, v in src.items():
        sd[k] = v
        if k.startswith("base.blocks.11."):
            sd["b1.0." + k[len("base.blocks.11."):]] = v
        elif k.startswith("base.norm."):
            sd["b1.1." + k[len("base.norm."):]] = v
    jpm.load_state_dict(sd)
    plain.eval(); jpm.eval()
    x = torch.randn(2, 3, 256, 128, generator=g).cuda()
    with torch.no_grad():
        a, b = plain(x), jpm(x)
    assert b.shape == (2, 3840) and torch.equal(b[:, :768], a)
    assert float(b[:, 768:].abs().max()) > 0


def test_transreid_local_feature_tokens(z):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from daliid_amd import vit_pytorch as VP
    net = VP.TransReID(img_size=(48, 48), patch_size=16, stride_size=16, embed_dim=768, depth=2, num_heads=12, mlp_ratio=4, qkv_bias=True,
                       camera=3, view=2, sie_xishu=3.0, local_feature=True, num_classes=1000)
    keys, shapes = [str(k) for k in z["C/keys"]], [str(s) for s in z["C/shapes"]]
    full = R.seeded_state(keys, shapes)
    net.load_state_dict({k[len("base."):]: v for k, v in full.items() if k.startswith("base.")})
    x = torch.randn(2, 3, 48, 48, generator=torch.Generator().manual_seed(int(z["C/geom"][6])))
    net.eval()
    with torch.no_grad():
        tok = net(x.cuda(), cam_label=z["C/cam"], view_label=z["C/view"]).cpu()
    ref = torch.from_numpy(z["C/tokens"])
    assert tok.shape == ref.shape == (2, 10, 768)
    e = R.rel_l2(tok, ref)
    print("local_feature tokens of case C: rel-L2 %.3e" % e)
    assert e < 2e-2
    net.train()
    with pytest.raises(NotImplementedError):
        net(x.cuda(), cam_label=z["C/cam"], view_label=z["C/view"])


def test_sie_training_output_and_gradient(z):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    model = _case_model(z, "train", jpm=False)
    g = torch.Generator().manual_seed(int(z["train/seed"]))
    x = torch.randn(6, 3, 48, 48, generator=g)
    w = torch.randn(6, 768, generator=g)
    cam, view = torch.from_numpy(z["train/cam"]), torch.from_numpy(z["train/view"])
    model.train()
    y = model(x.cuda(), cam_label=cam, view_label=view)
    (y * w.cuda()).sum().backward()
    e_y = R.rel_l2(y.detach().cpu(), torch.from_numpy(z["train/y"]))
    grad, ref = model.base.sie_embed.grad.cpu(), torch.from_numpy(z["train/sie_grad"])
    e_g = R.rel_l2(grad, ref)
    print("SIE train step: feat rel-L2 %.3e, sie_embed.grad rel-L2 %.3e" % (e_y, e_g))
    assert grad.shape == ref.shape == (6, 1, 768)
    assert e_y < 3e-2 and e_g < 8e-2
    used = set((cam * 2 + view).tolist())
    assert used == {0, 2, 3, 5}
    for i in range(6):
        assert (float(grad[i].abs().max()) > 0) == (i in used), i                        # rows of unused (camera, view) pairs: exactly 0
    for name, p in model.named_parameters():
        if name.startswith("base.fc.") or name == "bottleneck.bias":
            continue
        assert p.grad is not None and float(p.grad.abs().max()) > 0, name


def test_extract_features_and_validate_pass_sie_labels(z):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from daliid_amd import getFeatures, validateModels
    model = _case_model(z, "C").eval()
    g = torch.Generator().manual_seed(21)
    images = torch.randn(10, 3, 48, 48, generator=g)
    records = np.array([["img%02d" % i, str(i // 2), str(i % 3), "person"] for i in range(10)])
    cams, views = records[:, 2].astype(np.int64), np.arange(10) % 2
    loader = lambda paths, h, w, turb=None: images[[int(p[3:]) for p in paths]]
    getFeatures.set_image_loader(loader)
    try:
        fvs = getFeatures.extractFeatures(records, 48, 48, model, 4, gpu_index=0, keep_on_device=True, verbose=False, cam_labels=cams, view_labels=views)
        with torch.no_grad():
            direct = torch.cat([model(images[b:b + 4].cuda(), cam_label=cams[b:b + 4], view_label=views[b:b + 4]) for b in (0, 4, 8)], 0)
            other = model(images[:4].cuda(), cam_label=(cams[:4] + 1) % 3, view_label=views[:4])
        assert fvs.shape == (10, 3840) and torch.equal(fvs, direct)
        assert not torch.equal(other, direct[:4])                                        # the labels reach the model
        validator = validateModels.validationManager.getValidator("Market")
        validator.setParameters(48, 48, False, 0)
        validator.setSIE(cam_label_of=lambda s: s[:, 2].astype(np.int64), view_label_of=lambda s: np.array([int(r[0][3:]) % 2 for r in s]))
        # every identity once in the queries and once, under another camera, in the gallery
        cmc, mAP, distmat = validator.validate(records[::2], records[1::2], model)
        assert tuple(distmat.shape) == (5, 5) and bool(torch.isfinite(distmat).all()) and 0.0 <= mAP <= 1.0
        with torch.no_grad():
            fq = model(images[::2].cuda(), cam_label=cams[::2], view_label=views[::2])
            fg = model(images[1::2].cuda(), cam_label=cams[1::2], view_label=views[1::2])
        assert fq.shape == (5, 3840) and torch.equal(distmat, validator.distance(fq, fg))
    finally:
        getFeatures.set_image_loader(None)


@pytest.mark.parametrize("cfg_tuple,sizes", [((6, 64, 32, 16, 16, 128, 2, 2, 512, 10), (498112, 256, 3680768, 128, 34, 2)),
                                              ((3, 32, 32, 8, 8, 64, 3, 1, 256, 10), (164416, 128, 1437696, 64, 46, 2))])
def test_plain_plan_sizes_are_those_before_the_ext(cfg_tuple, sizes):
    """dali_vit_create (= create_ex with a zeroed ext): parameter elements, buffer elements, arena bytes, feature width and table lengths of two
    plain geometries, as the library gave them before dali_vit_ext existed (numbers taken from that build)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import ctypes
    from daliid_amd import _lib
    from daliid_amd.vit_pytorch import _VitCfg, _VitPlan
    h, cfg = ctypes.c_void_p(), _VitCfg(*cfg_tuple)
    _lib.check(_lib.lib().dali_vit_create(_lib.ctx(0), ctypes.byref(cfg), ctypes.byref(h)), "dali_vit_create")
    try:
        got = [ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()]
        _lib.check(_lib.lib().dali_vit_sizes(h, *[ctypes.byref(v) for v in got]), "dali_vit_sizes")
        assert tuple(v.value for v in got) == sizes
    finally:
        _lib.lib().dali_vit_destroy(h)
    ex = _VitPlan(torch.device("cuda", 0), cfg_tuple)                                    # what the Python side calls: create_ex, nothing set
    assert (ex.param_elems, ex.buffer_elems, ex.arena_bytes, ex.feat_dim, ex.n_params, ex.n_buffers) == sizes


def test_plan_takes_the_host_token_map_and_checks_it():
    """The plan has no shuffle of its own: it runs the map make_models.jpm_token_map computed, and refuses one that is missing or points outside
    the patch tokens."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from daliid_amd._lib import DaliError
    from daliid_amd.make_models import jpm_token_map
    from daliid_amd.vit_pytorch import _VitPlan
    dev, cfg_tuple = torch.device("cuda", 0), (2, 64, 48, 16, 16, 128, 2, 2, 512, 10)       # 4 x 3 = 12 patches
    good = jpm_token_map(12, 8, 4, 4, True)
    plan = _VitPlan(dev, cfg_tuple, dict(jpm=1, token_map=good, neck_after=1, id_classes=10))
    assert plan.feat_dim == 5 * 128 and [t[0] for t in plan.tensor_table(1)][-1] == "bottleneck_4.running_var"
    for bad in (None, np.zeros((4, 3), np.int32), np.full((4, 3), 13, np.int32)):
        with pytest.raises(DaliError, match="token_map"):
            _VitPlan(dev, cfg_tuple, dict(jpm=1, divide=4, token_map=bad, neck_after=1, id_classes=10))


def test_a_different_token_map_changes_only_the_local_slices(z):
    """groups = 4, shift = 8 against groups = 2, shift = 5 on the same weights and input (256x128: 128 patches divide by both): the global slice is
    untouched bit for bit, every local slice changes, and each output is within the models' bound of the fp32 restatement run with its own map."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from daliid_amd import make_models
    x = torch.randn(2, 3, 256, 128, generator=torch.Generator().manual_seed(9))
    outs = {}
    for groups, shift in ((2, 5), (4, 8)):
        model = make_models.make_model(_cfg((256, 128), 16, True, groups=groups, shift=shift), 10, 0, 0, depth=2, seed=4).eval()
        sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        with torch.no_grad():
            y = model(x.cuda()).cpu()
        ref = R.jpm_forward(sd, x, 12, 16, shift, groups, True, True)
        errs = [R.rel_l2(y[:, i * 768:(i + 1) * 768], ref[:, i * 768:(i + 1) * 768]) for i in range(5)]
        print("token map (groups %d, shift %d): rel-L2 vs the fp32 restatement %s" % (groups, shift, " ".join("%.3e" % e for e in errs)))
        assert max(errs) < 2e-2, errs
        outs[(groups, shift)] = y
    a, b = outs[(2, 5)], outs[(4, 8)]
    assert torch.equal(a[:, :768], b[:, :768])
    for i in range(1, 5):
        assert not torch.equal(a[:, i * 768:(i + 1) * 768], b[:, i * 768:(i + 1) * 768]), i


def test_load_param_round_trip(z, tmp_path):
    """load_param takes a file saved from an nn.DataParallel wrapper (``module.`` names), load_param_finetune the plain names; both fill every
    entry, change the next forward, and refuse a name the model does not have."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    src = _case_model(z, "C").eval()
    saved = {k: v.detach().cpu().clone() for k, v in src.state_dict().items()}
    torch.save({"module." + k: v for k, v in saved.items()}, str(tmp_path / "wrapped.pth"))
    torch.save(saved, str(tmp_path / "plain.pth"))
    torch.save(dict(saved, **{"no.such.weight": torch.zeros(1)}), str(tmp_path / "odd.pth"))
    x = torch.randn(2, 3, 48, 48, generator=torch.Generator().manual_seed(3)).cuda()
    lab = dict(cam_label=[0, 2], view_label=[1, 0])
    with torch.no_grad():
        want = src(x, **lab)
    for fname, method in (("wrapped.pth", "load_param"), ("plain.pth", "load_param_finetune")):
        from daliid_amd import make_models
        dst = make_models.make_model(_cfg((48, 48), 16, True, True, True), 10, 3, 2, depth=2, seed=1).eval()
        with torch.no_grad():
            before = dst(x, **lab)
        getattr(dst, method)(str(tmp_path / fname))
        for k, v in dst.state_dict().items():
            assert torch.equal(v.cpu(), saved[k]), k
        with torch.no_grad():
            assert torch.equal(dst(x, **lab), want) and not torch.equal(before, want)
        with pytest.raises(KeyError):
            dst.load_param_finetune(str(tmp_path / "odd.pth"))


def test_refusals(z):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from daliid_amd import make_models
    from daliid_amd._lib import DaliError
    model = _case_model(z, "C")
    x = torch.zeros(2, 3, 48, 48).cuda()
    model.train()
    with pytest.raises(NotImplementedError, match="eval only"):
        model(x, cam_label=[0, 1], view_label=[0, 0])
    model.eval()
    with pytest.raises(DaliError):
        model(x)                                                                          # SIE model without labels
    with pytest.raises(DaliError):
        model(x, cam_label=[0, 3], view_label=[0, 0])                                     # camera 3 of 3
    with pytest.raises(DaliError):
        make_models.make_model(_cfg((256, 128), 12, True, groups=4), 10, 0, 0, depth=1)  # 210 patches, 4 shuffle groups: the reference raises
    # a local_feature base without the JPM head has tokens and nothing else (vit_pytorch.py:393-396): no neck output, no cls feature
    from daliid_amd import vit_pytorch as VP
    net = VP.ViTNeckNet(img_size=(48, 48), embed_dim=128, depth=2, num_heads=2, local_feature=True).eval()
    with pytest.raises(DaliError, match="local_feature"):
        net(x)
    with pytest.raises(DaliError, match="local_feature"):
        net.global_feat(x)
    assert tuple(net.local_tokens(x).shape) == (2, 10, 128)
    import ctypes
    from daliid_amd import _lib
    plan, feat = net._plan(2), torch.full((2, 128), 7.0, device="cuda")
    rc = _lib.lib().dali_vit_forward_ex(plan.h, _lib.stream_ptr(), _lib.ptr(x), None, 0, _lib.ptr(feat), None, None)
    assert rc != 0 and "tokens_out" in _lib.last_error() and bool((feat == 7.0).all())   # refused, nothing written
