"""The ResNet plan's INFERENCE forward (daliid_amd/csrc/resnet_plan.hip: stem_forward / block_forward with training = 0), op by op, from the
plan's own tensors -- the method of tests/test_gpu_resnet_plan.py on the forward that every reported accuracy figure runs through.

That forward is not the training forward with BatchNorm switched off: the stem is one fused launch (stem.hip) or, where that kernel does not
take the shape, implicit GEMM -> raw0 -> the pool kernel; bn1 / bn2 + ReLU ride in the GEMMs' output stages (only a1 / a2 exist); a stride-1
downsample block may be folded into ONE [a2 | x] GEMM against a split hi + lo weight image on the persistent kernel (no rawd, no residual read);
the other downsample blocks read rawd as res_scale * rawd + bias in conv3's output stage; every BatchNorm's coefficients come from the running
statistics in one batched launch.  How these are strung together was checked end to end only (tests/test_gpu_e2e_parity.py, 4e-3 on the
embedding; tests/test_resnet_eval_twin_cpu.py measures what fits inside that).

One eval forward per net; every stored tensor is read back through dali_resnet_debug_tensor and checked against its op applied in fp64 to the
plan's own stored inputs, bf16 weight images and scale / shift vectors (tests/resnet_checks.py: eval_check_stem / eval_check_block /
eval_check_head, the functions the CPU test runs on its twin), so errors never chain.  Bounds are derived (one bf16 store + the fp32
accumulation over the number of products on the sum of magnitudes + the output stage's counted roundings) or the check is exact; none is taken
from the kernels.  The measured error / bound ratios are printed and recorded in docs/experiments.md, "ResNet plan, inference forward op by op".

Nets (Encoders.ResNet50ReID in eval mode, random weights with planted bf16 ties, non-trivial affines and running statistics):
  E1  width 32, layers (1, 1, 1, 1), batch 6 of 96 x 48: 1728 / 432 / 108 / 108 pixels (ragged against every tile; 3-wide maps in layer3 / 4).
      Nothing fused: the stem kernel refuses W = 48 (and 32 channels), so raw0 is written; width 32 fails the fold's 64-channel rule, so
      layer1.0 takes the rawd / res_scale path at stride 1.
  E2  width 64, layers (2, 1, 1, 1), 96 x 32 images, the smallest odd batch N with 192 N >= 128 CUs (171 at 256 CUs): the fused stem; layer1.0
      folded on the persistent kernel, whose last pixel tile is half full; layer1.1 a plain identity block at the same pixel count.
A sentinel planted in raw0 and block0.rawd before the forward shows which of the two ran: E1 overwrites both, E2 leaves both untouched."""
import ctypes
import functools
import time
import types

import pytest
import torch

from resnet_checks import eval_check_block, eval_check_head, eval_check_stem
from test_gpu_plan_only import plan_net, random_oracle_net, weight_image_expectations
from test_gpu_resnet_plan import bits, geometry, same_bits

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
f32 = torch.float32
SENTINEL16 = 0x7FC1                  # a quiet bf16 NaN with a payload, as int16

NETS = {"E1": dict(width=32, layers=(1, 1, 1, 1), N=6, H=96, W=48, seed=71),
        "E2": dict(width=64, layers=(2, 1, 1, 1), N=None, H=96, W=32, seed=72)}
MODES = ("both", "gap", "gmp")


def device_cus():
    """the persistent kernel's grid (conv.hip f1_cu_count), as test_folded_hi_lo_weight_image takes it"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus & ~7 if cus > 8 else 8


def config(name):
    cfg = dict(NETS[name])
    if cfg["N"] is None:
        px = (cfg["H"] // 4) * (cfg["W"] // 4)                                 # 192 pixels per image in layer1
        n = -(-128 * device_cus() // px)                                       # conv_cat_act_supported: 2 channel tiles x P / 128 >= 2 per CU
        cfg["N"] = n | 1                                                       # odd: 192 N = 64 (mod 128), the last pixel tile is half full
        assert px == 192 and px * cfg["N"] >= 128 * device_cus() and (px * cfg["N"]) % 128 == 64
    return cfg


def arena_view(net, name):
    """the plan's tensor `name` in place (int16 view of the arena): debug_tensor hands out copies"""
    ptr, nbytes = ctypes.c_void_p(), ctypes.c_int64()
    net._last_plan.call("debug_tensor", name.encode(), ctypes.byref(ptr), ctypes.byref(nbytes))
    off = ptr.value - net._arena.data_ptr()
    assert 0 <= off and off + nbytes.value <= net._arena.numel()
    return net._arena[off:off + nbytes.value].view(torch.int16)


def has_tensor(net, name):
    from daliid_amd import _lib
    ptr, nbytes = ctypes.c_void_p(), ctypes.c_int64()
    try:
        net._last_plan.call("debug_tensor", name.encode(), ctypes.byref(ptr), ctypes.byref(nbytes))
    except _lib.DaliError:
        return False
    return True


def read_tensors(net, cfg, geo):
    """every tensor the inference forward stores, on the host, by debug name (raw0 / block<i>.rawd whether or not this plan's forward writes them)"""
    N, wb = cfg["N"], cfg["width"]
    get = lambda name, dtype, *shape: net.debug_tensor(name, dtype, shape).cpu()
    t = {"ximg": get("ximg", bf16, N, cfg["H"] + 6, cfg["W"] + 8, 4), "w_stem": get("w_stem", bf16, wb, 7, 8, 4),
         "raw0": get("raw0", bf16, N, cfg["H"] // 2, cfg["W"] // 2, wb), "pool0": get("pool0", bf16, N, cfg["H"] // 4, cfg["W"] // 4, wb),
         "bn1.scale": get("bn1.scale", f32, -1), "bn1.shift": get("bn1.shift", f32, -1), "feat": get("feat", f32, N, -1)}
    for i, g in enumerate(geo):
        b = "block%d." % i
        t[b + "a1"] = get(b + "a1", bf16, N, g["hin"], g["win"], g["w"])
        t[b + "a2"] = get(b + "a2", bf16, N, g["hout"], g["wout"], g["w"])
        t[b + "y"] = get(b + "y", bf16, N, g["hout"], g["wout"], g["cout"])
        convs = (("1", g["w"], 1, g["cin"]), ("2", g["w"], 3, g["w"]), ("3", g["cout"], 1, g["w"])) + ((("d", g["cout"], 1, g["cin"]),) if g["has_ds"] else ())
        for c, co, k, ci in convs:
            t[b + "conv%s.w" % c] = get(b + "conv%s.w" % c, bf16, co, k, k, ci)
            t[b + "bn%s.scale" % c], t[b + "bn%s.shift" % c] = get(b + "bn%s.scale" % c, f32, -1), get(b + "bn%s.shift" % c, f32, -1)
        if g["has_ds"]:
            t[b + "rawd"] = get(b + "rawd", bf16, N, g["hout"], g["wout"], g["cout"])
        if has_tensor(net, b + "wcat"):
            t[b + "wcat"] = get(b + "wcat", bf16, g["cout"], 2 * (g["w"] + g["cin"]))
            t[b + "shcat"] = get(b + "shcat", f32, -1)
    return t


@functools.lru_cache(maxsize=None)
def run(name):
    """one eval forward of net `name` per feature mode; everything the tests read, on the host"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    t0 = time.time()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cfg = config(name)
    geo = geometry(cfg)
    ref = random_oracle_net(cfg["layers"], cfg["width"], cfg["seed"])
    ref.eval()
    net = plan_net(ref, cfg["layers"], cfg["width"])
    net.eval()
    x = torch.randn(cfg["N"], 3, cfg["H"], cfg["W"], generator=torch.Generator().manual_seed(cfg["seed"] + 1))
    xg = x.cuda()
    net._activate(net._plan(cfg["N"], cfg["H"], cfg["W"]))
    for planted in ("raw0", "block0.rawd"):
        arena_view(net, planted).fill_(SENTINEL16)
    torch.cuda.synchronize()
    r = types.SimpleNamespace(net=net, ref=ref, cfg=cfg, geo=geo, x=x, xg=xg, report={}, feat={}, emb={})
    r.emb["both"] = net._run_forward(xg, False).cpu()
    r.t = read_tensors(net, cfg, geo)
    r.feat["both"] = r.t["feat"]
    last = "block%d.y" % (len(geo) - 1)
    y_dev = net.debug_tensor(last, torch.int16, (-1,))
    for mode in MODES[1:]:
        net.feature = mode
        r.emb[mode] = net._run_forward(xg, False).cpu()
        r.feat[mode] = net.debug_tensor("feat", f32, (cfg["N"], -1)).cpu()
        assert torch.equal(net.debug_tensor(last, torch.int16, (-1,)), y_dev), "the trunk's output depends on the feature mode"
    net.feature = "both"
    r.written = {k: not bool((bits(r.t[k]) == SENTINEL16).all()) for k in ("raw0", "block0.rawd")}
    r.untouched = {k: bool((bits(r.t[k]) == SENTINEL16).all()) for k in ("raw0", "block0.rawd")}
    print("\nnet %s (batch %d): forwards + read-back %.1f s" % (name, cfg["N"], time.time() - t0))
    return r


def print_report(name, stage, report):
    print("\nnet %s %s, worst error / bound per op kind: %s" % (name, stage, ", ".join("%s %.3g" % kv for kv in sorted(report.items()))))


# ---------------------------------------------------------------------------------------------------------------------------------------
# which paths ran
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_E1_runs_nothing_fused():
    """E1: the un-fused stem wrote raw0, layer1.0 wrote rawd and has no folded image"""
    from daliid_amd import _lib
    r = run("E1")
    with pytest.raises(_lib.DaliError):
        r.net.debug_tensor("block0.wcat", bf16, (-1,))
    assert "block0.wcat" not in r.t
    assert _lib.lib().dali_stem_fused_supported(r.cfg["N"], r.cfg["H"], r.cfg["W"]) == 0
    assert r.written["raw0"] and bool(torch.isfinite(r.t["raw0"].float()).all()), "raw0 was not written by the un-fused stem"
    assert r.written["block0.rawd"] and bool(torch.isfinite(r.t["block0.rawd"].float()).all()), "layer1.0's rawd was not written"


def test_E2_runs_the_fused_stem_and_the_folded_block():
    """E2: block0.wcat is readable; neither raw0 nor layer1.0's rawd was touched by the forward (the sentinel planted before it is still there:
    the convolution's output never left the stem kernel, the folded GEMM has no branch output); the other downsample blocks are not folded"""
    from daliid_amd import _lib
    r = run("E2")
    g = r.geo[0]
    wcat = r.net.debug_tensor("block0.wcat", bf16, (g["cout"], 2 * (g["w"] + g["cin"])))        # raises if this plan does not fold the block
    assert same_bits(wcat.cpu(), r.t["block0.wcat"])
    assert _lib.lib().dali_stem_fused_supported(r.cfg["N"], r.cfg["H"], r.cfg["W"]) == 1
    assert r.untouched["raw0"], "the fused stem left raw0 alone?"
    assert r.untouched["block0.rawd"], "the folded block left rawd alone?"
    assert [i for i in range(len(r.geo)) if "block%d.wcat" % i in r.t] == [0]
    P = r.cfg["N"] * g["hout"] * g["wout"]
    assert P % 128 == 64 and not r.geo[1]["has_ds"] and r.geo[1]["hout"] * r.geo[1]["wout"] * r.cfg["N"] == P


# ---------------------------------------------------------------------------------------------------------------------------------------
# the walk: images and coefficients (bit for bit), stem, one layer at a time, head
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["E1", "E2"])
def test_operand_images_and_coefficients_bit_for_bit(name):
    """ximg and w_stem from the input and conv1.weight (the packing of test_stem_packing_bit_patterns); every conv's bf16 image and every
    BatchNorm's scale / shift against bn_eval_coeffs of the layer of THAT name (weight_image_expectations): a coefficient vector of another layer
    differs in every element"""
    r = run(name)
    cfg, t = r.cfg, r.t
    N, H, W, wb = cfg["N"], cfg["H"], cfg["W"], cfg["width"]
    want_x = torch.zeros(N, H + 6, W + 8, 4, dtype=bf16)
    want_x[:, 3:3 + H, 3:3 + W, :3] = r.x.permute(0, 2, 3, 1).to(bf16)
    assert same_bits(t["ximg"], want_x), "ximg"
    want_w = torch.zeros(wb, 7, 8, 4, dtype=bf16)
    want_w[:, :, :7, :3] = r.ref.conv1.weight.detach().permute(0, 2, 3, 1).to(bf16)
    assert same_bits(t["w_stem"], want_w), "w_stem"
    exp, _, _ = weight_image_expectations(r.ref)
    bad = [k for k, want in exp.items() if not k.endswith(".wt") and not same_bits(t[k], want)]
    assert not bad, (len(bad), bad[:8])
    assert sum(k.endswith(".scale") for k in exp) == 1 + sum(4 if g["has_ds"] else 3 for g in r.geo)


@pytest.mark.parametrize("name", ["E1", "E2"])
def test_stem_op_by_op(name):
    r = run(name)
    t = r.t if name == "E1" else {k: v for k, v in r.t.items() if k != "raw0"}           # E2's raw0 holds the sentinel: the fused stem's check
    report = {}
    n_neg = eval_check_stem(t, report, "net %s " % name)
    print("\nnet %s: %d border windows x channels of pool0 have a negative maximum" % (name, n_neg))
    print_report(name, "stem", report)


@pytest.mark.parametrize("layer", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["E1", "E2"])
def test_blocks_op_by_op(name, layer):
    """every pixel and channel of a1, a2, rawd and y of the layer's blocks (E2 layer1: the folded block -- the persistent kernel's tile walk with
    its half-full last tile -- and the identity block behind it)"""
    r = run(name)
    report = {}
    for i, g in enumerate(r.geo):
        if g["li"] == layer:
            x = r.t["pool0"] if i == 0 else r.t["block%d.y" % (i - 1)]
            eval_check_block(r.t, i, g, x, report, "net %s %s " % (name, g["name"]))
    want = {"a1", "a2"} | ({"y folded", "y identity"} if (name, layer) == ("E2", 0) else {"rawd", "y branch"})
    assert set(report) == want, sorted(report)
    print_report(name, "layer%d" % (layer + 1), report)


@pytest.mark.parametrize("name", ["E1", "E2"])
def test_head_and_neck_op_by_op(name):
    """feat in the three feature modes from the last y, the embedding from feat and the neck's parameters by its running statistics"""
    r = run(name)
    nk = r.ref.last_bn
    neck = (nk.weight.detach(), nk.bias.detach(), nk.running_mean, nk.running_var)
    report = {}
    y = r.t["block%d.y" % (len(r.geo) - 1)]
    for mode in MODES:
        eval_check_head(y, r.feat[mode], r.emb[mode], mode, neck, report, "net %s " % name)
    assert not same_bits(r.feat["gap"], r.feat["gmp"])
    print_report(name, "head", report)


# ---------------------------------------------------------------------------------------------------------------------------------------
# bit-for-bit properties (E1)
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_two_eval_forwards_are_identical():
    r = run("E1")
    again = r.net._run_forward(r.xg, False).cpu()
    assert same_bits(again, r.emb["both"])


@pytest.mark.parametrize("mode", MODES)
def test_single_whole_map_head_is_the_forward(mode):
    """dali_resnet_forward_heads with one whole-map head of mode m gives dali_resnet_forward's embedding under feature = m"""
    r = run("E1")
    got = r.net.forward_heads(r.xg, [(mode, None)])
    assert tuple(got.shape) == (1,) + tuple(r.emb[mode].shape)
    assert same_bits(got[0].cpu(), r.emb[mode])


def test_train_then_eval_keeps_no_batch_statistic():
    """A training forward leaves batch-statistic coefficients in every BatchNorm's scale / shift and moves the running statistics.  The eval
    forward behind it must agree, on every stored tensor, with a fresh net loaded with the first net's state after that training forward; a
    backward after the eval forward is refused."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from daliid_amd import Encoders, _lib
    cfg = config("E1")
    geo = geometry(cfg)
    ref = random_oracle_net(cfg["layers"], cfg["width"], cfg["seed"] + 10)
    a = plan_net(ref, cfg["layers"], cfg["width"])
    g = torch.Generator().manual_seed(cfg["seed"] + 11)
    x_train = torch.randn(cfg["N"], 3, cfg["H"], cfg["W"], generator=g).cuda()
    x_eval = torch.randn(cfg["N"], 3, cfg["H"], cfg["W"], generator=g).cuda()
    before = a.flat_buffers.clone()
    a.train()
    a._run_forward(x_train, True)
    assert not torch.equal(a.flat_buffers, before), "the training forward did not move the running statistics"
    train_scale = a.debug_tensor("block1.bn2.scale", f32, (-1,)).cpu()
    a.eval()
    emb_a = a._run_forward(x_eval, False).cpu()
    ta = read_tensors(a, cfg, geo)
    assert not same_bits(ta["block1.bn2.scale"], train_scale)
    b = Encoders.ResNet50ReID(layers=cfg["layers"], width=cfg["width"])
    b.load_state_dict(a.state_dict())
    b.eval()
    emb_b = b._run_forward(x_eval, False).cpu()
    tb = read_tensors(b, cfg, geo)
    assert set(ta) == set(tb)
    bad = [k for k in ta if not same_bits(ta[k], tb[k])]
    assert not bad, bad[:8]
    assert same_bits(emb_a, emb_b)
    d_emb = torch.randn(cfg["N"], a.feat_dim, generator=g).cuda()
    with pytest.raises(_lib.DaliError, match="the last forward was not in training mode"):
        a._backward_stage(d_emb, 0)
    torch.cuda.synchronize()
