"""The rounding-matched ViT twin (oracle/vit_bf16.py) on the CPU: (1) with rounding switched off its explicit backward IS the calculus of
oracle/vit.py (autograd, fp32 roundoff); (2) with rounding on, how far it sits from fp32 per quantity family; (3) the sensitivity table: each of
six single wiring defects must move at least one quantity of tests/test_gpu_vit_plan.py's block-by-block comparison by 3x that family's bound,
and how far the same defect moves the quantities the whole-net tests (tests/test_gpu_vit.py: 8e-2 on weights, 0.15 on biases) look at."""
import pytest
import torch

from oracle import vit as OV
from oracle import vit_bf16 as TW
from test_gpu_vit_plan import BOUND_B, BOUND_DX, BOUND_LN, BOUND_W

HEADS, PATCH = 2, 16
SMALL = dict(hw=(64, 32), stride=16, B=3, dim=128, depth=3, mlp=512)          # 9 tokens
NET_B = dict(hw=(256, 128), stride=12, B=4, dim=128, depth=3, mlp=512)        # 211 tokens, 844 rows: net B of the GPU test


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp(min=1e-30))


def make_state(cfg, seed):
    """a reference-keyed state dict at the GPU tests' scale: truncated-normal 0.02 weights, LayerNorm weights 1, biases 0, everything + 0.05 randn"""
    g = torch.Generator().manual_seed(seed)
    C, Hd = cfg["dim"], cfg["mlp"]
    T = ((cfg["hw"][0] - PATCH) // cfg["stride"] + 1) * ((cfg["hw"][1] - PATCH) // cfg["stride"] + 1) + 1
    shapes = {"base.cls_token": (1, 1, C), "base.pos_embed": (1, T, C), "base.patch_embed.proj.weight": (C, 3, PATCH, PATCH),
              "base.patch_embed.proj.bias": (C,), "base.norm.weight": (C,), "base.norm.bias": (C,)}
    for i in range(cfg["depth"]):
        p = "base.blocks.%d." % i
        shapes.update({p + "norm1.weight": (C,), p + "norm1.bias": (C,), p + "attn.qkv.weight": (3 * C, C), p + "attn.qkv.bias": (3 * C,),
                       p + "attn.proj.weight": (C, C), p + "attn.proj.bias": (C,), p + "norm2.weight": (C,), p + "norm2.bias": (C,),
                       p + "mlp.fc1.weight": (Hd, C), p + "mlp.fc1.bias": (Hd,), p + "mlp.fc2.weight": (C, Hd), p + "mlp.fc2.bias": (C,)})
    sd = {}
    for k, shp in shapes.items():
        base = torch.ones(shp) if "norm" in k and k.endswith("weight") else torch.zeros(shp) if k.endswith("bias") else 0.02 * torch.randn(shp, generator=g).clamp(-2, 2)
        sd[k] = base + 0.05 * torch.randn(shp, generator=g)
    x = torch.randn(cfg["B"], 3, *cfg["hw"], generator=g)
    w = torch.randn(cfg["B"], C, generator=g)
    return sd, x, w, g


def scales_of(rate, u, depth):
    """daliid_amd.vit_pytorch.ViTNeckNet._draw_drop_path"""
    keep = 1.0 - torch.linspace(0, rate, depth).repeat_interleave(2).unsqueeze(1)
    return ((keep + u).floor() / keep).contiguous()


def draws(g, depth, B):
    """uniform draws with a dropped and a kept sample in every branch of blocks 1.. (block 0 has rate 0)"""
    u = torch.rand(2 * depth, B, generator=g)
    u[:, 0], u[:, 1] = 0.01, 0.99
    return u


@pytest.mark.parametrize("rate", [0.0, 0.5], ids=["no_droppath", "droppath"])
def test_unrounded_twin_backward_is_autograd(rate):
    cfg = SMALL
    sd, x, w, g = make_state(cfg, 11)
    u = draws(g, cfg["depth"], cfg["B"])
    leaf = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    T = sd["base.pos_embed"].shape[1]
    pos_b = sd["base.pos_embed"].expand(cfg["B"], T, cfg["dim"]).clone().requires_grad_(True)      # one leaf per sample: its gradient is d x0
    fwd_sd = dict(leaf)
    fwd_sd["base.pos_embed"] = pos_b
    gf = OV.transreid_forward(fwd_sd, x, HEADS, PATCH, cfg["stride"], prefix="base.", drop_path=(rate, u) if rate else None)
    (gf * w).sum().backward()
    scales = scales_of(rate, u, cfg["depth"]) if rate else None
    gf_t, grads, dxs = TW.forward_backward(sd, x, w, HEADS, PATCH, cfg["stride"], scales=scales, rounding=False)
    assert rel_l2(gf_t, gf.detach()) < 1e-5
    assert rel_l2(dxs[0], pos_b.grad.reshape(-1, cfg["dim"])) < 1e-5                              # block 0's d x_in
    worst = ("", 0.0)
    for k in sd:
        ref = pos_b.grad.sum(0, keepdim=True) if k == "base.pos_embed" else leaf[k].grad
        e = rel_l2(grads[k], ref)
        worst = max(worst, (k, e), key=lambda t: t[1])
        assert e < 1e-5, (k, e)
    print("unrounded twin vs autograd (rate %.1f): worst rel-L2 %.2e at %s" % (rate, worst[1], worst[0]))


def family(name):
    if name == "dx_in":
        return "dx_in"
    if ".norm" in name:
        return "ln"
    if "blocks" not in name:
        return "tail"
    return "bias" if name.endswith(".bias") else "weight"


BOUNDS = {"dx_in": BOUND_DX, "ln": BOUND_LN, "weight": BOUND_W, "bias": BOUND_B, "tail": 0.0}       # the tail is compared exactly on the GPU


@pytest.fixture(scope="module")
def net_b():
    cfg = NET_B
    sd, x, w, g = make_state(cfg, 12)
    scales = scales_of(0.5, draws(g, cfg["depth"], cfg["B"]), cfg["depth"])
    clean = TW.forward_backward(sd, x, w, HEADS, PATCH, cfg["stride"], scales=scales)
    return cfg, sd, x, w, scales, clean


def test_rounded_twin_distance_from_fp32(net_b):
    """not a check of the kernels: the size of the bf16 rounding noise that a comparison against an fp32 reference has to leave room for"""
    cfg, sd, x, w, scales, (gf, grads, dxs) = net_b
    gf32, g32, dx32 = TW.forward_backward(sd, x, w, HEADS, PATCH, cfg["stride"], scales=scales, rounding=False)
    worst = {}
    for k in grads:
        if k.startswith("base.norm."):
            continue
        f = family(k)
        worst[f] = max(worst.get(f, 0.0), rel_l2(grads[k], g32[k]))
    worst["dx_in"] = max(rel_l2(a, b) for a, b in zip(dxs, dx32))
    print("rounded twin vs fp32, worst rel-L2 per family (whole chain, 844 rows): gf %.2e, %s" % (
        rel_l2(gf, gf32), ", ".join("%s %.2e" % kv for kv in sorted(worst.items()))))
    assert rel_l2(gf, gf32) < 3e-2 and all(v < 0.2 for v in worst.values())      # the twin is the same function up to bf16 noise


DEFECTS = [("1 bias gradients omit the last 4 of 844 rows", ("bias_rows", 1), None),
           ("2 LN1 backward reads x_mid", ("ln1_x_mid", 1), None),
           ("3 LN2 backward uses n1.rstd", ("ln2_rstd", 1), None),
           ("4 attention DropPath factors of block i+1", None, "next"),
           ("5 branch factors exchanged in the backward", None, "swap"),
           ("6 pos_embed gradient omits token 0", ("pos_token0", None), None)]


@pytest.mark.parametrize("case", DEFECTS, ids=lambda c: c[0].split()[0])
def test_sensitivity_to_single_defects(net_b, case):
    """the defect sits in block 1 (or in the tail); the block-by-block test feeds every block the plan's own tensors, so the quantities it would
    see move are block 1's own d x_in and 12 parameter gradients (the tail's four for defect 6)"""
    label, defect, wiring = case
    cfg, sd, x, w, scales, (gf, grads, dxs) = net_b
    bs = None
    if wiring:
        bs = scales.clone()
        if wiring == "next":
            bs[2] = scales[4]
        else:
            bs[2], bs[3] = scales[3], scales[2]
        assert not torch.equal(bs, scales)
    _, gd, dxd = TW.forward_backward(sd, x, w, HEADS, PATCH, cfg["stride"], scales=scales, defect=defect, bwd_scales=bs)
    own = "base.blocks.1." if label[0] != "6" else "base."
    moved = {"dx_in": rel_l2(dxd[1], dxs[1])} if label[0] != "6" else {}
    for k in grads:
        if k.startswith(own) and (label[0] != "6") == ("blocks" in k) and not k.startswith("base.norm."):
            moved[k] = rel_l2(gd[k], grads[k])
    ratios = {k: (v / BOUNDS[family(k)] if BOUNDS[family(k)] else float("inf") if v > 0 else 0.0) for k, v in moved.items()}
    best = max(ratios, key=ratios.get)
    # what the whole-net comparisons of tests/test_gpu_vit.py would see: every weight / norm gradient against 8e-2, every bias against 0.15
    net_w = max(rel_l2(gd[k], grads[k]) for k in grads if not k.endswith(".bias") and not k.startswith("base.norm."))
    net_b_ = max(rel_l2(gd[k], grads[k]) for k in grads if k.endswith(".bias") and not k.startswith("base.norm."))
    print("defect %-46s block test: %s moves %.3e = %.2fx its bound | whole net: weights %.2e (tol 8e-2), biases %.2e (tol 0.15)" % (
        label, best.replace(own, ""), moved[best], min(ratios[best], 1e9), net_w, net_b_))
    assert ratios[best] >= 3.0, (label, moved)


def test_sensitivity_neighbour_factors_one_percent_apart():
    """defect 4 at its smallest: depth 12 at the reference's default rate 0.1, every sample kept, block 10's attention factors taken from block 11
    (1 / 0.9091 against 1 / 0.9: 1 % apart).  The attention branch's gradients of block 10 scale by 1.01"""
    cfg = dict(hw=(64, 32), stride=16, B=6, dim=128, depth=12, mlp=512)
    sd, x, w, g = make_state(cfg, 13)
    scales = scales_of(0.1, torch.full((24, cfg["B"]), 0.9995), 12)
    bs = scales.clone()
    bs[20] = scales[22]
    assert 0.009 < float(bs[20, 0] / scales[20, 0]) - 1 < 0.011
    _, grads, dxs = TW.forward_backward(sd, x, w, HEADS, PATCH, cfg["stride"], scales=scales)
    _, gd, dxd = TW.forward_backward(sd, x, w, HEADS, PATCH, cfg["stride"], scales=scales, bwd_scales=bs)
    own = "base.blocks.10."
    moved = {k: rel_l2(gd[k], grads[k]) for k in grads if k.startswith(own)}
    moved["dx_in"] = rel_l2(dxd[10], dxs[10])
    ratios = {k: v / BOUNDS[family(k)] for k, v in moved.items()}
    best = max(ratios, key=ratios.get)
    net_w = max(rel_l2(gd[k], grads[k]) for k in grads if not k.endswith(".bias") and not k.startswith("base.norm."))
    net_b_ = max(rel_l2(gd[k], grads[k]) for k in grads if k.endswith(".bias") and not k.startswith("base.norm."))
    print("defect %-46s block test: %s moves %.3e = %.2fx its bound | whole net: weights %.2e (tol 8e-2), biases %.2e (tol 0.15)" % (
        "4b neighbour's factors, 1 % apart (depth 12)", best.replace(own, ""), moved[best], ratios[best], net_w, net_b_))
    assert ratios[best] >= 3.0, moved
