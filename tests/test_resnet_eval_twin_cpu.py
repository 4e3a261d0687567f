"""The sensitivity table of tests/test_gpu_resnet_eval_plan.py, on the CPU (the sibling of tests/test_resnet_twin_cpu.py).

A small ResNet50ReID (width 64, layers (1, 1, 1, 1), 16 images of 64 x 32) is run by an explicit fp32 twin of the plan's INFERENCE forward
(daliid_amd/csrc/resnet_plan.hip: stem_forward, block_forward with training = 0) that keeps every tensor the plan stores, in the plan's layouts:
the stem (bf16 of the convolution, bn1 without a ReLU, the 3x3 / 2 maximum over real positions), layer1.0 as the FOLDED block ([a2 | x] against the
split hi + lo image and the summed shift), layer2.0 as the un-folded downsample block (rawd stored, res_scale / bias in conv3's output stage),
layer3.0 and layer4.0 likewise, the head and the neck.  (1) Without a defect it is oracle.resnet50_bf16.forward_matched(training=False) bit for
bit, and every check of the GPU test passes on its tensors -- the same functions of tests/resnet_checks.py, so their references and bounds are
exercised here.  (2) Eight single wiring defects are planted one at a time.  For each: (a) the quantity the GPU test checks at the defective op,
fed the clean run's stored operands (that test never chains errors), must move by at least 3 x its bound, and the GPU test's own check must
refuse it; (b) how far the embedding moves beside the end-to-end bound of tests/test_gpu_e2e_parity.py (HIP_TWIN_EVAL_EMB = 4e-3): the defects
that stay inside it are the gap the op-by-op test closes."""
import pytest
import torch
import torch.nn.functional as F

from oracle import resnet50_bf16 as M
from resnet_checks import (eval_check_block, eval_check_head, eval_check_stem, eval_conv_act, eval_stem_pool, eval_y, eval_y_folded, rel_l2, stem_conv,
                           stored_bound)
from test_gpu_plan_only import random_oracle_net
from test_gpu_resnet_plan import geometry

bf16 = torch.bfloat16
Q = lambda t: t.to(bf16).float()
HIP_TWIN_EVAL_EMB = 4e-3                     # tests/test_gpu_e2e_parity.py
CFG = dict(width=64, layers=(1, 1, 1, 1), N=16, H=64, W=32)
N_CUS = 16                                   # the device on which 2048 pixels are 2 tiles of 128 x 128 per CU: there the plan folds layer1.0 at this size
FOLDED, BRANCH = 0, 1                        # block indices: layer1.0 (folded), layer2.0 (the un-folded downsample block under test)


def v4(c):
    return c.view(1, -1, 1, 1)


def nhwc16(t):
    return t.permute(0, 2, 3, 1).contiguous().to(bf16)


def pool_twin(z, defect):
    """the 3x3 / stride 2 / pad 1 maximum over the real positions of a window (the plan's kernels clamp or gate what lies outside)"""
    N, C, H, W = z.shape
    pad = 0.0 if defect == "pool_pads_with_0" else float("-inf")
    cols = F.unfold(F.pad(z, (1, 1, 1, 1), value=pad), 3, stride=2).view(N, C, 9, H // 2, W // 2).clone()
    if defect == "pool_last_column_window_one_short":
        cols[:, :, [2, 5, 8], :, -1] = float("-inf")
    return cols.max(2).values


def eval_twin(ref, img, defect=None):
    """-> (t, emb): every stored tensor by the plan's debug name in the plan's layout, and the embedding.  The order of the fp32 operations is
    forward_matched's (the output stage adds its terms in another order: within the roundings the GPU test's bounds count)."""
    t = {}
    co = M._bn_eval_coeffs
    with torch.no_grad():
        N, _, H, W = img.shape
        wb = ref.conv1.out_channels
        x = Q(img)
        ximg = torch.zeros(N, H + 6, W + 8, 4, dtype=bf16)
        ximg[:, 3:3 + H, 3:3 + W, :3] = nhwc16(x)
        w_stem = torch.zeros(wb, 7, 8, 4, dtype=bf16)
        w_stem[:, :, :7, :3] = nhwc16(ref.conv1.weight)
        s, h = co(ref.bn1)
        raw0 = Q(M._conv(x, ref.conv1))
        x = Q(pool_twin(raw0 * v4(s) + v4(h), defect))
        t.update({"ximg": ximg, "w_stem": w_stem, "raw0": nhwc16(raw0), "pool0": nhwc16(x), "bn1.scale": s, "bn1.shift": h})
        blocks = [b for l in (ref.layer1, ref.layer2, ref.layer3, ref.layer4) for b in l]
        for i, blk in enumerate(blocks):
            b = "block%d." % i
            here = i == BRANCH
            cf = {"1": co(blk.bn1), "2": co(blk.bn2), "3": co(blk.bn3), "d": co(blk.downsample[1])}
            convs = {"1": blk.conv1, "2": blk.conv2, "3": blk.conv3, "d": blk.downsample[0]}
            for k in cf:
                t[b + "bn%s.scale" % k], t[b + "bn%s.shift" % k] = cf[k]
                t[b + "conv%s.w" % k] = nhwc16(convs[k].weight)
            k1 = cf["2"] if defect == "bn2_coefficients_in_conv1" and here else cf["1"]
            z1 = M._conv(x, blk.conv1) * v4(k1[0]) + v4(k1[1])
            a1 = F.relu(z1)
            if defect == "a1_relu_skipped_on_4_channels" and here:
                a1 = torch.cat((z1[:, :4], a1[:, 4:]), 1)
            a1 = Q(a1)
            a2 = Q(F.relu(M._conv(a1, blk.conv2) * v4(cf["2"][0]) + v4(cf["2"][1])))
            (s3, h3), (sd, hd) = cf["3"], cf["d"]
            if i == FOLDED:
                assert M.cat_eval_supported(blk, a2.shape[0] * a2.shape[2] * a2.shape[3], N_CUS)
                img_parts, folded = [], []
                for sc, conv in ((s3, blk.conv3), (sd, blk.downsample[0])):
                    v = sc.view(-1, 1, 1, 1) * conv.weight                                   # from the fp32 master weights (fold_cat_weights_kernel)
                    hi = Q(v)
                    lo = Q(v - hi)
                    img_parts += [hi.flatten(1), lo.flatten(1)]
                    folded.append(hi if defect == "folded_image_without_low_halves" else hi + lo)
                shcat = h3 + hd
                used = shcat
                if defect == "summed_shift_without_the_branch":
                    used = h3
                elif defect == "summed_shift_without_the_branch_on_4_channels":
                    used = torch.cat((h3[:4], shcat[4:]))
                y = Q(F.relu(F.conv2d(a2, folded[0]) + F.conv2d(x, folded[1]) + v4(used)))
                t[b + "wcat"], t[b + "shcat"] = torch.cat(img_parts, 1).to(bf16), shcat
            else:
                rawd = Q(M._conv(x, blk.downsample[0]))
                rs = s3 if defect == "bn3_scale_as_res_scale" and here else sd
                y = Q(F.relu((M._conv(a2, blk.conv3) * v4(s3) + v4(h3)) + (rawd * v4(rs) + v4(hd))))
                t[b + "rawd"] = nhwc16(rawd)
            t.update({b + "a1": nhwc16(a1), b + "a2": nhwc16(a2), b + "y": nhwc16(y)})
            x = y
        f = x.mean((2, 3)) + F.adaptive_max_pool2d(x, 1).flatten(1)
        sn, hn = co(ref.last_bn)
        emb = f * sn.view(1, -1) + hn.view(1, -1)
        t["feat"] = f
    return t, emb


@pytest.fixture(scope="module")
def case():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    ref = random_oracle_net(CFG["layers"], CFG["width"], 61)
    ref.eval()
    img = torch.randn(CFG["N"], 3, CFG["H"], CFG["W"], generator=torch.Generator().manual_seed(62))
    t, emb = eval_twin(ref, img)
    return ref, img, t, emb


def test_explicit_twin_is_forward_matched(case, monkeypatch):
    """the same fp32 operations in the same order: equal bit for bit (forward_matched folds layer1.0 where a 256-CU device does; here it is asked
    as on a 16-CU device, where this batch fills the persistent kernel)"""
    ref, img, t, emb = case
    orig = M.cat_eval_supported
    monkeypatch.setattr(M, "cat_eval_supported", lambda blk, n_pixels: orig(blk, n_pixels, N_CUS))
    with torch.no_grad():
        want = M.forward_matched(ref, img, training=False)
    assert orig(ref.layer1[0], 2048, N_CUS) and not orig(ref.layer1[0], 2048)
    assert torch.equal(emb, want), rel_l2(emb, want)
    monkeypatch.setattr(M, "cat_eval_supported", lambda blk, n_pixels: False)
    with torch.no_grad():
        unfolded = M.forward_matched(ref, img, training=False)
    e = rel_l2(unfolded, want)
    print("\nexplicit eval twin == forward_matched(training=False) bit for bit; folded against un-folded layer1.0: embedding rel-L2 %.2e" % e)
    assert 0 < e < HIP_TWIN_EVAL_EMB                    # the fold is another rounding of the same function, not the same bits


def test_clean_twin_passes_every_check_of_the_gpu_test(case):
    """the references and bounds of tests/resnet_checks.py on a correctly wired forward in fp32 torch arithmetic: every ratio <= 1"""
    ref, img, t, emb = case
    geo = geometry(CFG)
    report = {}
    n_neg = eval_check_stem(t, report, "un-fused stem ")
    fused = {k: v for k, v in t.items() if k != "raw0"}
    eval_check_stem(fused, report, "fused stem ")
    x = t["pool0"]
    for i, g in enumerate(geo):
        x = eval_check_block(t, i, g, x, report, g["name"] + " ")
    neck = (ref.last_bn.weight.detach(), ref.last_bn.bias.detach(), ref.last_bn.running_mean, ref.last_bn.running_var)
    eval_check_head(x, t["feat"], emb, "both", neck, report)
    print("\nclean twin, worst error / bound per op kind: " + ", ".join("%s %.3g" % kv for kv in sorted(report.items())))
    print("border windows of pool0 (x channels) with a negative maximum: %d" % n_neg)
    assert set(report) == {"raw0", "pool0", "a1", "a2", "y folded", "rawd", "y branch", "feat both"} and max(report.values()) <= 1.0


DEFECTS = ["folded_image_without_low_halves", "summed_shift_without_the_branch", "summed_shift_without_the_branch_on_4_channels",
           "bn2_coefficients_in_conv1", "bn3_scale_as_res_scale", "a1_relu_skipped_on_4_channels", "pool_pads_with_0",
           "pool_last_column_window_one_short"]


def op_quantity(defect, t):
    """(debug name of the tensor at the defective op, what the GPU test calls it, (ref, E) from the CLEAN run's stored operands)"""
    geo = geometry(CFG)
    if defect in ("folded_image_without_low_halves", "summed_shift_without_the_branch", "summed_shift_without_the_branch_on_4_channels"):
        return "block0.y", "y folded", eval_y_folded(t["block0.a2"], t["pool0"], t["block0.wcat"], t["block0.shcat"])
    b, x = "block%d." % BRANCH, t["block%d.y" % (BRANCH - 1)]
    if defect in ("bn2_coefficients_in_conv1", "a1_relu_skipped_on_4_channels"):
        return b + "a1", "a1", eval_conv_act(x, t[b + "conv1.w"], 1, 0, t[b + "bn1.scale"], t[b + "bn1.shift"])
    if defect == "bn3_scale_as_res_scale":
        return b + "y", "y branch", eval_y(t[b + "a2"], t[b + "conv3.w"], t[b + "bn3.scale"], t[b + "bn3.shift"], t[b + "rawd"], t[b + "bnd.scale"],
                                           t[b + "bnd.shift"])
    if defect in ("pool_pads_with_0", "pool_last_column_window_one_short"):
        u, Eacc = stem_conv(t["ximg"], t["w_stem"])
        return "pool0", "pool0", eval_stem_pool(u, Eacc, t["bn1.scale"], t["bn1.shift"])[:2]
    raise AssertionError(defect)


def gpu_check_refuses(name, t_bad):
    """does the walk of tests/test_gpu_resnet_eval_plan.py fail on these tensors?  (the fused stem's form: no raw0)"""
    geo = geometry(CFG)
    try:
        if name == "pool0":
            eval_check_stem({k: v for k, v in t_bad.items() if k != "raw0"}, {})
        else:
            i = int(name[5:name.index(".")])
            eval_check_block(t_bad, i, geo[i], t_bad["pool0"] if i == 0 else t_bad["block%d.y" % (i - 1)], {})
    except AssertionError:
        return True
    return False


def measure(case, defect):
    ref, img, t, emb = case
    t_bad, emb_bad = eval_twin(ref, img, defect)
    name, kind, (qref, E) = op_quantity(defect, t)
    # the defect sits in one op: everything in front of it is the clean run's, bit for bit
    for k in t:
        if k == name:
            break
        if k in ("ximg", "w_stem", "raw0", "pool0") or k.endswith((".a1", ".a2", ".y", ".rawd")):
            assert torch.equal(t[k].float(), t_bad[k].float()), (defect, k)
    ratio = float(((t_bad[name].double() - t[name].double()).abs() / stored_bound(qref, E)).max())
    refused = gpu_check_refuses(name, dict(t, **{name: t_bad[name]}))
    return name, kind, ratio, refused, rel_l2(emb_bad, emb)


@pytest.mark.parametrize("defect", DEFECTS)
def test_sensitivity_to_single_defects(case, defect):
    name, kind, ratio, refused, e_emb = measure(case, defect)
    print("\ndefect %-46s op by op: %s (%s) moves %.3g x its bound, check %s | embedding rel-L2 %.2e: %s %.0e" % (
        defect, name, kind, ratio, "refuses" if refused else "PASSES", e_emb, "INSIDE" if e_emb < HIP_TWIN_EVAL_EMB else "outside", HIP_TWIN_EVAL_EMB))
    assert ratio >= 3.0, (defect, name, ratio)
    assert refused, (defect, name)


def test_which_defects_stay_inside_the_end_to_end_bound(case):
    """The gap that the op-by-op test closes: the defects whose embedding stays within HIP_TWIN_EVAL_EMB of the clean one (the end-to-end test
    compares against the rounding-matched twin at that bound).  The table is printed; what is asserted is that the set is not empty."""
    inside = [d for d in DEFECTS if measure(case, d)[-1] < HIP_TWIN_EVAL_EMB]
    print("\ninside the end-to-end bound %.0e: %s" % (HIP_TWIN_EVAL_EMB, inside))
    assert inside, "no planted defect stays inside the end-to-end bound at these shapes"
