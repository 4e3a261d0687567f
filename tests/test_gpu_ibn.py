"""GPU: the IBN-a encoders -- dali_ibn_act alone (exact integer data, an offset that separates a centred variance from E[x^2] - mean^2,
random data, batch independence, refusals), the IBN plan (dali_resnet_create_ex: tables, sizes, block wiring, refusals of training) and
the mirror classes ResNet50IBNReID / ResNet101IBNReID (golden output of the reference's wrapper, the rounding-matched twin at full size,
getDCNN, checkpoints, feature extraction).

References: fp64 torch on the same bf16 input for the kernel; tests/ibn_ref.py (checked against tests/golden/ibn.npz on the CPU by
tests/test_ibn_cpu.py) for the nets."""
import io

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ibn_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
EPS = 1e-5


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from daliid_amd import Encoders, _lib, getFeatures, ops_eval, ops_nn, synthetic, validateModels
    return dict(E=Encoders, lib=_lib, GF=getFeatures, ev=ops_eval, nn=ops_nn, syn=synthetic, VM=validateModels)


@pytest.fixture(scope="module")
def gold():
    return load_golden("ibn.npz")


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp(min=1e-30))


def bf16_ulp(v):
    """one bf16 ulp at |v| (fp64 tensor): 2^16 fp32 ulps"""
    return torch.from_numpy(np.spacing(np.abs(v.cpu().numpy()).astype(np.float32)).astype(np.float64) * 65536.0).to(v.device)


def f32_ulp(v):
    return torch.from_numpy(np.spacing(np.abs(v.cpu().numpy()).astype(np.float32)).astype(np.float64)).to(v.device)


def affine(c_in, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.5 + torch.rand(c_in, generator=g)).cuda(), (0.3 * torch.randn(c_in, generator=g)).cuda()


def reference(x, c_in, gamma, beta, relu=True):
    """fp64 on the bf16 input x [n, hw, C]: -> mean, var [n, c_in], the two summands of the IN half [n, hw, c_in], y [n, hw, C]"""
    xd = x.double()
    xi = xd[..., :c_in]
    mean = xi.mean(1)
    var = ((xi - mean[:, None]) ** 2).mean(1)
    invstd = 1.0 / torch.sqrt(var + float(np.float32(EPS)))
    t1 = gamma.double() * (xi - mean[:, None]) * invstd[:, None]
    y = torch.cat((t1 + beta.double(), xd[..., c_in:]), -1)
    return mean, var, invstd, t1, (y.clamp(min=0) if relu else y)


def pair_data(n, hw, C, seed, centre=None, spread=3):
    """integers mean + k and mean - k in pairs over the pixels (hw = 1: the mean itself), an integer mean per (n, c): centred values and
    their squares are exact in fp32, and so is every partial sum"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    mean = torch.randint(-4, 5, (n, 1, C), device="cuda", generator=g) if centre is None else torch.full((n, 1, C), centre, device="cuda")
    if hw == 1:
        return mean.to(bf16), None
    assert hw % 2 == 0
    k = torch.randint(0, spread + 1, (n, hw // 2, C), device="cuda", generator=g)
    return k, mean


def assemble(k, mean, seed):
    n, half, C = k.shape
    x = torch.cat((mean + k, mean - k), 1)
    perm = torch.randperm(2 * half, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))
    x = x[:, perm].contiguous()
    assert x.abs().max() <= 256                               # integers up to 256 are bf16 values
    return x.to(bf16)


def check_stats_exact(x, c_in, mean, invstd):
    rm, rv, rinv, _, _ = reference(x, c_in, torch.ones(c_in, device="cuda"), torch.zeros(c_in, device="cuda"))
    assert torch.equal(mean, rm.float()) and torch.equal(rm.float().double(), rm), "mean must equal the fp64 mean bit for bit"
    assert ((invstd.double() - rinv).abs() <= 4 * f32_ulp(rinv)).all(), float(((invstd.double() - rinv).abs() / f32_ulp(rinv)).max())


def check_y(y, x, c_in, gamma, beta, relu=True, extra=0.0):
    _, _, _, t1, ref = reference(x, c_in, gamma, beta, relu)
    tol = 2.0 ** -8 * ref.abs()
    tol[..., :c_in] += 0.5 * bf16_ulp(t1) + 0.5 * bf16_ulp(beta.double()) + extra
    err = (y.double() - ref).abs()
    assert (err <= tol).all(), float((err - tol).max())
    want = x[..., c_in:].float().clamp(min=0) if relu else x[..., c_in:].float()
    assert torch.equal(y[..., c_in:].float(), want), "the BatchNorm half passes through (ReLU only)"


EXACT_SHAPES = [(3, 1, 16, 8), (3, 8, 64, 32), (2, 32, 32, 16), (2, 128, 256, 128), (2, 512, 128, 64), (2, 2048, 64, 32), (2, 2048, 128, 64),
                (2, 3072, 64, 32), (1, 9216, 64, 32), (500, 128, 256, 128)]


# ---- 1. exact statistics ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hw,C,c_in", EXACT_SHAPES)
def test_exact_statistics(mods, n, hw, C, c_in):
    k, mean = pair_data(n, hw, C, seed=hw + C)
    x = k if mean is None else assemble(k, mean, seed=7)
    gamma, beta = affine(c_in, 3)
    y, m, inv = mods["nn"].ibn_act(x, c_in, gamma, beta, want_stats=True)
    check_stats_exact(x, c_in, m, inv)
    check_y(y, x, c_in, gamma, beta)
    if hw == 1:                                               # var = 0, x - mean = 0: y is the bias
        want = beta.clamp(min=0).to(bf16).expand(n, 1, c_in)
        assert torch.equal(y[..., :c_in], want)


# ---- 2. offset ----------------------------------------------------------------------------------------------------
def test_offset_needs_a_centred_variance(mods):
    """x = 224 + k, |k| <= 3: E[x^2] - mean^2 of raw fp32 sums is off by 1e-4 .. 4e-4 in the variance (x^2 ~ 50000 has an ulp of 2^-8
    and the sum of 2048 of them one of 8: sum k^2 is made no multiple of 8, so it cannot survive there), a centred sum is exact."""
    n, hw, C, c_in = 2, 2048, 64, 32
    k, mean = pair_data(n, hw, C, seed=5, centre=224)
    s = (k * k).sum(1)                                        # [n, C]; the tensor's sum of k^2 is twice this
    fix = (s % 4 == 0)
    k[:, 0, :] = torch.where(fix, torch.where(k[:, 0, :] % 2 == 0, torch.ones_like(s), torch.zeros_like(s)), k[:, 0, :])
    assert ((2 * (k * k).sum(1)) % 8 != 0).all()
    x = assemble(k, mean, seed=9)
    assert x.float().min() >= 221 and x.float().max() <= 227
    gamma, beta = affine(c_in, 4)
    y, m, inv = mods["nn"].ibn_act(x, c_in, gamma, beta, want_stats=True)
    check_stats_exact(x, c_in, m, inv)
    check_y(y, x, c_in, gamma, beta)
    # the separation, in fp32 on the same data: the raw-moment variance misses the bound that the kernel has just met
    xf = x.float()[..., :c_in]
    raw_var = (xf * xf).sum(1) / hw - (xf.sum(1) / hw) ** 2
    _, var, rinv, _, _ = reference(x, c_in, gamma, beta)
    raw_inv = 1.0 / torch.sqrt(raw_var.double().clamp(min=0) + float(np.float32(EPS)))
    assert ((raw_inv - rinv).abs() > 4 * f32_ulp(rinv)).float().mean() > 0.9


# ---- 3. random data -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hw,C,c_in", [(3, 8, 64, 32), (2, 2048, 128, 64), (2, 3072, 64, 32)])
@pytest.mark.parametrize("relu", [0, 1])
def test_random_data_against_fp64(mods, n, hw, C, c_in, relu):
    """Tolerances from the arithmetic, for ANY summation order of hw fp32 terms (u = 2^-24): |d mean| <= hw u mean|x|; the variance's
    relative error <= hw u (+ 4 ulp for the division, the eps, the square root and the reciprocal), so invstd's <= hw u / 2 + 2^-21; y adds
    the bf16 rounding 2^-8 |ref|, half a bf16 ulp of each summand (as for exact data: it covers the fp32 affine) and those two propagated:
    |gamma| invstd |d mean| + |t1| (hw u / 2 + 2^-21)."""
    g = torch.Generator().manual_seed(hw + relu)
    x = (torch.randn(n, hw, C, generator=g) * (0.5 + torch.rand(n, 1, C, generator=g) * 2) + torch.randn(n, 1, C, generator=g)).to(bf16).cuda()
    x[:, :, 3] = 1.5                                           # a constant channel: var = 0
    gamma, beta = affine(c_in, 6)
    nn = mods["nn"]
    y, m, inv = nn.ibn_act(x, c_in, gamma, beta, relu=bool(relu), want_stats=True)
    rm, var, rinv, t1, _ = reference(x, c_in, gamma, beta, bool(relu))
    u = 2.0 ** -24
    d_mean = hw * u * x.double()[..., :c_in].abs().mean(1)
    assert ((m.double() - rm).abs() <= d_mean + f32_ulp(rm)).all()
    rel_inv = hw * u / 2 + 2.0 ** -21
    assert ((inv.double() - rinv).abs() <= rel_inv * rinv + 0.5 * rinv ** 3 * d_mean ** 2).all()       # (the mean's error enters the centred sum squared)
    extra = (gamma.double() * rinv * d_mean)[:, None, :] + t1.abs() * rel_inv
    check_y(y, x, c_in, gamma, beta, bool(relu), extra=extra)
    assert torch.equal(m[:, 3], torch.full((n,), 1.5, device="cuda"))
    b3 = beta[3].clamp(min=0) if relu else beta[3]
    assert torch.equal(y[:, :, 3], b3.to(bf16).expand(n, hw))
    assert torch.equal(nn.ibn_act(x, c_in, gamma, beta, relu=bool(relu)), y), "want_stats must not change y"
    z = x.clone()
    assert nn.ibn_act(z, c_in, gamma, beta, relu=bool(relu), out=z) is z and torch.equal(z, y), "in place = out of place"
    assert torch.equal(nn.ibn_act(x, c_in, gamma, beta, relu=bool(relu)), y), "run to run"


# ---- 4. batch independence ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw,C,c_in", [(512, 128, 64), (2048, 64, 32), (3072, 64, 32), (128, 256, 128)])
def test_a_sample_does_not_see_its_batch(mods, hw, C, c_in):
    x = torch.randn(5, hw, C, generator=torch.Generator().manual_seed(hw)).to(bf16).cuda()
    gamma, beta = affine(c_in, 8)
    y, m, inv = mods["nn"].ibn_act(x, c_in, gamma, beta, want_stats=True)
    for i in (0, 3, 4):
        yi, mi, ii = mods["nn"].ibn_act(x[i:i + 1].contiguous(), c_in, gamma, beta, want_stats=True)
        assert torch.equal(yi[0], y[i]) and torch.equal(mi[0], m[i]) and torch.equal(ii[0], inv[i])


# ---- 5. refusals ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,c_in,word", [((2, 4, 16), 12, "c_in"), ((2, 4, 16), 24, "c_in"), ((2, 0, 16), 8, "hw"), ((2, 4, 12), 8, "C must")])
def test_refusals_launch_nothing(mods, shape, c_in, word):
    x = torch.ones(shape, dtype=bf16, device="cuda")
    out = torch.full(shape, 7.0, dtype=bf16, device="cuda")
    gamma, beta = torch.ones(32, device="cuda"), torch.zeros(32, device="cuda")
    with pytest.raises(mods["lib"].DaliError) as e:
        mods["nn"].ibn_act(x, c_in, gamma, beta, out=out)
    assert word in str(e.value) and word in mods["lib"].last_error(), str(e.value)
    torch.cuda.synchronize()
    assert (out == 7.0).all()


# ---- 6. plan tables ---------------------------------------------------------------------------------------------------
def plan_fields(p):
    return (p.param_elems, p.buffer_elems, p.arena_bytes, p.feat_dim, p.n_params, p.n_buffers)


def golden_params_buffers(gold, pre):
    extras = ("conv1x1_layer4", "conv1x1_squeeze_layer4", "conv1x1_expand_layer4", "attribute_classifier")
    rows = [(str(k), eval(str(s))) for k, s in zip(gold[pre + "keys"], gold[pre + "shapes"])]
    rows = [(k, s) for k, s in rows if k.split(".")[0] not in extras and not k.endswith("num_batches_tracked")]
    is_buf = lambda k: k.endswith("running_mean") or k.endswith("running_var")
    return [r for r in rows if not is_buf(r[0])], [r for r in rows if is_buf(r[0])]


def test_zero_ext_is_the_plain_plan_and_ibn_tables(mods, gold):
    E, dev = mods["E"], torch.device("cuda", 0)
    for layers, width, shape in (((1, 1, 1, 1), 32, (8, 64, 32)), ((1, 2, 1, 2), 64, (4, 128, 64))):
        plain, zero = E._Plan(dev, *shape, layers, width), E._Plan(dev, *shape, layers, width, ibn=(0, 0, 0, 0))
        assert plan_fields(zero) == plan_fields(plain)
        assert zero.tensor_table(0) == plain.tensor_table(0) and zero.tensor_table(1) == plain.tensor_table(1)
    assert plan_fields(E._Plan(dev, 8, 64, 32, (1, 1, 1, 1), 32, ibn=(0, 0, 0, 0))) == (2013440, 11904, 19311616, 1024, 53, 36)   # test_gpu_resnet's pin
    for pre, layers in (("small/", (1, 1, 1, 1)), ("r50/", (3, 4, 6, 3)), ("r101/", (3, 4, 23, 3))):
        p = E._Plan(dev, 2, 64, 32, layers, 64, ibn=(1, 1, 1, 0))
        params, buffers = golden_params_buffers(gold, pre)
        assert [(t[0], t[3]) for t in p.tensor_table(0)] == params
        assert [(t[0], t[3]) for t in p.tensor_table(1)] == buffers
        if pre == "r50/":
            assert sum(t[2] for t in p.tensor_table(0)) == 23512128
    # an eval plan reserves none of the backward's buffers
    assert E._Plan(dev, 8, 64, 32, (1, 1, 1, 1), 32, ibn=(1, 1, 1, 0)).arena_bytes < 19311616


# ---- the small net of the golden file ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(mods, gold):
    ref = R.build((1, 1, 1, 1), 64)
    ref.load_state_dict(R.seeded_state(ref.state_dict(), int(gold["small/w_seed"])))
    ref.eval()
    net = mods["E"].ResNet50IBNReID(layers=(1, 1, 1, 1), width=64, seed=1)
    net.load_state_dict(ref.state_dict())
    net.eval()
    n, h, w = [int(v) for v in gold["small/geom"][:3]]
    x = torch.randn(n, 3, h, w, generator=torch.Generator().manual_seed(int(gold["small/x_seed"])))
    return ref, net, x


# ---- 7. block wiring ----------------------------------------------------------------------------------------------------
def test_block0_wiring(mods, small):
    ref, net, x = small
    net(x.cuda())
    pool0 = net.debug_tensor("pool0", bf16, (4, 16, 8, 64)).float().cpu().permute(0, 3, 1, 2)
    a1 = net.debug_tensor("block0.a1", bf16, (4, 16, 8, 64)).float().cpu().permute(0, 3, 1, 2)
    mean = net.debug_tensor("block0.in1.mean", torch.float32, (4, 32)).cpu()
    invstd = net.debug_tensor("block0.in1.invstd", torch.float32, (4, 32)).cpu()
    blk = ref.layer1[0]
    with torch.no_grad():
        u1 = F.conv2d(pool0, blk.conv1.weight.to(bf16).float())
        scale, shift = R.T._bn_eval_coeffs(blk.bn1.BN)
        ref_bn = F.relu(u1[:, 32:] * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
        raw = R.T.Q(u1[:, :32])
        rmean, rinv = R.ibn_stats(raw)
        gamma, beta = blk.bn1.IN.weight.view(1, -1, 1, 1), blk.bn1.IN.bias.view(1, -1, 1, 1)
        ref_in = F.relu((raw - rmean) * (rinv * gamma) + beta)
    err = (a1[:, 32:] - ref_bn).abs()
    assert (err <= 2.0 ** -7 * ref_bn.abs() + 1e-3).all(), float(err.max())                 # test_gpu_conv's criterion
    # the IN half: what is left against the twin is summation order flipping one bf16 ulp of raw (at most 2^-8 |raw|), amplified by
    # gamma * invstd; the bound allows twice that
    err = (a1[:, :32] - ref_in).abs()
    tol = 2.0 ** -7 * ref_in.abs() + 2.0 ** -7 * gamma.abs() * rinv * raw.abs()
    assert (err <= tol).all(), float((err - tol).max())
    assert (ref_in > 0).float().mean() > 0.2 and (ref_bn > 0).float().mean() > 0.2
    # the statistics the launch saw, against those of the rounded raw: every element at most one bf16 ulp (2^-8 |raw|) away, so the mean moves by
    # at most 2^-8 mean|raw| and the standard deviation (1-Lipschitz in the rms of the perturbation) by at most 2^-8 rms(raw)
    rmean, rinv = rmean.flatten(1), rinv.flatten(1)
    assert ((mean - rmean).abs() <= 2.0 ** -8 * raw.abs().mean((2, 3)) + 1e-6).all()
    assert ((invstd - rinv).abs() <= rinv * (2.0 ** -8 * (raw ** 2).mean((2, 3)).sqrt() * rinv + 1e-5)).all()
    assert (mean.abs() > 1e-3).any() and (invstd > 0).all()


# ---- 8. golden output -----------------------------------------------------------------------------------------------------
def test_golden_output_of_the_reference_wrapper(mods, gold, small):
    ref, net, x = small
    y_ref = torch.from_numpy(gold["small/y_eval"])
    e_hip = rel_l2(net(x.cuda()).cpu(), y_ref)
    e_twin = rel_l2(R.forward_matched_eval(ref, x), y_ref)
    print("IBN small net vs the reference's output: rel-L2 HIP %.3e | twin %.3e" % (e_hip, e_twin))
    assert e_hip < 1.5 * e_twin + 5e-3, (e_hip, e_twin)
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == [(str(k), eval(str(s))) for k, s in zip(gold["small/keys"], gold["small/shapes"])]


# ---- 9 / 10. full-size nets ------------------------------------------------------------------------------------------------
def pretrained_like(model, seed):
    """tests/test_gpu_e2e_parity.pretrained_like (bn3 ~ 0.2: every bottleneck a small perturbation of its identity path), and the same for the IN affine"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, m in model.named_modules():
            if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.InstanceNorm2d)):
                lo = 0.2 if name.endswith("bn3") else 1.0
                m.weight.copy_(lo * (0.5 + torch.rand(m.weight.shape, generator=g)))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.running_mean.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
                    m.running_var.copy_(0.5 + torch.rand(m.bias.shape, generator=g))


def person_images(pids, H, W, seed, noise=0.4):
    g = torch.Generator().manual_seed(seed)
    pat = torch.randn(int(max(pids)) + 1, 3, 8, 4, generator=g)
    base = F.interpolate(pat[torch.as_tensor(pids)], size=(H, W), mode="bilinear", align_corners=False)
    return base + noise * torch.randn(len(pids), 3, H, W, generator=g)


# HIP vs the rounding-matched twin, ResNet-50-IBN-a, eval, batch 16 at 256 x 128: measured 5.7e-3 on MI355X, bound = measured + a third.
# (The plain net: 3.0e-3 measured, bound 4e-3.  The instance statistics are taken from the rounded conv1 output on both sides, so a bf16 ulp
# that flips on summation order moves a whole channel's mean and scale, not one element.)  A wiring mistake costs at least 1e-2.
IBN50_HIP_TWIN_EVAL = 7.6e-3


def test_full_resnet50_ibn_eval_vs_twin(mods):
    torch.manual_seed(1)
    ref = R.build((3, 4, 6, 3), 64)
    pretrained_like(ref, 2)
    ref.eval()
    net = mods["E"].ResNet50IBNReID(ref.state_dict())                      # model_base = a state_dict of the wrapper: loads whole
    net.eval()
    assert sum(p.numel() for n, p in net.named_parameters() if n in net._grad_views) == 23512128
    assert sum(p.numel() for p in net.parameters()) == sum(p.numel() for p in ref.parameters()) == 23512128 + 6476889
    torch.set_num_threads(max(torch.get_num_threads(), 8))
    x = person_images(np.arange(16) % 8, 256, 128, 11)
    e_twin = R.forward_matched_eval(ref, x)
    with torch.no_grad():
        e_fp32 = ref(x)
    e_hip = net(x.cuda()).cpu()
    hip_twin, twin_fp32 = rel_l2(e_hip, e_twin), rel_l2(e_twin, e_fp32)
    print("ResNet-50-IBN-a eval: embedding rel-L2 HIP-vs-twin %.3e | twin-vs-fp32 %.3e" % (hip_twin, twin_fp32))
    assert hip_twin < IBN50_HIP_TWIN_EVAL, hip_twin


def test_resnet101_ibn(mods, gold):
    torch.manual_seed(3)
    ref = R.build((3, 4, 23, 3), 64, wrapper=R.ResNet101IBNReID)
    pretrained_like(ref, 4)
    ref.eval()
    net = mods["E"].ResNet101IBNReID(seed=5)
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == [(str(k), eval(str(s))) for k, s in zip(gold["r101/keys"], gold["r101/shapes"])]
    assert sum(p.numel() for p in net.parameters()) == sum(p.numel() for p in ref.parameters())
    net.load_state_dict(ref.state_dict())
    net.eval()
    torch.set_num_threads(max(torch.get_num_threads(), 8))
    x = person_images(np.arange(2), 256, 128, 12)
    with torch.no_grad():
        y_ref = ref(x)
    e_hip, e_twin = rel_l2(net(x.cuda()).cpu(), y_ref), rel_l2(R.forward_matched_eval(ref, x), y_ref)
    print("ResNet-101-IBN-a eval vs fp32: rel-L2 HIP %.3e | twin %.3e" % (e_hip, e_twin))
    assert e_hip < 1.5 * e_twin + 5e-3, (e_hip, e_twin)


# ---- 11. getDCNN ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cls", [("resnet50IBN", "ResNet50IBNReID"), ("resnet101IBN", "ResNet101IBNReID")])
def test_getdcnn(mods, name, cls):
    E = mods["E"]
    on, mo = E.getDCNN([0], name, 2048)
    assert type(on.module).__name__ == type(mo.module).__name__ == cls
    assert not on.training and not mo.training and not on.module.training
    keys = list(on.state_dict().keys())
    assert keys[0] == "module.conv1.weight" and "module.layer1.0.bn1.IN.weight" in keys and keys == list(mo.state_dict().keys())
    for a, b in zip(on.state_dict().values(), mo.state_dict().values()):
        assert torch.equal(a, b)
    assert on.module.flat_params.data_ptr() != mo.module.flat_params.data_ptr()


def test_getdcnn_still_refuses_the_rest(mods):
    E = mods["E"]
    with pytest.raises(NotImplementedError):
        E.getDCNN([0], "osnet")
    with pytest.raises(NotImplementedError):
        E.getDCNN([0], "resnet50IBN", embedding_size=512)


# ---- 12. training is refused at every level --------------------------------------------------------------------------------
def test_train_mode_is_refused(mods, small):
    _, net, x = small
    L, lib = mods["lib"].lib(), mods["lib"]
    xd = x.cuda()
    before = net(xd).clone()
    net.train()
    try:
        with pytest.raises(NotImplementedError) as e:
            net(xd)
        assert "eval only" in str(e.value) and ".eval()" in str(e.value)
    finally:
        net.eval()
    plan = net._last_plan
    emb = torch.empty(4, 2048, device="cuda")
    rc = L.dali_resnet_forward(plan.h, lib.stream_ptr(), lib.ptr(xd), 1, lib.ptr(emb))
    assert rc != 0 and "eval only" in lib.last_error()
    rc = L.dali_resnet_backward(plan.h, lib.stream_ptr(), lib.ptr(emb), 0, 3)
    assert rc != 0 and "eval only" in lib.last_error()
    with pytest.raises(lib.DaliError) as e:
        net._run_forward(xd, training=True)
    assert "eval only" in str(e.value)
    assert torch.equal(net(xd), before), "the model stays usable, bit for bit"


# ---- 13. checkpoints and model_base ------------------------------------------------------------------------------------------
def test_checkpoint_and_model_base(mods, small):
    ref, net, x = small
    E, xd = mods["E"], x.cuda()
    before = net(xd).clone()
    buf = io.BytesIO()
    torch.save(net.state_dict(), buf)
    buf.seek(0)
    fresh = E.ResNet50IBNReID(layers=(1, 1, 1, 1), width=64, seed=9).eval()
    assert not torch.equal(fresh(xd), before)
    fresh.load_state_dict(torch.load(buf))
    assert torch.equal(fresh(xd), before)
    shim = E._DataParallelShim(E.ResNet50IBNReID(layers=(1, 1, 1, 1), width=64, seed=10)).eval()
    shim.load_state_dict({"module." + k: v for k, v in net.state_dict().items()})
    assert torch.equal(shim(xd), before)
    # model_base = an IBN-a trunk (with its classifier): the trunk is taken over, fc.* dropped, last_bn and the unused modules stay this model's own
    trunk = R.ibn_trunk((1, 1, 1, 1), 64)
    trunk.load_state_dict({k: v for k, v in ref.state_dict().items() if k in trunk.state_dict()}, strict=False)
    assert any(k.startswith("fc.") for k in trunk.state_dict())
    based = E.ResNet50IBNReID(trunk, layers=(1, 1, 1, 1), width=64, seed=11).eval()
    sd = based.state_dict()
    assert not any(k.startswith("fc.") for k in sd)
    for k, v in trunk.state_dict().items():
        if not k.startswith("fc."):
            assert torch.equal(sd[k].cpu(), v), k
    assert torch.equal(sd["last_bn.weight"].cpu(), torch.ones(2048))
    from oracle.resnet50_reid import ResNet50ReID as PlainNet
    with pytest.raises(mods["lib"].DaliError):
        E.ResNet50IBNReID(PlainNet(layers=(1, 1, 1, 1), width=64).state_dict(), layers=(1, 1, 1, 1), width=64)


# ---- 14. surface ----------------------------------------------------------------------------------------------------------------
def test_surface(mods, small):
    _, net, x = small
    E, GF, syn, VM, ev = mods["E"], mods["GF"], mods["syn"], mods["VM"], mods["ev"]
    xd = x.cuda()
    y = net(xd)
    assert torch.equal(net(xd, multipart=True, attention_map=True), y), "both flags are ignored"
    assert torch.equal(net.forward_heads(xd, [("both", None)])[0], y)
    assert net.head_map(64, 32) == (4, 2)
    net.feature = "gmp"
    try:
        assert torch.equal(net.forward_heads(xd, [("gmp", None)])[0], net(xd))
    finally:
        net.feature = "both"
    data = syn.SyntheticImages(n_ids=3, per_id=3, n_cams=2, seed=5, noise=0.4).install()
    try:
        sizes = []

        def counting(paths, img_height, img_width, turb=None):
            sizes.append(len(paths))
            return data.loader(paths, img_height, img_width, turb)

        GF.set_image_loader(counting)
        model = E._DataParallelShim(net).eval()
        rows = data.records[:5]
        fv = GF.extractFeatures(rows, 64, 32, model, 2, gpu_index=0, keep_on_device=True, verbose=False)
        assert sizes == [2, 2, 1]
        paths = [r[0] for r in rows]
        direct = torch.cat([net(data.loader(paths[b:b + 2], 64, 32)) for b in (0, 2, 4)])
        assert torch.equal(fv, direct)
        _, gallery, queries = data.split(1)
        v = VM.validateModels()
        v.setParameters(64, 32, False, 0)
        cmc, mAP, dist = v.validate(queries, gallery, model)
        fq, fg = net(data.loader([r[0] for r in queries], 64, 32)), net(data.loader([r[0] for r in gallery], 64, 32))
        assert torch.equal(dist, v.distance(fq, fg)) and 0.0 <= mAP <= 1.0 and len(cmc) >= 1
    finally:
        syn.SyntheticImages.uninstall()
