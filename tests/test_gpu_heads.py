"""GPU: the multi-output head -- dali_head_pool_multi and dali_channel_sum alone (exact data, normal data, refusals), the plan entry
dali_resnet_forward_heads under ResNet50ReID.forward_heads / forward(multipart=, attention_map=), and the one-pass fusion mirror.

References: tests/heads_ref.py (fp64 numpy, itself checked against the reference's classes through tests/golden/heads.npz on the CPU) and the
existing single-head kernel / forward, which whole-map heads must reproduce bit for bit."""
import numpy as np
import pytest
import torch

import heads_ref as R

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from daliid_amd import Encoders, _lib, evaluateCleanATModels, getFeatures, ops_nn, synthetic
    return dict(E=Encoders, lib=_lib, FUS=evaluateCleanATModels, GF=getFeatures, nn=ops_nn, syn=synthetic)


@pytest.fixture(scope="module")
def gold():
    return R.load_golden()


def _dev(a):
    """fp64 / fp32 numpy of bf16-representable values -> bf16 CUDA tensor."""
    t = torch.from_numpy(np.asarray(a, np.float32))
    assert torch.equal(t.to(bf16).float(), t), "test data must be bf16-representable"
    return t.to(bf16).cuda()


def _ulp(a):
    return np.spacing(np.abs(np.asarray(a, np.float32))).astype(np.float64)


def eight_heads(h):
    """All three modes over every row, overlapping ranges, a single-row range, a duplicate and (0, h) spelled out: eight heads at once."""
    return [("both", None), ("gap", None), ("gmp", None), ("gmp", (0, (h + 1) // 2)), ("gap", (h // 4, h // 4 + max(1, h // 2))),
            ("both", (h - 1, h)), ("gmp", None), ("gap", (0, h))]


def int_map(kind, shape, seed):
    """Small integers, |x| <= 8: every fp32 sum is exact in any order."""
    rng = np.random.default_rng(seed)
    if kind == "negative":
        return rng.integers(-8, 0, shape).astype(np.float64)          # all negative: the maximum is not 0
    if kind == "ties":
        return rng.integers(0, 2, shape).astype(np.float64) * 3       # two levels: the maximum is met many times, in several lanes
    return rng.integers(-8, 9, shape).astype(np.float64)


def check_exact(nn, x, heads):
    """Integer data: max exact; mean = fp32(sum) / fp32(P) within 1 ulp (the division); "both" one more rounding; whole-map heads equal
    head_pool_fwd bit for bit."""
    xd = _dev(x)
    got = nn.head_pool_multi(xd, heads)
    assert got.shape == (len(heads), x.shape[0], x.shape[3])
    for i, (mode, rows) in enumerate(heads):
        b, e = R.rows_of(rows, x.shape[1])
        part = x[:, b:e].reshape(x.shape[0], -1, x.shape[3])
        P = part.shape[1]
        mx = part.max(1)
        mean = (np.float32(part.sum(1)) / np.float32(P)).astype(np.float64)          # the sum is an exact small integer
        g = got[i].cpu().numpy().astype(np.float64)
        if mode == "gmp":
            assert np.array_equal(g, mx), (i, mode, rows)
        elif mode == "gap":
            assert np.all(np.abs(g - mean) <= _ulp(mean)), (i, mode, rows, float(np.abs(g - mean).max()))
        else:
            assert np.all(np.abs(g - (mean + mx)) <= _ulp(mean) + _ulp(mean + mx)), (i, mode, rows, float(np.abs(g - mean - mx).max()))
        if (b, e) == (0, x.shape[1]):
            single, _ = nn.head_pool_fwd(xd, mode)
            assert torch.equal(got[i], single), (i, mode, rows)
    return got


SHAPES = [(1, 16, 8, 2048),       # the fixture's shape
          (2, 4, 2, 1024),        # the small nets' map
          (3, 5, 3, 8),           # 15 pixels, not a multiple of the 8 lanes; one chunk per image; a mostly idle block
          (33, 2, 1, 16)]         # fewer pixels than lanes; 66 items crossing a wave


@pytest.mark.parametrize("kind", ["mixed", "negative", "ties"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_head_pool_multi_exact(mods, shape, kind):
    x = int_map(kind, shape, seed=sum(shape))
    got = check_exact(mods["nn"], x, eight_heads(shape[1]))
    assert torch.equal(got[2], got[6]), "duplicate heads agree"
    if kind == "negative":
        assert float(got[2].max()) <= -1.0
    cs = mods["nn"].channel_sum(_dev(x))
    assert cs.shape == shape[:3]
    assert np.array_equal(cs.cpu().numpy().astype(np.float64), R.channel_sum(x))


@pytest.mark.parametrize("n_ranges", range(1, 9))
def test_head_pool_multi_every_range_count(mods, n_ranges):
    """The kernel is instantiated per number of DISTINCT ranges (heads over the same rows share accumulators): each instance, with a second
    mode on the first range."""
    shape = (2, 16, 3, 16)
    x = int_map("mixed", shape, seed=n_ranges)
    ranges = [None, (0, 8), (4, 12), (8, 16), (15, 16), (0, 1), (3, 14), (7, 9)][:n_ranges]
    heads = [("gmp", r) for r in ranges]
    heads = (heads + [("both", ranges[0])])[:8] if n_ranges < 8 else heads[:7] + [("both", ranges[7])]
    check_exact(mods["nn"], x, heads)


def test_head_pool_multi_single_head_modes(mods):
    x = int_map("mixed", (3, 5, 3, 8), seed=5)
    for mode in R.MODES:
        check_exact(mods["nn"], x, [(mode, None)])
        check_exact(mods["nn"], x, [(mode, (1, 4))])


def _normal_maps(gold):
    g = torch.Generator().manual_seed(9)
    small = torch.randn(3, 5, 3, 8, generator=g).to(bf16).float().numpy().astype(np.float64)
    return {"fixture": gold["map"], "3x5x3x8": small}


@pytest.mark.parametrize("which", ["fixture", "3x5x3x8"])
def test_head_pool_multi_normal_data(mods, gold, which):
    """fp32 sums in any order: means within 2 * 2^-24 * (sum_p |x_pc| + |ref_c|) (heads_ref.mean_bound), max exact; the heat map within
    2 * 2^-24 * C * sum_c |x_c|."""
    x = _normal_maps(gold)[which]
    heads = eight_heads(x.shape[1])
    xd = _dev(x)
    got = mods["nn"].head_pool_multi(xd, heads).cpu().numpy().astype(np.float64)
    for i, (mode, rows) in enumerate(heads):
        ref = R.pool(x, mode, rows)
        err, bound = np.abs(got[i] - ref), R.mean_bound(x, ref, mode, rows)
        print("%s head %d %s %s: max err %.3e, max err / bound %.3f" % (which, i, mode, rows, err.max(), (err / np.maximum(bound, 1e-300)).max() if mode != "gmp" else 0))
        assert np.all(err <= bound), (i, mode, rows, float(err.max()))
        if rows is None:
            assert torch.equal(mods["nn"].head_pool_multi(xd, [(mode, None)])[0], mods["nn"].head_pool_fwd(xd, mode)[0])
    heat = mods["nn"].channel_sum(xd).cpu().numpy().astype(np.float64)
    err = np.abs(heat - R.channel_sum(x))
    print("%s heat map: max err %.3e, bound min %.3e" % (which, err.max(), R.heat_bound(x).min()))
    assert np.all(err <= R.heat_bound(x))
    assert torch.equal(mods["nn"].channel_sum(xd), mods["nn"].channel_sum(xd)), "no atomics: the same bits on every run"


def test_fixture_outputs_through_the_neck(mods, gold):
    """The reference classes' own outputs (tests/golden/heads.npz) against head_pool_multi + the eval neck (bn1d_fwd by running statistics).
    Tolerance: the pooling bound scaled by |gamma * invstd|, plus heads_ref.neck_bound for the neck's own fp32 roundings, which the two sides
    (this kernel: x * scale + shift; torch: its own BatchNorm arithmetic) take in different orders -- once per side."""
    nn, x = mods["nn"], gold["map"]
    heads = [(mode, rows) for _, mode, rows in R.GOLDEN_HEADS]
    pooled = nn.head_pool_multi(_dev(x), heads)
    w, b, rm, rv = (torch.from_numpy(t).cuda() for t in gold["bn"])
    y, _, _ = nn.bn1d_fwd(pooled.view(-1, pooled.shape[2]), w, b, rm, rv, training=False)
    y = y.view_as(pooled).cpu().numpy().astype(np.float64)
    scale, _ = R.neck_coeffs(*gold["bn"])
    for i, (key, mode, rows) in enumerate(R.GOLDEN_HEADS):
        ref = R.pool(x, mode, rows)
        tol = 2 * (R.mean_bound(x, ref, mode, rows) * np.abs(scale) + R.neck_bound(ref, *gold["bn"]))
        err = np.abs(y[i] - gold[key].astype(np.float64))
        print("%s: max err %.3e, max err / tol %.3f" % (key, err.max(), (err / tol).max()))
        assert np.all(err <= tol), (key, float(err.max()))
    heat = nn.channel_sum(_dev(x))[0].cpu().numpy().astype(np.float64)
    assert np.all(np.abs(heat - gold["heatmap"]) <= 2 * R.heat_bound(x)[0])


def test_refusals_leave_output_untouched(mods):
    """Every invalid spec returns DALI_ERR_INVALID before any launch: the output keeps its sentinel."""
    nn, _lib = mods["nn"], mods["lib"]
    L = _lib.lib()

    def call(shape, specs, n_heads=None):
        n, h, w, C = shape
        x = torch.zeros(n, h, w, C, dtype=bf16, device="cuda")
        f = torch.full((8, n, C), 7.5, device="cuda")
        arr = (nn.HeadSpec * 9)(*[nn.HeadSpec(*s) for s in specs])
        rc = L.dali_head_pool_multi(_lib.ctx(x.device), _lib.stream_ptr(), _lib.ptr(x), n, h, w, C, arr, len(specs) if n_heads is None else n_heads,
                                    _lib.ptr(f))
        torch.cuda.synchronize()
        assert bool((f == 7.5).all()), "a refused call wrote to f"
        return rc

    ok = (2, 4, 2, 16)
    bad = [(ok, [(2, 0, 0)], 0), (ok, [(2, 0, 0)] * 9, 9), (ok, [(2, 0, 0)], -1),       # n_heads < 1, > DALI_MAX_HEADS
           (ok, [(2, 0, 5)], None),                                                          # row_end > h
           (ok, [(2, 3, 3)], None), (ok, [(2, 3, 2)], None), (ok, [(2, 2, 0)], None),     # row_begin >= row_end, not both 0
           (ok, [(3, 0, 0)], None), (ok, [(-1, 0, 0)], None), (ok, [(2, 0, 0), (7, 0, 2)], None),      # a bad mode
           ((2, 4, 2, 12), [(2, 0, 0)], None),                                              # C % 8 != 0
           ((1, 32768, 1, 8), [(2, 0, 0)], None), ((1, 256, 128, 8), [(2, 0, 0)], None)]   # h * w >= 32768
    for shape, specs, nh in bad:
        assert call(shape, specs, nh) == -1, (shape, specs, nh)
        assert "head_pool_multi" in _lib.last_error()
    with pytest.raises(_lib.DaliError):
        nn.head_pool_multi(torch.zeros(ok, dtype=bf16, device="cuda"), [("max", None)])
    with pytest.raises(_lib.DaliError):
        nn.channel_sum(torch.zeros(2, 3, 12, dtype=bf16, device="cuda"))


def test_head_pool_multi_just_under_the_pixel_limit(mods):
    x = int_map("mixed", (1, 255, 128, 8), seed=1)                    # h * w = 32640 < 32768
    check_exact(mods["nn"], x, [("gmp", None), ("gap", (254, 255)), ("both", None)])


# ---- the plan ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net(mods):
    m = mods["E"].ResNet50ReID(layers=(1, 1, 1, 1), width=32, seed=4).eval()
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():                                    # a neck that does something: random affine and running statistics
        D = m.feat_dim
        m.last_bn.weight.copy_((torch.rand(D, generator=g) + 0.5).cuda())
        m.last_bn.bias.copy_((torch.randn(D, generator=g) * 0.3).cuda())
        m.last_bn.running_mean.copy_((torch.randn(D, generator=g) * 0.2 + 0.5).cuda())
        m.last_bn.running_var.copy_((torch.rand(D, generator=g) + 0.25).cuda())
    return m


def _images(B):
    return torch.randn(B, 3, 64, 32, generator=torch.Generator().manual_seed(B)).cuda()


@pytest.mark.parametrize("B", [5, 16])
def test_plan_heads(mods, net, B):
    x = _images(B)
    assert net.head_map(64, 32) == (4, 2)
    before = net(x).clone()
    singles = {}
    for mode in R.MODES:
        net.feature = mode
        singles[mode] = net(x).clone()
    net.feature = "both"
    assert torch.equal(singles["both"], before)
    heads = net.forward_heads(x, [(mode, None) for mode in R.MODES])
    assert heads.shape == (3, B, net.feat_dim) and not heads.requires_grad
    for i, mode in enumerate(R.MODES):
        assert torch.equal(heads[i], singles[mode]), mode
    parts = net(x, multipart=True)
    assert len(parts) == 4 and torch.equal(parts[3], singles["gmp"])
    emb, heat = net.forward_heads(x, [("gmp", rows) for rows in mods["E"].default_parts(4)] + [("gap", (1, 3))], heatmap=True)
    assert heat.shape == (B, 4, 2)
    for i in range(3):
        assert torch.equal(emb[i], parts[i])
    assert torch.equal(net(x, attention_map=True), heat[0])
    # against the fp64 restatement on the plan's own layer4 map
    ymap = net.debug_tensor("block3.y", bf16, (B, 4, 2, 1024)).float().cpu().numpy().astype(np.float64)
    bn = tuple(t.detach().cpu().numpy() for t in (net.last_bn.weight, net.last_bn.bias, net.last_bn.running_mean, net.last_bn.running_var))
    scale, _ = R.neck_coeffs(*bn)
    specs = [("gmp", rows) for rows in mods["E"].default_parts(4)] + [("gap", (1, 3))]
    for i, (mode, rows) in enumerate(specs):
        f = R.pool(ymap, mode, rows)                        # max: exact, so only the neck's roundings remain
        tol = R.mean_bound(ymap, f, mode, rows) * np.abs(scale) + R.neck_bound(f, *bn)
        err = np.abs(emb[i].cpu().numpy().astype(np.float64) - R.neck(f, *bn))
        print("B %d head %d %s %s: max err %.3e, max err / tol %.3f" % (B, i, mode, rows, err.max(), (err / tol).max()))
        assert np.all(err <= tol), (i, mode, rows, float(err.max()))
    herr = np.abs(heat.cpu().numpy().astype(np.float64) - R.channel_sum(ymap))
    assert np.all(herr <= R.heat_bound(ymap)), float(herr.max())
    assert net.feature == "both"
    assert torch.equal(net(x), before), "a plain forward gives the same bits after the multi-head calls"


def test_plan_heads_are_eval_only(mods, net):
    x = _images(5)
    net.train()
    try:
        for call in (lambda: net.forward_heads(x, [("gmp", None)]), lambda: net(x, multipart=True), lambda: net(x, attention_map=True)):
            with pytest.raises(mods["lib"].DaliError):
                call()
    finally:
        net.eval()
    with pytest.raises(mods["lib"].DaliError):
        net.forward_heads(x, [("gmp", (0, 5))])               # 4-row map
    with pytest.raises(mods["lib"].DaliError):
        net.forward_heads(x, [("gmp", None)] * 9)


# ---- the mirror -------------------------------------------------------------------------------------------------
def test_fusion_mirror_one_pass(mods):
    """validate() extracts every (model, subset) once and returns exactly what the sequence it replaces gives: four extractFeatures, twelve
    getWeightsByMagnitude, fuse_distmats and calculateMetrics, restated here from the public pieces."""
    E, FUS, GF, syn = mods["E"], mods["FUS"], mods["GF"], mods["syn"]
    from daliid_amd import ops_eval
    data = syn.SyntheticImages(n_ids=6, per_id=5, n_cams=3, seed=11, noise=0.4).install()
    try:
        nets = [E._DataParallelShim(E.ResNet50ReID(layers=(1, 1, 1, 1), width=32, seed=s)).eval() for s in (1, 2)]
        H, W = 64, 32
        _, gallery, queries = data.split(1)
        calls = []

        def counting(paths, img_height, img_width, turb=None):
            calls.append(len(paths))
            return data.loader(paths, img_height, img_width, turb)

        GF.set_image_loader(counting)
        res = FUS.validate(queries, gallery, nets[0], nets[1], H, W, [0], verbose=False)
        # every image once per model: 2 models x 2 subsets, each under 500 rows (the sequence below makes 16 calls)
        assert len(calls) == 4 and sum(calls) == 2 * (len(queries) + len(gallery)), calls
        del calls[:]
        ex = lambda s, m: GF.extractFeatures(s, H, W, m, 500, gpu_index=0, keep_on_device=True, verbose=False)
        q_c, q_d, g_c, g_d = ex(queries, nets[0]), ex(queries, nets[1]), ex(gallery, nets[0]), ex(gallery, nets[1])
        P = FUS.precision
        metrics = lambda dm: FUS.calculateMetrics(queries, gallery, dm, verbose=False)
        want = {"concatenation": metrics(ops_eval.pairdist(torch.cat((q_c, q_d), 1), torch.cat((g_c, g_d), 1), precision=P, normalize=True)),
                "clean": metrics(ops_eval.pairdist(q_c, g_c, precision=P, normalize=True)),
                "distortion": metrics(ops_eval.pairdist(q_d, g_d, precision=P, normalize=True)),
                "simple_ensemble": metrics(FUS.fuse_distmats(q_c, g_c, q_d, g_d))}
        for pooling in ("gap", "gmp", "both"):
            mag = lambda s, m: FUS.getWeightsByMagnitude(s, pooling, H, W, m, [0])[0]
            want["ensemble_" + pooling] = metrics(FUS.fuse_distmats(q_c, g_c, q_d, g_d, (mag(queries, nets[0]), mag(gallery, nets[0])),
                                                                    (mag(queries, nets[1]), mag(gallery, nets[1]))))
        assert len(calls) == 16
        assert list(res) == list(want)
        for name, (cmc, mAP) in want.items():
            assert res[name][1] == mAP, (name, res[name][1], mAP)
            assert np.array_equal(res[name][0], cmc), name
        # the three poolings from one pass, as getWeightsByMagnitude gives them one by one
        both = FUS.getWeightsByMagnitudeAll(queries, H, W, nets[0], [0])
        for pooling in ("gap", "gmp", "both"):
            norms, unit = FUS.getWeightsByMagnitude(queries, pooling, H, W, nets[0], [0])
            assert torch.equal(both[pooling][0], norms) and torch.equal(both[pooling][1], unit)
        # the multi-part extractor: four CPU tensors equal to forward(multipart=True) on the same batch
        parts = GF.extractFeaturesMultiPart(queries, H, W, nets[0], 4)
        imgs = data.loader(list(queries[:, 0]), H, W)
        ref = nets[0](imgs, multipart=True)
        assert len(parts) == 4
        for got, r in zip(parts, ref):
            assert got.device.type == "cpu" and got.shape == (len(queries), nets[0].module.feat_dim)
        # (batches of 4 against one batch of 6: every image's embedding depends on its own pixels only, the same kernels run on each)
        one = GF.extractFeaturesMultiPart(queries, H, W, nets[0], 500)
        for got, r in zip(one, ref):
            assert torch.equal(got, r.cpu())
        with pytest.raises(TypeError):
            GF.extractFeatures(queries, H, W, torch.nn.Identity(), 500, features=("gap",))
    finally:
        syn.SyntheticImages.uninstall()
