"""GPU: Weibull meta-recognition score fusion (include/daliid.h, dali_mr_*; ops_eval.mr_*; daliid_amd.evaluate) against the reference's
golden (tests/golden/metarec.npz) and against the numpy twin of the contract (tests/metarec_ref.py), both at the bounds of
tests/metarec_checks.py; the kill exactly; the fused kernel against mr_wscore + torch arithmetic; run-to-run identity; error paths; the
mirror classes; the switch of evaluateCleanATModels.validate.  Every comparison prints its distances before it asserts."""
import functools

import numpy as np
import pytest
import torch

import metarec_ref as R
from conftest import load_golden
from metarec_checks import case, check_fit, check_fused, golden_cases

pytestmark = pytest.mark.gpu

# the fit kernel's forms (csrc/metarec.hip): a wave per row up to n = 1024, a 256-thread workgroup up to 4096, 1024 threads beyond
N_WAVE, N_QUAD = 1024, 4096


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from daliid_amd import _lib, evaluate, ops_eval
    return ops_eval, evaluate, _lib


@pytest.fixture(scope="module")
def golden():
    return load_golden("metarec.npz")


def make_scores(nq, ng, seed, kind="cos"):
    g = np.random.default_rng(seed)
    if kind == "quant":                             # multiples of 1/8: ties cross the kill boundary and the tail boundary
        return (np.round(g.uniform(-1, 1, (nq, ng)) * 8) / 8).astype(np.float32)
    if kind == "neg":
        return g.uniform(-0.95, -0.05, (nq, ng)).astype(np.float32)
    d = 32
    unit = lambda x: x / np.linalg.norm(x, axis=1, keepdims=True)
    q, gal = unit(g.standard_normal((nq, d))), unit(g.standard_normal((ng, d)))
    for i in range(min(nq, ng)):                    # planted matches
        gal[i] = unit((q[i] + 0.6 * g.standard_normal(d) / d ** 0.5)[None])[0]
    return (q @ gal.T).astype(np.float32)


# (nq = n of the fit, ng, topk, use_columns, killscale, kind): n not a multiple of a wave, a workgroup or a transpose tile; one n just
# past each boundary between the fit kernel's forms; one long thin problem
TWIN_CASES = [(5, 7, 2, False, 1.0, "cos"), (63, 33, 5, True, 1.0, "cos"), (64, 130, 20, False, 1.0, "cos"), (65, 7, 20, True, 0.5, "cos"),
              (64, 33, 5, False, 0.5, "quant"), (257, 33, 20, False, 1.0, "quant"), (257, 33, 20, True, 1.0, "quant"),
              (1100, 7, 5, False, 1.0, "neg"), (1100, 130, 20, True, 1.0, "cos"), (N_WAVE + 1, 7, 5, False, 1.0, "cos"),
              (N_QUAD + 1, 7, 20, True, 1.0, "cos"), (5000, 24, 20, False, 1.0, "cos")]


@functools.lru_cache(maxsize=None)
def twin(nq, ng, topk, cols, ks, kind):
    S = make_scores(nq, ng, 1000 + nq + ng, kind)
    KT = R.kill_transpose(S, topk, cols, ks)
    fits, small, n_unfit, iters = R.fit_rows(KT, nq - topk - 1)
    for a in (S, KT, fits, small):
        a.setflags(write=False)
    return S, KT, fits, small, n_unfit, R.wscore(S, fits, small)


def gpu_metarec(ops_eval, S, topk, cols, ks):
    """-> (KT, fits, small, n_unfit, w) as numpy, through the three wrappers"""
    s = torch.tensor(S).cuda()                      # (a copy: the twin's arrays are read-only)
    kt = ops_eval.mr_kill_transpose(s, topk, use_columns=cols, killscale=ks)
    fits, small, n_unfit = ops_eval.mr_fit_rows(kt, S.shape[0] - topk - 1)
    w = ops_eval.mr_wscore(s, fits, small)
    return kt.cpu().numpy(), fits.cpu().numpy(), small.cpu().numpy(), n_unfit, w.cpu().numpy()


def test_gpu_matches_reference_golden(mods, golden):
    ops_eval = mods[0]
    for name in golden_cases(golden):
        c = case(golden, name)
        for a in range(c["m"]):
            _, fits, small, n_unfit, w = gpu_metarec(ops_eval, c["S"][a], c["topk"], c["use_columns"], c["killscale"])
            assert n_unfit == 0
            check_fit((fits, small, w), (c["fits"][a], c["small"][a], c["w"][a]), "golden %s model %d" % (name, a))
        if c["fused"] is not None:
            mats = [torch.from_numpy(s).cuda() for s in c["S"]]
            fused = ops_eval.mr_fuse(mats, topk=c["topk"], use_columns=c["use_columns"], killscale=c["killscale"], out_dtype=torch.float64)
            check_fused(fused.cpu().numpy(), c["fused"], sum(c["w"]), "golden " + name)


@pytest.mark.parametrize("nq,ng,topk,cols,ks,kind", TWIN_CASES)
def test_gpu_matches_twin(mods, nq, ng, topk, cols, ks, kind):
    ops_eval = mods[0]
    S, KT0, fits0, small0, n_unfit0, w0 = twin(nq, ng, topk, cols, ks, kind)
    KT, fits, small, n_unfit, w = gpu_metarec(ops_eval, S, topk, cols, ks)
    assert KT.shape == (ng, nq) and np.array_equal(KT, KT0), "kill + transpose differs from the twin"
    assert np.array_equal(np.signbit(KT), np.signbit(KT0))
    assert n_unfit == n_unfit0
    check_fit((fits, small, w), (fits0, small0, w0), "twin %s" % ((nq, ng, topk, cols, ks, kind),))


def test_fuse_matches_twin_and_wscore_arithmetic(mods):
    """Three models at 65 x 33 (the second with an unfit constant column): fused against the twin, and the fused kernel with fp64 and
    fp32 output against mr_wscore + torch arithmetic on the same fits."""
    ops_eval = mods[0]
    mats = [make_scores(65, 33, 7 + a, kind) for a, kind in enumerate(("cos", "cos", "quant"))]
    mats[1][:, 4] = -0.875                          # never among a row's five largest: the column stays constant after the kill
    fused0, sum_w0 = R.mrfuse(mats, topk=5, use_columns=False)
    dev = [torch.from_numpy(m).cuda() for m in mats]
    fused64 = ops_eval.mr_fuse(dev, topk=5, out_dtype=torch.float64)
    check_fused(fused64.cpu().numpy(), fused0, sum_w0, "twin 65 x 33 x 3")
    fits, smalls, ws = [], [], []
    for s in dev:
        f, sm, _ = ops_eval.mr_fit_rows(ops_eval.mr_kill_transpose(s, 5), 65 - 5 - 1)
        fits.append(f); smalls.append(sm); ws.append(ops_eval.mr_wscore(s, f, sm))
    assert torch.isnan(fits[1][4]).all() and bool((ws[1][:, 4] == 0).all())
    for m in (1, 2, 3):
        num = sum(w * s.double() for w, s in zip(ws[:m], dev[:m]))
        den = sum(ws[:m])
        ref = torch.where(den == 0, sum(s.double() for s in dev[:m]) / m, num / den)
        out64 = ops_eval.mr_fuse_fitted(dev[:m], fits[:m], smalls[:m], out_dtype=torch.float64)
        out32 = ops_eval.mr_fuse_fitted(dev[:m], fits[:m], smalls[:m], out_dtype=torch.float32)
        d = float((out64 - ref).abs().max())
        print("fuse m=%d against wscore arithmetic: %.3g" % (m, d))
        assert out64.dtype == torch.float64 and out32.dtype == torch.float32 and d <= 1e-12
        assert torch.equal(out32, out64.float())
    assert torch.equal(fused64, ops_eval.mr_fuse_fitted(dev, fits, smalls, out_dtype=torch.float64))


def test_all_unfit_falls_back_to_the_mean(mods):
    ops_eval = mods[0]
    dev = [torch.from_numpy(make_scores(9, 70, a)).cuda() for a in range(2)]
    nan = torch.full((70, 2), float("nan"), device="cuda", dtype=torch.float64)
    small = torch.zeros(70, device="cuda")
    out = ops_eval.mr_fuse_fitted(dev, [nan, nan], [small, small], out_dtype=torch.float64)
    assert torch.equal(out, (dev[0].double() + dev[1].double()) / 2)


def test_two_runs_are_identical(mods):
    ops_eval = mods[0]
    mats = [torch.from_numpy(make_scores(1100, 130, 40 + a)).cuda() for a in range(3)]

    def run():
        out = [ops_eval.mr_fuse(mats, topk=20, out_dtype=torch.float64)]
        for cols in (False, True):
            kt = ops_eval.mr_kill_transpose(mats[0], 20, use_columns=cols)
            fits, small, _, iters = ops_eval.mr_fit_rows(kt, 1100 - 21, return_iters=True)
            out += [kt, fits.view(torch.int64), small, iters]
        return out

    for a, b in zip(run(), run()):
        assert torch.equal(a, b)


def test_tail_of_one_is_unfit_everywhere(mods):
    ops_eval = mods[0]
    x = torch.from_numpy(make_scores(37, 100, 3)).cuda()                 # n - T + 1 = 100 <= 128
    fits, small, n_unfit = ops_eval.mr_fit_rows(x, 1)
    assert n_unfit == 37 and bool(torch.isnan(fits).all())
    assert torch.equal(small, x.max(dim=1).values)
    w = ops_eval.mr_wscore(x.t().contiguous(), fits, small)
    assert bool((w == 0).all())


def test_constant_column(mods):
    ops_eval = mods[0]
    S = make_scores(30, 6, 0)
    S[:, 2] = 0.375
    fits0, small0, n_unfit0 = R.metarec(S, 3, use_columns=True)
    _, fits, small, n_unfit, w = gpu_metarec(ops_eval, S, 3, True, 1.0)
    assert n_unfit == n_unfit0 == 1 and np.isnan(fits[2]).all() and np.isfinite(np.delete(fits, 2, 0)).all()
    assert (w[:, 2] == 0).all()
    check_fit((fits, small, w), (fits0, small0, R.wscore(S, fits0, small0)), "constant column")


def test_error_paths(mods):
    ops_eval, _, _lib = mods
    s = torch.from_numpy(make_scores(24, 40, 5)).cuda()
    with pytest.raises(_lib.DaliError, match="nq >= topk"):
        ops_eval.mr_kill_transpose(s, 23)                                # nq = 24 < topk + 2
    with pytest.raises(_lib.DaliError, match="entries per row"):
        ops_eval.mr_kill_transpose(s[:, :3].contiguous(), 5)             # ng = 3 < topk on the row axis
    with pytest.raises(_lib.DaliError, match="tail"):
        ops_eval.mr_fit_rows(s, 0)
    with pytest.raises(_lib.DaliError, match="tail"):
        ops_eval.mr_fit_rows(s, 41)
    wide = torch.from_numpy(make_scores(3, 200, 6)).cuda()
    with pytest.raises(_lib.DaliError, match="documented cap 128"):
        ops_eval.mr_fit_rows(wide, 200 - 128)                            # n - T + 1 = 129
    assert ops_eval.mr_fit_rows(wide, 200 - 127)[2] == 0                 # 128 is accepted
    with pytest.raises(_lib.DaliError, match="documented cap 16384"):
        ops_eval.mr_fit_rows(torch.zeros(1, 16385, device="cuda"), 16385 - 20)
    with pytest.raises(_lib.DaliError, match="contiguous"):
        ops_eval.mr_kill_transpose(s.t(), 5)
    with pytest.raises(_lib.DaliError, match="float32"):
        ops_eval.mr_fit_rows(s.double(), 10)
    with pytest.raises(ValueError, match="1 .. 3 models"):
        ops_eval.mr_fuse([s] * 4, topk=5)


def test_non_finite_score_sets_the_status(mods):
    ops_eval = mods[0]
    S = make_scores(40, 33, 8)
    for bad in (np.nan, np.inf):
        S[7, 11] = bad
        s = torch.from_numpy(S).cuda()
        with pytest.raises(ValueError, match="NaN or infinity"):
            ops_eval.mr_kill_transpose(s, 5)
        with pytest.raises(ValueError, match="NaN or infinity"):
            ops_eval.mr_fit_rows(s.t().contiguous(), 30)
        with pytest.raises(ValueError, match="NaN or infinity"):
            ops_eval.mr_fuse([s, s], topk=5)
    torch.cuda.synchronize()
    assert float(torch.ones(4, device="cuda").sum()) == 4.0


def test_longest_supported_row(mods):
    """n = 16384 fills the LDS row of the 1024-thread form."""
    ops_eval = mods[0]
    g = np.random.default_rng(9)
    x = g.uniform(0, 1, (3, 16384)).astype(np.float32)
    fits0, small0, n_unfit0, _ = R.fit_rows(x, 16384 - 21)
    fits, small, n_unfit = ops_eval.mr_fit_rows(torch.from_numpy(x).cuda(), 16384 - 21)
    fits, small = fits.cpu().numpy(), small.cpu().numpy()
    S = np.ascontiguousarray(x.T[:5])
    w = ops_eval.mr_wscore(torch.from_numpy(S).cuda(), torch.from_numpy(fits).cuda(), torch.from_numpy(small).cuda()).cpu().numpy()
    assert n_unfit == n_unfit0 == 0
    check_fit((fits, small, w), (fits0, small0, R.wscore(S, fits0, small0)), "n = 16384")


def test_mirror_classes(mods, golden):
    _, evaluate, _ = mods
    c = case(golden, "q72_g96_k20_three")
    fused = evaluate.Meta_Recognition().mrfuse(*[torch.from_numpy(s) for s in c["S"]])          # CPU tensors in, numpy out
    assert isinstance(fused, np.ndarray) and fused.dtype == np.float64 and fused.shape == (72, 96)
    check_fused(fused, c["fused"], sum(c["w"]), "mirror mrfuse")
    c = case(golden, "q64_g40_k20_cols")
    mr = evaluate.Meta_Recognition()
    w = mr.metarec(torch.from_numpy(c["S"][0]), 20)                                             # use_columns defaults to True
    assert w.dtype == torch.float64 and not w.is_cuda and tuple(w.shape) == (64, 40)
    assert tuple(mr.mr.wbFits.shape) == (40, 2) and tuple(mr.mr.smallScoreTensor.shape) == (40, 1)
    check_fit((mr.mr.wbFits.numpy(), mr.mr.smallScoreTensor[:, 0].numpy(), w.numpy()), (c["fits"][0], c["small"][0], c["w"][0]), "mirror metarec")
    w_dev = mr.metarec(torch.from_numpy(c["S"][0]).cuda(), 20, True, 1)                         # device tensors stay on the device
    assert w_dev.is_cuda and torch.equal(w_dev.cpu(), w)
    p = mr.mr.return_all_parameters()
    assert torch.equal(p["Shape"], mr.mr.wbFits[:, 0]) and torch.equal(p["Scale"], mr.mr.wbFits[:, 1]) and p["signTensor"] == 1
    mr.mr.tocpu()
    assert not mr.mr.wbFits.is_cuda and not mr.mr.smallScoreTensor.is_cuda
    assert torch.equal(mr.mr.wscore(torch.from_numpy(c["S"][0]), isReversed=True), 1 - w)
    w1 = mr.mr.wscore(torch.from_numpy(c["S"][0][0]))                                           # 1-D: repeated once per Weibull
    assert tuple(w1.shape) == (40, 40) and torch.equal(w1, w[0].repeat(40, 1))
    for call in (lambda: evaluate.libmr().FitLow(torch.zeros(2, 8), 3), lambda: evaluate.libmr(saved_model={"Scale": torch.ones(1)})):
        with pytest.raises(NotImplementedError, match="out of scope"):
            call()


def test_validate_switch_adds_one_entry(mods):
    """The small synthetic two-model setup of tests/test_gpu_fusion.py, with enough queries for mrfuse's topk = 20."""
    from daliid_amd import Encoders, evaluateCleanATModels as FUS, synthetic
    data = synthetic.SyntheticImages(n_ids=6, per_id=8, n_cams=3, seed=11, noise=0.4).install()
    try:
        nets = [Encoders._DataParallelShim(Encoders.ResNet50ReID(layers=(1, 1, 1, 1), width=32, seed=s)).eval() for s in (1, 2)]
        _, gallery, queries = data.split(4)
        assert len(queries) == 24 and len(gallery) == 24
        plain = FUS.validate(queries, gallery, nets[0], nets[1], 64, 32, [0], verbose=False)
        with_mr = FUS.validate(queries, gallery, nets[0], nets[1], 64, 32, [0], verbose=False, meta_recognition=True)
        assert set(with_mr) - set(plain) == {"ensemble_mr"} and set(plain) <= set(with_mr)
        for name, (cmc, mAP) in plain.items():
            assert np.array_equal(cmc, with_mr[name][0]) and mAP == with_mr[name][1], name
        cmc, mAP = with_mr["ensemble_mr"]
        assert 0.0 < mAP <= 1.0 and np.all(np.diff(cmc) >= 0)
    finally:
        synthetic.SyntheticImages.uninstall()
