"""GPU: the pair ROC (dali_roc_build / dali_roc_emit, ops_eval.roc_curve / roc_counts / verification_metrics, the mirror's
calculateMetrics(pooling=...)) against the numpy restatement of its definition (tests/roc_ref.py, pinned to sklearn 1.7.2 by
tests/test_roc_cpu.py) bit for bit, and at 1e9 pairs against an independent restatement on the device (torch.sort)."""
import os
import warnings

import numpy as np
import pytest
import torch

import roc_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _same(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


def _check(d, qp, gp, what):
    from daliid_amd import ops_eval
    for drop in (True, False):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = R.roc_curve(d.cpu().numpy() if isinstance(d, torch.Tensor) else d, qp, gp, drop_intermediate=drop)
            got = ops_eval.roc_curve(d, qp, gp, drop_intermediate=drop)
        for k, (a, b) in enumerate(zip(got, want)):
            _same(a, b, "%s drop=%s output %d" % (what, drop, k))


def test_goldens(dev):
    z = load_golden("roc.npz")
    from daliid_amd import ops_eval
    for name in sorted({k.split("/")[0] for k in z.files}):
        d, qp, gp = z[name + "/distmat"], z[name + "/q_ids"], z[name + "/g_ids"]
        for drop, tag in ((True, "drop"), (False, "all")):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                got = ops_eval.roc_curve(torch.from_numpy(d).to(dev), qp, gp, drop_intermediate=drop)
            for k, key in enumerate(("fpr", "tpr", "thr")):
                _same(got[k], z["%s/%s_%s" % (name, key, tag)], "%s %s %s" % (name, key, tag))


@pytest.mark.parametrize("nq,ng", [(1, 1), (1, 517), (433, 1), (37, 301), (130, 1024), (97, 1023), (3, 8191), (129, 65)])
def test_shapes(dev, nq, ng):
    rng = np.random.default_rng(nq * 7919 + ng)
    d = torch.from_numpy(rng.uniform(0, 2, (nq, ng)).astype(F32)).to(dev)
    _check(d, rng.integers(0, 5, nq), rng.integers(0, 5, ng), "%dx%d" % (nq, ng))


def test_host_input(dev):
    rng = np.random.default_rng(5)
    d = rng.uniform(0, 2, (20, 50))                          # float64 host array: converted to fp32 first
    _check(d.astype(F32), rng.integers(0, 3, 20), rng.integers(0, 3, 50), "host")
    from daliid_amd import ops_eval
    a = ops_eval.roc_curve(d, np.arange(20) % 3, np.arange(50) % 3)
    b = R.roc_curve(d.astype(F32), np.arange(20) % 3, np.arange(50) % 3)
    for x, y in zip(a, b):
        _same(x, y, "float64 host")


def test_quantised_ties(dev):
    rng = np.random.default_rng(11)
    nq, ng = 300, 2000
    d = torch.from_numpy((rng.integers(0, 256, (nq, ng)) / 128.0).astype(F32)).to(dev)
    _check(d, rng.integers(0, 7, nq), rng.integers(0, 7, ng), "256 levels")


def test_many_binades(dev):
    rng = np.random.default_rng(12)
    nq, ng = 200, 3000
    mag = np.exp2(rng.uniform(-120, 120, (nq, ng)))
    d = (rng.choice([-1.0, 1.0], (nq, ng)) * mag).astype(F32)
    d[0, :10] = [0, -0.0, 2, 1e38, -1e38, 3e-39, -3e-39, 1.0, 2.0, 2.0]
    _check(torch.from_numpy(d).to(dev), rng.integers(0, 4, nq), rng.integers(0, 4, ng), "binades")


def test_market_shape_features(dev):
    from daliid_amd import ops_eval
    from oracle import evalrank as E
    q, g, qp, gp, _, _ = E.synthetic_reid_set(752, 22, 5, 256, noise=1.0, seed=3)
    d = ops_eval.pairdist(q[:3368].to(dev), g[:15913].to(dev), normalize=True)
    assert tuple(d.shape) == (3368, 15913)
    _check(d, qp[:3368], gp[:15913], "market")


def test_deterministic_and_verification(dev):
    from daliid_amd import ops_eval
    rng = np.random.default_rng(21)
    d = torch.from_numpy((rng.integers(0, 64, (150, 900)) / 32.0).astype(F32)).to(dev)
    qp, gp = rng.integers(0, 6, 150), rng.integers(0, 6, 900)
    a = [t.cpu().numpy() for t in ops_eval.roc_counts(d, qp, gp)]
    b = [t.cpu().numpy() for t in ops_eval.roc_counts(d, qp, gp)]
    for x, y in zip(a, b):
        _same(x, y, "rerun")
    got = ops_eval.verification_metrics(d, qp, gp, fars=(0.5, 0.1, 1e-2, 1e-4))
    want = R.verification_metrics(d.cpu().numpy(), qp, gp, fars=(0.5, 0.1, 1e-2, 1e-4))
    assert got["n_pos"] == want["n_pos"] and got["n_neg"] == want["n_neg"]
    assert got["auc"] == want["auc"] and got["eer"] == want["eer"] and got["eer_threshold"] == want["eer_threshold"]
    for f in (0.5, 0.1, 1e-2, 1e-4):
        np.testing.assert_array_equal(got["tar_at_far"][f], want["tar_at_far"][f])


def test_errors(dev):
    import ctypes
    from daliid_amd import _lib, ops_eval
    d = torch.zeros(4, 5, device=dev)
    d[2, 3] = float("nan")
    with pytest.raises(ValueError):
        ops_eval.roc_curve(d, np.arange(4), np.arange(5))
    with pytest.raises(ValueError):
        ops_eval.roc_curve(torch.zeros(4, 5, device=dev), np.arange(3), np.arange(5))
    with pytest.raises(_lib.DaliError):
        ops_eval.roc_curve(torch.zeros(1, device=dev).expand(65536, 32768), np.zeros(65536), np.zeros(32768))
    L = _lib.lib()
    assert L.dali_roc_scratch_bytes(65536, 32768) == 0
    buf = torch.zeros(64, device=dev, dtype=torch.int64)
    st = L.dali_roc_build(_lib.ctx(dev), _lib.stream_ptr(), _lib.ptr(d), _lib.ptr(buf), _lib.ptr(buf), 65536, 32768, _lib.ptr(buf), 512,
                          _lib.ptr(buf))
    assert st == -4                                         # DALI_ERR_LIMIT before anything is read


def test_mirror_pooling_writes_the_reference_files(dev, tmp_path, monkeypatch):
    from daliid_amd import evaluateCleanATModels as M
    from oracle import evalrank as E
    q, g, qp, gp, qc, gc = E.synthetic_reid_set(20, 10, 2, 64, noise=2.0, seed=4)
    from daliid_amd import ops_eval
    d = ops_eval.pairdist(q.to(dev), g.to(dev), normalize=True)
    qi = np.stack([np.zeros(len(qp)), np.asarray(qp), np.asarray(qc)], 1).astype(str)
    gi = np.stack([np.zeros(len(gp)), np.asarray(gp), np.asarray(gc)], 1).astype(str)
    monkeypatch.chdir(tmp_path)
    cmc0, map0 = M.calculateMetrics(qi, gi, d, verbose=False)
    assert not os.listdir(tmp_path)
    cmc1, map1 = M.calculateMetrics(qi, gi, d, pooling="gap", version="t", verbose=False)
    assert map0 == map1 and np.array_equal(cmc0, cmc1)
    want = R.roc_curve(d.cpu().numpy(), qi[:, 1], gi[:, 1])
    for name, w in zip(("FPR_t.npy", "TPR_t.npy", "Thresholds_t.npy"), want):
        _same(np.load(tmp_path / name), w, name)


def _device_restatement(d, qp, gp, drop):
    """(thresholds, fps, tps) without the leading point, by torch.sort on the device; frees as it goes."""
    ng = d.shape[1]
    s = 1.0 - d.reshape(-1) / 2.0
    s, idx = torch.sort(s, descending=True)
    y = qp[idx // ng] == gp[idx % ng]
    del idx
    tps = torch.cumsum(y, 0)
    del y
    uniq, cnt = torch.unique_consecutive(s, return_counts=True)
    del s
    ends = torch.cumsum(cnt, 0) - 1
    del cnt
    tps = tps[ends]
    fps = ends + 1 - tps
    del ends
    if drop and uniq.numel() > 2:
        keep = torch.ones(uniq.numel(), dtype=torch.bool, device=d.device)
        keep[1:-1] = (torch.diff(fps, 2) != 0) | (torch.diff(tps, 2) != 0)
        uniq, fps, tps = uniq[keep], fps[keep], tps[keep]
    return uniq, fps, tps


@pytest.mark.parametrize("tied", [False, True])
def test_configs4_1e9_pairs(dev, tied):
    """10,000 x 100,000 (configs[4]): realistic feature distances, and the all-tied matrix (a 2-point curve)."""
    from daliid_amd import ops_eval
    nq, ng = 10000, 100000
    gen = torch.Generator(device=dev).manual_seed(9)
    qp = torch.randint(0, 2000, (nq,), device=dev, generator=gen, dtype=torch.int32)
    gp = torch.randint(0, 2000, (ng,), device=dev, generator=gen, dtype=torch.int32)
    if tied:
        d = torch.full((nq, ng), 0.7, device=dev)
    else:
        f = torch.randn(2000, 256, device=dev, generator=gen)
        q = f[qp.long()] + 1.2 * torch.randn(nq, 256, device=dev, generator=gen)
        g = f[gp.long()] + 1.2 * torch.randn(ng, 256, device=dev, generator=gen)
        d = ops_eval.pairdist(q, g, normalize=True)
        del q, g, f
    qn, gn = qp.cpu().numpy(), gp.cpu().numpy()
    for drop in (True, False):
        thr, fps, tps = ops_eval.roc_counts(d, qn, gn, drop_intermediate=drop)
        w_thr, w_fps, w_tps = _device_restatement(d, qp, gp, drop)
        if tied:
            assert thr.numel() == 2
        assert torch.equal(thr[1:], w_thr) and torch.equal(fps[1:], w_fps) and torch.equal(tps[1:], w_tps), drop
        assert thr[0].item() == float("inf") and fps[0].item() == 0 and tps[0].item() == 0
        del thr, fps, tps, w_thr, w_fps, w_tps
        torch.cuda.empty_cache()
    print("peak device memory %.1f GB" % (torch.cuda.max_memory_allocated() / 1e9))
