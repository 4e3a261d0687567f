"""GPU: k-reciprocal re-ranking (dali_rerank / ops_eval.re_ranking / validate(rerank=True)) against the numpy restatement of its
definition (tests/rerank_ref.py, pinned by tests/test_rerank_cpu.py).

Both sides start from the same fp32 blocks and form C with the same IEEE operations (x * x, then division by the column maximum), so C
is bitwise equal on both sides and the neighbour sets are the same sets.  What remains are rounding differences of the arithmetic on
top: expf (the device's and numpy's may differ by 1 ulp), carried through the normalisation, the query expansion and the Jaccard
sums, which run in the same order on both sides.  On values <= 1 that stayed below 3e-7 in every case; the bound is 2e-6, tighter
than the 1e-5 the definition allows."""
import ctypes

import numpy as np
import pytest
import torch

import rerank_ref as RR

pytestmark = pytest.mark.gpu

F32 = np.float32
TOL = 2e-6


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _coprime_multipliers(N, rng, n):
    from math import gcd
    cands = [m for m in range(2, max(3, 4 * N)) if gcd(m, N) == 1 and m % N != 1]
    return [int(cands[k]) for k in rng.choice(len(cands), n, replace=False)]


def _designed_blocks(nq, ng, seed):
    """Blocks whose every column of A holds N distinct values, spaced so that the order at every position is decided by a gap far above
    fp32 rounding: each region (q_q, q_g, g_g) draws from its own third of a shuffled grid of 3N levels in [0.1, 1), indexed by
    (a*i + b*j) mod N with multipliers coprime to N; the diagonals of q_q and g_g are 0.  q_q and g_g are not symmetric, so
    reciprocity holds for some neighbours and not for others."""
    N = nq + ng
    rng = np.random.default_rng(seed)
    levels = 0.1 + 0.9 * rng.permutation(3 * N) / (3 * N)
    L_qq, L_qg, L_gg = levels[:N], levels[N:2 * N], levels[2 * N:]
    a, b, c, d, e, f = _coprime_multipliers(N, rng, 6)
    qi, gi = np.arange(nq), np.arange(ng)
    q_q = L_qq[(c * qi[None, :] + d * qi[:, None]) % N]
    q_g = L_qg[(a * qi[:, None] + b * gi[None, :]) % N]
    g_g = L_gg[(e * gi[None, :] + f * gi[:, None]) % N]
    np.fill_diagonal(q_q, 0.0)
    np.fill_diagonal(g_g, 0.0)
    return q_g.astype(F32), q_q.astype(F32), g_g.astype(F32)


def _assert_no_near_ties(q_g, q_q, g_g, k1, k2):
    C = RR.dense_C(q_g, q_q, g_g)
    gap = RR.tie_gaps(np.sort(C, axis=1)[:, :k1 + 2], k1, k2)
    assert gap > 1e-6, gap


def _run(dev, q_g, q_q, g_g, k1, k2, lam):
    from daliid_amd import ops_eval
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return ops_eval.re_ranking(t(q_g), t(q_q), t(g_g), k1=k1, k2=k2, lambda_value=lam)


SHAPES = [(1, 40), (37, 300), (300, 1031), (512, 4000)]
VARIANTS = [(20, 6, 0.3), (20, 1, 0.3), (5, 6, 0.3)]


@pytest.mark.parametrize("k1,k2,lam", VARIANTS, ids=["k1_20_k2_6", "k2_1", "k1_5"])
@pytest.mark.parametrize("nq,ng", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_matches_restatement_on_designed_blocks(dev, nq, ng, k1, k2, lam):
    q_g, q_q, g_g = _designed_blocks(nq, ng, seed=nq * 7 + ng)
    _assert_no_near_ties(q_g, q_q, g_g, k1, k2)
    out = _run(dev, q_g, q_q, g_g, k1, k2, lam)
    ref = RR.re_ranking_ref(q_g, q_q, g_g, k1, k2, lam)
    assert out.dtype == torch.float32 and tuple(out.shape) == (nq, ng)
    err = float(np.abs(out.cpu().numpy() - ref).max())
    print("%dx%d k1=%d k2=%d: max |hip - ref| = %.3g" % (nq, ng, k1, k2, err))
    assert err <= TOL, err
    assert float(np.abs(ref - RR.re_ranking_ref(q_g, q_q, g_g, k1, k2, 1.0)).max()) > 0.05      # the Jaccard term is not trivial


def test_matches_restatement_on_feature_distances(dev):
    """Blocks of the distance kernel on clustered features (not bitwise symmetric): near-ties do occur in such rows; C is bitwise equal
    on both sides, so the neighbour sets still agree exactly."""
    from daliid_amd import ops_eval
    from oracle import evalrank as E
    q, g, *_ = E.synthetic_reid_set(60, 17, 5, 256, noise=1.2, seed=4)
    q, g = q.to(dev), g.to(dev)
    blocks = [ops_eval.pairdist(a, b, normalize=True) for a, b in ((q, g), (q, q), (g, g))]
    out = ops_eval.re_ranking(*blocks)
    ref = RR.re_ranking_ref(*[b.cpu().numpy() for b in blocks], 20, 6, 0.3)
    assert float(np.abs(out.cpu().numpy() - ref).max()) <= TOL
    # host inputs -> numpy out, the same numbers
    host = ops_eval.re_ranking(*[b.cpu().numpy() for b in blocks])
    assert isinstance(host, np.ndarray) and np.array_equal(host, out.cpu().numpy())
    host_t = ops_eval.re_ranking(*[b.cpu() for b in blocks])
    assert isinstance(host_t, np.ndarray) and np.array_equal(host_t, host)


def test_lambda_one_is_bitwise_the_normalised_block(dev):
    from daliid_amd import ops_eval
    gen = torch.Generator(device=dev).manual_seed(5)
    nq, ng = 130, 2100
    q_g = torch.rand(nq, ng, device=dev, generator=gen) * 2
    q_q = torch.rand(nq, nq, device=dev, generator=gen) * 2
    g_g = torch.rand(ng, ng, device=dev, generator=gen) * 2
    q_q[7, 3] = 5.0                                     # a query column whose max is in q_q, not in q_g's row
    out = ops_eval.re_ranking(q_g, q_q, g_g, lambda_value=1.0)
    colmax = torch.maximum((q_q * q_q).amax(dim=0), (q_g * q_g).amax(dim=1))
    assert torch.equal(out, (q_g * q_g) / colmax[:, None])


def test_bitwise_reproducible(dev):
    q_g, q_q, g_g = _designed_blocks(512, 4000, seed=3)
    a = _run(dev, q_g, q_q, g_g, 20, 6, 0.3)
    b = _run(dev, q_g, q_q, g_g, 20, 6, 0.3)
    assert torch.equal(a, b)


def test_guards_return_errors_and_launch_nothing(dev):
    from daliid_amd import _lib, ops_eval
    L = _lib.lib()
    nq, ng = 4, 30
    q_g, q_q, g_g = [torch.rand(*s, device=dev) for s in ((nq, ng), (nq, nq), (ng, ng))]
    out = torch.full((nq, ng), -7.0, device=dev)

    def call(nq_, ng_, k1, k2, lam, q_g_=q_g):
        return L.dali_rerank(_lib.ctx(dev), _lib.stream_ptr(), _lib.ptr(q_g_), _lib.ptr(q_q), _lib.ptr(g_g), nq_, ng_, k1, k2,
                             ctypes.c_double(lam), _lib.ptr(out))

    assert call(0, ng, 5, 2, 0.3) == -1                           # DALI_ERR_INVALID: empty query set
    assert call(nq, 0, 5, 2, 0.3) == -1
    assert call(nq, ng, 0, 1, 0.3) == -1                          # k1 < 1
    assert call(nq, ng, 5, 7, 0.3) == -1                          # k2 > k1 + 1
    assert call(nq, ng, 5, 0, 0.3) == -1                          # k2 < 1
    assert call(nq, ng, 34, 2, 0.3) == -1                         # k1 + 1 > N = 34
    assert call(nq, ng, 5, 2, 1.5) == -1 and call(nq, ng, 5, 2, -0.1) == -1
    assert call(nq, ng, 5, 2, 0.3, q_g_=None) == -1               # null block
    big = [torch.rand(*s, device=dev) for s in ((8, 100), (8, 8), (100, 100))]
    assert L.dali_rerank(_lib.ctx(dev), _lib.stream_ptr(), *[_lib.ptr(b) for b in big], 8, 100, 64, 2, ctypes.c_double(0.3),
                         _lib.ptr(out)) == -4                     # DALI_ERR_LIMIT: k1 above the cap 63
    assert "cap" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())                              # nothing was launched
    with pytest.raises(ValueError):
        ops_eval.re_ranking(q_g, q_q, g_g[:, :-1])
    with pytest.raises(_lib.DaliError):
        ops_eval.re_ranking(q_g, q_q, g_g, k1=20, k2=22)
    with pytest.raises(_lib.DaliError):
        ops_eval.re_ranking(*big, k1=ops_eval.RERANK_K1_MAX + 1, k2=2)
    # the cap itself runs
    assert torch.isfinite(ops_eval.re_ranking(*big, k1=ops_eval.RERANK_K1_MAX, k2=ops_eval.RERANK_K1_MAX + 1)).all()


# ---- a gallery past 46,340 rows: 64-bit offsets into g_g and the accumulator outside LDS ----

def _cluster_features(nq, ng, dev):
    """N = 21 * n_clusters unit rows in clusters of exactly k1 + 1 = 21: member m of a cluster sits at angle 1.3 (m / 20)^1.25 in the
    cluster's own 2-D plane (planes orthogonal), so every row's first 21 neighbours are its cluster (d = 1 to every other row) and
    the positions h / h + 1 and k2 - 1 / k2 inside it are decided by gaps of >= 1.2e-4 in C."""
    N = nq + ng
    assert N % 21 == 0
    n_cl = N // 21
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(17))
    cl, mem = perm // 21, perm % 21
    theta = 1.3 * (mem.double() / 20.0) ** 1.25
    x = torch.zeros(N, 2 * n_cl, dtype=torch.float32)
    rows = torch.arange(N)
    x[rows, 2 * cl] = torch.cos(theta).float()
    x[rows, 2 * cl + 1] = torch.sin(theta).float()
    return x[:nq].to(dev), x[nq:].to(dev)


def _device_checker(q_g, q_q, g_g, K, chunk=1024):
    """colmax, and R[:, :K] + the sorted C values [:, :K + 1] from a chunked stable torch.sort of the rows of C on the device."""
    nq, ng = q_g.shape
    N = nq + ng
    gmax = torch.zeros(ng, device=q_g.device)
    for r in range(0, ng, chunk):
        gmax = torch.maximum(gmax, (g_g[r:r + chunk] * g_g[r:r + chunk]).amax(dim=0))
    colmax = torch.cat([torch.maximum((q_q * q_q).amax(dim=0), (q_g * q_g).amax(dim=1)),
                        torch.maximum((q_g * q_g).amax(dim=0), gmax)])
    R = torch.empty(N, K, dtype=torch.int64)
    S = torch.empty(N, K + 1, dtype=torch.float64)
    colA = torch.cat([q_q, q_g.t()], dim=0)                      # columns of A for the query columns: [q_q[:, i]; q_g[i, :]]
    for c0 in range(0, N, chunk):
        c1 = min(N, c0 + chunk)
        parts = [colA[:, c0:min(c1, nq)]] if c0 < nq else []
        if c1 > nq:
            g0, g1 = max(c0, nq) - nq, c1 - nq
            parts.append(torch.cat([q_g[:, g0:g1], g_g[:, g0:g1]], dim=0))
        cols = torch.cat(parts, dim=1)
        a = cols * cols
        C = (a / colmax[c0:c1][None, :]).t().contiguous()
        vals, idx = torch.sort(C, dim=1, stable=True)
        R[c0:c1] = idx[:, :K].cpu()
        S[c0:c1] = vals[:, :K + 1].double().cpu()
    return colmax.cpu().numpy(), R.numpy(), S.numpy()


def test_large_gallery_matches_restatement(dev):
    from daliid_amd import ops_eval
    nq, ng, k1, k2, lam = 32, 46420, 20, 6, 0.3
    assert ng > 46340 and ng * ng > 2 ** 31
    q, g = _cluster_features(nq, ng, dev)
    q_g = ops_eval.pairdist(q, g, normalize=True)
    q_q = ops_eval.pairdist(q, q, normalize=True)
    g_g = ops_eval.pairdist(g, g, normalize=True)
    del q, g
    out = ops_eval.re_ranking(q_g, q_q, g_g, k1, k2, lam)
    colmax, R, S = _device_checker(q_g, q_q, g_g, k1 + 1)
    assert RR.tie_gaps(S, k1, k2) > 1e-6
    qq_flat, qg_flat, gg_flat = q_q.reshape(-1), q_g.reshape(-1), g_g.reshape(-1)

    def full_at(rows, cols):
        r = torch.from_numpy(np.asarray(rows, np.int64)).to(dev)
        c = torch.from_numpy(np.asarray(cols, np.int64)).to(dev)
        v = torch.empty(r.numel(), device=dev)
        for m, flat, off in (((r < nq) & (c < nq), qq_flat, lambda r, c: r * nq + c),
                             ((r < nq) & (c >= nq), qg_flat, lambda r, c: r * ng + (c - nq)),
                             ((r >= nq) & (c < nq), qg_flat, lambda r, c: c * ng + (r - nq)),
                             ((r >= nq) & (c >= nq), gg_flat, lambda r, c: (r - nq) * ng + (c - nq))):
            v[m] = flat[off(r[m], c[m])]
        return v.cpu().numpy()

    ref = RR.re_ranking_ref(q_g.cpu().numpy(), None, None, k1, k2, lam, R=R, colmax=colmax, full_at=full_at)
    err = float(np.abs(out.cpu().numpy() - ref).max())
    print("32 x %d: max |hip - ref| = %.3g" % (ng, err))
    assert err <= TOL, err
    assert float(ref.min()) < 0.5                                 # cluster mates are pulled in by the Jaccard term


# ---- end to end through the validator ----

@pytest.fixture(scope="module")
def env(dev):
    from daliid_amd import Encoders, synthetic, validateModels, getFeatures
    data = synthetic.SyntheticImages(n_ids=8, per_id=6, n_cams=3, seed=5, noise=0.4).install()
    yield Encoders, data, validateModels, getFeatures
    synthetic.SyntheticImages.uninstall()


def test_validate_rerank_matches_restatement_and_oracle(env, capsys):
    from oracle import evalrank as E
    Encoders, data, V, G = env
    online = Encoders._DataParallelShim(Encoders.ResNet50ReID(layers=(1, 1, 1, 1), width=32, seed=9)).eval()
    _, gallery, query = data.split(1)
    validator = V.validationManager.getValidator("Market")
    validator.setParameters(64, 32, True, 0)
    cmc, mAP, distmat = validator.validate(query, gallery, online)
    assert "Applying person re-ranking ..." in capsys.readouterr().out
    assert distmat.is_cuda and tuple(distmat.shape) == (len(query), len(gallery))
    # the validator's own three blocks
    q = G.extractFeatures(query, 64, 32, online, 500, 0, keep_on_device=True)
    g = G.extractFeatures(gallery, 64, 32, online, 500, 0, keep_on_device=True)
    blocks = [validator.distance(a, b).cpu().numpy() for a, b in ((q, g), (q, q), (g, g))]
    ref = RR.re_ranking_ref(*blocks, 20, 6, 0.3)
    assert float(np.abs(distmat.cpu().numpy() - ref).max()) <= TOL
    ref_cmc, ref_map = E.eval_market1501(distmat.cpu().numpy(), query[:, 1], gallery[:, 1], query[:, 2], gallery[:, 2])
    assert abs(mAP - ref_map) < 1e-4
    np.testing.assert_allclose(cmc, ref_cmc, atol=1.0 / len(query) + 1e-6)
    # the plain matrix is not what came back
    assert float((distmat - validator.distance(q, g)).abs().max()) > 1e-3
    # distmat_on_cpu is honoured
    validator.distmat_on_cpu = True
    _, mAP2, d_cpu = validator.validate(query, gallery, online)
    assert d_cpu.device.type == "cpu" and torch.equal(d_cpu, distmat.cpu()) and mAP2 == mAP
    # sharded evaluation refuses re-ranking
    with pytest.raises(NotImplementedError):
        validator.validate_sharded(query, gallery, online)
