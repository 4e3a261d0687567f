"""GPU: query expansion / database augmentation (ops_eval.qe_combine, ops_eval.query_expansion, validateModels.setQueryExpansion) against
tests/qe_ref.py: the combine kernel bit for bit against the float32 emulation of its arithmetic order, the wiring bit for bit against the
composition of the public pieces, and the whole against a float64 restatement within a bound derived from the reference's own numbers."""
import numpy as np
import pytest
import torch

import qe_ref as R
import topk_ref as T

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _case(rng, n, n_pool, d, k, val_is_distance):
    """pool rows of mixed scale; repeated indices inside a row; similarities of both signs with exact zeros (as distances: 0 .. 2 with
    exact 0 and exact 1, i.e. similarity 1 and 0)"""
    pool = (rng.standard_normal((n_pool, d)) * rng.uniform(0.5, 2, (n_pool, 1))).astype(F32)
    idx = rng.integers(0, n_pool, (n, k)).astype(np.int32)
    if k >= 2:
        idx[:, 1] = idx[:, 0]
    if val_is_distance:
        val = rng.uniform(0, 2, (n, k)).astype(F32)
        val[rng.random((n, k)) < 0.1] = 1.0
        val[rng.random((n, k)) < 0.1] = 0.0
    else:
        val = rng.uniform(-1, 1, (n, k)).astype(F32)
        val[rng.random((n, k)) < 0.1] = 0.0
    return pool, idx, val


def _pool_on_device(dev, pool, misaligned):
    """a contiguous [n_pool, d] tensor; ``misaligned``: a view that starts 4 bytes into a 16-byte aligned buffer (the scalar path)"""
    if not misaligned:
        return torch.from_numpy(pool).to(dev)
    buf = torch.empty(pool.size + 1, device=dev, dtype=torch.float32)
    view = buf[1:].view(pool.shape)
    view.copy_(torch.from_numpy(pool))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


# (n, n_pool, d, k, alpha, val_is_distance, misaligned pool): every d, k, n and alpha of the issue at least twice, n_pool != n in half
COMBINE_CASES = [
    (1, 1, 1, 1, 0, False, False), (5, 5, 1, 2, 1, True, False), (257, 300, 1, 10, 2, False, False), (257, 257, 1, 128, 1, False, False),
    (1, 7, 3, 128, 3, True, False), (5, 9, 3, 1, 16, False, False), (257, 257, 3, 2, 0, True, False), (5, 12, 3, 10, 16, True, False),
    (1, 1, 4, 10, 1, False, False), (5, 33, 4, 128, 2, True, False), (257, 257, 4, 1, 3, False, False), (1, 2, 4, 2, 16, True, False),
    (5, 5, 4, 10, 3, True, False),
    (1, 64, 8, 2, 16, True, False), (5, 5, 8, 10, 0, False, False), (257, 100, 8, 128, 1, True, False), (1, 3, 8, 128, 2, False, False),
    (1, 1, 260, 1, 2, True, False), (5, 17, 260, 2, 3, False, False), (257, 257, 260, 10, 16, True, False), (257, 31, 260, 10, 0, True, False),
    (5, 5, 260, 1, 2, False, False),
    (1, 40, 2048, 128, 0, False, False), (5, 5, 2048, 1, 1, True, False), (257, 300, 2048, 2, 2, False, False), (5, 5, 2048, 10, 3, True, False),
    (257, 513, 2048, 128, 16, False, False), (1, 1, 2048, 2, 3, False, False),
    (5, 9, 8, 10, 3, False, True), (257, 257, 260, 2, 1, True, True), (5, 6, 2048, 10, 3, True, True),
]


@pytest.mark.parametrize("n,n_pool,d,k,alpha,vid,misaligned", COMBINE_CASES)
def test_qe_combine_bitwise(dev, n, n_pool, d, k, alpha, vid, misaligned):
    from daliid_amd import ops_eval
    rng = np.random.default_rng(n * 7 + n_pool * 11 + d * 13 + k * 17 + alpha)
    pool, idx, val = _case(rng, n, n_pool, d, k, vid)
    want = R.combine_f32(pool, idx, val, alpha, vid)
    got = ops_eval.qe_combine(_pool_on_device(dev, pool, misaligned), torch.from_numpy(idx).to(dev), torch.from_numpy(val).to(dev),
                              alpha=alpha, val_is_distance=vid)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, d)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))


def test_indices_outside_the_pool_are_skipped_and_reported(dev):
    """an index outside the pool is never turned into an address: its term is left out, the call raises, the next call is unaffected"""
    from daliid_amd import _lib, ops_eval
    rng = np.random.default_rng(3)
    n, n_pool, d, k = 9, 20, 260, 10
    pool, idx, val = _case(rng, n, n_pool, d, k, False)
    good = idx.copy()
    idx[2, 0], idx[2, 9], idx[6, 4], idx[6, 5] = -1, n_pool, np.iinfo(np.int32).max, np.iinfo(np.int32).min
    bad_rows = np.array([2, 6])
    pd, vd = torch.from_numpy(pool).to(dev), torch.from_numpy(val).to(dev)
    out = torch.full((n, d), 7.0, device=dev)
    with pytest.raises(_lib.DaliError, match="outside the pool"):
        ops_eval.qe_combine(pd, torch.from_numpy(idx).to(dev), vd, alpha=3, out=out)
    got, want = out.cpu().numpy(), R.combine_f32(pool, idx, val, 3, False)
    ok_rows = np.setdiff1d(np.arange(n), bad_rows)
    assert np.array_equal(_bits(got[ok_rows]), _bits(want[ok_rows]))
    assert np.array_equal(_bits(got[bad_rows]), _bits(want[bad_rows]))                  # the remaining terms, still divided by k
    again = ops_eval.qe_combine(pd, torch.from_numpy(good).to(dev), vd, alpha=3)
    assert np.array_equal(_bits(again.cpu().numpy()), _bits(R.combine_f32(pool, good, val, 3, False)))


def test_refusals_launch_nothing(dev):
    from daliid_amd import _lib, ops_eval
    rng = np.random.default_rng(4)
    pool, idx, val = _case(rng, 6, 6, 8, 4, False)
    pd = torch.from_numpy(pool).to(dev)
    mk = lambda k: (torch.zeros(6, k, device=dev, dtype=torch.int32), torch.ones(6, k, device=dev, dtype=torch.float32))
    out = torch.full((6, 8), 7.0, device=dev)
    for k in (0, 129):
        with pytest.raises(_lib.DaliError, match="k=%d" % k):
            ops_eval.qe_combine(pd, *mk(k), out=out)
    for alpha in (17, -1, 2.5):
        with pytest.raises(ValueError):
            ops_eval.qe_combine(pd, *mk(4), alpha=alpha, out=out)
    # the C entry itself refuses alpha = 17 and names it
    i4, v4 = mk(4)
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    rc = _lib.lib().dali_qe_combine(_lib.ctx(dev), _lib.stream_ptr(), _lib.ptr(pd), 6, 8, _lib.ptr(i4), _lib.ptr(v4), 6, 4, 0, 17, _lib.ptr(out), _lib.ptr(status))
    assert rc != 0 and "alpha=17" in _lib.last_error()
    rc = _lib.lib().dali_qe_combine(_lib.ctx(dev), _lib.stream_ptr(), _lib.ptr(pd), 6, 0, _lib.ptr(i4), _lib.ptr(v4), 6, 4, 0, 3, _lib.ptr(out), _lib.ptr(status))
    assert rc != 0 and "d=0" in _lib.last_error()
    rc = _lib.lib().dali_qe_combine(_lib.ctx(dev), _lib.stream_ptr(), _lib.ptr(pd), 6, 8, _lib.ptr(i4), _lib.ptr(v4), 6, 4, 0, 3, _lib.c_void_p(0), _lib.ptr(status))
    assert rc != 0 and "null" in _lib.last_error()
    # out aliasing pool: the same tensor, and a partial overlap inside one buffer
    with pytest.raises(_lib.DaliError, match="overlaps"):
        ops_eval.qe_combine(pd, *mk(4), out=pd)
    buf = torch.zeros(10, 8, device=dev)
    with pytest.raises(_lib.DaliError, match="overlaps"):
        ops_eval.qe_combine(buf[:6], *mk(4), out=buf[4:10])
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and int(status.item()) == 0 and np.array_equal(pd.cpu().numpy(), pool)
    # n == 0 launches nothing and returns an empty result
    empty = ops_eval.qe_combine(pd, torch.zeros(0, 4, device=dev, dtype=torch.int32), torch.zeros(0, 4, device=dev))
    assert tuple(empty.shape) == (0, 8)
    # query_expansion's own argument checks
    q, g = pd[:2], pd[2:]
    for kwargs, exc in ((dict(alpha=2.5), ValueError), (dict(alpha=17), ValueError), (dict(times=0), ValueError), (dict(times=9), ValueError),
                        (dict(k=0), ValueError), (dict(k=129), _lib.DaliError), (dict(expand="queries"), ValueError)):
        with pytest.raises(exc):
            ops_eval.query_expansion(q, g, **kwargs)
    with pytest.raises(ValueError, match="non-integer"):
        ops_eval.query_expansion(q, g, alpha=2.5)
    with pytest.raises(ValueError):
        ops_eval.query_expansion(q, g[:, :4].contiguous())


# ---- the data of the issue: 40 identities x 10 samples in 64 dimensions, rows of mixed scale, 80 queries + 320 gallery rows ----

def _clustered(seed):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((40, 64))
    x = np.repeat(centres, 10, axis=0) + 0.6 * rng.standard_normal((400, 64))
    x *= rng.uniform(0.5, 2, (400, 1))
    x = x[rng.permutation(400)].astype(F32)
    return x[:80], x[80:]


@pytest.mark.parametrize("expand", ["all", "gallery"])
@pytest.mark.parametrize("times", [1, 2])
def test_query_expansion_is_the_composition_of_the_public_pieces(dev, expand, times):
    from daliid_amd import ops_eval
    q, g = _clustered(7)
    qd, gd = torch.from_numpy(q).to(dev), torch.from_numpy(g).to(dev)
    g_before = gd.clone()
    q1, g1 = ops_eval.query_expansion(qd, gd, k=10, alpha=3.0, times=times, expand=expand)
    feat = np.concatenate([q, g]) if expand == "all" else g
    for _ in range(times):
        P = ops_eval.PreparedRows(torch.from_numpy(feat).to(dev), normalize=True, precision="bf16x3")
        dist, idx = ops_eval.pairdist_topk(P, P, 10, metric="cosine")
        feat = R.combine_f32(feat, idx.cpu().numpy(), dist.cpu().numpy(), 3, True)
    assert q1.dtype == g1.dtype == torch.float32 and q1.is_cuda and g1.is_cuda
    assert torch.equal(gd, g_before)                                                   # the caller's tensors are read only
    if expand == "all":
        assert np.array_equal(_bits(q1.cpu().numpy()), _bits(feat[:80])) and np.array_equal(_bits(g1.cpu().numpy()), _bits(feat[80:]))
    else:
        assert q1 is qd
        assert np.array_equal(_bits(g1.cpu().numpy()), _bits(feat))


DELTA = 8e-6          # bf16x3 cosine distances against fp32 at small d (tests/test_gpu_eval.py)


@pytest.mark.parametrize("k,times", [(4, 1), (7, 1), (10, 1), (16, 1), (10, 2)])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_query_expansion_against_float64(dev, seed, k, times):
    """Rows whose k-th / (k+1)-th similarities are closer than 1e-4 in any iteration of the reference are left out (their neighbour set
    may legitimately differ); at most 5 % may be.  For the others, with s_min,t the smallest top-k similarity of iteration t:
    E_0 = 0, E_t = E_{t-1} + alpha (DELTA + 2 E_{t-1}) / s_min,t + (k + 2) 2^-24 bounds the relative error of a weighted term (a weight
    s^alpha moves by alpha ds / s, ds = the distance error plus twice the features' own relative error; the k + 2 roundings of the
    combine), and |got - ref|_2 <= 4 E_times (1 / k) sum_j |w_j| |x_j|_2 per row.  Largest error / bound observed on an MI355X: 0.079
    (k = 4, seed 0; docs/experiments.md)."""
    from daliid_amd import ops_eval
    alpha = 3
    q, g = _clustered(seed)
    rq, rg, info = R.aqe_f64(q, g, k, alpha, times, "all")
    ref = np.concatenate([rq, rg])
    left_out = np.zeros(400, dtype=bool)
    E = 0.0
    for it in info:
        left_out |= it["gap"] < 1e-4
        E = E + alpha * (DELTA + 2 * E) / it["smin"].min() + (k + 2) * 2.0 ** -24
    assert left_out.sum() <= 0.05 * 400, left_out.sum()
    q1, g1 = ops_eval.query_expansion(torch.from_numpy(q).to(dev), torch.from_numpy(g).to(dev), k=k, alpha=float(alpha), times=times)
    got = torch.cat([q1, g1]).cpu().numpy().astype(np.float64)
    err = np.linalg.norm(got - ref, axis=1)
    bound = 4 * E * info[-1]["scale"]
    ratio = (err / bound)[~left_out]
    print("query_expansion seed=%d k=%d times=%d: left out %d rows, smallest top-k similarity %.3f, E=%.3g, largest error / bound = %.4f"
          % (seed, k, times, left_out.sum(), min(it["smin"].min() for it in info), E, ratio.max()))
    assert np.all(ratio <= 1.0), ratio.max()


# ---- validator ----

class _Model:
    def eval(self):
        return self


def _validator(dev, queries, gallery, qf, gf):
    from daliid_amd import validateModels as V
    v = V.validationManager.getValidator("Market")
    v.setParameters(64, 32, False, 0)
    v._features = lambda subset, model: (qf if subset is queries else gf).clone()
    return v


def test_validator_expands_before_the_distance(dev, capsys):
    from daliid_amd import ops_eval
    q, g = _clustered(11)
    rng = np.random.default_rng(11)
    rows = lambda n: np.stack([np.arange(n), rng.integers(0, 12, n), rng.integers(0, 3, n)], axis=1)
    queries, gallery = rows(80), rows(320)
    qf, gf = torch.from_numpy(q).to(dev), torch.from_numpy(g).to(dev)
    v = _validator(dev, queries, gallery, qf, gf)
    plain = v.distance(qf, gf)
    cmc0, map0, d0 = v.validate(queries, gallery, _Model())
    assert torch.equal(d0, plain)
    v.setQueryExpansion(k=5)
    cmc1, map1, d1 = v.validate(queries, gallery, _Model())
    want = v.distance(*ops_eval.query_expansion(qf, gf, k=5, alpha=3.0, times=1, expand="all", precision=v.precision))
    assert torch.equal(d1, want) and not torch.equal(d1, plain)
    indices, distances = v.retrieve_features(qf, gf, k=7)
    wv, wi = T.topk(want.cpu().numpy(), 7)
    assert np.array_equal(indices.cpu().numpy(), wi) and np.array_equal(_bits(distances.cpu().numpy()), _bits(wv))
    indices2, _ = v.retrieve(queries, gallery, _Model(), k=7)
    assert torch.equal(indices2, indices)
    with pytest.raises(NotImplementedError, match="query expansion"):
        v.validate_sharded(queries, gallery, _Model())
    v.setQueryExpansion(k=5, expand="gallery")
    _, _, d2 = v.validate(queries, gallery, _Model())
    assert torch.equal(d2, v.distance(*ops_eval.query_expansion(qf, gf, k=5, expand="gallery")))
    v.rerank = True
    v.setQueryExpansion(k=5)
    _, _, d3 = v.validate(queries, gallery, _Model())
    eq, eg = ops_eval.query_expansion(qf, gf, k=5)
    assert torch.equal(d3, ops_eval.re_ranking(v.distance(eq, eg), v.distance(eq, eq), v.distance(eg, eg)))
    v.rerank = False
    v.setQueryExpansion(None)
    cmc4, map4, d4 = v.validate(queries, gallery, _Model())
    assert torch.equal(d4, plain) and map4 == map0 and np.array_equal(cmc4, cmc0)
    with pytest.raises(ValueError):
        v.setQueryExpansion(k=5, expand="queries")
