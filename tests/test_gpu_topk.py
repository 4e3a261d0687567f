"""GPU: exact top-k retrieval (dali_topk_rows / dali_topk_decode / dali_pairdist_topk, ops_eval.topk_rows / pairdist_topk) against the numpy
restatement of the order (tests/topk_ref.py, pinned by tests/test_topk_cpu.py).  Every comparison is bitwise on values and exact on
indices; the reference of pairdist_topk is the matrix dali_pairdist_prepared writes for the same operand images."""
import numpy as np
import pytest
import torch

import topk_ref as T

pytestmark = pytest.mark.gpu

F32 = np.float32
TUNING = (128, 512, 64)          # boot_cols, chunk_cols, cand_cap: every path of pairdist_topk within a few thousand gallery rows


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _same(got, want, what=""):
    gv, gi = (t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in got[:2])
    wv, wi = want
    assert gv.dtype == F32 and gi.dtype == np.int32 and gv.shape == wv.shape and gi.shape == wi.shape, (what, gv.dtype, gi.dtype, gv.shape, wv.shape)
    assert np.array_equal(gi, wi), (what, "indices", np.argwhere(gi != wi)[:5])
    assert np.array_equal(gv.view(np.uint32), wv.view(np.uint32)), (what, "values")


def _tied(rng, nq, ncols):
    """uniform values rounded to multiples of 1/8: dense ties"""
    return (np.round(rng.uniform(-4, 4, (nq, ncols)) * 8) / 8).astype(F32)


def _salt(rng, x):
    specials = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xffffffff], dtype=np.uint32).view(F32)
    x = x.copy()
    m = rng.uniform(size=x.shape) < 0.3
    x[m] = specials[rng.integers(0, len(specials), int(m.sum()))]
    return x


# ---- topk_rows ----

SHAPES = [(1, 1, 1), (3, 5, 8), (7, 64, 64), (5, 65, 64), (33, 1000, 50), (2, 8191, 128), (129, 300, 1), (4, 20000, 20)]


@pytest.mark.parametrize("largest", [False, True])
@pytest.mark.parametrize("nq,ncols,k", SHAPES)
def test_rows_shapes(dev, nq, ncols, k, largest):
    from daliid_amd import ops_eval
    x = _tied(np.random.default_rng(nq * 7919 + ncols), nq, ncols)
    got = ops_eval.topk_rows(torch.from_numpy(x).to(dev), k, largest=largest)
    _same(got, T.topk(x, min(k, ncols), largest), "%dx%d k=%d" % (nq, ncols, k))          # (the Python surface clamps k to the columns)


def _rows_raw(dev, x, k, largest, accumulate_into=None, col_offset=0):
    """dali_topk_rows with the k given (no clamp) -> (status, keys)"""
    from daliid_amd import _lib
    xd = torch.from_numpy(x).to(dev)
    keys = accumulate_into if accumulate_into is not None else torch.zeros(x.shape[0], max(k, 1), device=dev, dtype=torch.int64)
    rc = _lib.lib().dali_topk_rows(_lib.ctx(dev), _lib.stream_ptr(), _lib.ptr(xd), x.shape[0], x.shape[1], x.shape[1], col_offset, k, int(largest),
                                   int(accumulate_into is not None), _lib.ptr(keys))
    torch.cuda.synchronize()
    return rc, keys


@pytest.mark.parametrize("largest", [False, True])
def test_rows_sentinel_slots(dev, largest):
    """k beyond the columns seen: index -1 and +inf (-inf for largest) in the unfilled slots, which later columns then take"""
    from daliid_amd import ops_eval
    x = _tied(np.random.default_rng(3), 3, 5)
    rc, keys = _rows_raw(dev, x, 8, largest)
    assert rc == 0
    _same(ops_eval.topk_decode(keys, largest), T.topk(x, 8, largest), "unfilled")
    y = _tied(np.random.default_rng(4), 3, 2)
    rc, keys = _rows_raw(dev, y, 8, largest, accumulate_into=keys, col_offset=5)
    assert rc == 0
    _same(ops_eval.topk_decode(keys, largest), T.topk(np.concatenate([x, y], axis=1), 8, largest), "7 of 8 filled")


@pytest.mark.parametrize("largest", [False, True])
@pytest.mark.parametrize("nq,ncols,k", [(5, 65, 64), (33, 1000, 50), (3, 3000, 128)])
def test_rows_special_values(dev, nq, ncols, k, largest):
    from daliid_amd import ops_eval
    rng = np.random.default_rng(11 + ncols)
    x = _salt(rng, _tied(rng, nq, ncols))
    if ncols == 3000:                      # a row that is mostly NaN: NaN entries are selected, by ascending index
        x[1, 40:] = np.uint32(0xffc00000).view(F32)
    _same(ops_eval.topk_rows(torch.from_numpy(x).to(dev), k, largest=largest), T.topk(x, k, largest), "salted")


@pytest.mark.parametrize("lo,hi", [(100, 401), (101, 400)])
def test_rows_column_slice(dev, lo, hi):
    """a column slice of a contiguous matrix is read by its pitch (16-byte aligned rows, and rows that are only 4-byte aligned)"""
    from daliid_amd import ops_eval
    x = _tied(np.random.default_rng(5), 6, 1000)
    xd = torch.from_numpy(x).to(dev)
    view = xd[:, lo:hi]
    assert not view.is_contiguous()
    _same(ops_eval.topk_rows(view, 20), T.topk(x[:, lo:hi], 20), "slice")
    _same(ops_eval.topk_rows(view, 20, largest=True, col_offset=lo), T.topk(x[:, lo:hi], 20, True, col_offset=lo), "slice, offset")


@pytest.mark.parametrize("largest", [False, True])
def test_rows_accumulated_blocks(dev, largest):
    from daliid_amd import ops_eval
    x = _tied(np.random.default_rng(6), 9, 3000)
    xd = torch.from_numpy(x).to(dev)
    keys = None
    for lo, hi in ((0, 700), (700, 737), (737, 3000)):
        v, i, keys = ops_eval.topk_rows(xd[:, lo:hi], 50, largest=largest, col_offset=lo, running=keys, return_keys=True)
    want = T.topk(x, 50, largest)
    _same((v, i), want, "three blocks")
    one = ops_eval.topk_rows(xd, 50, largest=largest, return_keys=True)
    _same(one, want, "one shot")
    assert torch.equal(one[2], keys)


def test_rows_k_limit(dev):
    from daliid_amd import _lib, ops_eval
    assert ops_eval.TOPK_K_MAX == 128
    x = _tied(np.random.default_rng(7), 2, 400)
    with pytest.raises(_lib.DaliError, match="129"):
        ops_eval.topk_rows(torch.from_numpy(x).to(dev), 129)
    rc, _ = _rows_raw(dev, x, 129, False)
    assert rc == -4 and "129" in _lib.last_error()                      # DALI_ERR_LIMIT with a message
    _same(ops_eval.topk_rows(torch.from_numpy(x).to(dev), 128), T.topk(x, 128), "k = 128")


# ---- pairdist_topk ----

def _features(rng, n, d, real=False):
    if real:
        return rng.standard_normal((n, d)).astype(F32)
    return rng.integers(-1, 2, (n, d)).astype(F32)        # {-1, 0, 1}: equal distances abound, the index tie-break decides


def _prepared(dev, q, g, metric, precision):
    from daliid_amd import ops_eval
    norm = metric == "cosine"
    qp = ops_eval.PreparedRows(torch.from_numpy(q).to(dev), normalize=norm, precision=precision)
    gp = ops_eval.PreparedRows(torch.from_numpy(g).to(dev), normalize=norm, precision=precision)
    return qp, gp


METRICS = [("cosine", False), ("l2sq", False), ("dot", True)]
# k = 10 with cand_cap = 64: the thresholds of a round are the k-th keys of the s rows seen and a round takes n <= s new rows (whatever
# chunk_cols asks for), so for rows in random order the survivors of a query are negative binomial with mean n k / (s + 1) <= 10 and
# variance <= 20 (ties only lower them: an equal value with a larger index does not survive); 65 survivors need fewer than 10 of the first
# 75 rows of a random order to come from the seen half, a probability of about 1e-11 per query and round: no case here may overflow
K = 10


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
@pytest.mark.parametrize("nq,ng,d", [(1, 1, 32), (255, 127, 48), (257, 129, 32), (255, 1000, 48), (257, 4099, 2048), (1, 4099, 48), (257, 1000, 32)])
def test_pairdist_topk_matches_matrix(dev, nq, ng, d, precision):
    from daliid_amd import ops_eval
    rng = np.random.default_rng(nq * 31 + ng * 7 + d)
    q, g = _features(rng, nq, d), _features(rng, ng, d)
    for metric, largest in METRICS:
        qp, gp = _prepared(dev, q, g, metric, precision)
        D = ops_eval.pairdist_prepared(qp, gp, metric=metric).cpu().numpy()
        v, i, stats = ops_eval.pairdist_topk(qp, gp, K, metric=metric, largest=largest, return_stats=True, _tuning=TUNING)
        fused, matrix, overflow = stats.tolist()
        print("%dx%dx%d %s %s: stats %s" % (nq, ng, d, precision, metric, (fused, matrix, overflow)))
        _same((v, i), T.topk(D, min(K, ng), largest), "%s %s" % (metric, precision))
        # the first boot_cols rows give the thresholds through the matrix block; every row behind them is selected in the epilogue
        assert overflow == 0 and matrix == min(ng, TUNING[0]) and fused == ng - matrix
        if ng > TUNING[0]:
            assert fused > 0


def test_pairdist_topk_real_valued_and_features_in(dev):
    """continuous features; fp32 tensors in (prepared inside, normalize=True) give what the prepared images give"""
    from daliid_amd import ops_eval
    rng = np.random.default_rng(17)
    q, g = _features(rng, 257, 48, real=True), _features(rng, 1000, 48, real=True)
    qp, gp = _prepared(dev, q, g, "cosine", "bf16x3")
    D = ops_eval.pairdist_prepared(qp, gp, metric="cosine").cpu().numpy()
    want = T.topk(D, K)
    v, i, stats = ops_eval.pairdist_topk(qp, gp, K, return_stats=True, _tuning=TUNING)
    _same((v, i), want, "prepared")
    assert stats.tolist()[0] > 0 and stats.tolist()[2] == 0
    _same(ops_eval.pairdist_topk(torch.from_numpy(q).to(dev), torch.from_numpy(g).to(dev), K, normalize=True, _tuning=TUNING), want, "features")


def _adversarial(nq=5, ng=2000, d=32):
    """every query close to u = e0; gallery row i at an angle to u that shrinks with i: every later row is nearer to every query"""
    theta = 0.05 + 1.0 * (1.0 - np.arange(ng) / ng)
    g = np.zeros((ng, d))
    g[:, 0], g[:, 1] = np.cos(theta), np.sin(theta)
    q = np.zeros((nq, d))
    q[:, 0], q[:, 2] = 1.0, 0.01 * np.arange(nq)
    return q, g


def test_overflow_falls_back_to_the_matrix(dev):
    from daliid_amd import ops_eval
    q, g = _adversarial()
    # on the CPU first: the fp64 distances decrease strictly along every row, by far more than the kernel's error (1e-6), so the last k rows
    # are the answer and every row of a round beats every threshold: 512 survivors for 16 slots, whatever the implementation's constants
    D64 = 1.0 - (q / np.linalg.norm(q, axis=1, keepdims=True)) @ (g / np.linalg.norm(g, axis=1, keepdims=True)).T
    assert np.all(np.diff(D64, axis=1) < -1e-5)
    assert np.array_equal(T.topk(D64.astype(F32), K)[1], np.tile(np.arange(1999, 1999 - K, -1, dtype=np.int32), (5, 1)))
    qp, gp = _prepared(dev, q.astype(F32), g.astype(F32), "cosine", "bf16x3")
    D = ops_eval.pairdist_prepared(qp, gp, metric="cosine").cpu().numpy()
    v, i, stats = ops_eval.pairdist_topk(qp, gp, K, return_stats=True, _tuning=(128, 512, 16))
    fused, matrix, overflow = stats.tolist()
    print("adversarial: stats", (fused, matrix, overflow))
    _same((v, i), T.topk(D, K), "adversarial")
    assert np.array_equal(i.cpu().numpy(), np.tile(np.arange(1999, 1999 - K, -1, dtype=np.int32), (5, 1)))
    assert overflow > 0 and matrix > 128


def test_gallery_in_pieces(dev):
    """g_offset / running: the 4099-row gallery in pieces of 1000 / 37 / 3062 equals the one-shot result"""
    from daliid_amd import ops_eval
    rng = np.random.default_rng(23)
    q, g = _features(rng, 257, 48), _features(rng, 4099, 48)
    qd = torch.from_numpy(q).to(dev)
    one = ops_eval.pairdist_topk(qd, torch.from_numpy(g).to(dev), K, metric="l2sq", return_keys=True, _tuning=TUNING)
    keys = None
    for lo, hi in ((0, 1000), (1000, 1037), (1037, 4099)):
        v, i, keys = ops_eval.pairdist_topk(qd, torch.from_numpy(g[lo:hi]).to(dev), K, metric="l2sq", g_offset=lo, running=keys, return_keys=True,
                                            _tuning=TUNING)
    assert torch.equal(keys, one[2]) and torch.equal(v, one[0]) and torch.equal(i, one[1])
    qp, gp = _prepared(dev, q, g, "l2sq", "bf16x3")
    _same(one, T.topk(ops_eval.pairdist_prepared(qp, gp, metric="l2sq").cpu().numpy(), K), "one shot")


def test_default_tuning(dev):
    from daliid_amd import ops_eval
    rng = np.random.default_rng(29)
    q, g = _features(rng, 300, 256, real=True), _features(rng, 20000, 256, real=True)
    qp, gp = _prepared(dev, q, g, "cosine", "bf16x3")
    D = ops_eval.pairdist_prepared(qp, gp, metric="cosine").cpu().numpy()
    v, i, stats = ops_eval.pairdist_topk(qp, gp, 50, return_stats=True)
    print("default tuning: stats", stats.tolist())
    _same((v, i), T.topk(D, 50), "default tuning")
    assert stats.tolist()[0] > 0


def test_scratch_does_not_grow_with_the_gallery(dev):
    from daliid_amd import _lib
    f = _lib.lib().dali_pairdist_topk_scratch_bytes
    a, b = f(10000, 100000, 2048, 64, 0, 0, 0), f(10000, 1000000, 2048, 64, 0, 0, 0)
    assert a == b and 0 < a < 10000 * 100000 * 4 // 10


def test_run_to_run(dev):
    from daliid_amd import ops_eval
    rng = np.random.default_rng(31)
    q, g = _features(rng, 257, 48), _features(rng, 4099, 48)
    qp, gp = _prepared(dev, q, g, "cosine", "bf16")
    a = ops_eval.pairdist_topk(qp, gp, K, return_keys=True, _tuning=TUNING)
    b = ops_eval.pairdist_topk(qp, gp, K, return_keys=True, _tuning=TUNING)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    x = torch.from_numpy(_tied(rng, 33, 5000)).to(dev)
    a, b = ops_eval.topk_rows(x, 50, return_keys=True), ops_eval.topk_rows(x, 50, return_keys=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
