"""CPU: tests/topk_ref.py, the reference of the GPU top-k tests, pinned against np.sort and torch.topk where those define the answer
(no ties, no NaN) and by hand where they do not."""
import numpy as np
import torch

import topk_ref as T

F32 = np.float32


def _bits(a):
    return np.asarray(a, dtype=F32).view(np.uint32)


def test_against_numpy_and_torch_without_ties():
    rng = np.random.default_rng(0)
    for nq, n, k in ((1, 1, 1), (4, 37, 5), (3, 200, 64)):
        x = rng.permutation(nq * n).reshape(nq, n).astype(F32) * F32(0.25) - F32(7)          # distinct values
        v, i = T.topk(x, k)
        assert np.array_equal(v, np.sort(x, axis=1)[:, :k])
        assert np.array_equal(i, np.argsort(x, axis=1)[:, :k].astype(np.int32))
        tv, ti = torch.topk(torch.from_numpy(x), k, dim=1, largest=False)
        assert np.array_equal(v, tv.numpy()) and np.array_equal(i, ti.numpy().astype(np.int32))
        v, i = T.topk(x, k, largest=True)
        tv, ti = torch.topk(torch.from_numpy(x), k, dim=1, largest=True)
        assert np.array_equal(v, tv.numpy()) and np.array_equal(i, ti.numpy().astype(np.int32))


def test_by_hand():
    inf, nan = np.inf, np.nan
    neg_nan = np.uint32(0xffc00001).view(F32)
    x = np.array([[1.0, -0.0, inf, 1.0, 0.0, -inf],
                  [nan, 2.0, neg_nan, -inf, inf, 2.0]], dtype=F32)
    v, i = T.topk(x, 6)
    assert i.tolist() == [[5, 1, 4, 0, 3, 2], [3, 1, 5, 4, 0, 2]]
    qnan = np.uint32(0x7fc00000)
    assert _bits(v).tolist() == [_bits([-inf, 0.0, 0.0, 1.0, 1.0, inf]).tolist(),
                                 _bits([-inf, 2.0, 2.0, inf]).tolist() + [qnan, qnan]]
    v, i = T.topk(x, 6, largest=True)
    assert i.tolist() == [[2, 0, 3, 1, 4, 5], [4, 1, 5, 3, 0, 2]]          # values reversed; ties still by ascending index; NaN still last
    assert _bits(v).tolist() == [_bits([inf, 1.0, 1.0, 0.0, 0.0, -inf]).tolist(),
                                 _bits([inf, 2.0, 2.0, -inf]).tolist() + [qnan, qnan]]


def test_sentinel_slots_and_offset():
    x = np.array([[3.0, 1.0, 2.0]], dtype=F32)
    v, i = T.topk(x, 5, col_offset=10)
    assert i.tolist() == [[11, 12, 10, -1, -1]] and v.tolist() == [[1.0, 2.0, 3.0, np.inf, np.inf]]
    v, i = T.topk(x, 5, largest=True)
    assert i.tolist() == [[0, 2, 1, -1, -1]] and v.tolist() == [[3.0, 2.0, 1.0, -np.inf, -np.inf]]
