"""numpy restatement of the selection order of include/daliid.h (dali_topk_rows), the reference of tests/test_gpu_topk.py:
ascending by value, exact ties by ascending index, -0.0 == +0.0, NaN of either sign after +inf; ``largest`` reverses the value order
only (ties still by ascending index, NaN still last).  Pinned against np.sort / torch.topk and by hand in tests/test_topk_cpu.py."""
import numpy as np

F32 = np.float32


def fold(x):
    """fp32 values as the order sees them: -0.0 -> +0.0, every NaN -> the quiet NaN 0x7fc00000."""
    x = np.array(x, dtype=F32, copy=True)
    with np.errstate(invalid="ignore"):           # (a signalling NaN in the input: replaced below)
        x = x + F32(0.0)                          # -0.0 + +0.0 = +0.0 (round to nearest)
    x[np.isnan(x)] = np.uint32(0x7fc00000).view(F32)
    return x


def order(row, largest=False):
    """Indices of one row, best first."""
    row = fold(row)
    nan = np.isnan(row)
    key = np.where(nan, F32(0), -row if largest else row)      # (the negation is exact; NaN handled apart)
    idx = np.argsort(key, kind="stable")                       # stable: equal values keep ascending index
    return np.concatenate([idx[~nan[idx]], idx[nan[idx]]])     # NaN last either way, by ascending index


def topk(x, k, largest=False, col_offset=0):
    """-> (values fp32 [nq, k], indices int32 [nq, k]).  Slots beyond the number of columns hold the sentinel: index -1, value +inf
    (-inf for largest)."""
    x = np.asarray(x, dtype=F32)
    nq, n = x.shape
    vals = np.full((nq, k), -np.inf if largest else np.inf, dtype=F32)
    idx = np.full((nq, k), -1, dtype=np.int32)
    folded = fold(x)
    m = min(k, n)
    for i in range(nq):
        o = order(x[i], largest)[:m]
        vals[i, :m] = folded[i, o]
        idx[i, :m] = o + col_offset
    return vals, idx
