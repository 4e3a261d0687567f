"""Bounds and comparisons shared by tests/test_metarec_cpu.py (twin against the reference's golden) and tests/test_gpu_metarec.py (GPU
against the golden and against the twin): the GPU is one more restatement of the same arithmetic, so the same bounds hold.

shape 3e-6 relative, scale 1e-7 relative, small bitwise, w-scores 1e-6 absolute, fused 1e-6 absolute where the w-scores sum to at least
1e-3 (at most 1 % of the entries left out).  About four times the distance measured between the reference and the twin on shapes up to
1100 x 70 and 300 x 130 x 3 models (shape <= 7e-7, scale <= 1.1e-8, w <= 2.2e-7, fused <= 3e-8), which comes from the reference's fp32
mean of the logarithms and from libm differences."""
import numpy as np

SHAPE_RTOL, SCALE_RTOL, W_ATOL, FUSED_ATOL, SUMW_MIN, LEFT_OUT_MAX = 3e-6, 1e-7, 1e-6, 1e-6, 1e-3, 0.01


def golden_cases(z):
    return sorted({k.split("/")[0] for k in z.files})


def case(z, name):
    nq, ng, topk, cols, m = (int(v) for v in z[name + "/meta"])
    d = dict(nq=nq, ng=ng, topk=topk, use_columns=bool(cols), m=m, killscale=float(z[name + "/killscale"]))
    for key in ("S", "fits", "small", "w"):
        d[key] = [z["%s/%s%d" % (name, key, a)] for a in range(m)]
    d["fused"] = z[name + "/fused"] if name + "/fused" in z.files else None
    return d


def check_fit(got, want, what):
    """(fits, small, w) of the code under test against the expected triple; prints the distances, then asserts.  Unfit rows (NaN) must be
    the same rows on both sides.  -> (shape, scale, w) distances."""
    (fits, small, w), (fits0, small0, w0) = got, want
    unfit = np.isnan(fits0[:, 0])
    assert np.array_equal(np.isnan(fits), np.isnan(fits0)), (what, "different rows are unfit")
    ok = ~unfit
    rel = lambda x, y: float(np.max(np.abs(x - y) / np.abs(y))) if x.size else 0.0
    d_shape, d_scale = rel(fits[ok, 0], fits0[ok, 0]), rel(fits[ok, 1], fits0[ok, 1])
    d_w = float(np.max(np.abs(w - w0)))
    print("%s: shape %.3g scale %.3g w %.3g (%d unfit)" % (what, d_shape, d_scale, d_w, int(unfit.sum())))
    assert np.array_equal(small, small0), (what, "small differs")
    assert d_shape <= SHAPE_RTOL and d_scale <= SCALE_RTOL and d_w <= W_ATOL, (what, d_shape, d_scale, d_w)
    return d_shape, d_scale, d_w


def check_fused(fused, fused0, sum_w, what):
    keep = sum_w >= SUMW_MIN
    d = float(np.max(np.abs(fused - fused0)[keep]))
    print("%s fused: %.3g, %.3f %% left out" % (what, d, 100 * (1 - keep.mean())))
    assert 1 - keep.mean() <= LEFT_OUT_MAX and d <= FUSED_ATOL, (what, d, 1 - keep.mean())
    return d
