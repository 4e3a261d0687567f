"""fp64 numpy restatement of the multi-output head: pooling over row ranges of an NHWC map for the three modes, the eval-mode BatchNorm1d
neck and the channel sum.  Checked against the reference's own classes through tests/golden/heads.npz (tests/test_heads_cpu.py); the GPU
tests compare the kernels and the plan with it."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "heads.npz")
MODES = ("both", "gap", "gmp")
U = 2.0 ** -24                     # unit roundoff of fp32


def bf16_bits_to_f64(bits):
    """uint16 bf16 bit patterns -> the values, exactly, as fp64."""
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def rows_of(rows, h):
    return (0, h) if rows is None else (int(rows[0]), int(rows[1]))


def pool(x, mode, rows=None):
    """x [n, h, w, C] -> fp64 [n, C]: mean + max ("both"), mean ("gap") or max ("gmp") over rows [rows[0], rows[1]) (None: every row)."""
    x = np.asarray(x, np.float64)
    b, e = rows_of(rows, x.shape[1])
    part = x[:, b:e].reshape(x.shape[0], -1, x.shape[3])
    mean, mx = part.mean(1), part.max(1)
    return {"both": mean + mx, "gap": mean, "gmp": mx}[mode]


def abs_sum(x, rows=None):
    """sum_p |x[n, p, c]| over the same pixels: the scale of the summation error bound."""
    x = np.asarray(x, np.float64)
    b, e = rows_of(rows, x.shape[1])
    return np.abs(x[:, b:e]).reshape(x.shape[0], -1, x.shape[3]).sum(1)


def neck_coeffs(weight, bias, running_mean, running_var, eps=1e-5):
    """Eval-mode BatchNorm1d as y = x * scale + shift, fp64."""
    w, b, m, v = (np.asarray(t, np.float64) for t in (weight, bias, running_mean, running_var))
    scale = w / np.sqrt(v + eps)
    return scale, b - m * scale


def neck(f, weight, bias, running_mean, running_var, eps=1e-5):
    scale, shift = neck_coeffs(weight, bias, running_mean, running_var, eps)
    return np.asarray(f, np.float64) * scale + shift


def neck_bound(f, weight, bias, running_mean, running_var, eps=1e-5):
    """|fp32 eval neck of f - neck(f)| for y = f * scale + shift, scale = weight / sqrt(var + eps), shift = bias - mean * scale, each step
    rounded to fp32: scale carries 4 roundings (the sum, the root, the quotient, the product), f * scale and mean * scale one more each, and
    the two additions one each, so the error is within u * (6 |f scale| + 7 |mean scale| + 2 |bias|) to first order; stated as
    8 * 2^-24 * (|f scale| + |mean scale| + |bias|), which also covers the second-order terms."""
    scale, _ = neck_coeffs(weight, bias, running_mean, running_var, eps)
    return 8 * U * (np.abs(np.asarray(f, np.float64) * scale) + np.abs(np.asarray(running_mean, np.float64) * scale) + np.abs(np.asarray(bias, np.float64)))


def channel_sum(x):
    """x [..., C] -> fp64 [...]."""
    return np.asarray(x, np.float64).sum(-1)


def mean_bound(x, ref, mode, rows=None):
    """|fp32 pooled value - ref| for a mean ("gap") or mean + max ("both") head whose sum ran in fp32 in any order:
    2 * 2^-24 * (sum_p |x_pc| + |ref_c|).  First order, a sum of P terms is off by at most (P - 1) u sum|x|, its quotient by P adds a
    relative u and "both" one more addition: all of it within u * (sum|x| + |ref|); the factor 2 covers the second-order terms.  A max head
    is exact: bound 0."""
    if mode == "gmp":
        return np.zeros_like(np.asarray(ref, np.float64))
    return 2 * U * (abs_sum(x, rows) + np.abs(ref))


def heat_bound(x):
    """|fp32 channel sum - ref|: 2 * 2^-24 * C * sum_c |x_c| (loose by design: any order, factor 2 for second order)."""
    x = np.asarray(x, np.float64)
    return 2 * U * x.shape[-1] * np.abs(x).sum(-1)


def load_golden():
    """-> dict of the fixture with the map as fp64 NHWC [1, 16, 8, 2048] under "map" and its bits (NHWC) under "map_bits_nhwc"."""
    z = dict(np.load(GOLDEN))
    z["map_bits_nhwc"] = np.ascontiguousarray(z["map_bits"].transpose(0, 2, 3, 1))
    z["map"] = bf16_bits_to_f64(z["map_bits_nhwc"])
    z["bn"] = tuple(z["last_bn." + k] for k in ("weight", "bias", "running_mean", "running_var"))
    return z


# the fixture's embedding outputs as (key, mode, rows): four multipart heads, three poolings (the heat map is compared on its own)
GOLDEN_HEADS = (("multipart_upper", "gmp", (0, 8)), ("multipart_middle", "gmp", (4, 12)), ("multipart_lower", "gmp", (8, 16)),
                ("multipart_whole", "gmp", None), ("feature_gap", "gap", None), ("feature_gmp", "gmp", None), ("feature_both", "both", None))
