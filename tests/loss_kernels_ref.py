"""Plain fp64 restatements of the loss-head kernels (csrc/losses.hip) and of the Adam / EMA kernels (csrc/optim.hip), the per-element error
bounds the GPU tests hold those kernels to, and the input families both the GPU tests and the CPU self-tests draw from; test infrastructure only.

Written from the formulas in the kernel headers and the semantics of the reference's ``losses.py`` (oracle/losses.py restates those in fp32
torch; tests/test_loss_kernels_ref_cpu.py ties this file to the reference's own outputs in tests/golden/).  Every function takes the fp32 arrays
the kernel takes.  A scalar that crosses the C ABI as ``float`` (tau, lr, the betas, eps, weight decay, grad_scale, gscale) is used as that fp32
value widened to double; ``1/tau`` is the fp32 quotient ``fl(1/fl(tau))`` the ABI entry points pass to their kernels, widened to double.

Error bounds.  u = 2^-24 is the fp32 unit roundoff: one correctly rounded operation (+ - * / sqrt, all IEEE in the library's build, which also
forbids contraction into FMA) has relative error <= u.  The HIP math API documents expf, logf and log1pf at 1 ULP = 2^-23 = 2u relative.
Bounds are first order in u.  A result smaller than the least normal number 2^-126 may be flushed to zero, which the bounds of quantities that
can get that small allow for (``FLT_MIN``).  No constant here was fitted to what a GPU returned.
"""
import math

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
FLT_MIN = 2.0 ** -126
INT_MAX = 2 ** 31 - 1


def inv_tau(tau):
    """fl32(1 / fl32(tau)) as a double."""
    return float(F32(1.0) / F32(tau))


def f32(x):
    """the fp32 value of a scalar that crosses the ABI as float, as a double"""
    return float(F32(x))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# center head:  p_ij = softmax_j(S_ij / tau);  num_i = w_i sum_{j: cl_j == y_i} -log p_ij;  den_i = w_i cnt_i,  cnt_i = #{j: cl_j == y_i}
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _center_parts(S, y, cl, tau, _wrong=None):
    v = np.asarray(S, F64) * inv_tau(tau)
    m = v.max(axis=1)
    d = m[:, None] - v                                   # >= 0
    e = np.exp(-d)
    se = e.sum(axis=1)
    mask = np.asarray(cl)[None, :] == np.asarray(y)[:, None]
    cnt = mask.sum(axis=1).astype(F64)
    if _wrong == "cnt_min1":
        cnt = np.minimum(cnt, 1.0)
    return v, m, d, e, se, mask, cnt


def center_rows(S, y, cl, w, tau, _wrong=None):
    """-> dict: num, den [nb]; argmax [nb] (first index on ties); maxp [nb]; sums [2] = (sum num, sum den); and the intermediates the
    bounds need (cnt, m, logse, abspos)."""
    v, m, d, e, se, mask, cnt = _center_parts(S, y, cl, tau, _wrong)
    w = np.asarray(w, F64)
    logse = np.log(se)
    pos = (v * mask).sum(axis=1)
    num = w * (cnt * (m + logse) - pos)
    den = w * cnt
    Sf = np.asarray(S, F32)
    if _wrong == "argmax_last":
        am = Sf.shape[1] - 1 - np.argmax(Sf[:, ::-1], axis=1)
    else:
        am = np.argmax(Sf, axis=1)
    return dict(num=num, den=den, argmax=am.astype(np.int64), maxp=1.0 / se, sums=np.array([num.sum(), den.sum()]),
                cnt=cnt, m=m, logse=logse, abspos=(np.abs(v) * mask).sum(axis=1))


def center_bwd(S, y, cl, w, tau, denom, gscale=1.0, _wrong=None):
    """dense dS_ij = gscale w_i / (tau denom) (cnt_i p_ij - [cl_j == y_i]); ``denom`` is the global normaliser, whatever the local sum is."""
    v, m, d, e, se, mask, cnt = _center_parts(S, y, cl, tau, _wrong)
    w = np.asarray(w, F64)
    if _wrong == "denom_local":
        denom = (w * cnt).sum()
    coef = f32(gscale) * w * inv_tau(tau) / float(denom)
    return coef[:, None] * (cnt[:, None] * e / se[:, None] - mask)


def _depth(n_cols):
    """longest chain of additions in a wave's sum over a row: ceil(n/64) per lane, then 6 butterfly levels"""
    return math.ceil(n_cols / 64) + 6


def _logse_units(m, NC):
    """Error of the kernel's log(sum_j exp(v_j - m)) in units of u, the logf call itself excluded.
    v_j = fl(s_j/tau) is off by u|v_j| and the subtraction v_j - m by u d_j (d_j = m - v_j >= 0); log-sum-exp moves by sum_j p_j times that:
    u sum_j p_j (|v_j| + d_j) <= u (|m| + 2 sum_j p_j d_j), and sum_j p_j d_j = H(p) - log se <= ln NC (entropy; se >= 1).  Each expf adds 2u
    relative (-> 2u absolute on the log), and the sum of positive terms along a chain of `depth` additions adds depth u relative."""
    return np.abs(m) + 2.0 * math.log(max(NC, 2)) + 2.0 + _depth(NC)


CENTER_C1 = 6.0
CENTER_C2 = 1.0


def center_num_tol(ref, w, NC):
    """|num_gpu - num| <= u w [c1 (cnt (|m| + |log se|) + sum|v_pos|) + c2 cnt depth'],  c1 = 6, c2 = 1, depth' = depth + 2 ln NC + 2.

    num = w (cnt logz - pos), logz = m + logf(se).  Errors, in units of u:
      logz : _logse_units = |m| + depth'                       (arguments, expf, accumulation)
             + 2 |log se|                                       (logf, 1 ULP)
             + |m| + |log se|                                   (the addition m + log se)           -> 2|m| + 3|log se| + depth'
      cnt*logz : one product rounding, cnt (|m| + |log se|);  cnt <= 2^24 converts exactly
      pos  : each v_p is off by u|v_p|; a sum of cnt non-zero terms is cnt - 1 inexact additions wherever they sit in the lanes (adding zero is
             exact), each off by at most u sum|v_pos|                                               -> cnt sum|v_pos|
      the subtraction and the product with w: u (cnt(|m| + |log se|) + sum|v_pos|) each.
    Sum: cnt (|m| + |log se|) (2 + 3 + 1 + 2 -> at most 6 on either term) + (cnt + 2) sum|v_pos| + cnt depth'; cnt + 2 <= 6 for the at most
    four centers per identity the tests use (asserted).  Rows without a center give exactly 0."""
    cnt = ref["cnt"]
    assert cnt.max() <= 4
    depthp = _depth(NC) + 2.0 * math.log(max(NC, 2)) + 2.0
    return U * np.asarray(w, F64) * (CENTER_C1 * (cnt * (np.abs(ref["m"]) + np.abs(ref["logse"])) + ref["abspos"]) + CENTER_C2 * cnt * depthp)


def center_maxp_tol(ref, NC):
    """maxp = 1/se = exp(m - logz): relative error = the error of log se (_logse_units; the kernel's m is itself a rounded v, another u|m|)
    plus the division."""
    return U * ref["maxp"] * (_logse_units(ref["m"], NC) + np.abs(ref["m"]) + 1.0)


def center_bwd_tol(S, y, cl, w, tau, denom, gscale=1.0):
    """Per element of dS = coef (cnt p - mask), coef = ((gscale w) / tau) / denom  (3 roundings):
      p_j = expf(v_j - m) * (1/se): argument off by u (|v_j| + |m| + d_j) <= u (2|m| + 2 d_j), expf 2u, 1/se as center_maxp_tol minus the
            shared |m| (counted once here) plus its division, one product       -> relative u (3|m| + 2 d_j + 2 ln NC + depth + 6)
      cnt*p: u more.  cnt*p - mask, the product with coef and coef's own 3u: 5u |cnt p - mask|.
    An element below FLT_MIN may be flushed."""
    v, m, d, e, se, mask, cnt = _center_parts(S, y, cl, tau)
    NC = v.shape[1]
    coef = np.abs(f32(gscale) * np.asarray(w, F64) * inv_tau(tau) / float(denom))[:, None]
    p = e / se[:, None]
    rel_p = 3.0 * np.abs(m)[:, None] + 2.0 * d + 2.0 * math.log(max(NC, 2)) + _depth(NC) + 7.0
    return U * coef * (cnt[:, None] * p * rel_p + 5.0 * np.abs(cnt[:, None] * p - mask)) + FLT_MIN


# ---------------------------------------------------------------------------------------------------------------------------------------------
# proxy head: per row, positives = proxies of the row's id (n of them), negatives = the k = min(n, NP - n) most similar other-id proxies in
# (value descending, index ascending) order.  D = sum_sel e^{s/tau};  row = -w/n sum_pos (s_p/tau - log D);  den = w if n > 0.
#   d row/d s_p = w/tau (e_p/D - 1/n);  d row/d s_neg = w/tau e_neg/D
# ---------------------------------------------------------------------------------------------------------------------------------------------
def proxy_select(s_row, is_pos, _wrong=None):
    """-> (positives ascending, selected negatives in order).  A slot the wrong variant ``k_n`` cannot fill holds INT_MAX."""
    NP = len(s_row)
    pos = np.flatnonzero(is_pos)
    n = len(pos)
    neg = np.flatnonzero(~is_pos)
    if _wrong == "ignore_last_slot":
        neg = neg[neg < 256 * ((NP + 255) // 256 - 1)]
    k = n if _wrong == "k_n" else min(n, NP - n)
    tie_key = -neg if _wrong == "tie_desc" else neg
    order = neg[np.lexsort((tie_key, -s_row[neg].astype(F64)))]
    sel = order[:k]
    if len(sel) < k:
        sel = np.concatenate([sel, np.full(k - len(sel), INT_MAX, dtype=sel.dtype)])
    return pos, sel


def proxy_rows(S, y, pl, w, tau, kmax, _wrong=None):
    """-> dict: sel_idx [nb, 2 kmax] int32 (-1 padded), sel_coef [nb, 2 kmax] (0 padded), num, den [nb], sums [2], status (1 when an identity
    has more than kmax proxies; such a row's contents are unspecified: ``specified[i]`` is False and it is left out of ``sums``), and the
    per-slot / per-row bounds ``coef_tol``, ``num_tol`` (derivation: proxy_tolerances)."""
    S = np.asarray(S, F32)
    nb, NP = S.shape
    it = inv_tau(tau)
    pl, y, w = np.asarray(pl), np.asarray(y), np.asarray(w, F64)
    sel_idx = np.full((nb, 2 * kmax), -1, np.int32)
    sel_coef = np.zeros((nb, 2 * kmax))
    coef_tol = np.zeros((nb, 2 * kmax))
    num, den, num_tol = np.zeros(nb), np.zeros(nb), np.zeros(nb)
    specified = np.ones(nb, bool)
    status = 0
    for i in range(nb):
        is_pos = pl == y[i]
        n = int(is_pos.sum())
        if n == 0:
            continue
        if n > kmax:
            status, specified[i] = 1, False
            continue
        pos, neg = proxy_select(S[i], is_pos, _wrong)
        k = len(neg)
        real = neg[neg != INT_MAX]
        vp = S[i, pos].astype(F64) * it
        vn = np.concatenate([S[i, real].astype(F64) * it, np.full(k - len(real), -np.inf)])
        m = max(vp.max(), vn.max() if k else -np.inf)
        Drel = np.exp(vp - m).sum() + np.exp(vn - m).sum()
        logD = m + math.log(Drel)
        ep, en = np.exp(vp - logD), np.exp(vn - logD)
        num[i] = -w[i] * (vp.sum() / n - logD)
        den[i] = w[i]
        sel_idx[i, :n], sel_idx[i, kmax:kmax + k] = pos, neg
        sel_coef[i, :n] = w[i] * it * (ep - 1.0 / n)
        sel_coef[i, kmax:kmax + k] = w[i] * it * en
        t = proxy_tolerances(vp, vn, m, Drel, w[i], it)
        num_tol[i] = t[0]
        coef_tol[i, :n], coef_tol[i, kmax:kmax + k] = t[1], t[2]
    return dict(sel_idx=sel_idx, sel_coef=sel_coef, num=num, den=den, sums=np.array([num[specified].sum(), den[specified].sum()]),
                status=status, specified=specified, coef_tol=coef_tol, num_tol=num_tol)


def proxy_tolerances(vp, vn, m, Drel, w, it):
    """Bounds for one row -> (row bound, bounds of the positives' coefficients, of the negatives').  t = n + k <= 32 selected terms.

    log D = m + logf(Drel), Drel = sum_sel expf(v - m), in units of u (as _logse_units, the chain being the t sequential additions):
      E = [|m| + 2 ln t + 2 + t] + 2 |log Drel| + (|m| + |log Drel|)
    row = -w (possum / n - log D): every v_p off by u|v_p| and n - 1 additions off by u sum|v_p| each, divided by n -> sum|v_p|; the division
      sum|v_p| / n; the subtraction and the product with w: 2 |possum/n - log D|.
    coefficient of a positive, (w/tau) (expf(v_p - log D) - 1/n): argument off by u (|v_p| + E + |v_p - log D|), expf 2u; 1/n off by u/n; the
      subtraction, the product w * (1/tau) and the final product: 3 |e_p - 1/n|.
    coefficient of a negative, (w/tau) expf(v - log D): the same argument error and expf, and two products.
    Coefficients below FLT_MIN may be flushed."""
    n, t = len(vp), len(vp) + len(vn)
    L = abs(math.log(Drel))
    logD = m + math.log(Drel)
    E = 2.0 * abs(m) + 3.0 * L + 2.0 * math.log(max(t, 2)) + 2.0 + t
    sabs = np.abs(vp).sum()
    row = U * w * ((1.0 + 1.0 / n) * sabs + E + 2.0 * abs(vp.sum() / n - logD))
    ep, en = np.exp(vp - logD), np.exp(vn - logD)
    with np.errstate(invalid="ignore"):
        argn = np.where(np.isfinite(vn), np.abs(vn) + np.abs(vn - logD), 0.0)
    cpos = U * w * it * (ep * (np.abs(vp) + np.abs(vp - logD) + E + 2.0) + 1.0 / n + 3.0 * np.abs(ep - 1.0 / n)) + FLT_MIN
    cneg = U * w * it * en * (argn + E + 4.0) + FLT_MIN
    return row, cpos, cneg


def proxy_bwd(sel_idx, sel_coef, P, denom, gscale=1.0, accumulate=False, out=None):
    """dfn[i] (+)= gscale / denom * sum_{slots with sel_idx >= 0} coef P[sel_idx]; what an empty slot's coefficient holds is irrelevant."""
    sel_idx = np.asarray(sel_idx)
    P = np.asarray(P, F64)
    cf = np.where(sel_idx >= 0, np.asarray(sel_coef, F64), 0.0)
    res = np.einsum("ia,iad->id", cf, P[np.maximum(sel_idx, 0)]) * (f32(gscale) / float(denom))
    return res + np.asarray(out, F64) if accumulate else res


def proxy_bwd_tol(sel_idx, sel_coef, P, denom, gscale=1.0, accumulate=False, out=None):
    """A dot product of a = sel_idx.shape[1] terms summed in sequence: (a + 1) u sum|coef P| (a - 1 additions and the products; Higham, Accuracy
    and Stability, eq. 3.5, first order), z = gscale/denom and the product with it 2u more, the accumulation one rounding of the result."""
    sel_idx = np.asarray(sel_idx)
    cf = np.where(sel_idx >= 0, np.abs(np.asarray(sel_coef, F64)), 0.0)
    mag = np.einsum("ia,iad->id", cf, np.abs(np.asarray(P, F64)[np.maximum(sel_idx, 0)])) * abs(f32(gscale) / float(denom))
    tol = U * (sel_idx.shape[1] + 3) * mag + FLT_MIN
    if accumulate:
        tol = tol + U * np.abs(proxy_bwd(sel_idx, sel_coef, P, denom, gscale, True, out))
    return tol


# ---------------------------------------------------------------------------------------------------------------------------------------------
# in-batch triplet head: p_i = argmin_{j: y_j == y_i} S_ij (self included), n_i = argmax_{j: y_j != y_i} S_ij, lowest index on ties;
# x = (s_n - s_p)/tau;  row = w softplus(x);  coef = d row/d s_n = w sigmoid(x)/tau;  status 1 when a row has no negative (row all zero, -1)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def triplet_rows(S, y, w, tau):
    """-> dict: sel_idx [nb, 2] (p_i, n_i), sel_coef [nb], num, den [nb], sums [2], status, num_tol, coef_tol."""
    S = np.asarray(S, F32)
    nb = S.shape[0]
    y, w, it = np.asarray(y), np.asarray(w, F64), inv_tau(tau)
    sel_idx = np.full((nb, 2), -1, np.int32)
    sel_coef, num, den, num_tol, coef_tol = (np.zeros(nb) for _ in range(5))
    status = 0
    for i in range(nb):
        same = y == y[i]
        if same.all():
            status = 1
            continue
        pj = np.flatnonzero(same)
        nj = np.flatnonzero(~same)
        p = pj[np.argmin(S[i, pj])]                          # argmin / argmax return the first of equals
        q = nj[np.argmax(S[i, nj])]
        x = (float(S[i, q]) - float(S[i, p])) * it
        sp = max(x, 0.0) + math.log1p(math.exp(-abs(x)))
        sg = 1.0 / (1.0 + math.exp(-x)) if x > -700 else 0.0
        sel_idx[i] = (p, q)
        num[i], den[i], sel_coef[i] = w[i] * sp, w[i], w[i] * sg * it
        # x: the subtraction and the product, 2u|x|.  softplus has slope <= 1: 2u|x|; expf 2u on a term whose log1p has slope <= 1; log1pf
        # 2u log1p(.) <= 2u ln 2; the addition and the product with w, 2u sp.
        num_tol[i] = U * w[i] * (2.0 * abs(x) + 2.0 + 2.0 * math.log(2.0) + 2.0 * sp)
        # sigmoid'/sigmoid = 1 - sigmoid <= 1: 2u|x| relative; expf 2u, 1 + e, the division, two products: 6u.  Flushed below FLT_MIN.
        coef_tol[i] = U * sel_coef[i] * (2.0 * abs(x) + 6.0) + FLT_MIN * max(1.0, w[i] * it)
    return dict(sel_idx=sel_idx, sel_coef=sel_coef, num=num, den=den, sums=np.array([num.sum(), den.sum()]), status=status,
                num_tol=num_tol, coef_tol=coef_tol)


def triplet_bwd(sel_idx, sel_coef, denom, gscale=1.0):
    """dS + dS^T with dS[i][n_i] = +c_i, dS[i][p_i] = -c_i, c_i = gscale/denom * sel_coef[i]  (rows with sel_idx -1 contribute nothing)."""
    sel_idx = np.asarray(sel_idx)
    nb = sel_idx.shape[0]
    c = np.asarray(sel_coef, F64)
    dS = np.zeros((nb, nb))
    for i in range(nb):
        p, q = sel_idx[i]
        if q >= 0:
            dS[i, q] += c[i]
        if p >= 0:
            dS[i, p] -= c[i]
    return (dS + dS.T) * (f32(gscale) / float(denom))


def sums_tol(row_tol, sums):
    """sums = fl32(sum in double of the fp32 row statistics): the rows' own bounds add up, the double sum is exact to 2^-53 relative per
    addition (nothing beside u), and the final rounding to fp32 is u|sum|."""
    return float(np.sum(row_tol)) + U * abs(float(sums)) + FLT_MIN


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Adam (torch.optim.Adam: L2 decay folded into the gradient, NOT AdamW) and the EMA of the momentum model
# ---------------------------------------------------------------------------------------------------------------------------------------------
def adam_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    """-> (p', m', v').  gg = g grad_scale + wd p;  m' = b1 m + (1-b1) gg;  v' = b2 v + (1-b2) gg^2;
    p' = p - lr/(1 - b1^t) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps)."""
    p, g, m, v = (np.asarray(a, F64) for a in (p, g, m, v))
    b1, b2 = f32(beta1), f32(beta2)
    gg = g * f32(grad_scale) + f32(weight_decay) * p
    m1 = b1 * m + (1.0 - b1) * gg
    v1 = b2 * v + (1.0 - b2) * gg * gg
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p1 = p - (f32(lr) / bc1) * (m1 / (np.sqrt(v1) / math.sqrt(bc2) + f32(eps)))
    return p1, m1, v1


def adam_moment_tols(p, g, m, v, beta1, beta2, weight_decay, grad_scale=1.0):
    """-> (bound of exp_avg, bound of exp_avg_sq) after one call from the given state.
    gg = fl(fl(g gs) + fl(wd p)): |d gg| <= u (|g gs| + |wd p| + |gg|) <= 2u (|g gs| + |wd p|) =: u G.
    m' = fl(fl(b1 m) + fl((1-b1) gg)); 1 - b1 is exact in fp32 for b1 in [0.5, 1] (Sterbenz):
         u (|b1 m| + (1-b1)|gg| + |m'|) + (1-b1) u G.
    v' = fl(fl(b2 v) + fl(fl((1-b2) gg) gg)): u (b2 v + 2 (1-b2) gg^2 + v') + 2 (1-b2) |gg| u G.  gg^2 may fall below FLT_MIN."""
    p, g, m, v = (np.asarray(a, F64) for a in (p, g, m, v))
    b1, b2 = f32(beta1), f32(beta2)
    a, b = np.abs(g * f32(grad_scale)), np.abs(f32(weight_decay) * p)
    gg = g * f32(grad_scale) + f32(weight_decay) * p
    G = 2.0 * (a + b)
    m1 = b1 * m + (1.0 - b1) * gg
    v1 = b2 * v + (1.0 - b2) * gg * gg
    tm = U * (np.abs(b1 * m) + (1.0 - b1) * np.abs(gg) + np.abs(m1) + (1.0 - b1) * G)
    tv = U * (b2 * v + 2.0 * (1.0 - b2) * gg * gg + v1 + 2.0 * (1.0 - b2) * np.abs(gg) * G)
    nz = (a + b) > 0
    hi = 1.0 + 2.0 ** -20                               # second-order terms (at most 8 roundings: 8u relative to the bound) and the reference's own
    return tm * hi + FLT_MIN * nz, tv * hi + FLT_MIN * nz


def ema(mom, theta, beta):
    """beta mom + (1 - beta) theta"""
    b = f32(beta)
    return b * np.asarray(mom, F64) + (1.0 - b) * np.asarray(theta, F64)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# input families (shared by tests/test_gpu_loss_kernels.py and tests/test_loss_kernels_ref_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------------------------------
WEIGHTS = np.array([1.0, 0.8, 0.6, 0.4, 0.2, 0.1], F32)        # values the distortion table takes


def class_ids(n):
    return (np.arange(n) * 3 + 7).astype(np.int32)              # non-contiguous; 5 is never an id


def scattered_labels(counts, rng):
    """one entry per proxy / center: class c appears counts[c] times, positions shuffled"""
    lab = np.repeat(class_ids(len(counts)), counts)
    return lab[rng.permutation(len(lab))].astype(np.int32)


def ragged_counts(total, kmax):
    """counts 1, 2, .., kmax, 1, 2, .. summing to exactly `total`"""
    counts, c = [], 0
    while sum(counts) < total:
        counts.append(min(1 + c % kmax, total - sum(counts)))
        c += 1
    return np.array(counts)


def values(nb, n, family, rng):
    """'random': uniform in [-1, 1).  'ties': multiples of 2^-5 in [-1, 1], so equal values abound."""
    x = rng.uniform(-1.0, 1.0, size=(nb, n))
    if family == "ties":
        x = np.round(x * 32.0) / 32.0
    return x.astype(F32)


def raise_positives(S, y, lab, family):
    """similarities to the row's own identity moved up (still multiples of 2^-5 in the tie family, so a positive can equal a negative)"""
    mask = lab[None, :] == y[:, None]
    up = np.minimum(S + F32(0.25), F32(1.0)) if family == "ties" else (F32(0.5) + F32(0.5) * S).astype(F32)
    return np.where(mask, up, S).astype(F32)


def plant_ties(S, y, lab, rng):
    """The proxy head's tie family.  The quantised background is pushed below 1/2; then, per row with n positives, n // 2 other-id entries
    anywhere in the row are set to 1 and n - n // 2 + 1 .. + 3 more to 31/32 (every 256-entry stretch of a row gets its share over a batch),
    plus one 31/32 a multiple of 256 columns behind the first of them where the row is long enough.
    The k = n selected negatives are all the ones, wherever they lie, and the first by index of the 31/32s, of which at least one is always
    left out: a tie at the selection boundary in every row that has enough negatives.  The positives take 15/16, 31/32 or 1, so positives
    equal negatives."""
    S = (np.minimum(S, F32(0.5))).astype(F32)
    levels = np.array([0.9375, 0.96875, 1.0], F32)
    for i in range(S.shape[0]):
        pos = np.flatnonzero(lab == y[i])
        neg = np.flatnonzero(lab != y[i])
        n = max(len(pos), 1)
        pick = rng.choice(neg, min(len(neg), n + 1 + int(rng.integers(0, 3))), replace=False)
        S[i, pick] = levels[1]
        S[i, pick[:n // 2]] = levels[2]
        S[i, pos] = levels[rng.integers(0, 3, len(pos))]
        # the lowest-index 31/32 is always selected; a second 31/32 a multiple of 256 columns further on sits in the same thread's registers
        # (entry j is held by thread j % 256), so a tie is also broken inside one thread, not only between threads
        if len(pick) > n // 2:
            j0 = int(pick[n // 2:].min())
            later = np.arange(j0 + 256, S.shape[1], 256)
            later = later[(lab[later] != y[i]) & (S[i, later] < levels[1])]
            if len(later):
                S[i, later[i % len(later)]] = levels[1]
    return S


def head_inputs(nb, counts, family, seed, unknown_rows=0, raise_pos=True, y=None):
    """-> S [nb, sum(counts)] fp32, y [nb] int32, lab int32, w [nb] fp32.  ``unknown_rows`` leading rows carry an id nothing is labelled with.
    families: 'random', 'ties' (quantised everywhere), 'planted' (plant_ties)."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts)
    lab = scattered_labels(counts, rng)
    drawn = class_ids(len(counts))[rng.integers(0, len(counts), nb)]
    y = drawn if y is None else np.asarray(y)                 # given labels are in place before any tie is planted against them
    y[:unknown_rows] = 5
    S = values(nb, len(lab), "ties" if family == "planted" else family, rng)
    if family == "planted":
        S = plant_ties(S, y, lab, rng)
    elif raise_pos:
        S = raise_positives(S, y, lab, family)
    w = WEIGHTS[rng.integers(0, len(WEIGHTS), nb)]
    return S, y.astype(np.int32), lab, w


def with_argmax_ties(S, same_lane):
    """The two largest entries of every row made equal (row max + 1/8): in different lanes of the wave (column mod 64 differs), or in the same
    lane (columns 64 apart; needs more than 64 columns).  -> (S', expected arg-max = the lower of the two columns)."""
    S = S.copy()
    nb, NC = S.shape
    rng = np.random.default_rng(NC * 1000 + nb)
    first = np.empty(nb, np.int64)
    for i in range(nb):
        if same_lane:
            a = int(rng.integers(0, NC - 64))
            b = a + 64 * int(rng.integers(1, (NC - 1 - a) // 64 + 1))
        else:
            a, b = sorted(rng.choice(NC, 2, replace=False))
            if (b - a) % 64 == 0:
                b = b - 1 if b - 1 > a else b + 1
        top = F32(S[i].max() + F32(0.125))
        S[i, a] = S[i, b] = top
        first[i] = min(a, b)
    return S, first


def top_two_separated(S, rel=2.0 ** -21):
    """Rows whose arg-max can be compared exactly: the two largest entries are equal, or far enough apart that their fp32 products with 1/tau
    cannot coincide (a product moves a value by at most u relative; 8u apart is asked for).  -> bool [nb]"""
    t = np.sort(np.asarray(S, F64), axis=1)[:, -2:] if S.shape[1] > 1 else np.repeat(np.asarray(S, F64), 2, axis=1)
    gap = t[:, 1] - t[:, 0]
    return (gap == 0) | (gap > rel * np.maximum(np.abs(t[:, 1]), np.abs(t[:, 0])))


def boundary_tie_fraction(S, y, pl, sel_idx, kmax):
    """fraction of rows with negatives whose k-th selected negative equals the best rejected one"""
    hit = rows = 0
    for i in range(S.shape[0]):
        neg = sel_idx[i, kmax:]
        neg = neg[neg >= 0]
        if len(neg) == 0:
            continue
        rejected = np.ones(S.shape[1], bool)
        rejected[neg] = False
        rejected &= np.asarray(pl) != y[i]
        if not rejected.any():
            continue
        rows += 1
        hit += S[i, rejected].max() == S[i, neg[-1]]
    return hit / max(rows, 1)


def same_thread_tie_rows(S, y, pl, sel_idx, kmax):
    """number of rows in which a selected negative has an equal-valued negative a multiple of 256 columns behind it: both are held by one
    thread of the register path, which must then prefer the lower index itself"""
    rows = 0
    for i in range(S.shape[0]):
        neg = sel_idx[i, kmax:]
        hit = False
        for j in neg[neg >= 0]:
            later = np.arange(j + 256, S.shape[1], 256)
            hit = hit or bool(np.any((S[i, later] == S[i, j]) & (np.asarray(pl)[later] != y[i])))
        rows += hit
    return rows


def _per(n_classes, per):
    return np.full(n_classes, per)


def _split(total, per):
    """`total` entries in classes of `per`, the last class ragged"""
    return np.array([per] * (total // per) + ([total % per] if total % per else []))


_FAMILY = {"random": "random", "ties": "planted"}          # the proxy cases named *_ties use the planted tie family


PROXY_CASE_NAMES = tuple(sorted(
    ["%s_%s" % (n, f) for n in ("np5120", "np3755", "np2253", "np255", "np256", "np257", "np4096", "np4097") for f in ("random", "ties")]
    + ["nb1_ties", "nb3_ties", "nb261_ties", "tiny_np5", "tiny_all_positive", "tiny_np1", "kmax_exact", "kmax_plus1", "tau0p01"]))


def proxy_cases(kmax):
    """name -> (S, y, pl, w, tau): the proxy-forward inputs of the GPU tests.  Rows of at most 4096 proxies take the kernel's register path
    (NP = 3755 and 2253 are Market-1501 at 5 and 3 proxies per identity), longer ones its re-reading path (NP = 5120 is the benchmarked one)."""
    c = {}
    seed = 1000
    for name, nb, counts, unknown in (("np5120", 256, _per(1024, 5), 0), ("np3755", 256, _per(751, 5), 7), ("np2253", 256, _per(751, 3), 0),
                                      ("np255", 256, ragged_counts(255, kmax), 0), ("np256", 256, ragged_counts(256, kmax), 0),
                                      ("np257", 256, ragged_counts(257, kmax), 3), ("nb1", 1, _per(751, 3), 0), ("nb3", 3, _per(751, 3), 0),
                                      ("nb261", 261, _per(751, 5), 0)):
        for family, tau in (("random", 0.05), ("ties", 0.1)) if nb == 256 else (("ties", 0.05),):
            seed += 1
            c["%s_%s" % (name, family)] = head_inputs(nb, counts, _FAMILY[family], seed, unknown) + (tau,)
    # 4096 / 4097: ragged 1..kmax per class; the 4097th proxy has an id of its own and the lowest value, so both row lengths (register path,
    # re-reading path) must select exactly the same
    for family, tau in (("random", 0.1), ("ties", 0.05)):
        seed += 1
        S, y, pl, w = head_inputs(256, ragged_counts(4096, kmax), _FAMILY[family], seed)
        c["np4096_" + family] = (S, y, pl, w, tau)
        S1 = np.concatenate([S, np.full((256, 1), -1.0, F32)], axis=1)
        c["np4097_" + family] = (S1, y, np.concatenate([pl, np.array([4], np.int32)]), w, tau)
    S, y, pl, w = head_inputs(8, np.array([3, 2]), "planted", 77, y=np.array([7, 10] * 4, np.int32))
    c["tiny_np5"] = (S, y, pl, w, 0.1)                                                   # n = 3 -> k = 2; n = 2 -> k = 2
    S, y, pl, w = head_inputs(4, np.array([4]), "random", 78)
    c["tiny_all_positive"] = (S, y, pl, w, 0.05)                                         # NP = n: k = 0
    S, y, pl, w = head_inputs(3, np.array([1]), "random", 79, unknown_rows=1)
    c["tiny_np1"] = (S, y, pl, w, 0.05)
    S, y, pl, w = head_inputs(256, np.array([kmax, 3, 5, 1, kmax, 2] * 20), "planted", 80)
    c["kmax_exact"] = (S, y, pl, w, 0.05)
    S, y, pl, w = head_inputs(256, np.array([kmax, 3, 5, kmax + 1, 1, 2] * 20), "planted", 81)
    c["kmax_plus1"] = (S, y, pl, w, 0.05)
    S, y, pl, w = head_inputs(256, _per(751, 3), "random", 82, raise_pos=False)
    c["tau0p01"] = (S, y, pl, w, 0.01)                                                   # |S/tau| up to 100
    return c


_CENTER_SHAPES = ((256, 1024, 1, "random", 0.05, 0), (256, 1024, 2, "ties", 0.1, 0), (256, 1024, 3, "random", 0.01, 4),
                  (256, 751, 1, "random", 0.1, 0), (256, 751, 3, "ties", 0.05, 0), (3, 4, 2, "random", 0.1, 0),
                  (261, 130, 2, "random", 0.05, 5), (5, 63, 1, "random", 0.05, 0), (5, 64, 2, "random", 0.05, 1),
                  (5, 65, 3, "random", 0.05, 0))            # nb, NC, centers per identity, family, tau, rows of an unknown identity


def _center_names(nb, NC, per, family, tau):
    name = "%dx%d_c%d_%s_t%s" % (nb, NC, per, family, str(tau).replace(".", "p"))
    if family != "random":
        return [name]
    return [name, name + "_tie_lanes"] + ([name + "_tie_samelane"] if NC > 64 else [])


CENTER_CASE_NAMES = tuple(sorted(n for c in _CENTER_SHAPES for n in _center_names(*c[:5])))


def center_cases():
    """name -> (S, y, cl, w, tau, expected arg-max or None): the center-head inputs of the GPU tests"""
    c = {}
    seed = 2100
    for nb, NC, per, family, tau, unknown in _CENTER_SHAPES:
        seed += 1
        S, y, cl, w = head_inputs(nb, _split(NC, per), family, seed, unknown, raise_pos=tau != 0.01)
        name = _center_names(nb, NC, per, family, tau)[0]
        c[name] = (S, y, cl, w, tau, None)
        if family == "random":
            S2, first = with_argmax_ties(S, same_lane=False)
            c[name + "_tie_lanes"] = (S2, y, cl, w, tau, first)
            if NC > 64:
                S3, first = with_argmax_ties(S, same_lane=True)
                c[name + "_tie_samelane"] = (S3, y, cl, w, tau, first)
    return c


def crafted_selection(nb, NPROX, kmax, rng):
    """selections independent of any forward: 0..kmax positives and negatives per row, empty slots -1 with a garbage coefficient; dyadic
    coefficients (multiples of 2^-4)"""
    sel_idx = np.full((nb, 2 * kmax), -1, np.int32)
    sel_coef = np.full((nb, 2 * kmax), 123.4375, np.float32)            # garbage in the empty slots
    for i in range(nb):
        n, k = (int(v) for v in rng.integers(0, kmax + 1, 2))
        pick = rng.choice(NPROX, n + k, replace=False)
        sel_idx[i, :n], sel_idx[i, kmax:kmax + k] = pick[:n], pick[n:]
        sel_coef[i, :n] = rng.integers(-64, 65, n) / 16.0
        sel_coef[i, kmax:kmax + k] = rng.integers(-64, 65, k) / 16.0
    sel_idx[0], sel_coef[0] = -1, 7.5                                    # a row with nothing selected
    return sel_idx, sel_coef


PROXY_BWD_DIMS = (1, 100, 768, 2048)


def proxy_bwd_random_inputs(D, kmax):
    """-> sel_idx, sel_coef, P, denom, gscale, base: the random-data case of the proxy backward at embedding width D (empty slots keep a
    non-zero coefficient; ``base`` is what the output buffer holds before an accumulating call)"""
    rng = np.random.default_rng(400 + D)
    nb, NPROX = 61, 300
    sel_idx, _ = crafted_selection(nb, NPROX, kmax, rng)
    sel_coef = rng.standard_normal((nb, 2 * kmax)).astype(np.float32)
    P = rng.standard_normal((NPROX, D)).astype(np.float32)
    base = rng.standard_normal((nb, D)).astype(np.float32)
    return sel_idx, sel_coef, P, F32(37.3), 0.4, base


def triplet_inputs(nb, family, seed, lonely_row=True):
    """-> S [nb, nb] fp32 (not symmetric: the kernel reads row i only), y, w.  ``lonely_row``: row 0's identity appears nowhere else."""
    rng = np.random.default_rng(seed)
    n_ids = max(2, nb // 4)
    y = class_ids(n_ids)[rng.integers(0, n_ids, nb)]
    y[-1] = class_ids(n_ids)[0] if y[0] != class_ids(n_ids)[0] else class_ids(n_ids)[1]
    if lonely_row:
        y[0] = 5
    S = values(nb, nb, family, rng)
    w = WEIGHTS[rng.integers(0, len(WEIGHTS), nb)]
    if family == "ties":
        S, y = plant_triplet_ties(S, y)
    return S, y.astype(np.int32), w


def _pair(cols, same_lane):
    """the first two of `cols` (ascending) that lie 0 mod 64 apart (one lane of the wave reads both), or that do not; None if there is none"""
    for a in range(len(cols)):
        for b in range(a + 1, len(cols)):
            if ((cols[b] - cols[a]) % 64 == 0) == same_lane:
                return cols[a], cols[b]
    return None


def plant_triplet_ties(S, y):
    """The quantised values tie by themselves only among the many negatives.  Here, in three rows of four, two same-identity columns are set
    to 1/32 below the row's lowest positive and two other-identity columns to 1/32 above its highest negative: the hardest positive and the
    hardest negative are both tied, and the lower column must win.  Odd rows take pairs 64 columns apart where they exist (one lane of the
    wave holds both), the others pairs in different lanes.  For the former, batches of more than 64 get identities with members 64 apart."""
    S, y = S.copy(), y.copy()
    nb = len(y)
    for a in range(1, nb - 65, 8):
        y[a + 64] = y[a]
    for i in range(1, nb):
        if i % 4 == 0:
            continue
        same, other = np.flatnonzero(y == y[i]), np.flatnonzero(y != y[i])
        for cols, val in ((same, S[i, same].min() - F32(2.0 ** -5)), (other, S[i, other].max() + F32(2.0 ** -5))):
            pair = (_pair(cols, True) if i % 2 else None) or _pair(cols, False)
            if pair is not None:
                S[i, list(pair)] = val
    return S, y


def triplet_tie_rows(S, y, sel_idx):
    """-> {'pos_lanes', 'pos_samelane', 'neg_lanes', 'neg_samelane'}: the number of rows whose selected hardest positive (negative) has an
    equal-valued candidate in another lane of the wave (column differs mod 64) / in the same lane"""
    out = dict.fromkeys(("pos_lanes", "pos_samelane", "neg_lanes", "neg_samelane"), 0)
    for i in range(S.shape[0]):
        for kind, j, cand in (("pos", sel_idx[i, 0], y == y[i]), ("neg", sel_idx[i, 1], y != y[i])):
            if j < 0:
                continue
            tied = np.flatnonzero(cand & (S[i] == S[i, j]))
            tied = tied[tied != j]
            out[kind + "_samelane"] += bool(np.any((tied - j) % 64 == 0))
            out[kind + "_lanes"] += bool(np.any((tied - j) % 64 != 0))
    return out
