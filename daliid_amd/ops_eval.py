"""Python entry points of the evaluation kernels (thin wrappers over the C ABI)."""
import numpy as np
import torch

from . import _lib

METRIC_COSINE, METRIC_L2SQ, METRIC_DOT = 0, 1, 2
PREC_BF16X3, PREC_BF16 = 0, 1
_PREC = {"bf16x3": PREC_BF16X3, "bf16": PREC_BF16}
_METRIC = {"cosine": METRIC_COSINE, "l2sq": METRIC_L2SQ, "dot": METRIC_DOT}


def l2norm_rows(x, eps=0.0, return_norms=False):
    """y = x / (|x| + eps) per row (validateModels.py:41-42 eps=0; train_encodersKIT.py:198 eps=1e-9)."""
    assert x.dim() == 2
    y = torch.empty_like(x)
    norms = torch.empty(x.shape[0], device=x.device, dtype=torch.float32) if return_norms else None
    _lib.check(_lib.lib().dali_l2norm_rows(_lib.ctx(x.device), _lib.stream_ptr(), _lib.ptr(x, torch.float32, "x"),
                                            x.shape[0], x.shape[1], float(eps), _lib.ptr(y), _lib.ptr(norms)),
               "dali_l2norm_rows")
    return (y, norms) if return_norms else y


def l2norm_rows_bwd(x, dy, eps=0.0):
    dx = torch.empty_like(x)
    _lib.check(_lib.lib().dali_l2norm_rows_bwd(_lib.ctx(x.device), _lib.stream_ptr(), _lib.ptr(x, torch.float32, "x"),
                                                _lib.ptr(dy, torch.float32, "dy"), x.shape[0], x.shape[1], float(eps),
                                                _lib.ptr(dx)), "dali_l2norm_rows_bwd")
    return dx


def pairdist(q, g, metric="cosine", precision="bf16x3", normalize=False, out=None):
    """distmat[nq,ng] fp32 on the GPU: 1 - q@g.T (validateModels.py:47) or squared L2."""
    assert q.dim() == 2 and g.dim() == 2 and q.shape[1] == g.shape[1]
    nq, ng, d = q.shape[0], g.shape[0], q.shape[1]
    if out is None:
        out = torch.empty(nq, ng, device=q.device, dtype=torch.float32)
    if nq == 0 or ng == 0:
        return out
    _lib.check(_lib.lib().dali_pairdist(_lib.ctx(q.device), _lib.stream_ptr(), _lib.ptr(q, torch.float32, "q"),
                                         _lib.ptr(g, torch.float32, "g"), nq, ng, d, _METRIC[metric], _PREC[precision],
                                         int(bool(normalize)), _lib.ptr(out, torch.float32, "out")), "dali_pairdist")
    return out


class PreparedRows:
    """bf16 operand image of a feature matrix (dali_pairdist_prepare): opaque bytes + the squared row norms."""

    def __init__(self, x, normalize=False, precision="bf16x3"):
        assert x.dim() == 2
        self.n, self.d = x.shape
        self.precision = precision
        L = _lib.lib()
        nbytes = int(L.dali_pairdist_operand_bytes(self.n, self.d, _PREC[precision]))
        self.image = torch.empty(max(nbytes, 16), device=x.device, dtype=torch.uint8)
        self.sq = torch.empty(max(self.n, 1), device=x.device, dtype=torch.float32)
        _lib.check(L.dali_pairdist_prepare(_lib.ctx(x.device), _lib.stream_ptr(), _lib.ptr(x, torch.float32, "x"), self.n, self.d,
                                           int(bool(normalize)), _PREC[precision], _lib.ptr(self.image), _lib.ptr(self.sq)),
                   "dali_pairdist_prepare")


def pairdist_prepared(qp, gp, metric="cosine", out=None):
    assert qp.d == gp.d and qp.precision == gp.precision
    if out is None:
        out = torch.empty(qp.n, gp.n, device=qp.image.device, dtype=torch.float32)
    _lib.check(_lib.lib().dali_pairdist_prepared(_lib.ctx(out.device), _lib.stream_ptr(), _lib.ptr(qp.image), _lib.ptr(qp.sq),
                                                  _lib.ptr(gp.image), _lib.ptr(gp.sq), qp.n, gp.n, qp.d, _METRIC[metric],
                                                  _PREC[qp.precision], _lib.ptr(out, torch.float32, "out")),
               "dali_pairdist_prepared")
    return out


TOPK_K_MAX = 128          # keys per row the selection kernels keep (include/daliid.h, dali_topk_rows)


def _topk_k(k, avail, running, who):
    """k as the C entries take it: refused beyond the documented cap, clamped to the columns available when no list is being continued."""
    k = int(k)
    if k < 1:
        raise ValueError("%s: k=%d" % (who, k))
    if k > TOPK_K_MAX:
        raise _lib.DaliError("%s: k=%d above the documented cap %d" % (who, k, TOPK_K_MAX))
    if running is not None:
        if running.dim() != 2 or running.shape[1] != k or running.dtype != torch.int64:
            raise ValueError("%s: running must be the int64 [nq, %d] keys of an earlier call" % (who, k))
        return k
    return min(k, int(avail))


def topk_decode(keys, largest=False):
    """keys int64 [nq, k] (topk_rows / pairdist_topk, return_keys=True) -> (values fp32 [nq, k], indices int32 [nq, k])."""
    nq, k = keys.shape
    values = torch.empty(nq, k, device=keys.device, dtype=torch.float32)
    indices = torch.empty(nq, k, device=keys.device, dtype=torch.int32)
    if nq and k:
        _lib.check(_lib.lib().dali_topk_decode(_lib.ctx(keys.device), _lib.stream_ptr(), _lib.ptr(keys, torch.int64, "keys"), nq, k,
                                               int(bool(largest)), _lib.ptr(values), _lib.ptr(indices)), "dali_topk_decode")
    return values, indices


def topk_rows(distmat, k, largest=False, col_offset=0, running=None, return_keys=False):
    """The k best entries of every row of a CUDA fp32 matrix in the order of include/daliid.h (dali_topk_rows): ascending values
    (descending for ``largest``), exact ties by ascending index, -0.0 == +0.0, NaN last.  -> (values fp32 [nq, k], indices int32 [nq, k]
    [, keys int64 [nq, k]]) on the device, enqueued on the current stream.  ``distmat`` may be a column slice of a contiguous matrix
    (read by its pitch); its column j has index ``col_offset + j``.  ``running``: the keys of an earlier call on other columns of the
    same rows; the result is then the selection over both (the tensor passed in is left unchanged).  Without ``running`` k is clamped to
    the number of columns."""
    if distmat.dim() != 2:
        raise ValueError("topk_rows: distmat must be 2-D")
    nq, ncols = distmat.shape
    k = _topk_k(k, ncols, running, "topk_rows")
    if distmat.dtype != torch.float32 or not distmat.is_cuda:
        raise _lib.DaliError("topk_rows: distmat must be a CUDA float32 tensor")
    if ncols > 0 and nq > 0 and not (distmat.stride(1) == 1 and (nq == 1 or distmat.stride(0) >= ncols)):
        distmat = distmat.contiguous()
    ld = max(int(distmat.stride(0)), ncols) if nq > 1 else ncols
    dev = distmat.device
    if running is not None:
        if running.shape[0] != nq:
            raise ValueError("topk_rows: running has %d rows, distmat %d" % (running.shape[0], nq))
        keys = running.to(dev).contiguous().clone()
    else:
        keys = torch.empty(nq, k, device=dev, dtype=torch.int64)
    if nq > 0 and k > 0:
        _lib.check(_lib.lib().dali_topk_rows(_lib.ctx(dev), _lib.stream_ptr(), _lib.c_void_p(distmat.data_ptr()), nq, ncols, ld, int(col_offset), k,
                                             int(bool(largest)), int(running is not None), _lib.ptr(keys)), "dali_topk_rows")
    out = topk_decode(keys, largest)
    return out + (keys,) if return_keys else out


def pairdist_topk(q, g, k, metric="cosine", precision="bf16x3", normalize=False, largest=False, g_offset=0, running=None, return_keys=False,
                  return_stats=False, _tuning=None):
    """The k nearest gallery rows of every query WITHOUT the [nq, ng] matrix (include/daliid.h, dali_pairdist_topk): exactly
    ``topk_rows(pairdist_prepared(q, g, metric), k, largest, col_offset=g_offset)``, values bitwise those of the matrix, computed by the
    same distance kernel with a selecting epilogue.  q, g: fp32 feature tensors (prepared here with ``normalize`` / ``precision``) or
    ``PreparedRows``.  ``g_offset`` / ``running``: a gallery fed in slices (or held in shards) gives the lists of the whole.
    -> (values fp32 [nq, k], indices int32 [nq, k] [, keys int64] [, stats int32 [3] on the device: gallery rows selected in the
    epilogue, rows taken through the matrix block, overflow events]).  ``_tuning`` = (boot_cols, chunk_cols, cand_cap) is for tests."""
    qp = q if isinstance(q, PreparedRows) else PreparedRows(q.contiguous(), normalize=normalize, precision=precision)
    gp = g if isinstance(g, PreparedRows) else PreparedRows(g.contiguous(), normalize=normalize, precision=precision)
    assert qp.d == gp.d and qp.precision == gp.precision
    nq, ng = qp.n, gp.n
    k = _topk_k(k, ng, running, "pairdist_topk")
    dev = qp.image.device
    boot, chunk, cap = (int(v) for v in _tuning) if _tuning is not None else (0, 0, 0)
    if running is not None:
        if running.shape[0] != nq:
            raise ValueError("pairdist_topk: running has %d rows for %d queries" % (running.shape[0], nq))
        keys = running.to(dev).contiguous().clone()
    else:
        keys = torch.empty(nq, k, device=dev, dtype=torch.int64)
    stats = torch.zeros(3, device=dev, dtype=torch.int32)
    if nq > 0 and k > 0:
        _lib.check(_lib.lib().dali_pairdist_topk(_lib.ctx(dev), _lib.stream_ptr(), _lib.ptr(qp.image), _lib.ptr(qp.sq), _lib.ptr(gp.image),
                                                 _lib.ptr(gp.sq), nq, ng, qp.d, _METRIC[metric], _PREC[qp.precision], k, int(bool(largest)),
                                                 int(g_offset), int(running is not None), _lib.ptr(keys), boot, chunk, cap, _lib.ptr(stats)),
                   "dali_pairdist_topk")
    out = topk_decode(keys, largest)
    if return_keys:
        out += (keys,)
    if return_stats:
        out += (stats,)
    return out


def factorize_ids(*arrays):
    """Shared int32 codes for id columns (the reference carries pids / camids as numpy strings)."""
    flat = np.concatenate([np.asarray(a).ravel() for a in arrays])
    _, inv = np.unique(flat, return_inverse=True)
    out, o = [], 0
    for a in arrays:
        n = np.asarray(a).size
        out.append(inv[o:o + n].astype(np.int32))
        o += n
    return out


def rank_eval_codes(distmat, qp, gp, qc, gc, max_rank=50):
    """Device-side part of rank_eval: ids already int32 codes on the GPU.  -> dict of device tensors (no host sync)."""
    nq, ng = distmat.shape
    dev = distmat.device
    max_rank = min(max_rank, ng)
    out = dict(cmc=torch.empty(max_rank, device=dev, dtype=torch.float32), mAP=torch.empty(1, device=dev, dtype=torch.float32),
               map64=torch.empty(1, device=dev, dtype=torch.float64), nvalid=torch.empty(1, device=dev, dtype=torch.int32),
               status=torch.empty(1, device=dev, dtype=torch.int32), ap=torch.empty(nq, device=dev, dtype=torch.float32),
               first_rank=torch.empty(nq, device=dev, dtype=torch.int32))
    _lib.check(_lib.lib().dali_rank_eval(_lib.ctx(dev), _lib.stream_ptr(), _lib.ptr(distmat, torch.float32, "distmat"),
                                          _lib.ptr(qp, torch.int32), _lib.ptr(gp, torch.int32), _lib.ptr(qc, torch.int32), _lib.ptr(gc, torch.int32),
                                          nq, ng, max_rank, _lib.ptr(out["cmc"]), _lib.ptr(out["mAP"]), _lib.ptr(out["map64"]),
                                          _lib.ptr(out["nvalid"]), _lib.ptr(out["ap"]), _lib.ptr(out["first_rank"]), _lib.ptr(out["status"])),
               "dali_rank_eval")
    return out


def rank_eval(distmat, q_pids, g_pids, q_camids, g_camids, max_rank=50, return_per_query=False):
    """market1501 CMC/mAP of torchreid.metrics.evaluate_rank (validateModels.py:68) on the GPU.
    distmat: CUDA fp32 [nq,ng].  Returns (cmc numpy float32 [max_rank], mAP float)."""
    dev = distmat.device
    qp, gp = factorize_ids(q_pids, g_pids)
    qc, gc = factorize_ids(q_camids, g_camids)
    t = lambda a: torch.from_numpy(a).to(dev)
    o = rank_eval_codes(distmat, t(qp), t(gp), t(qc), t(gc), max_rank)
    st = int(o["status"].item())
    if st != 0:
        raise _lib.DaliError("dali_rank_eval: " + ("a query's identity has more than 4096 gallery entries (documented limit)" if st == 1 else
                                                   "identity codes span more than 2^20 values (documented limit)"))
    if int(o["nvalid"].item()) == 0:
        raise AssertionError("Error: all query identities do not appear in gallery")
    res = (o["cmc"].cpu().numpy(), float(o["map64"].item()))
    if return_per_query:
        return res + (o["ap"].cpu().numpy(), o["first_rank"].cpu().numpy())
    return res


def rank_eval_inp(distmat, q_pids, g_pids, q_camids, g_camids, return_per_query=False):
    """mINP (mean inverse negative penalty) under ``rank_eval``'s protocol and key order (include/daliid.h, dali_rank_eval_inp): per query
    INP = matches / (1-based position of the LAST match among the kept gallery entries); the mean over the valid queries, in fp64.
    -> mINP float [, inp float32 [nq], last_rank int32 [nq] (0-based, -1 = invalid query), n_rel int32 [nq]] as numpy.  Raises what
    ``rank_eval`` raises."""
    dev = distmat.device
    nq, ng = distmat.shape
    qp, gp = factorize_ids(q_pids, g_pids)
    qc, gc = factorize_ids(q_camids, g_camids)
    qp, gp, qc, gc = (torch.from_numpy(a).to(dev) for a in (qp, gp, qc, gc))
    inp = torch.empty(nq, device=dev, dtype=torch.float32)
    last_rank = torch.empty(nq, device=dev, dtype=torch.int32)
    n_rel = torch.empty(nq, device=dev, dtype=torch.int32)
    minp64 = torch.empty(1, device=dev, dtype=torch.float64)
    nvalid = torch.empty(1, device=dev, dtype=torch.int32)
    status = torch.empty(1, device=dev, dtype=torch.int32)
    _lib.check(_lib.lib().dali_rank_eval_inp(_lib.ctx(dev), _lib.stream_ptr(), _lib.ptr(distmat, torch.float32, "distmat"),
                                              _lib.ptr(qp, torch.int32), _lib.ptr(gp, torch.int32), _lib.ptr(qc, torch.int32),
                                              _lib.ptr(gc, torch.int32), nq, ng, _lib.ptr(inp), _lib.ptr(last_rank), _lib.ptr(n_rel),
                                              _lib.ptr(minp64), _lib.ptr(nvalid), _lib.ptr(status)), "dali_rank_eval_inp")
    st = int(status.item())
    if st != 0:
        raise _lib.DaliError("dali_rank_eval_inp: " + ("a query's identity has more than 4096 gallery entries (documented limit)" if st == 1 else
                                                       "identity codes span more than 2^20 values (documented limit)"))
    if int(nvalid.item()) == 0:
        raise AssertionError("Error: all query identities do not appear in gallery")
    minp = float(minp64.item())
    if return_per_query:
        return minp, inp.cpu().numpy(), last_rank.cpu().numpy(), n_rel.cpu().numpy()
    return minp


QE_ALPHA_MAX = 16         # integer exponents the combine kernel builds by repeated multiplication (include/daliid.h, dali_qe_combine)
QE_TIMES_MAX = 8


def _qe_alpha(alpha, who):
    if isinstance(alpha, bool) or float(alpha) != int(alpha) or not 0 <= int(alpha) <= QE_ALPHA_MAX:
        raise ValueError("%s: alpha=%r: only integer exponents 0..%d are built (non-integer exponents are not built)" % (who, alpha, QE_ALPHA_MAX))
    return int(alpha)


def _qe_combine(pool, idx, val, alpha, val_is_distance, out, status):
    """dali_qe_combine on checked tensors; ``status`` (device int32 [1]) collects out-of-range indices and is not read here."""
    n, k = idx.shape
    if n > 0:
        _lib.check(_lib.lib().dali_qe_combine(_lib.ctx(pool.device), _lib.stream_ptr(), _lib.ptr(pool, torch.float32, "pool"), pool.shape[0],
                                              pool.shape[1], _lib.ptr(idx, torch.int32, "idx"), _lib.ptr(val, torch.float32, "val"), n, k,
                                              int(bool(val_is_distance)), alpha, _lib.ptr(out, torch.float32, "out"), _lib.ptr(status)),
                   "dali_qe_combine")
    return out


def qe_combine(pool, idx, val, alpha=3, val_is_distance=False, out=None):
    """out[i] = (1 / k) * sum_j w_ij * pool[idx[i, j]], w = s ** alpha by repeated multiplication, s = val (or 1 - val for
    ``val_is_distance``), in the fixed fp32 order of include/daliid.h (dali_qe_combine).  pool fp32 [n_pool, d], idx int32 [n, k],
    val fp32 [n, k], all CUDA and contiguous; ``out`` fp32 [n, d] must not overlap ``pool``.  An index outside the pool is skipped by the
    kernel and raises ``DaliError`` here (one read of the status word)."""
    if pool.dim() != 2 or idx.dim() != 2 or val.dim() != 2:
        raise ValueError("qe_combine: pool, idx and val must be 2-D")
    if tuple(idx.shape) != tuple(val.shape):
        raise ValueError("qe_combine: idx %s and val %s differ in shape" % (tuple(idx.shape), tuple(val.shape)))
    alpha = _qe_alpha(alpha, "qe_combine")
    if not pool.is_cuda or pool.dtype != torch.float32:
        raise _lib.DaliError("qe_combine: pool must be a CUDA float32 tensor")
    n, d = idx.shape[0], pool.shape[1]
    if out is None:
        out = torch.empty(n, d, device=pool.device, dtype=torch.float32)
    elif tuple(out.shape) != (n, d):
        raise ValueError("qe_combine: out must be [%d, %d], got %s" % (n, d, tuple(out.shape)))
    status = torch.zeros(1, device=pool.device, dtype=torch.int32)
    _qe_combine(pool, idx, val, alpha, val_is_distance, out, status)
    if n > 0 and int(status.item()) != 0:
        raise _lib.DaliError("dali_qe_combine: a neighbour index lies outside the pool of %d rows (its term was skipped)" % pool.shape[0])
    return out


def query_expansion(q, g, k=10, alpha=3.0, times=1, expand="all", precision="bf16x3"):
    """Average / alpha-weighted query expansion and database augmentation without the (Nq + Ng)^2 similarity matrix: every feature row is
    replaced by the mean of its k nearest rows (itself included) weighted by cosine similarity ** alpha, ``times`` times.
    expand="all" (fast-reid's aqe): the pool is [q; g], every row is expanded, the result is split back at Nq.  expand="gallery" (DBA): the
    pool is g, only gallery rows are expanded and ``q`` is returned as it came.  Each iteration: PreparedRows(feat, normalize=True) ->
    pairdist_topk(P, P, k, "cosine") (ascending distance, ties by ascending index) -> dali_qe_combine on the UN-normalised current
    features with weights (1 - distance) ** alpha.  Nothing synchronises inside the loop; the status word is read once at the end.
    -> (q', g') fp32 CUDA tensors."""
    who = "query_expansion"
    if expand not in ("all", "gallery"):
        raise ValueError("%s: expand must be 'all' or 'gallery', got %r" % (who, expand))
    alpha = _qe_alpha(alpha, who)
    if isinstance(times, bool) or int(times) != times or not 1 <= int(times) <= QE_TIMES_MAX:
        raise ValueError("%s: times=%r outside 1..%d" % (who, times, QE_TIMES_MAX))
    if q.dim() != 2 or g.dim() != 2 or q.shape[1] != g.shape[1]:
        raise ValueError("%s: q %s and g %s must be 2-D with one width" % (who, tuple(q.shape), tuple(g.shape)))
    if not q.is_cuda or not g.is_cuda:
        raise _lib.DaliError("%s: q and g must be CUDA tensors" % who)
    nq = q.shape[0]
    if expand == "all":
        feat = torch.cat([q.to(torch.float32), g.to(torch.float32)])
        own = [feat]                             # the two buffers that ping-pong; the caller's gallery is never one of them
    else:
        feat, own = g.to(torch.float32).contiguous(), []
    if feat.shape[0] == 0:
        raise ValueError("%s: nothing to expand (empty pool)" % who)
    k = _topk_k(k, feat.shape[0], None, who)
    status = torch.zeros(1, device=feat.device, dtype=torch.int32)
    for _ in range(int(times)):
        out = next((b for b in own if b is not feat), None)
        if out is None:
            out = torch.empty_like(feat)
            own.append(out)
        P = PreparedRows(feat, normalize=True, precision=precision)
        dist, idx = pairdist_topk(P, P, k, metric="cosine")
        feat = _qe_combine(feat, idx, dist, alpha, True, out, status)
    if int(status.item()) != 0:
        raise _lib.DaliError("dali_qe_combine: a neighbour index lies outside the pool (its term was skipped)")
    if expand == "all":
        return feat[:nq], feat[nq:]
    return q, feat


RANK_PMAX = 4096          # matches + junk of one query the ranking kernels hold in LDS (csrc/rank.hip)


def shard_bounds(n, world):
    """Contiguous gallery slices of (almost) equal size, multiples of 128 rows (the distance kernel's gallery tile) where possible:
    -> list of world + 1 offsets."""
    per = -(-n // world)
    per = -(-per // 128) * 128
    return [min(r * per, n) for r in range(world + 1)]


def rank_shard_matches(dist_shard, qp, gp, qc, gc, g_offset, cap):
    """Step 1 (device, int32 code tensors): -> (keys int64 [nq, cap], counts int32 [nq], status int32 [1])."""
    nq, ng = dist_shard.shape
    dev = dist_shard.device
    keys = torch.full((nq, cap), -1, device=dev, dtype=torch.int64)
    counts = torch.zeros(nq, device=dev, dtype=torch.int32)
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    if ng > 0:
        _lib.check(_lib.lib().dali_rank_shard_matches(_lib.ctx(dev), _lib.stream_ptr(), _lib.ptr(dist_shard, torch.float32, "dist_shard"),
                                                       _lib.ptr(qp, torch.int32), _lib.ptr(gp, torch.int32), _lib.ptr(qc, torch.int32),
                                                       _lib.ptr(gc, torch.int32), nq, ng, int(g_offset), cap, _lib.ptr(keys), _lib.ptr(counts),
                                                       _lib.ptr(status)), "dali_rank_shard_matches")
    return keys, counts, status


def rank_shard_bins(dist_shard, qp, gp, qc, gc, g_offset, keys_all, counts_all, bins_cap):
    """Step 3: keys_all int64 [world, nq, cap], counts_all int32 [world, nq] (all shards, rank-major) -> (bins int32 [nq, bins_cap + 1], status)."""
    nq, ng = dist_shard.shape
    dev = dist_shard.device
    world, _, cap = keys_all.shape
    bins = torch.zeros(nq, bins_cap + 1, device=dev, dtype=torch.int32)
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    if ng > 0:
        _lib.check(_lib.lib().dali_rank_shard_bins(_lib.ctx(dev), _lib.stream_ptr(), _lib.ptr(dist_shard, torch.float32, "dist_shard"),
                                                    _lib.ptr(qp, torch.int32), _lib.ptr(gp, torch.int32), _lib.ptr(qc, torch.int32),
                                                    _lib.ptr(gc, torch.int32), nq, ng, int(g_offset), _lib.ptr(keys_all.contiguous(), torch.int64),
                                                    _lib.ptr(counts_all.contiguous(), torch.int32), world, cap, _lib.ptr(bins), bins_cap,
                                                    _lib.ptr(status)), "dali_rank_shard_bins")
    return bins, status


def rank_shard_finish(bins, counts_all, max_rank):
    """Step 5: the SUMMED bins -> dict of device tensors (cmc, mAP, map64, nvalid, ap, first_rank)."""
    dev = bins.device
    nq, bins_cap = bins.shape[0], bins.shape[1] - 1
    o = dict(cmc=torch.empty(max_rank, device=dev, dtype=torch.float32), mAP=torch.empty(1, device=dev, dtype=torch.float32),
             map64=torch.empty(1, device=dev, dtype=torch.float64), nvalid=torch.empty(1, device=dev, dtype=torch.int32),
             ap=torch.empty(nq, device=dev, dtype=torch.float32), first_rank=torch.empty(nq, device=dev, dtype=torch.int32))
    _lib.check(_lib.lib().dali_rank_shard_finish(_lib.ctx(dev), _lib.stream_ptr(), _lib.ptr(bins.contiguous(), torch.int32),
                                                  _lib.ptr(counts_all.contiguous(), torch.int32), counts_all.shape[0], nq, bins_cap, max_rank,
                                                  _lib.ptr(o["cmc"]), _lib.ptr(o["mAP"]), _lib.ptr(o["map64"]), _lib.ptr(o["nvalid"]),
                                                  _lib.ptr(o["ap"]), _lib.ptr(o["first_rank"])), "dali_rank_shard_finish")
    return o


def rank_eval_sharded(dist_shard, q_pids, g_pids_shard, q_camids, g_camids_shard, g_offset, group=None, max_rank=50, ng_total=None,
                      return_per_query=False):
    """market1501 CMC / mAP with the GALLERY sharded over the ranks of ``group`` (validateModels.py:41-47,61-69): this rank
    holds ``dist_shard`` [nq, ng_local] = all queries against its gallery slice, whose first entry has global index ``g_offset``.  Every
    rank passes all query ids and ITS slice of the gallery ids.  Two collectives: an all-gather of the per-query match keys (8 bytes per
    match) and an all-reduce (SUM) of integer bins; the result is bit-identical to ``rank_eval`` on the whole matrix and the same on
    every rank.  -> (cmc numpy float32 [max_rank], mAP float)"""
    import torch.distributed as dist
    dev = dist_shard.device
    nq, ng = dist_shard.shape
    world = dist.get_world_size(group) if (dist.is_available() and dist.is_initialized()) else 1
    qp, gp = factorize_ids(q_pids, g_pids_shard)                 # codes only need to agree between q and g on THIS rank
    qc, gc = factorize_ids(q_camids, g_camids_shard)
    t = lambda a: torch.from_numpy(a).to(dev)
    codes = (t(qp), t(gp), t(qc), t(gc))
    # cap: the largest identity of any shard (an upper bound of a query's matches inside one shard), agreed over the ranks
    caps = torch.tensor([int(np.bincount(gp).max()) if ng > 0 else 1, ng], dtype=torch.int64, device=dev)
    if world > 1:
        gathered = [torch.empty_like(caps) for _ in range(world)]
        dist.all_gather(gathered, caps, group=group)
        cap, ng_all = int(max(int(c[0]) for c in gathered)), int(sum(int(c[1]) for c in gathered))
    else:
        cap, ng_all = int(caps[0]), ng
    if ng_total is not None and ng_all != ng_total:
        raise _lib.DaliError("rank_eval_sharded: the gallery shards hold %d entries, expected %d" % (ng_all, ng_total))
    cap = max(1, min(cap, RANK_PMAX))
    bins_cap = min(world * cap, RANK_PMAX)
    keys, counts, st1 = rank_shard_matches(dist_shard, *codes, g_offset, cap)
    if world > 1:
        keys_l = [torch.empty_like(keys) for _ in range(world)]
        counts_l = [torch.empty_like(counts) for _ in range(world)]
        dist.all_gather(keys_l, keys, group=group)
        dist.all_gather(counts_l, counts, group=group)
        keys_all, counts_all = torch.stack(keys_l), torch.stack(counts_l)
    else:
        keys_all, counts_all = keys.unsqueeze(0), counts.unsqueeze(0)
    bins, st2 = rank_shard_bins(dist_shard, *codes, g_offset, keys_all, counts_all, bins_cap)
    status = torch.maximum(st1, st2)
    if world > 1:
        dist.all_reduce(bins, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(status, op=dist.ReduceOp.MAX, group=group)
    o = rank_shard_finish(bins, counts_all, min(max_rank, ng_all))
    stv = int(status.item())
    if stv != 0:
        raise _lib.DaliError("rank_eval_sharded: " + ("a query has more than %d matches (documented limit)" % RANK_PMAX if stv == 1 else
                                                      "identity codes span more than 2^20 values (documented limit)"))
    if int(o["nvalid"].item()) == 0:
        raise AssertionError("Error: all query identities do not appear in gallery")
    res = (o["cmc"].cpu().numpy(), float(o["map64"].item()))
    if return_per_query:
        return res + (o["ap"].cpu().numpy(), o["first_rank"].cpu().numpy())
    return res


def class_targets(fvs, order, bounds, first_pick, num_proxies=5):
    """Class centers + farthest-point proxies in one launch (train_encodersKIT.py:113-156, :252-284).
    fvs [N,D] fp32 CUDA; order [N] int32 (rows sorted by identity), bounds [NC+1] int32, first_pick [NC] int32 (position
    of the first proxy inside each identity's slice), all CUDA.
    -> centers [NC,D], proxies [NC*num_proxies,D] (zero rows where an identity has fewer images), proxy_rows
    [NC*num_proxies] int32 (row of fvs or -1), max_dist [NC]."""
    assert fvs.dim() == 2 and fvs.is_contiguous()
    n, d = fvs.shape
    nc = bounds.numel() - 1
    assert order.numel() == n and first_pick.numel() == nc
    dev = fvs.device
    centers = torch.empty(nc, d, device=dev, dtype=torch.float32)
    proxies = torch.empty(nc * num_proxies, d, device=dev, dtype=torch.float32)
    proxy_rows = torch.empty(nc * num_proxies, device=dev, dtype=torch.int32)
    max_dist = torch.empty(nc, device=dev, dtype=torch.float32)
    _lib.check(_lib.lib().dali_class_targets(_lib.ctx(dev), _lib.stream_ptr(), _lib.ptr(fvs, torch.float32, "fvs"), n, d,
                                              _lib.ptr(order, torch.int32, "order"), _lib.ptr(bounds, torch.int32, "bounds"), nc,
                                              _lib.ptr(first_pick, torch.int32, "first_pick"), int(num_proxies), _lib.ptr(centers),
                                              _lib.ptr(proxies), _lib.ptr(proxy_rows), _lib.ptr(max_dist)), "dali_class_targets")
    return centers, proxies, proxy_rows, max_dist


def pairdist_blend(distmat, q, g, mags_prev=None, mags=None, precision="bf16x3", normalize=True):
    """In place: distmat <- (w1*distmat + w2*(1 - q@g.T)) / (w1 + w2), w_m = max(qmag_m[:,None], gmag_m[None,:])
    (evaluateCleanATModels.py:154-157), computed in the distance kernel's epilogue.  mags_prev = (q_mag, g_mag) of the
    model that produced ``distmat``, mags = those of this model; both None -> plain average (:126)."""
    assert q.dim() == 2 and g.dim() == 2 and q.shape[1] == g.shape[1] and tuple(distmat.shape) == (q.shape[0], g.shape[0])
    assert (mags_prev is None) == (mags is None)
    nq, ng, d = q.shape[0], g.shape[0], q.shape[1]
    if nq == 0 or ng == 0:
        return distmat
    f32 = torch.float32
    m = [None] * 4 if mags is None else [t.reshape(-1).contiguous().float() for t in (*mags_prev, *mags)]
    if mags is not None:
        assert m[0].numel() == nq and m[1].numel() == ng and m[2].numel() == nq and m[3].numel() == ng
    _lib.check(_lib.lib().dali_pairdist_blend(_lib.ctx(q.device), _lib.stream_ptr(), _lib.ptr(q, f32, "q"), _lib.ptr(g, f32, "g"), nq, ng, d,
                                               _PREC[precision], int(bool(normalize)), _lib.ptr(m[0]), _lib.ptr(m[1]), _lib.ptr(m[2]),
                                               _lib.ptr(m[3]), _lib.ptr(distmat, f32, "distmat")), "dali_pairdist_blend")
    return distmat


RERANK_K1_MAX = 63        # k1 + 1 <= 64: one neighbour per lane of the selection wave (csrc/rerank.hip)


def re_ranking(q_g_dist, q_q_dist, g_g_dist, k1=20, k2=6, lambda_value=0.3):
    """k-reciprocal re-ranking with torchreid.utils.re_ranking's signature (validateModels.py:49-53; definition: include/daliid.h,
    dali_rerank).  CUDA tensors in -> CUDA fp32 [nq, ng] out, enqueued on the current stream.  numpy arrays or CPU tensors are copied
    to the current device and the result comes back as numpy, as torchreid returns it."""
    on_host = not all(isinstance(t, torch.Tensor) and t.is_cuda for t in (q_g_dist, q_q_dist, g_g_dist))
    dev = torch.device("cuda", torch.cuda.current_device()) if on_host else q_g_dist.device

    def prep(t):
        t = torch.as_tensor(np.asarray(t)) if not isinstance(t, torch.Tensor) else t
        return t.to(dev, dtype=torch.float32).contiguous()

    q_g, q_q, g_g = prep(q_g_dist), prep(q_q_dist), prep(g_g_dist)
    if q_g.dim() != 2 or q_q.dim() != 2 or g_g.dim() != 2:
        raise ValueError("re_ranking: the three distance blocks must be 2-D")
    nq, ng = q_g.shape
    if tuple(q_q.shape) != (nq, nq) or tuple(g_g.shape) != (ng, ng):
        raise ValueError("re_ranking: shapes q_g %s, q_q %s, g_g %s do not fit together" % (tuple(q_g.shape), tuple(q_q.shape), tuple(g_g.shape)))
    out = torch.empty(nq, ng, device=dev, dtype=torch.float32)
    _lib.check(_lib.lib().dali_rerank(_lib.ctx(dev), _lib.stream_ptr(), _lib.ptr(q_g, torch.float32, "q_g"), _lib.ptr(q_q, torch.float32, "q_q"),
                                       _lib.ptr(g_g, torch.float32, "g_g"), nq, ng, int(k1), int(k2), float(lambda_value), _lib.ptr(out)),
               "dali_rerank")
    return out.cpu().numpy() if on_host else out


ROC_MAX_PAIRS = 2 ** 31 - 1   # nq * ng the counting kernels index with 32 bits (include/daliid.h, dali_roc_build)


class UndefinedMetricWarning(UserWarning):
    """Raised as sklearn.metrics does when a class is absent (its rate is then NaN)."""


def _roc_inputs(distmat, q_pids, g_pids):
    """-> (device fp32 [nq, ng] 16-byte aligned, q codes, g codes, on_host).  Host input is copied to the current device."""
    if isinstance(distmat, torch.Tensor) and distmat.is_cuda:
        dev, on_host = distmat.device, False
    else:
        dev, on_host = torch.device("cuda", torch.cuda.current_device()), True
    shape = tuple(distmat.shape) if hasattr(distmat, "shape") else np.shape(distmat)
    if len(shape) != 2:
        raise ValueError("roc_curve: distmat must be 2-D, got shape %s" % (shape,))
    nq, ng = shape
    if nq * ng > ROC_MAX_PAIRS:
        raise _lib.DaliError("roc_curve: %d x %d = %d pairs exceeds the supported 2^31 - 1 (documented limit)" % (nq, ng, nq * ng))
    if nq == 0 or ng == 0:
        raise ValueError("roc_curve: empty distance matrix")
    qp, gp = factorize_ids(q_pids, g_pids)
    if qp.size != nq or gp.size != ng:
        raise ValueError("roc_curve: %d query ids and %d gallery ids for a %d x %d matrix" % (qp.size, gp.size, nq, ng))
    d = distmat if isinstance(distmat, torch.Tensor) else torch.as_tensor(np.asarray(distmat))
    d = d.to(dev, dtype=torch.float32).contiguous()
    if d.data_ptr() % 16:
        d = d.clone()
    t = lambda a: torch.from_numpy(a).to(dev)
    return d, t(qp), t(gp), on_host


def _roc_build(d, qp, gp):
    """dali_roc_build: -> (scratch, counts [n_drop, n_all, n_pos, n_neg] as ints).  Reads the five result words once."""
    nq, ng = d.shape
    L = _lib.lib()
    nbytes = int(L.dali_roc_scratch_bytes(nq, ng))
    scratch = torch.empty(nbytes, device=d.device, dtype=torch.uint8)
    out = torch.empty(5, device=d.device, dtype=torch.int64)
    _lib.check(L.dali_roc_build(_lib.ctx(d.device), _lib.stream_ptr(), _lib.ptr(d, torch.float32, "distmat"), _lib.ptr(qp, torch.int32),
                                _lib.ptr(gp, torch.int32), nq, ng, _lib.ptr(scratch), nbytes, _lib.ptr(out)), "dali_roc_build")
    n_drop, n_all, n_pos, n_neg, status = (int(v) for v in out.cpu().tolist())
    if status == 1:
        raise ValueError("Input contains NaN or infinity: a distance gives a non-finite score 1 - d/2")
    if status != 0:
        raise _lib.DaliError("dali_roc_build: internal count mismatch (status %d)" % status)
    return scratch, (n_drop, n_all, n_pos, n_neg)


def _roc_emit(scratch, d, n_points, drop_intermediate):
    """dali_roc_emit into device arrays with the leading (+inf, 0, 0) point."""
    nq, ng = d.shape
    dev = d.device
    thr = torch.empty(n_points + 1, device=dev, dtype=torch.float32)
    fps = torch.empty(n_points + 1, device=dev, dtype=torch.int64)
    tps = torch.empty(n_points + 1, device=dev, dtype=torch.int64)
    thr[0], fps[0], tps[0] = float("inf"), 0, 0
    _lib.check(_lib.lib().dali_roc_emit(_lib.ctx(dev), _lib.stream_ptr(), _lib.ptr(scratch), nq, ng, int(bool(drop_intermediate)), n_points,
                                        _lib.ptr(thr[1:]), _lib.ptr(fps[1:]), _lib.ptr(tps[1:])), "dali_roc_emit")
    return thr, fps, tps


def roc_counts(distmat, q_pids, g_pids, drop_intermediate=True):
    """Device side of ``roc_curve``: -> (thresholds fp32, fps int64, tps int64) CUDA tensors with the leading (+inf, 0, 0) point, for
    curves too long to bring to the host.  The partition scratch (12 bytes per pair) is freed before this returns."""
    d, qp, gp, _ = _roc_inputs(distmat, q_pids, g_pids)
    scratch, (n_drop, n_all, _, _) = _roc_build(d, qp, gp)
    out = _roc_emit(scratch, d, n_drop if drop_intermediate else n_all, drop_intermediate)
    del scratch
    return out


def _rates(fps, tps):
    """fpr, tpr as sklearn 1.7.2 forms them (float64 division by the last count; NaN and a warning for an absent class)."""
    import warnings
    fps, tps = fps.astype(np.float64), tps.astype(np.float64)
    if fps[-1] <= 0:
        warnings.warn("No negative samples in y_true, false positive value should be meaningless", UndefinedMetricWarning)
        fpr = np.repeat(np.nan, fps.shape)
    else:
        fpr = fps / fps[-1]
    if tps[-1] <= 0:
        warnings.warn("No positive samples in y_true, true positive value should be meaningless", UndefinedMetricWarning)
        tpr = np.repeat(np.nan, tps.shape)
    else:
        tpr = tps / tps[-1]
    return fpr, tpr


def roc_curve(distmat, q_pids, g_pids, drop_intermediate=True):
    """ROC over every query-gallery pair, bitwise what sklearn.metrics.roc_curve(labels, 1 - distmat.ravel() / 2, pos_label=1,
    drop_intermediate=...) returns with labels = (q_pids[i] == g_pids[j]) (evaluateCleanATModels.py:276-292; definition:
    include/daliid.h, dali_roc_build).  distmat: CUDA tensor, or a host array / CPU tensor copied to the current device; converted to
    fp32.  -> numpy (fpr float64, tpr float64, thresholds float32)."""
    thr, fps, tps = roc_counts(distmat, q_pids, g_pids, drop_intermediate)
    fpr, tpr = _rates(fps.cpu().numpy(), tps.cpu().numpy())
    return fpr, tpr, thr.cpu().numpy()


def verification_summary(fpr, tpr, thresholds, fpr_all, tpr_all, thresholds_all, fars):
    """AUC, EER and TAR@FAR from the dropped curve (fpr, tpr, thresholds) and the undropped one (*_all):
    auc = np.trapezoid(tpr, fpr); TAR@FAR=f = the largest tpr of an undropped point with fpr <= f, with the threshold of the first such
    point that reaches it; EER on the first dropped segment (f0, t0)-(f1, t1) where fpr + tpr reaches 1: f0 + lam (f1 - f0),
    lam = (1 - t0 - f0) / ((f1 - f0) + (t1 - t0)), threshold of the segment's end point."""
    auc = float(np.trapezoid(tpr, fpr))
    eer, eer_thr = float("nan"), float("nan")
    reach = np.nonzero(fpr + tpr >= 1.0)[0]
    if reach.size:
        k = int(reach[0])
        if k == 0:
            eer, eer_thr = float(fpr[0]), float(thresholds[0])
        else:
            f0, t0, f1, t1 = fpr[k - 1], tpr[k - 1], fpr[k], tpr[k]
            lam = (1.0 - t0 - f0) / ((f1 - f0) + (t1 - t0))
            eer, eer_thr = float(f0 + lam * (f1 - f0)), float(thresholds[k])
    tar = {}
    for f in fars:
        ok = np.nonzero(fpr_all <= f)[0]
        if ok.size == 0:
            tar[f] = (float("nan"), float("nan"))
            continue
        best = tpr_all[ok].max()
        first = int(ok[np.nonzero(tpr_all[ok] == best)[0][0]])
        tar[f] = (float(best), float(thresholds_all[first]))
    return auc, eer, eer_thr, tar


def verification_metrics(distmat, q_pids, g_pids, fars=(1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6)):
    """Verification summary of the pair ROC (roc_curve): one count on the device, both curves emitted from it.
    -> dict n_pos, n_neg, auc, eer, eer_threshold, tar_at_far {far: (tar, threshold)} (definitions: verification_summary)."""
    d, qp, gp, _ = _roc_inputs(distmat, q_pids, g_pids)
    scratch, (n_drop, n_all, n_pos, n_neg) = _roc_build(d, qp, gp)
    curves = []
    for drop, n in ((True, n_drop), (False, n_all)):
        thr, fps, tps = _roc_emit(scratch, d, n, drop)
        curves.append(_rates(fps.cpu().numpy(), tps.cpu().numpy()) + (thr.cpu().numpy(),))
        del thr, fps, tps
    del scratch
    auc, eer, eer_thr, tar = verification_summary(*curves[0], *curves[1], fars)
    return dict(n_pos=n_pos, n_neg=n_neg, auc=auc, eer=eer, eer_threshold=eer_thr, tar_at_far=tar)


# ---- Weibull meta-recognition score fusion (include/daliid.h, dali_mr_*; the reference's libmr / Meta_Recognition, evaluate.py:394-627) ----
MR_N_MAX = 16384          # longest row the fit kernel keeps in LDS (include/daliid.h, dali_mr_fit_rows)


def _mr_matrix(t, name):
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise ValueError("%s must be a 2-D tensor" % name)
    if not t.is_cuda or t.dtype != torch.float32:
        raise _lib.DaliError("%s must be a CUDA float32 tensor" % name)
    if not t.is_contiguous():
        raise _lib.DaliError("%s must be contiguous" % name)
    return t


def _mr_kill_transpose(scores, topk, use_columns, killscale):
    """-> (KT fp32 [ng, nq], status int32 [2] on the device); nothing synchronises."""
    s = _mr_matrix(scores, "scores")
    nq, ng = s.shape
    kt = torch.empty(ng, nq, device=s.device, dtype=torch.float32)
    status = torch.zeros(2, device=s.device, dtype=torch.int32)
    _lib.check(_lib.lib().dali_mr_kill_transpose(_lib.ctx(s.device), _lib.stream_ptr(), _lib.ptr(s), nq, ng, int(topk), int(bool(use_columns)),
                                                  float(killscale), _lib.ptr(kt), _lib.ptr(status)), "dali_mr_kill_transpose")
    return kt, status


def _mr_fit_rows(x, tail, iters=False):
    """-> (fits fp64 [nrows, 2], small fp32 [nrows], status int32 [2] = {non-finite input, unfit rows}[, iters int32 [nrows]]) on the
    device; nothing synchronises."""
    x = _mr_matrix(x, "x")
    nrows, n = x.shape
    dev = x.device
    fits = torch.empty(nrows, 2, device=dev, dtype=torch.float64)
    small = torch.empty(nrows, device=dev, dtype=torch.float32)
    status = torch.zeros(2, device=dev, dtype=torch.int32)
    it = torch.zeros(nrows, device=dev, dtype=torch.int32) if iters else None
    _lib.check(_lib.lib().dali_mr_fit_rows(_lib.ctx(dev), _lib.stream_ptr(), _lib.ptr(x), nrows, n, int(tail), _lib.ptr(fits), _lib.ptr(small),
                                           _lib.ptr(it), _lib.ptr(status)), "dali_mr_fit_rows")
    return (fits, small, status, it) if iters else (fits, small, status)


def _mr_check_finite(status, who):
    if int(status[0]) != 0:
        raise ValueError("%s: input contains NaN or infinity" % who)


def mr_kill_transpose(scores, topk, use_columns=False, killscale=1.0):
    """Meta_Recognition.metarec's kill (evaluate.py:597-618; include/daliid.h, dali_mr_kill_transpose): the ``topk`` largest entries of
    every row (``use_columns``: of every column) of the CUDA fp32 similarity matrix [nq, ng] become ``s - killscale * s``, in the order
    of ``topk_rows(largest=True)``; the result is returned TRANSPOSED, fp32 [ng, nq].  ``scores`` is left unchanged."""
    kt, status = _mr_kill_transpose(scores, topk, use_columns, killscale)
    _mr_check_finite(status, "mr_kill_transpose")
    return kt


def mr_fit_rows(x, tail, return_iters=False):
    """libmr.FitHigh (evaluate.py:444-447 -> :487-505 -> :541-590; include/daliid.h, dali_mr_fit_rows): a Weibull fitted by maximum
    likelihood to the ``tail`` largest values of every row of the CUDA fp32 matrix x [nrows, n].  -> (fits fp64 [nrows, 2] = (shape, scale),
    small fp32 [nrows] = the tail-th largest value, n_unfit[, iters int32 [nrows]]).  Unfit rows hold (NaN, NaN)."""
    out = _mr_fit_rows(x, tail, iters=return_iters)
    _mr_check_finite(out[2], "mr_fit_rows")
    return (out[0], out[1], int(out[2][1])) + ((out[3],) if return_iters else ())


def mr_wscore(scores, fits, small):
    """libmr.wscore (evaluate.py:449-485; include/daliid.h, dali_mr_wscore): fp64 [nq, ng] Weibull CDF of every score under its
    column's fit; exactly 0 at or below the column's ``small - 1`` and for an unfit column."""
    s = _mr_matrix(scores, "scores")
    nq, ng = s.shape
    if tuple(fits.shape) != (ng, 2) or small.numel() != ng:
        raise ValueError("mr_wscore: fits %s / small %s do not fit %d columns" % (tuple(fits.shape), tuple(small.shape), ng))
    out = torch.empty(nq, ng, device=s.device, dtype=torch.float64)
    _lib.check(_lib.lib().dali_mr_wscore(_lib.ctx(s.device), _lib.stream_ptr(), _lib.ptr(s), nq, ng, _lib.ptr(fits, torch.float64, "fits"),
                                         _lib.ptr(small.reshape(-1), torch.float32, "small"), _lib.ptr(out)), "dali_mr_wscore")
    return out


def mr_fuse_fitted(score_list, fits_list, small_list, out_dtype=torch.float32):
    """dali_mr_fuse on fitted columns: sum_a w_a s_a / sum_a w_a over 1 .. 3 models, the w-scores never stored; the plain mean where
    every w is 0.  fp64, or rounded once to fp32."""
    m = len(score_list)
    if not 1 <= m <= 3 or len(fits_list) != m or len(small_list) != m:
        raise ValueError("mr_fuse: 1 .. 3 models with one fit table each, got %d" % m)
    if out_dtype not in (torch.float32, torch.float64):
        raise ValueError("mr_fuse: out_dtype must be torch.float32 or torch.float64")
    ss = [_mr_matrix(s, "scores[%d]" % a) for a, s in enumerate(score_list)]
    nq, ng = ss[0].shape
    dev = ss[0].device
    smalls = [sm.reshape(-1) for sm in small_list]
    for s, f, sm in zip(ss, fits_list, smalls):
        if tuple(s.shape) != (nq, ng) or s.device != dev or tuple(f.shape) != (ng, 2) or sm.numel() != ng:
            raise ValueError("mr_fuse: the score matrices and fit tables do not have one shape")
    arr = lambda ts, dt, name: (_lib.c_void_p * m)(*[_lib.ptr(t, dt, name).value for t in ts])
    out = torch.empty(nq, ng, device=dev, dtype=out_dtype)
    _lib.check(_lib.lib().dali_mr_fuse(_lib.ctx(dev), _lib.stream_ptr(), arr(ss, torch.float32, "scores"), arr(fits_list, torch.float64, "fits"),
                                       arr(smalls, torch.float32, "small"), m, nq, ng, int(out_dtype == torch.float64), _lib.ptr(out)),
               "dali_mr_fuse")
    return out


def mr_fuse(score_list, topk=20, use_columns=False, killscale=1.0, out_dtype=torch.float32):
    """Meta_Recognition.mrfuse (evaluate.py:620-637) generalised to 1 .. 3 CUDA fp32 similarity matrices [nq, ng]: per model kill ->
    fit every gallery column with tail nq - topk - 1 -> w-score weighted blend (include/daliid.h, dali_mr_*).  One read of the status
    words at the end; a non-finite score raises ValueError."""
    if not 1 <= len(score_list) <= 3:
        raise ValueError("mr_fuse: 1 .. 3 models, got %d" % len(score_list))
    fits, smalls, stats = [], [], []
    for s in score_list:
        kt, st0 = _mr_kill_transpose(s, topk, use_columns, killscale)
        f, sm, st1 = _mr_fit_rows(kt, kt.shape[1] - int(topk) - 1)
        del kt
        fits.append(f); smalls.append(sm); stats += [st0, st1]
    out = mr_fuse_fitted(score_list, fits, smalls, out_dtype)
    if stats and int(torch.stack(stats)[:, 0].max()) != 0:
        raise ValueError("mr_fuse: input contains NaN or infinity")
    return out


# ---- template (set) evaluation (include/daliid.h, dali_pool_rows / dali_segment_reduce2d / dali_open_set_search) ----
_POOL_MODE = {"mean": 0, "max": 1}
_SEG_MODE = {"min": 0, "max": 1, "mean": 2}
_TPL_STATUS = {1: "a row number lies outside the rows", 2: "the bounds do not increase inside their range", 3: "row numbers and bounds lie outside their ranges"}


def template_index(keys):
    """Host: group rows into templates by key.  ``keys``: a 1-D array of any dtype (strings included) or a tuple of such columns (rows
    are equal when every column is).  Templates are numbered in the order of their first appearance, members keep their original row
    order.  -> (order int32 [n]: row numbers grouped by template, bounds int32 [T + 1], first int64 [T]: the first member of every
    template) -- the ``order`` / ``bounds`` convention of ``class_targets``."""
    cols = list(keys) if isinstance(keys, tuple) else [keys]
    if not cols:
        raise ValueError("template_index: no key column")
    code = None
    for col in cols:
        col = np.asarray(col)
        if col.ndim != 1:
            raise ValueError("template_index: a key column must be 1-D, got shape %s" % (col.shape,))
        if code is not None and col.shape[0] != code.shape[0]:
            raise ValueError("template_index: key columns of %d and %d rows" % (code.shape[0], col.shape[0]))
        _, inv = np.unique(col, return_inverse=True)
        inv = inv.reshape(-1).astype(np.int64)
        if code is None:
            code = inv
        else:                      # the pair (code so far, this column) renumbered densely: no product of cardinalities can overflow
            _, code = np.unique(np.stack([code, inv], axis=1), axis=0, return_inverse=True)
            code = code.reshape(-1).astype(np.int64)
    n = code.shape[0]
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(1, np.int32), np.zeros(0, np.int64)
    _, first_of, inv = np.unique(code, return_index=True, return_inverse=True)
    by_first = np.argsort(first_of, kind="stable")
    number = np.empty_like(by_first)
    number[by_first] = np.arange(by_first.size)
    t = number[inv.reshape(-1)]
    order = np.argsort(t, kind="stable").astype(np.int32)
    bounds = np.concatenate([[0], np.cumsum(np.bincount(t))]).astype(np.int32)
    return order, bounds, first_of[by_first].astype(np.int64)


def _check_bounds(bounds, n, who, what):
    """Host check of a bounds array: strictly increasing from 0 to n.  -> numpy int32."""
    b = np.asarray(bounds)
    if b.ndim != 1 or b.size < 2 or not np.issubdtype(b.dtype, np.integer):
        raise ValueError("%s: %s must be a 1-D integer array of at least 2 entries" % (who, what))
    b = b.astype(np.int64)
    if b[0] != 0 or b[-1] != n:
        raise ValueError("%s: %s run from %d to %d, not from 0 to %d" % (who, what, b[0], b[-1], n))
    if np.any(np.diff(b) <= 0):
        raise ValueError("%s: %s must increase strictly (template %d is empty)" % (who, what, int(np.nonzero(np.diff(b) <= 0)[0][0])))
    return b.astype(np.int32)


def _device_bounds(bounds, n, dev, who, what):
    """A host array is checked here and uploaded; a CUDA int32 tensor is taken as it is (the kernels compare every bound with its range
    and report through the status word)."""
    if isinstance(bounds, torch.Tensor) and bounds.is_cuda:
        if bounds.dtype != torch.int32 or bounds.dim() != 1 or bounds.numel() < 2 or not bounds.is_contiguous():
            raise ValueError("%s: %s on the device must be a contiguous 1-D int32 tensor of at least 2 entries" % (who, what))
        return bounds
    if isinstance(bounds, torch.Tensor):
        bounds = bounds.numpy()
    return torch.from_numpy(_check_bounds(bounds, n, who, what)).to(dev)


def _tpl_status(status, who):
    st = int(status.item())
    if st != 0:
        raise _lib.DaliError("%s: %s (skipped, never read)" % (who, _TPL_STATUS.get(st, "status %d" % st)))


def pool_templates(fvs, order, bounds, mode="mean", weights=None):
    """Feature-level pooling of CUDA fp32 rows ``fvs`` [n, d] into one row per template (include/daliid.h, dali_pool_rows), in the fixed
    fp32 order documented there.  ``order`` / ``bounds``: as ``template_index`` returns them (host arrays are checked here; CUDA int32
    tensors are taken as they are and checked by the kernel).  mode: "mean" (with ``weights`` fp32 [n] indexed by row: the weighted mean
    sum w f / sum w), "max", "magnitude" (weights = the rows' L2 norms, ``l2norm_rows(..., return_norms=True)``: the reference's
    confidence-by-magnitude inside a template) or "unit_mean" (weights = the reciprocal norms: the mean of the unit vectors; a zero row
    gives NaN).  -> fp32 [T, d] on the device."""
    who = "pool_templates"
    if mode not in ("mean", "max", "magnitude", "unit_mean"):
        raise ValueError("%s: mode must be 'mean', 'max', 'magnitude' or 'unit_mean', got %r" % (who, mode))
    if weights is not None and mode != "mean":
        raise ValueError("%s: weights go with mode='mean' only (mode=%r brings its own or takes none)" % (who, mode))
    if not isinstance(fvs, torch.Tensor) or fvs.dim() != 2:
        raise ValueError("%s: fvs must be a 2-D tensor" % who)
    if not fvs.is_cuda or fvs.dtype != torch.float32:
        raise _lib.DaliError("%s: fvs must be a CUDA float32 tensor" % who)
    n, d = fvs.shape
    if n == 0 or d == 0:
        raise ValueError("%s: nothing to pool (fvs is %d x %d)" % (who, n, d))
    dev = fvs.device
    fvs = fvs.contiguous()
    if isinstance(order, torch.Tensor) and order.is_cuda:
        if order.dtype != torch.int32 or order.dim() != 1 or not order.is_contiguous():
            raise ValueError("%s: order on the device must be a contiguous 1-D int32 tensor" % who)
        order_d = order
    else:
        o = np.asarray(order.numpy() if isinstance(order, torch.Tensor) else order)
        if o.ndim != 1 or not np.issubdtype(o.dtype, np.integer) or o.size != n:
            raise ValueError("%s: order must hold one integer row number per row (%d)" % (who, n))
        if o.min() < 0 or o.max() >= n:
            raise ValueError("%s: order holds a row number outside 0..%d" % (who, n - 1))
        order_d = torch.from_numpy(o.astype(np.int32)).to(dev)
    if order_d.numel() != n:
        raise ValueError("%s: order has %d entries for %d rows" % (who, order_d.numel(), n))
    bounds_d = _device_bounds(bounds, n, dev, who, "bounds")
    T = bounds_d.numel() - 1
    if mode in ("magnitude", "unit_mean"):
        _, norms = l2norm_rows(fvs, return_norms=True)
        weights = norms if mode == "magnitude" else torch.reciprocal(norms)
    elif weights is not None:
        if not isinstance(weights, torch.Tensor) or weights.numel() != n:
            raise ValueError("%s: weights must be a tensor of one weight per row (%d)" % (who, n))
        weights = weights.reshape(-1).contiguous()
    out = torch.empty(T, d, device=dev, dtype=torch.float32)
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    _lib.check(_lib.lib().dali_pool_rows(_lib.ctx(dev), _lib.stream_ptr(), _lib.ptr(fvs), n, d, _lib.ptr(order_d), _lib.ptr(bounds_d), T,
                                         _lib.ptr(weights, torch.float32, "weights"), _POOL_MODE["max" if mode == "max" else "mean"],
                                         _lib.ptr(out), _lib.ptr(status)), "dali_pool_rows")
    _tpl_status(status, who)
    return out


def segment_reduce2d(distmat, row_bounds, col_bounds, mode, out=None, out_row0=0, out_col0=0, _status=None):
    """Score-level linkage (include/daliid.h, dali_segment_reduce2d): entry (a, b) of the result is the "min" / "max" / "mean" of the
    sub-matrix rows(a) x cols(b) of the CUDA fp32 ``distmat``, whose rows and columns are cut into contiguous segments by ``row_bounds``
    [Tr + 1] / ``col_bounds`` [Tc + 1] (host arrays are checked here; CUDA int32 tensors are taken as they are).  ``distmat`` may be a
    column slice of a wider matrix (read by its pitch).  ``out``: a CUDA fp32 matrix that receives the [Tr, Tc] block at
    (out_row0, out_col0); its other entries are left as they are.  -> out (a new [Tr, Tc] tensor without ``out``).  ``_status``: a device
    status word the caller reads itself (link_templates: once for all its blocks)."""
    who = "segment_reduce2d"
    if mode not in _SEG_MODE:
        raise ValueError("%s: mode must be 'min', 'max' or 'mean', got %r" % (who, mode))
    if not isinstance(distmat, torch.Tensor) or distmat.dim() != 2:
        raise ValueError("%s: distmat must be a 2-D tensor" % who)
    if not distmat.is_cuda or distmat.dtype != torch.float32:
        raise _lib.DaliError("%s: distmat must be a CUDA float32 tensor" % who)
    rows, cols = distmat.shape
    if rows == 0 or cols == 0:
        raise ValueError("%s: empty matrix (%d x %d)" % (who, rows, cols))
    if not (distmat.stride(1) == 1 and (rows == 1 or distmat.stride(0) >= cols)):
        distmat = distmat.contiguous()
    ld = max(int(distmat.stride(0)), cols) if rows > 1 else cols
    dev = distmat.device
    rb = _device_bounds(row_bounds, rows, dev, who, "row_bounds")
    cb = _device_bounds(col_bounds, cols, dev, who, "col_bounds")
    Tr, Tc = rb.numel() - 1, cb.numel() - 1
    if out is None:
        if out_row0 or out_col0:
            raise ValueError("%s: out_row0 / out_col0 without out" % who)
        out = torch.empty(Tr, Tc, device=dev, dtype=torch.float32)
    else:
        if not isinstance(out, torch.Tensor) or out.dim() != 2 or not out.is_cuda or out.dtype != torch.float32 or out.stride(1) != 1 \
                or (out.shape[0] > 1 and out.stride(0) < out.shape[1]):
            raise ValueError("%s: out must be a 2-D CUDA float32 matrix with contiguous rows" % who)
        if out_row0 < 0 or out_col0 < 0 or out_row0 + Tr > out.shape[0] or out_col0 + Tc > out.shape[1]:
            raise ValueError("%s: the %d x %d block at (%d, %d) does not lie inside out %s" % (who, Tr, Tc, out_row0, out_col0, tuple(out.shape)))
    out_ld = max(int(out.stride(0)), out.shape[1]) if out.shape[0] > 1 else out.shape[1]
    status = torch.zeros(1, device=dev, dtype=torch.int32) if _status is None else _status
    _lib.check(_lib.lib().dali_segment_reduce2d(_lib.ctx(dev), _lib.stream_ptr(), _lib.c_void_p(distmat.data_ptr()), rows, cols, ld, _lib.ptr(rb), Tr,
                                                _lib.ptr(cb), Tc, _SEG_MODE[mode], _lib.c_void_p(out.data_ptr()), out.shape[0], out_ld,
                                                int(out_row0), int(out_col0), _lib.ptr(status)), "dali_segment_reduce2d")
    if _status is None:
        _tpl_status(status, who)
    return out


def _template_groups(bounds, cap):
    """Greedy runs of whole templates of at most ``cap`` rows each (a longer template is a run of its own): -> list of (t0, t1)."""
    groups, t0 = [], 0
    T = bounds.size - 1
    while t0 < T:
        t1 = t0 + 1
        while t1 < T and bounds[t1 + 1] - bounds[t0] <= cap:
            t1 += 1
        groups.append((t0, t1))
        t0 = t1
    return groups


def _local_bounds(bounds, groups, dev):
    """The bounds of every run, each starting at 0, as views of ONE uploaded tensor."""
    parts = [bounds[t0:t1 + 1] - bounds[t0] for t0, t1 in groups]
    flat = torch.from_numpy(np.concatenate(parts).astype(np.int32)).to(dev)
    views, o = [], 0
    for p in parts:
        views.append(flat[o:o + p.size])
        o += p.size
    return views


def link_templates(q, g, q_bounds, g_bounds, linkage="min", metric="cosine", precision="bf16x3", normalize=True, scratch_bytes=1 << 30):
    """Set-to-set distances [Tq, Tg] between templates whose members are CONTIGUOUS rows of the CUDA fp32 features ``q`` / ``g``
    (``q_bounds`` [Tq + 1], ``g_bounds`` [Tg + 1], host arrays): the "min" / "mean" / "max" over the frame-pair distances of ``pairdist``
    (single / average / complete linkage).  The frame-level matrix never exists as a whole: ``pairdist`` writes a block of whole
    templates x whole templates into a reused scratch of at most ``scratch_bytes`` and ``segment_reduce2d`` writes its output sub-block.
    A template pair whose frame block alone exceeds the scratch is refused with the size it needs."""
    who = "link_templates"
    if linkage not in _SEG_MODE:
        raise ValueError("%s: linkage must be 'min', 'mean' or 'max', got %r" % (who, linkage))
    if metric not in _METRIC or precision not in _PREC:
        raise ValueError("%s: metric %r / precision %r are not built" % (who, metric, precision))
    if q.dim() != 2 or g.dim() != 2 or q.shape[1] != g.shape[1]:
        raise ValueError("%s: q %s and g %s must be 2-D with one width" % (who, tuple(q.shape), tuple(g.shape)))
    if not q.is_cuda or not g.is_cuda or q.dtype != torch.float32 or g.dtype != torch.float32:
        raise _lib.DaliError("%s: q and g must be CUDA float32 tensors" % who)
    as_host = lambda b: b.cpu().numpy() if isinstance(b, torch.Tensor) else b
    qb = _check_bounds(as_host(q_bounds), q.shape[0], who, "q_bounds").astype(np.int64)
    gb = _check_bounds(as_host(g_bounds), g.shape[0], who, "g_bounds").astype(np.int64)
    qmax, gmax = int(np.diff(qb).max()), int(np.diff(gb).max())
    elems = int(scratch_bytes) // 4
    if qmax * gmax > elems:
        raise ValueError("%s: a template pair of %d x %d frames needs a scratch of %d bytes, scratch_bytes is %d"
                         % (who, qmax, gmax, qmax * gmax * 4, int(scratch_bytes)))
    q, g = q.contiguous(), g.contiguous()
    dev = q.device
    nq, ng = q.shape[0], g.shape[0]
    if elems // ng >= qmax:        # the whole gallery width fits: the gallery is prepared once per row block
        rcap = elems // ng
    else:
        rcap = max(qmax, min(int(np.sqrt(elems)), elems // gmax))
    row_groups = _template_groups(qb, rcap)
    row_local = _local_bounds(qb, row_groups, dev)
    col_cache = {}
    scratch = torch.empty(min(elems, max(int(qb[t1] - qb[t0]) for t0, t1 in row_groups) * ng), device=dev, dtype=torch.float32)
    out = torch.empty(qb.size - 1, gb.size - 1, device=dev, dtype=torch.float32)
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    for (a0, a1), rb in zip(row_groups, row_local):
        r0, r1 = int(qb[a0]), int(qb[a1])
        ccap = min(ng, elems // (r1 - r0))
        if ccap not in col_cache:
            groups = _template_groups(gb, ccap)
            col_cache[ccap] = (groups, _local_bounds(gb, groups, dev))
        for (b0, b1), cb in zip(*col_cache[ccap]):
            c0, c1 = int(gb[b0]), int(gb[b1])
            block = scratch[:(r1 - r0) * (c1 - c0)].view(r1 - r0, c1 - c0)
            pairdist(q[r0:r1], g[c0:c1], metric=metric, precision=precision, normalize=normalize, out=block)
            segment_reduce2d(block, rb, cb, linkage, out=out, out_row0=a0, out_col0=b0, _status=status)
    _tpl_status(status, who)
    return out


def open_set_search(distmat, q_subj, g_subj):
    """Per-probe open-set search (include/daliid.h, dali_open_set_search) of a CUDA fp32 ``distmat`` [nq, ng] (read by its pitch) with
    int32 subject codes ``q_subj`` [nq] / ``g_subj`` [ng] (host arrays or tensors).  -> device tensors (mate_dist fp32, mate_col int32,
    nonmate_dist fp32, nonmate_col int32, rank int32), each [nq]: the nearest gallery entry of the probe's own subject (+inf / -1 for
    a probe that is not mated), the nearest entry of any other subject, and the number of other-subject entries that sort before the
    best mate (-1: not mated)."""
    who = "open_set_search"
    if not isinstance(distmat, torch.Tensor) or distmat.dim() != 2:
        raise ValueError("%s: distmat must be a 2-D tensor" % who)
    if not distmat.is_cuda or distmat.dtype != torch.float32:
        raise _lib.DaliError("%s: distmat must be a CUDA float32 tensor" % who)
    nq, ng = distmat.shape
    if nq == 0 or ng == 0:
        raise ValueError("%s: empty distance matrix (%d x %d)" % (who, nq, ng))
    if not (distmat.stride(1) == 1 and (nq == 1 or distmat.stride(0) >= ng)):
        distmat = distmat.contiguous()
    ld = max(int(distmat.stride(0)), ng) if nq > 1 else ng
    dev = distmat.device

    def codes(a, n, name):
        a = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a).reshape(-1)))
        if a.numel() != n or a.dtype not in (torch.int32, torch.int64):
            raise ValueError("%s: %s must hold %d integer subject codes" % (who, name, n))
        return a.to(dev, dtype=torch.int32).reshape(-1).contiguous()

    qs, gs = codes(q_subj, nq, "q_subj"), codes(g_subj, ng, "g_subj")
    mate_dist, nonmate_dist = (torch.empty(nq, device=dev, dtype=torch.float32) for _ in range(2))
    mate_col, nonmate_col, rank = (torch.empty(nq, device=dev, dtype=torch.int32) for _ in range(3))
    _lib.check(_lib.lib().dali_open_set_search(_lib.ctx(dev), _lib.stream_ptr(), _lib.c_void_p(distmat.data_ptr()), nq, ng, ld, _lib.ptr(qs),
                                               _lib.ptr(gs), _lib.ptr(mate_dist), _lib.ptr(mate_col), _lib.ptr(nonmate_dist),
                                               _lib.ptr(nonmate_col), _lib.ptr(rank)), "dali_open_set_search")
    return mate_dist, mate_col, nonmate_dist, nonmate_col, rank


def open_set_summary(mate_dist, nonmate_dist, rank, fpirs=(1e-1, 1e-2, 1e-3), ranks=(1, 20)):
    """Host: open-set identification rates from ``open_set_search``'s per-probe results (numpy float32 comparisons).  A probe is mated
    when rank >= 0.  With ``nm`` the ascending nonmate_dist of the NON-mated probes and N_nm their count, for every fpir:
    m = floor(fpir * N_nm + 1e-9), threshold T = nm[m] (+inf when m >= N_nm, in particular without non-mated probes: everything is then
    accepted), a candidate is accepted iff d < T; realised FPIR = the share of non-mated probes with nonmate_dist < T (at most fpir;
    NaN without non-mated probes); FNIR(fpir, r) = the share of mated probes that do NOT have mate_dist < T and rank < r (NaN without
    mated probes, as the closed-set rates are).  -> dict: fnir {(fpir, r)}, fpir {fpir: realised}, threshold {fpir: float32},
    rank {r: share of mated probes with rank < r}, n_mated, n_nonmated."""
    to_np = lambda a, dt: (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(dt).reshape(-1)
    md, nd, rk = to_np(mate_dist, np.float32), to_np(nonmate_dist, np.float32), to_np(rank, np.int64)
    if not md.size == nd.size == rk.size:
        raise ValueError("open_set_summary: mate_dist, nonmate_dist and rank differ in length (%d, %d, %d)" % (md.size, nd.size, rk.size))
    mated = rk >= 0
    n_m, n_nm = int(mated.sum()), int((~mated).sum())
    nm = np.sort(nd[~mated])
    md_m, rk_m = md[mated], rk[mated]
    nan = float("nan")
    res = dict(fnir={}, fpir={}, threshold={}, rank={int(r): (float(np.mean(rk_m < r)) if n_m else nan) for r in ranks},
               n_mated=n_m, n_nonmated=n_nm)
    for f in fpirs:
        m = int(np.floor(float(f) * n_nm + 1e-9))
        thr = nm[m] if m < n_nm else np.float32(np.inf)
        res["threshold"][f] = np.float32(thr)
        res["fpir"][f] = float(np.mean(nm < thr)) if n_nm else nan
        for r in ranks:
            res["fnir"][(f, int(r))] = float(1.0 - np.mean((md_m < thr) & (rk_m < r))) if n_m else nan
    return res


def open_set_metrics(distmat, q_ids, g_ids, fpirs=(1e-1, 1e-2, 1e-3), ranks=(1, 20)):
    """``factorize_ids`` + ``open_set_search`` + ``open_set_summary``: FNIR at fixed FPIR of a CUDA fp32 distance matrix whose rows /
    columns carry the subject ids ``q_ids`` / ``g_ids`` (any dtype).  One copy of 5 nq words to the host."""
    qs, gs = factorize_ids(q_ids, g_ids)
    mate_dist, _, nonmate_dist, _, rank = open_set_search(distmat, qs, gs)
    return open_set_summary(mate_dist, nonmate_dist, rank, fpirs, ranks)
