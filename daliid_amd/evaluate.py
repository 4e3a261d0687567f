"""Mirror of the meta-recognition classes of the reference's ``evaluate.py``: ``libmr`` (:394-580, the Weibull tail fit and its w-score)
and ``Meta_Recognition`` (:583-627, ``metarec`` / ``mrfuse``), the fusion that evaluate.py:241-279 carries behind the commented-out line
``distmat = 1.0 - meta_rec.mrfuse(1 - distmat_backbone, 1 - distmat_head01, 1 - distmat_head02)`` (:277).  Names and argument order are
the reference's.  Inputs may be CPU or device tensors (or numpy arrays); the work runs on the GPU (include/daliid.h, dali_mr_*) and
results go back to where the input lived.  There is no CPU fallback.

Differences from the reference, both stated in include/daliid.h: a column whose fit fails holds (NaN, NaN) and gets w-score 0 (the
reference leaves (0, 0) or NaN and a w-score that is an accident of pow), and ``mrfuse`` gives the plain mean of the scores where all
w-scores are 0 (the reference: 0/0 = NaN).  ``mrfuse`` does not print the w-score corners (:618-620): the fused kernel never stores
the w-scores.  The evaluation CLI and the multi-head ``extractFeatures`` of the same file are out of scope."""
import numpy as np
import torch

from . import ops_eval


def _to_device(t):
    """-> (CUDA fp32 contiguous tensor, device the caller's data lived on)"""
    t = t if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t))
    home = t.device
    dev = home if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
    return t.detach().to(dev, dtype=torch.float32).contiguous(), home


class libmr:
    def __init__(self, saved_model=None, translateAmount=1):
        if saved_model:
            raise NotImplementedError("libmr(saved_model=...): loading saved Weibull models is out of scope")
        if translateAmount != 1:
            raise NotImplementedError("libmr: translateAmount other than 1 is out of scope (the kernels add exactly 1)")
        self.translateAmount = translateAmount

    def tocpu(self):
        self.wbFits = self.wbFits.cpu()
        self.smallScoreTensor = self.smallScoreTensor.cpu()

    def return_all_parameters(self):
        return dict(Scale=self.wbFits[:, 1], Shape=self.wbFits[:, 0], signTensor=self.sign, translateAmountTensor=self.translateAmount,
                    smallScoreTensor=self.smallScoreTensor)

    def FitLow(self, data, tailSize, isSorted=False, gpu=0):
        raise NotImplementedError("libmr.FitLow is out of scope (only the high tail of similarity scores is fitted)")

    def FitHigh(self, data, tailSize, isSorted=False, gpu=0):
        """:434-437.  data [weibulls, scores]: one Weibull per row from its ``tailSize`` largest values.  -> (wbFits float64 [rows, 2] =
        (shape, scale), smallScoreTensor float32 [rows, 1]), also kept on the object.  ``gpu`` is unused, as in the reference."""
        if isSorted:
            raise NotImplementedError("libmr.FitHigh(isSorted=True) is out of scope (no caller in the reference passes sorted data)")
        self.sign = 1
        self.splits = 1
        x, home = _to_device(data)
        if x.dim() != 2:
            raise ValueError("FitHigh: data must be 2-D [weibulls, scores]")
        fits, small, self.n_unfit = ops_eval.mr_fit_rows(x, int(tailSize))
        self.wbFits, self.smallScoreTensor = fits.to(home), small[:, None].to(home)
        return self.wbFits, self.smallScoreTensor

    def wscore(self, distances, isReversed=False):
        """:463-475.  distances [samples, weibulls] -> float64 CDF values (``isReversed``: 1 - CDF).  A 1-D tensor is repeated once per
        Weibull, as the reference does (:445-446)."""
        d, home = _to_device(distances)
        if d.dim() == 1:
            d = d.repeat(self.wbFits.shape[0], 1)
        small = self.smallScoreTensor
        small = small[:, 0] if small.dim() == 2 else small
        w = ops_eval.mr_wscore(d, self.wbFits.to(d.device).contiguous(), small.to(d.device).contiguous()).to(home)
        return 1 - w if isReversed else w


class Meta_Recognition(object):
    def __init__(self):
        self.mr = libmr()

    def metarec(self, scorematrix, topk, use_columns=True, killscale=1):
        """:587-608.  scorematrix [queries, gallery] similarities -> float64 w-scores of the same shape: the ``topk`` largest scores of
        every gallery column (``use_columns``) or of every query row are scaled down by ``killscale``, a Weibull is fitted to the
        queries - topk - 1 largest remaining scores of every gallery column, and every score becomes its column's CDF value."""
        s, home = _to_device(scorematrix)
        kt = ops_eval.mr_kill_transpose(s, int(topk), use_columns=bool(use_columns), killscale=float(killscale))
        self.mr.FitHigh(kt, int(kt.shape[1] - topk - 1), isSorted=False)
        w = self.mr.wscore(s).to(home)
        self.mr.wbFits, self.mr.smallScoreTensor = self.mr.wbFits.to(home), self.mr.smallScoreTensor.to(home)
        return w

    def mrfuse(self, scores01, scores02, scores03):
        """:610-627.  Three similarity matrices -> their w-score weighted blend (topk = 20 per query row), a float64 numpy array."""
        mats = [_to_device(s)[0] for s in (scores01, scores02, scores03)]
        return ops_eval.mr_fuse(mats, topk=20, use_columns=False, killscale=1.0, out_dtype=torch.float64).cpu().numpy()
