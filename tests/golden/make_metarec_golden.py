#!/usr/bin/env python3
"""Generate tests/golden/metarec.npz by RUNNING the reference's own libmr / Meta_Recognition (Person-ReID/evaluate.py:394-627).

Run in the build container only (the reference tree does not exist on the GPU box):

    python tests/golden/make_metarec_golden.py

evaluate.py is imported as-is, with the inert placeholder modules of make_golden.py standing in for what its header imports and never
calls on this path (torchreid, torchvision, joblib, sklearn, tabulate, PIL, termcolor and the reference's own Encoders / validateModels /
datasetUtils / getFeatures / config / make_models).  Only data is written: the score matrices, and per model the reference's wbFits, smallScoreTensor and w-scores; for the
three-model case its mrfuse result as well.  No reference source text is copied.

Cases (nq, ng, topk): (12, 33, 3), (40, 33, 5), (64, 40, 20) on both axes, (40, 33, 5) at killscale 0.5, (72, 96, 20) with three models.
topk = 20 is not used with nq <= 40: most columns are unfit there in the reference itself."""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (puts the reference directory and the repository root on sys.path)


def load_reference():
    MG.install_shims()
    for n in ["joblib", "sklearn", "sklearn.metrics", "sklearn.cluster", "tabulate", "PIL", "Encoders", "validateModels", "datasetUtils",
              "getFeatures", "config", "make_models"]:
        sys.modules[n] = MG._Inert(n)
    import evaluate as REF
    assert REF.__file__.startswith(MG.REF), REF.__file__
    return REF


def score_matrix(nq, ng, seed, d=64, noise=0.6):
    """Cosine similarities of random unit features; query i has planted matches at gallery i % ng and (i + nq) % ng."""
    g = torch.Generator().manual_seed(seed)
    q, gal = MG.unit_rows(nq, d, g), MG.unit_rows(ng, d, g)
    for i in range(nq):
        for j in {i % ng, (i + nq) % ng}:
            v = q[i] + noise * torch.randn(d, generator=g) / d ** 0.5
            gal[j] = v / v.norm()
    return (q @ gal.T).contiguous()


def run_metarec(REF, S, topk, use_columns, killscale):
    mr = REF.Meta_Recognition()
    w = mr.metarec(S, topk, use_columns=use_columns, killscale=killscale)
    fits, small = mr.mr.wbFits, mr.mr.smallScoreTensor[:, 0]
    assert fits.dtype == torch.float64 and small.dtype == torch.float32 and w.dtype == torch.float64
    unfit = ~torch.isfinite(fits).all(dim=1) | (fits[:, 0] == 0)
    assert not bool(unfit.any()), "the reference left %d unfit columns" % int(unfit.sum())
    return fits.numpy(), small.numpy(), w.numpy()


def main():
    REF = load_reference()
    out = {}
    cases = [("q12_g33_k3_rows", 12, 33, 3, False, 1.0, 1), ("q40_g33_k5_rows", 40, 33, 5, False, 1.0, 1),
             ("q64_g40_k20_rows", 64, 40, 20, False, 1.0, 1), ("q64_g40_k20_cols", 64, 40, 20, True, 1.0, 1),
             ("q40_g33_k5_half", 40, 33, 5, False, 0.5, 1), ("q72_g96_k20_three", 72, 96, 20, False, 1.0, 3)]
    for ci, (name, nq, ng, topk, cols, ks, m) in enumerate(cases):
        mats = [score_matrix(nq, ng, 100 * ci + a, noise=0.6 + 0.2 * a) for a in range(m)]
        out[name + "/meta"] = np.array([nq, ng, topk, int(cols), m], dtype=np.int64)
        out[name + "/killscale"] = np.array(ks, dtype=np.float64)
        for a, S in enumerate(mats):
            fits, small, w = run_metarec(REF, S, topk, cols, ks)
            out["%s/S%d" % (name, a)], out["%s/fits%d" % (name, a)] = S.numpy(), fits
            out["%s/small%d" % (name, a)], out["%s/w%d" % (name, a)] = small, w
        if m == 3:                                  # mrfuse fixes topk = 20, use_columns = False, killscale = 1
            assert (topk, cols, ks) == (20, False, 1.0)
            with contextlib.redirect_stdout(io.StringIO()):
                fused = REF.Meta_Recognition().mrfuse(*mats)
            assert fused.dtype == np.float64 and fused.shape == (nq, ng)
            den = sum(out["%s/w%d" % (name, a)] for a in range(3))
            low = float((den < 1e-3).mean())
            assert low <= 0.01, "%.2f %% of the fused entries have a w-score sum below 1e-3" % (100 * low)
            out[name + "/fused"] = fused
            print("%s: %.3f %% of entries under the w-score threshold" % (name, 100 * low))
    path = os.path.join(HERE, "metarec.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
