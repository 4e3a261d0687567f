"""k-reciprocal re-ranking at Market-1501 shape: 3,368 queries x 15,913 gallery x 2,048-d unit features (oracle.evalrank.synthetic_reid_set,
clustered identities).  Times the three distance blocks (q_g, q_q, g_g on the distance kernel) and ops_eval.re_ranking separately with
HIP events, after a warm-up, over --reps repetitions (median), and prints one JSON line with the milliseconds, N and the mAP without and
with re-ranking.  --cpu also times the numpy restatement (tests/rerank_ref.py) once on the same blocks.

    python scripts/bench_rerank.py [--reps 5] [--cpu]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from daliid_amd import ops_eval  # noqa: E402
from oracle import evalrank as E  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=3368)
    ap.add_argument("--ng", type=int, default=15913)
    ap.add_argument("--dim", type=int, default=2048)
    ap.add_argument("--noise", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu", action="store_true", help="also time the CPU restatement once")
    a = ap.parse_args()
    n_ids = 751                                          # Market-1501's test identities, 5 queries / 22 gallery images each, cut to size
    q, g, qp, gp, qc, gc = E.synthetic_reid_set(n_ids, -(-a.ng // n_ids), -(-a.nq // n_ids), a.dim, noise=a.noise, seed=12)
    q, qp, qc = q[:a.nq], qp[:a.nq], qc[:a.nq]
    g, gp, gc = g[:a.ng], gp[:a.ng], gc[:a.ng]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    q = torch.nn.functional.normalize(q).to(dev)
    g = torch.nn.functional.normalize(g).to(dev)

    def blocks():
        return [ops_eval.pairdist(x, y, normalize=True) for x, y in ((q, g), (q, q), (g, g))]

    b = blocks()                                         # warm-up (workspace growth, code load)
    rr = ops_eval.re_ranking(*b)
    torch.cuda.synchronize()
    t_blocks, t_rr = [], []
    for _ in range(a.reps):
        del b, rr
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        b = blocks()
        e1.record()
        rr = ops_eval.re_ranking(*b)
        e2.record()
        torch.cuda.synchronize()
        t_blocks.append(e0.elapsed_time(e1))
        t_rr.append(e1.elapsed_time(e2))
    _, map_plain = ops_eval.rank_eval(b[0], qp, gp, qc, gc)
    _, map_rr = ops_eval.rank_eval(rr, qp, gp, qc, gc)
    res = dict(bench="rerank", nq=a.nq, ng=a.ng, N=a.nq + a.ng, dim=a.dim, reps=a.reps,
               blocks_ms=round(float(np.median(t_blocks)), 3), rerank_ms=round(float(np.median(t_rr)), 3),
               rerank_ms_min=round(float(np.min(t_rr)), 3), mAP=round(map_plain, 6), mAP_rerank=round(map_rr, 6))
    if a.cpu:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import rerank_ref
        host = [x.cpu().numpy() for x in b]
        t0 = time.perf_counter()
        ref = rerank_ref.re_ranking_ref(*host, 20, 6, 0.3)
        res["cpu_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        res["cpu_max_abs_diff"] = float(np.abs(ref - rr.cpu().numpy()).max())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
