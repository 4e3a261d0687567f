"""Top-k retrieval (ops_eval.pairdist_topk / topk_rows) at configs[4] shape (10,000 x 100,000 x 2048) and Market-1501 shape
(3,368 x 15,913 x 2048), k = 50, both precisions, features resident on the device and prepared once (the operand images are an input
of all four paths).  Timed with HIP events on the stream, --reps repetitions, the paths interleaved inside a repetition; median and
spread (min .. max) per path:
    (a) pairdist         dali_pairdist_prepared into the [nq, ng] matrix
    (b) pairdist + topk  (a), then dali_topk_rows + dali_topk_decode on the matrix
    (c) pairdist_topk    dali_pairdist_topk + dali_topk_decode: no matrix
    (d) torch.topk       torch.topk(matrix, k, largest=False, sorted=True) on the matrix of (a), the matrix not counted
(c) - (a) is the price of the selection on top of the distance; (b) - (a) that of the selection through the matrix.  Also prints the
stats words of (c) (gallery rows selected in the epilogue, rows through the matrix block, overflow events), its scratch bytes, and
checks that (b) and (c) agree bit for bit.

    python scripts/bench_topk.py [--reps 5] [--sizes configs4,market] [--k 50]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from daliid_amd import _lib, ops_eval  # noqa: E402

SIZES = {"market": (3368, 15913, 2048), "configs4": (10000, 100000, 2048)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="configs4,market")
    ap.add_argument("--k", type=int, default=50)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    for size in a.sizes.split(","):
        nq, ng, d = SIZES[size]
        gen = torch.Generator(device=dev).manual_seed(1)
        centers = torch.randn(1500, d, device=dev, generator=gen)            # clustered features, as identities cluster
        q = centers[torch.randint(0, 1500, (nq,), device=dev, generator=gen)] + 1.2 * torch.randn(nq, d, device=dev, generator=gen)
        g = centers[torch.randint(0, 1500, (ng,), device=dev, generator=gen)] + 1.2 * torch.randn(ng, d, device=dev, generator=gen)
        for precision in ("bf16x3", "bf16"):
            qp = ops_eval.PreparedRows(q, normalize=True, precision=precision)
            gp = ops_eval.PreparedRows(g, normalize=True, precision=precision)
            D = torch.empty(nq, ng, device=dev, dtype=torch.float32)
            paths = {
                "a_pairdist": lambda: ops_eval.pairdist_prepared(qp, gp, out=D),
                "b_pairdist_then_topk_rows": lambda: ops_eval.topk_rows(ops_eval.pairdist_prepared(qp, gp, out=D), a.k, return_keys=True),
                "c_pairdist_topk": lambda: ops_eval.pairdist_topk(qp, gp, a.k, return_keys=True, return_stats=True),
                "d_torch_topk_on_matrix": lambda: torch.topk(D, a.k, dim=1, largest=False, sorted=True),
            }
            for fn in paths.values():                                          # warm-up: workspace growth, kernel attributes, torch's allocator
                fn()
            torch.cuda.synchronize()
            times = {name: [] for name in paths}
            outs = {}
            for _ in range(a.reps):
                for name, fn in paths.items():
                    ms, outs[name] = timed(fn)
                    times[name].append(ms)
            agree = bool(torch.equal(outs["b_pairdist_then_topk_rows"][2], outs["c_pairdist_topk"][2]))
            tv, ti = outs["d_torch_topk_on_matrix"]
            torch_values_agree = bool(torch.equal(tv, outs["c_pairdist_topk"][0]))   # (torch leaves the order of tied indices open)
            rec = dict(size=size, nq=nq, ng=ng, d=d, k=a.k, precision=precision, reps=a.reps)
            for name, t in times.items():
                rec[name + "_ms"] = dict(median=round(float(np.median(t)), 3), min=round(min(t), 3), max=round(max(t), 3))
            med = {name: float(np.median(t)) for name, t in times.items()}
            rec["c_minus_a_ms"] = round(med["c_pairdist_topk"] - med["a_pairdist"], 3)
            rec["b_minus_a_ms"] = round(med["b_pairdist_then_topk_rows"] - med["a_pairdist"], 3)
            rec["stats_fused_matrix_overflow"] = outs["c_pairdist_topk"][3].tolist()
            rec["scratch_bytes"] = int(L.dali_pairdist_topk_scratch_bytes(nq, ng, d, a.k, 0, 0, 0))
            rec["matrix_bytes"] = nq * ng * 4
            rec["b_equals_c_bitwise"] = agree
            rec["torch_values_equal"] = torch_values_agree
            print(json.dumps(rec), flush=True)
            del D, qp, gp, outs
            torch.cuda.empty_cache()
        del q, g
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
