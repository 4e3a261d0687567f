"""Pair ROC (ops_eval.roc_counts / roc_curve) at Market-1501 shape (3,368 x 15,913) and configs[4] shape (10,000 x 100,000), each
with realistic scores (clustered features through the distance kernel) and all tied.  Reports the HIP-event median over --reps of the
device work (dali_roc_build + dali_roc_emit of the dropped curve, scratch allocation excluded), the effective GB/s on the matrix
bytes and on the bytes the passes move (D read twice, the three 4-byte scratch arrays written and read), and separately the
end-to-end numpy return of roc_curve (which includes the device-to-host copy of the curve).  Per-kernel times: run under
`rocprofv3 --kernel-trace --stats`.  --cpu times the numpy restatement (tests/roc_ref.py) once at Market size.

    python scripts/bench_roc.py [--reps 5] [--sizes market,configs4] [--cpu]
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

from daliid_amd import _lib, ops_eval  # noqa: E402

SIZES = {"market": (3368, 15913), "configs4": (10000, 100000)}


def matrix(nq, ng, tied, dev):
    gen = torch.Generator(device=dev).manual_seed(1)
    qp = torch.randint(0, 1500, (nq,), device=dev, generator=gen, dtype=torch.int32)
    gp = torch.randint(0, 1500, (ng,), device=dev, generator=gen, dtype=torch.int32)
    if tied:
        return torch.full((nq, ng), 0.7, device=dev), qp, gp
    f = torch.randn(1500, 256, device=dev, generator=gen)
    q = f[qp.long()] + 1.2 * torch.randn(nq, 256, device=dev, generator=gen)
    g = f[gp.long()] + 1.2 * torch.randn(ng, 256, device=dev, generator=gen)
    return ops_eval.pairdist(q, g, normalize=True), qp, gp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="market,configs4")
    ap.add_argument("--cpu", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    for size in a.sizes.split(","):
        nq, ng = SIZES[size]
        for tied in (False, True):
            d, qp, gp = matrix(nq, ng, tied, dev)
            nbytes = int(L.dali_roc_scratch_bytes(nq, ng))
            scratch = torch.empty(nbytes, device=dev, dtype=torch.uint8)
            out = torch.empty(5, device=dev, dtype=torch.int64)
            ctx, st = _lib.ctx(dev), _lib.stream_ptr()

            def build():
                _lib.check(L.dali_roc_build(ctx, st, _lib.ptr(d), _lib.ptr(qp), _lib.ptr(gp), nq, ng, _lib.ptr(scratch), nbytes, _lib.ptr(out)))

            build()
            n = int(out[0].item())
            thr = torch.empty(n, device=dev)
            fps = torch.empty(n, device=dev, dtype=torch.int64)
            tps = torch.empty(n, device=dev, dtype=torch.int64)

            def emit():
                _lib.check(L.dali_roc_emit(ctx, st, _lib.ptr(scratch), nq, ng, 1, n, _lib.ptr(thr), _lib.ptr(fps), _lib.ptr(tps)))

            times = {"build": [], "emit": []}
            for _ in range(a.reps):
                for name, fn in (("build", build), ("emit", emit)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(); fn(); e1.record(); e1.synchronize()
                    times[name].append(e0.elapsed_time(e1))
            del scratch, thr, fps, tps
            torch.cuda.empty_cache()
            qn, gn = qp.cpu().numpy(), gp.cpu().numpy()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fpr, tpr, th = ops_eval.roc_curve(d, qn, gn)
            e2e = (time.perf_counter() - t0) * 1e3
            N = nq * ng
            ms_b, ms_e = float(np.median(times["build"])), float(np.median(times["emit"]))
            moved = N * 4 * 2 + N * 4 * 2 * 3
            rec = dict(size=size, nq=nq, ng=ng, tied=tied, n_points=n, n_records=int(out[1].item()), build_ms=round(ms_b, 3),
                       emit_ms=round(ms_e, 3), device_ms=round(ms_b + ms_e, 3), matrix_GBps=round(N * 4 / (ms_b + ms_e) / 1e6, 1),
                       moved_GBps=round(moved / (ms_b + ms_e) / 1e6, 1), numpy_e2e_ms=round(e2e, 1),
                       scratch_GB=round(nbytes / 1e9, 2))
            print(json.dumps(rec), flush=True)
            if a.cpu and size == "market" and not tied:
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                import roc_ref
                dn = d.cpu().numpy()
                t0 = time.perf_counter()
                roc_ref.roc_curve(dn, qn, gn)
                print(json.dumps(dict(size=size, cpu_roc_ref_ms=round((time.perf_counter() - t0) * 1e3, 1))), flush=True)
            del d
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
