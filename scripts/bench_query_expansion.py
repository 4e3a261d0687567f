"""Query expansion (ops_eval.query_expansion, expand="all") at Market-1501 size (3,368 + 15,913 rows x 2048) and at configs[4] size
(10,000 + 100,000 rows x 2048), k = 10, alpha = 3, times = 1, and mINP beside CMC / mAP.  HIP events on the stream, warm, --reps
repetitions (>= 20), median and spread (min .. max) per leg, the legs interleaved inside a repetition:
    prepare   dali_pairdist_prepare of the pool (normalise + bf16x3 image)
    topk      dali_pairdist_topk(P, P, k) + decode: the k nearest rows of every row, no (Nq + Ng)^2 matrix
    combine   dali_qe_combine: the gather.  It reads n k d 4 bytes of scattered rows and writes n d 4; printed with bytes / s
    torch     (Market size only) the yardstick: normalize, mm, topk, index_select, weighted mean -- it holds the N x N matrix
    rank_eval / rank_eval_inp   on one random [nq, ng] matrix with Market-like labels: the same matrix read once by either
Every step runs in a process of its own under `timeout`; the driver stops at the first step that does not exit 0.

    python scripts/bench_query_expansion.py [--reps 20] [--steps market,configs4,rank_market,rank_configs4]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"market": (3368, 15913, 2048), "configs4": (10000, 100000, 2048)}
STEP_SECONDS = {"market": 240, "configs4": 420, "rank_market": 180, "rank_configs4": 300}
K, ALPHA = 10, 3


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def summarise(times):
    import numpy as np
    return {name + "_ms": dict(median=round(float(np.median(t)), 3), min=round(min(t), 3), max=round(max(t), 3)) for name, t in times.items()}


def run_interleaved(paths, reps):
    import torch
    for fn in paths.values():                    # warm-up: workspace growth, torch's allocator
        fn()
    torch.cuda.synchronize()
    times, outs = {name: [] for name in paths}, {}
    for _ in range(reps):
        for name, fn in paths.items():
            ms, outs[name] = timed(fn)
            times[name].append(ms)
    return times, outs


def step_expand(size, reps):
    import numpy as np
    import torch
    from daliid_amd import ops_eval
    nq, ng, d = SIZES[size]
    n = nq + ng
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1)
    centers = torch.randn(1500, d, device=dev, generator=gen)                # clustered features, as identities cluster
    feat = centers[torch.randint(0, 1500, (n,), device=dev, generator=gen)] + 1.2 * torch.randn(n, d, device=dev, generator=gen)
    out = torch.empty_like(feat)
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    P = ops_eval.PreparedRows(feat, normalize=True, precision="bf16x3")
    dist, idx = ops_eval.pairdist_topk(P, P, K, metric="cosine")
    paths = {
        "prepare": lambda: ops_eval.PreparedRows(feat, normalize=True, precision="bf16x3"),
        "topk": lambda: ops_eval.pairdist_topk(P, P, K, metric="cosine"),
        "combine": lambda: ops_eval._qe_combine(feat, idx, dist, ALPHA, True, out, status),
        "whole": lambda: ops_eval.query_expansion(feat[:nq], feat[nq:], k=K, alpha=ALPHA, times=1, expand="all"),
    }

    def torch_yardstick():
        u = torch.nn.functional.normalize(feat, dim=1)
        s, i = torch.topk(u @ u.T, K, dim=1)
        return (feat.index_select(0, i.reshape(-1)).view(n, K, d) * (s ** ALPHA).unsqueeze(2)).mean(dim=1)

    if size == "market":
        paths["torch"] = torch_yardstick
    times, outs = run_interleaved(paths, reps)
    assert int(status.item()) == 0
    gather_bytes, write_bytes = n * K * d * 4, n * d * 4
    med = float(np.median(times["combine"]))
    rec = dict(step=size, n=n, d=d, k=K, alpha=ALPHA, reps=reps, gather_bytes=gather_bytes, write_bytes=write_bytes,
               combine_gather_GBps=round(gather_bytes / med / 1e6, 1), combine_total_GBps=round((gather_bytes + write_bytes) / med / 1e6, 1))
    rec.update(summarise(times))
    if size == "market":
        rec["torch_over_whole"] = round(float(np.median(times["torch"])) / float(np.median(times["whole"])), 2)
        rec["torch_max_abs_diff"] = float((outs["torch"] - torch.cat(outs["whole"])).abs().max())
    print(json.dumps(rec), flush=True)


def step_rank(size, reps):
    import numpy as np
    import torch
    from daliid_amd import ops_eval
    nq, ng, _ = SIZES[size[len("rank_"):]]
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(2)
    distmat = torch.rand(nq, ng, device=dev, generator=gen) * 2
    rng = np.random.default_rng(2)
    n_ids = max(ng // 21, 2)                                                  # Market: 15,913 gallery images of 751 identities
    qp, gp = rng.integers(0, n_ids, nq), rng.integers(0, n_ids, ng)
    qc, gc = rng.integers(0, 6, nq), rng.integers(0, 6, ng)
    # both timed from the Python entry: each includes the same id factorisation, upload and status read
    paths = {"rank_eval": lambda: ops_eval.rank_eval(distmat, qp, gp, qc, gc), "rank_eval_inp": lambda: ops_eval.rank_eval_inp(distmat, qp, gp, qc, gc)}
    times, outs = run_interleaved(paths, reps)
    rec = dict(step=size, nq=nq, ng=ng, reps=reps, mAP=outs["rank_eval"][1], mINP=outs["rank_eval_inp"],
               inp_over_rank_eval=round(float(np.median(times["rank_eval_inp"])) / float(np.median(times["rank_eval"])), 3))
    rec.update(summarise(times))
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", default="market,configs4,rank_market,rank_configs4")
    ap.add_argument("--step", default=None, help="run this one step in this process (what the driver starts)")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    if a.step is not None:
        import torch
        torch.cuda.set_device(0)
        (step_rank if a.step.startswith("rank_") else step_expand)(a.step, a.reps)
        return 0
    for step in a.steps.split(","):
        cmd = ["timeout", "-k", "10", str(STEP_SECONDS[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(a.reps)]
        rc = subprocess.call(cmd)
        if rc != 0:
            print("step %s ended with status %d: stopping" % (step, rc), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
