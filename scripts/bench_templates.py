"""Template evaluation (include/daliid.h: dali_pool_rows, dali_segment_reduce2d, dali_open_set_search) against the same arithmetic in
torch ops.  HIP events on the stream, warm, --reps repetitions (>= 20), median and spread (min .. max) per leg, the legs interleaved
inside a repetition; each kernel reads its input once, so each leg is also printed as bytes / time (to set beside the measured HBM copy
rate of DESIGN.md section 4):
    pool8 / pool64   ops_eval.pool_templates (mean, max) of 100 k x 2048 rows in templates of 8 / of 64, the rows of a template scattered
                     over the matrix; torch: index_add_ and a division / scatter_reduce(amax)
    link             ops_eval.link_templates (min) at Market-1501 size (3,368 x 15,912 frames x 2048, templates of 4) and its
                     segment_reduce2d alone; torch: the whole matrix by mm, then view(Tq, 4, Tg, 4).amin
    open_set         ops_eval.open_set_search on a 3,368 x 15,913 matrix; torch: a stable argsort of every row, the mates' mask, argmax
Every step runs in a process of its own under `timeout`; the driver stops at the first step that does not exit 0.

    python scripts/bench_templates.py [--reps 20] [--steps pool8,pool64,link,open_set]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_SECONDS = {"pool8": 240, "pool64": 240, "link": 300, "open_set": 240}


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


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


def report(rec, times, nbytes):
    import numpy as np
    for name, t in times.items():
        rec[name + "_ms"] = dict(median=round(float(np.median(t)), 3), min=round(min(t), 3), max=round(max(t), 3))
        if name in nbytes:
            rec[name + "_GBps"] = round(nbytes[name] / float(np.median(t)) / 1e6, 1)
    print(json.dumps(rec), flush=True)


def step_pool(step, reps):
    import numpy as np
    import torch
    from daliid_amd import ops_eval
    L = int(step[len("pool"):])
    d = 2048
    T = 100000 // L
    n = T * L
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1)
    fvs = torch.randn(n, d, device=dev, generator=gen)
    order = torch.randperm(n, device=dev, generator=gen).to(torch.int32)
    bounds = torch.arange(0, n + 1, L, device=dev, dtype=torch.int32)
    tid = torch.empty(n, device=dev, dtype=torch.int64)
    tid[order.long()] = torch.arange(T, device=dev).repeat_interleave(L)

    def torch_mean():
        return torch.zeros(T, d, device=dev).index_add_(0, tid, fvs) / float(L)

    def torch_max():
        return torch.full((T, d), float("-inf"), device=dev).scatter_reduce(0, tid.unsqueeze(1).expand(n, d), fvs, "amax")

    paths = {"mean": lambda: ops_eval.pool_templates(fvs, order, bounds, "mean"), "max": lambda: ops_eval.pool_templates(fvs, order, bounds, "max"),
             "torch_mean": torch_mean, "torch_max": torch_max}
    times, outs = run_interleaved(paths, reps)
    nbytes = (n + T) * d * 4
    rec = dict(step=step, n=n, d=d, templates=T, reps=reps, bytes=nbytes, mean_max_abs_diff=float((outs["mean"] - outs["torch_mean"]).abs().max()),
               max_equal=bool(torch.equal(outs["max"], outs["torch_max"])),
               torch_over_mean=round(float(np.median(times["torch_mean"])) / float(np.median(times["mean"])), 2),
               torch_over_max=round(float(np.median(times["torch_max"])) / float(np.median(times["max"])), 2))
    report(rec, times, {"mean": nbytes, "max": nbytes})


def step_link(step, reps):
    import numpy as np
    import torch
    from daliid_amd import ops_eval
    L, d = 4, 2048
    Tq, Tg = 3368 // L, 15913 // L
    nq, ng = Tq * L, Tg * L
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(2)
    q, g = torch.randn(nq, d, device=dev, generator=gen), torch.randn(ng, d, device=dev, generator=gen)
    qb, gb = np.arange(0, nq + 1, L, dtype=np.int32), np.arange(0, ng + 1, L, dtype=np.int32)
    qbd, gbd = torch.from_numpy(qb).to(dev), torch.from_numpy(gb).to(dev)
    frames = ops_eval.pairdist(q, g, normalize=True)

    def torch_link():
        full = 1.0 - torch.nn.functional.normalize(q, dim=1) @ torch.nn.functional.normalize(g, dim=1).T
        return full.view(Tq, L, Tg, L).amin(dim=(1, 3))

    paths = {"link": lambda: ops_eval.link_templates(q, g, qb, gb, linkage="min"), "pairdist": lambda: ops_eval.pairdist(q, g, normalize=True),
             "segment_min": lambda: ops_eval.segment_reduce2d(frames, qbd, gbd, "min"), "segment_mean": lambda: ops_eval.segment_reduce2d(frames, qbd, gbd, "mean"),
             "torch_link": torch_link, "torch_segment_min": lambda: frames.view(Tq, L, Tg, L).amin(dim=(1, 3))}
    times, outs = run_interleaved(paths, reps)
    nbytes = (nq * ng + Tq * Tg) * 4
    rec = dict(step=step, nq=nq, ng=ng, d=d, template=L, reps=reps, bytes=nbytes, link_equals_segment=bool(torch.equal(outs["link"], outs["segment_min"])),
               segment_equals_torch=bool(torch.equal(outs["segment_min"], outs["torch_segment_min"])),
               link_max_abs_diff_torch=float((outs["link"] - outs["torch_link"]).abs().max()),
               torch_over_link=round(float(np.median(times["torch_link"])) / float(np.median(times["link"])), 2),
               torch_over_segment_min=round(float(np.median(times["torch_segment_min"])) / float(np.median(times["segment_min"])), 2))
    report(rec, times, {"segment_min": nbytes, "segment_mean": nbytes})


def step_open_set(step, reps):
    import numpy as np
    import torch
    from daliid_amd import ops_eval
    nq, ng = 3368, 15913
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(3)
    D = torch.rand(nq, ng, device=dev, generator=gen) * 2
    rng = np.random.default_rng(3)
    gs = torch.from_numpy(rng.integers(0, 751, ng).astype(np.int32)).to(dev)          # Market: 15,913 gallery images of 751 identities
    qs = torch.from_numpy(rng.integers(0, 900, nq).astype(np.int32)).to(dev)          # about one probe in six is not mated

    def torch_search():
        srt = torch.argsort(D, dim=1, stable=True)
        mate = gs[srt] == qs.unsqueeze(1)
        pos, npos = mate.to(torch.int8).argmax(dim=1), (~mate).to(torch.int8).argmax(dim=1)
        mated = mate.any(dim=1)
        col, ncol = srt.gather(1, pos.unsqueeze(1)).squeeze(1), srt.gather(1, npos.unsqueeze(1)).squeeze(1)
        inf = torch.full((nq,), float("inf"), device=dev)
        return (torch.where(mated, D.gather(1, col.unsqueeze(1)).squeeze(1), inf), torch.where(mated, col, -1).to(torch.int32),
                D.gather(1, ncol.unsqueeze(1)).squeeze(1), ncol.to(torch.int32), torch.where(mated, pos, -1).to(torch.int32))

    paths = {"open_set_search": lambda: ops_eval.open_set_search(D, qs, gs), "torch": torch_search}
    times, outs = run_interleaved(paths, reps)
    nbytes = nq * ng * 4
    rec = dict(step=step, nq=nq, ng=ng, reps=reps, bytes=nbytes, equal=all(bool(torch.equal(a, b)) for a, b in zip(outs["open_set_search"], outs["torch"])),
               mated=int((outs["open_set_search"][4] >= 0).sum()),
               torch_over_kernel=round(float(np.median(times["torch"])) / float(np.median(times["open_set_search"])), 2))
    report(rec, times, {"open_set_search": nbytes})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", default="pool8,pool64,link,open_set")
    ap.add_argument("--step", default=None, help="run this one step in this process (what the driver starts)")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    if a.step is not None:
        import torch
        torch.cuda.set_device(0)
        (step_pool if a.step.startswith("pool") else step_link if a.step == "link" else step_open_set)(a.step, a.reps)
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
