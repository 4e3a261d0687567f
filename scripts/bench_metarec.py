"""Weibull meta-recognition fusion at Market-1501 shape: three similarity matrices of 3,368 queries x 15,913 gallery images, topk = 20
(Meta_Recognition.mrfuse, evaluate.py:610-627).  Times ops_eval.mr_fuse as a whole and its three stages (kill + transpose, the tail fit of
every gallery column, the fused w-score blend) with HIP events, after a warm-up, over --reps repetitions (median and minimum), and sets
them beside a torch-op restatement of the same arithmetic on the same GPU: a yardstick written from the contract in include/daliid.h
(dense fp64 temporaries of [ng, tail], every row stepped until the last one stops, as the reference does), not a port of anything.
Prints one JSON line: the milliseconds, the Newton step counts and the largest differences between the two results.

    python scripts/bench_metarec.py [--reps 5] [--nq 3368 --ng 15913 --topk 20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from daliid_amd import ops_eval  # noqa: E402


def score_matrices(nq, ng, m, dev, dim=128, n_ids=751):
    """Cosine similarities of unit features clustered by identity (every model sees the same identities through its own noise)."""
    g = torch.Generator().manual_seed(12)
    centers = torch.randn(n_ids, dim, generator=g)
    q_id, g_id = torch.arange(nq) % n_ids, torch.arange(ng) % n_ids
    out = []
    for a in range(m):
        noise = 0.8 + 0.2 * a
        q = torch.nn.functional.normalize(centers[q_id] + noise * torch.randn(nq, dim, generator=g)).to(dev)
        gal = torch.nn.functional.normalize(centers[g_id] + noise * torch.randn(ng, dim, generator=g)).to(dev)
        out.append((q @ gal.T).contiguous())
    return out


# ---- the yardstick: the contract in torch ops -------------------------------------------------------------------------------------------
def torch_kill_transpose(S, topk):
    val, idx = torch.topk(S, topk, dim=1)
    return (S - torch.zeros_like(S).scatter_(1, idx, val)).T.contiguous()


def torch_fit_rows(x, T, iters=100, eps=1e-6):
    tail = torch.topk(x, T, dim=1).values
    small = tail[:, T - 1]
    xt = (tail + 1.0) - small[:, None]
    L = torch.log(xt.double())
    l = L.float().double()
    mean_l = l.sum(1) / T
    k = torch.ones(x.shape[0], dtype=torch.float64, device=x.device)
    shape = torch.full_like(k, float("nan"))
    live = torch.ones_like(k, dtype=torch.bool)
    steps = torch.zeros_like(k, dtype=torch.int32)
    for _ in range(iters):
        if not bool(live.any()):
            break
        e = torch.exp(k[:, None] * L)
        el = e * l
        fg, ff, ffp = e.sum(1), el.sum(1), (el * l).sum(1)
        q = ff / fg
        f = q - mean_l - 1.0 / k
        fp = ffp / fg - q * q + 1.0 / (k * k)
        kn = k - f / fp
        steps += live.int()
        bad = live & ~(torch.isfinite(f) & torch.isfinite(fp) & torch.isfinite(kn))
        done = live & ~bad & ((kn - k).abs() < eps)
        shape = torch.where(done, kn, shape)
        live = live & ~bad & ~done
        k = torch.where(live, kn, k)
    scale = (torch.exp(shape[:, None] * L).sum(1) / T) ** (1.0 / shape)
    return torch.stack((shape, scale), 1), small, steps


def torch_wscore(S, fits, small):
    d = ((S + 1.0) - small[None, :]).clamp(min=0)
    w = 1.0 - torch.exp(-torch.pow(d.double() / fits[:, 1][None, :], fits[:, 0][None, :]))
    return torch.where((d == 0) | torch.isnan(fits).any(1)[None, :], torch.zeros_like(w), w)


def torch_fuse(mats, fits, smalls):
    ws = [torch_wscore(S, f, sm) for S, f, sm in zip(mats, fits, smalls)]
    den = sum(ws)
    return torch.where(den == 0, sum(S.double() for S in mats) / len(mats), sum(w * S.double() for w, S in zip(ws, mats)) / den)


def timed(fn, reps):
    """-> (last result, [ms per repetition]); one warm-up call first."""
    out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        del out
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return out, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=3368)
    ap.add_argument("--ng", type=int, default=15913)
    ap.add_argument("--topk", type=int, default=20)
    ap.add_argument("--models", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-yardstick", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    mats = score_matrices(a.nq, a.ng, a.models, dev)
    T = a.nq - a.topk - 1
    stat = lambda ms: (round(float(np.median(ms)), 3), round(float(np.min(ms)), 3))
    res = dict(bench="metarec", nq=a.nq, ng=a.ng, topk=a.topk, models=a.models, tail=T, reps=a.reps)

    fused, ms = timed(lambda: ops_eval.mr_fuse(mats, topk=a.topk, out_dtype=torch.float64), a.reps)
    res["mr_fuse_ms"], res["mr_fuse_ms_min"] = stat(ms)
    kts, ms = timed(lambda: [ops_eval.mr_kill_transpose(S, a.topk) for S in mats], a.reps)
    res["kill_transpose_ms"], res["kill_transpose_ms_min"] = stat(ms)
    fit, ms = timed(lambda: [ops_eval._mr_fit_rows(kt, T, iters=True) for kt in kts], a.reps)
    res["fit_rows_ms"], res["fit_rows_ms_min"] = stat(ms)
    fits, smalls = [f[0] for f in fit], [f[1] for f in fit]
    _, ms = timed(lambda: ops_eval.mr_fuse_fitted(mats, fits, smalls, out_dtype=torch.float64), a.reps)
    res["fuse_ms"], res["fuse_ms_min"] = stat(ms)
    steps = torch.cat([f[3] for f in fit]).cpu().numpy()
    res["newton_steps"] = dict(min=int(steps.min()), median=float(np.median(steps)), mean=round(float(steps.mean()), 2), max=int(steps.max()))
    res["unfit_columns"] = int(sum(int(f[2][1]) for f in fit))

    if not a.no_yardstick:
        t_kts, ms = timed(lambda: [torch_kill_transpose(S, a.topk) for S in mats], a.reps)
        res["torch_kill_transpose_ms"], _ = stat(ms)
        t_fit, ms = timed(lambda: [torch_fit_rows(kt, T) for kt in t_kts], a.reps)
        res["torch_fit_rows_ms"], _ = stat(ms)
        t_fits, t_smalls = [f[0] for f in t_fit], [f[1] for f in t_fit]
        t_fused, ms = timed(lambda: torch_fuse(mats, t_fits, t_smalls), a.reps)
        res["torch_fuse_ms"], _ = stat(ms)
        res["torch_total_ms"] = round(res["torch_kill_transpose_ms"] + res["torch_fit_rows_ms"] + res["torch_fuse_ms"], 3)
        res["torch_global_steps"] = int(max(int(f[2].max()) for f in t_fit))
        ok = torch.isfinite(torch.stack(t_fits)).all(2) & torch.isfinite(torch.stack(fits)).all(2)
        rel = ((torch.stack(fits) - torch.stack(t_fits)).abs() / torch.stack(t_fits).abs())[ok]
        res["kill_transpose_equal"] = bool(all(torch.equal(x, y) for x, y in zip(kts, t_kts)))
        res["fits_max_rel_diff"] = float(rel.max())
        res["fused_max_abs_diff"] = float((fused - t_fused).abs().max())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
