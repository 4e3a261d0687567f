"""ViT-B/16 linear weight gradients at batch 128 (25216 rows), with and without the bias gradient riding on the GEMM, median of 3:
    python scripts/bench_vit_wgrad.py"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from daliid_amd import ops_vit as V
bf16 = torch.bfloat16
rows = 128 * 197
def timeit(fn, n=20):
    fn(); fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3
xs = {k: torch.randn(rows, k, device="cuda").to(bf16) for k in (768, 2304, 3072)}
print("%-22s | with / without the bias gradient" % "layer (K x N)")
tot = np.zeros(2)
for name, K, N, cnt in (("qkv 768x2304", 768, 2304, 12), ("proj 768x768", 768, 768, 12), ("fc1 768x3072", 768, 3072, 12), ("fc2 3072x768", 3072, 768, 12)):
    t = np.zeros((3, 2))
    for r in range(3):
        t[r, 0] = timeit(lambda: V.linear_wgrad(xs[K], xs[N], want_bias=True))
        t[r, 1] = timeit(lambda: V.linear_wgrad(xs[K], xs[N], want_bias=False))
    m = np.median(t, 0); tot += m * cnt
    fl = 2.0 * rows * K * N
    print("%-22s | bias %6.1f us %4.0f TF, none %6.1f us" % (name, m[0], fl / m[0] / 1e6, m[1]), flush=True)
print("x12 layers (ms): bias %.3f, none %.3f" % (tot[0] / 1e3, tot[1] / 1e3))
