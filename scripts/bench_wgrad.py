"""Weight-gradient launches (incl. the split-K reduce) at the ResNet-50-ReID shapes, per layer, median of reps:
    python scripts/bench_wgrad.py [--filter l4] [--reps 5]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np, torch
from daliid_amd import ops_nn as nn
from bench_convs_shapes import L
bf16 = torch.bfloat16
B = int(os.environ.get("B", "256"))
args = sys.argv[1:]
flt, reps = "", 5
while args:
    a = args.pop(0)
    if a == "--filter": flt = args.pop(0)
    elif a == "--reps": reps = int(args.pop(0))
def timeit(fn, n=20):
    fn(); fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3
tot = 0.0
print("%-14s %3s %5s %6s %8s | time (TFLOP/s, fastest rep)" % ("layer", "x", "Cm", "Ntot", "P"))
for name, H, W, cin, cout, k, st, cnt in L:
    if flt and flt not in name: continue
    pad = k // 2
    x = torch.randn(B, H, W, cin, device="cuda").to(bf16)
    ho, wo = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
    dy = torch.randn(B, ho, wo, cout, device="cuda").to(bf16)
    fl = 2.0 * B * ho * wo * cout * cin * k * k
    t = np.array([timeit(lambda: nn.conv2d_wgrad(x, dy, (k, k), st, pad)) for _ in range(reps)])
    med = np.median(t)
    tot += med * cnt
    print("%-14s x%d %5d %6d %8d | %7.1f us %5.0f TF (%4.1f)" % (name, cnt, cout, cin * k * k, B * ho * wo, med, fl / med / 1e6, t.min()), flush=True)
print("total x count (ms): %.3f" % (tot / 1e3))
