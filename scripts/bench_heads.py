"""The multi-output head against one forward per output, full ResNet-50 at batch B, 256 x 128 (timed as scripts/time_eval_forward.py does:
3 warm-up runs, then HIP events around `reps` back-to-back runs):
  (a) one model(x);  (b) three forwards, one per pooling;  (c) one forward_heads with the three poolings;
  (d) one forward_heads with seven heads (three poolings, three body parts and their whole-body max) plus the heat map;
  (e) the head kernels alone on a layer4-sized map: dali_head_pool_fwd x 7 against one dali_head_pool_multi with the seven heads.
   python scripts/bench_heads.py [B=500] [reps=20]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from daliid_amd import Encoders, ops_nn

B = int(sys.argv[1]) if len(sys.argv) > 1 else 500
n = int(sys.argv[2]) if len(sys.argv) > 2 else 20
POOLINGS = ("both", "gap", "gmp")


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(n):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / n


net = Encoders.ResNet50ReID(seed=12).eval()
x = torch.randn(B, 3, 256, 128, device="cuda")
rows, cols = net.head_map(256, 128)
seven = [(p, None) for p in POOLINGS] + [("gmp", r) for r in Encoders.default_parts(rows)] + [("gmp", None)]


def three_forwards():
    for p in POOLINGS:
        net.feature = p
        net(x)
    net.feature = "both"


with torch.no_grad():
    res = [("one model(x)", timed(lambda: net(x))),
           ("three forwards, one per pooling", timed(three_forwards)),
           ("forward_heads, three poolings", timed(lambda: net.forward_heads(x, [(p, None) for p in POOLINGS]))),
           ("forward_heads, seven heads + heat map", timed(lambda: net.forward_heads(x, seven, heatmap=True)))]
    fmap = torch.randn(B, rows, cols, net.feat_dim, device="cuda").relu().to(torch.bfloat16)
    res += [("head_pool_fwd x 7", timed(lambda: [ops_nn.head_pool_fwd(fmap, p) for p, _ in seven])),
            ("head_pool_multi, seven heads", timed(lambda: ops_nn.head_pool_multi(fmap, seven))),
            ("channel_sum", timed(lambda: ops_nn.channel_sum(fmap)))]
print("B=%d, %d reps, %s" % (B, n, torch.cuda.get_device_name(0)))
for name, ms in res:
    print("%-40s %8.3f ms" % (name, ms))
