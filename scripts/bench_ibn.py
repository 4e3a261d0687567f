"""IBN-a: (a) dali_ibn_act at batch B on the 13 launches of ResNet-50-IBN-a at 256 x 128 against dali_bn_act on the same tensors in the same
run (the same bytes, one read and one write, no reduction; both from x to a separate y), and dali_ibn_act in place as the plan runs it; (b) the eval forward of
ResNet-50-IBN-a against plain ResNet-50, and ResNet-101-IBN-a, at batch B.

Timing: HIP events around `reps` back-to-back calls after 3 warm-up calls, the variants alternating over 3 rounds (the median is
reported, the spread beside it).  The op cycles through enough tensors that a pass does not find its input in the 256 MB Infinity Cache.
GB/s = (one read + one write of the tensor) / time.
   python scripts/bench_ibn.py [B=500] [reps=200] [fwd_reps=10]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import statistics

import torch
from daliid_amd import Encoders, _lib

B = int(sys.argv[1]) if len(sys.argv) > 1 else 500
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
fwd_reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
SHAPES = [(2048, 64, 3), (2048, 128, 1), (512, 128, 3), (512, 256, 1), (128, 256, 5)]          # (hw, C, launches per forward)
bf16 = torch.bfloat16


def timed(fn, n):
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


def rounds(variants, n):
    """{name: fn} -> {name: (median ms, min, max)} over 3 alternating rounds"""
    t = {k: [] for k in variants}
    for _ in range(3):
        for k, fn in variants.items():
            t[k].append(timed(fn, n))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def op_table():
    L, ctx = _lib.lib(), _lib.ctx(0)
    print("%-14s %10s %8s %10s %8s %7s %12s   (min .. max of 3 rounds)" % ("(hw, C) x n", "ibn_act us", "GB/s", "bn_act us", "GB/s", "ratio", "in place us"))
    total = 0.0
    for hw, C, count in SHAPES:
        nbytes = B * hw * C * 2
        pool = max(2, -(-600 * 2 ** 20 // nbytes))
        xs = [torch.randn(B, hw, C, device="cuda").to(bf16) for _ in range(pool)]
        ys = [torch.empty_like(xs[0]) for _ in range(pool)]              # outputs cycle as the inputs do: neither op's stores stay in the cache
        c_in = C // 2
        gamma, beta = torch.rand(c_in, device="cuda") + 0.5, torch.randn(c_in, device="cuda")
        scale, shift = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda")
        i = [0]

        def ibn(inplace=False):
            x = xs[i[0] % pool]; y = x if inplace else ys[i[0] % pool]; i[0] += 1
            _lib.check(L.dali_ibn_act(ctx, _lib.stream_ptr(), _lib.ptr(x), B, hw, C, c_in, _lib.ptr(gamma), _lib.ptr(beta), 1e-5, 1, _lib.ptr(y), None, None))

        def bn():
            x = xs[i[0] % pool]; y = ys[i[0] % pool]; i[0] += 1
            _lib.check(L.dali_bn_act(ctx, _lib.stream_ptr(), _lib.ptr(x), _lib.ptr(scale), _lib.ptr(shift), None, None, None, None, 1, B * hw, C,
                                     _lib.ptr(y), None))

        r = rounds({"ibn": ibn, "bn": bn, "inplace": lambda: ibn(True)}, reps)
        gbs = lambda ms: 2 * nbytes / ms / 1e6
        print("(%4d, %3d) x %d %10.1f %8.0f %10.1f %8.0f %7.2f %12.1f   ibn %.1f .. %.1f, bn %.1f .. %.1f" % (
            hw, C, count, r["ibn"][0] * 1e3, gbs(r["ibn"][0]), r["bn"][0] * 1e3, gbs(r["bn"][0]), r["ibn"][0] / r["bn"][0], r["inplace"][0] * 1e3,
            r["ibn"][1] * 1e3, r["ibn"][2] * 1e3, r["bn"][1] * 1e3, r["bn"][2] * 1e3))
        total += count * r["inplace"][0]
        del xs, ys
    print("the 13 ibn_act launches of one forward: %.3f ms" % total)
    return total


def forwards():
    x = torch.randn(B, 3, 256, 128, device="cuda")
    nets = {"resnet50": Encoders.ResNet50ReID(seed=12).eval(), "resnet50IBN": Encoders.ResNet50IBNReID(seed=12).eval()}
    with torch.no_grad():
        r = rounds({k: (lambda net=net: net(x)) for k, net in nets.items()}, fwd_reps)
        for k, v in r.items():
            print("%-14s eval forward %8.2f ms (%.2f .. %.2f)  %7.0f img/s  arena %.2f GB" % (k, v[0], v[1], v[2], B / v[0] * 1e3, nets[k]._arena.numel() / 1e9))
        print("ratio resnet50IBN / resnet50: %.3f (derived share of the IBN pass: +11 %%; accepted up to 1.22)" % (r["resnet50IBN"][0] / r["resnet50"][0]))
        del nets
        torch.cuda.empty_cache()
        net = Encoders.ResNet101IBNReID(seed=12).eval()
        v = rounds({"resnet101IBN": lambda: net(x)}, fwd_reps)["resnet101IBN"]
        print("%-14s eval forward %8.2f ms (%.2f .. %.2f)  %7.0f img/s  arena %.2f GB" % ("resnet101IBN", v[0], v[1], v[2], B / v[0] * 1e3, net._arena.numel() / 1e9))
    return r


if __name__ == "__main__":
    print("B=%d, %d op reps, %d forward reps, %s" % (B, reps, fwd_reps, torch.cuda.get_device_name(0)))
    ibn_ms = op_table()
    r = forwards()
    print("forward difference %.3f ms, of which the ibn_act launches %.3f ms" % (r["resnet50IBN"][0] - r["resnet50"][0], ibn_ms))
