"""A/B of two library builds on the kernels of nnops.hip / vit_ops.hip / conv.hip (select the build with DALIID_LIB; one process per build):

  python scripts/ab_nnops.py bits OUT.json [ODD_DIR]   sha256 of every output on seeded inputs: bn_bwd (three mask modes, single / dual, with / without
                                                       dz), maxpool_bn_bwd, bn_act, head pool, LayerNorm, attention, linear bias gradients (colsum),
                                                       bnlin (transposed weights), the conv / conv1x1_* / linear single ops (every output stage of
                                                       conv.hip, edge shapes included), one ResNet and one ViT train step (features + every gradient),
                                                       one ResNet eval forward; the odd-sided max-pool outputs go to ODD_DIR as .npz
  python scripts/ab_nnops.py cmp A.json B.json [ODD_DIR_A ODD_DIR_B]   differing arrays; ulp distances of the odd-sided max-pool outputs
  python scripts/ab_nnops.py time [N H W C]            maxpool_bn_bwd (default 256x63x33x64, the odd path): 5 runs of 20 launches, us per launch
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
bf16 = torch.bfloat16
ODD_SHAPES = [(2, 7, 5, 64), (1, 5, 8, 32), (1, 6, 9, 16), (2, 3, 1, 8), (1, 1, 1, 8), (256, 63, 33, 64)]


def _raw(t):
    t = t.detach().contiguous().cpu()
    return t.view(torch.int16).numpy() if t.dtype == bf16 else t.numpy()


def _bn_inputs(P, C, g):
    raw = torch.randn(P, C, generator=g).to(bf16)
    mean, invstd = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    scale = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.3, -1.0, 1.0) * invstd
    return raw, mean, invstd, scale, torch.randn(C, generator=g) * 0.3


def _pool_inputs(shape, g):
    n, h, w, C = shape
    raw, mean, invstd, scale, shift = _bn_inputs(n * h * w, C, g)
    dp = torch.randn(n, (h + 1) // 2, (w + 1) // 2, C, generator=g).to(bf16)
    return [t.cuda() for t in (raw.view(n, h, w, C), mean, invstd, scale, shift, dp)]


def _pack_bits(b):
    b = b.flatten().to(torch.int32).view(-1, 8)
    return (b << torch.arange(8, dtype=torch.int32, device=b.device)).sum(1).to(torch.uint8)


def _conv_bits(put, ops_nn, ops_vit, g):
    """every output stage of conv.hip's forward / data-gradient / linear GEMMs: the convolution single ops over the shapes of tests/test_gpu_conv.py,
    the conv1x1_* and linear single ops over its 1x1 / stride-1 shapes and over edge and 256 x 320-tile shapes (out_shift with bias included)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("conv_cases", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "test_gpu_conv.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    def rnd(*shape, s=1.0):
        return (torch.randn(shape, generator=g) * s).to(bf16).cuda()

    def vec(n, lo=0.5, hi=1.5):
        return (lo + (hi - lo) * torch.rand(n, generator=g)).cuda()

    def keep(n):
        return _pack_bits(torch.rand(n, generator=g) < 0.6).cuda()

    def try_put(name, fn):
        """an entry point that refuses a shape is recorded as refused (both builds must then refuse it)"""
        from daliid_amd import _lib
        try:
            put(name, fn())
        except _lib.DaliError as e:
            put(name + " refused", (torch.tensor([len(str(e))]),))

    flat = [(300, 32, 136), (300, 32, 64), (300, 32, 72), (25216, 768, 3072), (25216, 3072, 768), (32896, 512, 512)]
    for n, h, w, cin, cout, r, s, stride, pad in mod.CASES:
        name = "conv %s" % ((n, h, w, cin, cout, r, s, stride, pad),)
        ho, wo = (h + 2 * pad - r) // stride + 1, (w + 2 * pad - s) // stride + 1
        x, wt_f, wt_d = rnd(n, h, w, cin), rnd(cout, r, s, cin, s=0.1), rnd(cin, r, s, cout, s=0.1)
        dy, res = rnd(n, ho, wo, cout), rnd(n, h, w, cin)
        try_put(name + " fwd", lambda: ops_nn.conv2d_fwd(x, wt_f, stride, pad, want_stats=True))
        try_put(name + " fwd in_bn", lambda: ops_nn.conv2d_fwd(x, wt_f, stride, pad, in_scale=vec(cin), in_shift=vec(cin, -0.5, 0.5), in_relu=True, want_stats=True))
        try_put(name + " bn_act", lambda: (ops_nn.conv2d_bn_act(x, wt_f, vec(cout), vec(cout, -0.5, 0.5), stride, pad, relu=True),))
        try_put(name + " dgrad", lambda: (ops_nn.conv2d_dgrad(dy, wt_d, (h, w), stride, pad),))
        try_put(name + " dgrad res mask", lambda: (ops_nn.conv2d_dgrad(dy, wt_d, (h, w), stride, pad, residual=res, residual_mask=keep(res.numel())),))
        if r == 1 and stride == 1:
            flat.append((n * h * w, cin, cout))
    for P, cin, cout in flat:
        name = "flat %dx%dx%d" % (P, cin, cout)
        x, w, res = rnd(P, cin), rnd(cout, cin, s=cin ** -0.5), rnd(P, cout)
        sc, sh, bi, rsc = vec(cout), vec(cout, -0.5, 0.5), vec(cout, -0.5, 0.5), vec(cout)
        try_put(name + " fused full", lambda: ops_nn.conv1x1_fused(x, w, out_scale=sc, out_shift=sh, residual=res, res_scale=rsc, relu=True, want_bits=True,
                                                                   out_mask=keep(P * cout)))
        try_put(name + " fused shift+bias", lambda: ops_nn.conv1x1_fused(x, w, out_scale=sc, out_shift=sh, bias=bi, residual=res, res_scale=rsc, relu=True, want_bits=True))
        try_put(name + " fused bias", lambda: (ops_nn.conv1x1_fused(x, w, out_scale=sc, bias=bi, relu=True), ops_nn.conv1x1_fused(x, w, out_shift=sh)))
        if cin % 64 == 0:
            x1, x2 = x[:, :cin // 2].contiguous(), x[:, cin // 2:].contiguous()
            try_put(name + " cat", lambda: (ops_nn.conv1x1_cat(x1, x2, w, bias=bi),))
        try_put(name + " linear", lambda: ops_vit.linear_fwd(x, w, bias=bi, act=1, want_pre=True) + (ops_vit.linear_fwd(x, w, bias=bi, residual=res), ops_vit.linear_fwd(x, w)))
        try_put(name + " linear scaled", lambda: (ops_vit.linear_fwd_scaled(x, w, vec(P, 0.0, 1.2), bias=bi, residual=res), ops_vit.linear_fwd_scaled(x, w, vec(P), bias=bi, act=1)))
        try_put(name + " linear dgrad", lambda: (ops_vit.linear_dgrad(x, w, gelu_pre=res), ops_vit.linear_dgrad(x, w, residual=res)))


def run_bits(out_json, odd_dir):
    from daliid_amd import Encoders, ops_nn, ops_vit, vit_pytorch
    res = {}

    def put(name, tensors):
        for i, t in enumerate(tensors):
            if t is not None:
                res["%s/%d" % (name, i)] = hashlib.sha256(_raw(t).tobytes()).hexdigest()

    for P, C in [(4 * 6 * 5, 64), (2 * 5 * 5, 96), (3 * 3 * 3, 2048), (65000, 256), (32768, 2048)]:
        g = torch.Generator().manual_seed(P + C)
        grad = torch.randn(P, C, generator=g).to(bf16).cuda()
        a = [t.cuda() for t in _bn_inputs(P, C, g)]
        b = [t.cuda() for t in _bn_inputs(P, C, g)]
        y = (a[0].float() * a[3] + a[4] + b[0].float() * b[3] + b[4]).to(bf16)
        bits = ((y.flatten().float() > 0).view(-1, 8).to(torch.int32) << torch.arange(8, dtype=torch.int32, device="cuda")).sum(1).to(torch.uint8)
        for mode, kw in [("recompute", {}), ("ymask", dict(ymask=y)), ("ybits", dict(ybits=bits))]:
            for dual in (False, True):
                for dz in (False, True):
                    out = ops_nn.bn_bwd(grad, a[0], a[1], a[2], a[3], a[4], relu=True, side_b=tuple(b[:4]) if dual else None, want_dz=dz, **kw)
                    put("bn_bwd %dx%d %s dual%d dz%d" % (P, C, mode, dual, dz), out)
        put("bn_act %dx%d" % (P, C), ops_nn.bn_act(a[0], a[3], a[4], raw2=b[0], scale2=b[3], shift2=b[4], relu=True, want_mask=True))
    for shape in [(2, 8, 6, 64), (256, 128, 64, 64)] + ODD_SHAPES:
        raw, mean, invstd, scale, shift, dp = _pool_inputs(shape, torch.Generator().manual_seed(sum(shape)))
        pooled, arg = ops_nn.maxpool_bn_fwd(raw, scale, shift)
        out = ops_nn.maxpool_bn_bwd(dp, arg, raw, mean, invstd, scale)
        name = "maxpool %dx%dx%dx%d" % shape
        if shape in ODD_SHAPES:
            put(name + " fwd", (pooled, arg))
            if odd_dir:
                os.makedirs(odd_dir, exist_ok=True)
                # fp64 sums through torch's own pool (z in fp32 as the kernel forms it; ties are as good as absent in normal deviates)
                n, h, w, C = shape
                _, idx = torch.nn.functional.max_pool2d((raw.float() * scale + shift).permute(0, 3, 1, 2), 3, 2, 1, return_indices=True)
                dz = torch.zeros(n, C, h * w, dtype=torch.float64, device="cuda").scatter_add_(2, idx.flatten(2), dp.permute(0, 3, 1, 2).flatten(2).double())
                dz = dz.view(n, C, h, w).permute(0, 2, 3, 1)
                xhat = (raw.double() - mean.double()) * invstd.double()
                np.savez(os.path.join(odd_dir, name.replace(" ", "_") + ".npz"), draw=_raw(out[0]), dgamma=_raw(out[1]), dbeta=_raw(out[2]),
                         ref_dgamma=_raw((dz * xhat).sum((0, 1, 2))), ref_dbeta=_raw(dz.sum((0, 1, 2))), abs_dgamma=_raw((dz * xhat).abs().sum((0, 1, 2))))
        else:
            put(name, (pooled, arg) + tuple(out))
    g = torch.Generator().manual_seed(7)
    for shape in [(4, 16, 8, 2048), (3, 5, 3, 64)]:
        x = torch.randn(shape, generator=g).to(bf16).cuda()
        f, arg = ops_nn.head_pool_fwd(x)
        put("head_pool %dx%dx%dx%d" % shape, (f, arg, ops_nn.head_pool_bwd(torch.randn(f.shape, generator=g).cuda(), arg, shape[1:3])))
    for rows, C in [(197 * 3, 768), (50, 64), (7, 2048)]:
        x, dy = torch.randn(rows, C, generator=g).to(bf16).cuda(), torch.randn(rows, C, generator=g).to(bf16).cuda()
        gamma, beta = (torch.rand(C, generator=g) + 0.5).cuda(), torch.randn(C, generator=g).cuda()
        yln, mean, rstd = ops_vit.layernorm_fwd(x, gamma, beta)
        put("layernorm %dx%d" % (rows, C), (yln, mean, rstd) + tuple(ops_vit.layernorm_bwd(dy, x, gamma, mean, rstd)))
    for rows, K, N in [(197 * 2, 768, 2304), (100, 3072, 768), (333, 768, 3072)]:           # bias gradient = column sums at C = 2304, 768, 3072
        x, dy = torch.randn(rows, K, generator=g).to(bf16).cuda(), torch.randn(rows, N, generator=g).to(bf16).cuda()
        put("linear_wgrad %dx%dx%d" % (rows, K, N), ops_vit.linear_wgrad(x, dy))
    for B, T, H in [(2, 197, 12), (3, 53, 4)]:
        qkv = torch.randn(B * T, 3 * H * 64, generator=g).to(bf16).cuda()
        o, lse = ops_vit.attention_fwd(qkv, B, T, H)
        put("attention %d %d %d" % (B, T, H), (o, lse, ops_vit.attention_bwd(qkv, o, torch.randn(o.shape, generator=g).to(bf16).cuda(), lse, B, T, H)))
    for P, C, w in [(4096, 256, 64), (131072, 512, 128), (32768, 2048, 512)]:
        a, W = torch.randn(P, w, generator=g).to(bf16).cuda(), (torch.randn(C, w, generator=g) * 0.2).to(bf16).cuda()
        fwd = ops_nn.bnlin_fwd(a, W, (torch.rand(C, generator=g) + 0.5).cuda(), torch.randn(C, generator=g).cuda())
        bwd = ops_nn.bnlin_bwd(torch.randn(P, C, generator=g).to(bf16).cuda(), a, W, fwd)
        put("bnlin %d %d %d" % (P, C, w), [fwd[k] for k in sorted(fwd)] + [bwd[k] for k in sorted(bwd)])
    _conv_bits(put, ops_nn, ops_vit, g)
    for name, net, img in [("resnet", Encoders.ResNet50ReID(seed=2), (32, 3, 256, 128)),
                           ("vit", vit_pytorch.ViTNeckNet(img_size=(224, 224), num_classes=10, seed=3), (16, 3, 224, 224))]:
        net.train()
        emb = net._run_forward(torch.randn(img, generator=g).cuda(), True)
        d = torch.randn(emb.shape, generator=g).cuda()
        for s in range(net.n_bwd_stages if name == "vit" else 4):
            net._backward_stage(d, s)
        put(name + " train step", (emb, net.flat_grads, net.flat_buffers))
        if name == "resnet":
            net.eval()
            put("resnet eval forward", (net._run_forward(torch.randn(img, generator=g).cuda(), False),))
    torch.cuda.synchronize()
    json.dump(res, open(out_json, "w"), indent=0)
    print("%d arrays hashed with %s" % (len(res), os.environ.get("DALIID_LIB", "the tree's library")))


def _ulps(a, b):
    """distance in units of the last place between two arrays of bf16 (held as int16) or fp32 bit patterns"""
    if a.dtype == np.float32:
        a, b = a.view(np.int32), b.view(np.int32)
    top = 1 << (8 * a.dtype.itemsize - 1)
    a, b = a.astype(np.int64), b.astype(np.int64)
    a, b = np.where(a < 0, -(a + top), a), np.where(b < 0, -(b + top), b)          # sign-magnitude -> monotonic
    return np.abs(a - b)


def run_cmp(ja, jb, da, db):
    A, B = json.load(open(ja)), json.load(open(jb))
    diff = [k for k in A if A[k] != B.get(k)] + [k for k in B if k not in A]
    print("%d arrays compared, %d differ" % (len(A), len(diff)))
    for k in diff:
        print("  DIFFERS:", k)
    if da:
        for f in sorted(os.listdir(da)):
            za, zb = np.load(os.path.join(da, f)), np.load(os.path.join(db, f))
            msg = []
            for k in ("draw", "dgamma", "dbeta"):
                u = _ulps(za[k], zb[k])
                msg.append("%s %d of %d differ (max %d ulp)" % (k, int((u > 0).sum()), u.size, int(u.max(initial=0))))
            err = [float((np.abs(z["dgamma"].astype(np.float64) - z["ref_dgamma"]) / z["abs_dgamma"]).max()) for z in (za, zb)]
            msg.append("dgamma error / sum of |terms| against fp64: A %.2e, B %.2e" % tuple(err))
            print("  %s: %s" % (f[:-4], "; ".join(msg)))
    return 1 if diff else 0


def run_time(shape):
    from daliid_amd import ops_nn
    raw, mean, invstd, scale, shift, dp = _pool_inputs(shape, torch.Generator().manual_seed(1))
    _, arg = ops_nn.maxpool_bn_fwd(raw, scale, shift)
    fn = lambda: ops_nn.maxpool_bn_bwd(dp, arg, raw, mean, invstd, scale)
    for _ in range(5):
        fn()
    us = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / 20)
    print("%s maxpool_bn_bwd %dx%dx%dx%d: mean %.1f us, runs %s" % (os.path.basename(os.environ.get("DALIID_LIB", "tree")), *shape, sum(us) / 5,
                                                                   " ".join("%.1f" % u for u in us)))


if __name__ == "__main__":
    mode, a = sys.argv[1], sys.argv[2:]
    if mode == "bits":
        run_bits(a[0], a[1] if len(a) > 1 else None)
    elif mode == "cmp":
        sys.exit(run_cmp(a[0], a[1], a[2] if len(a) > 3 else None, a[3] if len(a) > 3 else None))
    else:
        run_time(tuple(int(v) for v in a) if a else (256, 63, 33, 64))
