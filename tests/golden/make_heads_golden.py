#!/usr/bin/env python3
"""Writes tests/golden/heads.npz by RUNNING the reference's own model classes on a stub trunk: ``mainKIT.ResNet50ReID`` for the four
``multipart`` outputs and the ``attention_map``, ``evaluateCleanATModels.ResNet50ReID`` for the gap / gmp / both poolings.

Run where the reference is present (the GPU tests read the .npz only):

    python tests/golden/make_heads_golden.py

Both classes are imported as they are, under ``make_golden.install_shims()``.  ``model_base`` is a stub whose conv1 ... layer3 are identity
modules and whose layer4 is one identity block carrying the ``conv2`` and ``downsample[0]`` attributes the constructors set a stride on, so
that the input IS the layer4 map and only the heads compute.  Only data is written: the map (bf16-representable, stored as its uint16 bits),
randomised ``last_bn`` parameters and running statistics, and the classes' outputs in eval mode (fp32 torch on the CPU)."""
import contextlib
import io
import os

import numpy as np
import torch
from torch import nn

import make_golden  # noqa: F401  (puts the reference on sys.path)

SHAPE = (1, 2048, 16, 8)          # NCHW: the layer4 map of one 256 x 128 image


class _Block(nn.Identity):
    def __init__(self):
        super().__init__()
        self.conv2 = nn.Identity()
        self.downsample = nn.Sequential(nn.Identity())


class _StubBase(nn.Module):
    def __init__(self):
        super().__init__()
        for name in ("conv1", "bn1", "relu", "maxpool", "layer1", "layer2", "layer3"):
            setattr(self, name, nn.Identity())
        self.layer4 = nn.Sequential(_Block())


def main():
    make_golden.install_shims()
    with contextlib.redirect_stdout(io.StringIO()):
        import evaluateCleanATModels as ref_eval
        import mainKIT as ref_main
    g = torch.Generator().manual_seed(20)
    # like a layer4 map: mostly positive with exact zeros, a few channels wholly negative (their maximum is negative), bf16-representable
    x = torch.randn(SHAPE, generator=g).mul(1.5).add(0.5)
    x = torch.where(torch.rand(SHAPE, generator=g) < 0.3, torch.zeros(()), x)
    x[:, :5] = -x[:, :5].abs() - 0.25
    x = x.to(torch.bfloat16)
    C = SHAPE[1]
    bn = dict(weight=torch.rand(C, generator=g) + 0.5, bias=torch.randn(C, generator=g) * 0.3,
              running_mean=torch.randn(C, generator=g) * 0.5 + 1.0, running_var=torch.rand(C, generator=g) * 2 + 0.25)

    def build(cls, **kw):
        net = cls(_StubBase(), **kw).eval()
        with torch.no_grad():
            for k, v in bn.items():
                getattr(net.last_bn, k).copy_(v)
        return net

    z = {"map_bits": x.view(torch.int16).numpy().view(np.uint16)}
    z.update({"last_bn." + k: v.numpy() for k, v in bn.items()})
    z["last_bn.eps"] = np.float64(nn.BatchNorm1d(1).eps)
    xf = x.float()
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        net = build(ref_main.ResNet50ReID)
        for name, out in zip(("upper", "middle", "lower", "whole"), net(xf, multipart=True)):
            z["multipart_" + name] = out.numpy()
        z["heatmap"] = net(xf, attention_map=True).numpy()
        for feature in ("gap", "gmp", "both"):
            z["feature_" + feature] = build(ref_eval.ResNet50ReID, feature=feature)(xf).numpy()
    assert z["heatmap"].shape == SHAPE[2:] and z["multipart_middle"].shape == (1, C)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "heads.npz")
    np.savez_compressed(path, **z)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
