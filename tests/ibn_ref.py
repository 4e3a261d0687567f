"""CPU references for the IBN-a encoders (TEST INFRASTRUCTURE ONLY, like oracle/).

* ``IBN`` / ``ibn_trunk``: IBN-Net's ``resnet50_ibn_a`` / ``resnet101_ibn_a`` restated from torch primitives (the package is third-party and
  not available): ``IBN(planes)`` = InstanceNorm2d(affine) on the first ``int(planes * 0.5)`` channels, BatchNorm2d on the rest, as ``bn1`` of
  every bottleneck of the stages whose ``ibn_cfg`` entry is 'a' (('a', 'a', 'a', None): layer1-3); stride on conv2.  Built on
  ``oracle.resnet50_reid.ResNet50ReID`` with those ``bn1`` replaced.  Parity with IBN-Net itself is unpinned at this boundary (as SURVEY 8c
  records for torchvision); what the golden file pins is the reference's own wrapper class over such a trunk.
* ``ResNet50IBNReID`` / ``ResNet101IBNReID``: the wrapper (Encoders.py:462-603) restated: the trunk's modules, the four modules that no
  forward calls, ``last_bn``; forward = trunk without the stem ReLU, avg-pool + max-pool, ``last_bn``.
* ``seeded_state``: deterministic per-key weights (the golden file stores the seeds, not the weights).
* ``forward_matched_eval``: the rounding-matched eval twin, ``oracle.resnet50_bf16.forward_matched``'s eval branch with the IBN block's
  rounding points (resnet_plan.hip): conv1's accumulator -> bf16 (IN half as it is, BN half after the running-statistics affine), instance
  statistics ON the rounded values, affine (x - mean) * (invstd * gamma) + beta and ReLU in fp32, bf16.
"""
import torch
import torch.nn.functional as F
from torch import nn

from oracle import resnet50_bf16 as T
from oracle.resnet50_reid import ResNet50ReID as _PlainNet

IBN_A = ("a", "a", "a", None)


class IBN(nn.Module):
    def __init__(self, planes, ratio=0.5):
        super().__init__()
        self.half = int(planes * ratio)
        self.IN = nn.InstanceNorm2d(self.half, affine=True)
        self.BN = nn.BatchNorm2d(planes - self.half)

    def forward(self, x):
        split = torch.split(x, self.half, 1)
        out1 = self.IN(split[0].contiguous())
        out2 = self.BN(split[1].contiguous())
        return torch.cat((out1, out2), 1)


def ibn_trunk(layers=(3, 4, 6, 3), width=64, ibn_cfg=IBN_A, num_classes=1000):
    """A ResNet-IBN-a trunk: conv1, bn1, relu, maxpool, layer1-4 and the classifier ``fc`` that the ReID wrappers drop."""
    net = _PlainNet(layers=layers, width=width)
    for cfg, layer in zip(ibn_cfg, (net.layer1, net.layer2, net.layer3, net.layer4)):
        if cfg == "a":
            for blk in layer:
                blk.bn1 = IBN(blk.bn1.num_features)
    del net.last_bn
    net.fc = nn.Linear(width * 32, num_classes)
    return net


class ResNet50IBNReID(nn.Module):
    def __init__(self, model_base):
        super().__init__()
        self.conv1 = model_base.conv1
        self.bn1 = model_base.bn1
        self.relu = model_base.relu
        self.maxpool = model_base.maxpool
        self.layer1 = model_base.layer1
        self.layer2 = model_base.layer2
        self.layer3 = model_base.layer3
        self.layer4 = model_base.layer4
        self.layer4[0].conv2.stride = (1, 1)
        self.layer4[0].downsample[0].stride = (1, 1)
        self.global_avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.global_maxpool = nn.AdaptiveMaxPool2d((1, 1))
        self.conv1x1_layer4 = nn.Conv2d(2048, 1, (1, 1), stride=1)
        self.conv1x1_squeeze_layer4 = nn.Conv2d(4096, 1024, (1, 1), stride=1)
        self.conv1x1_expand_layer4 = nn.Conv2d(1024, 2048, (1, 1), stride=1)
        self.attribute_classifier = nn.Linear(2048, 88, bias=True)
        self.last_bn = nn.BatchNorm1d(model_base.layer4[-1].conv3.out_channels)

    def forward(self, x, multipart=False, attention_map=False):
        x = self.maxpool(self.bn1(self.conv1(x)))             # no ReLU after the stem BatchNorm
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        x = self.global_avgpool(x) + self.global_maxpool(x)
        return self.last_bn(x.view(x.size(0), -1))


class ResNet101IBNReID(ResNet50IBNReID):
    pass


def build(layers, width=64, ibn_cfg=IBN_A, wrapper=ResNet50IBNReID):
    return wrapper(ibn_trunk(layers, width, ibn_cfg))


def seeded_state(state_dict, seed):
    """key i of ``state_dict`` from Generator(seed + i): running_var in [0.5, 1.5], running_mean and 1-d biases 0.1 N(0, 1), 1-d weights
    (norm scales) 1 + 0.1 N(0, 1), convolutions N(0, 2 / fan_in), matrices 0.02 N(0, 1); integer entries as they are."""
    sd = {}
    for i, (k, v) in enumerate(state_dict.items()):
        g = torch.Generator().manual_seed(seed + i)
        if not v.dtype.is_floating_point:
            sd[k] = v.clone()
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(v.shape, generator=g)
        elif v.dim() == 1:
            sd[k] = (1.0 if k.endswith("weight") else 0.0) + 0.1 * torch.randn(v.shape, generator=g)
        elif v.dim() == 4:
            sd[k] = torch.randn(v.shape, generator=g) * (2.0 / (v.shape[1] * v.shape[2] * v.shape[3])) ** 0.5
        else:
            sd[k] = 0.02 * torch.randn(v.shape, generator=g)
    return sd


def key_shapes(model):
    return [(k, tuple(v.shape)) for k, v in model.state_dict().items()]


def ibn_stats(raw_in):
    """per (sample, channel) mean and 1 / sqrt(biased variance + 1e-5) of raw_in [N, c, H, W], centred"""
    mean = raw_in.mean((2, 3), keepdim=True)
    var = ((raw_in - mean) ** 2).mean((2, 3), keepdim=True)
    return mean, 1.0 / torch.sqrt(var + 1e-5)


def ibn_act_matched(u1, ibn):
    """a1 of an IBN block from conv1's fp32 result u1 [N, C, H, W]: the plan's rounding points (module docstring)"""
    h = ibn.half
    raw_in = T.Q(u1[:, :h])
    raw_bn = T.Q(T._bn_eval(None, u1[:, h:], ibn.BN))
    mean, invstd = ibn_stats(raw_in)
    y_in = (raw_in - mean) * (invstd * ibn.IN.weight.view(1, -1, 1, 1)) + ibn.IN.bias.view(1, -1, 1, 1)
    return T.Q(F.relu(torch.cat((y_in, raw_bn), 1)))


@torch.no_grad()
def forward_matched_eval(model, x):
    Q = T.Q
    x = Q(x)
    u = T._conv(x, model.conv1)
    x = Q(F.max_pool2d(T._bn_eval(u, Q(u), model.bn1), 3, 2, 1))
    for layer in (model.layer1, model.layer2, model.layer3, model.layer4):
        for blk in layer:
            u1 = T._conv(x, blk.conv1)
            a1 = ibn_act_matched(u1, blk.bn1) if isinstance(blk.bn1, IBN) else Q(F.relu(T._bn_eval(u1, u1, blk.bn1)))
            u2 = T._conv(a1, blk.conv2)
            a2 = Q(F.relu(T._bn_eval(u2, u2, blk.bn2)))
            if T.cat_eval_supported(blk, a2.shape[0] * a2.shape[2] * a2.shape[3]):
                s3, h3 = T._bn_eval_coeffs(blk.bn3)
                sd, hd = T._bn_eval_coeffs(blk.downsample[1])

                def hi_lo(v):
                    hi = v.to(torch.bfloat16).float()
                    return hi + (v - hi).to(torch.bfloat16).float()
                f3 = hi_lo(s3.view(-1, 1, 1, 1) * blk.conv3.weight)
                fd = hi_lo(sd.view(-1, 1, 1, 1) * blk.downsample[0].weight)
                x = Q(F.relu(F.conv2d(a2, f3) + F.conv2d(x, fd) + (h3 + hd).view(1, -1, 1, 1)))
                continue
            u3 = T._conv(a2, blk.conv3)
            out = T._bn_eval(u3, Q(u3) if T.stores_raw3(blk) else u3, blk.bn3)
            if blk.downsample is not None:
                ud = T._conv(x, blk.downsample[0])
                idn = T._bn_eval(ud, Q(ud), blk.downsample[1])
            else:
                idn = x
            x = Q(F.relu(out + idn))
    f = x.mean((2, 3)) + F.adaptive_max_pool2d(x, 1).flatten(1)
    return T._bn_eval(f, f, model.last_bn)
