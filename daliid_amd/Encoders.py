"""Mirror of the reference's ``Encoders.py`` for the paths in scope: ``getDCNN("resnet50")`` with ``ResNet50ReID`` (Encoders.py:25-48,
306-351) and, eval only, ``getDCNN("resnet50IBN" | "resnet101IBN")`` with ``ResNet50IBNReID`` / ``ResNet101IBNReID`` (:462-603),
backed by the native HIP net plan (``dali_resnet_*`` in
include/daliid.h) instead of torchvision + cuDNN.

What is kept from the reference surface
  * ``getDCNN(gpu_indexes, model_name, embedding_size=None) -> (model_online, model_momentum)``; both come back
    wrapped (``.module`` attribute, ``module.``-prefixed state_dict keys like ``nn.DataParallel``), momentum
    initialised from online, both in eval mode (Encoders.py:39-48).
  * ``ResNet50ReID``: callable ``x[B,3,H,W] fp32 -> [B,2048] fp32``; ``.train()/.eval()``; ``.parameters()``;
    ``state_dict()/load_state_dict()`` with torchvision key names (``conv1.weight`` ... ``last_bn.bias``).
What differs by design
  * storage: all parameters are views into ONE flat fp32 buffer (conv weights in channels_last / OHWI storage),
    gradients into one flat fp32 buffer, BN running stats into a third: fused Adam/EMA and bucketed RCCL
    all-reduce run on the flat buffers.
  * ``torchvision.models.resnet50(pretrained=True)`` (Encoders.py:33,36) needs a network fetch; here the weights are
    torchvision's random init (kaiming fan_out) unless a state_dict is loaded.
  * one process drives ONE GPU (data parallelism = one process per GPU + RCCL), so ``gpu_indexes`` only selects
    the device of this process.
"""
import ctypes

import torch
from torch import nn

from . import _lib, ops_nn
from .plan_net import PlanHandle, PlanNet


class _Cfg(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int), ("height", ctypes.c_int), ("width", ctypes.c_int),
                ("layers", ctypes.c_int * 4), ("width_base", ctypes.c_int)]


class _Ext(ctypes.Structure):
    """dali_resnet_ext (include/daliid.h): the stages whose bottlenecks are IBN-a blocks."""
    _fields_ = [("ibn", ctypes.c_int * 4)]


def _Plan(device, batch, height, width, layers, width_base, ibn=None):
    """One dali_resnet plan for a fixed (batch, H, W).  ``ibn`` given: dali_resnet_create_ex (all zero is dali_resnet_create's plan)."""
    cfg = _Cfg(batch, height, width, (ctypes.c_int * 4)(*layers), width_base)
    ext = None if ibn is None else _Ext((ctypes.c_int * 4)(*[int(bool(v)) for v in ibn]))
    return PlanHandle("resnet", device, cfg, ext)


_FEATURE_MODES = {"both": 0, "gap": 1, "gmp": 2}        # dali_feature in include/daliid.h


def default_parts(map_rows):
    """Row ranges (upper, middle, lower) of a ``map_rows``-row layer4 map: ``((0, R//2), (R//4, R//4 + R//2), (R//2, R))``.  At the
    reference's 16-row map (256-row images) these are exactly its slices ``:8``, ``4:12`` and ``8:`` (mainKIT.py:252-254).  The reference
    hard-codes those three slices whatever the image height; the proportional split for other heights is this project's choice."""
    R = int(map_rows)
    if R < 2:
        raise _lib.DaliError("default_parts: a map of %d row(s) has no upper / middle / lower parts (at least 2 rows)" % R)
    return (0, R // 2), (R // 4, R // 4 + R // 2), (R // 2, R)


class ResNet50ReID(PlanNet):
    """Encoders.ResNet50ReID (Encoders.py:306-351) on the HIP net plan."""

    _ibn = None                              # dali_resnet_ext.ibn of this class' plans (None: dali_resnet_create)
    _own_prefixes = ("last_bn.",)           # what a trunk handed in as model_base does not carry

    def __init__(self, model_base=None, layers=(3, 4, 6, 3), width=64, device=None, seed=None):
        super().__init__(device)
        self._layers, self._width = tuple(layers), int(width)
        self.feature = "both"               # head pooling: "both" | "gap" | "gmp" (evaluateCleanATModels.py:249-256, :335-340)
        self._register_plan_tensors(self._plan(1, 32, 32))
        self.reset_parameters(seed)
        if model_base is not None:
            self._load_base(model_base.state_dict() if isinstance(model_base, nn.Module) else model_base)

    def _make_plan(self, batch, height, width):
        return _Plan(self._device, batch, height, width, self._layers, self._width, self._ibn)

    def _load_base(self, sd):
        """``ResNet50ReID(model_base)`` as the reference calls it (Encoders.py:33-37, 306-328): model_base is a torchvision ``resnet50``,
        whose trunk (conv1 ... layer4) is taken over; its classifier ``fc.*`` is dropped (Encoders.py:312-328 never copies it) and
        ``last_bn`` is this module's own fresh BatchNorm1d (Encoders.py:350).  A state_dict of this class (with ``last_bn.*``) loads whole.
        Anything else missing or unexpected is an error, as in a strict load."""
        sd = {k: v for k, v in sd.items() if not k.startswith("fc.")}
        res = self.load_state_dict(sd, strict=False)
        missing = [k for k in res.missing_keys if not k.startswith(self._own_prefixes)]
        if missing or res.unexpected_keys:
            raise _lib.DaliError("%s(model_base): model_base is not a trunk of this architecture (missing %s, unexpected %s)"
                                 % (type(self).__name__, missing[:4], list(res.unexpected_keys)[:4]))

    @staticmethod
    def _view(flat, off, numel, shape):
        v = flat[off:off + numel]
        if len(shape) == 4:                       # a conv weight: logical OIHW over OHWI storage (channels_last)
            o, i, r, s = shape
            return v.view(o, r, s, i).permute(0, 3, 1, 2)
        return v.view(*shape)

    def reset_parameters(self, seed=None):
        """torchvision's ResNet init: conv kaiming_normal_(fan_out, relu); BN weight 1 / bias 0; stats 0 / 1."""
        gen = torch.Generator(device="cpu")
        gen.manual_seed(int(seed) if seed is not None else int(torch.initial_seed()) & 0x7fffffff)
        params = dict(self.named_parameters())
        with torch.no_grad():
            for name in self._param_names:               # the plan's tensors, in table order
                p = params[name]
                if p.dim() == 4:
                    o, i, r, s = p.shape
                    std = (2.0 / (o * r * s)) ** 0.5
                    p.copy_((torch.randn(o, i, r, s, generator=gen) * std).to(p.device))
                elif name.endswith(".weight"):
                    p.fill_(1.0)
                else:
                    p.zero_()
            for name, b in self.named_buffers():
                if name.endswith("running_var"):
                    b.fill_(1.0)
                else:
                    b.zero_()
        self.mark_weights_changed()

    def _run_forward(self, x, training):
        if x.dim() != 4 or x.shape[1] != 3:
            raise _lib.DaliError("expected images [B,3,H,W], got %s" % (tuple(x.shape),))
        x = x.to(device=self._device, dtype=torch.float32).contiguous()
        plan = self._plan(x.shape[0], x.shape[2], x.shape[3])
        self._activate(plan)
        emb = torch.empty(x.shape[0], plan.feat_dim, device=self._device, dtype=torch.float32)
        if self.feature not in _FEATURE_MODES:
            raise _lib.DaliError("feature must be 'both', 'gap' or 'gmp' (got %r)" % (self.feature,))
        plan.call("set_feature", _FEATURE_MODES[self.feature])
        plan.call("forward", _lib.stream_ptr(), _lib.ptr(x), int(training), _lib.ptr(emb))
        if training:
            self._trained(plan)
        return emb

    def _eval_only(self, what):
        if self.training:
            raise _lib.DaliError("%s is an inference output (running statistics); call .eval() first" % what)

    def head_map(self, height, width, batch=1):
        """(rows, columns) of the layer4 map for images of height x width: what the row ranges of ``forward_heads`` count."""
        h, w = ctypes.c_int(), ctypes.c_int()
        self._plan(batch, height, width).call("head_map", ctypes.byref(h), ctypes.byref(w))
        return h.value, w.value

    def forward_heads(self, x, heads, heatmap=False):
        """Several heads from ONE trunk pass (dali_resnet_forward_heads), eval mode only, no autograd graph.
        ``heads``: sequence of ``(mode_name, rows)``, mode_name "both" | "gap" | "gmp", rows ``None`` (the whole map) or ``(row_begin, row_end)``
        of the layer4 map (``head_map`` / ``default_parts``).  -> ``[n_heads, B, feat_dim]`` fp32, every head through ``last_bn``; with
        ``heatmap=True`` also the channel-sum activation map ``[B, Hm, Wm]``.  A whole-map head equals ``forward`` under
        ``feature = mode_name`` bit for bit.  ``self.feature`` is neither read nor changed."""
        self._eval_only("forward_heads")
        if x.dim() != 4 or x.shape[1] != 3:
            raise _lib.DaliError("expected images [B,3,H,W], got %s" % (tuple(x.shape),))
        specs, nh = ops_nn.head_specs(heads)
        with torch.no_grad():
            x = x.to(device=self._device, dtype=torch.float32).contiguous()
            plan = self._plan(x.shape[0], x.shape[2], x.shape[3])
            self._activate(plan)
            emb = torch.empty(nh, x.shape[0], plan.feat_dim, device=self._device, dtype=torch.float32)
            heat = torch.empty((x.shape[0],) + self.head_map(x.shape[2], x.shape[3], x.shape[0]), device=self._device,
                               dtype=torch.float32) if heatmap else None
            plan.call("forward_heads", _lib.stream_ptr(), _lib.ptr(x), specs, nh, _lib.ptr(emb), _lib.ptr(heat))
        return (emb, heat) if heatmap else emb

    def debug_tensor(self, name, dtype, shape):
        ptr, nbytes = ctypes.c_void_p(), ctypes.c_int64()
        self._last_plan.call("debug_tensor", name.encode(), ctypes.byref(ptr), ctypes.byref(nbytes))
        off = ptr.value - self._arena.data_ptr()
        return self._arena[off:off + nbytes.value].view(dtype).view(*shape).clone()

    # ---- nn.Module protocol -----------------------------------------------------------------------------
    def forward(self, x, multipart=False, attention_map=False):
        """``multipart``: (upper, middle, lower, whole), each max-pooled over its rows (``default_parts``) and passed through ``last_bn``, whatever
        ``self.feature`` says (mainKIT.py:251-292).  ``attention_map``: the channel-sum map [Hm, Wm] of image 0 (mainKIT.py:294-298).  Both are
        eval-only; with both set, the parts are returned, as in the reference."""
        if multipart:
            self._eval_only("forward(multipart=True)")
            parts = default_parts(self.head_map(x.shape[2], x.shape[3], x.shape[0])[0])
            return tuple(self.forward_heads(x, [("gmp", rows) for rows in parts] + [("gmp", None)]))
        if attention_map:
            self._eval_only("forward(attention_map=True)")
            return self.forward_heads(x, [("gmp", None)], heatmap=True)[1][0]
        if self.training and torch.is_grad_enabled():
            return self._forward_with_grad(x)
        return self._run_forward(x, training=self.training)


class ResNet50IBNReID(ResNet50ReID):
    """Encoders.ResNet50IBNReID (Encoders.py:462-531) over IBN-Net's ``resnet50_ibn_a``: the bottlenecks of layer1-3 carry ``bn1 = IBN(planes)``,
    InstanceNorm2d (affine, per-sample statistics in eval mode too) on the first half of the channels and BatchNorm2d on the rest; layer4 is
    plain.  State-dict keys, order and shapes are the reference's, the four modules it builds and never calls included
    (``conv1x1_layer4``, ``conv1x1_squeeze_layer4``, ``conv1x1_expand_layer4``, ``attribute_classifier``: plain parameters outside the plan,
    ``grad`` None).

    EVAL ONLY: the plan has no half-channel batch statistics and no instance-norm backward, so a forward in train mode raises
    ``NotImplementedError``; call ``.eval()``.  ``model_base``: an IBN-a trunk (Module or state_dict), ``fc.*`` dropped."""

    _ibn = (1, 1, 1, 0)
    _own_prefixes = ("last_bn.", "conv1x1_layer4.", "conv1x1_squeeze_layer4.", "conv1x1_expand_layer4.", "attribute_classifier.")

    def __init__(self, model_base=None, layers=(3, 4, 6, 3), width=64, device=None, seed=None):
        super().__init__(model_base, layers, width, device, seed)

    def _before_param(self, name):
        """The modules of the reference class that sit between ``layer4`` and ``last_bn`` in its state_dict and that no forward runs."""
        if name != "last_bn.weight":
            return
        # literal shapes, as in the reference (Encoders.py:483-487), whatever `width` is
        dev = self._device
        self.conv1x1_layer4 = nn.Conv2d(2048, 1, (1, 1), stride=1, device=dev)
        self.conv1x1_squeeze_layer4 = nn.Conv2d(4096, 1024, (1, 1), stride=1, device=dev)
        self.conv1x1_expand_layer4 = nn.Conv2d(1024, 2048, (1, 1), stride=1, device=dev)
        self.attribute_classifier = nn.Linear(2048, 88, bias=True, device=dev)

    def reset_parameters(self, seed=None):
        """The plan's tensors as ResNet50ReID (``IN.weight`` 1, ``IN.bias`` 0); the unused modules uniform in +-1/sqrt(fan_in), from the seed."""
        super().reset_parameters(seed)
        gen = torch.Generator(device="cpu")
        gen.manual_seed((int(seed) if seed is not None else int(torch.initial_seed())) + 1 & 0x7fffffff)
        with torch.no_grad():
            for prefix in self._own_prefixes[1:]:
                mod = getattr(self, prefix[:-1])
                bound = (mod.weight[0].numel()) ** -0.5
                for p in (mod.weight, mod.bias):
                    p.copy_(((torch.rand(p.shape, generator=gen) * 2 - 1) * bound).to(p.device))

    def attach_grads(self):
        raise NotImplementedError("%s is eval only (IBN-a blocks have no backward here): there are no gradients to attach; call .eval()" % type(self).__name__)

    def forward(self, x, multipart=False, attention_map=False):
        """-> [B, 2048].  ``multipart`` and ``attention_map`` are accepted and IGNORED, as the reference's IBN classes ignore them
        (Encoders.py:492-515); body parts, the three poolings and the heat map come from ``forward_heads``."""
        if self.training:
            raise NotImplementedError("%s is eval only: training an IBN-a net needs half-channel batch statistics and an instance-norm backward, "
                                      "which the plan does not have; call .eval()" % type(self).__name__)
        return self._run_forward(x, training=False)


class ResNet101IBNReID(ResNet50IBNReID):
    """Encoders.ResNet101IBNReID (Encoders.py:534-603) over ``resnet101_ibn_a``: ResNet50IBNReID at depth (3, 4, 23, 3)."""

    def __init__(self, model_base=None, layers=(3, 4, 23, 3), width=64, device=None, seed=None):
        super().__init__(model_base, layers, width, device, seed)


class _DataParallelShim(nn.Module):
    """Keeps the reference's ``nn.DataParallel`` object protocol (``.module``, ``module.``-prefixed keys) for a
    one-GPU-per-process design."""

    def __init__(self, module):
        super().__init__()
        self.module = module

    def forward(self, *a, **k):
        return self.module(*a, **k)

    def cuda(self, device=None):
        return self


def getEnsembles(gpu_indexes):
    """Encoders.getEnsembles (Encoders.py:245-303) builds ResNet-50 + OSNet + DenseNet-121 pairs; OSNet and DenseNet are outside the
    scope table.  The name exists so that ``from Encoders import getDCNN, getEnsembles`` (mainKIT.py:27,
    train_encodersKIT.py:25, evaluateCleanATModels.py:13) keeps importing; mainKIT.main never calls it."""
    raise NotImplementedError("getEnsembles: the OSNet / DenseNet-121 ensemble members are out of scope of this build (SURVEY.md 2.1); "
                              "use getDCNN(gpu_indexes, 'resnet50')")


def getDCNN(gpu_indexes, model_name, embedding_size=None):
    """Encoders.getDCNN (Encoders.py:25-48, 241): -> (model_online, model_momentum), both eval()."""
    nets = {"resnet50": ResNet50ReID, "resnet50IBN": ResNet50IBNReID, "resnet101IBN": ResNet101IBNReID}      # (the IBN-a pairs are eval only)
    if model_name not in nets:
        raise NotImplementedError("getDCNN: model_name must be one of %s in this build (got %r)" % (sorted(nets), model_name))
    if embedding_size not in (None, 2048):
        raise NotImplementedError("getDCNN: embedding_size is fixed at 2048 for %s" % model_name)
    dev = torch.device("cuda", gpu_indexes[0] if len(gpu_indexes) else 0)
    model_source = _DataParallelShim(nets[model_name](device=dev))
    model_momentum = _DataParallelShim(nets[model_name](device=dev))
    model_momentum.load_state_dict(model_source.state_dict())
    return model_source.eval(), model_momentum.eval()
