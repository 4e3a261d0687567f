"""What the two plan-backed nets (``Encoders.ResNet50ReID`` on ``dali_resnet_*``, ``vit_pytorch.ViTNeckNet`` on ``dali_vit_*``) share,
written once: the handle of one native plan (``PlanHandle``) and the module that owns the flat storages the plans are bound to
(``PlanNet``).  Nothing here knows an architecture; a subclass builds its plans, presents a tensor of the table as a view, initialises
the parameters and runs its forward.
"""
import ctypes

import torch
from torch import nn

from . import _lib


class PlanHandle:
    """One native plan of ``kind`` "resnet" | "vit" for one fixed input shape: ``dali_<kind>_create`` (``ext`` None) or
    ``dali_<kind>_create_ex``, the sizes and the two tensor tables of ``PlanTable`` (csrc/plan_table.h), destroyed with the object."""

    def __init__(self, kind, device, cfg, ext=None):
        self._prefix = "dali_%s_" % kind
        h, ctx = ctypes.c_void_p(), _lib.ctx(device)
        if ext is None:
            _lib.check(self._fn("create")(ctx, ctypes.byref(cfg), ctypes.byref(h)), self._prefix + "create")
        else:
            _lib.check(self._fn("create_ex")(ctx, ctypes.byref(cfg), ctypes.byref(ext), ctypes.byref(h)), self._prefix + "create_ex")
        self.h = h
        pe, be, ab = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        fd, np_, nb = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self.call("sizes", ctypes.byref(pe), ctypes.byref(be), ctypes.byref(ab), ctypes.byref(fd), ctypes.byref(np_), ctypes.byref(nb))
        self.param_elems, self.buffer_elems, self.arena_bytes = pe.value, be.value, ab.value
        self.feat_dim, self.n_params, self.n_buffers = fd.value, np_.value, nb.value
        # the backward runs per stage (= gradient bucket of the data-parallel reducer), last layers first: the ResNet ABI fixes
        # 0: neck + head + layer4, 1: layer3, 2: layer2, 3: layer1 + stem; the ViT groups its blocks
        self.n_stages = 4 if kind == "resnet" else int(self._fn("num_stages")(h))
        self._backward = "backward" if kind == "resnet" else "backward_stages"

    def _fn(self, name):
        return getattr(_lib.lib(), self._prefix + name)

    def call(self, name, *args):
        """``dali_<kind>_<name>(plan, *args)``, status checked."""
        _lib.check(self._fn(name)(self.h, *args), self._prefix + name)

    def tensor_table(self, kind):
        """[(name, offset, numel, shape)] of the parameters (``kind`` 0) or the buffers (1), offsets in elements of the flat storage."""
        out, name = [], ctypes.create_string_buffer(128)
        off, numel, ndim, shape = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int(), (ctypes.c_int * 4)()
        for i in range(self.n_params if kind == 0 else self.n_buffers):
            self.call("tensor_info", kind, i, name, 128, ctypes.byref(off), ctypes.byref(numel), shape, ctypes.byref(ndim))
            out.append((name.value.decode(), off.value, numel.value, tuple(shape[:ndim.value])))
        return out

    def stage_range(self, stage):
        """[begin, end) of the flat gradient buffer that backward stage ``stage`` completes."""
        b, e = ctypes.c_int64(), ctypes.c_int64()
        self.call("stage_param_range", stage, ctypes.byref(b), ctypes.byref(e))
        return b.value, e.value

    def backward_stage(self, stream, d_out, stage):
        self.call(self._backward, stream, d_out, stage, stage)

    def __del__(self):
        try:
            self._fn("destroy")(self.h)
        except Exception:
            pass


class _PlanFn(torch.autograd.Function):
    """autograd glue: forward = the net's ``_run_forward`` in training mode, backward = one C-ABI call per stage."""

    @staticmethod
    def forward(ctx, x, anchor, net, kwargs):
        ctx.net = net
        return net._run_forward(x, True, **kwargs)

    @staticmethod
    def backward(ctx, d_out):
        ctx.net._run_backward(d_out.contiguous())
        return None, torch.zeros_like(ctx.net._anchor), None, None


class PlanNet(nn.Module):
    """A module whose parameters are views into ONE flat fp32 buffer (``flat_params``), gradients into a second (``flat_grads``), BatchNorm
    running statistics into a third (``flat_buffers``) and ``num_batches_tracked`` counters into one int64 vector (``flat_nbt``): fused
    Adam / EMA and the bucketed all-reduce run on the flat buffers, and every plan of the net is bound to them.

    A subclass supplies ``_make_plan(*shape)`` (a ``PlanHandle``), ``reset_parameters(seed)`` and ``_run_forward(x, training, ...)``, which
    calls ``_activate(plan)`` first and, in training mode, ``_trained(plan)`` last; it may override ``_view`` and ``_before_param``."""

    def __init__(self, device=None):
        super().__init__()
        if device is None and torch.cuda.is_available():
            device = torch.device("cuda", torch.cuda.current_device())
        if device is None:
            raise _lib.DaliError("%s needs a gfx950 GPU; there is no CPU path" % type(self).__name__)
        self._device = torch.device(device)
        self._plans = {}
        self._arena = None
        self._last_plan = None               # the plan bound to the flat buffers and the arena
        self._bwd_plan = None                # the plan of the last training forward
        self._refreshed = (None, -1)         # (plan, flat_params._version) of the last dali_*_refresh_weights

    # ---- construction -----------------------------------------------------------------------------------
    def _register_plan_tensors(self, probe):
        """Allocate the flat storages for the tables of ``probe`` (any plan of this net: the tables do not depend on the input shape) and
        register every entry under its dotted name, in table order: that is the order of ``state_dict()``."""
        dev = self._device
        self.feat_dim, self.n_bwd_stages = probe.feat_dim, probe.n_stages
        self.flat_params = torch.zeros(probe.param_elems, device=dev, dtype=torch.float32)
        self.flat_grads = torch.zeros(probe.param_elems, device=dev, dtype=torch.float32)
        self.flat_buffers = torch.zeros(probe.buffer_elems, device=dev, dtype=torch.float32)
        self._anchor = torch.zeros(1, device=dev, requires_grad=True)
        self._grad_views, self._param_names = {}, []
        for name, off, numel, shape in probe.tensor_table(0):
            self._before_param(name)
            leaf, attr = self._leaf(name)
            leaf.register_parameter(attr, nn.Parameter(self._view(self.flat_params, off, numel, shape)))
            self._grad_views[name] = self._view(self.flat_grads, off, numel, shape)
            self._param_names.append(name)
        buffers = probe.tensor_table(1)
        self.flat_nbt = torch.zeros(sum(1 for t in buffers if t[0].endswith("running_var")), dtype=torch.long, device=dev)
        n_norms = 0
        for name, off, numel, shape in buffers:
            leaf, attr = self._leaf(name)
            leaf.register_buffer(attr, self._view(self.flat_buffers, off, numel, shape))
            if attr == "running_var":
                leaf.register_buffer("num_batches_tracked", self.flat_nbt[n_norms])
                n_norms += 1
        self.register_load_state_dict_post_hook(lambda module, incompatible: module.mark_weights_changed())

    @staticmethod
    def _view(flat, off, numel, shape):
        """The tensor of a table entry as the module presents it: here, the stored order."""
        return flat[off:off + numel].view(*shape)

    def _before_param(self, name):
        """Called before the parameter ``name`` of the table is registered: where a subclass registers modules the plan does not hold, so
        that they take the place they have in the reference's state_dict."""

    def _leaf(self, dotted):
        parts, mod = dotted.split("."), self
        for p in parts[:-1]:
            if p not in mod._modules:
                mod.add_module(p, nn.Module())
            mod = mod._modules[p]
        return mod, parts[-1]

    # ---- state ------------------------------------------------------------------------------------------
    def mark_weights_changed(self):
        # every in-place write through any parameter view (optimizer step, copy_, load_state_dict) bumps the version counter the views
        # share with the flat buffer; kernels that write it behind torch's back call this
        torch.autograd.graph.increment_version(self.flat_params)

    def _apply(self, fn, recurse=True):
        # parameters are views into flat storages owned by this module: device / dtype moves are not supported
        probe = fn(torch.zeros(1, device=self._device))
        if probe.device != self._device or probe.dtype != torch.float32:
            raise _lib.DaliError("%s lives on %s in fp32 storage; .to()/.half()/.cpu() are not supported" % (type(self).__name__, self._device))
        return self

    # ---- plans ------------------------------------------------------------------------------------------
    def _plan(self, *shape):
        p = self._plans.get(shape)
        if p is None:
            p = self._plans[shape] = self._make_plan(*shape)
        return p

    def _activate(self, plan):
        """Make ``plan`` the one that runs next: grow the arena to hold it, bind it when another plan ran last, and re-cast the weights
        when this plan has not seen the current ``flat_params`` (another plan refreshed last, or the version moved)."""
        if self._arena is None or self._arena.numel() < plan.arena_bytes:
            self._arena = None
            torch.cuda.synchronize(self._device)
            self._arena = torch.empty(plan.arena_bytes + 256, device=self._device, dtype=torch.uint8)
            self._refreshed = (None, -1)
        if self._last_plan is not plan:
            plan.call("bind", _lib.ptr(self.flat_params), _lib.ptr(self.flat_grads), _lib.ptr(self.flat_buffers), _lib.ptr(self._arena),
                      self._arena.numel())
            self._last_plan = plan
        version = self.flat_params._version
        if self._refreshed[0] is not plan or self._refreshed[1] != version:
            plan.call("refresh_weights", _lib.stream_ptr())
            self._refreshed = (plan, version)

    def _trained(self, plan):
        """After a training forward of ``plan``: the BatchNorm counters move, and the backward belongs to this plan."""
        self.flat_nbt += 1
        self._bwd_plan = plan

    # ---- backward ---------------------------------------------------------------------------------------
    def _forward_with_grad(self, x, **kwargs):
        """A training ``_run_forward(x, True, **kwargs)`` that autograd can differentiate (``.backward()`` fills ``flat_grads``)."""
        return _PlanFn.apply(x, self._anchor, self, kwargs)

    def _backward_stage(self, d_out, stage):
        plan = self._bwd_plan
        if plan is not self._last_plan:
            raise _lib.DaliError("backward() after another forward of a different shape is not supported")
        plan.backward_stage(_lib.stream_ptr(), _lib.ptr(d_out, torch.float32, "d_out"), stage)

    def _run_backward(self, d_out):
        for stage in range(self.n_bwd_stages):
            self._backward_stage(d_out, stage)
        self.attach_grads()

    def attach_grads(self):
        """Point the .grad of every parameter of the plan at its view of the flat gradient buffer (torch optimizers read .grad); None where
        ``requires_grad`` is off.  Paired by name: a parameter outside the plan is left alone."""
        for name in self._param_names:
            p = self.get_parameter(name)
            p.grad = self._grad_views[name] if p.requires_grad else None
