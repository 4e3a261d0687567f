"""Mirror of the reference's ``vit_pytorch.py`` for the path in scope: the ``TransReID`` encoder
(vit_pytorch.py:291-408) and its factories ``vit_base_`` / ``vit_small_`` / ``deit_small_patch16_224_TransReID`` (:453-476), on the native HIP ViT plan
(``dali_vit_*``).  ``make_models.build_transformer`` (the BN-neck wrapper the reference actually instantiates,
make_models.py:121-205) is the module that owns the plan; ``TransReID`` here is the same plan exposed at the pre-neck
feature so the reference's key names (``cls_token``, ``pos_embed``, ``patch_embed.proj.*``, ``blocks.N.*``, ``norm.*``,
``fc.*``) and call signature ``forward(x, cam_label=None, view_label=None)`` are kept.

Supported: drop / attn_drop = 0; SIE camera / view embeddings (vit_pytorch.py:316-331, 382-387: ``sie_embed`` added to every token as
``sie_xishu * sie_embed[index]``, trained through ``dali_vit_sie_grad``); ``local_feature=True`` (:393-396: ``blocks[:-1]``, all tokens, no
final norm; eval mode only).  ``make_models.build_transformer_local`` puts the JPM head on the same plan.  Geometries up to 1024 tokens
(384x128 at stride 12 = 311, 256x256 at stride 16 = 257, 384x384 at stride 16 = 577); past 256 tokens a model is eval only, its train-mode
forward raises.  Head widths 64 and 96: ``qkv_bias=False`` and a set ``qk_scale`` (vit_pytorch.py:145-147) work at both; at head_dim 96 (ViT-Small:
dim 768, 8 heads) only the attention forward exists, so such a model is eval only as well.  ``resize_pos_embed`` / ``TransReID.load_param`` (vit_pytorch.py:410-450) bring a checkpoint of another size in.  DropPath (vit_pytorch.py:45-62; per-block rate
``linspace(0, drop_path_rate, depth)``, :338) is applied in training mode: one uniform draw per (branch, sample) on the
device per step, scale = floor(keep + u) / keep; ``drop_path_uniform`` can be set to inject the draws (parity tests hand
the same ones to the oracle).  In eval mode it is the identity, as in the reference.
"""
import ctypes
import math

import numpy as np
import torch
from torch import nn

from . import _lib
from .plan_net import PlanHandle, PlanNet


TRAIN_MAX_TOKENS = 256      # the attention backward's limit; the forward alone (eval mode) runs up to 1024 tokens
TRAIN_HEAD_DIM = 64         # the attention backward's head width; the forward alone also runs at 96


class _VitCfg(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("batch", "height", "width", "patch", "stride", "dim", "depth", "heads", "mlp_hidden", "num_classes")]


class _VitExt(ctypes.Structure):
    _fields_ = [("n_sie", ctypes.c_int), ("sie_coef", ctypes.c_float), ("local_feature", ctypes.c_int), ("jpm", ctypes.c_int),
                ("divide", ctypes.c_int), ("token_map", ctypes.c_void_p), ("neck_after", ctypes.c_int), ("id_classes", ctypes.c_int),
                ("no_qkv_bias", ctypes.c_int), ("qk_scale", ctypes.c_float)]


def _VitPlan(device, cfg_tuple, ext=None):
    """One dali_vit plan for a fixed batch, always through dali_vit_create_ex (nothing set is dali_vit_create's plan).  ``ext``: a dict of
    dali_vit_ext's fields; ``token_map`` is int32 [divide, L] on the host, the plan copies it during the call."""
    ext = dict(ext or {})
    token_map = ext.pop("token_map", None)
    if token_map is not None:
        token_map = np.ascontiguousarray(token_map, dtype=np.int32)
        ext["divide"], ext["token_map"] = token_map.shape[0], token_map.ctypes.data
    return PlanHandle("vit", device, _VitCfg(*cfg_tuple), _VitExt(**ext))


class ViTNeckNet(PlanNet):
    """TransReID encoder + BatchNorm1d neck on the HIP plan; state_dict keys as make_models.build_transformer
    (``base.*``, ``bottleneck.*``).  ``camera`` / ``view`` > 1 add the SIE parameter ``base.sie_embed`` (vit_pytorch.py:316-331);
    ``jpm`` (a dict of dali_vit_ext's JPM fields: ``token_map``, ``neck_after``, ``id_classes``; set by make_models.build_transformer_local) adds ``b1.*``, ``b2.*``, ``classifier*`` and
    ``bottleneck_1..4`` and makes the output [B, 5 * embed_dim].  ``qkv_bias=False`` drops every ``attn.qkv.bias``; ``qk_scale`` replaces the attention
    scale ``head_dim ** -0.5`` (vit_pytorch.py:145-147).  ``embed_dim // num_heads`` is 64 or 96; a 96-wide model is eval only."""

    def __init__(self, img_size=(224, 224), patch_size=16, stride_size=16, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4.0,
                 num_classes=1000, drop_path_rate=0.0, device=None, seed=None, camera=0, view=0, sie_xishu=1.0, local_feature=False, jpm=None,
                 qkv_bias=True, qk_scale=None):
        super().__init__(device)
        self.cam_num, self.view_num, self.sie_xishu = int(camera), int(view), float(sie_xishu)
        # vit_pytorch.py:317-331: one row per (camera, view) pair, per camera, or per view
        n_sie = camera * view if camera > 1 and view > 1 else camera if camera > 1 else view if view > 1 else 0
        self.local_feature = bool(local_feature or jpm)
        self._ext = dict(n_sie=int(n_sie), sie_coef=float(sie_xishu), local_feature=int(self.local_feature),
                         no_qkv_bias=int(not qkv_bias), qk_scale=float(qk_scale or 0.0))          # `qk_scale or`, as vit_pytorch.py:145
        self.head_dim = embed_dim // max(int(num_heads), 1)
        if jpm:
            self._ext.update(jpm=1, **jpm)
        self._sie_idx = None
        self.img_size = (img_size, img_size) if isinstance(img_size, int) else tuple(img_size)
        self._geom = (patch_size, stride_size, embed_dim, depth, num_heads, int(embed_dim * mlp_ratio), num_classes)
        self.drop_path_rate = float(drop_path_rate)
        self.drop_path_uniform = None            # optional [2*depth, B] uniform draws in [0,1) used instead of torch.rand (tests)
        self._dp_scales = None
        self.in_planes = embed_dim
        self._register_plan_tensors(self._plan(1))            # every tensor in its stored order, the 4-D patch projection included
        for name, p in self.named_parameters():
            if name.startswith("bottleneck") and name.endswith(".bias"):
                p.requires_grad_(False)                                              # make_models.py:181, :290-304
        # base.fc is built but never called (vit_pytorch.py:405-408 returns the cls feature): its grad stays None in the
        # reference, so torch.optim.Adam skips it (no weight decay either)
        self._no_grad_params = ("base.fc.weight", "base.fc.bias")
        self.reset_parameters(seed)

    def _make_plan(self, batch):
        ps, st, dim, depth, heads, hidden, ncls = self._geom
        return _VitPlan(self._device, (batch, self.img_size[0], self.img_size[1], ps, st, dim, depth, heads, hidden, ncls), self._ext)

    def reset_parameters(self, seed=None):
        """vit_pytorch.py:350-361 + PatchEmbed_overlap init (:268-271) + weights_init_kaiming on the neck (make_models.py:182)."""
        gen = torch.Generator().manual_seed(int(seed) if seed is not None else int(torch.initial_seed()) & 0x7fffffff)
        tn = lambda shape, std: torch.nn.init.trunc_normal_(torch.empty(shape), std=std, a=-2.0, b=2.0, generator=gen)
        with torch.no_grad():
            for name, p in self.named_parameters():
                if name.endswith("cls_token") or name.endswith("pos_embed") or name.endswith("sie_embed"):
                    p.copy_(tn(p.shape, 0.02).to(p.device))
                elif "patch_embed.proj.weight" in name:
                    n = p.shape[2] * p.shape[3] * p.shape[0]
                    p.copy_((torch.randn(p.shape, generator=gen) * math.sqrt(2.0 / n)).to(p.device))
                elif name.startswith("classifier"):
                    p.copy_((torch.randn(p.shape, generator=gen) * 0.001).to(p.device))       # weights_init_classifier, make_models.py:42-47
                elif name.endswith(".weight") and p.dim() == 2:
                    p.copy_(tn(p.shape, 0.02).to(p.device))
                elif name.endswith(".weight"):
                    p.fill_(1.0)                       # LayerNorm / BatchNorm weights
                else:
                    p.zero_()                          # every bias
            self._copy_jpm_branches()
            self.flat_buffers.zero_()
            for name, b in self.named_buffers():
                if name.endswith("running_var"):
                    b.fill_(1.0)
        self.mark_weights_changed()

    def _copy_jpm_branches(self):
        """make_models.py:249-258: b1 and b2 start as deep copies of the last block and the final norm (of the pretrained base, when one was loaded)"""
        if not self._ext.get("jpm"):
            return
        with torch.no_grad():
            sd = self.state_dict()
            last = "base.blocks.%d." % (self._geom[3] - 1)
            for name in self._param_names:
                if name.startswith(("b1.0.", "b2.0.")):
                    sd[name].copy_(sd[last + name[5:]])
                elif name.startswith(("b1.1.", "b2.1.")):
                    sd[name].copy_(sd["base.norm." + name[5:]])
        self.mark_weights_changed()

    def sie_index(self, cam_label, view_label, batch):
        """vit_pytorch.py:382-389: the row of ``sie_embed`` per sample, ``cam * view_num + view``, ``cam`` or ``view``, validated on the host
        -> int32 [batch] on the device (None for a model without SIE).  Labels: an int, a numpy array or a tensor of length ``batch``."""
        if self._ext["n_sie"] == 0:
            return None

        def host(lab, n, what):
            if lab is None:
                raise _lib.DaliError("this model has SIE %s embeddings: forward() needs %s_label" % (what, what if what == "view" else "cam"))
            a = lab.detach().cpu().numpy() if isinstance(lab, torch.Tensor) else np.asarray(lab)
            a = np.broadcast_to(a.reshape(-1), (batch,)) if a.size == 1 else a.reshape(-1)
            if a.shape != (batch,) or a.dtype.kind not in "iu":
                raise _lib.DaliError("%s labels must be %d integers" % (what, batch))
            if a.min() < 0 or a.max() >= n:
                raise _lib.DaliError("%s label out of range [0, %d)" % (what, n))
            return a.astype(np.int64)
        if self.cam_num > 1 and self.view_num > 1:
            idx = host(cam_label, self.cam_num, "camera") * self.view_num + host(view_label, self.view_num, "view")
        elif self.cam_num > 1:
            idx = host(cam_label, self.cam_num, "camera")
        else:
            idx = host(view_label, self.view_num, "view")
        return torch.from_numpy(idx.astype(np.int32)).to(self._device)

    def _run_forward(self, x, training, want_global=False, sie_idx=None, want_tokens=False):
        if x.dim() != 4 or tuple(x.shape[1:]) != (3,) + self.img_size:
            raise _lib.DaliError("Input image size (%s) doesn't match model (%s)" % (tuple(x.shape[2:]), self.img_size))   # vit_pytorch.py:282-284
        x = x.to(device=self._device, dtype=torch.float32).contiguous()
        plan = self._plan(x.shape[0])
        self._activate(plan)
        self._dp_scales = self._draw_drop_path(x.shape[0]) if training else None
        plan.call("set_drop_path", _lib.ptr(self._dp_scales))
        if self._ext["n_sie"] and sie_idx is None:
            raise _lib.DaliError("this model has SIE embeddings: forward() needs cam_label / view_label")
        if training:
            self._sie_idx = sie_idx                  # the backward's sie_grad reads it
        if want_tokens:
            tokens = torch.empty(x.shape[0], self.base.pos_embed.shape[1], self.in_planes, device=self._device)
            plan.call("forward_ex", _lib.stream_ptr(), _lib.ptr(x), _lib.ptr(sie_idx), 0, None, None, _lib.ptr(tokens))
            return tokens
        feat = torch.empty(x.shape[0], plan.feat_dim, device=self._device)
        gf = torch.empty(x.shape[0], self.in_planes, device=self._device) if want_global else None
        plan.call("forward_ex", _lib.stream_ptr(), _lib.ptr(x), _lib.ptr(sie_idx), int(training), _lib.ptr(feat), _lib.ptr(gf), None)
        if training:
            self._trained(plan)
        return (feat, gf) if want_global else feat

    def _draw_drop_path(self, batch):
        """vit_pytorch.py:45-62 for every residual branch of every block at once: fp32 [2*depth, batch] of floor(keep + u)/keep,
        keep = 1 - linspace(0, rate, depth)[block]; blocks whose rate is 0 are nn.Identity in the reference (:171)."""
        if self.drop_path_rate <= 0:
            return None
        depth = self._geom[3]
        dpr = torch.linspace(0, self.drop_path_rate, depth).repeat_interleave(2).to(self._device).unsqueeze(1)      # :338
        u = self.drop_path_uniform
        if u is None:
            u = torch.rand(2 * depth, batch, device=self._device)
        elif tuple(u.shape) != (2 * depth, batch):
            raise _lib.DaliError("drop_path_uniform must be [2*depth, batch] = %s" % ((2 * depth, batch),))
        keep = 1.0 - dpr
        return ((keep + u.to(self._device, torch.float32)).floor() / keep).contiguous()

    @property
    def num_tokens(self):
        return int(self.base.pos_embed.shape[1])

    def forward(self, x, label=None, cam_label=None, view_label=None):
        """make_models.py:184-205: returns the post-neck ``feat``."""
        self._refuse_tokens_only("forward()")
        idx = self.sie_index(cam_label, view_label, x.shape[0])
        if self.training and torch.is_grad_enabled():
            if self.num_tokens > TRAIN_MAX_TOKENS:
                # past 256 tokens only the attention forward exists (the plan holds none of the backward's buffers)
                raise _lib.DaliError("training needs at most %d tokens (this model has %d): it is eval mode only -- call .eval() and run under "
                                     "torch.no_grad()" % (TRAIN_MAX_TOKENS, self.num_tokens))
            if self.head_dim != TRAIN_HEAD_DIM:
                # at head_dim 96 only the attention forward exists (the plan holds none of the backward's buffers)
                raise _lib.DaliError("training needs head_dim %d (this model has %d): it is eval mode only -- call .eval() and run under "
                                     "torch.no_grad()" % (TRAIN_HEAD_DIM, self.head_dim))
            return self._forward_with_grad(x, sie_idx=idx)
        return self._run_forward(x, self.training, sie_idx=idx)

    def global_feat(self, x, cam_label=None, view_label=None):
        """The pre-neck cls feature = ``TransReID.forward`` (vit_pytorch.py:405-408); eval-mode helper."""
        self._refuse_tokens_only("global_feat()")
        return self._run_forward(x, False, want_global=True, sie_idx=self.sie_index(cam_label, view_label, x.shape[0]))[1]

    def _refuse_tokens_only(self, what):
        if self.local_feature and not self._ext.get("jpm"):
            raise _lib.DaliError("%s: a local_feature model without the JPM head has no cls feature and no neck output "
                                 "(vit_pytorch.py:393-396 returns the tokens); call local_tokens()" % what)

    def local_tokens(self, x, cam_label=None, view_label=None):
        """``TransReID.forward`` with local_feature=True (vit_pytorch.py:393-396): the tokens after ``blocks[:-1]``, fp32 [B, T, C]; eval only."""
        if not self.local_feature:
            raise _lib.DaliError("local_tokens() needs a model built with local_feature=True")
        return self._run_forward(x, False, sie_idx=self.sie_index(cam_label, view_label, x.shape[0]), want_tokens=True)


class TransReID(nn.Module):
    """vit_pytorch.TransReID (vit_pytorch.py:291-408) at the pre-neck feature; shares the plan of a ViTNeckNet."""

    def __init__(self, img_size=224, patch_size=16, stride_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12, num_heads=12,
                 mlp_ratio=4., qkv_bias=False, qk_scale=None, drop_rate=0., attn_drop_rate=0., camera=0, view=0, drop_path_rate=0.,
                 hybrid_backbone=None, norm_layer=None, local_feature=False, sie_xishu=1.0, device=None, seed=None):
        super().__init__()
        if in_chans != 3 or hybrid_backbone is not None:
            raise NotImplementedError("TransReID: only in_chans=3 and no hybrid backbone are in scope")
        if drop_rate != 0. or attn_drop_rate != 0.:
            raise NotImplementedError("TransReID: dropout is not supported (the reference's callers use 0)")
        self.net = ViTNeckNet(img_size, patch_size, stride_size, embed_dim, depth, num_heads, mlp_ratio, num_classes, drop_path_rate, device, seed,
                              camera=camera, view=view, sie_xishu=sie_xishu, local_feature=local_feature, qkv_bias=qkv_bias, qk_scale=qk_scale)
        self.local_feature, self.cam_num, self.view_num, self.sie_xishu = bool(local_feature), camera, view, sie_xishu
        self.num_features = self.embed_dim = embed_dim
        self.num_classes = num_classes

    def state_dict(self, *a, **k):
        return {key[len("base."):]: v for key, v in self.net.state_dict().items() if key.startswith("base.")}

    def load_state_dict(self, sd, strict=True):
        full = dict(self.net.state_dict())
        full.update({"base." + k: v for k, v in sd.items()})
        return self.net.load_state_dict(full, strict=strict)

    def load_param(self, model_path):
        """vit_pytorch.py:410-434, see load_base_param."""
        return load_base_param(self.net, model_path)

    def forward(self, x, cam_label=None, view_label=None):
        if self.local_feature:
            if self.training and torch.is_grad_enabled():
                raise NotImplementedError("TransReID(local_feature=True) is eval only: call .eval() or run under torch.no_grad()")
            return self.net.local_tokens(x, cam_label, view_label)
        return self.net.global_feat(x, cam_label, view_label)


def load_base_param(net, model_path):
    """``TransReID.load_param`` (vit_pytorch.py:410-434) on the ``base.*`` entries of a ViTNeckNet: load a pretrained ViT checkpoint (a local
    file) in place.  ``'model'`` / ``'state_dict'`` wrappers are unwrapped, keys containing ``head`` or ``dist`` are skipped, a 2-D patch
    projection (from before the conv patchification) is reshaped, and ``pos_embed`` of another token grid is resized (resize_pos_embed).  As
    in the reference a key this model lacks, or one whose shape does not fit, is reported and left out, not fatal; the list of those keys is
    returned."""
    param_dict = torch.load(model_path, map_location="cpu")
    for wrapper in ("model", "state_dict"):
        if wrapper in param_dict:
            param_dict = param_dict[wrapper]
    own = {key[len("base."):]: v for key, v in net.state_dict().items() if key.startswith("base.")}
    ps, st = net._geom[0], net._geom[1]
    num_y, num_x = (net.img_size[0] - ps) // st + 1, (net.img_size[1] - ps) // st + 1
    left_out = []
    with torch.no_grad():
        for k, v in param_dict.items():
            if "head" in k or "dist" in k:
                continue
            if "patch_embed.proj.weight" in k and v.dim() < 4:
                O, _, H, W = own["patch_embed.proj.weight"].shape
                v = v.reshape(O, -1, H, W)
            elif k == "pos_embed" and v.shape != own["pos_embed"].shape:
                if "distilled" in str(model_path):      # a distilled checkpoint carries a second (distillation) token after cls
                    v = torch.cat([v[:, 0:1], v[:, 2:]], dim=1)
                v = resize_pos_embed(v, own["pos_embed"], num_y, num_x)
            if k not in own or tuple(own[k].shape) != tuple(v.shape):
                print("load_param: left out %s: checkpoint %s vs model %s" % (k, tuple(v.shape), tuple(own[k].shape) if k in own else None))
                left_out.append(k)
                continue
            own[k].copy_(v.to(own[k].device, own[k].dtype))
    net.mark_weights_changed()
    return left_out


def resize_pos_embed(posemb, posemb_new, height, width):
    """vit_pytorch.py:436-450: position embedding [1, 1 + g*g, C] of a square g x g patch grid -> [1, 1 + height*width, C].  The cls row is
    kept, the grid is interpolated bilinearly (align_corners=False, torch's default) to height x width.  Host-side torch, on posemb's device;
    ``posemb_new`` only has to be the target tensor (its token count must be 1 + height*width)."""
    if posemb.dim() != 3 or posemb.shape[0] != 1:
        raise ValueError("resize_pos_embed: posemb must be [1, tokens, C], got %s" % (tuple(posemb.shape),))
    gs_old = int(math.sqrt(posemb.shape[1] - 1))
    if gs_old * gs_old != posemb.shape[1] - 1:
        raise ValueError("resize_pos_embed: %d patch tokens are not a square grid" % (posemb.shape[1] - 1))
    if posemb_new.shape[1] != 1 + height * width:
        raise ValueError("resize_pos_embed: the target holds %d tokens, not 1 + %d x %d" % (posemb_new.shape[1], height, width))
    cls_row, grid = posemb[:, :1], posemb[0, 1:]
    grid = grid.reshape(1, gs_old, gs_old, -1).permute(0, 3, 1, 2)
    grid = torch.nn.functional.interpolate(grid, size=(height, width), mode="bilinear")
    grid = grid.permute(0, 2, 3, 1).reshape(1, height * width, -1)
    return torch.cat([cls_row, grid], dim=1)


def vit_base_patch16_224_TransReID(img_size=(256, 128), stride_size=16, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.1, camera=0, view=0,
                                   local_feature=False, sie_xishu=1.5, **kwargs):
    """vit_pytorch.py:453-459."""
    return TransReID(img_size=img_size, patch_size=16, stride_size=stride_size, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4, qkv_bias=True,
                     camera=camera, view=view, drop_path_rate=drop_path_rate, drop_rate=drop_rate, attn_drop_rate=attn_drop_rate,
                     sie_xishu=sie_xishu, local_feature=local_feature, **kwargs)


def vit_small_patch16_224_TransReID(img_size=(256, 128), stride_size=16, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.1, camera=0, view=0,
                                    local_feature=False, sie_xishu=1.5, **kwargs):
    """vit_pytorch.py:461-468: dim 768, depth 8, 8 heads (head_dim 96), MLP ratio 3, no qkv bias, and the scale of the FULL width, 768 ** -0.5.
    Eval only (there is no attention backward at head_dim 96)."""
    kwargs.setdefault('qk_scale', 768 ** -0.5)
    return TransReID(img_size=img_size, patch_size=16, stride_size=stride_size, embed_dim=768, depth=8, num_heads=8, mlp_ratio=3., qkv_bias=False,
                     drop_path_rate=drop_path_rate, camera=camera, view=view, drop_rate=drop_rate, attn_drop_rate=attn_drop_rate,
                     sie_xishu=sie_xishu, local_feature=local_feature, **kwargs)


def deit_small_patch16_224_TransReID(img_size=(256, 128), stride_size=16, drop_path_rate=0.1, drop_rate=0.0, attn_drop_rate=0.0, camera=0, view=0,
                                     local_feature=False, sie_xishu=1.5, **kwargs):
    """vit_pytorch.py:470-476: dim 384, depth 12, 6 heads (head_dim 64), MLP ratio 4; trains and evaluates."""
    return TransReID(img_size=img_size, patch_size=16, stride_size=stride_size, embed_dim=384, depth=12, num_heads=6, mlp_ratio=4, qkv_bias=True,
                     drop_path_rate=drop_path_rate, drop_rate=drop_rate, attn_drop_rate=attn_drop_rate, camera=camera, view=view,
                     sie_xishu=sie_xishu, local_feature=local_feature, **kwargs)
