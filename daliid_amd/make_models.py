"""Mirror of the reference's ``make_models.py`` for the path in scope: ``make_model(cfg, num_class, camera_num, view_num)``
(make_models.py:399-410) -> ``build_transformer`` (:121-218): TransReID ViT encoder + BatchNorm1d neck with frozen bias,
``forward(x, label=None, cam_label=None, view_label=None)`` returning the post-neck ``feat`` (:184-205), or, with ``cfg.MODEL.JPM``,
``build_transformer_local`` (:221-389): the JPM head (global branch + four shuffled local runs through a shared block, five necks) whose
eval forward returns ``[B, 5 * 768]``.  ``cfg.MODEL.TRANSFORMER_TYPE`` takes the reference's four names (make_models.py:392-397): ViT-B/16 under
two of them, DeiT-Small (dim 384, trains) and ViT-Small (head_dim 96: eval only; JPM in eval).  SIE camera / view embeddings follow ``cfg.MODEL.SIE_CAMERA`` / ``SIE_VIEW`` / ``SIE_COE``.

``cfg`` is the same yacs-like attribute tree the reference reads (cfg.MODEL.*, cfg.TEST.NECK_FEAT, cfg.INPUT.SIZE_TRAIN).
Out of scope: ``Backbone`` (broken in the reference, make_models.py:63) and JPM's train-mode forward (classifier scores for an
ID loss the trainer never uses).
"""
import os

import numpy as np
import torch

from ._lib import DaliError
from .vit_pytorch import ViTNeckNet, load_base_param

_GEOM = {  # factory name -> (embed_dim, depth, heads, mlp_ratio, qkv_bias, qk_scale)   (vit_pytorch.py:453-476, make_models.py:392-397)
    "vit_base_patch16_224_TransReID": (768, 12, 12, 4.0, True, None),
    "deit_base_patch16_224_TransReID": (768, 12, 12, 4.0, True, None),
    "vit_small_patch16_224_TransReID": (768, 8, 8, 3.0, False, 768 ** -0.5),       # head_dim 96: eval only
    "deit_small_patch16_224_TransReID": (384, 12, 6, 4.0, True, None),             # in_planes 384 (make_models.py:148-149)
}


def jpm_token_map(n_patches, shift, groups, divide=4, rearrange=True):
    """Which patch token (1-based, i.e. its index among the ``1 + n_patches`` tokens) the JPM branch puts where: int32 ``[divide, L]``,
    ``L = n_patches // divide``; row i is the i-th local run (make_models.py:323-349).  With ``rearrange``: ``shuffle_unit``
    (make_models.py:8-25) -- the tokens rotated to start at ``shift``, then split into ``groups`` and interleaved; a length that does not
    divide by ``groups`` gets the second-to-last token appended once (it lands at the very end, behind every run).  Raises DaliError where
    the reference raises at run time, and for ``shift`` outside ``[1, n_patches)``.  The map does not depend on the data."""
    n_patches, shift, groups, divide = int(n_patches), int(shift), int(groups), int(divide)
    if divide < 1 or n_patches // divide < 1:
        raise DaliError("jpm_token_map: %d patch tokens cannot be cut into %d runs" % (n_patches, divide))
    if rearrange:
        if shift < 1 or shift >= n_patches:
            raise DaliError("jpm_token_map: shift %d outside [1, %d)" % (shift, n_patches))
        if groups < 1:
            raise DaliError("jpm_token_map: groups must be positive")
        x = list(range(shift, n_patches + 1)) + list(range(1, shift))
        if len(x) % groups:
            x.append(x[-2])
        if len(x) % groups:
            raise DaliError("jpm_token_map: %d patch tokens (+1 padded) do not divide into %d shuffle groups" % (n_patches, groups))
        x = np.asarray(x, dtype=np.int32).reshape(groups, -1).T.reshape(-1)
    else:
        x = np.arange(1, n_patches + 1, dtype=np.int32)
    L = n_patches // divide
    return np.ascontiguousarray(x[:divide * L].reshape(divide, L).astype(np.int32))


def _base_kwargs(cfg, camera_num, view_num, depth, device, seed, who):
    name = cfg.MODEL.TRANSFORMER_TYPE
    if name not in _GEOM:
        raise NotImplementedError("%s: transformer type %r is out of scope (admitted: %s)" % (who, name, ", ".join(_GEOM)))
    if getattr(cfg.MODEL, "DROP_OUT", 0.0) != 0.0 or getattr(cfg.MODEL, "ATT_DROP_RATE", 0.0) != 0.0:
        raise NotImplementedError("%s: dropout is not supported" % who)
    if cfg.MODEL.PRETRAIN_CHOICE == 'imagenet' and not os.path.isfile(str(cfg.MODEL.PRETRAIN_PATH)):
        raise NotImplementedError("%s: ImageNet checkpoint loading needs a file fetched from the network; "
                                  "load a state_dict with load_state_dict instead" % who)
    dim, geom_depth, heads, ratio, qkv_bias, qk_scale = _GEOM[name]
    print('using Transformer_type: {} as a backbone'.format(name))
    return dict(img_size=cfg.INPUT.SIZE_TRAIN, patch_size=16, stride_size=cfg.MODEL.STRIDE_SIZE, embed_dim=dim, depth=geom_depth if depth is None else depth,
                num_heads=heads, mlp_ratio=ratio, num_classes=1000, drop_path_rate=cfg.MODEL.DROP_PATH, device=device, seed=seed,
                camera=camera_num if cfg.MODEL.SIE_CAMERA else 0, view=view_num if cfg.MODEL.SIE_VIEW else 0,      # make_models.py:135-142
                sie_xishu=cfg.MODEL.SIE_COE, qkv_bias=qkv_bias, qk_scale=qk_scale)


def _load_pretrained(model, cfg):
    """make_models.py:150-152, :245-247: with PRETRAIN_CHOICE 'imagenet' the base loads cfg.MODEL.PRETRAIN_PATH (a local file, checked in _base_kwargs)
    through TransReID.load_param: head / dist keys skipped, pos_embed resized to this geometry."""
    if cfg.MODEL.PRETRAIN_CHOICE == 'imagenet':
        load_base_param(model, cfg.MODEL.PRETRAIN_PATH)
        model._copy_jpm_branches()                       # make_models.py:247-258 copies the block and norm after the base has loaded
        print('Loading pretrained ImageNet model......from {}'.format(cfg.MODEL.PRETRAIN_PATH))


class _Checkpoints:
    """``load_param`` / ``load_param_finetune`` of the reference's builders (make_models.py:208-218, :379-389): every tensor of a saved state
    dict goes into the entry of the same name; the first also accepts the ``module.`` names an ``nn.DataParallel`` wrapper saves.  Entries the
    file does not hold keep their values; a name this model does not have is an error, as it is there."""

    def _load_file(self, path, strip_wrapper):
        saved = torch.load(path, map_location="cpu")
        renamed = {(name.replace("module.", "") if strip_wrapper else name): tensor for name, tensor in saved.items()}
        unknown = sorted(set(renamed) - set(self.state_dict()))
        if unknown:
            raise KeyError("checkpoint %s holds entries this model does not have: %s" % (path, ", ".join(unknown[:5])))
        self.load_state_dict(renamed, strict=False)          # the post hook marks the weights as changed

    def load_param(self, trained_path):
        self._load_file(trained_path, strip_wrapper=True)
        print("Loaded the trained model %s" % trained_path)

    def load_param_finetune(self, model_path):
        self._load_file(model_path, strip_wrapper=False)
        print("Loaded %s for finetuning" % model_path)


class build_transformer(_Checkpoints, ViTNeckNet):
    def __init__(self, num_classes, camera_num, view_num, cfg, factory=None, device=None, seed=None, depth=None):
        super().__init__(**_base_kwargs(cfg, camera_num, view_num, depth, device, seed, "build_transformer"))
        self.neck, self.neck_feat, self.cos_layer = cfg.MODEL.NECK, cfg.TEST.NECK_FEAT, cfg.MODEL.COS_LAYER
        self.num_classes, self.ID_LOSS_TYPE = num_classes, cfg.MODEL.ID_LOSS_TYPE
        _load_pretrained(self, cfg)


class build_transformer_local(_Checkpoints, ViTNeckNet):
    """make_models.py:221-389, eval mode: ``cat([bottleneck(global), bottleneck_i(local_i) / 4])`` (``cfg.TEST.NECK_FEAT == 'after'``) or the
    same without the necks, [B, 5 * 768].  State-dict keys as the reference's: ``base.*``, ``b1.0.*``, ``b1.1.*``, ``b2.0.*``, ``b2.1.*``,
    ``classifier*.weight``, ``bottleneck*``."""

    def __init__(self, num_classes, camera_num, view_num, cfg, factory=None, rearrange=True, device=None, seed=None, depth=None):
        kw = _base_kwargs(cfg, camera_num, view_num, depth, device, seed, "build_transformer_local")
        if kw["embed_dim"] != 768:
            raise NotImplementedError("build_transformer_local: JPM with %s is out of scope: the reference builds 768-wide necks there "
                                      "(in_planes = 768, make_models.py:229) over a %d-wide base and fails on its first forward"
                                      % (cfg.MODEL.TRANSFORMER_TYPE, kw["embed_dim"]))
        if cfg.MODEL.ID_LOSS_TYPE in ('arcface', 'cosface', 'amsoftmax', 'circle'):
            raise NotImplementedError("build_transformer_local: margin classifiers (ID_LOSS_TYPE %r) are out of scope" % cfg.MODEL.ID_LOSS_TYPE)
        groups, shift, divide = int(cfg.MODEL.SHUFFLE_GROUP), int(cfg.MODEL.SHIFT_NUM), int(cfg.MODEL.DEVIDE_LENGTH)
        if divide != 4:
            raise DaliError("build_transformer_local: DEVIDE_LENGTH must be 4 (the reference's forward cuts four runs, make_models.py:331-349)")
        h, w = (kw["img_size"], kw["img_size"]) if isinstance(kw["img_size"], int) else kw["img_size"]
        n_patches = ((h - 16) // kw["stride_size"] + 1) * ((w - 16) // kw["stride_size"] + 1)
        token_map = jpm_token_map(n_patches, shift, groups, divide, rearrange)          # raises here where the reference would at run time
        super().__init__(jpm=dict(token_map=token_map, neck_after=int(cfg.TEST.NECK_FEAT == 'after'), id_classes=int(num_classes)), **kw)
        self.shuffle_groups, self.shift_num, self.divide_length, self.rearrange, self.token_map = groups, shift, divide, bool(rearrange), token_map
        print("JPM head: %d runs of %d tokens, shift %d, %d shuffle groups%s" % (divide, token_map.shape[1], shift, groups, "" if rearrange else " (not rearranged)"))
        self.neck, self.neck_feat, self.cos_layer = cfg.MODEL.NECK, cfg.TEST.NECK_FEAT, cfg.MODEL.COS_LAYER
        self.num_classes, self.ID_LOSS_TYPE = num_classes, cfg.MODEL.ID_LOSS_TYPE
        _load_pretrained(self, cfg)

    def forward(self, x, label=None, cam_label=None, view_label=None):
        if self.training:
            raise NotImplementedError("build_transformer_local: the train-mode forward returns classifier scores for an ID loss that this "
                                      "project's trainer never uses (make_models.py:358-370); JPM is eval only, call .eval()")
        return self._run_forward(x, False, sie_idx=self.sie_index(cam_label, view_label, x.shape[0]))


def make_model(cfg, num_class, camera_num, view_num, device=None, seed=None, depth=None):
    """make_models.py:399-410."""
    if cfg.MODEL.NAME != 'transformer':
        raise NotImplementedError("make_model: the ResNet `Backbone` branch is broken in the reference (make_models.py:63) and out of scope; "
                                  "use Encoders.getDCNN('resnet50')")
    if cfg.MODEL.JPM:
        model = build_transformer_local(num_class, camera_num, view_num, cfg, None, rearrange=cfg.MODEL.RE_ARRANGE, device=device, seed=seed, depth=depth)
        print('=========== built the transformer with its JPM head ===========')
    else:
        model = build_transformer(num_class, camera_num, view_num, cfg, None, device=device, seed=seed, depth=depth)
        print('===========building transformer===========')
    return model
