#!/usr/bin/env python3
"""Generate tests/golden/vit_small.npz by RUNNING the reference's own make_models.py / vit_pytorch.py on the CPU (as make_vit_long_golden.py
does), for the two small backbones of make_models.py:392-397:

    python tests/golden/make_vit_small_golden.py

The reference tree exists on the build machine only; never run this where there is a GPU to test.  Weights are seeded per key
(tests/vit_small_ref.py::seeded_state), so the file stores keys, shapes, geometry and the reference's outputs -- data only.

  vs16    make_model with vit_small_patch16_224_TransReID (dim 768, depth 8, 8 heads = head_dim 96, MLP ratio 3, no qkv bias, scale 768 ** -0.5),
          256x128 at stride 16 (129 tokens), eval mode, B = 2, input randn seed 77: y_eval and global_feat
  vs12    the same at 384x128, stride 12 (311 tokens)
  vsjpm   build_transformer_local with the vit_small factory at depth 2, 256x128 at stride 16 (four runs of 32 + cls = 33 tokens),
          3 cameras x 2 views, 'after'
  ds16    make_model with deit_small_patch16_224_TransReID (dim 384, depth 12, 6 heads), 256x128 at stride 16, eval mode

With 0.02-std weights the attention is nearly uniform and a wrong scale hides, so the ViT-Small cases seed attn.qkv.weight at std 0.05.  Each
of them is rerun with qk_scale = 96 ** -0.5 (the head width's scale, which the reference does NOT use): y must move by at least 0.1 rel-L2,
five times the GPU test's bound of 2e-2; the figure is stored as <case>/scale_shift.
"""
import contextlib
import functools
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))            # tests/ (vit_small_ref)

import make_golden  # noqa: E402, F401  (puts the reference tree on sys.path, as for the other goldens)
from make_vit_jpm_golden import cfg_of  # noqa: E402
from vit_small_ref import rel_l2, seeded_state  # noqa: E402

VS, DS = "vit_small_patch16_224_TransReID", "deit_small_patch16_224_TransReID"
QKV_STD, X_SEED, JPM_SEED, MIN_SHIFT = 0.05, 77, 86, 0.1


def cfg_for(name, size, stride, jpm=False, sie=False):
    cfg = cfg_of(size, stride, jpm, sie, sie, 3.0, "after")
    cfg.MODEL.TRANSFORMER_TYPE = name
    cfg.MODEL.RE_ARRANGE = jpm
    return cfg


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def load(model, out, pre, qkv_std):
    keys = list(model.state_dict().keys())
    shapes = [str(tuple(v.shape)) for v in model.state_dict().values()]
    out[pre + "keys"], out[pre + "shapes"] = np.array(keys), np.array(shapes)
    model.load_state_dict(seeded_state(keys, shapes, qkv_std))
    return model.eval()


def small_factory(V, depth, **extra):
    """the reference's vit_small factory at another depth and, for the scale rerun, another qk_scale (its **kwargs reach TransReID)"""
    def make(**kw):
        kw = dict(kw, **extra)
        kw.setdefault("qk_scale", 768 ** -0.5)
        return V.TransReID(patch_size=16, embed_dim=768, depth=depth, num_heads=8, mlp_ratio=3., qkv_bias=False,
                           norm_layer=functools.partial(torch.nn.LayerNorm, eps=1e-6), **kw)
    return {VS: make}


def main():
    import make_models as M
    import vit_pytorch as V
    out = {}
    for name, typ, size, stride in (("vs16", VS, (256, 128), 16), ("vs12", VS, (384, 128), 12), ("ds16", DS, (256, 128), 16)):
        cfg = cfg_for(typ, size, stride)
        full = load(quiet(M.make_model, cfg, 10, 0, 0), out, name + "/", QKV_STD if typ == VS else 0.02)
        x = torch.randn(2, 3, *size, generator=torch.Generator().manual_seed(X_SEED))
        with torch.no_grad():
            y, gf = full(x), full.base(x)
        out[name + "/y_eval"], out[name + "/global_feat"] = y.numpy(), gf.numpy()
        out[name + "/geom"] = np.array([size[0], size[1], stride], dtype=np.int64)
        print(name, "tokens", full.base.pos_embed.shape[1], "y", tuple(y.shape), "keys", len(out[name + "/keys"]))
        if typ == VS:
            assert not any(k.endswith("attn.qkv.bias") for k in full.state_dict())
            other = quiet(M.build_transformer, 10, 0, 0, cfg, small_factory(V, 8, qk_scale=96 ** -0.5))
            other.load_state_dict(full.state_dict())
            other.eval()
            with torch.no_grad():
                shift, shift_gf = rel_l2(other(x), y), rel_l2(other.base(x), gf)
            print("   qk_scale 96^-0.5 instead of 768^-0.5 moves y_eval by %.3f rel-L2, global_feat by %.3f" % (shift, shift_gf))
            assert shift >= MIN_SHIFT, shift
            out[name + "/scale_shift"] = np.float64(shift)

    size, stride, depth, cams, views = (256, 128), 16, 2, 3, 2
    cfg = cfg_for(VS, size, stride, jpm=True, sie=True)
    model = load(quiet(M.build_transformer_local, 10, cams, views, cfg, small_factory(V, depth), rearrange=True), out, "vsjpm/", QKV_STD)
    x = torch.randn(2, 3, *size, generator=torch.Generator().manual_seed(JPM_SEED))
    cam, view = [1, 2], [0, 1]
    with torch.no_grad():
        y = model(x, cam_label=torch.tensor(cam), view_label=torch.tensor(view))
    other = quiet(M.build_transformer_local, 10, cams, views, cfg, small_factory(V, depth, qk_scale=96 ** -0.5), rearrange=True)
    other.load_state_dict(model.state_dict())
    other.eval()
    with torch.no_grad():
        shift = rel_l2(other(x, cam_label=torch.tensor(cam), view_label=torch.tensor(view)), y)
    print("vsjpm y", tuple(y.shape), "keys", len(out["vsjpm/keys"]), "; qk_scale 96^-0.5 moves y by %.3f rel-L2" % shift)
    assert shift >= MIN_SHIFT, shift
    out["vsjpm/y"], out["vsjpm/scale_shift"] = y.numpy(), np.float64(shift)
    out["vsjpm/geom"] = np.array([size[0], size[1], stride, depth, cams, views, JPM_SEED], dtype=np.int64)
    out["vsjpm/coef"], out["vsjpm/neck_feat"] = np.float64(3.0), np.array("after")
    out["vsjpm/cam"], out["vsjpm/view"] = np.array(cam, dtype=np.int64), np.array(view, dtype=np.int64)
    out["qkv_std"], out["x_seed"] = np.float64(QKV_STD), np.int64(X_SEED)
    path = os.path.join(HERE, "vit_small.npz")
    np.savez_compressed(path, **out)
    print("vit_small.npz ok:", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
