#!/usr/bin/env python3
"""Generate tests/golden/vit_long.npz by RUNNING the reference's own make_models.py / vit_pytorch.py on the CPU (as make_golden.py and
make_vit_jpm_golden.py do), at geometries past 256 tokens:

    python tests/golden/make_vit_long_golden.py

The reference tree exists on the build machine only; never run this where there is a GPU to test.  Weights are seeded per key, so the file
stores keys, shapes and the reference's outputs -- data only.

  s12, v16      make_models.make_model, ViT-B/16 + BN neck, eval mode, B = 2: 384x128 at stride 12 (311 tokens) and 256x256 at stride 16 (257);
                weights per key as make_golden.gen_vit seeds them (seed 1000 + i), input randn seed 77; y_eval and global_feat
  jpm           build_transformer_local at 384x128, stride 12 (310 patches, four runs of 77), depth 2, 3 cameras x 2 views, 'after';
                weights by vit_jpm_ref.seeded_state, as make_vit_jpm_golden.py's cases
  resize        resize_pos_embed of randn(1, 1 + 14*14, 16) (seed 91) to (31, 10) and to (16, 16)
"""
import contextlib
import io
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))            # tests/ (vit_jpm_ref)

import make_golden  # noqa: E402, F401  (puts the reference tree on sys.path, as for the other goldens)
from make_vit_jpm_golden import cfg_of, factory, load_seeded  # noqa: E402

RESIZE_SEED, JPM_SEED = 91, 85


def gen_vit_state(model):
    """make_golden.gen_vit's deterministic re-init: per-key seeded, reproducible in the test without the reference"""
    sd = {}
    for i, (k, v) in enumerate(model.state_dict().items()):
        gg = torch.Generator().manual_seed(1000 + i)
        if not v.dtype.is_floating_point:
            sd[k] = v.clone()
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(v.shape, generator=gg)
        elif k.endswith("norm1.weight") or k.endswith("norm2.weight") or k.endswith("norm.weight") or k == "bottleneck.weight":
            sd[k] = 1.0 + 0.1 * torch.randn(v.shape, generator=gg)
        else:
            sd[k] = 0.02 * torch.randn(v.shape, generator=gg)
    return sd


def main():
    import make_models as M
    import vit_pytorch as V
    out = {}
    for name, size, stride in (("s12", (384, 128), 12), ("v16", (256, 256), 16)):
        cfg = cfg_of(size, stride, False, False, False, 3.0, "after")
        cfg.MODEL.RE_ARRANGE = False
        with contextlib.redirect_stdout(io.StringIO()):
            torch.manual_seed(8)
            full = M.make_model(cfg, 10, 0, 0)
        out[name + "/keys"] = np.array(list(full.state_dict().keys()))
        out[name + "/shapes"] = np.array([str(tuple(v.shape)) for v in full.state_dict().values()])
        full.load_state_dict(gen_vit_state(full))
        full.eval()
        x = torch.randn(2, 3, *size, generator=torch.Generator().manual_seed(77))
        with torch.no_grad():
            out[name + "/y_eval"], out[name + "/global_feat"] = full(x).numpy(), full.base(x).numpy()
        out[name + "/geom"] = np.array([size[0], size[1], stride], dtype=np.int64)
        print(name, "tokens", full.base.pos_embed.shape[1], "y", out[name + "/y_eval"].shape)

    size, stride, depth, cams, views = (384, 128), 12, 2, 3, 2
    cfg = cfg_of(size, stride, True, True, True, 3.0, "after")
    with contextlib.redirect_stdout(io.StringIO()):
        model = M.build_transformer_local(10, cams, views, cfg, factory(V, depth), rearrange=True)
    load_seeded(model, out, "jpm/")
    model.eval()
    x = torch.randn(2, 3, *size, generator=torch.Generator().manual_seed(JPM_SEED))
    cam, view = [1, 2], [0, 1]
    with torch.no_grad():
        out["jpm/y"] = model(x, cam_label=torch.tensor(cam), view_label=torch.tensor(view)).numpy()
    out["jpm/geom"] = np.array([size[0], size[1], stride, depth, cams, views, JPM_SEED], dtype=np.int64)
    out["jpm/coef"], out["jpm/neck_feat"] = np.float64(3.0), np.array("after")
    out["jpm/cam"], out["jpm/view"] = np.array(cam, dtype=np.int64), np.array(view, dtype=np.int64)
    print("jpm y", out["jpm/y"].shape, "keys", len(out["jpm/keys"]))

    pos = torch.randn(1, 1 + 14 * 14, 16, generator=torch.Generator().manual_seed(RESIZE_SEED))
    for h, w in ((31, 10), (16, 16)):
        with contextlib.redirect_stdout(io.StringIO()):
            out["resize/%dx%d" % (h, w)] = V.resize_pos_embed(pos, torch.zeros(1, 1 + h * w, 16), h, w).numpy()
    out["resize/seed"] = np.int64(RESIZE_SEED)
    path = os.path.join(HERE, "vit_long.npz")
    np.savez_compressed(path, **out)
    print("vit_long.npz ok:", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
