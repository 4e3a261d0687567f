#!/usr/bin/env python3
"""Generate tests/golden/vit_jpm.npz by RUNNING the reference's own make_models.py / vit_pytorch.py (as make_golden.py does), on the CPU:

    python tests/golden/make_vit_jpm_golden.py

The reference tree exists on the build machine only; never run this where there is a GPU to test.  Weights are seeded per key
(tests/vit_jpm_ref.py::seeded_state), so the file stores keys, shapes, input seeds, labels and the reference's outputs -- data only.

  shuffle/<n>_<groups>_<shift>   shuffle_unit on tokens that carry their own index: the shuffled order (1-based patch indices)
  shuffle/raises                 the (n, groups) pairs, shift 5, at which shuffle_unit raises
  A, B, C                        build_transformer_local in eval mode, B = 2 (256x128 stride 16 depth 12 'after';
                                 256x128 stride 12 depth 12, 6 cameras, SIE_COE 3.0, 'before'; 48x48 depth 2, 3 cameras x 2 views, 'after')
  C/tokens                       the local_feature tokens of case C (base(x) of the JPM model)
  train                          build_transformer with C's SIE geometry, train mode, B = 6: output and sie_embed.grad for a seeded cotangent
"""
import contextlib
import functools
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
from vit_jpm_ref import seeded_state  # noqa: E402

NAME = "vit_base_patch16_224_TransReID"


def cfg_of(size, stride, jpm, sie_cam, sie_view, coef, neck_feat, groups=2, shift=5):
    return types.SimpleNamespace(
        MODEL=types.SimpleNamespace(NAME="transformer", JPM=jpm, LAST_STRIDE=1, PRETRAIN_PATH="", PRETRAIN_CHOICE="none", COS_LAYER=False,
                                    NECK="bnneck", TRANSFORMER_TYPE=NAME, SIE_CAMERA=sie_cam, SIE_VIEW=sie_view, SIE_COE=coef,
                                    STRIDE_SIZE=stride, DROP_PATH=0.0, DROP_OUT=0.0, ATT_DROP_RATE=0.0, ID_LOSS_TYPE="softmax",
                                    RE_ARRANGE=True, SHUFFLE_GROUP=groups, SHIFT_NUM=shift, DEVIDE_LENGTH=4),
        TEST=types.SimpleNamespace(NECK_FEAT=neck_feat), INPUT=types.SimpleNamespace(SIZE_TRAIN=size))


def factory(V, depth):
    def make(**kw):
        return V.TransReID(patch_size=16, embed_dim=768, depth=depth, num_heads=12, mlp_ratio=4, qkv_bias=True,
                           norm_layer=functools.partial(torch.nn.LayerNorm, eps=1e-6), **kw)
    return {NAME: make}


def load_seeded(model, out, pre):
    keys = list(model.state_dict().keys())
    shapes = [str(tuple(v.shape)) for v in model.state_dict().values()]
    out[pre + "keys"], out[pre + "shapes"] = np.array(keys), np.array(shapes)
    model.load_state_dict(seeded_state(keys, shapes))


def main():
    import make_models as M
    import vit_pytorch as V
    out = {}
    # ---- shuffle_unit on index-valued tokens ----
    raises = []
    for n, groups, shift in [(128, 2, 5), (210, 2, 5), (9, 2, 5), (12, 4, 5), (7, 4, 5), (7, 2, 5), (128, 4, 8), (210, 4, 5), (9, 4, 5)]:
        feats = torch.arange(n + 1, dtype=torch.float32).reshape(1, n + 1, 1)
        try:
            order = M.shuffle_unit(feats, shift, groups).reshape(-1).to(torch.int32).numpy()
        except Exception:
            raises.append((n, groups))
            continue
        out["shuffle/%d_%d_%d" % (n, groups, shift)] = order
    out["shuffle/raises"] = np.array(raises, dtype=np.int32)

    # ---- end-to-end cases ----
    cases = {
        "A": dict(size=(256, 128), stride=16, depth=12, cams=0, views=0, coef=3.0, neck="after", cam=None, view=None, seed=81),
        "B": dict(size=(256, 128), stride=12, depth=12, cams=6, views=0, coef=3.0, neck="before", cam=[1, 4], view=None, seed=82),
        "C": dict(size=(48, 48), stride=16, depth=2, cams=3, views=2, coef=3.0, neck="after", cam=[1, 2], view=[0, 1], seed=83),
    }
    for name, c in cases.items():
        cfg = cfg_of(c["size"], c["stride"], True, c["cams"] > 1, c["views"] > 1, c["coef"], c["neck"])
        with contextlib.redirect_stdout(io.StringIO()):
            model = M.build_transformer_local(10, c["cams"], c["views"], cfg, factory(V, c["depth"]), rearrange=True)
        load_seeded(model, out, name + "/")
        model.eval()
        x = torch.randn(2, 3, *c["size"], generator=torch.Generator().manual_seed(c["seed"]))
        cam = None if c["cam"] is None else torch.tensor(c["cam"])
        view = None if c["view"] is None else torch.tensor(c["view"])
        with torch.no_grad():
            y = model(x, cam_label=cam, view_label=view)
            if name == "C":
                out["C/tokens"] = model.base(x, cam_label=cam, view_label=view).numpy()
        out[name + "/y"] = y.numpy()
        out[name + "/geom"] = np.array([c["size"][0], c["size"][1], c["stride"], c["depth"], c["cams"], c["views"], c["seed"]], dtype=np.int64)
        out[name + "/coef"] = np.float64(c["coef"])
        out[name + "/neck_feat"] = np.array(c["neck"])
        out[name + "/cam"] = np.array(c["cam"] if c["cam"] is not None else [], dtype=np.int64)
        out[name + "/view"] = np.array(c["view"] if c["view"] is not None else [], dtype=np.int64)
        print(name, "y", tuple(y.shape), "keys", len(out[name + "/keys"]))

    # ---- SIE training: build_transformer, C's geometry, B = 6 (a BatchNorm over two samples has no gradient to speak of) ----
    cfg = cfg_of((48, 48), 16, False, True, True, 3.0, "after")
    with contextlib.redirect_stdout(io.StringIO()):
        model = M.build_transformer(10, 3, 2, cfg, factory(V, 2))
    load_seeded(model, out, "train/")
    model.train()
    g = torch.Generator().manual_seed(84)
    x = torch.randn(6, 3, 48, 48, generator=g)
    w = torch.randn(6, 768, generator=g)
    cam, view = torch.tensor([1, 2, 1, 1, 0, 1]), torch.tensor([0, 1, 0, 1, 0, 1])        # rows 2, 5, 2, 3, 0, 3: rows 1 and 4 stay unused
    y = model(x, cam_label=cam, view_label=view)
    (y * w).sum().backward()
    out["train/y"], out["train/sie_grad"] = y.detach().numpy(), model.base.sie_embed.grad.numpy()
    out["train/cam"], out["train/view"], out["train/seed"] = cam.numpy(), view.numpy(), np.int64(84)
    np.savez_compressed(os.path.join(HERE, "vit_jpm.npz"), **out)
    print("vit_jpm.npz ok:", os.path.getsize(os.path.join(HERE, "vit_jpm.npz")), "bytes; raises at", raises)


if __name__ == "__main__":
    main()
