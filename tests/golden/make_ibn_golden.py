#!/usr/bin/env python3
"""Generate tests/golden/ibn.npz by RUNNING the reference's own Encoders.py on the CPU (as make_golden.py does for the other files):

    python tests/golden/make_ibn_golden.py

The reference tree exists on the build machine only.  The trunk (IBN-Net's resnet50_ibn_a / resnet101_ibn_a) is third-party and absent, so it
is tests/ibn_ref.ibn_trunk; what is pinned here is the reference's wrapper classes over such a trunk.  Weights are seeded per key
(ibn_ref.seeded_state), so the file stores key names, shapes, seeds and the reference's output -- data only.

  r50/, r101/   keys and shapes of Encoders.ResNet50IBNReID / ResNet101IBNReID over the full-depth trunks
  small/        ResNet50IBNReID over a (1, 1, 1, 1) / width-64 trunk (IBN in layer1-3): keys, shapes, and the eval output [4, 2048] for
                randn(4, 3, 64, 32) (seed small/x_seed), weights seeded_state(seed small/w_seed)
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))            # tests/ (ibn_ref)

import make_golden  # noqa: E402  (puts the reference tree and the repository root on sys.path)
import ibn_ref  # noqa: E402

W_SEED, X_SEED = 4100, 79


def table(model, out, pre):
    out[pre + "keys"] = np.array(list(model.state_dict().keys()))
    out[pre + "shapes"] = np.array([str(tuple(v.shape)) for v in model.state_dict().values()])


def main():
    make_golden.install_shims()
    with contextlib.redirect_stdout(io.StringIO()):
        import Encoders as R                          # the reference's
    assert R.__file__.startswith(make_golden.REF), R.__file__
    out = {}
    table(R.ResNet50IBNReID(ibn_ref.ibn_trunk((3, 4, 6, 3))), out, "r50/")
    table(R.ResNet101IBNReID(ibn_ref.ibn_trunk((3, 4, 23, 3))), out, "r101/")
    model = R.ResNet50IBNReID(ibn_ref.ibn_trunk((1, 1, 1, 1), 64))
    table(model, out, "small/")
    model.load_state_dict(ibn_ref.seeded_state(model.state_dict(), W_SEED))
    model.eval()
    x = torch.randn(4, 3, 64, 32, generator=torch.Generator().manual_seed(X_SEED))
    with torch.no_grad():
        out["small/y_eval"] = model(x).numpy()
    out["small/w_seed"], out["small/x_seed"] = np.int64(W_SEED), np.int64(X_SEED)
    out["small/geom"] = np.array([4, 64, 32, 1, 1, 1, 1, 64], dtype=np.int64)        # batch, H, W, layers, width
    for pre in ("r50/", "r101/", "small/"):
        print(pre, len(out[pre + "keys"]), "keys")
    path = os.path.join(HERE, "ibn.npz")
    np.savez_compressed(path, **out)
    print("ibn.npz ok:", os.path.getsize(path), "bytes; |y| mean", float(np.abs(out["small/y_eval"]).mean()))


if __name__ == "__main__":
    main()
