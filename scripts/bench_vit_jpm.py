#!/usr/bin/env python3
"""Timings behind the JPM rows of docs/experiments.md, HIP-event medians after warm-up, the two sides of each comparison alternating in one process:

  python scripts/bench_vit_jpm.py attention     the 13-tile and the 4-tile attention forward at B = 2000, H = 12, T = 33 and 53
  python scripts/bench_vit_jpm.py model         eval forward at batch 500, 256x128, stride 16: plain ViT-B/16 + neck against the JPM model

Prints one JSON line per comparison.  Needs an MI355X; nothing here runs on the CPU."""
import json
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fns, warmup=5, reps=30, inner=1):
    """median ms per call of each callable, round-robin so that drift hits all alike.  One event pair brackets `inner` back-to-back calls: with
    inner = 1 the window of a 0.1 ms kernel also holds the host's launch gap on an idle stream; a batch keeps the queue fed."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                f()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b) / inner)
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def attention():
    from daliid_amd import ops_vit
    B, H = 2000, 12
    for T in (33, 53):
        qkv = torch.randn(B * T, 3 * H * 64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(T)).to(torch.bfloat16)
        o13, _ = ops_vit.attention_fwd(qkv, B, T, H)
        o4, _ = ops_vit.attention_fwd_short(qkv, B, T, H)
        (m13, lo13, hi13), (m4, lo4, hi4) = timed([lambda: ops_vit.attention_fwd(qkv, B, T, H), lambda: ops_vit.attention_fwd_short(qkv, B, T, H)], inner=20)
        print(json.dumps({"what": "attention_fwd", "B": B, "T": T, "H": H, "tile13_ms": round(m13, 4), "tile13_range": [round(lo13, 4), round(hi13, 4)],
                          "tile4_ms": round(m4, 4), "tile4_range": [round(lo4, 4), round(hi4, 4)], "ratio_4_over_13": round(m4 / m13, 3),
                          "bitwise_equal": bool(torch.equal(o13, o4))}))


def model():
    from daliid_amd import make_models

    def cfg(jpm):
        return types.SimpleNamespace(
            MODEL=types.SimpleNamespace(NAME="transformer", JPM=jpm, LAST_STRIDE=1, PRETRAIN_PATH="", PRETRAIN_CHOICE="none", COS_LAYER=False,
                                        NECK="bnneck", TRANSFORMER_TYPE="vit_base_patch16_224_TransReID", SIE_CAMERA=False, SIE_VIEW=False,
                                        SIE_COE=3.0, STRIDE_SIZE=16, DROP_PATH=0.0, DROP_OUT=0.0, ATT_DROP_RATE=0.0, ID_LOSS_TYPE="softmax",
                                        RE_ARRANGE=True, SHUFFLE_GROUP=2, SHIFT_NUM=5, DEVIDE_LENGTH=4),
            TEST=types.SimpleNamespace(NECK_FEAT="after"), INPUT=types.SimpleNamespace(SIZE_TRAIN=(256, 128)))
    plain = make_models.make_model(cfg(False), 751, 0, 0, seed=1).eval()
    jpm = make_models.make_model(cfg(True), 751, 0, 0, seed=1).eval()
    x = torch.randn(500, 3, 256, 128, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    with torch.no_grad():
        (mp, lop, hip_), (mj, loj, hij) = timed([lambda: plain(x), lambda: jpm(x)], warmup=3, reps=15)
    print(json.dumps({"what": "eval_forward", "batch": 500, "size": [256, 128], "stride": 16, "plain_ms": round(mp, 3), "plain_range": [round(lop, 3), round(hip_, 3)],
                      "jpm_ms": round(mj, 3), "jpm_range": [round(loj, 3), round(hij, 3)], "ratio": round(mj / mp, 3)}))


if __name__ == "__main__":
    {"attention": attention, "model": model}[sys.argv[1] if len(sys.argv) > 1 else "model"]()
