"""Timing of the attention forward past 256 tokens (attention_fwd_long_kernel) at H = 12, head_dim 64: (B, T) = (500, 311) = 384x128 at
stride 12, (500, 257) = 256x256 at stride 16, (128, 577) = 384x384 at stride 16; and the whole eval forward of ViT-B/16 at 384x128 / stride 12,
batch 500, in images/s, with the plan's arena size.  Two yardsticks per shape, measured in the same run on the same GPU:
  * the <= 256-token kernel at (B, 256), scaled by (T / 256)^2 -- what the existing code would need if its cost grew with the score matrix;
  * torch.nn.functional.scaled_dot_product_attention on bf16 [B, H, T, 64] operands.
Per launch: HIP-event time over windows of INNER launches after WARM warm-ups, median and range of WINDOWS windows.  One JSON line per result;
MD=path appends a markdown table.  SKIP_MODEL=1 leaves the whole-model part out."""
import json
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from daliid_amd import ops_vit as V

bf16 = torch.bfloat16
H = 12
WARM, INNER, WINDOWS = int(os.environ.get("WARM", 5)), int(os.environ.get("INNER", 50)), int(os.environ.get("WINDOWS", 5))


def timed(fn, inner=INNER, windows=WINDOWS, warm=WARM):
    """ms per call: (median, min, max) over `windows` device-synchronised windows of `inner` calls"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def attention_case(B, T, g):
    qkv = torch.randn(B * T, 3 * H * 64, device="cuda", generator=g).to(bf16)
    q, k, v = (t.contiguous() for t in qkv.reshape(B, T, 3, H, 64).permute(2, 0, 3, 1, 4))
    base = torch.randn(B * 256, 3 * H * 64, device="cuda", generator=g).to(bf16)
    ours = timed(lambda: V.attention_fwd(qkv, B, T, H))
    short = timed(lambda: V.attention_fwd(base, B, 256, H))
    sdpa = timed(lambda: F.scaled_dot_product_attention(q, k, v))
    flops = 4.0 * B * H * T * T * 64                      # Q K^T and P V
    r = {"what": "attention_fwd", "B": B, "T": T, "H": H, "ms": round(ours[0], 4), "ms_range": [round(ours[1], 4), round(ours[2], 4)],
         "tflops": round(flops / ours[0] / 1e9, 1),
         "t256_ms": round(short[0], 4), "t256_scaled_ms": round(short[0] * (T / 256.0) ** 2, 4),
         "sdpa_bf16_ms": round(sdpa[0], 4), "sdpa_range": [round(sdpa[1], 4), round(sdpa[2], 4)]}
    print(json.dumps(r), flush=True)
    return r


def model_case(batch=500):
    from daliid_amd import make_models
    cfg = types.SimpleNamespace(
        MODEL=types.SimpleNamespace(NAME="transformer", JPM=False, LAST_STRIDE=1, PRETRAIN_PATH="", PRETRAIN_CHOICE="none", COS_LAYER=False,
                                    NECK="bnneck", TRANSFORMER_TYPE="vit_base_patch16_224_TransReID", SIE_CAMERA=False, SIE_VIEW=False,
                                    SIE_COE=3.0, STRIDE_SIZE=12, DROP_PATH=0.0, DROP_OUT=0.0, ATT_DROP_RATE=0.0, ID_LOSS_TYPE="softmax",
                                    RE_ARRANGE=False),
        TEST=types.SimpleNamespace(NECK_FEAT="after"), INPUT=types.SimpleNamespace(SIZE_TRAIN=(384, 128)))
    model = make_models.make_model(cfg, 10, 0, 0, seed=1).eval()
    x = torch.randn(batch, 3, 384, 128, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    with torch.no_grad():
        med, lo, hi = timed(lambda: model(x), inner=5, windows=5, warm=2)
    r = {"what": "vit_b16_eval_forward", "size": [384, 128], "stride": 12, "tokens": model.num_tokens, "batch": batch, "ms": round(med, 2),
         "ms_range": [round(lo, 2), round(hi, 2)], "images_per_s": round(batch / med * 1e3, 1), "arena_bytes": int(model._plan(batch).arena_bytes)}
    print(json.dumps(r), flush=True)
    return r


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_attention_long: needs the GPU (no CPU timing is meaningful)")
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = [attention_case(B, T, g) for B, T in ((500, 311), (500, 257), (128, 577))]
    model = None if os.environ.get("SKIP_MODEL") else model_case()
    if os.environ.get("MD"):
        with open(os.environ["MD"], "a") as f:
            f.write("\n| B | T | ms per launch (range) | TFLOP/s | T = 256 kernel x (T/256)^2, ms | SDPA bf16, ms |\n|---:|---:|---|---:|---:|---:|\n")
            for r in rows:
                f.write("| %d | %d | %.4f (%.4f .. %.4f) | %.1f | %.4f | %.4f |\n" % (r["B"], r["T"], r["ms"], r["ms_range"][0], r["ms_range"][1], r["tflops"],
                                                                                 r["t256_scaled_ms"], r["sdpa_bf16_ms"]))
            if model:
                f.write("\nViT-B/16 eval forward, 384x128 stride 12 (%d tokens), batch %d: %.2f ms (%.2f .. %.2f) = %.1f images/s; arena %.2f GB\n"
                        % (model["tokens"], model["batch"], model["ms"], model["ms_range"][0], model["ms_range"][1], model["images_per_s"],
                           model["arena_bytes"] / 1e9))


if __name__ == "__main__":
    main()
