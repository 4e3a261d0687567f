"""Timing of the head-dim-96 attention forward (attention_fwd_long_kernel<96, 128>) at H = 8, ViT-Small's heads: (B, T) = (500, 129) = 256x128
at stride 16, (500, 211) = stride 12, (500, 311) = 384x128 at stride 12, with the scale ViT-Small uses (768 ** -0.5); the yardstick, measured in
the same run on the same GPU, is torch.nn.functional.scaled_dot_product_attention on bf16 [B, H, T, 96] operands with the same scale.  Then the
whole eval forward of ViT-Small and DeiT-Small at 256x128 / stride 16, batch 500, in images/s.  Timing as scripts/bench_attention_long.py
(HIP-event windows after WARM warm-ups, median and range of WINDOWS windows; ATT_INNER = 1000 launches and MODEL_INNER = 30 forwards per
window).  One JSON line per result; MD=path appends a markdown table.  SKIP_MODEL=1 leaves the whole-model part out.  There is no target: the
SDPA ratio says whether a one-pass head-dim-96 kernel for T <= 256 would be worth writing."""
import json
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from bench_attention_long import timed
from daliid_amd import ops_vit as V

bf16 = torch.bfloat16
H, HD, SCALE = 8, 96, 768 ** -0.5
# windows of a few tenths of a second: 1000 launches of 0.2 .. 0.5 ms, 30 forwards of 7 .. 10 ms
ATT_INNER, MODEL_INNER = int(os.environ.get("ATT_INNER", 1000)), int(os.environ.get("MODEL_INNER", 30))


def attention_case(B, T, g):
    qkv = torch.randn(B * T, 3 * H * HD, device="cuda", generator=g).to(bf16)
    q, k, v = (t.contiguous() for t in qkv.reshape(B, T, 3, H, HD).permute(2, 0, 3, 1, 4))
    ours = timed(lambda: V.attention_fwd(qkv, B, T, H, SCALE), inner=ATT_INNER)
    sdpa = timed(lambda: F.scaled_dot_product_attention(q, k, v, scale=SCALE), inner=ATT_INNER)
    flops = 4.0 * B * H * T * T * HD                      # Q K^T and P V
    r = {"what": "attention_fwd_hd96", "B": B, "T": T, "H": H, "ms": round(ours[0], 4), "ms_range": [round(ours[1], 4), round(ours[2], 4)],
         "tflops": round(flops / ours[0] / 1e9, 1), "sdpa_bf16_ms": round(sdpa[0], 4), "sdpa_range": [round(sdpa[1], 4), round(sdpa[2], 4)],
         "ours_over_sdpa": round(ours[0] / sdpa[0], 3)}
    print(json.dumps(r), flush=True)
    return r


def model_case(name, batch=500, size=(256, 128), stride=16):
    from daliid_amd import make_models
    cfg = types.SimpleNamespace(
        MODEL=types.SimpleNamespace(NAME="transformer", JPM=False, LAST_STRIDE=1, PRETRAIN_PATH="", PRETRAIN_CHOICE="none", COS_LAYER=False,
                                    NECK="bnneck", TRANSFORMER_TYPE=name, SIE_CAMERA=False, SIE_VIEW=False, SIE_COE=3.0, STRIDE_SIZE=stride,
                                    DROP_PATH=0.0, DROP_OUT=0.0, ATT_DROP_RATE=0.0, ID_LOSS_TYPE="softmax", RE_ARRANGE=False),
        TEST=types.SimpleNamespace(NECK_FEAT="after"), INPUT=types.SimpleNamespace(SIZE_TRAIN=size))
    model = make_models.make_model(cfg, 10, 0, 0, seed=1).eval()
    x = torch.randn(batch, 3, *size, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    with torch.no_grad():
        med, lo, hi = timed(lambda: model(x), inner=MODEL_INNER, windows=5, warm=2)
    r = {"what": "eval_forward", "model": name, "size": list(size), "stride": stride, "tokens": model.num_tokens, "batch": batch, "ms": round(med, 2),
         "ms_range": [round(lo, 2), round(hi, 2)], "images_per_s": round(batch / med * 1e3, 1), "arena_bytes": int(model._plan(batch).arena_bytes)}
    print(json.dumps(r), flush=True)
    return r


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_attention_hd96: needs the GPU (no CPU timing is meaningful)")
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = [attention_case(B, T, g) for B, T in ((500, 129), (500, 211), (500, 311))]
    models = [] if os.environ.get("SKIP_MODEL") else [model_case(n) for n in ("vit_small_patch16_224_TransReID", "deit_small_patch16_224_TransReID")]
    if os.environ.get("MD"):
        with open(os.environ["MD"], "a") as f:
            f.write("\n| B | T | ms per launch (range) | TFLOP/s | SDPA bf16, ms (range) | ours / SDPA |\n|---:|---:|---|---:|---|---:|\n")
            for r in rows:
                f.write("| %d | %d | %.4f (%.4f .. %.4f) | %.1f | %.4f (%.4f .. %.4f) | %.2f |\n"
                        % (r["B"], r["T"], r["ms"], r["ms_range"][0], r["ms_range"][1], r["tflops"], r["sdpa_bf16_ms"], r["sdpa_range"][0],
                           r["sdpa_range"][1], r["ours_over_sdpa"]))
            for m in models:
                f.write("\n%s eval forward, %dx%d stride %d (%d tokens), batch %d: %.2f ms (%.2f .. %.2f) = %.1f images/s; arena %.2f GB\n"
                        % (m["model"], m["size"][0], m["size"][1], m["stride"], m["tokens"], m["batch"], m["ms"], m["ms_range"][0], m["ms_range"][1],
                           m["images_per_s"], m["arena_bytes"] / 1e9))


if __name__ == "__main__":
    main()
