#!/usr/bin/env python3
"""gpurun_out/gemm_launch_table.txt + gemm_dump_bench.json -> profiles/<ROUND>_gemm_launches_in_step.md and
gpurun_out/prof_eval/ (scripts/profile_eval_forward.sh) -> profiles/<ROUND>_eval_forward.{md,_kernel_stats.csv,_pmc_traffic.json}."""
import json, os, shutil
RND = os.environ.get("ROUND", "r05")
n = RND[1:].lstrip("0")

b = json.loads(open("gpurun_out/gemm_dump_bench.json").read().strip().splitlines()[-1])
r = b["roofline"]
tab = open("gpurun_out/gemm_launch_table.txt").read().rstrip()
open("profiles/%s_gemm_launches_in_step.md" % RND, "w").write("""# Round %s -- every GEMM launch INSIDE the train step against its own roof

Produced on an MI355X box by

    DALI_GEMM_PROFILE_DUMP=gemm_launches.csv python bench.py --full --steps 5 --warmup 3 --no-cpu-baseline --no-distance --no-vit --no-epoch
    python scripts/gemm_launch_table.py gemm_launches.csv 3

(`bench.py`'s event-bracketed profile steps: every `igemm_*` / `fused1x1_persist` launch of three consecutive steps between two HIP events on the launch
stream, grouped by signature).  Step of this run: %.3f ms, GEMM launches %.3f ms per step (forward + data gradient %.3f, weight gradient %.3f).
`roof us` = max(FLOPs / 2.5 PFLOP/s, algorithmic bytes / 6 TB/s) of the launch (operand + output + residual + mask bytes, weights left out);
`over roof` = microseconds per step above that roof, the table is sorted by it.  `fused=1`: the bn3 + residual + ReLU + mask output stage rides in the
launch (K <= 256: the persistent streaming kernel of `csrc/fused1x1.h`); `lin=1`: column sums (Gram scheme) ride on the weight gradient, or a
two-operand-tensor GEMM (`X2`) on the data-gradient side; `sub=2`: the four parity classes of a stride-2 data gradient in one launch.
Against `r04_gemm_launches_in_step.md` (same command): the `fused=1` rows went from 131.9 / 166.9 us (K = 64, plain / `lin=1`), 78.8 / 94.9 (K = 128),
50.0 / 54.6 (K = 256) to the rows below (about 1.1 / 1.3 / 1.7 x their roofs; the verdict's <= 1.5 x holds for layer1 / layer2);
the K = 512 rows (layer4, 125-139 us against a 50 us roof) stay on the tile-per-workgroup kernels: a 128 x 128 tile's 32 KB per k-step against the
~50 KB per microsecond a CU's L2 -> LDS path delivers (docs/experiments.md, round 5).

```
%s
```
""" % (n, b["ms_per_step"], r["kernel_ms_per_step"], r["by_class_ms_per_step"]["conv_fwd_dgrad"], r["by_class_ms_per_step"]["wgrad"], tab))

src = "gpurun_out/prof_eval"
pm = json.load(open(src + "/pmc_traffic.json"))
plain = [l for l in open(src + "/plain.txt").read().splitlines() if "eval forward" in l]
ks = open(src + "/kstats.txt").read().rstrip().splitlines()
md = open(src + "/pmc_traffic.md").read().rstrip()
tot = pm["all_kernels_hbm_bytes_per_step"]
open("profiles/%s_eval_forward.md" % RND, "w").write("""# Round %s -- inference forward (extractFeatures' batch of 500, `getFeatures.py:56-67`) kernel profile

Produced by `bash scripts/profile_eval_forward.sh` on an MI355X box: `python scripts/time_eval_forward.py 500 20`, the same under
`rocprofv3 --kernel-trace --stats`, and under `--pmc FETCH_SIZE` / `--pmc WRITE_SIZE`,
each in its own run (4 timed + 3 warm-up forwards per process); summaries by `scripts/kstats.py`, `scripts/pmc_traffic.py`, `scripts/make_profile_extra_md.py`.

```
%s
```

HBM traffic of one forward of 500 images (PMC; %s): **%.2f GB = %.1f MB per image**;
per family: %s.

## Per-kernel summary (23 forwards in the process)

```
%s
```

## Largest movers of bytes (MB per forward)

%s
""" % (n, "\n".join(plain), pm["corrections"], tot / 1e9, tot / 500 / 1e6, json.dumps(pm["per_family_bytes_per_step"]), "\n".join(l[:170] for l in ks[:22]), md))
shutil.copy(src + "/kernel_stats.csv", "profiles/%s_eval_forward_kernel_stats.csv" % RND)
shutil.copy(src + "/pmc_traffic.json", "profiles/%s_eval_forward_pmc_traffic.json" % RND)
print("wrote profiles/%s_gemm_launches_in_step.md, profiles/%s_eval_forward.md" % (RND, RND))
