#!/bin/bash
# A/B of two library builds on one box: bash scripts/ab_step.sh <lib A> <lib B> [reps] [bench args ...]; A and B alternate, 30 timed steps each.
# One line per run: the ResNet-50 train step, and where the run has them (no --no-vit / --no-epoch) the ViT-B/16 step and the eval forward.
A=$1; B=$2; REPS=${3:-3}; shift 3
for rep in $(seq 1 $REPS); do
for L in $A $B; do
DALIID_LIB=$PWD/$L timeout -k 10 300 python bench.py --full --steps 30 --warmup 5 --no-cpu-baseline --no-distance "$@" 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('$L: ms_per_step', d['ms_per_step'], 'vit_ms_per_step', d.get('vit', {}).get('ms_per_step'), 'eval_ms_per_batch', d.get('epoch', {}).get('inference_forward_only', {}).get('ms_per_batch'), 'gemm', d['roofline']['kernel_ms_per_step'], d['roofline']['by_class_ms_per_step'])" || exit 124
done
done
