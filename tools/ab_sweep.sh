#!/bin/bash
# usage (GPU box): tools/ab_sweep.sh -- the pass A geometry variant of round 5 against the shipped build on one box (bench.py,
# HIP-event kernel times; build it first: tools/variant.sh pa_c2 gpa_sweep -DGPA_PA_C12=2)
cd "$GRAFT_REPO_ROOT" || exit 1
KERNEL=pass bash tools/gpu_variants.sh base pa_c2
