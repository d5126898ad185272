#!/bin/bash
# One-box measurement of a round (run on the GPU box from the repo root):
#   bench JSON (--full: roofline, headlines, CPU baselines), rocprofv3 kernel stats of the SAME build
#   (training loop and attention bench), PMC passes for the DeiT-S training step and the ViT-B@384
#   attention headline.
# usage: tools/gpu_measure.sh <tag>     -> $SAE_OUT/<tag>_*   (SAE_OUT defaults to measure_out)
set -e
tag=${1:-r02g}
out=${SAE_OUT:-measure_out}
export TMPDIR=/tmp
mkdir -p $out
timeout -k 10 400 python -u bench.py --full > $out/${tag}_bench.json 2> $out/${tag}_bench.err
timeout -k 10 300 python -u bench.py --full --no-cpu-baseline --no-headline --model vit_b_patch16 --img-size 384 --batch 32 > $out/${tag}_bench_vitb16_384.json 2>> $out/${tag}_bench.err
timeout -k 10 300 python -u bench.py --full --no-cpu-baseline --no-headline --model cait_s_24 > $out/${tag}_bench_cait_s24.json 2>> $out/${tag}_bench.err
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $out/${tag}_prof_train -o run -- python3 bench.py --full --profile --steps 5 --warmup 3 > $out/${tag}_prof_train.log 2>&1
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $out/${tag}_prof_attn -o run -- python3 tools/attn_bench.py --iters 10 > $out/${tag}_prof_attn.log 2>&1
timeout -k 10 300 python3 tools/attn_bench.py --iters 20 > $out/${tag}_attn_bench.txt 2>&1
timeout -k 10 300 python3 tools/attn_bench.py --shapes bot14,bot7 --rel --iters 20 >> $out/${tag}_attn_bench.txt 2>&1
timeout -k 10 300 python3 tools/attn_bench.py --shapes cait_s24,cait_m24 --th --iters 20 >> $out/${tag}_attn_bench.txt 2>&1
tools/pmc.sh $out/${tag}_pmc_b384 python3 tools/attn_bench.py --shapes vitb384 --iters 3
tools/pmc.sh $out/${tag}_pmc_th python3 tools/attn_bench.py --shapes cait_s24 --th --iters 3
tools/pmc.sh $out/${tag}_pmc_th_m24 python3 tools/attn_bench.py --shapes cait_m24 --th --iters 3
tools/pmc.sh $out/${tag}_pmc_deit python3 tools/attn_bench.py --shapes deit_s --iters 3
echo ALL_DONE
