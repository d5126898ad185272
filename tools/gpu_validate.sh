#!/bin/bash
# Validation pass on the GPU box (run from the repo root): GPU suite, smoke(), the bench with --full.
#   tools/gpu_validate.sh <tag>   -> $SAE_OUT/<tag>_{tests.log,smoke.log,bench.json,bench.err}
#   (SAE_OUT defaults to measure_out)
set -o pipefail
tag=${1:-val}
out=${SAE_OUT:-measure_out}
export TMPDIR=/tmp
mkdir -p $out
timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread \
  > $out/${tag}_tests.log 2>&1 || { echo "TESTS FAILED"; tail -30 $out/${tag}_tests.log; exit 1; }
tail -3 $out/${tag}_tests.log
timeout -k 10 200 python -u -c "import __graft_entry__ as g; g.smoke()" > $out/${tag}_smoke.log 2>&1 \
  || { echo "SMOKE FAILED"; tail -20 $out/${tag}_smoke.log; exit 1; }
tail -1 $out/${tag}_smoke.log
timeout -k 10 300 python -u bench.py --full > $out/${tag}_bench.json 2> $out/${tag}_bench.err \
  || { echo "BENCH FAILED"; tail -20 $out/${tag}_bench.err; exit 1; }
cat $out/${tag}_bench.json
