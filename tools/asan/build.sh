#!/bin/bash
# Host AddressSanitizer build + run of the C ABI (tools/asan/capi_asan.cpp).  Device code is
# compiled as in build.py (its units and their flags); only the host side is instrumented (GPU
# ASan is unavailable on the pool).  CPU only: no GPU is touched.  Usage: tools/asan/build.sh [outdir]
set -euo pipefail
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${1:-/tmp/sae_asan}
mkdir -p "$OUT"
SRC="$ROOT/self-attention-experiments-vision_amd/csrc"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
COMMON=(--offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -fno-honor-nans -fno-slp-vectorize -I "$ROOT/include"
        -Xarch_host -fsanitize=address -Xarch_host -fno-omit-frame-pointer)
OBJS=()
PIDS=()
while IFS=$'\t' read -r src extra; do
  "$HIPCC" "${COMMON[@]}" $extra -c "$SRC/$src" -o "$OUT/${src%.hip}.o" &
  PIDS+=($!)
  OBJS+=("$OUT/${src%.hip}.o")
done < <(python3 "$ROOT/build.py" --list-units)
"$HIPCC" -O1 -g -std=c++17 -I "$ROOT/include" -Xarch_host -fsanitize=address -x c++ \
  -c "$ROOT/tools/asan/capi_asan.cpp" -o "$OUT/driver.o" &
PIDS+=($!)
for p in "${PIDS[@]}"; do wait "$p"; done
"$HIPCC" --offload-arch=gfx950 -fsanitize=address -fno-gpu-sanitize "${OBJS[@]}" "$OUT/driver.o" -o "$OUT/capi_asan"
ASAN_OPTIONS=detect_leaks=0:abort_on_error=0 "$OUT/capi_asan"
