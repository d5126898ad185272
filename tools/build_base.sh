#!/bin/bash
# Build the library from a git revision's csrc (default HEAD) as <pkg>/libsae_attn_base.so, for
# same-box A/B runs against the working tree (load it with SAE_ATTN_LIB=<that path>).  The units
# and their flags are that revision's: its `build.py --list-units`, or, for a revision from before
# the option, every .hip with the VGPR-form MFMA flag on capi.hip alone.
set -e
cd "$(dirname "$0")/.."
rev=${1:-HEAD}
tmp=$(mktemp -d)
git archive "$rev" build.py self-attention-experiments-vision_amd/csrc include | tar -x -C "$tmp"
src="$tmp/self-attention-experiments-vision_amd/csrc"
units=$(python3 "$tmp/build.py" --list-units 2>/dev/null) || {
  units=$(for f in "$src"/*.hip; do
    f=$(basename "$f"); [ "$f" = capi.hip ] && printf '%s\t%s\n' "$f" "-mllvm -amdgpu-mfma-vgpr-form=1" || printf '%s\t\n' "$f"
  done)
}
common=(/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function
        -fno-honor-nans -fno-slp-vectorize -I "$tmp/include")
objs=()
while IFS=$'\t' read -r f extra; do
  "${common[@]}" $extra -c "$src/$f" -o "$src/$f.o" &
  objs+=("$src/$f.o")
done <<< "$units"
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC "${objs[@]}" -o self-attention-experiments-vision_amd/libsae_attn_base.so
rm -rf "$tmp"
echo "built libsae_attn_base.so from $rev"
