#!/bin/bash
# Instruction histogram of one kernel (mangled-name substring) of the HIP library, over every
# translation unit of build.py with its flags.
root=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p /tmp/isa && cd /tmp/isa && rm -f ./*.s
python3 "$root/build.py" --list-units | while IFS=$'\t' read -r src extra; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-honor-nans -fno-slp-vectorize $extra -I "$root/include" \
    -c "$root/self-attention-experiments-vision_amd/csrc/$src" -save-temps -o "/tmp/isa/$src.o" 2>/dev/null
done
python3 - "$1" <<'PY'
import glob, sys, re
from collections import Counter
pat = sys.argv[1]
for f in sorted(glob.glob('/tmp/isa/*-hip-amdgcn-amd-amdhsa-gfx950.s')):
    s = open(f).read()
    for name in re.findall(r'^(_Z\S+):', s, re.M):
        if pat not in name: continue
        i = s.index(name + ':'); j = s.index('.Lfunc_end', i)
        lines = [l.strip() for l in s[i:j].split('\n') if l.strip() and not l.strip().startswith(('.', ';', '_Z'))]
        c = Counter(l.split()[0] for l in lines)
        print(name, 'total', len(lines))
        print('  ', ', '.join(f'{k}:{v}' for k, v in c.most_common(45)))
PY
