"""One definition per kernel across the translation units (CPU: ``nm`` over the build's objects).

A kernel template instantiated by two units is a weak symbol in both, each with its own device
code object; the host handle merges into one symbol and the body a launch reaches is then decided
by the order in which the runtime registers the two binaries.  Every test still passes, only the
register allocation of that kernel is undefined (this happened to
``attn_bwd2_dkdv_kernel<128, 4, 1, false, true>``, DESIGN.md "Translation units").  So: every
``__device_stub__`` function and every kernel handle is defined by exactly one object, and the
linked library holds exactly those kernels."""
import os
import re
import shutil
import subprocess
from collections import defaultdict

import build as B

STUB = "__device_stub__"


def _nm(path):
    nm = shutil.which("nm") or os.path.join(os.path.dirname(B.HIPCC), "..", "llvm", "bin", "llvm-nm")
    out = subprocess.run([nm, "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return [line.split(None, 2)[2] for line in out.splitlines() if len(line.split(None, 2)) == 3]


def _objects():
    objs = B.object_files()
    if not all(os.path.exists(o) for o in objs):
        B.build(force=True, verbose=False)
    return objs


def test_one_definition_per_kernel():
    owners = defaultdict(list)   # mangled symbol -> objects defining it
    for obj in _objects():
        for name in set(_nm(obj)):
            owners[name].append(os.path.basename(obj))
    stubs = {n for n in owners if STUB in n}
    assert len(stubs) > 200, len(stubs)
    # the handle carries the kernel's own name: the stub's with the prefix (and its length) taken out
    handles = {re.sub(r"(\d*)" + STUB, lambda m: str(int(m.group(1)) - len(STUB)) if m.group(1) else "", n)
               for n in stubs}
    assert len(handles) == len(stubs) and handles <= set(owners), sorted(handles - set(owners))
    kernel_syms = stubs | handles
    dup = {n: o for n, o in owners.items() if n in kernel_syms and len(o) != 1}
    assert not dup, dup
    lib_stubs = {n for n in _nm(B.OUT) if STUB in n}
    assert lib_stubs == stubs, (sorted(lib_stubs - stubs), sorted(stubs - lib_stubs))


def test_the_loss_is_one_kernel_family():
    """misc.hip holds the loss once (csrc/loss.h): ce_fwd_kernel<{__bf16, float}, {false, true}>,
    ce_mean_kernel<{false, true}>, ce_bwd_kernel<{__bf16, float}, {false, true}> (split on MIX after
    the timing check, profiles/loss_unify_ab.txt) and ce_accumulate_kernel, and no second copy of the
    formula for the one-label case (no kernel named smoothed_ce)."""
    (obj,) = [o for o in _objects() if os.path.basename(o) == "misc.hip.o"]
    syms = set(_nm(obj))
    assert not [n for n in syms if "smoothed_ce" in n and not n.startswith("sae_smoothed_ce_")]
    assert {"sae_smoothed_ce_fwd", "sae_smoothed_ce_bwd", "sae_mixed_ce_fwd", "sae_mixed_ce_bwd"} <= syms
    # Itanium names: sae::<kernel><template arguments>; DF16b is __bf16, f float, Lb0E / Lb1E false / true
    got = set()
    for n in syms:
        m = re.match(r"_ZN3sae\d+((?:[a-z0-9]+_)*ce_[a-z_]+_kernel)(?:I((?:DF16b|f)?(?:Lb[01]E)?)E)?Ev?", n)
        if m and STUB not in n:
            got.add((m.group(1), m.group(2) or ""))
    want = {(k, t + r) for k in ("ce_fwd_kernel", "ce_bwd_kernel") for t in ("DF16b", "f") for r in ("Lb0E", "Lb1E")}
    want |= {("ce_mean_kernel", "Lb0E"), ("ce_mean_kernel", "Lb1E"), ("ce_accumulate_kernel", "")}
    assert got == want, (sorted(got - want), sorted(want - got))
