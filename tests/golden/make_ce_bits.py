#!/usr/bin/env python3
"""Record the bits of the one-label training loss: tests/golden/ce_parent_bits.json.

    python tests/golden/make_ce_bits.py --commit <commit the library was built from> [--out FILE]

Needs a GPU.  Per case, SHA-256 digests of the raw bytes of ``loss`` (fp32 scalar), ``row_loss`` (fp32
[R]) and ``dlogits`` (the logits' dtype, [R, K] contiguous, upstream gradient 0.6).  ``loss`` and
``dlogits`` come from ``ops.smoothed_cross_entropy``, ``row_loss`` from the no-partner form of
``ops.mixed_cross_entropy_rows``: API that exists on both sides of the change that made the smoothed
loss a special case of the mixed one, so the file is made by running this script, unchanged, on the
PARENT of such a change (or of a toolchain bump) -- never from the code under test.
tests/test_gpu_mixed_loss.py::test_ce_bits_are_the_parent_kernels recomputes the digests through every
form of the one-label loss.

Cases: the six SHAPES of tests/test_gpu_mixed_loss.py (K < 5, K < 256, K a multiple of 256, R = 1,
R > 256 so the mean's per-thread range exceeds one row, and the bench shape 128 x 1000) and a
row-strided view (64 rows, K = 1000 of pitch 1024), each in bf16 and fp32 at alpha 0.1 and 0.  The
inputs are a function of the seed alone: np.random.RandomState on the host, rounded to the dtype by
torch on the CPU, then copied to the device.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
DEFAULT_OUT = os.path.join(HERE, "ce_parent_bits.json")

# (R, K, pitch): pitch > K is a row-strided view of a [R, pitch] buffer
SHAPES = [(128, 1000, 1000), (7, 10, 10), (300, 37, 37), (1, 1000, 1000), (4, 512, 512), (5, 3, 3),
          (64, 1000, 1024)]
DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}
ALPHAS = (0.1, 0.0)
UPSTREAM = 0.6


def cases():
    """(key, R, K, pitch, dtype, alpha) of every recorded case."""
    for R, K, pitch in SHAPES:
        for name, dt in DTYPES.items():
            for alpha in ALPHAS:
                yield f"{R}x{K}_ld{pitch}_{name}_a{alpha}", R, K, pitch, dt, alpha


def case_inputs(dev, R, K, pitch, dt):
    """``(x, y0, y1)``: logits [R, K] of row pitch ``pitch`` on ``dev``, labels, and partner labels (for
    the ratio == 1 form, which must not feel them).  A function of (R, K, pitch) alone."""
    rs = np.random.RandomState(100003 * R + 101 * K + pitch)
    buf = torch.from_numpy((3 * rs.randn(R, pitch)).astype(np.float32)).to(dt).to(dev)
    y0 = torch.from_numpy(rs.randint(0, K, R).astype(np.int64)).to(dev)
    y1 = torch.from_numpy(rs.randint(0, K, R).astype(np.int64)).to(dev)
    x = buf[:, :K]
    assert x.stride(0) == pitch and x.is_contiguous() == (pitch == K)
    return x, y0, y1


def digest(t: torch.Tensor) -> str:
    """SHA-256 of the tensor's elements in row-major order, as the device holds them."""
    raw = t.detach().contiguous().reshape(-1).cpu().view(torch.uint8).numpy().tobytes()
    return hashlib.sha256(raw).hexdigest()


def loss_and_grad(fn, x):
    """``fn`` on a leaf that keeps x's strides (the kernels read a strided view in place): the loss
    and d(UPSTREAM * loss) / dx."""
    leaf = x.detach().requires_grad_(True)
    out = fn(leaf)
    (UPSTREAM * out).backward()
    return out.detach(), leaf.grad


def recorded_forms(ops, x, y0, alpha):
    """The digests this script records, from the API common to both sides."""
    loss, dx = loss_and_grad(lambda t: ops.smoothed_cross_entropy(t, y0, alpha), x)
    row_loss = ops.mixed_cross_entropy_rows(x, y0, None, None, alpha, False)[2]
    return {"loss": digest(loss), "row_loss": digest(row_loss), "dlogits": digest(dx)}


def _toolchain():
    out = {"torch": torch.__version__, "hip": torch.version.hip, "device": torch.cuda.get_device_name(0)}
    sys.path.insert(0, ROOT)
    import build as B
    try:
        v = subprocess.run([B.HIPCC, "--version"], capture_output=True, text=True, check=True).stdout.splitlines()
        out["hipcc"] = [line for line in v if "HIP version" in line or "clang version" in line]
    except (OSError, subprocess.CalledProcessError) as e:
        out["hipcc"] = [f"unavailable: {e}"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library under measurement was built from")
    ap.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from sae_vision_amd import ops
    dev = torch.device("cuda:0")
    doc = {"made_from": a.commit, "toolchain": _toolchain(), "upstream_gradient": UPSTREAM, "cases": {}}
    for key, R, K, pitch, dt, alpha in cases():
        x, y0, _ = case_inputs(dev, R, K, pitch, dt)
        doc["cases"][key] = recorded_forms(ops, x, y0, alpha)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"[ce_bits] {len(doc['cases'])} cases -> {a.out}")


if __name__ == "__main__":
    main()
