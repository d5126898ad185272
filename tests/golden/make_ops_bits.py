#!/usr/bin/env python3
"""Record the bits of the LayerNorm and attention operators: tests/golden/ops_parent_bits.json.

    python tests/golden/make_ops_bits.py --commit <commit the tree was built from> [--out FILE]

Needs a GPU.  Per case, SHA-256 digests of the raw bytes of every output and every gradient of one
public call of ``ops``: ``layer_norm``, ``layer_norm_pass``, ``add_layer_norm``,
``add_layer_norm_scaled``, ``cls_add_layer_norm``, ``attention``, ``attention_packed``,
``talking_heads_attention``, ``talking_heads_attention_packed`` (with ``relpos_bias`` and
``DropoutRng``).  That API exists on both sides of the change that gave each of the two families one
autograd Function, so the file is made by running this script, unchanged, on the PARENT of such a
change (or of a toolchain bump) -- never from the code under test.
tests/test_gpu_ops_bits.py::test_ops_bits_are_the_parent_ops recomputes the digests.

LayerNorm cases: C in {4, 192, 384, 768, 1024} (1, 1, 2, 3, 4 float4 chunks a lane; C = 4 leaves most
lanes idle) x M in {3, 37} (odd row counts, 37 a ragged last workgroup): plain, pass, add with a bf16
and with an fp32 addend, add with dropout 0.25; per C the scaled form at (B, N) = (3, 37) with and
without a rowscale that has a 0 entry, and the class-row form at (B, N) = (3, 5) with and without
dropout.  Every two-output form runs under three upstream patterns: gradients on both outputs, on the
stream only (y unused), on y only.

Attention cases, fp32 and bf16: self-attention B2 N17 H3 D64 unpacked and packed (plain, rotary, rotary
on a view one element past a 16-byte boundary, which the fused-rotary route refuses, dropout 0.25,
dropout + rotary), cross-attention Nq 1 x Nk 12, relative logits on a 7 x 7 grid H2 D32 (with and
without rotary), and talking heads B1 N50 H4 D48 with fp32 transforms (plain, rotary, the misaligned
view, and one parameter passed as both transforms), unpacked and packed.

The inputs are a function of the case's seed alone: np.random.RandomState on the host, rounded to the
dtype by torch on the CPU, then copied to the device.  A dropout case passes its own DropoutRng seeded
with the case's seed, so its masks are a function of the case.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
DEFAULT_OUT = os.path.join(HERE, "ops_parent_bits.json")

LN_C = (4, 192, 384, 768, 1024)
LN_M = (3, 37)
SCALED_BN = (3, 37)
CLS_BN = (3, 5)
PATTERNS = ("both", "stream", "y")      # which outputs of a two-output form carry an upstream gradient
RATE = 0.25
ROPE = 10000.0
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def cases():
    """``(key, kind, spec)`` of every recorded case; ``kind`` is 'ln', 'attn' or 'th'."""
    for C in LN_C:
        for M in LN_M:
            yield f"ln_plain_{M}x{C}", "ln", dict(form="plain", shape=(M, C))
            for form in ("pass", "add_bf16", "add_f32", "add_drop"):
                for pat in PATTERNS:
                    yield f"ln_{form}_{M}x{C}_{pat}", "ln", dict(form=form, shape=(M, C), pattern=pat)
        for form in ("scaled", "scaled_rows"):
            for pat in PATTERNS:
                yield (f"ln_{form}_{SCALED_BN[0]}x{SCALED_BN[1]}x{C}_{pat}", "ln",
                       dict(form=form, shape=SCALED_BN + (C,), pattern=pat))
        for form in ("cls", "cls_drop"):
            yield f"ln_{form}_{CLS_BN[0]}x{CLS_BN[1]}x{C}", "ln", dict(form=form, shape=CLS_BN + (C,))
    for dt in DTYPES:
        for packed in (False, True):
            p = "packed" if packed else "qkv"
            for form in ("plain", "rot", "rot_misaligned", "drop", "drop_rot"):
                yield (f"attn_{p}_{form}_b2_n17_h3_d64_{dt}", "attn",
                       dict(form=form, packed=packed, dims=(2, 17, 17, 3, 64), dt=dt))
            for form in ("plain", "rot", "rot_misaligned", "both"):
                yield (f"th_{p}_{form}_b1_n50_h4_d48_{dt}", "th",
                       dict(form=form, packed=packed, dims=(1, 50, 50, 4, 48), dt=dt))
        for form in ("plain", "rot", "drop", "drop_rot"):
            yield f"attn_qkv_{form}_b2_nq1_nk12_h4_d48_{dt}", "attn", dict(form=form, packed=False,
                                                                           dims=(2, 1, 12, 4, 48), dt=dt)
        for form in ("plain", "bias", "bias_rot"):
            yield f"attn_qkv_{form}_b1_7x7_h2_d32_{dt}", "attn", dict(form=form, packed=False,
                                                                      dims=(1, 49, 49, 2, 32), dt=dt, grid=(7, 7))


def digest(t: torch.Tensor) -> str:
    """SHA-256 of the tensor's elements in row-major order, as the device holds them."""
    raw = t.detach().contiguous().reshape(-1).cpu().view(torch.uint8).numpy().tobytes()
    return hashlib.sha256(raw).hexdigest()


def _seed(key: str) -> int:
    return zlib.crc32(key.encode())


class _Draw:
    """Seeded host values of one case, rounded to their dtype on the CPU, then copied to the device."""

    def __init__(self, key, dev):
        self.rs, self.dev = np.random.RandomState(_seed(key)), dev

    def __call__(self, shape, dtype=torch.float32, scale=1.0, shift=0.0, misaligned=False, grad=False):
        t = torch.from_numpy((scale * self.rs.randn(*shape) + shift).astype(np.float32)).to(dtype)
        if misaligned:   # the same values one element past the (16-byte aligned) start of a longer buffer
            buf = torch.empty(t.numel() + 1, dtype=dtype, device=self.dev)
            buf[1:].copy_(t.reshape(-1))
            t = buf[1:].view(shape)
            assert t.data_ptr() % 16 != 0
        else:
            t = t.to(self.dev)
        return t.requires_grad_(grad)


def _grads(outs, ups, leaves):
    """Digests of d(sum_i <outs_i, ups_i>) / d leaf for the named leaves; an output whose upstream
    gradient is None carries none (autograd sees it as unused)."""
    pairs = [(o, u) for o, u in zip(outs, ups) if u is not None]
    got = torch.autograd.grad([o for o, _ in pairs], list(leaves.values()), [u for _, u in pairs], allow_unused=True)
    return {"d" + name: digest(g) for name, g in zip(leaves, got) if g is not None}


def run_ln(ops, dev, key, form, shape, pattern="both"):
    draw = _Draw(key, dev)
    C = shape[-1]
    x = draw(shape, scale=3.0, shift=1.0, grad=True)
    gamma, beta = draw((C,), scale=0.25, shift=1.0, grad=True), draw((C,), grad=True)
    leaves = {"x": x, "gamma": gamma, "beta": beta}
    if form not in ("plain", "pass"):
        leaves["delta"] = delta = draw(shape, torch.float32 if form == "add_f32" else torch.bfloat16, grad=True)
    dropout = (RATE, ops.DropoutRng(_seed(key), dev)) if form.endswith("_drop") else None
    gx, gy = draw(shape), draw(shape, torch.bfloat16)
    if form == "plain":
        outs, ups = (ops.layer_norm(x, gamma, beta),), (gy,)
    elif form in ("cls", "cls_drop"):
        outs, ups = (ops.cls_add_layer_norm(x, delta, gamma, beta, dropout=dropout),), (gy[:, 0].contiguous(),)
    else:
        if form == "pass":
            outs = ops.layer_norm_pass(x, gamma, beta)
        elif form in ("scaled", "scaled_rows"):
            leaves["layerscale"] = ls = draw((C,), scale=0.25, shift=0.5, grad=True)
            rows = torch.tensor([0.0, 1.25, 1.25][:shape[0]], device=dev) if form == "scaled_rows" else None
            outs = ops.add_layer_norm_scaled(x, delta, gamma, beta, ls, rows)
        else:
            outs = ops.add_layer_norm(x, delta, gamma, beta, dropout=dropout)
        ups = {"both": (gx, gy), "stream": (gx, None), "y": (None, gy)}[pattern]
    out = {name: digest(o) for name, o in zip(("y",) if len(outs) == 1 else ("stream", "y"), outs)}
    out.update(_grads(outs, ups, leaves))
    return out


def run_attn(ops, dev, key, form, packed, dims, dt, grid=None):
    draw = _Draw(key, dev)
    B, Nq, Nk, H, D = dims
    td = DTYPES[dt]
    mis = form == "rot_misaligned"
    rotary = ROPE if "rot" in form else None
    dropout = (RATE, ops.DropoutRng(_seed(key), dev)) if "drop" in form else None
    if packed:
        qkv = draw((B, Nq, 3, H, D), td, misaligned=mis, grad=True)
        leaves = {"qkv": qkv}
        o = ops.attention_packed(qkv, rotary=rotary, dropout=dropout)
    else:
        q, k, v = (draw((B, n, H, D), td, misaligned=mis, grad=True) for n in (Nq, Nk, Nk))
        leaves = {"q": q, "k": k, "v": v}
        bias = None
        if grid is not None and "bias" in form:
            leaves["emb_h"] = eh = draw((2 * grid[0] - 1, D), scale=D ** -0.5, grad=True)
            leaves["emb_w"] = ew = draw((2 * grid[1] - 1, D), scale=D ** -0.5, grad=True)
            bias = ops.relpos_bias(q, eh, ew, grid) + (grid,)
        o = ops.attention(q, k, v, bias=bias, rotary=rotary, dropout=dropout)
    out = {"o": digest(o)}
    out.update(_grads((o,), (draw((B, Nq, H, D), td),), leaves))
    return out


def run_th(ops, dev, key, form, packed, dims, dt):
    draw = _Draw(key, dev)
    B, N, _, H, D = dims
    td = DTYPES[dt]
    mis = form == "rot_misaligned"
    rotary = ROPE if "rot" in form else None
    leaves = {"th1": draw((H, H), scale=0.3, shift=0.2, grad=True)}
    if form != "both":
        leaves["th2"] = draw((H, H), scale=0.3, shift=0.2, grad=True)
    th1, th2 = leaves["th1"], leaves.get("th2", leaves["th1"])
    if packed:
        leaves["qkv"] = qkv = draw((B, N, 3, H, D), td, misaligned=mis, grad=True)
        o = ops.talking_heads_attention_packed(qkv, th1, th2, rotary=rotary)
    else:
        q, k, v = (draw((B, N, H, D), td, misaligned=mis, grad=True) for _ in range(3))
        leaves.update(q=q, k=k, v=v)
        o = ops.talking_heads_attention(q, k, v, th1, th2, rotary=rotary)
    out = {"o": digest(o)}
    out.update(_grads((o,), (draw((B, N, H, D), td),), leaves))
    return out


RUN = {"ln": run_ln, "attn": run_attn, "th": run_th}


def record(ops, dev):
    """key -> {tensor name -> digest} of every case."""
    return {key: RUN[kind](ops, dev, key, **spec) for key, kind, spec in cases()}


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
    ap.add_argument("--commit", required=True, help="the commit the tree under measurement was built from")
    ap.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from sae_vision_amd import ops
    dev = torch.device("cuda:0")
    doc = {"made_from": a.commit, "toolchain": _toolchain(), "cases": record(ops, dev)}
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"[ops_bits] {len(doc['cases'])} cases -> {a.out}")


if __name__ == "__main__":
    main()
