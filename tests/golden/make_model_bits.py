#!/usr/bin/env python3
"""Record the bits of whole models: tests/golden/model_parent_bits.json.

    python tests/golden/make_model_bits.py --commit <commit the tree was built from> --out RUN1.json
    python tests/golden/make_model_bits.py --commit <the same> --out RUN2.json          (a second process)
    python tests/golden/make_model_bits.py --merge RUN1.json RUN2.json [--out FILE]

Needs a GPU.  Per case, SHA-256 digests of the logits (or the encoder output), of every parameter
gradient keyed by parameter name (``d<name>``; ``dinput`` for an encoder's stream) and, for CvT, of every
buffer after the call (``buf:<name>``).  Only the model classes and their call signatures are used, which
exist on both sides of a change to the Python glue of vit.py / cait.py / cvt.py / layers/, so the file is
made by running this script, unchanged, on the PARENT of such a change (or of a toolchain bump) -- never
from the code under test.  ``--merge`` keeps the tensors on which two runs agree and lists the others
under ``"unstable"``; it refuses a case that lost its output, and more than one unstable tensor in fifty.
tests/test_gpu_model_bits.py::test_model_bits_are_the_parent_models recomputes the digests.

Cases, all at batch 2 and 64 px, the smallest shapes that take every branch of the glue:
  * ``vit.ViT(10, 2, 3, 192, (16, 16), 64, 4, ...)`` (N = 17, C = 192, D = 64): bf16 training at
    (attn_dropout_rate, dropout_rate) = (0, 0) and (0.1, 0.25), bf16 evaluation, fp32 training at
    (0.1, 0.25), fp32 evaluation.
  * ``vit.Encoder`` called directly at the same width with rates (0.1, 0.25): bf16 and fp32 training with
    ``cls_only`` False and True, and bf16 with ``pos_added=True`` on a non-contiguous fp32 stream (the
    route is decided on the stream that enters the first block and held: framework LayerNorm throughout).
  * ``cait.CaiT(10, 2, 2, 4, 192, (16, 16), sd, 1.0, img_size=64)`` (trunk N = 16, class attention over 17
    tokens, H = 4, D = 48): bf16 training at sd 0 and 0.5, bf16 evaluation, fp32 training at 0.5, and a
    bf16 model with ``trunk_dtype=torch.float32``.
  * CvT, the tiny configuration of tests/test_gpu_cvt.py (sizes (1, 1, 2), heads (1, 2, 2), widths
    (32, 64, 64)): bf16 training, bf16 evaluation, fp32 training.

A case is a function of its key alone: the model is built on the CPU under ``torch.manual_seed(seed)``,
the parameters that start at 0 or 1 (head, class token, LayerScale, LayerNorm and BatchNorm scale / bias,
BatchNorm statistics) are moved off those values with seeded host values, and the model is moved to the
device; the input and the upstream gradient are seeded host values; ``ops.seed_dropout(seed)`` and
``torch.manual_seed(seed)`` (stochastic depth draws from torch's device generator) run before the call.
A stochastic-depth case takes the first seed at or after its own whose predicted draw leaves every branch a live
sample (the recorded fp32 cases then have no all-zero gradient; the bf16 case still has EncoderBlock_0's at zero).
"""
import argparse
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
from make_ops_bits import _Draw, _seed, _toolchain, digest  # noqa: E402

DEFAULT_OUT = os.path.join(HERE, "model_parent_bits.json")
BATCH, PX, CLASSES = 2, 64, 10
RATES = (0.1, 0.25)                       # (attn_dropout_rate, dropout_rate)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
CVT = ((1, 1, 2), (1, 2, 2), (32, 64, 64))   # stage sizes, heads, widths


def cases():
    """``(key, kind, spec)`` of every recorded case; ``kind`` is 'vit', 'encoder', 'cait' or 'cvt'."""
    yield "vit_bf16_train", "vit", dict(dt="bf16", rates=(0.0, 0.0), train=True)
    yield "vit_bf16_train_drop", "vit", dict(dt="bf16", rates=RATES, train=True)
    yield "vit_bf16_eval", "vit", dict(dt="bf16", rates=RATES, train=False)
    yield "vit_f32_train_drop", "vit", dict(dt="f32", rates=RATES, train=True)
    yield "vit_f32_eval", "vit", dict(dt="f32", rates=RATES, train=False)
    for dt in ("bf16", "f32"):
        for cls_only in (False, True):
            yield f"encoder_{dt}_train_{'cls' if cls_only else 'all'}", "encoder", dict(dt=dt, cls_only=cls_only)
    yield "encoder_bf16_train_pos_added_strided", "encoder", dict(dt="bf16", cls_only=False, strided=True)
    yield "cait_bf16_train_sd0", "cait", dict(dt="bf16", sd=0.0, train=True)
    yield "cait_bf16_train_sd0.5", "cait", dict(dt="bf16", sd=0.5, train=True)
    yield "cait_bf16_eval", "cait", dict(dt="bf16", sd=0.5, train=False)
    yield "cait_f32_train_sd0.5", "cait", dict(dt="f32", sd=0.5, train=True)
    yield "cait_bf16_trunk_f32_train_sd0.5", "cait", dict(dt="bf16", sd=0.5, train=True, trunk="f32")
    yield "cvt_bf16_train", "cvt", dict(dt="bf16", train=True)
    yield "cvt_bf16_eval", "cvt", dict(dt="bf16", train=False)
    yield "cvt_f32_train", "cvt", dict(dt="f32", train=True)


def _off_init(model, key, dev):
    """Move every parameter and buffer that starts at a constant off it, then the model to the device."""
    draw = _Draw(key + "/params", torch.device("cpu"))
    with torch.no_grad():
        for n, p in model.named_parameters():
            leaf = n.rsplit(".", 2)[-2:]
            norm = len(leaf) == 2 and leaf[0].startswith(("LayerNorm_", "BatchNorm_"))
            if n == "Dense_0.kernel":                                  # the zero-initialised head
                p.copy_(draw(p.shape, scale=0.125))
            elif leaf[-1] == "cls":
                p.copy_(draw(p.shape, scale=0.5))
            elif leaf[-1] == "layerscale":
                p.copy_(draw(p.shape, scale=0.25, shift=0.5))
            elif norm and leaf[1] == "scale":
                p.copy_(draw(p.shape, scale=0.3, shift=1.0))
            elif norm and leaf[1] == "bias":
                p.copy_(draw(p.shape, scale=0.3))
        for n, b in model.named_buffers():                             # BatchNorm statistics
            b.copy_(draw(b.shape, scale=0.2) if n.endswith("mean") else 1.0 + 0.5 * draw(b.shape).abs())
    return model.to(dev)


def _sd_seed(key, dev, model, rate):
    """The first seed, counting up from the case's, whose stochastic-depth draw keeps a sample alive in every
    branch and drops one somewhere: the model's joint draw is the first device draw of its forward,
    ``torch.rand((blocks, batch))`` (``cait.draw_stochastic_depth``).  At batch 2 and rate 0.5 most seeds drop
    both samples of some branch, whose parameters then take all-zero gradients."""
    blocks = sum(1 for m in model.modules() if getattr(m, "drop_rate", 0.0) > 0.0)
    seed = _seed(key)
    while blocks:
        torch.manual_seed(seed)
        alive = torch.floor(1.0 - rate + torch.rand((blocks, BATCH), device=dev, dtype=torch.float32)).cpu()
        if bool((alive.sum(1) > 0).all()) and bool((alive == 0).any()):
            break
        seed += 1
    return seed


def _run(ops, model, key, dev, call, x, train, leaves=None, seed=None):
    """One call of ``model`` on ``x`` and, when training, one backward from a seeded upstream gradient."""
    seed = _seed(key) if seed is None else seed
    ops.seed_dropout(seed)
    torch.manual_seed(seed)
    if not train:
        with torch.no_grad():
            out = {"out": digest(call(x))}
    else:
        y = call(x)
        y.float().backward(_Draw(key + "/upstream", dev)(tuple(y.shape)))
        out = {"out": digest(y)}
        out.update({"d" + n: digest(p.grad) for n, p in model.named_parameters() if p.grad is not None})
        out.update({"d" + n: digest(t.grad) for n, t in (leaves or {}).items()})
    out.update({"buf:" + n: digest(b) for n, b in model.named_buffers()})
    return out


def _build(key, make):
    torch.manual_seed(_seed(key))
    return make()


def run_vit(ops, dev, key, dt, rates, train):
    from sae_vision_amd import vit
    m = _build(key, lambda: vit.ViT(CLASSES, 2, 3, 192, (16, 16), PX, 4, DTYPES[dt], None, rates[0], rates[1]))
    x = _Draw(key, dev)((BATCH, PX, PX, 3))
    return _run(ops, _off_init(m, key, dev), key, dev, lambda t: m(t, is_training=train), x, train)


def run_encoder(ops, dev, key, dt, cls_only, strided=False):
    from sae_vision_amd import vit
    m = _build(key, lambda: vit.Encoder(17, 192, 2, 3, 4, DTYPES[dt], None, RATES[0], RATES[1]))
    x = _Draw(key, dev)((BATCH, 17, 384 if strided else 192), grad=True)
    view = x[..., :192] if strided else x
    assert view.is_contiguous() != strided
    return _run(ops, _off_init(m, key, dev), key, dev,
                lambda t: m(t, is_training=True, pos_added=strided, cls_only=cls_only), view, True, {"input": x})


def run_cait(ops, dev, key, dt, sd, train, trunk=None):
    from sae_vision_amd import cait
    m = _build(key, lambda: cait.CaiT(CLASSES, 2, 2, 4, 192, (16, 16), sd, 1.0, img_size=PX, dtype=DTYPES[dt],
                                      trunk_dtype=DTYPES[trunk] if trunk else None))
    x = _Draw(key, dev)((BATCH, PX, PX, 3))
    m = _off_init(m, key, dev)
    return _run(ops, m, key, dev, lambda t: m(t, is_training=train), x, train, seed=_sd_seed(key, dev, m, sd))


def run_cvt(ops, dev, key, dt, train):
    from sae_vision_amd import cvt
    m = _build(key, lambda: cvt.CvT(CLASSES, *CVT, dtype=DTYPES[dt]))
    x = _Draw(key, dev)((BATCH, PX, PX, 3))
    return _run(ops, _off_init(m, key, dev), key, dev, lambda t: m(t, is_training=train), x, train)


RUN = {"vit": run_vit, "encoder": run_encoder, "cait": run_cait, "cvt": run_cvt}


def record(ops, dev, only=None):
    """key -> {tensor name -> digest} of every case (of the case ``only``)."""
    return {key: RUN[kind](ops, dev, key, **spec) for key, kind, spec in cases() if only in (None, key)}


def merge(a, b):
    """The document of two runs of one tree: the digests on which they agree, the rest under "unstable"."""
    assert a["made_from"] == b["made_from"] and a["toolchain"] == b["toolchain"] and set(a["cases"]) == set(b["cases"])
    kept, unstable, total = {}, [], 0
    for key, da in a["cases"].items():
        db = b["cases"][key]
        assert set(da) == set(db), key
        total += len(da)
        kept[key] = {n: d for n, d in da.items() if db[n] == d}
        unstable += [f"{key}/{n}" for n in sorted(da) if db[n] != da[n]]
        if "out" not in kept[key]:
            raise SystemExit(f"{key}: the output differs between the two runs")
    if 50 * len(unstable) > total:
        raise SystemExit(f"{len(unstable)} of {total} tensors differ between the two runs: {unstable}")
    return {"made_from": a["made_from"], "toolchain": a["toolchain"], "cases": kept, "unstable": unstable}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", help="the commit the tree under measurement was built from")
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--only", metavar="KEY", help="run this case alone (for a launch trace) and write nothing")
    ap.add_argument("--merge", nargs=2, metavar="RUN", help="two recorded runs of one tree -> the committed file")
    a = ap.parse_args()
    if a.merge:
        doc = merge(*(json.load(open(p)) for p in a.merge))
    else:
        sys.path.insert(0, ROOT)
        from sae_vision_amd import ops
        got = record(ops, torch.device("cuda:0"), a.only)
        torch.cuda.synchronize()
        if a.only:
            print(f"[model_bits] {a.only}: {len(got[a.only])} tensors, out {got[a.only]['out']}")
            return
        if not a.commit:
            ap.error("--commit is required to record")
        doc = {"made_from": a.commit, "toolchain": _toolchain(), "cases": got}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"[model_bits] {len(doc['cases'])} cases, {sum(len(c) for c in doc['cases'].values())} tensors, "
          f"{len(doc.get('unstable', []))} unstable -> {a.out}")


if __name__ == "__main__":
    main()
