"""Whole models give the bits they gave before their Python glue (vit.py, cait.py, cvt.py, layers/) was
rewritten on layers/stream.py: the same kernels, launched in the same order with the same arguments."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu


def _model_bits():
    """tests/golden/make_model_bits.py as a module: the cases, their seeded models and inputs, the digest."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_model_bits.py")
    spec = importlib.util.spec_from_file_location("make_model_bits", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_model_bits_are_the_parent_models(dev):
    """The logits (or encoder output), every parameter gradient and, for CvT, every buffer after the call
    have the SHA-256 digests tests/golden/model_parent_bits.json records, for ViT, ``vit.Encoder`` called
    directly (``cls_only``, and ``pos_added`` on a non-contiguous stream: the framework route held for the
    whole encoder), CaiT and CvT, in bf16 and fp32, training (dropout, stochastic depth) and evaluation.

    The file is made by tests/golden/make_model_bits.py, which uses only the model classes and their call
    signatures, on the PARENT of the change that gave each block one body: two recordings in two
    processes agreed on all 772 tensors of the 18 cases (``"unstable"`` is empty).  When the toolchain
    changes the bits, regenerate it on the parent of the toolchain bump (check that commit out, build it
    with the new toolchain, run the script there twice and ``--merge``, copy the file here): never from
    the code under test."""
    from sae_vision_amd import ops
    M = _model_bits()
    with open(os.path.join(os.path.dirname(M.__file__), "model_parent_bits.json")) as f:
        doc = json.load(f)
    want, unstable = doc["cases"], set(doc["unstable"])
    got = M.record(ops, dev)
    assert sorted(got) == sorted(want)
    wrong = [(key, name) for key in want for name in sorted(set(got[key]) | set(want[key]))
             if f"{key}/{name}" not in unstable and got[key].get(name) != want[key].get(name)]
    for key, name in wrong:
        print(key, name)
    assert not wrong, wrong
