"""The LayerNorm and attention operators of ops.py give the bits of the operators they replaced, and the
backward of a two-output LayerNorm form whose ``y`` nobody reads."""
import importlib.util
import json
import os

import pytest
import torch

from _util import rel_err

pytestmark = pytest.mark.gpu


def _ops_bits():
    """tests/golden/make_ops_bits.py as a module: the cases, their seeded inputs and the digest."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_ops_bits.py")
    spec = importlib.util.spec_from_file_location("make_ops_bits", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_ops_bits_are_the_parent_ops(dev):
    """Every output and gradient of every form of the public LayerNorm and attention calls has the
    SHA-256 digest tests/golden/ops_parent_bits.json records: the bits of the five LayerNorm Functions
    and the packed / unpacked Function pairs ops.py had before each family became one Function.

    The file is made by tests/golden/make_ops_bits.py, which uses only public API older than that
    change.  When the toolchain changes the bits, regenerate it on the PARENT of the toolchain bump
    (check that commit out, build it with the new toolchain, run the script there, copy the file
    here): never from the code under test."""
    from sae_vision_amd import ops
    M = _ops_bits()
    with open(os.path.join(os.path.dirname(M.__file__), "ops_parent_bits.json")) as f:
        want = json.load(f)["cases"]
    got = M.record(ops, dev)
    assert sorted(got) == sorted(want)
    wrong = [(key, name) for key in got for name in sorted(set(got[key]) | set(want[key]))
             if got[key].get(name) != want[key].get(name)]
    assert not wrong, wrong


@pytest.mark.parametrize("form", ["add", "pass"])
def test_layer_norm_unused_y_backward(dev, form):
    """A gradient on the residual stream only: the LayerNorm backward kernel runs with dy = 0, so
    dx = 0 * rstd + dxin is the upstream gradient bit for bit, dgamma and dbeta are exactly zero, and the
    addend's gradient is the upstream gradient rounded to bf16 (the file test_gpu_ln.py's bf16 bar)."""
    import sae_vision_amd.ops as ops
    M, C = 37, 192
    g = torch.Generator(device=dev).manual_seed(M + C)
    x = (torch.randn(M, C, device=dev, generator=g) * 3 + 1).requires_grad_()
    gamma = (torch.rand(C, device=dev, generator=g) + 0.5).requires_grad_()
    beta = torch.randn(C, device=dev, generator=g).requires_grad_()
    delta = torch.randn(M, C, device=dev, generator=g).to(torch.bfloat16).requires_grad_()
    dxo = torch.randn(M, C, device=dev, generator=g)
    if form == "add":
        xo, _ = ops.add_layer_norm(x, delta, gamma, beta)
    else:
        xo, _ = ops.layer_norm_pass(x, gamma, beta)
    xo.backward(dxo)
    assert torch.equal(x.grad, dxo)
    assert torch.count_nonzero(gamma.grad) == 0 and torch.count_nonzero(beta.grad) == 0
    if form == "add":
        assert delta.grad.dtype == torch.bfloat16
        assert rel_err(delta.grad.float(), dxo.double().cpu().numpy()) <= 2e-2
