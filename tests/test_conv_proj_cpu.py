"""CPU tests of the CvT convolutional projection (depthwise 3x3 + BatchNorm): the SAME padding
table, the float64 reference's hand-written backward against autograd, the host predicate, and the
C ABI's symbols and refusals (validation runs on the host, before any GPU call)."""
import ctypes
import re
import subprocess
import types

import pytest
import torch

import _conv_proj_ref as R


@pytest.mark.parametrize("n,s,pads", [(14, 2, (0, 1)), (15, 2, (1, 1)), (1, 2, (1, 1)), (14, 1, (1, 1)),
                                      (1, 1, (1, 1)), (7, 1, (1, 1))])
def test_same_pads(n, s, pads):
    import sae_vision_amd.ops as ops
    assert ops.same_pads(n, 3, s) == pads
    assert R.same_pads(n, 3, s) == pads


@pytest.mark.parametrize("shape,s", [((2, 5, 7, 8), 1), ((2, 6, 4, 8), 2)])
def test_reference_backward_is_autograd(shape, s):
    g = torch.Generator().manual_seed(3)
    C = shape[-1]
    x = torch.randn(shape, dtype=torch.float64, generator=g, requires_grad=True)
    w = (torch.randn((3, 3, 1, C), dtype=torch.float64, generator=g) / 3).requires_grad_(True)
    gamma = (1 + 0.5 * torch.randn(C, dtype=torch.float64, generator=g)).requires_grad_(True)
    beta = (0.5 * torch.randn(C, dtype=torch.float64, generator=g)).requires_grad_(True)
    fw = R.forward(x, w, gamma, beta, s, 1e-5)
    dy = torch.randn(fw["y"].shape, dtype=torch.float64, generator=g)
    fw["y"].backward(dy)
    with torch.no_grad():
        bw = R.backward(x, w, gamma, fw, dy, s)
    for name, leaf in (("dx", x), ("dw", w), ("dgamma", gamma), ("dbeta", beta)):
        err = float((bw[name] - leaf.grad).abs().max() / leaf.grad.abs().max())
        assert err <= 1e-10, (name, err)


def _fake(shape, cuda=True, requires_grad=False):
    return types.SimpleNamespace(shape=tuple(shape), is_cuda=cuda, requires_grad=requires_grad)


def test_dwconv_bn_ok_decisions():
    import sae_vision_amd.ops as ops
    bf, f32 = torch.bfloat16, torch.float32
    ok = ops.dwconv_bn_ok
    assert ok(_fake((2, 14, 14, 368)), 3, 1, bf) and ok(_fake((2, 15, 15, 368)), 3, 2, bf)
    assert ok(_fake((2, 5, 7, 8)), 3, 2, bf) and ok(_fake((2, 5, 7, 4)), 3, 1, f32)
    assert ok(_fake((128, 56, 56, 64)), 3, 1, bf) and ok(_fake((3, 1, 3, 8)), 3, 2, f32)
    assert not ok(_fake((2, 5, 7, 8), cuda=False), 3, 1, bf)            # a GPU tensor
    assert not ok(torch.zeros(2, 5, 7, 8), 3, 1, f32)
    assert not ok(_fake((2, 5, 7, 8)), 5, 1, bf)                        # kernel 3 only
    assert not ok(_fake((2, 5, 7, 8)), 3, 3, bf)                        # stride 1 or 2
    assert not ok(_fake((2, 5, 7, 12)), 3, 1, bf)                       # C % 8 in bf16
    assert ok(_fake((2, 5, 7, 12)), 3, 1, f32)                          # ... C % 4 in fp32
    assert not ok(_fake((2, 5, 7, 6)), 3, 1, f32)
    assert not ok(_fake((2, 5, 7, 8)), 3, 1, torch.float16)
    assert not ok(_fake((5, 7, 8)), 3, 1, bf)
    # evaluation has no backward
    assert ok(_fake((2, 5, 7, 8), requires_grad=True), 3, 1, bf, training=True)
    assert not ok(_fake((2, 5, 7, 8), requires_grad=True), 3, 1, bf, training=False)
    assert ok(_fake((2, 5, 7, 8)), 3, 1, bf, training=False)
    assert not ok(_fake((2, 5, 7, 8)), 3, 1, bf, training=False, needs_grad=True)
    with torch.no_grad():
        assert ok(_fake((2, 5, 7, 8), requires_grad=True), 3, 1, bf, training=False)


NAMES = ("sae_dwconv_bn_workspace_bytes", "sae_dwconv_bn_fwd", "sae_dwconv_bn_bwd")


def test_symbols_declared_and_exported():
    import sae_vision_amd
    from sae_vision_amd import _lib as L
    lib = sae_vision_amd.load_library()
    assert set(NAMES) <= set(L.EXPORTED_SYMBOLS)
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (sae_\w+)", nm))
    assert set(NAMES) <= exported
    assert lib.sae_abi_version() == 1
    assert ctypes.sizeof(L.SaeDwconvDesc) == 9 * 4
    assert lib.sae_dwconv_bn_workspace_bytes(2, 5, 7, 8, 1) > 0
    assert lib.sae_dwconv_bn_workspace_bytes(2, 5, 7, 8, 3) == 0
    # partial rows (a few MB at most) and the backward's dt, one fp32 per output element at most
    assert lib.sae_dwconv_bn_workspace_bytes(128, 56, 56, 64, 1) <= (16 << 20) + 128 * 56 * 56 * 64 * 4


def _desc(L, **kw):
    f = dict(batch=2, height=5, width=7, channels=8, stride=1, dtype=L.SAE_DTYPE_BF16, training=1, momentum=0.9,
             eps=1e-5)
    f.update(kw)
    return L.SaeDwconvDesc(**f)


def _call(lib, which, d, null=None):
    """fwd / bwd with dummy non-null (aligned, never dereferenced: every refusal is host-side) pointers."""
    p = [ctypes.c_void_p(64)] * (11 if which == "fwd" else 12)
    if null is not None:
        p[null] = None
    fn = lib.sae_dwconv_bn_fwd if which == "fwd" else lib.sae_dwconv_bn_bwd
    return fn(None, ctypes.byref(d) if d is not None else None, *p)


@pytest.mark.parametrize("which", ["fwd", "bwd"])
@pytest.mark.parametrize("kw,code,msg", [
    (dict(batch=0), "EINVAL", "must be >= 1"),
    (dict(height=-1), "EINVAL", "height -1"),
    (dict(channels=0), "EINVAL", "must be >= 1"),
    (dict(stride=3), "EUNSUPPORTED", "stride 3"),
    (dict(stride=0), "EUNSUPPORTED", "stride 0"),
    (dict(channels=12), "EUNSUPPORTED", "multiple of 8 in bf16"),
    (dict(channels=6, dtype=0), "EUNSUPPORTED", "multiple of 4 in fp32"),
    (dict(dtype=7), "EINVAL", "dtype 7"),
])
def test_validation_errors(which, kw, code, msg):
    import sae_vision_amd
    from sae_vision_amd import _lib as L
    lib = sae_vision_amd.load_library()
    rc = _call(lib, which, _desc(L, **kw))
    assert rc == getattr(L, "SAE_" + code), (rc, lib.sae_last_error().decode())
    assert msg in lib.sae_last_error().decode()
    assert f"dwconv_bn_{which}" in lib.sae_last_error().decode()


def test_null_arguments_and_eval_backward():
    import sae_vision_amd
    from sae_vision_amd import _lib as L
    lib = sae_vision_amd.load_library()
    assert _call(lib, "fwd", None) == L.SAE_EINVAL and "NULL descriptor" in lib.sae_last_error().decode()
    for which, n in (("fwd", 11), ("bwd", 12)):
        for i in range(n):
            assert _call(lib, which, _desc(L), null=i) == L.SAE_EINVAL, (which, i)
            assert "dwconv_bn_" + which in lib.sae_last_error().decode()
    # evaluation: t, mean, rstd, workspace are optional in the forward -- x is not
    assert _call(lib, "fwd", _desc(L, training=0), null=0) == L.SAE_EINVAL
    assert "NULL x" in lib.sae_last_error().decode()
    assert _call(lib, "bwd", _desc(L, training=0)) == L.SAE_EUNSUPPORTED
    assert "training = 0" in lib.sae_last_error().decode()
    # misaligned pointer
    p = [ctypes.c_void_p(64)] * 11
    p[0] = ctypes.c_void_p(68)
    assert lib.sae_dwconv_bn_fwd(None, ctypes.byref(_desc(L)), *p) == L.SAE_EINVAL
    assert "16-byte" in lib.sae_last_error().decode()
