"""GPU tests of the CvT convolutional token embedding: the window-matrix kernels
(sae_conv_window_gather / _scatter) bit for bit against the unfold / fold of _cvt_ref.py, and
``ops.conv_tokens`` (gather + the project's GEMMs + scatter) against the float64 convolution and, in
bf16, the framework route it replaces (ConvTokenEmbedBlock._framework_conv)."""
import copy
import functools

import numpy as np
import pytest

import _cvt_ref as R
from _util import TOL, randn, rel_err

pytestmark = pytest.mark.gpu

# (B, H, W, Cin, E, k, s): the smallest shapes at which each index path can go wrong
SHAPES = [
    (2, 9, 11, 3, 16, 7, 4),       # Cin = 3: the element path, Kp = 152 > K = 147, pads (3, 3) / (2, 2)
    (2, 8, 8, 3, 16, 7, 4),        # pads (1, 2)
    (2, 6, 4, 8, 16, 3, 2),        # pads (0, 1)
    (2, 7, 5, 8, 24, 3, 2),        # pads (1, 1)
    (3, 1, 3, 8, 8, 3, 2),         # H = 1
    (2, 5, 6, 16, 8, 3, 1),        # stride 1: nine windows per pixel
    (2, 14, 14, 64, 192, 3, 2),    # M = 98, K = 576
    (1, 28, 28, 192, 384, 3, 2),   # K = 1728
]
NAMES = ("y", "dx", "dw", "db")


def _td(mode):
    import torch
    return torch.bfloat16 if mode == "bf16" else torch.float32


@functools.lru_cache(maxsize=None)
def _case(shape, mode):
    """Inputs (numpy, x and dy representable in the compute dtype) and the float64 reference, once."""
    import torch
    B, H, W, C, E, k, s = shape
    rng = np.random.default_rng(100 * sum(shape) + (mode == "bf16"))
    x = randn(rng, (B, H, W, C), mode)
    w = (rng.standard_normal((k, k, C, E)) / np.sqrt(k * k * C)).astype(np.float32)
    b = (0.5 * rng.standard_normal(E)).astype(np.float32)
    dy = randn(rng, (B, -(-H // s) * -(-W // s), E), mode)
    tx, tw, tb = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, w, b))
    y = R.conv_tokens(tx, tw, tb, k, s, mode)
    y.backward(torch.tensor(dy, dtype=torch.float64))
    ref = dict(y=y.detach().numpy(), dx=tx.grad.numpy(), dw=tw.grad.numpy(), db=tb.grad.numpy())
    return dict(x=x, w=w, b=b, dy=dy, k=k, s=s, ref=ref)


def _leaves(c, dev, mode, x_grad=True):
    import torch
    x = torch.tensor(c["x"], device=dev).to(_td(mode)).requires_grad_(x_grad)
    w, b = (torch.tensor(c[n], device=dev, requires_grad=True) for n in ("w", "b"))
    return x, w, b


def _hip(c, dev, mode, x_grad=True):
    import torch
    import sae_vision_amd.ops as ops
    x, w, b = _leaves(c, dev, mode, x_grad)
    y = ops.conv_tokens(x, w, b, c["k"], c["s"], _td(mode))
    y.backward(torch.tensor(c["dy"], device=dev).to(_td(mode)))
    return dict(y=y.detach(), dx=x.grad, dw=w.grad, db=b.grad)


def _block(c, dev, mode):
    import torch
    from sae_vision_amd import cvt
    k, _, C, E = c["w"].shape
    blk = cvt.ConvTokenEmbedBlock(E, k, c["s"], _td(mode), in_ch=C, device=dev)
    with torch.no_grad():
        blk.Conv_0.kernel.copy_(torch.tensor(c["w"], device=dev))
        blk.Conv_0.bias.copy_(torch.tensor(c["b"], device=dev))
    return blk


def _framework(c, dev, mode):
    import torch
    blk = _block(c, dev, mode)
    x = torch.tensor(c["x"], device=dev).to(_td(mode)).requires_grad_(True)
    y = blk._framework_conv(x)
    y.backward(torch.tensor(c["dy"], device=dev).to(_td(mode)))
    return dict(y=y.detach(), dx=x.grad, dw=blk.Conv_0.kernel.grad, db=blk.Conv_0.bias.grad)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode,x_mode", [("f32", "f32"), ("bf16", "bf16"), ("bf16", "f32")])
def test_window_matrix_bits(dev, shape, mode, x_mode):
    """P is the unfold of the padded input rounded to the compute dtype (an fp32 input is rounded as it
    is staged); the columns K .. Kp are zero."""
    import torch
    import sae_vision_amd.ops as ops
    B, H, W, C, E, k, s = shape
    x = torch.tensor(_case(shape, "f32")["x"]).to(_td(x_mode))     # unrounded values when x_mode is f32
    P = ops.conv_window_matrix(x.to(dev), k, s, _td(mode)).cpu()
    K = k * k * C
    assert P.dtype == _td(mode) and tuple(P.shape) == (B * -(-H // s) * -(-W // s), -(-K // 8) * 8)
    want = R.window_matrix(x.to(_td(mode)).double(), k, s).to(_td(mode))
    assert torch.equal(P[:, :K], want)
    assert not P[:, K:].any()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_scatter_bits(dev, shape, mode):
    """Integer-valued dP, |v| <= 8: at most nine terms per pixel, every sum exact in bf16, so the
    result equals the float64 fold bit for bit."""
    import torch
    import sae_vision_amd.ops as ops
    B, H, W, C, E, k, s = shape
    K, Kp = k * k * C, -(-(k * k * C) // 8) * 8
    M = B * -(-H // s) * -(-W // s)
    rng = np.random.default_rng(7 + sum(shape))
    dP = torch.tensor(rng.integers(-8, 9, size=(M, Kp)).astype(np.float32))
    dX = ops.conv_window_scatter(dP.to(_td(mode)).to(dev), (B, H, W, C), k, s).cpu()
    assert dX.dtype == _td(mode) and tuple(dX.shape) == (B, H, W, C)
    want = R.window_fold(dP[:, :K].double(), (B, H, W, C), k, s)
    assert torch.equal(dX.double(), want)


@pytest.mark.parametrize("shape", SHAPES)
def test_parity_f32(dev, shape):
    c = _case(shape, "f32")
    got = _hip(c, dev, "f32")
    errs = {n: rel_err(got[n], c["ref"][n]) for n in NAMES}
    print(shape, errs)
    assert max(errs.values()) <= TOL["f32"], errs


@pytest.mark.parametrize("shape", SHAPES)
def test_parity_bf16(dev, shape):
    """bf16: no further from the float64 reference than TOL, or than twice the framework route
    (rounding at the same points, another summation order) on the same inputs."""
    c = _case(shape, "bf16")
    got = _hip(c, dev, "bf16")
    fwk = _framework(c, dev, "bf16")
    errs = {n: (rel_err(got[n], c["ref"][n]), rel_err(fwk[n], c["ref"][n])) for n in NAMES}
    print(shape, errs)
    bad = {n: e for n, e in errs.items() if e[0] > max(TOL["bf16"], 2 * e[1])}
    assert not bad, f"(hip, framework) errors: {bad}"


@pytest.mark.parametrize("shape,mode", [((2, 9, 11, 3, 16, 7, 4), "bf16"), ((2, 14, 14, 64, 192, 3, 2), "bf16"),
                                        ((2, 5, 6, 16, 8, 3, 1), "f32"), ((1, 28, 28, 192, 384, 3, 2), "f32")])
def test_deterministic(dev, shape, mode):
    import torch
    c = _case(shape, mode)
    a, b = _hip(c, dev, mode), _hip(c, dev, mode)
    for n in NAMES:
        assert torch.equal(a[n], b[n]), n


@pytest.mark.parametrize("shape,mode", [((2, 14, 14, 64, 192, 3, 2), "bf16"), ((2, 9, 11, 3, 16, 7, 4), "f32")])
def test_graph_capture(dev, shape, mode):
    """Forward + backward captured once on one stream; replayed on a new x it gives the eager bits."""
    import torch
    import sae_vision_amd.ops as ops
    c = _case(shape, mode)
    dt, k, s = _td(mode), c["k"], c["s"]
    xs, w, b = _leaves(c, dev, mode)
    dys = torch.tensor(c["dy"], device=dev).to(dt)

    def step():
        y = ops.conv_tokens(xs, w, b, k, s, dt)
        return (y,) + torch.autograd.grad(y, (xs, w, b), dys)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    x2 = randn(np.random.default_rng(11), c["x"].shape, mode)
    with torch.no_grad():
        xs.copy_(torch.tensor(x2, device=dev).to(dt))
    graph.replay()
    torch.cuda.synchronize()
    eager = _hip(dict(c, x=x2), dev, mode)
    for n, t in zip(NAMES, outs):
        assert torch.equal(t, eager[n]), n


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_launch_counts(dev, mode):
    """An input that takes no gradient (the image batch) launches neither the dP product nor the scatter."""
    import sae_vision_amd.ops as ops
    c = _case((2, 7, 5, 8, 24, 3, 2), mode)
    counts = {}
    for x_grad in (True, False):
        timer = ops.KernelTimer()
        ops.set_kernel_timer(timer)
        try:
            got = _hip(c, dev, mode, x_grad)
        finally:
            ops.set_kernel_timer(None)
        counts[x_grad] = {n: v["launches"] for n, v in timer.summary().items()}
        assert (got["dx"] is not None) == x_grad
    for x_grad, n in counts.items():
        assert n.get("conv_tokens_fwd") == 1 and n.get("conv_tokens_bwd") == 1 and n.get("conv_window_gather") == 1, n
    assert counts[True].get("conv_tokens_dp") == 1 and counts[True].get("conv_window_scatter") == 1, counts
    assert "conv_tokens_dp" not in counts[False] and "conv_window_scatter" not in counts[False], counts
    if mode == "f32":   # forward, dW (+ dP): the exact-fp32 GEMM is timed by name
        assert counts[True].get("gemm_f32") == 3 and counts[False].get("gemm_f32") == 2, counts
    else:
        assert counts[True].get("gemm_dw") == 1 and counts[False].get("gemm_dw") == 1, counts


@pytest.mark.parametrize("k,E", [(9, 16), (3, 12)])
def test_fallback_is_the_framework_route(dev, k, E):
    """Outside the envelope (a 9 x 9 kernel; 12 output channels) forward() is _framework_forward, bit for bit."""
    import torch
    import sae_vision_amd.ops as ops
    from sae_vision_amd import cvt
    torch.manual_seed(1)
    blk = cvt.ConvTokenEmbedBlock(E, k, 2, torch.bfloat16, in_ch=8, device=dev)
    ref = copy.deepcopy(blk)
    x = torch.tensor(np.random.default_rng(2).standard_normal((2, 11, 10, 8)).astype(np.float32), device=dev)
    assert not ops.conv_tokens_ok(x, blk.Conv_0.kernel, k, 2, torch.bfloat16)
    timer = ops.KernelTimer()
    ops.set_kernel_timer(timer)
    try:
        y = blk(x)
    finally:
        ops.set_kernel_timer(None)
    assert "conv_tokens_fwd" not in timer.summary()
    assert torch.equal(y, ref._framework_forward(x))
    with pytest.raises(ValueError, match="conv_tokens_ok"):
        ops.conv_tokens(x, blk.Conv_0.kernel, blk.Conv_0.bias, k, 2, torch.bfloat16)


def test_module_takes_the_hip_route(dev):
    """Inside the envelope the stem is conv_tokens + the LayerNorm kernel, close to the framework route."""
    import torch
    import sae_vision_amd.ops as ops
    c = _case((2, 14, 14, 64, 192, 3, 2), "bf16")
    blk = _block(c, dev, "bf16")
    x = torch.tensor(c["x"], device=dev)
    timer = ops.KernelTimer()
    ops.set_kernel_timer(timer)
    try:
        y = blk(x)
    finally:
        ops.set_kernel_timer(None)
    assert timer.summary()["conv_tokens_fwd"]["launches"] == 1
    ref = blk._framework_forward(x).detach()
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (2, 49, 192)
    assert rel_err(y, ref.float().cpu().numpy()) <= TOL["bf16"]
