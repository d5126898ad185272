"""GPU parity of the CvT convolutional projection kernels (sae_dwconv_bn_*: depthwise 3x3 with SAME
padding + BatchNorm, forward / backward, running statistics, evaluation) against the float64
reference of _conv_proj_ref.py, and of the modules that route to them against the framework route
they replace (ConvProjectionBlock._framework_forward)."""
import copy
import functools

import numpy as np
import pytest

import _conv_proj_ref as R
from _util import TOL, randn, rel_err

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.9
SHAPES = [
    (2, 5, 7, 8, 1),
    (2, 5, 7, 8, 2),
    (2, 6, 4, 40, 2),        # even sizes at stride 2: pads (0, 1)
    (3, 1, 3, 8, 2),         # H = 1
    (2, 14, 14, 368, 1),
    (2, 15, 15, 368, 2),
]
NAMES = ("y", "dx", "dw", "dgamma", "dbeta")


def _td(mode):
    import torch
    return torch.bfloat16 if mode == "bf16" else torch.float32


@functools.lru_cache(maxsize=None)
def _case(shape, mode, big_mean=False):
    """Inputs (numpy, representable in the compute dtype) and the float64 reference, computed once."""
    import torch
    B, H, W, C, s = shape
    rng = np.random.default_rng(1000 * sum(shape) + (mode == "bf16") + 2 * big_mean)
    x = randn(rng, (B, H, W, C), mode)
    w = (rng.standard_normal((3, 3, 1, C)) / 3).astype(np.float32)
    if big_mean:   # t far from zero: x ~ N(100, 1), positive taps
        x = (x + 100).astype(np.float32)
        w = (np.abs(w) + 0.05).astype(np.float32)
    gamma = (1 + 0.5 * rng.standard_normal(C)).astype(np.float32)
    beta = (0.5 * rng.standard_normal(C)).astype(np.float32)
    dy = randn(rng, (B, -(-H // s), -(-W // s), C), mode)
    f64 = lambda a: torch.tensor(a, dtype=torch.float64)
    fw = R.forward(f64(x), f64(w), f64(gamma), f64(beta), s, EPS, mode)
    bw = R.backward(f64(x), f64(w), f64(gamma), fw, f64(dy), s, mode)
    ref = dict(y=fw["y"], dx=bw["dx"], dw=bw["dw"], dgamma=bw["dgamma"], dbeta=bw["dbeta"], mu=fw["mu"], var=fw["var"])
    return dict(x=x, w=w, gamma=gamma, beta=beta, dy=dy, s=s, ref={k: v.numpy() for k, v in ref.items()})


def _leaves(c, dev, mode):
    import torch
    x = torch.tensor(c["x"], device=dev).to(_td(mode)).requires_grad_(True)
    w, gamma, beta = (torch.tensor(c[k], device=dev, requires_grad=True) for k in ("w", "gamma", "beta"))
    return x, w, gamma, beta


def _buffers(C, dev):
    import torch
    return torch.zeros(C, device=dev), torch.ones(C, device=dev)


def _hip(c, dev, mode, bufs=None):
    """One training forward + backward on the HIP route: outputs by name, and the running buffers."""
    import torch
    import sae_vision_amd.ops as ops
    x, w, gamma, beta = _leaves(c, dev, mode)
    rm, rv = bufs if bufs is not None else _buffers(x.shape[-1], dev)
    y = ops.dwconv_bn(x, w, gamma, beta, rm, rv, c["s"], MOM, EPS, True, _td(mode))
    y.backward(torch.tensor(c["dy"], device=dev).to(_td(mode)))
    return dict(y=y.detach(), dx=x.grad, dw=w.grad, dgamma=gamma.grad, dbeta=beta.grad), (rm, rv)


def _framework(c, dev, mode):
    """The same on ConvProjectionBlock._framework_forward with an identity 1x1 convolution (exact in
    either dtype: one non-zero product per output)."""
    import torch
    from sae_vision_amd.layers import cvt
    x, w, gamma, beta = _leaves(c, dev, mode)
    C = x.shape[-1]
    blk = cvt.ConvProjectionBlock(C, C, 3, c["s"], False, MOM, EPS, _td(mode), dev)
    with torch.no_grad():
        blk.Conv_0.kernel.copy_(w)
        blk.BatchNorm_0.scale.copy_(gamma)
        blk.BatchNorm_0.bias.copy_(beta)
        blk.Conv_1.kernel.copy_(torch.eye(C, device=dev).reshape(1, 1, C, C))
    y = blk._framework_forward(x, True)
    y.backward(torch.tensor(c["dy"], device=dev).to(_td(mode)))
    return dict(y=y.detach(), dx=x.grad, dw=blk.Conv_0.kernel.grad, dgamma=blk.BatchNorm_0.scale.grad,
                dbeta=blk.BatchNorm_0.bias.grad)


@pytest.mark.parametrize("shape", SHAPES)
def test_parity_f32(dev, shape):
    c = _case(shape, "f32")
    got, _ = _hip(c, dev, "f32")
    errs = {n: rel_err(got[n], c["ref"][n]) for n in NAMES}
    print(shape, errs)
    assert max(errs.values()) <= TOL["f32"], errs


@pytest.mark.parametrize("shape", SHAPES)
def test_parity_bf16(dev, shape):
    """bf16: no further from the float64 reference than TOL, or than twice the framework route (the
    parent's code, rounding at the same points, another summation order) on the same inputs."""
    c = _case(shape, "bf16")
    got, _ = _hip(c, dev, "bf16")
    fwk = _framework(c, dev, "bf16")
    errs = {n: (rel_err(got[n], c["ref"][n]), rel_err(fwk[n], c["ref"][n])) for n in NAMES}
    print(shape, errs)
    bad = {n: e for n, e in errs.items() if e[0] > max(TOL["bf16"], 2 * e[1])}
    assert not bad, f"(hip, framework) errors: {bad}"


def test_statistics_do_not_cancel(dev):
    """x ~ N(100, 1) and positive taps put t's mean far from zero: fp32 sums of t and t^2 lose the
    variance there, the fp64 sums of the kernels do not."""
    c = _case((2, 6, 4, 40, 2), "f32", True)
    got, _ = _hip(c, dev, "f32")
    err = rel_err(got["y"], c["ref"]["y"])
    print("y", err, "mean |t| / std", float(np.abs(c["ref"]["mu"]).mean() / np.sqrt(c["ref"]["var"]).mean()))
    assert err <= TOL["f32"], err


@pytest.mark.parametrize("shape,mode", [((2, 5, 7, 8, 2), "f32"), ((2, 14, 14, 368, 1), "f32"),
                                        ((2, 6, 4, 40, 2), "bf16")])
def test_running_statistics_and_evaluation(dev, shape, mode):
    import torch
    import sae_vision_amd.ops as ops
    c = _case(shape, mode)
    bufs = _buffers(shape[3], dev)
    _hip(c, dev, mode, bufs)
    _hip(c, dev, mode, bufs)
    mean, var = np.zeros(shape[3]), np.ones(shape[3])
    for _ in range(2):
        mean, var = R.running(mean, var, c["ref"]["mu"], c["ref"]["var"], MOM)
    assert rel_err(bufs[0], mean) <= TOL["f32"] and rel_err(bufs[1], var) <= TOL["f32"]
    # evaluation: those buffers in the place of the batch statistics, and left alone
    before = [b.clone() for b in bufs]
    x, w, gamma, beta = _leaves(c, dev, mode)
    with torch.no_grad():
        y = ops.dwconv_bn(x, w, gamma, beta, bufs[0], bufs[1], c["s"], MOM, EPS, False, _td(mode))
    f64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    ref = R.forward(f64(c["x"]), f64(c["w"]), f64(c["gamma"]), f64(c["beta"]), c["s"], EPS, mode,
                    stats=(f64(mean), f64(var)))["y"].numpy()
    assert rel_err(y, ref) <= TOL[mode]
    assert all(torch.equal(a, b) for a, b in zip(before, bufs))


@pytest.mark.parametrize("shape,mode", [((2, 15, 15, 368, 2), "bf16"), ((2, 14, 14, 368, 1), "f32"),
                                        ((2, 6, 4, 40, 2), "bf16")])
def test_deterministic(dev, shape, mode):
    import torch
    c = _case(shape, mode)
    a, _ = _hip(c, dev, mode)
    b, _ = _hip(c, dev, mode)
    for n in NAMES:
        assert torch.equal(a[n], b[n]), n


@pytest.mark.parametrize("shape,mode", [((2, 15, 15, 368, 2), "bf16"), ((2, 5, 7, 8, 1), "f32")])
def test_graph_capture(dev, shape, mode):
    """Forward + backward captured once on one stream; replayed on a new x it gives the eager bits, and
    the running buffers advance once per replay."""
    import torch
    import sae_vision_amd.ops as ops
    c, c2 = _case(shape, mode), _case(shape, mode, True)
    dt, s = _td(mode), c["s"]
    xs, w, gamma, beta = _leaves(c, dev, mode)
    dys = torch.tensor(c["dy"], device=dev).to(dt)
    rm, rv = _buffers(shape[3], dev)

    def step():
        y = ops.dwconv_bn(xs, w, gamma, beta, rm, rv, s, MOM, EPS, True, dt)
        return (y,) + torch.autograd.grad(y, (xs, w, gamma, beta), dys)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    with torch.no_grad():
        xs.copy_(torch.tensor(c2["x"], device=dev).to(dt))
        rm.zero_()
        rv.fill_(1)
    graph.replay()
    torch.cuda.synchronize()
    c_new = dict(c, x=c2["x"])
    eager, bufs = _hip(c_new, dev, mode)
    for n, t in zip(NAMES, outs):
        assert torch.equal(t, eager[n]), n
    assert torch.equal(rm, bufs[0]) and torch.equal(rv, bufs[1])
    graph.replay()
    _hip(c_new, dev, mode, bufs)
    torch.cuda.synchronize()
    assert torch.equal(rm, bufs[0]) and torch.equal(rv, bufs[1])
    assert not torch.equal(rm, torch.zeros_like(rm))


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_module_matches_framework_route(dev, mode):
    """CvTSelfAttentionBlock, training forward + backward: the HIP projections against a second module
    with the same parameters whose projections are forced onto _framework_forward."""
    import torch
    import sae_vision_amd.layers as layers
    import sae_vision_amd.ops as ops
    B, S, C, H = 2, 14, 96, 3
    torch.manual_seed(0)
    mod = layers.CvTSelfAttentionBlock(num_heads=H, dtype=_td(mode), in_ch=C, device=dev)
    rng = np.random.default_rng(5)
    with torch.no_grad():   # BatchNorm parameters away from their init values
        for i in range(3):
            bn = getattr(mod, f"ConvProjectionBlock_{i}").BatchNorm_0
            bn.scale.copy_(torch.tensor(1 + 0.3 * rng.standard_normal(C), device=dev))
            bn.bias.copy_(torch.tensor(0.3 * rng.standard_normal(C), device=dev))
    ref = copy.deepcopy(mod)
    for i in range(3):
        blk = getattr(ref, f"ConvProjectionBlock_{i}")
        blk.forward = blk._framework_forward
    tree = layers.flax_params(mod)
    for i in range(3):
        assert set(tree[f"ConvProjectionBlock_{i}"]) == {"Conv_0", "BatchNorm_0", "Conv_1"}
        assert set(tree[f"ConvProjectionBlock_{i}"]["BatchNorm_0"]) == {"scale", "bias"}
        assert set(tree[f"ConvProjectionBlock_{i}"]["Conv_0"]) == {"kernel"}
    assert [n for n, _ in mod.named_buffers()] == [n for n, _ in ref.named_buffers()]
    assert len(list(mod.named_buffers())) == 6
    x = rng.standard_normal((B, S, S, C)).astype(np.float32)
    dy = torch.tensor(randn(rng, (B, S * S, C), mode), device=dev).to(_td(mode))
    timer = ops.KernelTimer()
    outs = []
    for m in (mod, ref):
        ops.set_kernel_timer(timer if m is mod else None)
        try:
            tx = torch.tensor(x, device=dev, requires_grad=True)
            y = m(tx, is_training=True)
            y.backward(dy)
        finally:
            ops.set_kernel_timer(None)
        outs.append((y.detach(), tx.grad))
    launches = {k: v["launches"] for k, v in timer.summary().items()}
    assert launches.get("dwconv_bn_fwd") == 3 and launches.get("dwconv_bn_bwd") == 3, launches
    assert rel_err(outs[0][0], outs[1][0].float().cpu().numpy()) <= TOL[mode]
    assert rel_err(outs[0][1], outs[1][1].float().cpu().numpy()) <= TOL[mode]
    grads = {n: p.grad.float().cpu().numpy() for n, p in ref.named_parameters()}
    # The key projection's BatchNorm bias shifts every key by one vector, which moves each query's
    # scores by a constant: the softmax does not see it and the gradient is zero in exact arithmetic.
    # What either route holds there is rounding noise, so its error is measured against the largest
    # BatchNorm-bias gradient of the three projections (the same quantity, dL / dbeta) instead of itself.
    zero = "ConvProjectionBlock_1.BatchNorm_0.bias"
    bias_scale = max(np.abs(grads[f"ConvProjectionBlock_{i}.BatchNorm_0.bias"]).max() for i in range(3))
    assert np.abs(grads[zero]).max() <= TOL[mode] * bias_scale
    for n, p in mod.named_parameters():
        err = rel_err(p.grad, grads[n])
        if n == zero:
            err *= np.abs(grads[n]).max() / bias_scale
        print(n, err)
        assert err <= TOL[mode], (n, err)
    for (n, b), (_, b2) in zip(mod.named_buffers(), ref.named_buffers()):
        assert rel_err(b, b2.cpu().numpy()) <= TOL["f32"], n


@pytest.mark.parametrize("kw", [dict(kernel_size=5, in_ch=96), dict(kernel_size=3, in_ch=12)])
def test_fallback_is_the_framework_route(dev, kw):
    """Outside the envelope (a 5x5 kernel; 12 channels in bf16) forward() is _framework_forward, bit for bit."""
    import torch
    import sae_vision_amd.ops as ops
    from sae_vision_amd.layers import cvt
    C = kw["in_ch"]
    torch.manual_seed(1)
    blk = cvt.ConvProjectionBlock(C, 24, kw["kernel_size"], 2, True, MOM, EPS, torch.bfloat16, dev)
    ref = copy.deepcopy(blk)
    x = torch.tensor(np.random.default_rng(2).standard_normal((2, 7, 6, C)).astype(np.float32), device=dev)
    assert not ops.dwconv_bn_ok(x, kw["kernel_size"], 2, torch.bfloat16)
    timer = ops.KernelTimer()
    ops.set_kernel_timer(timer)
    try:
        y = blk(x, True)
    finally:
        ops.set_kernel_timer(None)
    assert "dwconv_bn_fwd" not in timer.summary()
    y_ref = ref._framework_forward(x, True)
    assert torch.equal(y, y_ref)
    assert torch.equal(blk.BatchNorm_0.mean, ref.BatchNorm_0.mean) and torch.equal(blk.BatchNorm_0.var, ref.BatchNorm_0.var)
