"""GPU parity of the LeFF feed-forward: the BatchNorm + GELU kernels over token rows (sae_bn_gelu_*,
csrc/bn_rows.h: forward / backward, class-token lead rows on either side, running statistics,
evaluation, determinism, graph capture) against the float64 reference of _leff_ref.py, and LeFFBlock on
its HIP route against the framework route it replaces (LeFFBlock._framework_forward) and, in fp32,
against the float64 block."""
import copy
import ctypes
import functools

import numpy as np
import pytest

import _leff_ref as R
from _util import TOL, randn, rel_err

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.9
# (B, L, C, x_lead, y_lead)
SHAPES = [
    (1, 1, 8, 0, 0),         # one row: var = 0, rstd = rsqrt(eps)
    (2, 4, 8, 0, 0),
    (3, 9, 40, 1, 0),
    (2, 9, 40, 0, 1),
    (2, 9, 12, 1, 1),        # fp32 only (C % 8 != 0)
    (2, 196, 768, 1, 0),     # three channel chunks in bf16 and in fp32, many workgroups
    (2, 4, 2056, 0, 0),      # 257 (bf16) / 514 (fp32) channel vectors: several chunks, the last one partial
]
NAMES = ("y", "dx", "dgamma", "dbeta")


def _td(mode):
    import torch
    return torch.bfloat16 if mode == "bf16" else torch.float32


def _modes(shape):
    return ["f32"] if shape[2] % 8 else ["f32", "bf16"]


@functools.lru_cache(maxsize=None)
def _case(shape, mode, big_mean=False):
    """Inputs (numpy, representable in the compute dtype; the skipped lead rows of x are NaN) and the
    float64 reference over the participating rows, computed once."""
    import torch
    B, L, C, xl, yl = shape
    rng = np.random.default_rng(1000 * sum(shape) + (mode == "bf16") + 2 * big_mean)
    xp = randn(rng, (B, L, C), mode)
    if big_mean:   # x ~ N(100, 1)
        xp = (xp + 100).astype(np.float32)
    x = np.full((B, L + xl, C), np.nan, np.float32)
    x[:, xl:] = xp
    gamma = (1 + 0.5 * rng.standard_normal(C)).astype(np.float32)
    beta = (0.5 * rng.standard_normal(C)).astype(np.float32)
    dy = randn(rng, (B, L + yl, C), mode)
    lead = randn(rng, (B, 3, C), mode)   # the lead rows are lead[:, :1]: a view with a sample pitch of 3 C
    f64 = lambda a: torch.tensor(a, dtype=torch.float64)
    fw = R.bn_gelu_forward(f64(xp).reshape(-1, C), f64(gamma), f64(beta), EPS, mode)
    bw = R.bn_gelu_backward(f64(gamma), fw, f64(dy[:, yl:]).reshape(-1, C))
    ref = dict(y=fw["y"].reshape(B, L, C), dx=bw["dx"].reshape(B, L, C), dgamma=bw["dgamma"], dbeta=bw["dbeta"],
               mu=fw["mu"], var=fw["var"], r=fw["r"])
    return dict(x=x, gamma=gamma, beta=beta, dy=dy, lead=lead, ref={k: v.numpy() for k, v in ref.items()})


def _leaves(c, dev, mode):
    import torch
    x = torch.tensor(c["x"], device=dev).to(_td(mode)).requires_grad_(True)
    gamma, beta = (torch.tensor(c[k], device=dev, requires_grad=True) for k in ("gamma", "beta"))
    base = torch.tensor(c["lead"], device=dev).to(_td(mode)).requires_grad_(True)
    return x, gamma, beta, base


def _buffers(C, dev):
    import torch
    return torch.zeros(C, device=dev), torch.ones(C, device=dev)


def _hip(c, shape, dev, mode, bufs=None):
    """One training forward + backward through ops.bn_gelu: y and dx over the participating rows, the
    parameter gradients, and the whole tensors (Y, DX, dbase) for the lead-row checks."""
    import torch
    import sae_vision_amd.ops as ops
    xl, yl = shape[3:]
    x, gamma, beta, base = _leaves(c, dev, mode)
    rm, rv = bufs if bufs is not None else _buffers(shape[2], dev)
    y = ops.bn_gelu(x, gamma, beta, rm, rv, MOM, EPS, True, _td(mode), xl, yl, base[:, :1] if yl else None)
    y.backward(torch.tensor(c["dy"], device=dev).to(_td(mode)))
    return dict(y=y.detach()[:, yl:], dx=x.grad[:, xl:], dgamma=gamma.grad, dbeta=beta.grad, Y=y.detach(),
                DX=x.grad, dbase=base.grad, base=base.detach()), (rm, rv)


def _framework(c, shape, dev, mode):
    """The same over the participating rows as framework ops: the BatchNorm of layers/cvt.py and
    F.gelu(approximate="tanh"), autograd's backward."""
    import torch
    import torch.nn.functional as F
    from sae_vision_amd.layers import cvt
    B, L, C, xl, yl = shape
    x = torch.tensor(c["x"][:, xl:], device=dev).to(_td(mode)).requires_grad_(True)
    bn = cvt._BatchNorm(C, MOM, EPS, dev)
    with torch.no_grad():
        bn.scale.copy_(torch.tensor(c["gamma"], device=dev))
        bn.bias.copy_(torch.tensor(c["beta"], device=dev))
    y = F.gelu(bn(x.view(B, 1, L, C), True), approximate="tanh").view(B, L, C)
    y.backward(torch.tensor(c["dy"][:, yl:], device=dev).to(_td(mode)))
    return dict(y=y.detach(), dx=x.grad, dgamma=bn.scale.grad, dbeta=bn.bias.grad)


def _lead_checks(got, c, shape, dev, mode):
    """x_lead: the NaN rows of x reached nothing and their dx is exactly zero.  y_lead: row 0 of y is
    `lead` bit for bit and the gradient of `lead` is row 0 of dy."""
    import torch
    xl, yl = shape[3:]
    for n in NAMES:
        assert torch.isfinite(got[n]).all(), n
    if xl:
        assert torch.count_nonzero(got["DX"][:, :1]) == 0 and not torch.isnan(got["DX"]).any()
    if yl:
        dy = torch.tensor(c["dy"], device=dev).to(_td(mode))
        assert torch.equal(got["Y"][:, :1], got["base"][:, :1])
        assert torch.equal(got["dbase"][:, :1], dy[:, :1]) and torch.count_nonzero(got["dbase"][:, 1:]) == 0
    else:
        assert got["dbase"] is None


@pytest.mark.parametrize("shape", SHAPES)
def test_parity_f32(dev, shape):
    c = _case(shape, "f32")
    got, _ = _hip(c, shape, dev, "f32")
    errs = {n: rel_err(got[n], c["ref"][n]) for n in NAMES}
    print(shape, errs)
    assert max(errs.values()) <= TOL["f32"], errs
    _lead_checks(got, c, shape, dev, "f32")


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[2] % 8 == 0])
def test_parity_bf16(dev, shape):
    """bf16: no further from the float64 reference than TOL, or than twice the framework route (rounding
    at the same points, another summation order) on the same inputs."""
    c = _case(shape, "bf16")
    got, _ = _hip(c, shape, dev, "bf16")
    fwk = _framework(c, shape, dev, "bf16")
    errs = {n: (rel_err(got[n], c["ref"][n]), rel_err(fwk[n], c["ref"][n])) for n in NAMES}
    print(shape, errs)
    bad = {n: e for n, e in errs.items() if e[0] > max(TOL["bf16"], 2 * e[1])}
    assert not bad, f"(hip, framework) errors: {bad}"
    _lead_checks(got, c, shape, dev, "bf16")


@pytest.mark.parametrize("shape,mode", [((3, 9, 40, 1, 0), "f32"), ((2, 9, 12, 1, 1), "f32"), ((3, 9, 40, 1, 0), "bf16"),
                                        ((2, 196, 768, 1, 0), "bf16")])
def test_c_abi_with_poisoned_lead_rows(dev, shape, mode):
    """The C ABI called directly, with the lead rows of x and the whole dx buffer NaN beforehand: the
    saved statistics are those of the participating rows, the lead rows of dx come back exactly zero,
    and everything equals what ops.bn_gelu returns, bit for bit."""
    import torch
    from sae_vision_amd import _lib as L
    lib = L.load()
    B, Lt, C, xl, yl = shape
    dt = _td(mode)
    c = _case(shape, mode)
    x, gamma, beta, base = (t.detach() for t in _leaves(c, dev, mode))
    assert torch.isnan(x[:, :xl]).all()
    dy = torch.tensor(c["dy"], device=dev).to(dt)
    lead = base[:, :1]
    rm, rv = _buffers(C, dev)
    y = torch.full((B, Lt + yl, C), float("nan"), dtype=dt, device=dev)
    dx = torch.full_like(x, float("nan"))
    mean, rstd, dg, db = (torch.full((C,), float("nan"), device=dev) for _ in range(4))
    ws = torch.empty(lib.sae_bn_gelu_workspace_bytes(B, Lt, C), dtype=torch.uint8, device=dev)
    assert ws.numel() > 0
    d = L.SaeBnrowsDesc(B, Lt, C, xl, yl, L.SAE_DTYPE_BF16 if mode == "bf16" else L.SAE_DTYPE_F32, 1, MOM, EPS)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    L.check(lib.sae_bn_gelu_fwd(st, ctypes.byref(d), p(x), p(gamma), p(beta), p(rm), p(rv), p(lead) if yl else None,
                                lead.stride(0) if yl else 0, p(y), p(mean), p(rstd), p(ws)))
    L.check(lib.sae_bn_gelu_bwd(st, ctypes.byref(d), p(x), p(gamma), p(beta), p(mean), p(rstd), p(dy), p(dx), p(dg),
                                p(db), p(ws)))
    torch.cuda.synchronize()
    assert rel_err(mean, c["ref"]["mu"]) <= TOL["f32"] and rel_err(rstd, c["ref"]["r"]) <= TOL["f32"]
    assert torch.count_nonzero(dx[:, :xl]) == 0 and not torch.isnan(dx).any() and not torch.isnan(y).any()
    got, bufs = _hip(c, shape, dev, mode)
    for a, b in ((y, got["Y"]), (dx, got["DX"]), (dg, got["dgamma"]), (db, got["dbeta"]), (rm, bufs[0]), (rv, bufs[1])):
        assert torch.equal(a, b)


def test_statistics_do_not_cancel(dev):
    """x ~ N(100, 1): fp32 sums of x and x^2 lose the variance there, the fp64 sums of the kernels do not."""
    shape = (3, 9, 40, 1, 0)
    c = _case(shape, "f32", True)
    got, _ = _hip(c, shape, dev, "f32")
    errs = {n: rel_err(got[n], c["ref"][n]) for n in NAMES}
    print(errs, "mean |x| / std", float(np.abs(c["ref"]["mu"]).mean() / np.sqrt(c["ref"]["var"]).mean()))
    assert errs["y"] <= TOL["f32"], errs


@pytest.mark.parametrize("shape,mode", [((3, 9, 40, 1, 0), "f32"), ((2, 196, 768, 1, 0), "f32"),
                                        ((2, 9, 40, 0, 1), "bf16")])
def test_running_statistics_and_evaluation(dev, shape, mode):
    import torch
    import sae_vision_amd.ops as ops
    B, L, C, xl, yl = shape
    c = _case(shape, mode)
    bufs = _buffers(C, dev)
    _hip(c, shape, dev, mode, bufs)
    _hip(c, shape, dev, mode, bufs)
    mean, var = np.zeros(C), np.ones(C)
    for _ in range(2):
        mean, var = R.running(mean, var, c["ref"]["mu"], c["ref"]["var"], MOM)
    assert rel_err(bufs[0], mean) <= TOL["f32"] and rel_err(bufs[1], var) <= TOL["f32"]
    # evaluation: those buffers in the place of the batch statistics, and left alone
    before = [b.clone() for b in bufs]
    x, gamma, beta, base = _leaves(c, dev, mode)
    lead = base[:, :1] if yl else None
    with torch.no_grad():
        y = ops.bn_gelu(x, gamma, beta, bufs[0], bufs[1], MOM, EPS, False, _td(mode), xl, yl, lead)
    f64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    ref = R.bn_gelu_forward(f64(c["x"][:, xl:]).reshape(-1, C), f64(c["gamma"]), f64(c["beta"]), EPS, mode,
                            stats=(f64(mean), f64(var)))["y"].reshape(B, L, C).numpy()
    assert rel_err(y[:, yl:], ref) <= TOL[mode]
    if yl:
        assert torch.equal(y[:, :1], lead)
    assert all(torch.equal(a, b) for a, b in zip(before, bufs))
    # the evaluation form has no backward: the predicate refuses it when a gradient is wanted
    assert ops.bn_gelu_ok(x, _td(mode), training=False, needs_grad=False, x_lead=xl)
    assert not ops.bn_gelu_ok(x, _td(mode), training=False, needs_grad=True, x_lead=xl)
    assert not ops.bn_gelu_ok(x, _td(mode), training=False, x_lead=xl)   # x requires a gradient, grad mode on
    y = ops.bn_gelu(x, gamma, beta, bufs[0], bufs[1], MOM, EPS, False, _td(mode), xl, yl, lead)
    with pytest.raises(RuntimeError, match="no backward"):
        y.float().sum().backward()


@pytest.mark.parametrize("shape,mode", [((2, 196, 768, 1, 0), "bf16"), ((2, 196, 768, 1, 0), "f32"),
                                        ((2, 4, 2056, 0, 0), "bf16"), ((2, 9, 12, 1, 1), "f32")])
def test_deterministic(dev, shape, mode):
    import torch
    c = _case(shape, mode)
    a, _ = _hip(c, shape, dev, mode)
    b, _ = _hip(c, shape, dev, mode)
    for n in ("Y", "DX", "dgamma", "dbeta"):
        assert torch.equal(a[n], b[n]), n


@pytest.mark.parametrize("shape,mode", [((2, 196, 768, 1, 0), "bf16"), ((2, 9, 12, 1, 1), "f32")])
def test_graph_capture(dev, shape, mode):
    """Forward + backward captured once on one stream; replayed on a new x it gives the eager bits, and
    the running buffers advance once per replay."""
    import torch
    import sae_vision_amd.ops as ops
    B, L, C, xl, yl = shape
    c, c2 = _case(shape, mode), _case(shape, mode, True)
    dt = _td(mode)
    xs, gamma, beta, base = _leaves(c, dev, mode)
    leaves = (xs, gamma, beta) + ((base,) if yl else ())
    dys = torch.tensor(c["dy"], device=dev).to(dt)
    rm, rv = _buffers(C, dev)

    def step():
        y = ops.bn_gelu(xs, gamma, beta, rm, rv, MOM, EPS, True, dt, xl, yl, base[:, :1] if yl else None)
        return (y,) + torch.autograd.grad(y, leaves, dys)

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
    eager, bufs = _hip(c_new, shape, dev, mode)
    for n, t in zip(("Y", "DX", "dgamma", "dbeta", "dbase"), outs):
        assert torch.equal(t, eager[n]), n
    assert torch.equal(rm, bufs[0]) and torch.equal(rv, bufs[1])
    graph.replay()
    _hip(c_new, shape, dev, mode, bufs)
    torch.cuda.synchronize()
    assert torch.equal(rm, bufs[0]) and torch.equal(rv, bufs[1])
    assert not torch.equal(rm, torch.zeros_like(rm))


# ------------------------------------------------------------------------------ LeFFBlock
ZERO = ("Dense_0.bias", "Conv_0.bias", "Dense_1.bias")   # each feeds a BatchNorm: its gradient is sum dx = 0


@functools.lru_cache(maxsize=None)
def _block_case(L, C, k, mode):
    """Parameters (the module's init under a fixed seed, BatchNorm parameters moved off theirs), inputs
    and the float64 block with every gradient, computed once.  Inputs are representable in the compute
    dtype; the parameters are the fp32 masters both routes cast themselves."""
    import torch
    import sae_vision_amd.layers as layers
    B = 2
    torch.manual_seed(L + C + k)
    mod = layers.LeFFBlock(expand_ratio=4, kernel_size=k, dtype=_td(mode), in_ch=C)
    rng = np.random.default_rng(7 * L + C + k)
    with torch.no_grad():
        for i in range(3):
            bn = getattr(mod, f"BatchNorm_{i}")
            bn.scale.copy_(torch.tensor(1 + 0.3 * rng.standard_normal(bn.scale.shape[0])))
            bn.bias.copy_(torch.tensor(0.3 * rng.standard_normal(bn.bias.shape[0])))
    x = randn(rng, (B, 1 + L, C), mode)
    dy = randn(rng, (B, 1 + L, C), mode)
    p = {n: t.detach().double().requires_grad_(True) for n, t in mod.named_parameters()}
    assert set(p) == set(R.PARAMS)
    x64 = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    y, batch, bn_in = R.leff_block(x64, p, k, EPS)
    for t in bn_in:
        t.retain_grad()
    y.backward(torch.tensor(dy, dtype=torch.float64))
    # the size of the terms that cancel in each zero gradient: max_c sum_rows |dx[:, c]| of its BatchNorm
    cancel = {n: float(t.grad.abs().reshape(-1, t.shape[-1]).sum(0).max()) for n, t in zip(ZERO, bn_in)}
    ref = dict(y=y.detach().numpy(), dx=x64.grad.numpy(), grads={n: t.grad.numpy() for n, t in p.items()},
               bufs={f"BatchNorm_{i}.{s}": (MOM * (s == "var") + (1 - MOM) * batch[i][j]).numpy()
                     for i in range(3) for j, s in enumerate(("mean", "var"))})
    return dict(state=copy.deepcopy(mod.state_dict()), x=x, dy=dy, ref=ref, cancel=cancel)


def _run_block(mod, c, dev, mode, timer=None):
    import torch
    import sae_vision_amd.ops as ops
    x = torch.tensor(c["x"], device=dev).to(_td(mode)).requires_grad_(True)
    ops.set_kernel_timer(timer)
    try:
        y = mod(x, is_training=True)
        y.backward(torch.tensor(c["dy"], device=dev).to(_td(mode)))
    finally:
        ops.set_kernel_timer(None)
    assert y.dtype == _td(mode) and y.shape == x.shape
    return dict(y=y.detach(), dx=x.grad, grads={n: p.grad for n, p in mod.named_parameters()},
                bufs=dict(mod.named_buffers()))


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("C", [16, 96])
@pytest.mark.parametrize("L", [9, 196])
def test_module_matches_framework_route_and_reference(dev, L, C, k, mode):
    """LeFFBlock, training forward + backward: the HIP route against a deep copy forced onto
    _framework_forward and against the float64 block.  fp32: both within TOL.  bf16: no further from
    the float64 block than TOL or twice the framework route's distance from it."""
    import sae_vision_amd.layers as layers
    import sae_vision_amd.ops as ops
    c = _block_case(L, C, k, mode)
    mod = layers.LeFFBlock(expand_ratio=4, kernel_size=k, dtype=_td(mode), in_ch=C, device=dev)
    mod.load_state_dict(c["state"])
    fwk = copy.deepcopy(mod)
    fwk.forward = fwk._framework_forward
    assert {a: set(b) for a, b in layers.flax_params(mod).items()} == {
        n: {"kernel", "bias"} if n[0] in "DC" else {"scale", "bias"}
        for n in ("Dense_0", "BatchNorm_0", "Conv_0", "BatchNorm_1", "Dense_1", "BatchNorm_2")}
    assert len(list(mod.named_buffers())) == 6
    timer = ops.KernelTimer()
    hip = _run_block(mod, c, dev, mode, timer)
    ref_route = _run_block(fwk, c, dev, mode)
    launches = {n: v["launches"] for n, v in timer.summary().items()}
    assert launches.get("bn_gelu_fwd") == 3 and launches.get("bn_gelu_bwd") == 3, launches
    assert launches.get("conv_tokens_fwd") == 1, launches
    ref = c["ref"]
    # the class token passes through, and takes the output's gradient of its row (plus nothing else)
    x16 = hip["y"].new_tensor(c["x"])
    assert (hip["y"][:, 0] == x16[:, 0]).all()
    assert rel_err(hip["dx"][:, 0], ref["dx"][:, 0]) <= TOL[mode]

    def pairs():
        yield "y", hip["y"], ref_route["y"], ref["y"]
        yield "dx", hip["dx"], ref_route["dx"], ref["dx"]
        for n in R.PARAMS:
            if n not in ZERO:
                yield n, hip["grads"][n], ref_route["grads"][n], ref["grads"][n]
        for n in ref["bufs"]:
            yield n, hip["bufs"][n], ref_route["bufs"][n], ref["bufs"][n]

    bad = {}
    for n, a, b, r64 in pairs():
        e_hip, e_fwk, e_ab = rel_err(a, r64), rel_err(b, r64), rel_err(a, b.float().cpu().numpy())
        print(n, "hip", e_hip, "framework", e_fwk, "hip vs framework", e_ab)
        if mode == "f32":
            ok = e_hip <= TOL["f32"] and e_ab <= TOL["f32"]
        else:
            ok = e_hip <= max(TOL["bf16"], 2 * e_fwk)
        if not ok:
            bad[n] = (e_hip, e_fwk, e_ab)
    assert not bad, f"(hip, framework, hip vs framework) errors: {bad}"
    # the three gradients that are zero in exact arithmetic: rounding noise, bounded against the size
    # of the terms that cancel
    for n in ZERO:
        g = float(hip["grads"][n].abs().max())
        print(n, g, "bound", TOL[mode] * c["cancel"][n])
        assert np.abs(ref["grads"][n]).max() <= 1e-9 * c["cancel"][n]
        assert g <= TOL[mode] * c["cancel"][n], (n, g, TOL[mode] * c["cancel"][n])


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_module_evaluation(dev, mode):
    """Evaluation without a gradient takes the HIP route (three single kernels, no conv backward),
    reads the running buffers and leaves them alone; with a gradient wanted it is the framework route."""
    import torch
    import sae_vision_amd.layers as layers
    import sae_vision_amd.ops as ops
    c = _block_case(9, 16, 3, mode)
    mod = layers.LeFFBlock(expand_ratio=4, kernel_size=3, dtype=_td(mode), in_ch=16, device=dev)
    mod.load_state_dict(c["state"])
    _run_block(mod, c, dev, mode)   # moves the buffers off their init values
    fwk = copy.deepcopy(mod)
    before = {n: b.clone() for n, b in mod.named_buffers()}
    x = torch.tensor(c["x"], device=dev).to(_td(mode))
    timer = ops.KernelTimer()
    ops.set_kernel_timer(timer)
    try:
        with torch.no_grad():
            y = mod(x, is_training=False)
        n_eval = timer.summary()["bn_gelu_fwd"]["launches"]
        y_grad = mod(x, is_training=False)   # parameters require gradients: no backward on the HIP route
    finally:
        ops.set_kernel_timer(None)
    assert n_eval == 3 and timer.summary()["bn_gelu_fwd"]["launches"] == 3
    with torch.no_grad():
        y_ref = fwk._framework_forward(x, False)
    assert rel_err(y, y_ref.float().cpu().numpy()) <= TOL[mode]
    assert torch.equal(y_grad, y_ref)
    assert all(torch.equal(b, before[n]) for n, b in mod.named_buffers())


@pytest.mark.parametrize("kw", [dict(in_ch=12, kernel_size=3), dict(in_ch=16, kernel_size=9),
                                dict(in_ch=16, kernel_size=3, activation_fn="relu")])
def test_fallback_is_the_framework_route(dev, kw):
    """Outside the envelope (12 channels in bf16; a 9x9 kernel; another activation) forward() is
    _framework_forward, bit for bit, and no bn_gelu kernel runs."""
    import torch
    import sae_vision_amd.layers as layers
    import sae_vision_amd.ops as ops
    kw = dict(kw)
    if "activation_fn" in kw:
        kw["activation_fn"] = torch.nn.functional.relu
    torch.manual_seed(1)
    blk = layers.LeFFBlock(expand_ratio=4, dtype=torch.bfloat16, device=dev, **kw)
    ref = copy.deepcopy(blk)
    x = torch.tensor(np.random.default_rng(2).standard_normal((2, 10, kw["in_ch"])).astype(np.float32), device=dev)
    timer = ops.KernelTimer()
    ops.set_kernel_timer(timer)
    try:
        y = blk(x, True)
    finally:
        ops.set_kernel_timer(None)
    assert "bn_gelu_fwd" not in timer.summary()
    y_ref = ref._framework_forward(x, True)
    assert torch.equal(y, y_ref)
    if "activation_fn" in kw:
        assert float(y.detach()[:, 1:].min()) >= 0   # that callable is what ran
    for (n, a), (_, b) in zip(blk.named_buffers(), ref.named_buffers()):
        assert torch.equal(a, b), n
