"""GPU tests of the CvT model (sae_vision_amd/cvt.py) on a tiny configuration: 64 px, batch 2, 10
classes, stage_sizes (1, 1, 2), heads (1, 2, 2), embed_dim (32, 64, 64) -- grids 16 x 16, 8 x 8, then
16 + 1 = 17 tokens zero-padded to 5 x 5.  fp32 against the float64 reference of _cvt_ref.py, bf16
against the same model with its stems on the framework route, evaluation, and the captured
training step against the eager one."""
import copy
import functools

import numpy as np
import pytest

import _cvt_ref as R
from _util import TOL, rel_err

pytestmark = pytest.mark.gpu

SIZES, HEADS, DIMS, CLASSES, PX, BATCH = (1, 1, 2), (1, 2, 2), (32, 64, 64), 10, 64, 2
ZERO = "ConvProjectionBlock_1.BatchNorm_0.bias"   # zero in exact arithmetic, see _check_grads


def _model(dev, dtype):
    """The tiny CvT with the head kernel, the class token and the BatchNorm parameters and statistics
    away from their init values (a zero head would make every trunk gradient zero)."""
    import torch
    from sae_vision_amd import cvt
    torch.manual_seed(0)
    m = cvt.CvT(CLASSES, SIZES, HEADS, DIMS, dtype=dtype)   # built on the CPU: the same init on every device
    rng = np.random.default_rng(1)
    t = lambda a: torch.tensor(np.asarray(a, np.float32))
    with torch.no_grad():
        m.Dense_0.kernel.copy_(t(rng.standard_normal((DIMS[-1], CLASSES)) / 8))
        m.Stage_2.cls.copy_(t(0.5 * rng.standard_normal((1, 1, DIMS[-1]))))
        for n, p in m.named_parameters():
            if n.endswith("BatchNorm_0.scale"):
                p.copy_(t(1 + 0.3 * rng.standard_normal(p.shape)))
            elif n.endswith("BatchNorm_0.bias"):
                p.copy_(t(0.3 * rng.standard_normal(p.shape)))
        for n, b in m.named_buffers():
            b.copy_(t(0.2 * rng.standard_normal(b.shape)) if n.endswith("mean") else t(1 + 0.5 * rng.random(b.shape)))
    return m.to(dev)


@functools.lru_cache(maxsize=None)
def _data():
    rng = np.random.default_rng(2)
    return (rng.standard_normal((BATCH, PX, PX, 3)).astype(np.float32),
            rng.standard_normal((BATCH, CLASSES)).astype(np.float32))


def _tree64(m):
    """The model's Flax tree as float64 CPU leaves, and ``{parameter name: leaf}``."""
    import torch
    tree, leaves = {}, {}
    for name, p in m.named_parameters():
        node, parts = tree, name.split(".")
        for part in parts[:-1]:
            node = node.setdefault(part, {})
        leaves[name] = node[parts[-1]] = p.detach().double().cpu().requires_grad_(True)
    return tree, leaves


def _stats64(m):
    bufs = {n: b.detach().double().cpu() for n, b in m.named_buffers()}
    return {n[:-5]: (bufs[n], bufs[n[:-5] + ".var"]) for n in bufs if n.endswith(".mean")}


@functools.lru_cache(maxsize=None)
def _reference(training):
    """float64: logits, parameter gradients (training) and the statistics after the call, once."""
    import torch
    m = _model(torch.device("cpu"), torch.float32)
    x, dlogits = _data()
    tree, leaves = _tree64(m)
    logits, stats = R.cvt(torch.tensor(x, dtype=torch.float64), tree, _stats64(m), SIZES, HEADS, training=training)
    grads = {}
    if training:
        logits.backward(torch.tensor(dlogits, dtype=torch.float64))
        grads = {n: t.grad.numpy() for n, t in leaves.items()}
    return logits.detach().numpy(), grads, {n: (a.numpy(), b.numpy()) for n, (a, b) in stats.items()}


def _train_once(m, dev):
    import torch
    x, dlogits = _data()
    m.zero_grad(set_to_none=True)
    logits = m(torch.tensor(x, device=dev), is_training=True)
    logits.float().backward(torch.tensor(dlogits, device=dev))
    return logits.detach()


def _check_grads(got, ref, tol):
    """Every gradient within tol of the reference's (max-norm).  The key projection's BatchNorm bias
    shifts every key by one vector, which moves each query's scores by a constant the softmax does not
    see: its gradient is zero in exact arithmetic and rounding noise in either route, so its error is
    measured against the largest BatchNorm-bias gradient of its block's three projections."""
    assert set(got) == set(ref)
    for n in sorted(got):
        if n.endswith(ZERO):
            block = n[:-len(ZERO)]
            scale = max(np.abs(ref[f"{block}ConvProjectionBlock_{i}.BatchNorm_0.bias"]).max() for i in range(3))
            err = float(np.abs(got[n] - ref[n]).max() / scale)
            assert np.abs(ref[n]).max() <= tol * scale, n
        else:
            err = rel_err(got[n], ref[n])
        print(n, err)
        assert err <= tol, (n, err)


def test_f32_matches_the_float64_reference(dev):
    import torch
    m = _model(dev, torch.float32)
    ref_logits, ref_grads, ref_stats = _reference(True)
    logits = _train_once(m, dev)
    err = rel_err(logits, ref_logits)
    print("logits", err)
    assert tuple(logits.shape) == (BATCH, CLASSES) and err <= TOL["f32"], err
    _check_grads({n: p.grad.double().cpu().numpy() for n, p in m.named_parameters()}, ref_grads, TOL["f32"])
    for n, (mean, var) in _stats64(m).items():
        assert rel_err(mean, ref_stats[n][0]) <= TOL["f32"] and rel_err(var, ref_stats[n][1]) <= TOL["f32"], n


@functools.lru_cache(maxsize=None)
def _bf16_pair(dev):
    """One training forward + backward of the bf16 model (HIP stems, timed) and of a deep copy whose stems
    are forced onto _framework_forward: (logits, gradients, buffers) of each and the launch counts."""
    import torch
    import sae_vision_amd.ops as ops
    from sae_vision_amd import cvt
    m = _model(dev, torch.bfloat16)
    ref = copy.deepcopy(m)
    for mod in ref.modules():
        if isinstance(mod, cvt.ConvTokenEmbedBlock):
            mod.forward = mod._framework_forward
    timer = ops.KernelTimer()
    ops.set_kernel_timer(timer)
    try:
        logits = _train_once(m, dev)
    finally:
        ops.set_kernel_timer(None)
    launches = {k: v["launches"] for k, v in timer.summary().items()}
    ref_logits = _train_once(ref, dev)
    pack = lambda mod, lg: (lg, {n: p.grad.double().cpu().numpy() for n, p in mod.named_parameters()},
                            {n: b.double().cpu().numpy() for n, b in mod.named_buffers()})
    return pack(m, logits), pack(ref, ref_logits), launches


def test_bf16_stems_launch_the_kernels(dev):
    _, _, launches = _bf16_pair(dev)
    assert launches.get("conv_tokens_fwd") == 3 and launches.get("conv_tokens_bwd") == 3, launches
    # stages 2 and 3 take an input gradient, the image batch does not
    assert launches.get("conv_window_scatter") == 2 and launches.get("conv_tokens_dp") == 2, launches


def test_bf16_logits_and_statistics_match_the_framework_stems(dev):
    import torch
    (logits, _, bufs), (ref_logits, _, ref_bufs), _ = _bf16_pair(dev)
    err = rel_err(logits, ref_logits.float().cpu().numpy())
    print("logits", err)
    assert logits.dtype == torch.bfloat16 and err <= TOL["bf16"], err
    for n in bufs:
        e = rel_err(bufs[n], ref_bufs[n])
        print(n, e)
        assert e <= TOL["bf16"], (n, e)


def test_bf16_gradients_match_the_framework_stems(dev):
    """Every parameter gradient of the bf16 model against the deep copy with framework stems, within
    TOL["bf16"] = 2e-2 (max-norm).  The two routes round at the same points (operands at bf16, fp32
    sums, one rounding of the output), so they part only by summation order: measured 1.2e-2 at most.
    Either route is 3e-3 .. 7e-2 from the fp32 model at this size (bf16 noise of the whole network at
    batch 2), which is why the comparison is route against route."""
    (_, grads, _), (_, ref_grads, _), _ = _bf16_pair(dev)
    _check_grads(grads, ref_grads, TOL["bf16"])


def test_evaluation(dev):
    import torch
    m = _model(dev, torch.float32)
    before = {n: b.clone() for n, b in m.named_buffers()}
    x, _ = _data()
    with torch.no_grad():
        logits = m(torch.tensor(x, device=dev), is_training=False)
    ref_logits, _, _ = _reference(False)
    err = rel_err(logits, ref_logits)
    print("logits", err)
    assert err <= TOL["f32"], err
    for n, b in m.named_buffers():
        assert torch.equal(b, before[n]), n
    # the train-step feed layout [H, W, C, N] is rearranged by the model
    with torch.no_grad():
        again = m(torch.tensor(x, device=dev).permute(1, 2, 3, 0).contiguous(), is_training=False, layout="HWCN")
    assert torch.equal(again, logits)


def test_graph_step_matches_eager_bits(dev):
    """TrainStep(graph=True) over three steps: the loss bits and the BatchNorm statistics of an eager
    TrainStep from the same initial state (the warm-up before the capture leaves no trace in them)."""
    import torch
    from sae_vision_amd import train
    m_e = _model(dev, torch.bfloat16)
    m_g = copy.deepcopy(m_e)
    s_e = train.TrainStep(m_e, global_batch=BATCH, device=dev)
    s_g = train.TrainStep(m_g, global_batch=BATCH, device=dev, graph=True)
    g = torch.Generator(device=dev).manual_seed(3)
    data = [(torch.randn(BATCH, PX, PX, 3, device=dev, generator=g),
             torch.randint(0, CLASSES, (BATCH,), device=dev, generator=g)) for _ in range(3)]
    try:
        for x, y in data:
            le, lg = s_e(x, y).clone(), s_g(x, y).clone()
            assert s_g._g is not None                                  # captured, not fallen back to eager
            assert bool(torch.isfinite(le)) and torch.equal(le, lg), (float(le), float(lg))
            for (n, b), (_, b2) in zip(m_e.named_buffers(), m_g.named_buffers()):
                assert torch.equal(b, b2), n
        moved = [n for (n, b), (_, b0) in zip(m_g.named_buffers(), _model(dev, torch.bfloat16).named_buffers())
                 if not torch.equal(b, b0)]
        assert len(moved) == len(list(m_g.named_buffers()))
    finally:
        s_g.close()
        s_e.close()
