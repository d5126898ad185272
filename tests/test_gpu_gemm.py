"""Projection-gradient kernel (sae_gemm_dw) against a float64 reference of the same bf16 inputs.

dW = X^T dY and db = colsum(dY) are what the JAX autodiff of the reference's Dense /
DenseGeneral projections computes (attention.py:29-37,60-63; ff.py:8-34); the kernel sums in
fp32, so the bar is fp32 accumulation error (1e-5 of the largest magnitude)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [  # (M, I, J)
    (25216, 384, 1152),   # DeiT-S QKV projection, batch 128
    (25216, 1536, 384),   # DeiT-S FF Dense_1
    (197, 768, 1000),     # ragged tokens, head-like J
    (3000, 768, 1000),    # two wave groups, an odd stage count per group (10 stages per chunk)
    (4616, 768, 2304),    # ViT-B QKV-like output (108 tiles > 64): one wave group per workgroup
    (1000, 24, 40),       # tiny, I/J below one tile
    (64, 8, 8),
]


@pytest.mark.parametrize("M,I,J", SHAPES)
@pytest.mark.parametrize("bias", [False, True])
def test_gemm_dw(dev, M, I, J, bias):
    import sae_vision_amd.ops as ops
    g = torch.Generator(device=dev).manual_seed(M + I + J)
    x = torch.randn(M, I, device=dev, generator=g).to(torch.bfloat16)
    dy = torch.randn(M, J, device=dev, generator=g).to(torch.bfloat16)
    dw = torch.empty(I, J, device=dev)
    db = torch.empty(J, device=dev) if bias else None
    ops.gemm_dw(x, dy, dw, db)
    ref = (x.double().t() @ dy.double())
    err = float((dw.double() - ref).abs().max() / ref.abs().max())
    assert err <= 1e-5, err
    if bias:
        rb = dy.double().sum(0)
        assert float((db.double() - rb).abs().max() / rb.abs().max()) <= 1e-5


def test_gemm_dw_accumulate_strided(dev):
    """accumulate=True adds into an existing gradient; x / dy may be column slices of wider rows."""
    import sae_vision_amd.ops as ops
    g = torch.Generator(device=dev).manual_seed(7)
    M, I, J = 3000, 128, 256
    xw = torch.randn(M, I + 64, device=dev, generator=g).to(torch.bfloat16)
    dyw = torch.randn(M, J + 8, device=dev, generator=g).to(torch.bfloat16)
    x, dy = xw[:, 64:], dyw[:, :J]
    dw0 = torch.randn(I, J, device=dev, generator=g)
    db0 = torch.randn(J, device=dev, generator=g)
    dw, db = dw0.clone(), db0.clone()
    ops.gemm_dw(x, dy, dw, db, accumulate=True)
    ref = dw0.double() + x.double().t() @ dy.double()
    assert float((dw.double() - ref).abs().max() / ref.abs().max()) <= 1e-5
    rb = db0.double() + dy.double().sum(0)
    assert float((db.double() - rb).abs().max() / rb.abs().max()) <= 1e-5


def test_gemm_dw_deterministic(dev):
    import sae_vision_amd.ops as ops
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(25216, 384, device=dev, generator=g).to(torch.bfloat16)
    dy = torch.randn(25216, 384, device=dev, generator=g).to(torch.bfloat16)
    a, b = torch.empty(384, 384, device=dev), torch.empty(384, 384, device=dev)
    ops.gemm_dw(x, dy, a)
    ops.gemm_dw(x, dy, b)
    assert torch.equal(a, b)


def test_dense_grads_match_autograd(dev):
    """ops.dense (library fwd / dX, HIP dW / db) against float64 products of the same bf16 values."""
    import sae_vision_amd.ops as ops
    g = torch.Generator(device=dev).manual_seed(11)
    x = torch.randn(4, 197, 384, device=dev, generator=g).to(torch.bfloat16).requires_grad_()
    w = (torch.randn(384, 1152, device=dev, generator=g) * 0.05).requires_grad_()
    b = torch.randn(1152, device=dev, generator=g).requires_grad_()
    dy = torch.randn(4, 197, 1152, device=dev, generator=g).to(torch.bfloat16)
    y = ops.dense(x, w, b, torch.bfloat16)
    y.backward(dy)
    xd, wd = x.detach().double(), w.detach().to(torch.bfloat16).double()
    ref_w = xd.reshape(-1, 384).t() @ dy.double().reshape(-1, 1152)
    assert float((w.grad.double() - ref_w).abs().max() / ref_w.abs().max()) <= 1e-5
    ref_b = dy.double().reshape(-1, 1152).sum(0)
    assert float((b.grad.double() - ref_b).abs().max() / ref_b.abs().max()) <= 1e-5
    ref_x = dy.double() @ wd.t()
    assert float((x.grad.double() - ref_x).abs().max() / ref_x.abs().max()) <= 2e-2



@pytest.mark.parametrize("rows,C", [(32, 768), (128, 384)])
def test_classifier_head_dense(dev, rows, C):
    """The classifier head (C -> 1000 classes: K = 1000 is a multiple of 8 but not of 64 in the input
    gradient) runs on the HIP kernels: forward and dX on sae_gemm_nt (dX on its K-tail row), dW / db on
    sae_gemm_dw; against float64 products of the same bf16 values.  (A class count that is no multiple
    of 8 takes the "dw_t" route: test_small_head_dgrad_on_gemm_dw.)"""
    import sae_vision_amd.ops as ops
    g = torch.Generator(device=dev).manual_seed(rows)
    x = torch.randn(rows, C, device=dev, generator=g).to(torch.bfloat16).requires_grad_()
    w = (torch.randn(C, 1000, device=dev, generator=g) * 0.05).requires_grad_()
    b = torch.randn(1000, device=dev, generator=g).requires_grad_()
    dy = torch.randn(rows, 1000, device=dev, generator=g).to(torch.bfloat16)
    y = ops.dense(x, w, b, torch.bfloat16)
    wd = w.detach().to(torch.bfloat16).double()
    ref_y = x.detach().double() @ wd + b.detach().double()
    assert float((y.double() - ref_y).abs().max() / ref_y.abs().max()) <= 2e-2
    y.backward(dy)
    ref_x = dy.double() @ wd.t()
    assert float((x.grad.double() - ref_x).abs().max() / ref_x.abs().max()) <= 2e-2
    ref_w = x.detach().double().t() @ dy.double()
    assert float((w.grad.double() - ref_w).abs().max() / ref_w.abs().max()) <= 1e-5


@pytest.mark.parametrize("rows,C,J", [(16, 192, 10), (128, 384, 10), (24, 768, 37)])
def test_small_head_dgrad_on_gemm_dw(dev, monkeypatch, rows, C, J):
    """A small-M classifier head whose class count J is not a multiple of 8 (e.g. 10 classes): the
    input gradient dX = dY W^T reduces over J, so it runs on the weight-gradient kernel over the
    ROWS of dY^T [J, M] and the bf16 W^T [J, C] the forward saved (ops.py: the "dw_t" route of dense_bwd_plan); the
    test asserts that route is taken (not the library GEMM) and checks dX against float64."""
    import sae_vision_amd.ops as ops
    calls = []
    real = ops.gemm_dw

    def spy(x2, dy2, dw, *a, **k):
        calls.append((tuple(x2.shape), tuple(dy2.shape), tuple(dw.shape)))
        return real(x2, dy2, dw, *a, **k)

    monkeypatch.setattr(ops, "gemm_dw", spy)
    g = torch.Generator(device=dev).manual_seed(rows + J)
    x = torch.randn(rows, C, device=dev, generator=g).to(torch.bfloat16).requires_grad_()
    w = (torch.randn(C, J, device=dev, generator=g) * 0.05).requires_grad_()
    b = torch.randn(J, device=dev, generator=g).requires_grad_()
    dy = torch.randn(rows, J, device=dev, generator=g).to(torch.bfloat16)
    y = ops.dense(x, w, b, torch.bfloat16)
    y.backward(dy)
    assert ((J, rows), (J, C), (rows, C)) in calls, calls   # dX = (dY^T)^T W^T on sae_gemm_dw
    wd = w.detach().to(torch.bfloat16).double()
    ref_x = dy.double() @ wd.t()
    assert float((x.grad.double() - ref_x).abs().max() / ref_x.abs().max()) <= 2e-2


def test_gemm_dw_blocked_layout(dev):
    """sae_gemm_dw_blocked: dW in contiguous column blocks [J/jb, I, jb] equals the plain layout."""
    import sae_vision_amd.ops as ops
    g = torch.Generator(device=dev).manual_seed(17)
    M, I, J, jb = 3000, 384, 1152, 384
    x = torch.randn(M, I, device=dev, generator=g).to(torch.bfloat16)
    dy = torch.randn(M, J, device=dev, generator=g).to(torch.bfloat16)
    dw = torch.empty(I, J, device=dev)
    db = torch.empty(J, device=dev)
    ops.gemm_dw(x, dy, dw, db)
    dwb = torch.empty(J // jb, I, jb, device=dev)
    db2 = torch.empty(J, device=dev)
    ops.gemm_dw(x, dy, dwb, db2, jblock=jb)
    for k in range(J // jb):
        assert torch.equal(dwb[k], dw[:, k * jb:(k + 1) * jb])
    assert torch.equal(db, db2)
