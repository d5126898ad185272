"""The loss against mixup / cutmix targets with top-k ranks (sae_mixed_ce_fwd / _bwd, train.py:83-90
with ``mix_labels`` / ``ratio``, utils.topk_correct of train.py:98-99) and the evaluation accumulator
(sae_ce_accumulate).

Parity: torch's cross entropy with probability targets in fp32 on the same logits, to the bounds
tests/test_gpu_loss.py holds the one-label arithmetic to (loss 1e-5 relative; dlogits 1e-6 of
max|grad| for fp32 logits, one bf16 rounding 2^-8 for bf16 logits).  Bit-exactness against
``ops.smoothed_cross_entropy`` without a partner label and with ratio == 1.  Top-k: exact on every row
against ``np.argsort(kind="stable")``, under heavy ties, NaN and -0."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(128, 1000), (7, 10), (300, 37), (1, 1000), (4, 512), (5, 3)]


def _mix_case(dev, R, K, dt, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = (3 * torch.randn(R, K, device=dev, generator=g)).to(dt)
    y0 = torch.randint(0, K, (R,), device=dev, generator=g)
    y1 = torch.randint(0, K, (R,), device=dev, generator=g)
    rho = torch.rand(R, device=dev, generator=g)
    rho[0::5] = 0.0            # the partner alone
    rho[1::5] = 1.0            # the first label alone
    y1[2::5] = y0[2::5]        # both labels the same class
    return x, y0, y1, rho


@pytest.mark.parametrize("R,K", SHAPES)
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("alpha", [0.1, 0.0])
def test_mixed_ce_matches_torch(dev, R, K, dt, alpha):
    from sae_vision_amd import ops
    x, y0, y1, rho = _mix_case(dev, R, K, dt, R * K + 1)
    xa = x.clone().requires_grad_(True)
    xr = x.float().clone().requires_grad_(True)
    loss = ops.mixed_cross_entropy(xa, y0, y1, rho, alpha)
    target = rho[:, None] * F.one_hot(y0, K).float() + (1 - rho[:, None]) * F.one_hot(y1, K).float()
    ref = F.cross_entropy(xr, target, label_smoothing=alpha)
    lv, rv = float(loss.detach()), float(ref.detach())
    print("loss", lv, "ref", rv)
    assert abs(lv - rv) <= 1e-5 * abs(rv), (lv, rv)
    (1.7 * loss).backward()
    (1.7 * ref).backward()
    assert xa.grad.dtype == dt
    tol = 1e-6 if dt == torch.float32 else 2 ** -8
    err = float((xa.grad.float() - xr.grad).abs().max() / xr.grad.abs().max())
    print("grad err", err)
    assert err <= tol, err


def _loss_and_grad(fn, x):
    xa = x.clone().requires_grad_(True)
    out = fn(xa)
    (0.6 * out).backward()
    return out.detach(), xa.grad


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("alpha", [0.1, 0.0])
def test_mixed_ce_bit_exact_against_one_label_loss(dev, dt, alpha):
    """No partner label, ratio == 1 with any partner, and metrics=True: the bits of
    ops.smoothed_cross_entropy, loss and gradient; also on a row-strided view, and on a second call.
    ops.smoothed_cross_entropy is the no-partner form, so these pairs compare the kernels' paths with
    each other (RANK off / on, mix NULL / set); test_ce_bits_are_the_parent_kernels below holds them all
    to recorded bits."""
    from sae_vision_amd import ops
    for R, K in SHAPES:
        x, y0, y1, _ = _mix_case(dev, R, K, dt, 7 * R + K)
        ones = torch.ones(R, device=dev)
        l0, g0 = _loss_and_grad(lambda t: ops.smoothed_cross_entropy(t, y0, alpha), x)
        l1, g1 = _loss_and_grad(lambda t: ops.mixed_cross_entropy(t, y0, alpha=alpha), x)
        l2, g2 = _loss_and_grad(lambda t: ops.mixed_cross_entropy(t, y0, y1, ones, alpha), x)
        l3, g3 = _loss_and_grad(lambda t: ops.mixed_cross_entropy(t, y0, alpha=alpha, metrics=True)[0], x)
        for l, g in ((l1, g1), (l2, g2), (l3, g3)):
            assert torch.equal(l, l0) and torch.equal(g, g0), (R, K)
    g = torch.Generator(device=dev).manual_seed(1)
    big = torch.randn(64, 1024, device=dev, generator=g).to(dt)
    x = big[:, :1000]
    y0 = torch.randint(0, 1000, (64,), device=dev, generator=g)
    y1 = torch.randint(0, 1000, (64,), device=dev, generator=g)
    rho = torch.rand(64, device=dev, generator=g)
    ones = torch.ones(64, device=dev)
    assert x.stride(0) == 1024 and not x.is_contiguous()

    def on_view(fn):
        """Loss and gradient with the kernels reading the row-strided view itself (ld = 1024 != K):
        the leaf is the padded buffer, the slice is what the loss sees."""
        leaf = big.clone().requires_grad_(True)
        out = fn(leaf[:, :1000])
        (0.6 * out).backward()
        assert float(leaf.grad[:, 1000:].abs().max()) == 0.0   # nothing written past the K columns
        return out.detach(), leaf.grad[:, :1000]

    l0, g0 = on_view(lambda t: ops.smoothed_cross_entropy(t, y0, alpha))
    l1, g1 = on_view(lambda t: ops.mixed_cross_entropy(t, y0, alpha=alpha))
    l2, g2 = on_view(lambda t: ops.mixed_cross_entropy(t, y0, y1, ones, alpha))
    for l, gr in ((l1, g1), (l2, g2)):
        assert torch.equal(l, l0) and torch.equal(gr, g0)
    # a random ratio: the view against its contiguous copy, and a second call, loss and gradient
    la, ga = on_view(lambda t: ops.mixed_cross_entropy(t, y0, y1, rho, alpha))
    lb, gb = on_view(lambda t: ops.mixed_cross_entropy(t, y0, y1, rho, alpha))
    lc, gc = _loss_and_grad(lambda t: ops.mixed_cross_entropy(t, y0, y1, rho, alpha), x.contiguous())
    assert torch.equal(la, lb) and torch.equal(ga, gb)
    assert torch.equal(la, lc) and torch.equal(ga, gc)
    assert not torch.equal(ga, g0)                             # the partner labels were felt


def _ce_bits():
    """tests/golden/make_ce_bits.py as a module: the cases, their seeded inputs and the digest."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_ce_bits.py")
    spec = importlib.util.spec_from_file_location("make_ce_bits", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _smoothed_ce_c_abi(x, y0, alpha, upstream):
    """``(loss, row_loss, dlogits)`` from sae_smoothed_ce_fwd / _bwd called directly."""
    import sae_vision_amd
    from sae_vision_amd import _lib as L
    lib = sae_vision_amd.load_library()
    R, K = x.shape
    f32 = dict(dtype=torch.float32, device=x.device)
    lse, row_loss, loss = torch.empty(R, **f32), torch.empty(R, **f32), torch.empty((), **f32)
    g = torch.tensor(upstream, **f32)
    dx = torch.empty(R, K, dtype=x.dtype, device=x.device)
    st = torch.cuda.current_stream(x.device).cuda_stream
    code = L.SAE_DTYPE_BF16 if x.dtype == torch.bfloat16 else L.SAE_DTYPE_F32
    L.check(lib.sae_smoothed_ce_fwd(st, R, K, x.data_ptr(), x.stride(0), code, y0.data_ptr(), alpha, lse.data_ptr(),
                                    row_loss.data_ptr(), loss.data_ptr()))
    L.check(lib.sae_smoothed_ce_bwd(st, R, K, x.data_ptr(), x.stride(0), code, y0.data_ptr(), alpha, lse.data_ptr(),
                                    g.data_ptr(), dx.data_ptr(), dx.stride(0)))
    return loss, row_loss, dx


def test_ce_bits_are_the_parent_kernels(dev):
    """Every form of the one-label loss -- ops.smoothed_cross_entropy, the mixed loss without a partner,
    with ratio == 1, with metrics=True, and the sae_smoothed_ce_* entry points called directly -- gives
    the loss, row losses and dlogits whose SHA-256 digests tests/golden/ce_parent_bits.json records:
    the bits of the separate smoothed_ce_* kernels the loss had before it became one family.

    The file is made by tests/golden/make_ce_bits.py, which uses only API older than that change.  When
    the toolchain changes the bits, regenerate it on the PARENT of the toolchain bump (check that
    commit out, build it with the new toolchain, run the script there, copy the file here): never from
    the code under test."""
    from sae_vision_amd import ops
    M = _ce_bits()
    with open(os.path.join(os.path.dirname(M.__file__), "ce_parent_bits.json")) as f:
        doc = json.load(f)
    keys = []
    for key, R, K, pitch, dt, alpha in M.cases():
        keys.append(key)
        want = doc["cases"][key]
        x, y0, y1 = M.case_inputs(dev, R, K, pitch, dt)
        ones = torch.ones(R, device=dev)

        def rows(mix, ratio, metrics):
            """(loss, row_loss, dlogits) of one form of ops.mixed_cross_entropy_rows"""
            kept = []

            def fn(t):
                out = ops.mixed_cross_entropy_rows(t, y0, mix, ratio, alpha, metrics)
                kept.append(out[2])
                return out[0]
            loss, dx = M.loss_and_grad(fn, x)
            return loss, kept[0], dx

        l0, g0 = M.loss_and_grad(lambda t: ops.smoothed_cross_entropy(t, y0, alpha), x)
        forms = {"smoothed": (l0, None, g0), "no partner": rows(None, None, False), "ratio 1": rows(y1, ones, False),
                 "metrics": rows(None, None, True), "C ABI": _smoothed_ce_c_abi(x, y0, alpha, M.UPSTREAM)}
        for form, got in forms.items():
            for name, t in zip(("loss", "row_loss", "dlogits"), got):
                if t is not None:
                    assert M.digest(t) == want[name], (key, form, name)
    assert sorted(keys) == sorted(doc["cases"]) and doc["upstream_gradient"] == M.UPSTREAM


def _stable_topk(x: np.ndarray, y: np.ndarray, k: int) -> np.ndarray:
    """utils.topk_correct with numpy's stable argsort: is the label among the last k of the order?"""
    order = np.argsort(x, axis=1, kind="stable")
    return (order[:, -k:] == y[:, None]).any(axis=1)


def _check_topk(ops, x, y):
    R, K = x.shape
    loss, top1, top5 = ops.mixed_cross_entropy(x, y, alpha=0.0, metrics=True)
    rank = ops.mixed_cross_entropy_rows(x, y, None, None, 0.0, True)[3].cpu().numpy()
    xn, yn = x.float().cpu().numpy(), y.cpu().numpy()
    for k, top in ((1, top1), (5, top5)):
        ref = _stable_topk(xn, yn, k)
        assert np.array_equal(rank < k, ref), (K, k, np.nonzero((rank < k) != ref)[0][:8])
        assert float(top) == np.float32(ref.sum()) / np.float32(R)
    # the full rank, not only its first five values: the label's distance from the end of the order
    order = np.argsort(xn, axis=1, kind="stable")
    pos = (order == yn[:, None]).argmax(axis=1)
    assert np.array_equal(rank, K - 1 - pos)


@pytest.mark.parametrize("K", [3, 5, 6, 37, 1000])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_topk_is_the_stable_argsort_under_ties_nan_and_negative_zero(dev, K, dt):
    from sae_vision_amd import ops
    R = 256
    g = torch.Generator(device=dev).manual_seed(K)
    x = torch.randint(-3, 4, (R, K), device=dev, generator=g).float()
    u = torch.rand(R, K, device=dev, generator=g)
    x[u < 0.02] = float("nan")
    x[(u >= 0.02) & (u < 0.07)] = -0.0
    y = torch.randint(0, K, (R,), device=dev, generator=g)
    _check_topk(ops, x.to(dt), y)


def test_topk_label_tied_at_the_fifth_place(dev):
    """bf16 3 randn at K = 1000: rows whose 5th and 6th largest logits are equal, the label put at the
    6th place of the stable order.  A count of strictly greater logits calls these rows top-5."""
    from sae_vision_amd import ops
    g = torch.Generator(device=dev).manual_seed(5)
    x = (3 * torch.randn(2048, 1000, device=dev, generator=g)).to(torch.bfloat16)
    xn = x.float().cpu().numpy()
    order = np.argsort(xn, axis=1, kind="stable")
    rows = np.arange(xn.shape[0])
    tied = xn[rows, order[:, -5]] == xn[rows, order[:, -6]]
    assert tied.sum() >= 32, tied.sum()
    y = torch.from_numpy(np.where(tied, order[:, -6], order[:, -5])).to(dev)
    keep = torch.from_numpy(np.nonzero(tied)[0][:256]).to(dev)
    xs, ys = x[keep].contiguous(), y[keep]
    strictly_greater = (xs.float() > xs.float().gather(1, ys[:, None])).sum(1)
    assert int((strictly_greater < 5).sum()) == xs.shape[0]       # the naive count gets every row wrong
    rank = ops.mixed_cross_entropy_rows(xs, ys, None, None, 0.0, True)[3]
    assert int((rank == 5).sum()) == xs.shape[0]
    _check_topk(ops, xs, ys)
    _check_topk(ops, x[:256].contiguous(), y[:256])              # tied and untied rows mixed


def test_label_outside_the_classes(dev):
    from sae_vision_amd import ops
    x = torch.randn(4, 10, device=dev)
    y = torch.tensor([3, -1, 10, 0], device=dev)
    rank = ops.mixed_cross_entropy_rows(x, y, None, None, 0.0, True)[3].cpu()
    assert int(rank[1]) == 10 and int(rank[2]) == 10 and 0 <= int(rank[0]) < 10


def test_ce_accumulate(dev):
    from sae_vision_amd import ops
    acc = torch.zeros(4, dtype=torch.int64, device=dev)
    g = torch.Generator(device=dev).manual_seed(9)
    want_loss, want1, want5, n = 0.0, 0, 0, 0
    for R in (8, 300, 1):
        x = (3 * torch.randn(R, 37, device=dev, generator=g)).to(torch.bfloat16)
        y = torch.randint(0, 37, (R,), device=dev, generator=g)
        _, _, row_loss, rank = ops.mixed_cross_entropy_rows(x, y, None, None, 0.0, True)
        ops.ce_accumulate(row_loss, rank, acc)
        want_loss += float(np.sum(row_loss.cpu().numpy().astype(np.float64)))
        want1 += int((rank < 1).sum())
        want5 += int((rank < 5).sum())
        n += R
    loss_sum, top1, top5, samples = ops.read_ce_accumulator(acc)
    print("loss_sum", loss_sum, "want", want_loss)
    assert abs(loss_sum - want_loss) <= 1e-6 * abs(want_loss)
    assert (top1, top5, samples) == (want1, want5, n) and 0 < top5 < n
    acc.zero_()
    assert ops.read_ce_accumulator(acc) == (0.0, 0, 0, 0)
    ops.ce_accumulate(row_loss, rank, acc)
    assert ops.read_ce_accumulator(acc)[3] == 1


def test_mixed_ce_refusals(dev):
    from sae_vision_amd import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.mixed_cross_entropy(torch.randn(2, 5), torch.zeros(2, dtype=torch.int64))
    x = torch.randn(2, 5, device=dev)
    y = torch.zeros(2, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="go together"):
        ops.mixed_cross_entropy(x, y, ratio=torch.ones(2, device=dev))
    with pytest.raises(ValueError, match="go together"):
        ops.mixed_cross_entropy(x, y, mix_labels=y)
