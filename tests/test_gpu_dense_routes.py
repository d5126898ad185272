"""Every route of ``ops.dense`` on the GPU: the launches it makes and the values it returns.

One case per pinned row of tests/_dense_rows.py that a device can run, at M <= 256 (the two GEMM_LIB rows at
4096 / 4097).  Each case spies ``ops.gemm_nt`` / ``ops.gemm_dw`` / ``ops.gemm_f32`` and asserts the
hard-coded sequence of calls (operand shapes, ``jblock``, ``offload``); a product on the library GEMM shows
as the absence of a call.  The expectations are written from the routing rules (tests/_dense_rows.py), not
from a run, and the file uses nothing but ``ops.dense``, the three wrappers, ``ops.GEMM_LIB`` and
``GradSinks``, so it states what any implementation of the routing must launch.

Values against float64 products of the same inputs: 1e-5 of the largest magnitude for dW / db (fp32
accumulation on sae_gemm_dw, as tests/test_gpu_gemm.py) and for everything on the fp32 route
(tests/test_gpu_gemm_f32.py); 2e-2 for bf16 results (y, dX, and a dW the library GEMM returns in bf16).
The sink cases run inside a ``GradSinks.backward()`` window over a buffer filled with ones: a gradient written
into its sink overwrites them and autograd gets None (the sink holds g, not g + 1 or 2 g), any other gradient
is added to them by autograd (g + 1); the listener sees the claimed sinks in claim order."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32


def NT(M, K, N):
    return ("nt", (M, K), (N, K))


def DW(x, dy, dw, jblock=0, offload=False):
    return ("dw", x, dy, dw, jblock, offload)


def F(a, b):
    return ("f32", a, b)


def _std(M, I, J, dw=None, jblock=0, offload=False):
    """forward and dX on sae_gemm_nt, one sae_gemm_dw launch"""
    return [NT(M, I, J), NT(M, J, I), DW((M, I), (M, J), dw or (I, J), jblock, offload)]


# (id, call, spied calls in order, sinks claimed in order, dW comes from the library in bf16)
CASES = [
    ("single", dict(M=256, I=64, widths=(128,)), _std(256, 64, 128), [], False),
    ("single_strided_dy", dict(M=256, I=64, widths=(128,), strided_dy=True), _std(256, 64, 128), [], False),
    ("blocks", dict(M=256, I=64, widths=(64, 64, 64)), _std(256, 64, 192, (3, 64, 64), 64), [], False),
    ("blocks_adjacent_sinks", dict(M=256, I=64, widths=(64, 64, 64), sinks=("w0", "w1", "w2", "b")),
     _std(256, 64, 192, (3, 64, 64), 64, True), ["b", "w0", "w1", "w2"], False),
    ("blocks_apart_sinks", dict(M=256, I=64, widths=(64, 64, 64), sinks=("w0", "w1", "w2", "b"), apart=True),
     _std(256, 64, 192, (3, 64, 64), 64), ["b"], False),
    ("blocks_some_sinks", dict(M=256, I=64, widths=(64, 64, 64), sinks=("w0", "w2")),
     _std(256, 64, 192, (3, 64, 64), 64), [], False),
    ("unequal_blocks", dict(M=256, I=64, widths=(64, 32)), _std(256, 64, 96), [], False),
    ("unequal_blocks_sinks", dict(M=256, I=64, widths=(64, 32), sinks=("w0", "w1", "b")), _std(256, 64, 96), [], False),
    ("blocks_of_6", dict(M=256, I=64, widths=(6, 6, 6, 6)), _std(256, 64, 24), [], False),
    ("head_1000", dict(M=128, I=128, widths=(1000,)), _std(128, 128, 1000), [], False),
    ("head_10", dict(M=24, I=64, widths=(10,)), [DW((10, 24), (10, 64), (24, 64))], [], True),
    ("head_10_m20", dict(M=20, I=64, widths=(10,)), [], [], True),
    ("in_12", dict(M=64, I=12, widths=(64,)), [], [], True),
    ("f32", dict(M=64, I=64, widths=(64,), dtype=F32),
     [F((64, 64), (64, 64)), F((64, 64), (64, 64)), F((64, 64), (64, 64))], [], False),
    ("f32_blocks_sinks", dict(M=64, I=128, widths=(64, 12), dtype=F32, sinks=("w0", "w1", "b")),
     [F((64, 128), (128, 76)), F((64, 76), (76, 128)), F((128, 64), (64, 64)), F((128, 64), (64, 12))],
     ["b", "w0", "w1"], False),
    ("f32_head_10", dict(M=64, I=64, widths=(10,), dtype=F32), [], [], False),
    ("lib_m4096", dict(M=4096, I=64, widths=(64,), gemm_lib=True),
     [NT(4096, 64, 64), DW((4096, 64), (4096, 64), (64, 64))], [], False),
    ("lib_m4097", dict(M=4097, I=64, widths=(64,), gemm_lib=True), [DW((4097, 64), (4097, 64), (64, 64))], [], False),
    ("sunk_bias_sink", dict(M=256, I=64, widths=(128,), sinks=("w0", "b")),
     _std(256, 64, 128, offload=True), ["b", "w0"], False),
    ("sunk_bias_no_sink", dict(M=256, I=64, widths=(128,), sinks=("w0",)), _std(256, 64, 128), ["w0"], False),
    ("sunk_no_bias", dict(M=256, I=64, widths=(128,), bias=False, sinks=("w0",)),
     _std(256, 64, 128, offload=True), ["w0"], False),
    ("blocks_sunk_bias_no_sink", dict(M=256, I=64, widths=(64, 64), sinks=("w0", "w1")),
     _std(256, 64, 128, (2, 64, 64), 64), ["w0", "w1"], False),
    ("blocks_sunk_no_bias", dict(M=256, I=64, widths=(64, 64), bias=False, sinks=("w0", "w1")),
     _std(256, 64, 128, (2, 64, 64), 64, True), ["w0", "w1"], False),
    ("unsunk_bias_sink", dict(M=256, I=64, widths=(128,), sinks=("b",)), _std(256, 64, 128), ["b"], False),
]


def _rel(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max())


def _spies(ops, monkeypatch, calls):
    real_nt, real_dw, real_f32 = ops.gemm_nt, ops.gemm_dw, ops.gemm_f32

    def nt(a2, bt, *a, **k):
        calls.append(NT(a2.shape[0], a2.shape[1], bt.shape[0]))
        assert bt.shape[1] == a2.shape[1]
        return real_nt(a2, bt, *a, **k)

    def dw(x2, dy2, dw, db=None, accumulate=False, jblock=0, offload=False):
        calls.append(DW(tuple(x2.shape), tuple(dy2.shape), tuple(dw.shape), jblock, offload))
        return real_dw(x2, dy2, dw, db, accumulate, jblock, offload)

    def f32(a, b, *r, **k):
        calls.append(F(tuple(a.shape), tuple(b.shape)))
        return real_f32(a, b, *r, **k)

    monkeypatch.setattr(ops, "gemm_nt", nt)
    monkeypatch.setattr(ops, "gemm_dw", dw)
    monkeypatch.setattr(ops, "gemm_f32", f32)


@pytest.mark.parametrize("call,want_calls,want_claimed,lib_dw", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_dense_route(dev, monkeypatch, call, want_calls, want_claimed, lib_dw):
    import sae_vision_amd.ops as ops
    from sae_vision_amd.sinks import GradSinks
    M, I, widths = call["M"], call["I"], call["widths"]
    dt, J = call.get("dtype", BF16), sum(widths)
    g = torch.Generator(device=dev).manual_seed(M + I + J)
    x = torch.randn(2, M // 2, I, device=dev, generator=g).to(dt) if M % 2 == 0 else \
        torch.randn(M, I, device=dev, generator=g).to(dt)
    x.requires_grad_()
    ws = [(torch.randn(I, n, device=dev, generator=g) * 0.05).requires_grad_() for n in widths]
    b = torch.randn(J, device=dev, generator=g).requires_grad_() if call.get("bias", True) else None
    dy = torch.randn(*x.shape[:-1], J + 8, device=dev, generator=g).to(dt)
    dy = dy[..., :J] if call.get("strided_dy") else dy[..., :J].contiguous()
    params = {f"w{k}": w for k, w in enumerate(ws)}
    if b is not None:
        params["b"] = b

    # sinks: views of one flat buffer of ones, back to back in parameter order (or 16 floats apart)
    names = call.get("sinks", ())
    gap = 16 if call.get("apart") else 0
    flat = torch.ones(sum(params[n].numel() + gap for n in names), device=dev)
    views, at = {}, 0
    for n in names:
        views[n] = flat[at:at + params[n].numel()].view(params[n].shape)
        params[n].grad = views[n]
        at += params[n].numel() + gap
    heard = []
    sinks = GradSinks([params[n] for n in names], [views[n] for n in names], listener=heard.append)

    calls = []
    _spies(ops, monkeypatch, calls)
    monkeypatch.setattr(ops, "GEMM_LIB", call.get("gemm_lib", False))
    with sinks.backward():
        y = ops.dense(x, ws if len(ws) > 1 else ws[0], b, dt)
        y.backward(dy)
    torch.cuda.synchronize()
    assert calls == want_calls
    by_ptr = {v.data_ptr(): n for n, v in views.items()}
    assert [by_ptr[p] for p in heard] == want_claimed

    exact = dt == F32
    xd = x.detach().double().reshape(M, I)
    wd = torch.cat([w.detach() for w in ws], dim=1).to(dt).double()
    dyd = dy.double().reshape(M, J)
    ref_y = xd @ wd + (b.detach().double() if b is not None else 0)
    assert y.dtype == dt and y.shape == (*x.shape[:-1], J)
    assert _rel(y.detach().reshape(M, J), ref_y) <= (1e-5 if exact else 2e-2)
    assert x.grad.dtype == dt
    assert _rel(x.grad.reshape(M, I), dyd @ wd.t()) <= (1e-5 if exact else 2e-2)
    ref = {"b": dyd.sum(0)}
    for k, r in enumerate((xd.t() @ dyd).split(list(widths), dim=1)):
        ref[f"w{k}"] = r
    for n, p in params.items():
        got = p.grad.double()
        if n in views:
            assert p.grad.data_ptr() == views[n].data_ptr(), n   # still the sink
            if n not in want_claimed:
                got = got - 1                                    # added by autograd onto the ones
        assert p.grad.dtype == F32
        assert _rel(got, ref[n]) <= (2e-2 if lib_dw and n != "b" else 1e-5), n
