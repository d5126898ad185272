"""Ownership of the training step's host state, on CPU tensors: a GradSinks (sinks.py) holds one
step's gradient sinks and is seen by the ops only inside its own backward() window; the registry
of bf16 weight copies (ops._CASTS) drops entries by parameter and by owner.  No kernel runs: the
sink-writing op is a stand-in that goes through ops._sink / _grad_out / _unsunk / _sinking exactly
as the HIP ops' backwards do, and the registry's one cast launch is replaced by a stub."""
import pytest
import torch

from sae_vision_amd import ops
from sae_vision_amd.sinks import GradSinks

_LOG = []   # ("returned", data_ptr) from the stand-in's backward, ("heard", data_ptr) from a listener


class _Lin(torch.autograd.Function):
    """y = x @ w with dW written into w's sink when the open window has one (as ops._Dense does)."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        ctx.sink = ops._sink(w)
        return x @ w

    @staticmethod
    @ops._sinking
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dw = ops._grad_out(ctx.sink, w.shape, w.device)
        dw.copy_(x.t() @ dy)
        _LOG.append(("returned", dw.data_ptr()))
        return dy @ w.t(), ops._unsunk(dw, ctx.sink)


def _params(seed, fill=0.0):
    """Two [6, 6] parameters whose .grad are views of one flat buffer filled with ``fill``."""
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(6, 6, generator=g)) for _ in range(2)]
    flat = torch.full((72,), fill)
    for i, p in enumerate(ps):
        p.grad = flat[36 * i:36 * (i + 1)].view(6, 6)
    return ps, flat


def _loss(ps, x):
    return _Lin.apply(_Lin.apply(x, ps[0]), ps[1]).sum()


def _reference(ps, x):
    ws = [p.detach().clone().requires_grad_() for p in ps]
    _loss(ws, x).backward()
    return [w.grad for w in ws]


X = torch.randn(5, 6, generator=torch.Generator().manual_seed(9))


def test_window_sinks_its_own_parameters_only():
    pa, fa = _params(1, fill=1.0)
    pb, fb = _params(2, fill=1.0)
    sa, sb = GradSinks(pa, [p.grad for p in pa]), GradSinks(pb, [p.grad for p in pb])
    ra, rb = _reference(pa, X), _reference(pb, X)
    with sa.backward():
        (_loss(pa, X) + _loss(pb, X)).backward()
    assert sa.written == {p.grad.data_ptr() for p in pa} and not sb.written
    for p, r in zip(pa, ra):
        assert torch.equal(p.grad, r)            # written over the ones, not added to them
    for p, r in zip(pb, rb):
        assert torch.equal(p.grad, 1.0 + r)      # left to autograd: accumulated
    assert torch.equal(fa, torch.cat([r.flatten() for r in ra]))
    # outside every window nothing is sunk: autograd accumulates into A's views too
    (_loss(pa, X)).backward()
    for p, r in zip(pa, ra):
        assert torch.equal(p.grad, r + r)
    assert sa.written == {p.grad.data_ptr() for p in pa}   # still readable after the window closed


def test_second_claim_in_one_window_raises():
    ps, _ = _params(3)
    with GradSinks(ps, [p.grad for p in ps]).backward():
        _loss(ps, X).backward()
        msg = "gradient sink written twice in one backward: a parameter feeds two ops"
        with pytest.raises(RuntimeError, match=msg):
            _loss(ps, X).backward()


def test_replaced_grad_is_not_sunk():
    ps, flat = _params(4)
    sinks = GradSinks(ps, [p.grad for p in ps])
    ps[0].grad = torch.zeros(6, 6)               # replaced: the registered view is no longer the .grad
    ref = _reference(ps, X)
    with sinks.backward():
        _loss(ps, X).backward()
    assert sinks.written == {ps[1].grad.data_ptr()}
    assert float(flat[:36].abs().max()) == 0.0   # the old view stays zero
    assert torch.equal(ps[0].grad, ref[0]) and torch.equal(ps[1].grad, ref[1])


def test_listener_hears_each_sink_once_after_its_backward_returns():
    ps, _ = _params(5)
    heard = lambda ptr: _LOG.append(("heard", ptr))
    del _LOG[:]
    with GradSinks(ps, [p.grad for p in ps], listener=heard).backward():
        _loss(ps, X).backward()
    p0, p1 = ps[0].grad.data_ptr(), ps[1].grad.data_ptr()
    # the backward runs ps[1]'s op first; each op's sink is reported right after that op returns
    assert _LOG == [("returned", p1), ("heard", p1), ("returned", p0), ("heard", p0)]


def test_nested_window_raises_and_a_failed_body_closes_it():
    pa, _ = _params(6)
    pb, _ = _params(7)
    sa, sb = GradSinks(pa, [p.grad for p in pa]), GradSinks(pb, [p.grad for p in pb])
    with sa.backward():
        for inner in (sa, sb):
            with pytest.raises(RuntimeError, match="already open"):
                with inner.backward():
                    pass
        assert ops._ACTIVE_SINKS is sa           # the refused entry left the open window alone
    assert ops._ACTIVE_SINKS is None
    with pytest.raises(KeyError):
        with sa.backward():
            raise KeyError("body failed")
    assert ops._ACTIVE_SINKS is None
    with sb.backward():                          # ... so the next window opens
        assert ops._sink(pb[0]) is not None and ops._sink(pa[0]) is None


def test_sink_must_match_its_parameter():
    p = torch.nn.Parameter(torch.zeros(4, 4))
    for bad in (torch.zeros(4, 4, dtype=torch.float64), torch.zeros(4, 8)[:, ::2], torch.zeros(16)):
        with pytest.raises(ValueError, match="fp32 contiguous view shaped like its parameter"):
            GradSinks([p], [bad])


# ------------------------------------------------------------------- registry of the bf16 copies
@pytest.fixture
def casts(monkeypatch):
    """The registry with its cast launch stubbed (entries become current, nothing runs): the
    number of entries of each would-be launch."""
    launches = []

    def stub(entries):
        for e in entries:
            e.versions = ops._versions(e.weights)
        launches.append(len(entries))
    monkeypatch.setattr(ops, "_run_casts", stub)
    monkeypatch.setattr(ops, "_CASTS", {})
    return launches


def _group(*widths, K=8):
    ws = [torch.zeros(K, n) for n in widths]
    N = sum(widths)
    return ws, torch.zeros(K, N, dtype=torch.bfloat16), torch.zeros(N, K, dtype=torch.bfloat16)


def test_release_by_parameter(casts):
    (g1, a1, t1), (g2, a2, t2) = _group(4, 12), _group(8)
    ops.register_persistent_casts([g1, g2], [a1, a2], [t1, t2], owner=object())
    assert casts == [2]                          # registering casts both groups, one launch
    assert ops._cast_lookup(g1)[0] is a1 and ops._cast_lookup(g2)[1] is t2
    ops.release_persistent_casts([g1[1]])        # one member is enough to drop its whole group
    assert ops._cast_lookup(g1) is None and ops._cast_lookup(g2)[0] is a2
    ops.release_persistent_casts([torch.zeros(8, 8)])   # a stranger releases nothing
    assert ops._cast_lookup(g2)[0] is a2


def test_unregister_is_owner_scoped(casts):
    (g, a, t), (h, ah, th) = _group(8), _group(4)
    first, second = object(), object()
    ops.register_persistent_casts([g, h], [a, ah], [t, th], owner=first)
    a2, t2 = torch.zeros_like(a), torch.zeros_like(t)
    ops.register_persistent_casts([g], [a2], [t2], owner=second)   # a later registration takes over
    ops.unregister_persistent_casts(first)                         # ... and outlives the first owner's close
    assert ops._cast_lookup(g)[0] is a2 and ops._cast_lookup(h) is None
    ops.unregister_persistent_casts(second)
    assert ops._cast_lookup(g) is None
    with pytest.raises(ValueError):
        ops.register_persistent_casts([g], [a], [t], owner=None)


def test_refresh_and_forward_casts(casts):
    (g1, a1, t1), (g2, _, _), (g3, _, _) = _group(4, 4), _group(8), _group(16)
    ops.register_persistent_casts([g1], [a1], [t1], owner=object())
    del casts[:]
    ops.refresh_persistent_casts([g1, g2], only_if_stale=True)
    assert casts == []                                             # nothing moved: no launch
    g1[0].add_(1.0)
    ops.refresh_persistent_casts([g1, g2], only_if_stale=True)
    ops.refresh_persistent_casts([g1, g2])
    assert casts == [1, 1]                                         # g2 is not registered
    bad = [torch.zeros(8, 4), torch.zeros(4, 4)]                   # mixed K: skipped
    with ops.forward_casts([g1, g2, bad, [torch.zeros(8, 4, dtype=torch.float64)]]):
        assert casts == [1, 1, 1]                                  # g2 only; g1 is the optimizer's
        assert ops._cast_lookup(g1)[0] is a1 and ops._cast_lookup(g2) is not None
        assert ops._cast_lookup(bad) is None
        with ops.forward_casts([g3]):
            assert ops._cast_lookup(g3) is not None
        assert ops._cast_lookup(g3) is None and ops._cast_lookup(g2) is not None   # only what it added
        g2[0].add_(1.0)
        assert ops._cast_lookup(g2) is None                        # a per-forward entry gone stale
    assert ops._cast_lookup(g2) is None and ops._cast_lookup(g1)[0] is a1
    with ops.forward_casts([g3]):
        ops.clear_weight_cache()                                   # per-forward entries only
        assert ops._cast_lookup(g3) is None and ops._cast_lookup(g1)[0] is a1
    assert ops._cast_lookup(g3) is None
