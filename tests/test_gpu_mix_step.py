"""TrainStep with mixup / cutmix targets and in-step metrics (``mix=True``, ``metrics=True``) and the
evaluation step (train.EvalStep: the reference's eval_step, train.py:112-120, with top-k and a
device accumulator), eager and as captured graphs."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, CLASSES, IMG = 8, 10, 64


def _vit(dev, **kw):
    from sae_vision_amd import vit
    torch.manual_seed(0)
    m = vit.ViT(CLASSES, 2, 3, 192, (16, 16), IMG, 4, torch.bfloat16, dev, **kw)
    with torch.no_grad():   # the head starts at zero (every logit tied): give the ranks something to order
        m.Dense_0.kernel.normal_(0.0, 0.5)
    return m


def _cait(dev):
    from sae_vision_amd import cait
    torch.manual_seed(0)
    m = cait.CaiT(num_classes=CLASSES, num_layers=2, num_layers_token_only=2, num_heads=4, embed_dim=192,
                  patch_shape=(16, 16), stoch_depth_rate=0.2, layerscale_eps=1e-5, img_size=IMG,
                  dtype=torch.bfloat16, device=dev)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("layerscale"):
                p.fill_(1.0)
        m.Dense_0.kernel.normal_(0.0, 0.5)
    return m


def _batches(dev, n=4, seed=3):
    g = torch.Generator(device=dev).manual_seed(seed)
    out = []
    for _ in range(n):
        out.append((torch.randn(B, IMG, IMG, 3, device=dev, generator=g),
                    torch.randint(0, CLASSES, (B,), device=dev, generator=g),
                    torch.randint(0, CLASSES, (B,), device=dev, generator=g),
                    torch.rand(B, device=dev, generator=g)))
    return out


def _close(steps):
    for s in steps:
        s.close()


def test_mix_graph_step_matches_eager(dev):
    """Every call brings its own mix_labels and ratio: a replay that read a stale static buffer
    would leave the eager step's losses and parameters."""
    from sae_vision_amd import train
    m_e = _vit(dev)
    m_g = copy.deepcopy(m_e)
    s_e = train.TrainStep(m_e, global_batch=B, device=dev, mix=True, flat_grads=False)
    s_g = train.TrainStep(m_g, global_batch=B, device=dev, mix=True, graph=True)
    try:
        data = _batches(dev)
        le = [float(s_e(*d)) for d in data]
        lg = [float(s_g(*d)) for d in data]
        assert s_g._g is not None
        assert s_g.mix_buffers()[0].data_ptr() == s_g._mix_labels.data_ptr() and s_g.mix_buffers()[1].dtype == torch.float32
        assert len(s_g.input_buffers()) == 2
        for a, b in zip(le, lg):
            assert abs(a - b) <= 1e-3 * abs(a), (le, lg)
        for (n, pe), pg in zip(m_e.named_parameters(), m_g.parameters()):
            err = float((pe - pg).detach().abs().max())
            assert err <= 1e-3 * max(1.0, float(pe.detach().abs().max())), (n, err)
    finally:
        _close((s_e, s_g))


def test_mix_with_ratio_one_is_the_plain_step(dev):
    from sae_vision_amd import train
    m_a = _vit(dev)
    m_b = copy.deepcopy(m_a)
    s_a = train.TrainStep(m_a, global_batch=B, device=dev, graph=True)
    s_b = train.TrainStep(m_b, global_batch=B, device=dev, graph=True, mix=True)
    try:
        ones = torch.ones(B, device=dev)
        for x, y, y1, _ in _batches(dev, 3):
            la, lb = s_a(x, y).clone(), s_b(x, y, y1, ones).clone()
            assert torch.equal(la, lb)
        assert s_a.mix_buffers() is None and s_a.top1 is None and s_b.top1 is None
        for (n, pa), pb in zip(m_a.named_parameters(), m_b.parameters()):
            assert torch.equal(pa, pb), n
    finally:
        _close((s_a, s_b))


@pytest.mark.parametrize("graph", [False, True])
def test_step_metrics_are_the_batch_topk(dev, graph):
    from sae_vision_amd import train
    m = _vit(dev)
    step = train.TrainStep(m, global_batch=B, device=dev, graph=graph, mix=True, metrics=True)
    try:
        for x, y, y1, rho in _batches(dev):
            with torch.no_grad():
                logits = m(x, True).float().cpu().numpy()
            step(x, y, y1, rho)
            order = np.argsort(logits, axis=1, kind="stable")
            yn = y.cpu().numpy()
            for k, got in ((1, step.top1), (5, step.top5)):
                want = (order[:, -k:] == yn[:, None]).any(axis=1).sum()
                assert got.dim() == 0 and got.is_cuda
                assert float(got) == want / B, (k, float(got), want)
        assert (step._g is not None) == graph
        with pytest.raises(ValueError, match="every call needs"):
            step(x, y)
    finally:
        step.close()
    plain = train.TrainStep(_vit(dev), global_batch=B, device=dev)
    with pytest.raises(ValueError, match="need mix=True"):
        plain(x, y, y1, rho)
    plain.close()


def _reference_eval(model, batches):
    """float64 cross entropy and stable-argsort counts on the eager logits of ``model``."""
    loss, top1, top5, n = 0.0, 0, 0, 0
    for x, y in batches:
        with torch.no_grad():
            z = model(x, is_training=False).float().cpu().numpy().astype(np.float64)
        yn = y.cpu().numpy()
        zmax = z.max(axis=1, keepdims=True)
        lse = zmax[:, 0] + np.log(np.exp(z - zmax).sum(axis=1))
        loss += float((lse - z[np.arange(len(yn)), yn]).sum())
        order = np.argsort(z, axis=1, kind="stable")
        top1 += int((order[:, -1:] == yn[:, None]).any(axis=1).sum())
        top5 += int((order[:, -5:] == yn[:, None]).any(axis=1).sum())
        n += len(yn)
    return {"loss": loss / n, "top_1_acc": top1 / n, "top_5_acc": top5 / n, "samples": n}


def _assert_result(got, want):
    print("eval", got, "reference", want)
    assert abs(got["loss"] - want["loss"]) <= 1e-5 * abs(want["loss"]), (got, want)
    assert {k: got[k] for k in ("top_1_acc", "top_5_acc", "samples")} == \
           {k: want[k] for k in ("top_1_acc", "top_5_acc", "samples")}


def test_eval_graph_matches_eager(dev):
    from sae_vision_amd import train
    m = _vit(dev)
    batches = [(x, y) for x, y, _, _ in _batches(dev, 3, seed=11)]
    e_e = train.EvalStep(m, device=dev)
    e_g = train.EvalStep(m, device=dev, graph=True)
    try:
        for x, y in batches:
            le, lg = e_e(x, y), e_g(x, y)
            assert le.dim() == 0 and le.is_cuda and torch.equal(le, lg)
        assert e_g._g is not None and len(e_g.input_buffers()) == 2
        assert torch.equal(e_e._acc, e_g._acc)
        want = _reference_eval(m, batches)
        _assert_result(e_e.result(), want)
        _assert_result(e_g.result(), want)
        assert 0 < want["top_5_acc"] < 1
        e_g.reset()
        assert e_g.result() == {"loss": 0.0, "top_1_acc": 0.0, "top_5_acc": 0.0, "samples": 0}
    finally:
        e_g.close()


@pytest.mark.parametrize("model", ["vit", "cait"])
def test_eval_after_training_reads_the_current_weights(dev, model):
    """The replayed evaluation graph must not serve the bf16 copies of the weights it was captured
    with: after two optimizer updates it equals a fresh eager forward on the current weights.  CaiT:
    with stoch_depth_rate > 0, so evaluation runs with stochastic depth off."""
    from sae_vision_amd import train
    m = _vit(dev) if model == "vit" else _cait(dev)
    data = _batches(dev, 3, seed=13)
    batches = [(x, y) for x, y, _, _ in data]
    ev = train.EvalStep(m, device=dev, graph=True)
    step = None
    try:
        for x, y in batches:
            ev(x, y)
        before = ev.result()
        _assert_result(before, _reference_eval(m, batches))
        step = train.TrainStep(m, global_batch=B, device=dev, graph=True, lr=0.1)   # x batch / 512: steps of 1.6e-3
        for x, y, _, _ in data[:2]:
            step(x, y)
        ev.reset()
        for x, y in batches:
            ev(x, y)
        after = ev.result()
        _assert_result(after, _reference_eval(m, batches))
        assert after["loss"] != before["loss"]
        # ... and once more with the graph that was captured beside the optimizer's copies
        step(*data[2][:2])
        ev.reset()
        for x, y in batches:
            ev(x, y)
        _assert_result(ev.result(), _reference_eval(m, batches))
        assert ev._g is not None and step._g is not None
        # the optimizer lets go of the copies and the weights change in place: the evaluation
        # captures again, now holding the casts itself
        # (a replay of the old graph would read the closed optimizer's buffers, which nothing
        # updates any more, and miss the reference below; the identity of the graph object then
        # shows how the step got it right: a fresh capture, not a fall-back to the eager step)
        captured = ev._g
        step.close()
        with torch.no_grad():
            m.Dense_0.kernel.mul_(0.5)
        ev.reset()
        for x, y in batches:
            ev(x, y)
        _assert_result(ev.result(), _reference_eval(m, batches))
        assert ev._g is not None and ev._g is not captured
    finally:
        ev.close()
        if step is not None:
            step.close()


@pytest.mark.parametrize("graph", [False, True])
def test_eval_with_dropout_is_deterministic_and_leaves_state_alone(dev, graph):
    from sae_vision_amd import ops, train
    m = _vit(dev, dropout_rate=0.25)
    batches = [(x, y) for x, y, _, _ in _batches(dev, 2, seed=17)]
    # some parameters with a gradient, some without
    m(batches[0][0], is_training=True).float().sum().backward()
    m.cls.grad = None
    grads = {n: (None if p.grad is None else p.grad.clone()) for n, p in m.named_parameters()}
    rng = ops.dropout_rng(dev).state.clone()
    ev = train.EvalStep(m, device=dev, graph=graph)
    try:
        results = []
        for _ in range(2):
            ev.reset()
            for x, y in batches:
                ev(x, y)
            results.append(ev.result())
        assert results[0] == results[1] and results[0]["samples"] == 2 * B
        _assert_result(results[0], _reference_eval(m, batches))
        assert torch.equal(ops.dropout_rng(dev).state, rng) and (ev._g is not None) == graph
        for n, p in m.named_parameters():
            if grads[n] is None:
                assert p.grad is None, n
            else:
                assert torch.equal(p.grad, grads[n]), n
    finally:
        ev.close()
