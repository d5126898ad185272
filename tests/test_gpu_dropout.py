"""GPU tests of the attention-probability dropout (sae_attn_fwd_dropout / sae_attn_bwd_dropout):
the device mask against the numpy definition bit for bit, forward / backward parity against the
fp64 helper with that mask on every route, the layers, and the training step (eager and captured).

Tolerances (north_star, tests/_util.py): fp32 max|a-b|/max|ref| <= 1e-5, bf16 <= 2e-2."""
import copy
import math

import numpy as np
import pytest

import _dropout_ref as DR
import attention_ref as R
from _util import TOL, randn, rel_err

pytestmark = pytest.mark.gpu

SEED = 1234


def _td(mode):
    import torch
    return torch.bfloat16 if mode == "bf16" else torch.float32


def _rng(dev, seed=SEED, offset=0):
    import sae_vision_amd.ops as ops
    r = ops.DropoutRng(seed, dev)
    r.seed(seed, offset)
    return r


# ---------------------------------------------------------------------------- mask equality
@pytest.mark.parametrize("shape", [(2, 3, 197, 197), (1, 2, 1, 130), (1, 1, 33, 513)])
@pytest.mark.parametrize("rate", [0.1, 0.5])
@pytest.mark.parametrize("offset", [0, 2 ** 32 + 5])
@pytest.mark.parametrize("sid", [0, 7])
def test_mask_equals_definition(dev, shape, rate, offset, sid):
    import sae_vision_amd.ops as ops
    keep = ops.dropout_mask(*shape, rate, _rng(dev, SEED, offset), sid).cpu().numpy()
    assert set(np.unique(keep)) <= {0, 1}
    assert np.array_equal(keep.astype(bool), DR.keep_mask(*shape, rate, SEED, offset, sid))


# ----------------------------------------------------------------------------------- parity
CASES = [
    # B, Nq, Nk, H, D, mode                       route / what it covers
    (2, 197, 197, 3, 64, "bf16"),                # DeiT layer: Nk <= 256, a 5-key tail tile
    (1, 130, 300, 2, 64, "bf16"),                # Nk > 256, Nq != Nk
    (2, 196, 196, 2, 48, "bf16"),                # head_dim 48 in 64-wide tiles
    (2, 100, 37, 3, 32, "bf16"),                 # head_dim 32
    (1, 49, 49, 2, 128, "bf16"),                 # head_dim 128
    (2, 1, 197, 4, 48, "bf16"),                  # Nq = 1
    (2, 17, 17, 3, 64, "f32"),
    (1, 129, 65, 1, 64, "f32"),
    (3, 16, 16, 4, 10, "f32"),                   # unaligned head_dim
]


def _inputs(B, Nq, Nk, H, D, mode):
    rng = np.random.default_rng(0)
    q, k, v = (randn(rng, (B, n, H, D), mode) for n in (Nq, Nk, Nk))
    do = randn(np.random.default_rng(2), (B, Nq, H, D), mode)
    return q, k, v, do


def _run(dev, q, k, v, do, mode, rate, rng):
    """One forward + backward through ops.attention with dropout: (o, dq, dk, dv) as torch tensors."""
    import torch
    import sae_vision_amd.ops as ops
    td = _td(mode)
    tq, tk, tv = (torch.tensor(x, device=dev, dtype=td, requires_grad=True) for x in (q, k, v))
    o = ops.attention(tq, tk, tv, dropout=(rate, rng))
    o.backward(torch.tensor(do, device=dev, dtype=td))
    torch.cuda.synchronize()
    return o.detach(), tq.grad, tk.grad, tv.grad


@pytest.mark.parametrize("rate", [0.1, 0.5])
@pytest.mark.parametrize("B,Nq,Nk,H,D,mode", CASES)
def test_dropout_fwd_bwd(dev, B, Nq, Nk, H, D, mode, rate):
    q, k, v, do = _inputs(B, Nq, Nk, H, D, mode)
    o, dq, dk, dv = _run(dev, q, k, v, do, mode, rate, _rng(dev))      # a fresh state: stream id 0
    keep = DR.keep_mask(B, H, Nq, Nk, rate, SEED, 0, 0)
    o_ref, _ = DR.fwd(q, k, v, keep, rate)
    g = DR.bwd(q, k, v, do, keep, rate)
    errs = {"o": rel_err(o, o_ref), "dq": rel_err(dq, g["dq"]), "dk": rel_err(dk, g["dk"]),
            "dv": rel_err(dv, g["dv"])}
    print(errs)
    for name, e in errs.items():
        assert e <= TOL[mode], f"{name}: rel err {e:.3e}"


@pytest.mark.parametrize("rate", [0.1, 0.5])
def test_dropout_packed(dev, rate):
    """The packed [B, N, 3, H, D] form: q / k / v read and dq / dk / dv written in place by strides."""
    import torch
    import sae_vision_amd.ops as ops
    B, N, H, D = 2, 197, 3, 64
    q, k, v, do = _inputs(B, N, N, H, D, "bf16")
    qkv = torch.tensor(np.stack([q, k, v], axis=2), device=dev, dtype=torch.bfloat16, requires_grad=True)
    o = ops.attention_packed(qkv, dropout=(rate, _rng(dev)))
    o.backward(torch.tensor(do, device=dev, dtype=torch.bfloat16))
    torch.cuda.synchronize()
    keep = DR.keep_mask(B, H, N, N, rate, SEED, 0, 0)
    assert rel_err(o, DR.fwd(q, k, v, keep, rate)[0]) <= TOL["bf16"]
    g = DR.bwd(q, k, v, do, keep, rate)
    for i, name in enumerate(("dq", "dk", "dv")):
        e = rel_err(qkv.grad[:, :, i], g[name])
        assert e <= TOL["bf16"], f"{name}: rel err {e:.3e}"


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_dropout_lse_is_undropped(dev, mode):
    import torch
    import sae_vision_amd.ops as ops
    B, N, H, D = 2, 197, 3, 64
    rng = np.random.default_rng(0)
    q, k, v = (randn(rng, (B, N, H, D), mode) for _ in range(3))
    r = _rng(dev)
    _, lse = ops._fwd(*(torch.tensor(x, device=dev, dtype=_td(mode)) for x in (q, k, v)), 1.0 / math.sqrt(D),
                      drop=(0.5, r.state, 0))
    _, aux = R.attention_core_fwd(q, k, v, "f64", return_aux=True)
    np.testing.assert_allclose(lse.cpu().numpy(), aux["lse"], rtol=0, atol=1e-4 if mode == "f32" else 2e-2)


def test_dropout_is_deterministic_until_advanced(dev):
    import torch
    q, k, v, do = _inputs(2, 197, 197, 3, 64, "bf16")
    a = _run(dev, q, k, v, do, "bf16", 0.1, _rng(dev))
    b = _run(dev, q, k, v, do, "bf16", 0.1, _rng(dev))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    r = _rng(dev)
    r.advance()
    c = _run(dev, q, k, v, do, "bf16", 0.1, r)
    assert int(r.state[1]) == 1 and not torch.equal(a[0], c[0])
    keep = DR.keep_mask(2, 3, 197, 197, 0.1, SEED, 1, 0)               # the advanced offset, by the definition
    assert rel_err(c[0], DR.fwd(q, k, v, keep, 0.1)[0]) <= TOL["bf16"]


@pytest.mark.parametrize("B,Nq,Nk,H,D,mode", [(2, 197, 197, 3, 64, "bf16"), (2, 17, 17, 3, 64, "f32"),
                                              (1, 49, 49, 2, 128, "bf16")])
def test_rate_zero_is_bit_identical(dev, B, Nq, Nk, H, D, mode):
    """T == 0 (rate 0, and any rate below 1 / 512) forwards to the plain entry points."""
    import torch
    import sae_vision_amd.ops as ops
    q, k, v, do = _inputs(B, Nq, Nk, H, D, mode)
    td = _td(mode)
    tq, tk, tv = (torch.tensor(x, device=dev, dtype=td, requires_grad=True) for x in (q, k, v))
    o = ops.attention(tq, tk, tv)
    o.backward(torch.tensor(do, device=dev, dtype=td))
    plain = (o.detach(), tq.grad, tk.grad, tv.grad)
    for rate in (0.0, 0.0019):
        for x, y in zip(plain, _run(dev, q, k, v, do, mode, rate, _rng(dev))):
            assert torch.equal(x, y)


@pytest.mark.parametrize("B,N,H,D,mode", [(2, 197, 3, 64, "bf16"), (2, 17, 3, 64, "f32")])
def test_rescale_applied_once(dev, B, N, H, D, mode):
    """With v = 1 every column of o is rowsum(P o m), with do = 1 every column of dv is its column
    sum: a 1 / pk applied twice or never shows as a factor."""
    q, k, _, _ = _inputs(B, N, N, H, D, mode)
    ones = np.ones((B, N, H, D), np.float32)
    rate = 0.5
    o, _, _, dv = _run(dev, q, k, ones, ones, mode, rate, _rng(dev))
    keep = DR.keep_mask(B, H, N, N, rate, SEED, 0, 0)
    _, pk = DR.threshold(rate)
    pm = DR.probs(q, k)[0] * (keep / pk)                                # [B, H, Nq, Nk]
    o_ref = np.broadcast_to(pm.sum(-1).transpose(0, 2, 1)[..., None], (B, N, H, D))
    dv_ref = np.broadcast_to(pm.sum(-2).transpose(0, 2, 1)[..., None], (B, N, H, D))
    assert rel_err(o, o_ref) <= TOL[mode] and rel_err(dv, dv_ref) <= TOL[mode]


# ----------------------------------------------------------------------------------- layers
def _block_ref(mod, xq, xkv, keep, rate):
    """The module's math (attention.py:29-63 with dropout on the probabilities) in torch fp64 on the
    CPU, weights rounded to the compute dtype as the module casts them; returns (y, leaves)."""
    import torch
    H = mod.num_heads
    leaves = {n: p.detach().to(mod.dtype).double().cpu().requires_grad_(True) for n, p in mod.named_parameters()}
    q = torch.einsum("bnc,chd->bnhd", xq, leaves["queries.kernel"])
    k = torch.einsum("bnc,chd->bnhd", xkv, leaves["keys.kernel"])
    v = torch.einsum("bnc,chd->bnhd", xkv, leaves["values.kernel"])
    D = q.shape[-1]
    p = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", q, k) / math.sqrt(D), dim=-1)
    _, pk = DR.threshold(rate)
    p = p * torch.tensor(keep / pk, dtype=torch.float64)
    o = torch.einsum("bhqk,bkhd->bqhd", p, v)
    assert o.shape[2] == H
    return torch.einsum("bnhd,hdc->bnc", o, leaves["DenseGeneral_0.kernel"]), leaves


@pytest.mark.parametrize("kind", ["self", "cross", "class"])
def test_layers_with_dropout(dev, kind):
    import torch
    import sae_vision_amd.ops as ops
    from sae_vision_amd import layers
    torch.manual_seed(0)
    B, N, C, H, rate = 2, 50, 192, 3, 0.25
    cls = {"self": layers.SelfAttentionBlock, "cross": layers.AttentionBlock,
           "class": layers.ClassSelfAttentionBlock}[kind]
    mod = cls(num_heads=H, attn_dropout_rate=rate, dtype=torch.bfloat16, in_ch=C, device=dev)
    rng = np.random.default_rng(3)
    x = randn(rng, (B, N, C), "bf16")
    xq_np = {"self": x, "cross": randn(rng, (B, 20, C), "bf16"), "class": x[:, 0:1]}[kind]
    dy = randn(rng, xq_np.shape, "bf16")
    tx = torch.tensor(x, device=dev, dtype=torch.bfloat16)
    ops.seed_dropout(11)
    if kind == "cross":
        y = mod(torch.tensor(xq_np, device=dev, dtype=torch.bfloat16), tx, is_training=True)
    else:
        y = mod(tx, is_training=True)
    y.backward(torch.tensor(dy, device=dev, dtype=torch.bfloat16))
    torch.cuda.synchronize()
    keep = DR.keep_mask(B, H, xq_np.shape[1], N, rate, 11, 0, 0)
    y_ref, leaves = _block_ref(mod, torch.tensor(xq_np, dtype=torch.float64), torch.tensor(x, dtype=torch.float64),
                               keep, rate)
    y_ref.backward(torch.tensor(dy, dtype=torch.float64))
    assert rel_err(y, y_ref.detach().numpy()) <= 2e-2
    for n, p in mod.named_parameters():
        e = rel_err(p.grad, leaves[n].grad.numpy())
        assert e <= 2e-2, f"{n}: rel err {e:.3e}"


def test_layer_inference_ignores_the_rate(dev):
    import torch
    from sae_vision_amd import layers
    torch.manual_seed(0)
    a = layers.SelfAttentionBlock(num_heads=3, attn_dropout_rate=0.25, dtype=torch.bfloat16, in_ch=192, device=dev)
    b = layers.SelfAttentionBlock(num_heads=3, dtype=torch.bfloat16, in_ch=192, device=dev)
    b.load_state_dict(a.state_dict())
    x = torch.randn(2, 50, 192, device=dev).bfloat16()
    assert torch.equal(a(x, is_training=False), b(x, is_training=False))
    assert torch.equal(a(x, is_training=False), b(x, is_training=True))


def test_talking_heads_dropout_still_refused(dev):
    import torch
    from sae_vision_amd import layers
    m = layers.SelfAttentionBlock(num_heads=3, talking_heads=True, attn_dropout_rate=0.25, dtype=torch.bfloat16,
                                  in_ch=192, device=dev)
    x = torch.randn(2, 50, 192, device=dev).bfloat16()
    with pytest.raises(NotImplementedError, match="talking_heads"):
        m(x, is_training=True)
    m(x, is_training=False)


def test_cvt_block_with_dropout(dev):
    """CvTSelfAttentionBlock: the training call runs the dropout path (it used to raise): it
    repeats bit for bit from the same state and changes with the offset, and rate 0 does neither."""
    import torch
    import sae_vision_amd.ops as ops
    from sae_vision_amd.layers import cvt
    torch.manual_seed(0)
    m = cvt.CvTSelfAttentionBlock(num_heads=3, attn_dropout_rate=0.25, dtype=torch.bfloat16, in_ch=96, device=dev)
    x = torch.randn(2, 14, 14, 96, device=dev).bfloat16()
    outs = []
    for advance in (False, False, True):
        ops.seed_dropout(5)
        if advance:
            ops.dropout_rng(dev).advance()
        outs.append(m(x, is_training=True))
    assert torch.isfinite(outs[0].float()).all()
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
    m.attn_dropout_rate = 0.0
    assert not torch.equal(m(x, is_training=True), outs[0])


# ---------------------------------------------------------------------------- training step
def _data(dev, n):
    import torch
    g = torch.Generator(device=dev).manual_seed(3)
    return [(torch.randn(8, 224, 224, 3, device=dev, generator=g),
             torch.randint(0, 1000, (8,), device=dev, generator=g)) for _ in range(n)]


def test_graph_step_with_dropout_matches_eager(dev):
    """Three steps eager against three replays of the captured step, both from dropout seed 7 (the
    assertions of test_gpu_train_graph.py::test_graph_step_matches_eager); the replays see the
    offset the captured advance kernel bumps: it ends at 3, and the losses differ from those of a
    run whose offset never moves."""
    import torch
    from sae_vision_amd import ops, train, vit
    torch.manual_seed(0)
    m_e = vit.create_model("deit_ti_patch16", 1000, torch.bfloat16, device=dev, attn_dropout_rate=0.1)
    # the ViT head starts at zero (vit.py:97): the first loss would be ln(1000) whatever the mask
    torch.nn.init.normal_(m_e.Dense_0.kernel, std=0.02)
    m_g, m_f = copy.deepcopy(m_e), copy.deepcopy(m_e)
    data = _data(dev, 3)
    rng = ops.dropout_rng(dev)

    ops.seed_dropout(7)
    s_e = train.TrainStep(m_e, global_batch=8, device=dev, flat_grads=False)
    assert s_e._drop_rng is rng
    le = [float(s_e(x, y)) for x, y in data]
    assert int(rng.state[1]) == 3

    ops.seed_dropout(7)
    s_g = train.TrainStep(m_g, global_batch=8, device=dev, graph=True)
    lg = [float(s_g(x, y)) for x, y in data]
    assert s_g._g is not None and int(rng.state[1]) == 3
    for a, b in zip(le, lg):
        assert abs(a - b) <= 1e-3 * abs(a), (le, lg)
    assert s_g._zero_ranges == []
    for (n, pe), pg in zip(m_e.named_parameters(), m_g.parameters()):
        err = float((pe.detach() - pg.detach()).abs().max())
        assert err <= 1e-3 * max(1.0, float(pe.detach().abs().max())), (n, err)

    ops.seed_dropout(7)
    s_f = train.TrainStep(m_f, global_batch=8, device=dev, graph=True)
    s_f._drop_rng = None                                               # the offset is never advanced
    lf = [float(s_f(x, y)) for x, y in data]
    assert int(rng.state[1]) == 0
    for a, b in zip(lg, lf):
        assert a != b, (lg, lf)
    for s in (s_e, s_g, s_f):
        s.close()


def test_rate_zero_step_is_unchanged(dev):
    """A rate-0 model takes the step it always took: no dropout state, no extra launch, and the
    model built through the new keyword steps bit for bit like the one built without it."""
    import torch
    from sae_vision_amd import train, vit
    losses, params = [], []
    for kw in ({}, {"attn_dropout_rate": 0.0}):
        torch.manual_seed(0)
        m = vit.create_model("deit_ti_patch16", 1000, torch.bfloat16, device=dev, **kw)
        s = train.TrainStep(m, global_batch=8, device=dev)
        assert s._drop_rng is None
        losses.append([s(x, y).clone() for x, y in _data(dev, 2)])
        params.append([p.detach().clone() for p in m.parameters()])
        s.close()
    assert all(torch.equal(a, b) for a, b in zip(*losses))
    assert all(torch.equal(a, b) for a, b in zip(*params))
