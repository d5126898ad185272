"""GPU tests of the hidden-state dropout (dropout_rate > 0): the device row mask against the numpy
definition bit for bit, every kernel that applies it (sae_dropout_rows, the add + LayerNorm, tokens
and GELU GEMM forms) against float64 with that mask, the encoder on its fused and unfused paths
against one float64 restatement, and the training step (eager and captured).

Tolerances (north_star, tests/_util.py): fp32 max|a-b|/max|ref| <= 1e-5, bf16 <= 2e-2."""
import copy
import math

import numpy as np
import pytest

import _dropout_ref as DR
import _dropout_rows_ref as RR
from _util import TOL

pytestmark = pytest.mark.gpu

SEED = 1234
SHAPES = [(5, 200), (33, 192), (394, 384), (100, 1024)]   # a partial 16-column block; LayerNorm's 1 / 2 / 4 chunks per lane


def _rng(dev, seed=SEED, offset=0):
    import sae_vision_amd.ops as ops
    r = ops.DropoutRng(seed, dev)
    r.seed(seed, offset)
    return r


def _keep(dev, M, C, rate, sid=0, offset=0, row0=0, row_step=1, seed=SEED):
    """The numpy mask as a float64 device tensor [M, C] of 0 / 1, and pk."""
    import torch
    m = RR.keep_rows(M, C, rate, seed, offset, sid, row0, row_step)
    return torch.tensor(m, device=dev, dtype=torch.float64), DR.threshold(rate)[1]


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


# ---------------------------------------------------------------------------- mask equality
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("rate", [0.1, 0.5])
@pytest.mark.parametrize("offset", [0, 2 ** 32 + 5])
@pytest.mark.parametrize("sid", [0, 7])
def test_mask_equals_definition(dev, shape, rate, offset, sid):
    import sae_vision_amd.ops as ops
    keep = ops.dropout_rows_mask(*shape, rate, _rng(dev, SEED, offset), sid).cpu().numpy()
    assert set(np.unique(keep)) <= {0, 1}
    assert np.array_equal(keep.astype(bool), RR.keep_rows(*shape, rate, SEED, offset, sid))


def test_mask_row0_row_step(dev):
    import sae_vision_amd.ops as ops
    keep = ops.dropout_rows_mask(3, 192, 0.25, _rng(dev), 2, row0=0, row_step=197).cpu().numpy().astype(bool)
    assert np.array_equal(keep, RR.keep_rows(3, 192, 0.25, SEED, 0, 2, 0, 197))
    assert np.array_equal(keep, RR.keep_rows(3 * 197, 192, 0.25, SEED, 0, 2)[::197])
    big = ops.dropout_rows_mask(2, 48, 0.5, _rng(dev), 0, row0=2 ** 33 + 1, row_step=3).cpu().numpy().astype(bool)
    assert np.array_equal(big, RR.keep_rows(2, 48, 0.5, SEED, 0, 0, 2 ** 33 + 1, 3))


# ----------------------------------------------------------------------------- dropout_rows
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("shape", [(33, 200), (7, 10), (2, 17, 192)])
def test_dropout_rows(dev, mode, shape):
    """Forward, backward (the same kernel on the gradient) and in place."""
    import torch
    import sae_vision_amd.ops as ops
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.randn(shape, device=dev, generator=g).to(dt).requires_grad_()
    dy = torch.randn(shape, device=dev, generator=g).to(dt)
    C = shape[-1]
    rng = _rng(dev)
    rng.next_stream()                                   # this call draws stream id 1
    y = ops.dropout_rows(x, (0.25, rng))
    y.backward(dy)
    keep, pk = _keep(dev, x.numel() // C, C, 0.25, sid=1)
    keep = keep.view(shape)
    assert y.dtype == dt and y.shape == x.shape
    assert bool((y[keep == 0] == 0).all()) and bool((x.grad[keep == 0] == 0).all())
    assert rel(y, x.detach().double() * keep / pk) <= TOL[mode]
    assert rel(x.grad, dy.double() * keep / pk) <= TOL[mode]
    z = x.detach().clone().view(-1, C)
    ops._dropout_rows_call(z, z, (0.25, rng.state, 1))   # y may alias x
    assert torch.equal(z.view(shape), y.detach())
    assert ops.dropout_rows(x, None) is x


# ------------------------------------------------------------------- add + LayerNorm forms
def _ln_inputs(dev, M, C, seed=3):
    import torch
    g = torch.Generator(device=dev).manual_seed(seed + M + C)
    x = torch.randn(M, C, device=dev, generator=g) * 3 + 1
    delta = torch.randn(M, C, device=dev, generator=g).to(torch.bfloat16)
    gamma = torch.rand(C, device=dev, generator=g) + 0.5
    beta = torch.randn(C, device=dev, generator=g)
    dxo = torch.randn(M, C, device=dev, generator=g)
    dy = torch.randn(M, C, device=dev, generator=g).to(torch.bfloat16)
    return x, delta, gamma, beta, dxo, dy


def _ln64(xr, gamma, beta):
    mu = xr.mean(-1, keepdim=True)
    var = ((xr - mu) ** 2).mean(-1, keepdim=True)
    return (xr - mu) / (var + 1e-6).sqrt() * gamma + beta


@pytest.mark.parametrize("M,C", SHAPES)
@pytest.mark.parametrize("rate,sid", [(0.1, 0), (0.5, 3)])
def test_add_layer_norm_dropout(dev, M, C, rate, sid):
    import torch
    import sae_vision_amd.ops as ops
    x, delta, gamma, beta, dxo, dy = _ln_inputs(dev, M, C)
    leaves = [t.clone().requires_grad_() for t in (x, delta, gamma, beta)]
    rng = _rng(dev)
    for _ in range(sid):
        rng.next_stream()
    xo, y = ops.add_layer_norm(*leaves, dropout=(rate, rng))
    torch.autograd.backward([xo, y], [dxo, dy])
    keep, pk = _keep(dev, M, C, rate, sid=sid)
    r = [t.clone().double().requires_grad_() for t in (x, delta, gamma, beta)]
    xr = r[0] + r[1] * keep / pk
    yr = _ln64(xr, r[2], r[3])
    torch.autograd.backward([xr, yr], [dxo.double(), dy.double()])
    assert torch.equal(xo[keep == 0], x[keep == 0])                    # bit for bit where dropped
    assert rel(xo, xr) <= TOL["f32"] and rel(y, yr) <= TOL["bf16"]
    assert bool((leaves[1].grad[keep == 0] == 0).all())
    assert rel(leaves[0].grad, r[0].grad) <= TOL["f32"]
    assert rel(leaves[1].grad, r[1].grad) <= TOL["bf16"]
    assert rel(leaves[2].grad, r[2].grad) <= TOL["f32"]
    assert rel(leaves[3].grad, r[3].grad) <= TOL["f32"]


@pytest.mark.parametrize("M,C", SHAPES)
def test_add_layer_norm_dropout_rescales_once(dev, M, C):
    """x = 0, delta = 1: xout is keep / pk itself (a rescale applied twice or never shows as a factor)."""
    import torch
    import sae_vision_amd.ops as ops
    rate = 0.25
    xo, _ = ops.add_layer_norm(torch.zeros(M, C, device=dev), torch.ones(M, C, device=dev, dtype=torch.bfloat16),
                               torch.ones(C, device=dev), torch.zeros(C, device=dev), dropout=(rate, _rng(dev)))
    keep, pk = _keep(dev, M, C, rate)
    inv = float(np.float32(256.0) / np.float32(256 - DR.threshold(rate)[0]))   # 1 / pk as the kernels hold it
    assert torch.equal(xo, keep.float() * inv)
    assert rel(xo, keep / pk) <= 1e-7


def test_cls_add_layer_norm_dropout_equals_class_rows(dev):
    """The class-token form draws rows b * N of the full tensor's mask (row_step = N)."""
    import torch
    import sae_vision_amd.ops as ops
    B, N, C, rate = 3, 17, 192, 0.25
    x, delta, gamma, beta, _, dy = _ln_inputs(dev, B * N, C)
    x, delta = x.view(B, N, C), delta.view(B, N, C)
    dyc = dy.view(B, N, C)[:, 0].contiguous()
    a = [t.clone().requires_grad_() for t in (x, delta, gamma, beta)]
    b = [t.clone().requires_grad_() for t in (x, delta, gamma, beta)]
    yc = ops.cls_add_layer_norm(*a, dropout=(rate, _rng(dev)))
    yc.backward(dyc)
    xo, y = ops.add_layer_norm(*b, dropout=(rate, _rng(dev)))
    dyf = torch.zeros_like(y)
    dyf[:, 0] = dyc
    torch.autograd.backward([xo, y], [torch.zeros_like(xo), dyf])
    assert yc.shape == (B, C) and torch.equal(yc, y[:, 0])
    assert torch.equal(a[0].grad[:, 0], b[0].grad[:, 0]) and torch.equal(a[1].grad[:, 0], b[1].grad[:, 0])
    assert not bool(a[0].grad[:, 1:].any()) and not bool(a[1].grad[:, 1:].any())
    keep, _ = _keep(dev, B, C, rate, row_step=N)
    assert bool((a[1].grad[:, 0][keep == 0] == 0).all()) and bool((a[1].grad[:, 0][keep == 1] != 0).any())
    assert rel(a[2].grad, b[2].grad) <= TOL["f32"] and rel(a[3].grad, b[3].grad) <= TOL["f32"]


# ---------------------------------------------------------------------------------- tokens
@pytest.mark.parametrize("B,Lt,E", [(3, 16, 192), (2, 4, 200)])
def test_encoder_tokens_dropout(dev, B, Lt, E):
    import torch
    import sae_vision_amd.ops as ops
    rate = 0.25
    g = torch.Generator(device=dev).manual_seed(11)
    tok = torch.randn(B, Lt, E, device=dev, generator=g).to(torch.bfloat16)
    cls = torch.randn(1, 1, E, device=dev, generator=g)
    pos = torch.randn(1, Lt + 1, E, device=dev, generator=g)
    dx = torch.randn(B, Lt + 1, E, device=dev, generator=g)
    a = [t.clone().requires_grad_() for t in (tok, cls, pos)]
    x = ops.encoder_tokens(*a, dropout=(rate, _rng(dev)))
    x.backward(dx)
    keep, pk = _keep(dev, B * (Lt + 1), E, rate)
    keep = keep.view(B, Lt + 1, E)
    r = [t.clone().double().requires_grad_() for t in (tok, cls, pos)]
    xr = (torch.cat([r[1].expand(B, 1, E), r[0]], dim=1) + r[2]) * keep / pk
    xr.backward(dx.double())
    assert bool((x[keep == 0] == 0).all())
    assert rel(x, xr) <= TOL["f32"]
    assert bool((a[0].grad[keep[:, 1:] == 0] == 0).all())
    assert rel(a[0].grad, r[0].grad) <= TOL["bf16"]
    assert rel(a[2].grad, r[2].grad) <= TOL["f32"] and rel(a[1].grad, r[1].grad) <= TOL["f32"]
    assert torch.equal(a[1].grad.view(-1), a[2].grad[0, 0])            # dcls == dpos[0]


# -------------------------------------------------------------------------------- GELU GEMM
ROUTE_TILE128, ROUTE_KTAIL, ROUTE_GEMM8, ROUTE_GEMM8X = 1, 2, 3, 4
GEMMS = [
    # M, N, K, routes                                   what it covers
    (300, 136, 64, (ROUTE_TILE128,)),                 # the 128-row kernel, N % 16 == 8 (half a Philox block last)
    (300, 136, 72, (ROUTE_KTAIL,)),                   # the K tail instance
    (4100, 1536, 384, (ROUTE_GEMM8, ROUTE_GEMM8X)),   # DeiT-S FF Dense_0: an LDS-DMA route
    (4100, 3072, 768, (ROUTE_GEMM8, ROUTE_GEMM8X)),   # ViT-B FF Dense_0: an LDS-DMA route
    (4100, 1024, 768, (ROUTE_GEMM8X,)),               # the ping-pong kernel (N % 256 == 0, N % 192 != 0)
]


def _gelu64(h):
    import torch
    u = math.sqrt(2.0 / math.pi) * (h + 0.044715 * h ** 3)
    t = torch.tanh(u)
    gelu = 0.5 * h * (1 + t)
    dgelu = 0.5 * (1 + t) + 0.5 * h * (1 - t * t) * math.sqrt(2.0 / math.pi) * (1 + 3 * 0.044715 * h * h)
    return gelu, dgelu


@pytest.mark.parametrize("M,N,K,routes", GEMMS)
def test_gelu_gemm_dropout(dev, M, N, K, routes):
    import torch
    import sae_vision_amd
    import sae_vision_amd.ops as ops
    lib = sae_vision_amd.load_library()
    assert lib.sae_gemm_nt_route(M, N, K, ops.EPI_GELU_GRAD) in routes
    rate, sid = 0.25, 5
    g = torch.Generator(device=dev).manual_seed(13)
    a = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
    bt = (torch.randn(N, K, device=dev, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    bias = torch.randn(N, device=dev, generator=g) * 0.1
    rng = _rng(dev)
    c, c2 = ops.gemm_nt(a, bt, bias, ops.EPI_GELU_GRAD, drop=(rate, rng.state, sid))
    keep, pk = _keep(dev, M, N, rate, sid=sid)
    assert bool((c[keep == 0] == 0).all()) and bool((c2[keep == 0] == 0).all())
    assert float((c2[keep == 1] != 0).double().mean()) > 0.99          # the mask, not a zero output
    h = (a.double() @ bt.double().t() + bias.double()).to(torch.bfloat16).double()
    gelu, dgelu = _gelu64(h)
    assert rel(c, gelu * keep / pk) <= TOL["bf16"]
    assert rel(c2, dgelu * keep / pk) <= TOL["bf16"]


@pytest.mark.parametrize("M,I,Hd", [(300, 64, 136), (4100, 384, 1536)])
def test_ff_block_dropout(dev, M, I, Hd):
    """Forward and all five gradients of the FF block with the hidden dropout against float64."""
    import torch
    import sae_vision_amd.ops as ops
    rate = 0.25
    g = torch.Generator(device=dev).manual_seed(17)
    x = torch.randn(M, I, device=dev, generator=g).to(torch.bfloat16)
    w0 = torch.randn(I, Hd, device=dev, generator=g) / math.sqrt(I)
    b0 = torch.randn(Hd, device=dev, generator=g) * 0.1
    w1 = torch.randn(Hd, I, device=dev, generator=g) / math.sqrt(Hd)
    b1 = torch.randn(I, device=dev, generator=g) * 0.1
    dy = torch.randn(M, I, device=dev, generator=g).to(torch.bfloat16)
    a = [t.clone().requires_grad_() for t in (x, w0, b0, w1, b1)]
    try:
        y = ops.ff_block(*a, dropout=(rate, _rng(dev)))
        y.backward(dy)
    finally:
        ops.clear_weight_cache()
    keep, pk = _keep(dev, M, Hd, rate)
    r = [t.clone().double().requires_grad_() for t in (x, w0, b0, w1, b1)]
    q = lambda w: w.detach().to(torch.bfloat16).double() + (w - w.detach())   # bf16 value, identity gradient
    h = r[0] @ q(r[1]) + r[2]
    yr = (torch.nn.functional.gelu(h, approximate="tanh") * keep / pk) @ q(r[3]) + r[4]
    yr.backward(dy.double())
    assert rel(y, yr) <= TOL["bf16"]
    for got, want, name in zip(a, r, ("x", "w0", "b0", "w1", "b1")):
        assert rel(got.grad, want.grad) <= TOL["bf16"], name


# --------------------------------------------------------------- rate 0, rates below 1 / 512
@pytest.mark.parametrize("rate", [0.0, 0.0019])
def test_rate_zero_is_the_plain_op(dev, rate):
    """T = 0: every new op is bit-identical to the plain one, forward and backward."""
    import torch
    import sae_vision_amd.ops as ops
    assert DR.threshold(rate)[0] == 0
    B, N, C = 3, 17, 192
    x, delta, gamma, beta, dxo, dy = _ln_inputs(dev, B * N, C)
    g = torch.Generator(device=dev).manual_seed(19)
    tok = torch.randn(B, N - 1, C, device=dev, generator=g).to(torch.bfloat16)
    cls, pos = torch.randn(1, 1, C, device=dev, generator=g), torch.randn(1, N, C, device=dev, generator=g)
    w0, b0 = torch.randn(C, 4 * C, device=dev, generator=g) / 14, torch.randn(4 * C, device=dev, generator=g)
    w1, b1 = torch.randn(4 * C, C, device=dev, generator=g) / 28, torch.randn(C, device=dev, generator=g)

    def run(drop):
        kw = {} if drop is None else {"dropout": drop}
        outs = []
        lv = [t.clone().requires_grad_() for t in (x, delta, gamma, beta)]
        xo, y = ops.add_layer_norm(*lv, **kw)
        torch.autograd.backward([xo, y], [dxo, dy])
        outs += [xo, y] + [t.grad for t in lv]
        lv = [t.clone().view(B, N, C).requires_grad_() if t.dim() == 2 else t.clone().requires_grad_()
              for t in (x, delta, gamma, beta)]
        yc = ops.cls_add_layer_norm(*lv, **kw)
        yc.backward(dy.view(B, N, C)[:, 0].contiguous())
        outs += [yc] + [t.grad for t in lv]
        lv = [t.clone().requires_grad_() for t in (tok, cls, pos)]
        xt = ops.encoder_tokens(*lv, **kw)
        xt.backward(dxo.view(B, N, C))
        outs += [xt] + [t.grad for t in lv]
        lv = [t.clone().requires_grad_() for t in (delta, w0, b0, w1, b1)]
        try:
            yf = ops.ff_block(*lv, **kw)
            yf.backward(dy)
        finally:
            ops.clear_weight_cache()
        outs += [yf] + [t.grad for t in lv]
        outs.append(ops.dropout_rows(x, drop))
        outs.append(ops.dropout_rows(delta, drop))
        return outs

    rng = _rng(dev)
    for p, d in zip(run(None), run((rate, rng))):
        assert torch.equal(p, d)


# ------------------------------------------------------------- the state decides the mask
def test_same_state_same_mask_advanced_state_another(dev):
    import torch
    import sae_vision_amd.ops as ops
    M, C, rate = 33, 192, 0.25
    zeros, ones = torch.zeros(M, C, device=dev), torch.ones(M, C, device=dev, dtype=torch.bfloat16)
    gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    rng = _rng(dev, SEED, 9)
    outs = []
    for advance in (False, False, True):
        rng.seed(SEED, 9)
        if advance:
            rng.advance()
        outs.append(ops.add_layer_norm(zeros, ones, gamma, beta, dropout=(rate, rng))[0])
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
    assert int(rng.state[1]) == 10
    for out, off in ((outs[0], 9), (outs[2], 10)):
        keep, _ = _keep(dev, M, C, rate, offset=off)
        assert torch.equal(out != 0, keep != 0)


# --------------------------------------------------------------------------------- encoder
def _encoder64(enc, inputs, rate, attn_rate, quant, dev, seed):
    """models/vit.py:35-58 in float64 with the numpy masks of stream ids 0, 1, 2, ... in the order
    of the training forward: the input, then per block (the attention probabilities,) the attention
    output, the FF hidden activation, the FF output.  ``quant``: Dense kernels at their bf16 values
    (identity gradient), as the bf16 model reads them.  Returns the output and {parameter: grad fn}."""
    import torch
    B, N, C = inputs.shape
    P = {n: p.detach().double().requires_grad_() for n, p in enc.named_parameters()}
    qz = (lambda w: w.detach().to(torch.bfloat16).double() + (w - w.detach())) if quant else (lambda w: w)
    sid = [0]
    _, pk = DR.threshold(rate)

    def mask(C_):
        m = torch.tensor(RR.keep_rows(B * N, C_, rate, seed, 0, sid[0]), device=dev, dtype=torch.float64) / pk
        sid[0] += 1
        return m.view(B, N, C_)

    def ln(x, pre):
        mu = x.mean(-1, keepdim=True)
        var = ((x - mu) ** 2).mean(-1, keepdim=True)
        return (x - mu) / (var + 1e-6).sqrt() * P[pre + ".scale"] + P[pre + ".bias"]

    x = (inputs.double() + P["AddAbsPosEmbed_0.pos_embed"]) * mask(C)
    for i in range(enc.num_layers):
        pre = f"EncoderBlock_{i}."
        att = pre + "SelfAttentionBlock_0."
        H = getattr(enc, f"EncoderBlock_{i}").SelfAttentionBlock_0.num_heads
        h = ln(x, pre + "LayerNorm_0")
        q, k, v = (torch.einsum("bnc,chd->bnhd", h, qz(P[att + w + ".kernel"])) for w in ("queries", "keys", "values"))
        p = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", q, k) / math.sqrt(q.shape[-1]), dim=-1)
        if attn_rate > 0:
            am = DR.keep_mask(B, H, N, N, attn_rate, seed, 0, sid[0]) / DR.threshold(attn_rate)[1]
            sid[0] += 1
            p = p * torch.tensor(am, device=dev, dtype=torch.float64)
        o = torch.einsum("bhqk,bkhd->bqhd", p, v)
        a = torch.einsum("bnhd,hdc->bnc", o, qz(P[att + "DenseGeneral_0.kernel"]))
        x = x + a * mask(C)
        h = ln(x, pre + "LayerNorm_1")
        ff = pre + "FFBlock_0."
        hid = torch.nn.functional.gelu(h @ qz(P[ff + "Dense_0.kernel"]) + P[ff + "Dense_0.bias"], approximate="tanh")
        hid = hid * mask(hid.shape[-1])
        f = hid @ qz(P[ff + "Dense_1.kernel"]) + P[ff + "Dense_1.bias"]
        x = x + f * mask(C)
    return ln(x, "LayerNorm_0"), P


def _encoder_case(dev, dtype, rate, attn_rate, cls_only=False):
    import torch
    from sae_vision_amd import ops, vit
    B, N, C, H = 2, 17, 192, 3
    torch.manual_seed(0)
    enc = vit.Encoder(N, C, 2, H, 4, dtype, dev, attn_rate, rate)
    with torch.no_grad():   # biases and LayerNorm parameters off their trivial initial values
        for n, p in enc.named_parameters():
            if n.endswith("bias"):
                p.normal_(0, 0.1)
            elif n.endswith("scale"):
                p.uniform_(0.5, 1.5)
    g = torch.Generator(device=dev).manual_seed(23)
    inputs = torch.randn(B, N, C, device=dev, generator=g)
    dout = torch.randn(B, N, C, device=dev, generator=g).to(dtype)
    ops.seed_dropout(SEED)
    out = enc(inputs, True, cls_only=cls_only)
    ref, P = _encoder64(enc, inputs, rate, attn_rate, dtype == torch.bfloat16, dev, SEED)
    if cls_only:
        ref, dout = ref[:, 0], dout[:, 0].contiguous()
    out.backward(dout)
    ref.backward(dout.double())
    tol = TOL["bf16" if dtype == torch.bfloat16 else "f32"]
    assert out.dtype == dtype and rel(out, ref) <= tol, rel(out, ref)
    errs = {n: rel(p.grad, P[n].grad) for n, p in enc.named_parameters()}
    assert max(errs.values()) <= tol, sorted(errs.items(), key=lambda kv: -kv[1])[:4]
    return ops.dropout_rng(dev)._calls


def test_encoder_fused_bf16(dev):
    import torch
    assert _encoder_case(dev, torch.bfloat16, 0.25, 0.0) == 7            # 1 + 2 blocks x 3 sites


def test_encoder_fused_bf16_cls_only(dev):
    import torch
    assert _encoder_case(dev, torch.bfloat16, 0.25, 0.0, cls_only=True) == 7


def test_encoder_unfused_f32(dev):
    """The same seed gives the unfused path the same masks: same ids, same order, each applied once."""
    import torch
    assert _encoder_case(dev, torch.float32, 0.25, 0.0) == 7


def test_encoder_both_rates(dev):
    import torch
    assert _encoder_case(dev, torch.bfloat16, 0.25, 0.1) == 9


def test_inference_draws_nothing(dev):
    """is_training=False: no stream id is drawn and the output is the rate-0 model's, bit for bit."""
    import torch
    from sae_vision_amd import ops, vit
    outs = []
    for rate in (0.25, 0.0):
        torch.manual_seed(0)
        m = vit.ViT(10, 2, 3, 192, (16, 16), 64, 4, torch.bfloat16, dev, 0.0, rate)
        torch.nn.init.normal_(m.Dense_0.kernel, std=0.02)
        x = torch.randn(2, 64, 64, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        ops.seed_dropout(SEED)
        with torch.no_grad():
            outs.append(m(x, False))
        assert ops.dropout_rng(dev)._calls == 0
    assert torch.equal(*outs)
    with torch.no_grad():   # the whole model, training: input + 2 x 3 sites
        y = vit.ViT(10, 2, 3, 192, (16, 16), 64, 4, torch.bfloat16, dev, 0.0, 0.25)(x, True)
    assert ops.dropout_rng(dev)._calls == 7 and bool(torch.isfinite(y.float()).all())


# ---------------------------------------------------------------------------- training step
def _data(dev, n):
    import torch
    g = torch.Generator(device=dev).manual_seed(3)
    return [(torch.randn(8, 224, 224, 3, device=dev, generator=g),
             torch.randint(0, 1000, (8,), device=dev, generator=g)) for _ in range(n)]


def test_graph_step_with_hidden_dropout_matches_eager(dev):
    """The assertions of test_gpu_dropout.py::test_graph_step_with_dropout_matches_eager for
    dropout_rate = 0.1: eager and captured agree over three steps, the offset ends at 3, and the
    losses differ from those of a run whose offset never moves."""
    import torch
    from sae_vision_amd import ops, train, vit
    torch.manual_seed(0)
    m_e = vit.create_model("deit_ti_patch16", 1000, torch.bfloat16, device=dev, dropout_rate=0.1)
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
    """A model built with dropout_rate=0.0 steps bit for bit like one built without the keyword,
    and takes no dropout state."""
    import torch
    from sae_vision_amd import train, vit
    losses, params = [], []
    for kw in ({}, {"dropout_rate": 0.0}):
        torch.manual_seed(0)
        m = vit.create_model("deit_ti_patch16", 1000, torch.bfloat16, device=dev, **kw)
        s = train.TrainStep(m, global_batch=8, device=dev)
        assert s._drop_rng is None
        losses.append([s(x, y).clone() for x, y in _data(dev, 2)])
        params.append([p.detach().clone() for p in m.parameters()])
        s.close()
    assert all(torch.equal(a, b) for a, b in zip(*losses))
    assert all(torch.equal(a, b) for a, b in zip(*params))
