"""CPU tests of the LeFF feed-forward: the float64 restatement of BatchNorm + GELU over token rows
(tests/_leff_ref.py) against autograd, the running-statistics recurrence, the host predicate of
ops.bn_gelu, and LeFFBlock's parameter tree, buffers, inits and width rules (no GPU, no kernel)."""
import types

import numpy as np
import pytest
import torch

import _leff_ref as R

EPS = 1e-5


def _rows(seed, N, C):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, dtype=torch.float64, generator=g) * 1.5 + 0.3
    gamma = 1 + 0.5 * torch.randn(C, dtype=torch.float64, generator=g)
    beta = 0.5 * torch.randn(C, dtype=torch.float64, generator=g)
    dy = torch.randn(N, C, dtype=torch.float64, generator=g)
    return x, gamma, beta, dy


@pytest.mark.parametrize("N,C", [(1, 8), (7, 4), (50, 24)])
def test_hand_backward_is_autograd(N, C):
    x, gamma, beta, dy = _rows(N + C, N, C)
    fw = R.bn_gelu_forward(x, gamma, beta, EPS)
    bw = R.bn_gelu_backward(gamma, fw, dy)
    xa, ga, ba = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    mu, var = xa.mean(0), xa.var(0, unbiased=False)
    z = (xa - mu) / torch.sqrt(var + EPS) * ga + ba
    y = torch.nn.functional.gelu(z, approximate="tanh")
    assert (y - fw["y"]).abs().max() <= 1e-12
    y.backward(dy)
    for name, t in (("dx", xa), ("dgamma", ga), ("dbeta", ba)):
        err = (t.grad - bw[name]).abs().max() / max(1.0, t.grad.abs().max())
        assert err <= 1e-10, (name, float(err))


def test_zero_variance_stays_finite():
    """One participating row: var = 0, rstd = rsqrt(eps), z = beta and dx = 0."""
    x, gamma, beta, dy = _rows(3, 1, 8)
    fw = R.bn_gelu_forward(x, gamma, beta, EPS)
    assert torch.equal(fw["var"], torch.zeros(8, dtype=torch.float64))
    assert torch.allclose(fw["z"], beta) and torch.isfinite(fw["y"]).all()
    assert R.bn_gelu_backward(gamma, fw, dy)["dx"].abs().max() == 0


def test_bf16_mode_rounds_z_and_y():
    x, gamma, beta, _ = _rows(5, 20, 8)
    fw = R.bn_gelu_forward(x, gamma, beta, EPS, "bf16")
    for k in ("z", "y"):
        assert torch.equal(fw[k], fw[k].to(torch.bfloat16).to(torch.float64)), k
    exact = R.bn_gelu_forward(x, gamma, beta, EPS)
    assert 0 < (fw["y"] - exact["y"]).abs().max() <= 2 ** -7 * exact["y"].abs().max()


def test_running_recurrence_and_evaluation():
    x, gamma, beta, _ = _rows(9, 30, 4)
    fw = R.bn_gelu_forward(x, gamma, beta, EPS)
    mean, var = torch.zeros(4, dtype=torch.float64), torch.ones(4, dtype=torch.float64)
    for _ in range(2):
        mean, var = R.running(mean, var, fw["mu"], fw["var"], 0.9)
    assert torch.allclose(mean, 0.19 * fw["mu"]) and torch.allclose(var, 0.81 + 0.19 * fw["var"])
    ev = R.bn_gelu_forward(x, gamma, beta, EPS, stats=(mean, var))
    z = (x - mean) / torch.sqrt(var + EPS) * gamma + beta
    assert torch.allclose(ev["y"], torch.nn.functional.gelu(z, approximate="tanh"), rtol=0, atol=1e-12)


def test_block_reference_matches_its_parts():
    """leff_block: the class token passes through, and the three BatchNorms see N = B * L rows."""
    g = torch.Generator().manual_seed(1)
    B, L, C, hid, k = 2, 9, 4, 8, 3
    shapes = {"Dense_0.kernel": (C, hid), "Dense_0.bias": (hid,), "Conv_0.kernel": (k, k, hid, hid),
              "Conv_0.bias": (hid,), "Dense_1.kernel": (hid, C), "Dense_1.bias": (C,),
              "BatchNorm_0.scale": (hid,), "BatchNorm_0.bias": (hid,), "BatchNorm_1.scale": (hid,),
              "BatchNorm_1.bias": (hid,), "BatchNorm_2.scale": (C,), "BatchNorm_2.bias": (C,)}
    assert set(shapes) == set(R.PARAMS)
    p = {n: 0.4 * torch.randn(s, dtype=torch.float64, generator=g) for n, s in shapes.items()}
    x = torch.randn(B, 1 + L, C, dtype=torch.float64, generator=g)
    y, batch, bn_in = R.leff_block(x, p, k, EPS)
    assert y.shape == x.shape and torch.equal(y[:, 0], x[:, 0])
    assert [tuple(t.shape) for t in bn_in] == [(B, L, hid), (B, L, hid), (B, L, C)]
    fw = R.bn_gelu_forward(bn_in[2].reshape(-1, C), p["BatchNorm_2.scale"], p["BatchNorm_2.bias"], EPS)
    assert torch.allclose(y[:, 1:].reshape(-1, C), fw["y"], rtol=0, atol=1e-12)
    assert torch.allclose(batch[2][0], fw["mu"]) and torch.allclose(batch[2][1], fw["var"])


def test_bn_gelu_ok_envelope():
    import sae_vision_amd.ops as ops
    bf, f32 = torch.bfloat16, torch.float32
    fake = lambda *shape, cuda=True: types.SimpleNamespace(is_cuda=cuda, shape=shape, requires_grad=False)
    assert ops.bn_gelu_ok(fake(2, 9, 8), bf) and ops.bn_gelu_ok(fake(2, 9, 12), f32)
    assert ops.bn_gelu_ok(fake(1, 2, 8), bf, x_lead=1)
    assert not ops.bn_gelu_ok(torch.zeros(2, 9, 8), f32)                 # a CPU tensor
    assert not ops.bn_gelu_ok(fake(2, 9, 8, cuda=False), f32)
    assert not ops.bn_gelu_ok(fake(2, 9, 12), bf)                        # C % 8 in bf16
    assert not ops.bn_gelu_ok(fake(2, 9, 6), f32)                        # C % 4 in fp32
    assert not ops.bn_gelu_ok(fake(18, 8), f32)                          # not [B, L, C]
    assert not ops.bn_gelu_ok(fake(2, 3, 3, 8), f32)
    assert not ops.bn_gelu_ok(fake(2, 9, 8), torch.float16)
    assert not ops.bn_gelu_ok(fake(2, 9, 8), torch.float64)
    assert not ops.bn_gelu_ok(fake(0, 9, 8), f32) and not ops.bn_gelu_ok(fake(2, 0, 8), f32)
    assert not ops.bn_gelu_ok(fake(2, 1, 8), f32, x_lead=1)              # no participating row left
    assert not ops.bn_gelu_ok(fake(2, 9, 8), f32, x_lead=2)
    assert ops.bn_gelu_ok(fake(1, 2 ** 28 - 2, 8), f32)                  # B (L + 1) C = 2^31 - 8
    assert not ops.bn_gelu_ok(fake(1, 2 ** 28 - 1, 8), f32)              # B (L + 1) C = 2^31
    assert ops.bn_gelu_ok(fake(1, 2 ** 28 - 1, 8), f32, x_lead=1)        # L = 2^28 - 2 of those rows take part
    assert not ops.bn_gelu_ok(fake(1, 2 ** 28, 8), f32, x_lead=1)
    # the evaluation form has no backward
    assert ops.bn_gelu_ok(fake(2, 9, 8), f32, training=False, needs_grad=False)
    assert not ops.bn_gelu_ok(fake(2, 9, 8), f32, training=False, needs_grad=True)
    assert ops.bn_gelu_ok(fake(2, 9, 8), f32, training=True, needs_grad=True)


def test_bn_gelu_refuses_cpu_tensors():
    import sae_vision_amd.ops as ops
    x, c = torch.zeros(2, 9, 8), torch.zeros(8)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.bn_gelu(x, c, c, c.clone(), c.clone(), 0.9, EPS, True, torch.float32)


def test_capi_refusals():
    """sae_bn_gelu_*: the envelope is checked on the host, before any HIP call."""
    import ctypes
    from sae_vision_amd import _lib as L
    lib = L.load()
    assert ctypes.sizeof(L.SaeBnrowsDesc) == 9 * 4
    assert lib.sae_bn_gelu_workspace_bytes(2, 9, 8) > 0 and lib.sae_bn_gelu_workspace_bytes(2, 9, 12) > 0
    for bad in ((0, 9, 8), (2, 0, 8), (2, 9, 6), (1, 2 ** 28 - 1, 8)):
        assert lib.sae_bn_gelu_workspace_bytes(*bad) == 0, bad
    p, odd = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 8)
    desc = lambda **kw: L.SaeBnrowsDesc(**{**dict(batch=2, tokens=9, channels=8, x_lead=0, y_lead=0, dtype=L.SAE_DTYPE_BF16,
                                                  training=1, momentum=0.9, eps=EPS), **kw})

    def fwd(d, x=p, lead=None, pitch=0):
        return lib.sae_bn_gelu_fwd(None, ctypes.byref(d), x, p, p, p, p, lead, pitch, p, p, p, p)

    # every refusal below returns before any HIP call (the pointers are made up)
    for kw, args, want, msg in [(dict(channels=12), {}, L.SAE_EUNSUPPORTED, "multiple of 8"),
                                (dict(channels=6, dtype=L.SAE_DTYPE_F32), {}, L.SAE_EUNSUPPORTED, "multiple of 4"),
                                (dict(tokens=0), {}, L.SAE_EUNSUPPORTED, ">= 1"),
                                (dict(x_lead=2), {}, L.SAE_EINVAL, "0 or 1"),
                                (dict(batch=1, tokens=2 ** 28 - 1), {}, L.SAE_EUNSUPPORTED, "2^31"),
                                (dict(), dict(x=odd), L.SAE_EUNSUPPORTED, "16-byte"),
                                (dict(y_lead=1), {}, L.SAE_EINVAL, "needs lead"),
                                (dict(y_lead=1), dict(lead=p, pitch=12), L.SAE_EUNSUPPORTED, "lead_pitch")]:
        rc = fwd(desc(**kw), **args)
        assert rc == want and msg in lib.sae_last_error().decode(), (kw, rc, lib.sae_last_error())
    d = desc(training=0)
    rc = lib.sae_bn_gelu_bwd(None, ctypes.byref(d), p, p, p, p, p, p, p, p, p, p)
    assert rc == L.SAE_EUNSUPPORTED and "no backward" in lib.sae_last_error().decode()


# ------------------------------------------------------------------------------ LeFFBlock
TREE = {"Dense_0": {"kernel", "bias"}, "BatchNorm_0": {"scale", "bias"}, "Conv_0": {"kernel", "bias"},
        "BatchNorm_1": {"scale", "bias"}, "Dense_1": {"kernel", "bias"}, "BatchNorm_2": {"scale", "bias"}}


def test_leff_block_parameters_and_buffers():
    import sae_vision_amd.layers as layers
    torch.manual_seed(0)
    blk = layers.LeFFBlock(expand_ratio=4, in_ch=48)
    tree = layers.flax_params(blk)
    assert {k: set(v) for k, v in tree.items()} == TREE
    shapes = {n: tuple(p.shape) for n, p in blk.named_parameters()}
    assert shapes["Dense_0.kernel"] == (48, 192) and shapes["Dense_0.bias"] == (192,)
    assert shapes["Conv_0.kernel"] == (5, 5, 192, 192) and shapes["Conv_0.bias"] == (192,)   # kernel_size = 5
    assert shapes["Dense_1.kernel"] == (192, 48) and shapes["Dense_1.bias"] == (48,)
    assert shapes["BatchNorm_0.scale"] == shapes["BatchNorm_1.bias"] == (192,) and shapes["BatchNorm_2.scale"] == (48,)
    assert all(p.dtype == torch.float32 for p in blk.parameters())
    bufs = dict(blk.named_buffers())
    assert sorted(bufs) == sorted(f"BatchNorm_{i}.{s}" for i in range(3) for s in ("mean", "var"))
    for n, b in bufs.items():
        assert b.dtype == torch.float32 and b.is_contiguous()
        assert torch.equal(b, torch.zeros_like(b) if n.endswith("mean") else torch.ones_like(b)), n
    # inits: zero biases, unit scales, lecun_normal kernels (std = 1 / sqrt(fan_in), truncated at 2 sigma)
    for n, p in blk.named_parameters():
        if n.endswith(".bias"):
            assert torch.count_nonzero(p) == 0, n
        elif n.endswith(".scale"):
            assert torch.equal(p, torch.ones_like(p)), n
    for n, fan_in in (("Dense_0", 48), ("Conv_0", 25 * 192), ("Dense_1", 192)):
        w = tree[n]["kernel"]
        assert abs(float(w.std()) * np.sqrt(fan_in) - 1) < 0.05, (n, float(w.std()))
        assert float(w.abs().max()) <= 2 / 0.87962566103423978 / np.sqrt(fan_in) + 1e-6
    layers.load_flax_params(blk, {k: {n: torch.zeros_like(t) for n, t in v.items()} for k, v in tree.items()})
    assert all(torch.count_nonzero(p) == 0 for p in blk.parameters())


def test_leff_block_width_rules():
    import sae_vision_amd.layers as layers
    hidden = lambda **kw: layers.LeFFBlock(in_ch=10, **kw).Dense_0.kernel.shape[1]
    assert hidden(expand_ratio=4) == 40
    assert hidden(expand_ratio=0.25) == 2                    # int(2.5)
    assert hidden(expand_ratio=0.01) == 1                    # max(1, int(0.1))
    assert hidden(hidden_ch=24) == 24
    assert hidden(expand_ratio=2, hidden_ch=24) == 20        # expand_ratio wins, as in the reference
    assert layers.LeFFBlock(hidden_ch=8, kernel_size=3, in_ch=10).Conv_0.kernel.shape == (3, 3, 8, 8)
    with pytest.raises(ValueError, match="expand_ratio or hidden_ch"):
        layers.LeFFBlock()
    lazy = layers.LeFFBlock(expand_ratio=4)                  # built at the first call, like the Flax module
    assert not list(lazy.parameters())


@pytest.mark.parametrize("tokens", [1, 1 + 8, 1 + 15])
def test_leff_block_needs_a_square_grid(tokens):
    import sae_vision_amd.layers as layers
    blk = layers.LeFFBlock(expand_ratio=2, in_ch=8)
    with pytest.raises(ValueError, match="square"):
        blk(torch.zeros(2, tokens, 8), is_training=True)
