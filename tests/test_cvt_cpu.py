"""CPU tests of the CvT model and of its convolutional token embedding: the token bookkeeping
(``zero_pad_and_reshape``, per-stage counts), the Flax parameter tree, the model table, the C ABI's new
symbols and host-side refusals, the host predicate, and the gather / scatter index rule (restated in
numpy) against the float64 convolution and its transpose.  No kernel runs here."""
import ctypes
import math
import re
import subprocess

import numpy as np
import pytest
import torch

import _cvt_ref as R

# (B, H, W, Cin, E, k, s): the small shapes of tests/test_gpu_conv_tokens.py
SMALL = [(2, 9, 11, 3, 16, 7, 4), (2, 8, 8, 3, 16, 7, 4), (2, 6, 4, 8, 16, 3, 2), (2, 7, 5, 8, 24, 3, 2),
         (3, 1, 3, 8, 8, 3, 2), (2, 5, 6, 16, 8, 3, 1)]


def _tiny(dtype=torch.float32):
    from sae_vision_amd import cvt
    return cvt.CvT(num_classes=10, stage_sizes=(1, 1, 2), num_heads=(1, 2, 2), embed_dim=(32, 64, 64), dtype=dtype)


def test_zero_pad_and_reshape():
    from sae_vision_amd.cvt import zero_pad_and_reshape
    x = torch.arange(2 * 197 * 3, dtype=torch.float32).reshape(2, 197, 3) + 1
    g = zero_pad_and_reshape(x)
    assert tuple(g.shape) == (2, 15, 15, 3)
    flat = g.reshape(2, 225, 3)
    assert torch.equal(flat[:, :197], x) and torch.equal(flat[:, 197:], torch.zeros(2, 28, 3))
    assert torch.equal(g[:, 0, 0], x[:, 0])                       # the class token at grid position (0, 0)
    y = x[:, :196]
    assert torch.equal(zero_pad_and_reshape(y), y.reshape(2, 14, 14, 3))
    assert torch.equal(R.zero_pad_and_reshape(x.double()), g.double())


def test_parameter_tree():
    import sae_vision_amd.layers as layers
    m = _tiny()
    tree = layers.flax_params(m)
    assert set(tree) == {"Stage_0", "Stage_1", "Stage_2", "Dense_0"}
    assert set(tree["Dense_0"]) == {"kernel", "bias"}
    for i, (size, cin, c, k) in enumerate(((1, 3, 32, 7), (1, 32, 64, 3), (2, 64, 64, 3))):
        st = tree[f"Stage_{i}"]
        assert set(st) == {"ConvTokenEmbedBlock_0"} | {f"StageBlock_{j}" for j in range(size)} | ({"cls"} if i == 2 else set())
        emb = st["ConvTokenEmbedBlock_0"]
        assert set(emb) == {"Conv_0", "LayerNorm_0"} and set(emb["LayerNorm_0"]) == {"scale", "bias"}
        assert tuple(emb["Conv_0"]["kernel"].shape) == (k, k, cin, c) and tuple(emb["Conv_0"]["bias"].shape) == (c,)
        for j in range(size):
            blk = st[f"StageBlock_{j}"]
            assert set(blk) == {"CvTSelfAttentionBlock_0", "LayerNorm_0", "FFBlock_0"}
            assert set(blk["FFBlock_0"]) == {"Dense_0", "Dense_1"}
            att = blk["CvTSelfAttentionBlock_0"]
            assert set(att) == {"ConvProjectionBlock_0", "ConvProjectionBlock_1", "ConvProjectionBlock_2", "DenseGeneral_0"}
            assert set(att["ConvProjectionBlock_1"]) == {"Conv_0", "BatchNorm_0", "Conv_1"}
            assert set(att["ConvProjectionBlock_1"]["BatchNorm_0"]) == {"scale", "bias"}   # mean / var are buffers
    assert tuple(tree["Stage_2"]["cls"].shape) == (1, 1, 64)
    assert float(tree["Dense_0"]["kernel"].abs().max()) == 0.0                             # zero-initialised head
    bufs = [n for n, _ in m.named_buffers()]
    assert len(bufs) == 4 * 3 * 2 and all(n.endswith(("BatchNorm_0.mean", "BatchNorm_0.var")) for n in bufs)
    # a tree goes back in: load_flax_params on a second model gives the same parameters
    m2 = _tiny()
    layers.load_flax_params(m2, {k: v for k, v in tree.items()})
    for (n, p), (_, q) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.equal(p, q), n


def test_configs_and_refusal():
    from sae_vision_amd import cvt
    assert cvt.CVT_CONFIGS == {"cvt-13": ((1, 2, 10), (1, 3, 6), (64, 192, 384)),
                               "cvt-21": ((1, 4, 16), (1, 3, 6), (64, 192, 384)),
                               "cvt-w24": ((2, 2, 20), (3, 12, 16), (192, 768, 1024))}
    with pytest.raises(ValueError, match="368"):    # create_model.py's width: the reference's own assertion refuses it
        cvt.CvT(num_classes=10, stage_sizes=(1, 2, 10), num_heads=(1, 3, 6), embed_dim=(64, 192, 368))
    with pytest.raises(ValueError, match="unknown model"):
        cvt.create_cvt("cvt-14")
    assert cvt.cvt_token_counts(224) == ((3136, 784), (784, 196), (225, 64))
    assert cvt.cvt_token_counts(64) == ((256, 64), (64, 16), (25, 9))
    f13, f21 = cvt.cvt_flops_per_image("cvt-13"), cvt.cvt_flops_per_image("cvt-21")
    assert 8e9 < f13 < 12e9 and f13 < f21          # about 4.5 / 7.1 GMAC in the paper's table


def test_exports():
    import sae_vision_amd
    from sae_vision_amd import _lib as L
    import sae_vision_amd.ops as ops
    from sae_vision_amd import cvt
    names = ("sae_conv_window_cols", "sae_conv_window_gather", "sae_conv_window_scatter")
    lib = sae_vision_amd.load_library()
    assert set(names) <= set(L.EXPORTED_SYMBOLS)
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    assert set(names) <= set(re.findall(r" T (sae_\w+)", nm))
    assert lib.sae_abi_version() == 1
    assert ctypes.sizeof(L.SaeConvtokDesc) == 8 * 4
    assert lib.sae_conv_window_cols(3, 7) == 152 and lib.sae_conv_window_cols(64, 3) == 576
    assert lib.sae_conv_window_cols(3, 8) == 0 and lib.sae_conv_window_cols(0, 3) == 0
    assert ops.conv_window_cols(3, 7) == 152 and ops.conv_window_cols(192, 3) == 1728
    for n in ("conv_tokens", "conv_tokens_ok", "conv_window_matrix", "conv_window_scatter"):
        assert n in ops.__all__ and callable(getattr(ops, n))
    for n in ("zero_pad_and_reshape", "ConvTokenEmbedBlock", "StageBlock", "Stage", "CvT", "create_cvt", "CVT_CONFIGS",
              "cvt_flops_per_image"):
        assert n in cvt.__all__ and hasattr(cvt, n)


def _desc(L, **kw):
    f = dict(batch=2, height=9, width=11, channels=8, kernel=3, stride=2, in_dtype=L.SAE_DTYPE_BF16,
             dtype=L.SAE_DTYPE_BF16)
    f.update(kw)
    return L.SaeConvtokDesc(**f)


def _call(lib, which, d, a=64, b=64):
    """Dummy non-null pointers, never dereferenced: every refusal is host-side."""
    fn = lib.sae_conv_window_gather if which == "gather" else lib.sae_conv_window_scatter
    return fn(None, ctypes.byref(d) if d is not None else None, ctypes.c_void_p(a) if a else None,
              ctypes.c_void_p(b) if b else None)


@pytest.mark.parametrize("which", ["gather", "scatter"])
@pytest.mark.parametrize("kw,code,msg", [
    (dict(kernel=0), "EUNSUPPORTED", "kernel 0 (1..7)"),
    (dict(kernel=8), "EUNSUPPORTED", "kernel 8 (1..7)"),
    (dict(stride=0), "EINVAL", "stride 0 must be >= 1"),
    (dict(batch=0), "EINVAL", "must be >= 1"),
    (dict(channels=-3), "EINVAL", "channels -3"),
    (dict(dtype=7), "EINVAL", "bad dtype 7"),
    (dict(batch=4096, height=1024, width=1024, channels=8), "EUNSUPPORTED", "element offsets exceed 2^31 - 1"),
    (dict(batch=128, height=224, width=224, channels=64, kernel=7, stride=1), "EUNSUPPORTED", "element offsets exceed"),
])
def test_validation_errors(which, kw, code, msg):
    import sae_vision_amd
    from sae_vision_amd import _lib as L
    lib = sae_vision_amd.load_library()
    rc = _call(lib, which, _desc(L, **kw))
    err = lib.sae_last_error().decode()
    assert rc == getattr(L, "SAE_" + code), (rc, err)
    assert msg in err and f"conv_window_{which}" in err


def test_null_and_misaligned_arguments():
    import sae_vision_amd
    from sae_vision_amd import _lib as L
    lib = sae_vision_amd.load_library()
    for which in ("gather", "scatter"):
        assert _call(lib, which, None) == L.SAE_EINVAL and "NULL descriptor" in lib.sae_last_error().decode()
        assert _call(lib, which, _desc(L), a=0) == L.SAE_EINVAL and "NULL" in lib.sae_last_error().decode()
        assert _call(lib, which, _desc(L), b=0) == L.SAE_EINVAL and "NULL" in lib.sae_last_error().decode()
        assert _call(lib, which, _desc(L), a=68) == L.SAE_EINVAL and "16-byte" in lib.sae_last_error().decode()
        assert _call(lib, which, _desc(L), b=68) == L.SAE_EINVAL and "16-byte" in lib.sae_last_error().decode()
    # the gather reads in_dtype; a bf16 x cannot make an fp32 window matrix
    assert _call(lib, "gather", _desc(L, in_dtype=5)) == L.SAE_EINVAL and "bad in_dtype 5" in lib.sae_last_error().decode()
    assert _call(lib, "gather", _desc(L, dtype=L.SAE_DTYPE_F32)) == L.SAE_EUNSUPPORTED
    assert "bf16 x with an fp32" in lib.sae_last_error().decode()


class _Fake:
    def __init__(self, shape, dtype=torch.bfloat16, cuda=True, contiguous=True, ptr=256):
        self.shape, self.dtype, self.is_cuda, self._c, self._p = tuple(shape), dtype, cuda, contiguous, ptr

    def dim(self):
        return len(self.shape)

    def numel(self):
        return math.prod(self.shape)

    def is_contiguous(self):
        return self._c

    def data_ptr(self):
        return self._p


def test_conv_tokens_ok_decisions():
    import sae_vision_amd.ops as ops
    bf, f32 = torch.bfloat16, torch.float32
    ok = ops.conv_tokens_ok
    w = lambda k, c, e: _Fake((k, k, c, e), f32)
    assert ok(_Fake((128, 224, 224, 3), f32), w(7, 3, 64), 7, 4, bf)          # the three cvt-13 stems
    assert ok(_Fake((128, 56, 56, 64), f32), w(3, 64, 192), 3, 2, bf)
    assert ok(_Fake((128, 28, 28, 192), f32), w(3, 192, 384), 3, 2, bf)
    assert ok(_Fake((2, 9, 11, 3), f32), w(7, 3, 16), 7, 4, f32) and ok(_Fake((2, 9, 11, 3)), w(7, 3, 16), 7, 4, bf)
    assert not ok(_Fake((2, 9, 11, 3), cuda=False), w(7, 3, 16), 7, 4, bf)     # a GPU tensor
    assert not ok(_Fake((2, 20, 20, 8)), w(9, 8, 16), 9, 4, bf)                # k <= 7
    assert not ok(_Fake((2, 9, 11, 8)), w(3, 8, 12), 3, 2, bf)                 # E % 8
    assert not ok(_Fake((2, 9, 11, 8)), w(3, 8, 16), 3, 0, bf)                 # stride >= 1
    assert not ok(_Fake((2, 9, 11, 8)), w(3, 8, 16), 3, 2, torch.float16)      # a supported dtype
    assert not ok(_Fake((2, 9, 11, 8), torch.float16), w(3, 8, 16), 3, 2, bf)
    assert not ok(_Fake((2, 9, 11, 8), contiguous=False), w(3, 8, 16), 3, 2, bf)
    assert not ok(_Fake((2, 9, 11, 8), ptr=260), w(3, 8, 16), 3, 2, bf)        # 16-byte aligned
    assert not ok(_Fake((9, 11, 8)), w(3, 8, 16), 3, 2, bf)
    assert not ok(_Fake((2, 9, 11, 8)), w(3, 4, 16), 3, 2, bf)                 # kernel [k, k, Cin, E] of this input
    assert not ok(_Fake((128, 224, 224, 64)), w(7, 64, 64), 7, 1, bf)          # window matrix past 2^31 elements


# ---- the index rule of the kernels, restated: P[m][(ky k + kx) C + c] = x[b][oy s - pt + ky][ox s - pl + kx][c]
def _gather_np(x, k, s):
    B, H, W, C = x.shape
    Ho, Wo = -(-H // s), -(-W // s)
    pt, pl = max((Ho - 1) * s + k - H, 0) // 2, max((Wo - 1) * s + k - W, 0) // 2
    Kp = -(-(k * k * C) // 8) * 8
    P = np.zeros((B * Ho * Wo, Kp))
    for m in range(B * Ho * Wo):
        b, p = divmod(m, Ho * Wo)
        oy, ox = divmod(p, Wo)
        for col in range(k * k * C):
            tap, c = divmod(col, C)
            ky, kx = divmod(tap, k)
            iy, ix = oy * s - pt + ky, ox * s - pl + kx
            if 0 <= iy < H and 0 <= ix < W:
                P[m, col] = x[b, iy, ix, c]
    return P


def _scatter_np(dP, shape, k, s):
    B, H, W, C = shape
    Ho, Wo = -(-H // s), -(-W // s)
    pt, pl = max((Ho - 1) * s + k - H, 0) // 2, max((Wo - 1) * s + k - W, 0) // 2
    dX = np.zeros(shape)
    reads = 0
    for b in range(B):
        for iy in range(H):
            for ix in range(W):
                n = 0
                for ky in range((iy + pt) % s, k, s):
                    oy = (iy + pt - ky) // s
                    if not 0 <= oy < Ho:
                        continue
                    for kx in range((ix + pl) % s, k, s):
                        ox = (ix + pl - kx) // s
                        if not 0 <= ox < Wo:
                            continue
                        dX[b, iy, ix] += dP[(b * Ho + oy) * Wo + ox, (ky * k + kx) * C:(ky * k + kx + 1) * C]
                        n += 1
                reads = max(reads, n)
    return dX, reads


@pytest.mark.parametrize("shape", SMALL)
def test_index_rule_is_the_convolution_and_its_transpose(shape):
    B, H, W, C, E, k, s = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn((B, H, W, C), dtype=torch.float64, generator=g, requires_grad=True)
    w = torch.randn((k, k, C, E), dtype=torch.float64, generator=g)
    bias = torch.randn(E, dtype=torch.float64, generator=g)
    y = R.conv_tokens(x, w, bias, k, s)
    dy = torch.randn(y.shape, dtype=torch.float64, generator=g)
    y.backward(dy)
    K = k * k * C
    P = _gather_np(x.detach().numpy(), k, s)
    assert P.shape == (B * -(-H // s) * -(-W // s), -(-K // 8) * 8) and not P[:, K:].any()
    assert np.array_equal(P[:, :K], R.window_matrix(x.detach(), k, s).numpy())
    assert np.abs(P[:, :K] @ w.reshape(K, E).numpy() + bias.numpy() - y.detach().reshape(-1, E).numpy()).max() <= 1e-12
    dP = np.zeros_like(P)
    dP[:, :K] = dy.reshape(-1, E).numpy() @ w.reshape(K, E).numpy().T
    dX, reads = _scatter_np(dP, (B, H, W, C), k, s)
    assert reads <= math.ceil(k / s) ** 2
    assert np.abs(dX - x.grad.numpy()).max() <= 1e-12 * max(1.0, float(x.grad.abs().max()))
    assert np.abs(dX - R.window_fold(torch.tensor(dP[:, :K]), (B, H, W, C), k, s).numpy()).max() <= 1e-12


@pytest.mark.parametrize("n,k,s,pads", [(9, 7, 4, (3, 3)), (11, 7, 4, (2, 2)), (8, 7, 4, (1, 2)), (6, 3, 2, (0, 1)),
                                        (7, 3, 2, (1, 1)), (1, 3, 2, (1, 1)), (224, 7, 4, (1, 2)), (56, 3, 2, (0, 1))])
def test_same_pads(n, k, s, pads):
    import sae_vision_amd.ops as ops
    assert ops.same_pads(n, k, s) == pads and R.same_pads(n, k, s) == pads
