"""Hidden-state dropout (dropout_rate > 0), the parts that need no GPU: the row mask's definition
(tests/_dropout_rows_ref.py restates include/sae_attn.h), its statistics, the host-side validation
of the new C ABI entry points, and the ``dropout_rate`` plumbing of the ViT family."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import _dropout_ref as DR
import _dropout_rows_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sae_dropout_rows", "sae_dropout_rows_mask", "sae_layernorm_fwd_dropout", "sae_layernorm_bwd_dropout",
       "sae_tokens_fwd_dropout", "sae_tokens_bwd_dropout", "sae_gemm_nt_gelu_dropout"]


# ------------------------------------------------------------------------------ definition
def test_keep_rows_matches_the_scalar_definition():
    """The vectorised helper against the definition spelled out element by element: a 64-bit seed,
    an offset above 2^32, rows above 2^32 (both row counter words in use)."""
    M, C, rate, seed, off, sid = 5, 37, 0.25, (1 << 63) + 5, (1 << 32) + 5, 7
    row0, step = (1 << 33) + 3, 197
    keep = RR.keep_rows(M, C, rate, seed, off, sid, row0, step)
    assert keep.shape == (M, C) and keep.dtype == bool
    t, _ = DR.threshold(rate)
    k0, k1 = (int(x) for x in DR.philox4x32_10((off & DR.U32, off >> 32, sid, 0), (seed & DR.U32, seed >> 32))[:2])
    for i in range(M):
        row = row0 + i * step
        for col in range(C):
            w = DR.philox4x32_10((col >> 4, row & DR.U32, row >> 32, 1), (k0, k1))
            byte = (int(w[(col >> 2) & 3]) >> (8 * (col & 3))) & 0xff
            assert keep[i, col] == (byte >= t), (i, col)


def test_row0_row_step_select_rows_of_the_full_mask():
    full = RR.keep_rows(3 * 17, 192, 0.25, 1234, 0, 2)
    assert np.array_equal(RR.keep_rows(3, 192, 0.25, 1234, 0, 2, 0, 17), full[0::17])
    assert np.array_equal(RR.keep_rows(4, 192, 0.25, 1234, 0, 2, 5, 11), full[5::11][:4])
    assert np.array_equal(RR.keep_rows(51, 100, 0.25, 1234, 0, 2), full[:, :100])


# ------------------------------------------------------------------------- mask statistics
SEED = 1234


@pytest.fixture(scope="module", params=[(s, r) for s in [(394, 384), (394, 1536), (100, 192)] for r in (0.1, 0.25, 0.5)],
                ids=lambda p: f"{p[0][0]}x{p[0][1]}-{p[1]}")
def masks(request):
    (M, C), rate = request.param
    mk = lambda seed=SEED, off=0, sid=0: RR.keep_rows(M, C, rate, seed, off, sid)
    other = {"stream": mk(sid=1), "offset": mk(off=1), "seed": mk(seed=SEED + 1),
             "attention mask": DR.keep_mask(1, 1, M, C, rate, SEED, 0, 0)[0, 0]}
    return rate, mk(), other


def _sigma(p, n):
    return math.sqrt(p * (1 - p) / n)


def test_mask_keep_fraction(masks):
    rate, m, _ = masks
    _, pk = DR.threshold(rate)
    assert abs(m.mean() - pk) <= 5 * _sigma(pk, m.size)
    assert np.abs(m.mean(axis=1) - pk).max() <= 5 * _sigma(pk, m.shape[1])    # every row
    assert np.abs(m.mean(axis=0) - pk).max() <= 5 * _sigma(pk, m.shape[0])    # every column


def test_mask_independence(masks):
    """Two independent Bernoulli(pk) masks agree with probability pk^2 + (1 - pk)^2."""
    rate, m, other = masks
    _, pk = DR.threshold(rate)
    a = pk * pk + (1 - pk) * (1 - pk)
    pairs = {name: (m, o) for name, o in other.items()}
    pairs["adjacent rows"] = (m[:-1], m[1:])
    pairs["adjacent columns"] = (m[:, :-1], m[:, 1:])
    pairs["16 columns on"] = (m[:, :-16], m[:, 16:])
    for name, (x, y) in pairs.items():
        agree = (x == y).mean()
        assert abs(agree - a) <= 5 * _sigma(a, x.size), (name, agree, a)


# ----------------------------------------------------------------------------------- C ABI
def test_header_declares_and_library_exports():
    import sae_vision_amd
    from sae_vision_amd import _lib as L
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sae_attn.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sae_[a-z0-9_]+)\s*\(", src))
    lib = sae_vision_amd.load_library()
    for n in NEW:
        assert n in declared and n in L.EXPORTED_SYMBOLS and hasattr(lib, n), n
    assert L.ABI_VERSION == 1 and lib.sae_abi_version() == 1
    assert "#define SAE_ABI_VERSION 1" in src


def _calls(lib, rate, rng, row_step):
    """Every new entry point with dummy pointers (never dereferenced on the host)."""
    p = ctypes.c_void_p(4096)
    yield "dropout_rows", lib.sae_dropout_rows(None, 4, 16, 1, p, 16, p, 16, rate, rng, 0, 0, row_step)
    yield "dropout_rows_mask", lib.sae_dropout_rows_mask(None, 4, 16, rate, rng, 0, 0, row_step, p)
    yield "layernorm_fwd_dropout", lib.sae_layernorm_fwd_dropout(None, 4, 16, p, p, p, p, p, p, p, p, 1e-6, rate, rng,
                                                                 0, 0, row_step)
    yield "layernorm_bwd_dropout", lib.sae_layernorm_bwd_dropout(None, 4, 16, p, p, p, p, p, p, p, p, p, p, p, rate,
                                                                 rng, 0, 0, row_step)
    if row_step >= 1:   # the tokens and GEMM forms take no row_step
        yield "tokens_fwd_dropout", lib.sae_tokens_fwd_dropout(None, 2, 4, 16, p, p, p, p, rate, rng, 0)
        yield "tokens_bwd_dropout", lib.sae_tokens_bwd_dropout(None, 2, 4, 16, p, p, p, p, rate, rng, 0)
        yield "gemm_nt_gelu_dropout", lib.sae_gemm_nt_gelu_dropout(None, 8, 8, 8, p, 8, p, 8, p, p, 8, p, rate, rng, 0)


@pytest.mark.parametrize("rate,rng,row_step,msg", [
    (1.0, 4096, 1, "rate"),
    (-0.1, 4096, 1, "rate"),
    (float("nan"), 4096, 1, "rate"),
    (0.1, None, 1, "rng"),
    (0.1, 4096, 0, "row_step"),
    (0.1, 4096, -3, "row_step"),
])
def test_validation_errors(rate, rng, row_step, msg):
    """Refused on the host, before any HIP call (dummy pointers, no device)."""
    import sae_vision_amd
    from sae_vision_amd import _lib as L
    lib = sae_vision_amd.load_library()
    n = 0
    for name, rc in _calls(lib, rate, None if rng is None else ctypes.c_void_p(rng), row_step):
        err = lib.sae_last_error().decode()
        assert rc == L.SAE_EINVAL, (name, rc, err)
        assert msg in err and name in err, (name, err)
        n += 1
    assert n == (7 if row_step >= 1 else 4)


def test_dropout_forms_keep_the_plain_checks():
    """Past the dropout arguments the validation is the plain entry point's, at T = 0 (forwarded)
    and at T > 0 alike."""
    import sae_vision_amd
    from sae_vision_amd import _lib as L
    lib = sae_vision_amd.load_library()
    p, rng = ctypes.c_void_p(4096), ctypes.c_void_p(4096)
    for rate in (0.0, 0.001, 0.1):
        assert lib.sae_layernorm_fwd_dropout(None, 4, 2048, p, p, p, p, p, p, p, p, 1e-6, rate, rng, 0, 0, 1) == \
            L.SAE_EUNSUPPORTED and "layernorm" in lib.sae_last_error().decode()
        assert lib.sae_layernorm_bwd_dropout(None, 4, 18, p, p, p, p, p, p, p, p, p, p, p, rate, rng, 0, 0, 1) == \
            L.SAE_EUNSUPPORTED
        assert lib.sae_tokens_fwd_dropout(None, 2, 4, 18, p, p, p, p, rate, rng, 0) == L.SAE_EINVAL
        assert lib.sae_tokens_bwd_dropout(None, 2, 4, 16, p, None, p, p, rate, rng, 0) == L.SAE_EINVAL
        assert lib.sae_gemm_nt_gelu_dropout(None, 8, 12, 8, p, 8, p, 8, p, p, 16, p, rate, rng, 0) == L.SAE_EUNSUPPORTED
        assert lib.sae_gemm_nt_gelu_dropout(None, 8, 8, 8, p, 8, p, 8, p, p, 8, None, rate, rng, 0) == L.SAE_EINVAL
        assert "c2" in lib.sae_last_error().decode()
    assert lib.sae_layernorm_fwd_dropout(None, 4, 16, p, None, None, p, p, p, p, p, 1e-6, 0.1, rng, 0, 0, 1) == L.SAE_EINVAL
    assert "delta" in lib.sae_last_error().decode()
    assert lib.sae_dropout_rows(None, 4, 16, 7, p, 16, p, 16, 0.1, rng, 0, 0, 1) == L.SAE_EINVAL
    assert lib.sae_dropout_rows(None, 4, 16, 1, p, 8, p, 16, 0.1, rng, 0, 0, 1) == L.SAE_EINVAL
    assert lib.sae_dropout_rows_mask(None, 4, 16, 0.1, rng, 0, 0, 1, None) == L.SAE_EINVAL


# ---------------------------------------------------------------------------------- Python
def test_vit_carries_dropout_rate():
    import torch
    from sae_vision_amd import vit
    models = [vit.ViT(num_classes=10, num_layers=2, num_heads=3, embed_dim=48, patch_shape=(16, 16), img_size=32,
                      dtype=torch.bfloat16, dropout_rate=0.1),
              vit.create_model("deit_ti_patch16", 10, torch.bfloat16, img_size=32, dropout_rate=0.1)]
    for m in models:
        assert m.dropout_rate == 0.1 and m.Encoder_0.dropout_rate == 0.1
        blocks = [b for b in m.modules() if isinstance(b, vit.EncoderBlock)]
        ffs = [b for b in m.modules() if isinstance(b, vit.FFBlock)]
        assert len(blocks) == len(ffs) == m.Encoder_0.num_layers
        assert all(b.dropout_rate == 0.1 for b in blocks + ffs)
        # the block owns the attention-output dropout; the attention module keeps none of its own
        assert all(b.SelfAttentionBlock_0.out_dropout_rate == 0.0 and b.SelfAttentionBlock_0.attn_dropout_rate == 0.0
                   for b in blocks)
    plain = vit.create_model("deit_ti_patch16", 10, torch.bfloat16, img_size=32)
    assert plain.dropout_rate == 0.0 and plain.Encoder_0.dropout_rate == 0.0
    assert all(b.dropout_rate == 0.0 for b in plain.modules() if isinstance(b, (vit.EncoderBlock, vit.FFBlock)))


def test_positional_callers_keep_working():
    """dropout_rate is appended after the existing parameters."""
    import torch
    from sae_vision_amd import vit
    m = vit.ViT(10, 1, 3, 48, (16, 16), 32, 4, torch.float32, None, 0.2)
    assert m.Encoder_0.EncoderBlock_0.SelfAttentionBlock_0.attn_dropout_rate == 0.2 and m.dropout_rate == 0.0
    m = vit.ViT(10, 1, 3, 48, (16, 16), 32, 4, torch.float32, None, 0.2, 0.3)
    assert m.Encoder_0.EncoderBlock_0.FFBlock_0.dropout_rate == 0.3
    assert vit.FFBlock(48, 4, None).dropout_rate == 0.0 and vit.FFBlock(48, 4, None, 0.3).dropout_rate == 0.3
    e = vit.Encoder(5, 48, 1, 3, 4, torch.float32, None, 0.2, 0.3)
    assert e.dropout_rate == 0.3 and e.EncoderBlock_0.dropout_rate == 0.3
    assert vit.create_model("deit_ti_patch16", 10, torch.float32, 32, None, 0.2, 0.3).dropout_rate == 0.3

