"""Attention-probability dropout, the parts that need no GPU: the generator and mask definition
(tests/_dropout_ref.py restates include/sae_attn.h), the mask's statistics, the host-side
validation of the new C ABI entry points, and the ``attn_dropout_rate`` plumbing of the ViT family."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import _dropout_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sae_attn_fwd_dropout", "sae_attn_bwd_dropout", "sae_attn_dropout_mask", "sae_dropout_advance"]


# ------------------------------------------------------------------------------- generator
@pytest.mark.parametrize("ctr,key,out", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, out):
    assert tuple(int(x) for x in DR.philox4x32_10(ctr, key)) == out


@pytest.mark.parametrize("rate,t", [(0.0, 0), (0.001, 0), (0.1, 26), (0.25, 64), (0.5, 128), (0.999, 255)])
def test_threshold(rate, t):
    got, pk = DR.threshold(rate)
    assert got == t and pk == (256 - t) / 256


def test_mask_matches_the_scalar_definition():
    """The vectorised helper against the definition spelled out element by element."""
    B, H, Nq, Nk, rate, seed, off, sid = 1, 2, 6, 9, 0.25, (1 << 63) + 5, (1 << 32) + 5, 7
    keep = DR.keep_mask(B, H, Nq, Nk, rate, seed, off, sid)
    t, _ = DR.threshold(rate)
    k0, k1 = (int(x) for x in DR.philox4x32_10((off & DR.U32, off >> 32, sid, 0), (seed & DR.U32, seed >> 32))[:2])
    for bh in range(B * H):
        for q in range(Nq):
            for k in range(Nk):
                w = DR.philox4x32_10((k >> 2, q >> 2, bh, 0), (k0, k1))
                byte = (int(w[q & 3]) >> (8 * (k & 3))) & 0xff
                assert keep[bh // H, bh % H, q, k] == (byte >= t)


# ------------------------------------------------------------------------- mask statistics
SHAPE, SEED = (2, 3, 197, 197), 1234


@pytest.fixture(scope="module", params=[0.1, 0.25, 0.5])
def masks(request):
    rate = request.param
    mk = lambda seed=SEED, off=0, sid=0: DR.keep_mask(*SHAPE, rate, seed, off, sid)
    return rate, mk(), {"stream": mk(sid=1), "offset": mk(off=1), "seed": mk(seed=SEED + 1)}


def _sigma(p, n):
    return math.sqrt(p * (1 - p) / n)


def test_mask_keep_fraction(masks):
    rate, m, _ = masks
    _, pk = DR.threshold(rate)
    assert abs(m.mean() - pk) <= 5 * _sigma(pk, m.size)
    assert np.abs(m.mean(axis=3) - pk).max() <= 5 * _sigma(pk, m.shape[3])    # every row
    assert np.abs(m.mean(axis=2) - pk).max() <= 5 * _sigma(pk, m.shape[2])    # every column


def test_mask_independence(masks):
    """Two independent Bernoulli(pk) masks agree with probability pk^2 + (1 - pk)^2."""
    rate, m, other = masks
    _, pk = DR.threshold(rate)
    a = pk * pk + (1 - pk) * (1 - pk)
    pairs = {name: (m, o) for name, o in other.items()}
    pairs["head"] = (m[:, 0], m[:, 1])
    pairs["adjacent queries"] = (m[:, :, :-1], m[:, :, 1:])
    pairs["adjacent keys"] = (m[..., :-1], m[..., 1:])
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


def _calls(lib, d, rate, rng):
    dummy = ctypes.c_void_p(16)
    yield lib.sae_attn_fwd_dropout(None, ctypes.byref(d), dummy, dummy, dummy, dummy, None, rate, rng, 0)
    yield lib.sae_attn_bwd_dropout(None, ctypes.byref(d), dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy,
                                   dummy, dummy, rate, rng, 0)


@pytest.mark.parametrize("rate,rng,flags,code,msg", [
    (1.0, 16, 0, "SAE_EINVAL", "rate"),
    (-0.1, 16, 0, "SAE_EINVAL", "rate"),
    (float("nan"), 16, 0, "SAE_EINVAL", "rate"),
    (0.1, None, 0, "SAE_EINVAL", "rng"),
    (0.1, 16, 1, "SAE_EUNSUPPORTED", "flags"),
])
def test_dropout_validation_errors(rate, rng, flags, code, msg):
    """Refused on the host, before any HIP call (dummy pointers, no device)."""
    import sae_vision_amd
    from sae_vision_amd import _lib as L
    lib = sae_vision_amd.load_library()
    d = L.SaeAttnDesc()
    lib.sae_attn_desc_init(ctypes.byref(d), 1, 1, 4, 4, 64, L.SAE_DTYPE_F32, 1.0)
    assert L.SAE_FLAG_RELPOS == 1
    d.flags = flags
    for rc in _calls(lib, d, rate, None if rng is None else ctypes.c_void_p(rng)):
        assert rc == getattr(L, code)
        assert msg in lib.sae_last_error().decode()


def test_dropout_keeps_the_descriptor_checks():
    import sae_vision_amd
    from sae_vision_amd import _lib as L
    lib = sae_vision_amd.load_library()
    d = L.SaeAttnDesc()
    lib.sae_attn_desc_init(ctypes.byref(d), 1, 1, 4, 4, 256, L.SAE_DTYPE_F32, 1.0)
    for rate in (0.0, 0.1):   # T == 0 forwards to the plain entry points, which validate alike
        for rc in _calls(lib, d, rate, ctypes.c_void_p(16)):
            assert rc == L.SAE_EUNSUPPORTED and "head_dim 256" in lib.sae_last_error().decode()
    dummy = ctypes.c_void_p(16)
    assert lib.sae_attn_dropout_mask(None, 1, 1, 4, 4, 1.5, dummy, 0, dummy) == L.SAE_EINVAL
    assert "rate" in lib.sae_last_error().decode()
    assert lib.sae_attn_dropout_mask(None, 1, 1, 4, 4, 0.5, None, 0, dummy) == L.SAE_EINVAL
    assert lib.sae_dropout_advance(None, None, 1) == L.SAE_EINVAL


# ---------------------------------------------------------------------------------- Python
def test_vit_carries_attn_dropout_rate():
    import torch
    from sae_vision_amd import vit
    from sae_vision_amd.layers import SelfAttentionBlock
    models = [vit.ViT(num_classes=10, num_layers=2, num_heads=3, embed_dim=48, patch_shape=(16, 16), img_size=32,
                      dtype=torch.bfloat16, attn_dropout_rate=0.1),
              vit.create_model("deit_ti_patch16", 10, torch.bfloat16, img_size=32, attn_dropout_rate=0.1)]
    for m in models:
        blocks = [b for b in m.modules() if isinstance(b, SelfAttentionBlock)]
        assert len(blocks) == m.Encoder_0.num_layers and all(b.attn_dropout_rate == 0.1 for b in blocks)
    plain = vit.create_model("deit_ti_patch16", 10, torch.bfloat16, img_size=32)
    assert all(b.attn_dropout_rate == 0.0 for b in plain.modules() if isinstance(b, SelfAttentionBlock))
