"""Drop-in attention modules mirroring the reference's Flax API.

Reference: models/layers/attentions/attention.py:10-74 (AttentionBlock, SelfAttentionBlock),
models/layers/attentions/talking_heads.py:5-14 (TalkingHeadsBlock), models/cait.py:10-15
(ClassSelfAttentionBlock), models/ceit.py:11-16 (LCSelfAttentionBlock).

Same dataclass fields, same call signatures (``(inputs_q, inputs_kv, is_training)`` /
``(inputs, is_training)``), same parameter tree (``queries/kernel [C,H,D]``,
``keys/kernel``, ``values/kernel``, ``DenseGeneral_0/kernel [H,D,C]``, optional ``bias``,
``TalkingHeadsBlock_0/talking_heads_transform [H,H]`` and ``_1``), parameters kept in fp32 and
cast to ``dtype`` for compute like Flax's DenseGeneral.  Parameters are created at
construction when ``in_ch`` is given, otherwise at the first call (Flax ``init`` semantics).

Compute path: projections go through ``ops.dense``.  bf16 forward and input gradient run on the
hand-written ``sae_gemm_nt`` for every width that is a multiple of 8 (the C ABI picks the kernel:
the persistent LDS-DMA ``gemm8`` for 192-wide output tiles -- every DeiT-S / CaiT shape and the
ViT-B wide forwards --, the ping-pong ``gemm8x`` for the 768 / 1024-feature outputs at K >= 768,
the 128-row kernel for the rest, K-tail instances included); the fp32 compute dtype runs on the
exact-f32 MFMA GEMM ``sae_gemm_f32``; weight / bias gradients go straight into fp32 through the
split-token MFMA kernels (``sae_gemm_dw``).  The self-attention Q/K/V projection is ONE GEMM
producing a packed [B, N, 3, H, D] buffer that the attention kernel reads in place by strides; the
attention core is the fused HIP kernel (``ops.attention*``).  There is no eager/CPU fallback.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops

# rotary base (position_embed.py: build-defined, survey D6); the standalone ops.rotary default
ROTARY_BASE = 10000.0

__all__ = ["DenseGeneral", "AttentionBlock", "SelfAttentionBlock", "TalkingHeadsBlock",
           "ClassSelfAttentionBlock", "LCSelfAttentionBlock", "attention_tail", "lecun_normal_", "numbered",
           "flax_params", "load_flax_params"]


def lecun_normal_(t: torch.Tensor, fan_in: int) -> torch.Tensor:
    """Flax ``initializers.lecun_normal()``: variance_scaling(1, 'fan_in', 'truncated_normal')."""
    std = math.sqrt(1.0 / fan_in) / 0.87962566103423978
    with torch.no_grad():
        return nn.init.trunc_normal_(t, mean=0.0, std=std, a=-2.0 * std, b=2.0 * std)


class DenseGeneral(nn.Module):
    """Parameter holder named like Flax's ``nn.DenseGeneral`` (kernel [*in, *out], bias [*out])."""

    def __init__(self, in_shape, out_shape, use_bias: bool, device=None):
        super().__init__()
        in_shape, out_shape = tuple(in_shape), tuple(out_shape)
        self.in_shape, self.out_shape = in_shape, out_shape
        fan_in = int(math.prod(in_shape))
        self.kernel = nn.Parameter(lecun_normal_(torch.empty(in_shape + out_shape, device=device), fan_in))
        self.bias = nn.Parameter(torch.zeros(out_shape, device=device)) if use_bias else None


class TalkingHeadsBlock(nn.Module):
    """``TalkingHeadsBlock(num_heads)`` (talking_heads.py:5-14).  Holds the fp32
    ``talking_heads_transform`` [H, H] (orthogonal init, indexed [h_in, h_out]).  Inside
    AttentionBlock the mix is fused into the HIP kernel; calling the block directly applies
    ``einsum('h i, b h ... -> b i ...')`` as the reference does."""

    def __init__(self, num_heads: int, device=None):
        super().__init__()
        self.num_heads = num_heads
        t = torch.empty(num_heads, num_heads, device=device)
        nn.init.orthogonal_(t)
        self.talking_heads_transform = nn.Parameter(t)

    def forward(self, inputs: torch.Tensor) -> torch.Tensor:
        w = self.talking_heads_transform
        return torch.einsum("hi,bh...->bi...", w.to(torch.promote_types(w.dtype, inputs.dtype)),
                            inputs.to(torch.promote_types(w.dtype, inputs.dtype)))


def attention_tail(blk, q, k, v, is_training: bool, qkv=None, rope=None) -> torch.Tensor:
    """What follows the projections of ``blk`` (attention.py:39-67, cvt_attention.py:85-113): the core on q, k, v
    [B, N, H, D] or on the packed ``qkv`` [B, N, 3, H, D] they are views of, the output projection, its dropout."""
    drop = None   # attention-probability dropout (attention.py:54-58): inside the attention kernels
    if is_training and blk.attn_dropout_rate > 0.0:
        if blk.talking_heads:
            raise NotImplementedError(
                "attn_dropout_rate > 0 with talking_heads=True is not implemented: the reference drops after the "
                "second head mix (attention.py:50-56, cvt_attention.py:100-104); the talking-heads kernels have none")
        drop = (blk.attn_dropout_rate, ops.dropout_rng(q.device))
    B, Nq, H, D = q.shape
    scale = 1.0 / math.sqrt(D)
    if blk.talking_heads:
        th = (blk.TalkingHeadsBlock_0.talking_heads_transform, blk.TalkingHeadsBlock_1.talking_heads_transform)
        o = (ops.talking_heads_attention_packed(qkv, *th, scale, rope) if qkv is not None else
             ops.talking_heads_attention(q, k, v, *th, scale, rope))
    elif qkv is not None:
        o = ops.attention_packed(qkv, scale, rope, dropout=drop)
    else:
        o = ops.attention(q, k, v, scale, rotary=rope, dropout=drop)
    out = blk.DenseGeneral_0
    y = ops.dense(o.reshape(B, Nq, H * D), out.kernel.reshape(H * D, -1), out.bias if blk.use_bias else None, blk.dtype)
    return F.dropout(y, p=blk.out_dropout_rate, training=is_training) if blk.out_dropout_rate > 0.0 else y


class AttentionBlock(nn.Module):
    """``AttentionBlock`` (attention.py:10-67)."""

    def __init__(self, num_heads: int, head_ch: Optional[int] = None, out_ch: Optional[int] = None,
                 talking_heads: bool = False, attn_dropout_rate: float = 0.0, out_dropout_rate: float = 0.0,
                 use_bias: bool = False, dtype: torch.dtype = torch.float32, *, in_ch: Optional[int] = None,
                 rotary: bool = False, device=None):
        super().__init__()
        self.num_heads = num_heads
        self.head_ch = head_ch
        self.out_ch = out_ch
        self.talking_heads = talking_heads
        self.attn_dropout_rate = attn_dropout_rate
        self.out_dropout_rate = out_dropout_rate
        self.use_bias = use_bias
        self.dtype = dtype
        self.rotary = rotary          # build-defined rotary on q/k (README to-do, survey D6)
        self._in_ch = None
        if in_ch is not None:
            self._build(in_ch, device)

    # -- parameters --------------------------------------------------------------------
    def _build(self, in_ch: int, device=None):
        assert in_ch % self.num_heads == 0
        head_ch = self.head_ch or int(in_ch / self.num_heads)
        out_ch = self.out_ch or in_ch
        H = self.num_heads
        self._in_ch, self._head_ch_eff, self._out_ch_eff = in_ch, head_ch, out_ch
        self.queries = DenseGeneral((in_ch,), (H, head_ch), self.use_bias, device)
        self.keys = DenseGeneral((in_ch,), (H, head_ch), self.use_bias, device)
        self.values = DenseGeneral((in_ch,), (H, head_ch), self.use_bias, device)
        if self.talking_heads:
            self.TalkingHeadsBlock_0 = TalkingHeadsBlock(H, device)
            self.TalkingHeadsBlock_1 = TalkingHeadsBlock(H, device)
        self.DenseGeneral_0 = DenseGeneral((H, head_ch), (out_ch,), self.use_bias, device)

    def weight_groups(self):
        """The fp32 kernels as the 2-D column blocks the projections use (``ops.forward_casts``)."""
        if self._in_ch is None:
            return []
        C, HD = self._in_ch, self.num_heads * self._head_ch_eff
        return [[m.kernel.reshape(C, HD) for m in (self.queries, self.keys, self.values)],
                [self.DenseGeneral_0.kernel.reshape(HD, self._out_ch_eff)]]

    def cross_weight_groups(self):
        """The column blocks the projections use when queries and keys / values come from
        different inputs (class / last-token attention): [queries], [keys | values], [output]."""
        if self._in_ch is None:
            return []
        C, HD = self._in_ch, self.num_heads * self._head_ch_eff
        return [[self.queries.kernel.reshape(C, HD)],
                [m.kernel.reshape(C, HD) for m in (self.keys, self.values)],
                [self.DenseGeneral_0.kernel.reshape(HD, self._out_ch_eff)]]

    # -- forward -----------------------------------------------------------------------
    def forward(self, inputs_q: torch.Tensor, inputs_kv: torch.Tensor, is_training: bool) -> torch.Tensor:
        assert inputs_q.ndim == inputs_kv.ndim == 3
        in_ch = inputs_q.shape[-1]
        assert in_ch % self.num_heads == 0
        if self._in_ch is None:
            self._build(in_ch, inputs_q.device)
        elif self._in_ch != in_ch:
            raise ValueError(f"AttentionBlock built for {self._in_ch} channels, got {in_ch}")
        H, D, dt = self.num_heads, self._head_ch_eff, self.dtype
        B, Nq, _ = inputs_q.shape
        xq, qkv = inputs_q.to(dt), None
        bias = lambda *ms: torch.stack([m.bias for m in ms], 0).reshape(-1) if self.use_bias else None
        if inputs_q is inputs_kv:
            # ONE projection GEMM producing the packed [B, N, 3, H, D] buffer the kernels read in place
            qkv = ops.dense(xq, self.weight_groups()[0], bias(self.queries, self.keys, self.values), dt)
            qkv = qkv.view(B, Nq, 3, H, D)
            q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
        else:
            wq, wkv, _ = self.cross_weight_groups()
            q = ops.dense(xq, wq, self.queries.bias.reshape(-1) if self.use_bias else None, dt).view(B, Nq, H, D)
            kv = ops.dense(inputs_kv.to(dt), wkv, bias(self.keys, self.values), dt).view(B, -1, 2, H, D)
            k, v = kv[:, :, 0], kv[:, :, 1]
        # rotary (position_embed.py:8-20) rides inside the attention kernels: q / k stay un-rotated
        return attention_tail(self, q, k, v, is_training, qkv, ROTARY_BASE if self.rotary else None)


class SelfAttentionBlock(AttentionBlock):
    """``SelfAttentionBlock`` (attention.py:70-74): ``AttentionBlock(inputs, inputs)``."""

    def forward(self, inputs: torch.Tensor, is_training: bool) -> torch.Tensor:  # type: ignore[override]
        return super().forward(inputs, inputs, is_training=is_training)


class ClassSelfAttentionBlock(AttentionBlock):
    """CaiT class attention (models/cait.py:10-15): query = token 0 (CLS), keys = all tokens."""

    def forward(self, inputs: torch.Tensor, is_training: bool) -> torch.Tensor:  # type: ignore[override]
        inputs_q = inputs[:, 0:1, :]
        return super().forward(inputs_q, inputs, is_training=is_training)


class LCSelfAttentionBlock(AttentionBlock):
    """CeiT layer-wise class-token attention (models/ceit.py:11-16): query = last token."""

    def forward(self, inputs: torch.Tensor, is_training: bool) -> torch.Tensor:  # type: ignore[override]
        inputs_q = inputs[:, -1:, :]
        return super().forward(inputs_q, inputs, is_training=is_training)


# ------------------------------------------------------------------ Flax param-tree interop
def numbered(module: nn.Module, name: str):
    """The Flax-style numbered children ``name_0, name_1, ...`` of ``module``, by number."""
    found = ((key.rpartition("_"), m) for key, m in module.named_children())
    return [m for _, m in sorted((int(n), m) for (stem, _, n), m in found if stem == name and n.isdigit())]


def flax_params(module: nn.Module) -> Dict:
    """Nested dict of fp32 tensors in the reference's Flax param-tree layout
    (``{'queries': {'kernel': ...}, 'DenseGeneral_0': {...}, ...}``)."""
    tree: Dict = {}
    for name, p in module.named_parameters():
        node = tree
        parts = name.split(".")
        for part in parts[:-1]:
            node = node.setdefault(part, {})
        node[parts[-1]] = p.detach()
    return tree


def load_flax_params(module: nn.Module, tree: Dict) -> None:
    """Copy a Flax-layout param tree (nested dict of arrays / tensors) into ``module``."""
    params = dict(module.named_parameters())

    def walk(node, prefix):
        for k, v in node.items():
            key = f"{prefix}.{k}" if prefix else k
            if isinstance(v, dict):
                walk(v, key)
            else:
                if key not in params:
                    raise KeyError(f"unexpected parameter {key!r}")
                t = torch.as_tensor(v)
                if tuple(t.shape) != tuple(params[key].shape):
                    raise ValueError(f"{key}: shape {tuple(t.shape)} != {tuple(params[key].shape)}")
                with torch.no_grad():
                    params[key].copy_(t.to(params[key].dtype))

    walk(tree, "")
