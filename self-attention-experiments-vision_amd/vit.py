"""ViT / DeiT -- the caller of the attention hot path used for the end-to-end img/s metric.

Mirrors models/vit.py:9-99 (EncoderBlock, Encoder, ViT), models/layers/stems/patch_embed.py:8-26
(PatchEmbedBlock), models/layers/feedforwards/ff.py:8-34 (FFBlock) and
models/layers/position_embed.py:48-57 (AddAbsPosEmbed), with Flax-style submodule names so
the parameter tree matches (``PatchEmbedBlock_0/Dense_0/kernel``, ``cls``,
``Encoder_0/EncoderBlock_i/SelfAttentionBlock_0/queries/kernel``, ...).  Numerics follow the
reference's mixed precision: fp32 params, ``dtype`` compute, fp32 residual stream (the fp32
cls / pos-embed params promote it, vit.py:46,85), LayerNorm eps 1e-6, tanh-GELU (Flax
``nn.gelu`` default).

The attention is ``layers.SelfAttentionBlock`` (fused HIP kernels); Dense / DenseGeneral go through ``ops.dense``
(library GEMM forward and input gradient, HIP split-token weight/bias gradients).  The block is written once,
``EncoderBlock.body``, on the stream operations of ``layers/stream.py``: every residual add is made together with the
LayerNorm that follows it.  ``Encoder.forward`` decides the route once, on the stream that enters the first block,
and runs one loop of bodies.  HIP route (bf16 compute): each add + LayerNorm is one kernel (``ops.add_layer_norm``),
every Dense kernel of the encoder is cast to bf16 in one launch up front and the FF block runs as ``ops.ff_block``
(tanh-GELU and its derivative fused into the GEMM epilogues).  Framework route: the same adds and LayerNorms as
framework ops, in the same order.

``dropout_rate`` (vit.py:12,39,68) reaches four places per training forward, each drawing one stream id of the
device's ``ops.DropoutRng`` in this order: the encoder input after the position embedding (vit.py:47); then per block
the attention probabilities (``attn_dropout_rate``, inside the attention kernels), the attention output (attention.py
``out_dropout_rate``), the FF hidden activation after the GELU (ff.py:30) and the FF output (ff.py:32).  On the HIP
route none of them is a pass of its own: the input dropout rides in ``ops.encoder_tokens``, the hidden one in the GELU
GEMM's epilogue, the two output ones in the ``ops.add_layer_norm`` that follows; the framework route applies
``ops.dropout_rows`` at the same places.  Both routes run the one body, so one seed gives one set of masks.
"""
from __future__ import annotations

import contextlib
from typing import Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .layers.attention import DenseGeneral, SelfAttentionBlock, lecun_normal_, numbered
from .layers.stream import add_norm, fused, hidden_dropout, norm_pass

__all__ = ["ViT", "create_model", "MODEL_CONFIGS", "vit_flops_per_image"]


class Dense(nn.Module):
    """Flax ``nn.Dense`` param holder (kernel [in, out] lecun_normal, bias zeros)."""

    def __init__(self, in_features, features, use_bias=True, zero_init=False, device=None):
        super().__init__()
        k = torch.zeros(in_features, features, device=device)
        if not zero_init:
            lecun_normal_(k, in_features)
        self.kernel = nn.Parameter(k)
        self.bias = nn.Parameter(torch.zeros(features, device=device)) if use_bias else None

    def forward(self, x, dtype):
        return ops.dense(x, self.kernel, self.bias, dtype)


class LayerNorm(nn.Module):
    """Flax ``nn.LayerNorm(dtype)``: params ``scale`` / ``bias``, eps 1e-6, output in dtype."""

    def __init__(self, dim, device=None):
        super().__init__()
        self.scale = nn.Parameter(torch.ones(dim, device=device))
        self.bias = nn.Parameter(torch.zeros(dim, device=device))

    def forward(self, x, dtype):
        return F.layer_norm(x.float(), (x.shape[-1],), self.scale, self.bias, 1e-6).to(dtype)


class FFBlock(nn.Module):
    """ff.py:8-34 (expand_ratio, Dense -> GELU -> Dropout -> Dense -> Dropout)."""

    def __init__(self, dim, expand_ratio=4, device=None, dropout_rate: float = 0.0):
        super().__init__()
        hid = max(1, int(expand_ratio * dim))
        self.dropout_rate = dropout_rate
        self.Dense_0 = Dense(dim, hid, device=device)
        self.Dense_1 = Dense(hid, dim, device=device)

    def forward(self, x, dtype, is_training: bool = False, out_dropout: bool = True):
        """``out_dropout=False``: the caller applies the output dropout (ff.py:32) itself, inside the
        residual add that follows (``stream.add_norm(dropout=...)``)."""
        d0, d1 = self.Dense_0, self.Dense_1
        drop = hidden_dropout(self.dropout_rate, is_training, x.device)
        if dtype == torch.bfloat16 and ops.ff_block_ok(x, d0.kernel, d1.kernel):
            # GELU (and the hidden dropout) fused into Dense_0's GEMM epilogue, its derivative into
            # Dense_1's dX GEMM
            y = ops.ff_block(x, d0.kernel, d0.bias, d1.kernel, d1.bias, dropout=drop)
        else:
            y = d1(ops.dropout_rows(F.gelu(d0(x, dtype), approximate="tanh"), drop), dtype)
        return ops.dropout_rows(y, drop) if out_dropout else y


class EncoderBlock(nn.Module):
    """vit.py:9-32.  ``body`` is the block; ``forward`` runs it on a stream of its own."""

    def __init__(self, dim, num_heads, expand_ratio, dtype, device=None, attn_dropout_rate: float = 0.0,
                 dropout_rate: float = 0.0):
        super().__init__()
        self.dtype = dtype
        self.dropout_rate = dropout_rate
        self.LayerNorm_0 = LayerNorm(dim, device)
        # out_dropout_rate stays 0: the block applies the attention-output dropout (vit.py:22) in its residual add
        self.SelfAttentionBlock_0 = SelfAttentionBlock(num_heads=num_heads, attn_dropout_rate=attn_dropout_rate,
                                                       dtype=dtype, in_ch=dim, device=device)
        self.LayerNorm_1 = LayerNorm(dim, device)
        self.FFBlock_0 = FFBlock(dim, expand_ratio, device, dropout_rate)

    def body(self, x, h, next_ln, is_training, route, cls_only=False):
        """The block on the stream ``x`` and ``h = LayerNorm_0(x)`` -> ``(x', next_ln(x'))`` (``stream.add_norm``)."""
        drop = hidden_dropout(self.dropout_rate, is_training, x.device)
        a = self.SelfAttentionBlock_0(h, is_training=is_training)
        x, h = add_norm(x, a, self.LayerNorm_1, self.dtype, route, dropout=drop)
        f = self.FFBlock_0(h, self.dtype, is_training, out_dropout=False)
        return add_norm(x, f, next_ln, self.dtype, route, dropout=drop, cls_only=cls_only)

    def forward(self, inputs, is_training):
        """The body on the route of ``inputs``: a lone bf16 block now runs the HIP LayerNorms too, as in the encoder."""
        route = fused(inputs, self.dtype)
        x, h = norm_pass(inputs, self.LayerNorm_0, self.dtype, route)
        return self.body(x, h, None, is_training, route)[0]


def encoder_weight_groups(blocks):
    """Column-block groups of every Dense kernel of the blocks (attention QKV / output projection,
    FF Dense_0 / Dense_1) for ``ops.forward_casts``."""
    groups = []
    for blk in blocks:
        groups += blk.SelfAttentionBlock_0.weight_groups()
        groups += [[blk.FFBlock_0.Dense_0.kernel], [blk.FFBlock_0.Dense_1.kernel]]
    return groups


def encoder_casts(blocks, route: bool):
    """For an encoder's loop: on the HIP route every Dense kernel of ``blocks`` cast in one launch up front."""
    return ops.forward_casts(encoder_weight_groups(blocks)) if route else contextlib.nullcontext()


class Encoder(nn.Module):
    """vit.py:35-58 (AddAbsPosEmbed_0 + EncoderBlock_i + LayerNorm_0)."""

    def __init__(self, num_tokens, dim, num_layers, num_heads, expand_ratio, dtype, device=None,
                 attn_dropout_rate: float = 0.0, dropout_rate: float = 0.0):
        super().__init__()
        self.dtype = dtype
        self.dropout_rate = dropout_rate
        self.AddAbsPosEmbed_0 = nn.Module()
        self.AddAbsPosEmbed_0.pos_embed = nn.Parameter(torch.randn(1, num_tokens, dim, device=device) * 0.02)
        for i in range(num_layers):
            setattr(self, f"EncoderBlock_{i}", EncoderBlock(dim, num_heads, expand_ratio, dtype, device,
                                                            attn_dropout_rate, dropout_rate))
        self.num_layers = num_layers
        self.LayerNorm_0 = LayerNorm(dim, device)

    def forward(self, inputs, is_training, pos_added: bool = False, cls_only: bool = False):
        """``pos_added``: ``inputs`` already hold the position embedding and, when training with
        ``dropout_rate > 0``, the input dropout of vit.py:47 (ops.encoder_tokens).
        ``cls_only``: return only token 0 of the normalised output, [B, E] (what ViT's head reads,
        vit.py:95): the final residual add and LayerNorm (row-wise) then run on those rows only."""
        x = inputs
        if not pos_added:
            x = inputs.float() + self.AddAbsPosEmbed_0.pos_embed
            x = ops.dropout_rows(x, hidden_dropout(self.dropout_rate, is_training, x.device))
        blocks = numbered(self, "EncoderBlock")
        route = bool(blocks) and fused(x, self.dtype)   # decided on the first block's input, and held
        lns = [blk.LayerNorm_0 for blk in blocks] + [self.LayerNorm_0]   # lns[i + 1] reads block i's output
        with encoder_casts(blocks, route):
            x, h = norm_pass(x, lns[0], self.dtype, route)
            for blk, ln in zip(blocks, lns[1:]):
                x, h = blk.body(x, h, ln, is_training, route, cls_only and ln is lns[-1])
        return h[:, 0] if cls_only and not blocks else h


def patch_tokens(pe: nn.Module, inputs: torch.Tensor, patch_shape: Tuple[int, int], dtype: torch.dtype,
                 layout: str = "NHWC") -> torch.Tensor:
    """``PatchEmbedBlock_0`` (patch_embed.py:15-26) of ``inputs`` in the model call layout
    "NHWC" [B, H, W, C] or the train-step feed "HWCN" [H, W, C, B] (train.py:80): in bf16 one
    fused patch-gather GEMM (``ops.patch_embed``); otherwise (fp32 compute, shapes the kernel
    does not take) the einops rearrange and a Dense."""
    w = pe.Dense_0.kernel
    if dtype == torch.bfloat16 and ops.patch_embed_ok(inputs, w, patch_shape, layout):
        return ops.patch_embed(inputs, w, pe.Dense_0.bias, patch_shape, layout)
    if layout == "HWCN":
        inputs = inputs.permute(3, 0, 1, 2)                        # 'H W C N -> N H W C'
    b, H, W, c = inputs.shape
    ph, pw = patch_shape
    x = inputs.to(dtype).reshape(b, H // ph, ph, W // pw, pw, c).permute(0, 1, 3, 2, 4, 5)
    x = x.reshape(b, (H // ph) * (W // pw), ph * pw * c)          # 'b (h ph) (w pw) c -> b (h w) (ph pw c)'
    return pe.Dense_0(x, dtype)


class ViT(nn.Module):
    """vit.py:61-99.  ``forward(inputs [B, H, W, 3], is_training)`` -> logits [B, classes]."""

    def __init__(self, num_classes: int, num_layers: int, num_heads: int, embed_dim: int,
                 patch_shape: Tuple[int, int], img_size: int = 224, expand_ratio: float = 4,
                 dtype: torch.dtype = torch.float32, device=None, attn_dropout_rate: float = 0.0,
                 dropout_rate: float = 0.0):
        super().__init__()
        assert embed_dim % num_heads == 0
        self.patch_shape, self.dtype, self.embed_dim = tuple(patch_shape), dtype, embed_dim
        self.dropout_rate = dropout_rate
        ph, pw = self.patch_shape
        self.PatchEmbedBlock_0 = nn.Module()
        self.PatchEmbedBlock_0.Dense_0 = Dense(ph * pw * 3, embed_dim, use_bias=False, device=device)
        self.cls = nn.Parameter(torch.zeros(1, 1, embed_dim, device=device))
        n = (img_size // ph) * (img_size // pw) + 1
        self.Encoder_0 = Encoder(n, embed_dim, num_layers, num_heads, expand_ratio, dtype, device, attn_dropout_rate,
                                 dropout_rate)
        self.Dense_0 = Dense(embed_dim, num_classes, zero_init=True, device=device)

    def cast_groups(self):
        """Every Dense kernel the bf16 forward reads as a bf16 copy (the encoder's column-block
        groups, the patch embedding, the head): the optimizer may keep these copies
        (FusedAdamW ``cast_groups``).  None when the model computes in fp32."""
        if self.dtype != torch.bfloat16:
            return None
        return (encoder_weight_groups(numbered(self.Encoder_0, "EncoderBlock")) +
                [[self.PatchEmbedBlock_0.Dense_0.kernel]] + [[self.Dense_0.kernel]])

    def forward(self, inputs: torch.Tensor, is_training: bool, layout: str = "NHWC") -> torch.Tensor:
        """``layout`` "HWCN": ``inputs`` is the train-step feed [H, W, C, B] (train.py:80)."""
        x = patch_tokens(self.PatchEmbedBlock_0, inputs, self.patch_shape, self.dtype, layout)
        b = x.shape[0]
        pos = self.Encoder_0.AddAbsPosEmbed_0.pos_embed
        if self.dtype == torch.bfloat16 and ops.encoder_tokens_ok(x, self.cls, pos):
            # concat(cls, tokens) + pos_embed (and the input dropout) into the fp32 residual stream in one pass
            drop = hidden_dropout(self.dropout_rate, is_training, x.device)
            x = self.Encoder_0(ops.encoder_tokens(x, self.cls, pos, dropout=drop), is_training, pos_added=True,
                               cls_only=True)
        else:
            x = torch.cat([self.cls.expand(b, 1, self.embed_dim), x.float()], dim=1)   # fp32 (promotion)
            x = self.Encoder_0(x, is_training, cls_only=True)
        return self.Dense_0(x, self.dtype)   # the class token (vit.py:95-98)


# name -> (layers, heads, embed_dim, patch); create_model.py:10-37 plus the DeiT entries (survey D10)
MODEL_CONFIGS = {
    "vit_b_patch32": (12, 12, 768, 32),
    "vit_b_patch16": (12, 12, 768, 16),
    "vit_l_patch32": (24, 16, 1024, 32),
    "vit_l_patch16": (24, 16, 1024, 16),
    "deit_ti_patch16": (12, 3, 192, 16),
    "deit_s_patch16": (12, 6, 384, 16),
}


def create_model(model_name: str, num_classes: int = 1000, dtype: torch.dtype = torch.float32,
                 img_size: int = 224, device=None, attn_dropout_rate: float = 0.0, dropout_rate: float = 0.0) -> ViT:
    """``create_model`` (models/create_model.py:6-215) for the ViT/DeiT family."""
    if model_name not in MODEL_CONFIGS:
        raise ValueError(f"unknown model {model_name!r}; ViT/DeiT family: {sorted(MODEL_CONFIGS)}")
    L, Hh, C, p = MODEL_CONFIGS[model_name]
    return ViT(num_classes=num_classes, num_layers=L, num_heads=Hh, embed_dim=C, patch_shape=(p, p),
               img_size=img_size, dtype=dtype, device=device, attn_dropout_rate=attn_dropout_rate,
               dropout_rate=dropout_rate)


def vit_flops_per_image(model_name: str, img_size: int = 224, num_classes: int = 1000) -> float:
    """Forward FLOPs per image (2 per MAC): patch GEMM + per layer 4 projections, QK^T, AV and
    the MLP + head.  Training = 3x."""
    L, Hh, C, p = MODEL_CONFIGS[model_name]
    n = (img_size // p) ** 2 + 1
    per_layer = 2 * n * C * 3 * C + 2 * n * n * C * 2 + 2 * n * C * C + 2 * n * C * 4 * C * 2
    return float(2 * (n - 1) * p * p * 3 * C + L * per_layer + 2 * C * num_classes)
