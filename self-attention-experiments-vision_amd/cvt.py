"""CvT -- the model around ``layers.CvTSelfAttentionBlock`` (models/cvt.py:10-171): three stages, each
a convolutional token embedding (``ConvTokenEmbedBlock``: a k x k convolution with stride s < k and
Flax SAME padding, then LayerNorm; 7/4, 3/2, 3/2) followed by ``StageBlock`` s, and a Dense head on
the class token.

Class names, fields, call signatures and the Flax parameter tree are the reference's:
``Stage_i/ConvTokenEmbedBlock_0/{Conv_0/{kernel, bias}, LayerNorm_0/{scale, bias}}``,
``Stage_i/StageBlock_j/{CvTSelfAttentionBlock_0/..., LayerNorm_0, FFBlock_0/Dense_{0,1}}``,
``Stage_{last}/cls``, ``Dense_0``; the BatchNorm ``mean`` / ``var`` of the convolutional projections are
buffers (Flax ``batch_stats``).

The stem's convolution is ``ops.conv_tokens`` (the window matrix written once by ``sae_conv_window_gather``, then the
project's GEMMs; the input gradient through ``sae_conv_window_scatter``, for stages 2 and 3 only: the image batch
takes none); calls outside ``ops.conv_tokens_ok`` keep the framework route,
``ConvTokenEmbedBlock._framework_forward``.  A stage block is ``zero_pad_and_reshape`` -> ``CvTSelfAttentionBlock``
-> residual add + LayerNorm -> ``ops.ff_block`` -> residual add.  The stem and each stage block decide the route of
their LayerNorm per call, on their own stream (``layers/stream.py``): ``ops.layer_norm`` and one
``ops.add_layer_norm`` kernel on the HIP route, framework ops on the other.
Numerics follow the other models here: fp32 parameters, ``dtype`` compute, fp32 residual stream.

Behaviour of the reference that is kept as it is:
  * The last stage inserts the class token BEFORE its blocks, and every block starts with
    ``zero_pad_and_reshape``: at 224 px its 14 x 14 + 1 = 197 tokens are zero-padded to a 15 x 15 grid
    and the residual is taken against the PADDED input, so the sequence is 225 tokens from that
    stage's first block on.  The class token sits at grid position (0, 0), the image tokens are
    shifted by one, and the 28 pad rows are ordinary tokens afterwards.  Keys and values are 8 x 8.
  * There is no final LayerNorm; the head is a zero-initialised Dense on ``x[:, 0]``.
  * create_model.py:169-178 gives cvt-13 / cvt-21 ``embed_dim = (64, 192, 368)`` with 6 heads in the
    last stage; 368 % 6 != 0, which the reference's own assertion (cvt_attention.py:65) refuses, so
    those two names cannot be built there.  Its cvt_test.py uses (64, 192, 384), the CvT paper's
    widths; ``CVT_CONFIGS`` takes that value.  ``CvT(...)`` with channels not divisible by heads raises.

Out of scope: a gather from the HWCN train-step feed (``layout="HWCN"`` rearranges with a framework
permute), ``cast_groups`` (the optimizer keeps no bf16 weight copies for this model: they are cast
per forward) and hidden-state dropout (the reference's CvT has none).
"""
from __future__ import annotations

import math
from typing import Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .layers.attention import numbered
from .layers.cvt import CvTSelfAttentionBlock, _Conv
from .layers.stream import add_norm, fused, norm
from .vit import Dense, FFBlock, LayerNorm

__all__ = ["zero_pad_and_reshape", "ConvTokenEmbedBlock", "StageBlock", "Stage", "CvT", "create_cvt",
           "CVT_CONFIGS", "cvt_flops_per_image", "cvt_token_counts"]


def _grid_side(l: int) -> int:
    """ceil(sqrt(l)) in integers."""
    s = math.isqrt(l)
    return s if s * s == l else s + 1


def zero_pad_and_reshape(inputs: torch.Tensor) -> torch.Tensor:
    """cvt.py:10-16: [b, l, c] -> [b, S, S, c] with S = ceil(sqrt(l)), zero rows appended."""
    assert inputs.ndim == 3
    b, l, c = inputs.shape
    S = _grid_side(l)
    if S * S != l:
        inputs = F.pad(inputs, (0, 0, 0, S * S - l))
    return inputs.reshape(b, S, S, c)


class ConvTokenEmbedBlock(nn.Module):
    """cvt.py:19-35: Conv(out_ch, k x k, strides, SAME) -> 'b H W c -> b (H W) c' -> LayerNorm."""

    def __init__(self, out_ch: int, kernel_size: int, strides: int, dtype: torch.dtype = torch.float32, *,
                 in_ch: int, device=None):
        super().__init__()
        self.out_ch, self.kernel_size, self.strides, self.dtype = out_ch, kernel_size, strides, dtype
        self.Conv_0 = _Conv(kernel_size, in_ch, out_ch, True, device)
        self.LayerNorm_0 = LayerNorm(out_ch, device)

    def forward(self, inputs: torch.Tensor, **unused_kwargs) -> torch.Tensor:   # [b, H, W, c] -> [b, Ho Wo, out]
        assert inputs.ndim == 4
        k, s, dt = self.kernel_size, self.strides, self.dtype
        if not ops.conv_tokens_ok(inputs, self.Conv_0.kernel, k, s, dt):
            return self._framework_forward(inputs)
        y = ops.conv_tokens(inputs, self.Conv_0.kernel, self.Conv_0.bias, k, s, dt).float()
        return norm(y, self.LayerNorm_0, dt, fused(y, dt))

    def _framework_conv(self, inputs: torch.Tensor) -> torch.Tensor:
        """The convolution as ``F.conv2d`` on explicitly SAME-padded input -> [b, Ho Wo, out] in dtype.
        It rounds where the kernels round, as ``ConvProjectionBlock._framework_forward`` does: input and
        kernel cast to the compute dtype first (as Flax's Conv does), products and sums in fp32, the fp32
        bias added, the output rounded once.  (The library's bf16 convolution is 3e-3 .. 6e-3 from the
        float64 result, more than half a bf16 ulp; tests/test_gpu_conv_tokens.py measured it.)"""
        k, s, dt = self.kernel_size, self.strides, self.dtype
        (pt, pb), (pl, pr) = ops.same_pads(inputs.shape[1], k, s), ops.same_pads(inputs.shape[2], k, s)
        xp = F.pad(inputs.to(dt).float().permute(0, 3, 1, 2), (pl, pr, pt, pb))  # NCHW
        w = self.Conv_0.kernel.to(dt).float().permute(3, 2, 0, 1)                 # [out, in, k, k]
        y = F.conv2d(xp, w, self.Conv_0.bias.float(), stride=s).permute(0, 2, 3, 1)
        return y.reshape(y.shape[0], -1, self.out_ch).to(dt)

    def _framework_forward(self, inputs: torch.Tensor, **unused_kwargs) -> torch.Tensor:
        """The same stem as framework ops: every call ``ops.conv_tokens_ok`` refuses."""
        return self.LayerNorm_0(self._framework_conv(inputs), self.dtype)


class StageBlock(nn.Module):
    """cvt.py:38-68.  ``inputs`` [b, l, c] is the fp32 residual stream; the output has S * S tokens,
    S = ceil(sqrt(l)) (the residual is taken against the zero-padded input)."""

    def __init__(self, num_heads: int, embed_dim: int, kernel_size: int = 3, use_bias: bool = False,
                 bn_momentum: float = 0.9, bn_epsilon: float = 1e-5, expand_ratio: float = 4,
                 dtype: torch.dtype = torch.float32, device=None):
        super().__init__()
        self.dtype = dtype
        self.CvTSelfAttentionBlock_0 = CvTSelfAttentionBlock(
            num_heads=num_heads, kernel_size=kernel_size, use_bias=use_bias, bn_momentum=bn_momentum,
            bn_epsilon=bn_epsilon, dtype=dtype, in_ch=embed_dim, device=device)
        self.LayerNorm_0 = LayerNorm(embed_dim, device)
        self.FFBlock_0 = FFBlock(embed_dim, expand_ratio, device)

    def forward(self, inputs: torch.Tensor, is_training: bool) -> torch.Tensor:
        grid = zero_pad_and_reshape(inputs)
        a = self.CvTSelfAttentionBlock_0(grid, is_training=is_training)
        res = grid.reshape(grid.shape[0], -1, grid.shape[3])
        route = fused(res, self.dtype)
        x, y = add_norm(res, a, self.LayerNorm_0, self.dtype, route)
        return add_norm(x, self.FFBlock_0(y, self.dtype, is_training), None, self.dtype, route)[0]


class Stage(nn.Module):
    """cvt.py:71-113: token embedding, the class token in front (``insert_cls``), ``size`` blocks."""

    def __init__(self, size: int, num_heads: int, embed_dim: int, embed_kernel_size: int, embed_strides: int,
                 sa_kernel_size: int = 3, use_bias: bool = False, bn_momentum: float = 0.9, bn_epsilon: float = 1e-5,
                 expand_ratio: float = 4, insert_cls: bool = False, dtype: torch.dtype = torch.float32, *,
                 in_ch: int, device=None):
        super().__init__()
        self.size, self.embed_dim, self.insert_cls = size, embed_dim, insert_cls
        self.ConvTokenEmbedBlock_0 = ConvTokenEmbedBlock(embed_dim, embed_kernel_size, embed_strides, dtype,
                                                         in_ch=in_ch, device=device)
        if insert_cls:
            self.cls = nn.Parameter(torch.zeros(1, 1, embed_dim, device=device))
        for i in range(size):
            setattr(self, f"StageBlock_{i}", StageBlock(num_heads, embed_dim, sa_kernel_size, use_bias, bn_momentum,
                                                        bn_epsilon, expand_ratio, dtype, device))

    def forward(self, inputs: torch.Tensor, is_training: bool) -> torch.Tensor:
        x = self.ConvTokenEmbedBlock_0(inputs, is_training=is_training).float()   # the fp32 residual stream
        if self.insert_cls:
            x = torch.cat([self.cls.expand(x.shape[0], 1, self.embed_dim), x], dim=1)
        for blk in numbered(self, "StageBlock"):
            x = blk(x, is_training=is_training)
        return x


class CvT(nn.Module):
    """cvt.py:116-171.  ``forward(inputs [B, H, W, in_ch], is_training)`` -> logits [B, classes]."""

    def __init__(self, num_classes: int, stage_sizes: Tuple[int, ...], num_heads: Tuple[int, ...],
                 embed_dim: Tuple[int, ...], embed_kernel_size: Tuple[int, ...] = (7, 3, 3),
                 embed_strides: Tuple[int, ...] = (4, 2, 2), sa_kernel_size: Tuple[int, ...] = (3, 3, 3),
                 use_bias: bool = False, expand_ratio: float = 4, bn_momentum: float = 0.9, bn_epsilon: float = 1e-5,
                 dtype: torch.dtype = torch.float32, *, in_ch: int = 3, device=None):
        super().__init__()
        n = len(stage_sizes)
        if not all(len(t) == n for t in (num_heads, embed_dim, embed_kernel_size, embed_strides, sa_kernel_size)):
            raise ValueError("CvT: every per-stage tuple needs one entry per stage")
        for c, h in zip(embed_dim, num_heads):
            if c % h:   # the reference's assertion, cvt_attention.py:65
                raise ValueError(f"CvT: embed_dim {c} is not divisible by num_heads {h}")
        self.stage_sizes, self.dtype = tuple(stage_sizes), dtype
        for i in range(n):
            setattr(self, f"Stage_{i}", Stage(
                stage_sizes[i], num_heads[i], embed_dim[i], embed_kernel_size[i], embed_strides[i], sa_kernel_size[i],
                use_bias, bn_momentum, bn_epsilon, expand_ratio, insert_cls=i == n - 1, dtype=dtype,
                in_ch=in_ch if i == 0 else embed_dim[i - 1], device=device))
        self.Dense_0 = Dense(embed_dim[-1], num_classes, zero_init=True, device=device)

    def forward(self, inputs: torch.Tensor, is_training: bool, layout: str = "NHWC") -> torch.Tensor:
        """``layout`` "HWCN": ``inputs`` is the train-step feed [H, W, C, B], rearranged here."""
        if layout == "HWCN":
            inputs = inputs.permute(3, 0, 1, 2).contiguous()
        elif layout != "NHWC":
            raise ValueError(f"CvT: layout must be 'NHWC' or 'HWCN', got {layout!r}")
        *stages, last = numbered(self, "Stage")
        x = inputs
        for stage in stages:
            x = stage(x, is_training=is_training)
            b, l, c = x.shape
            S = math.isqrt(l)                     # 'b (H W) c -> b H W c', H = int(sqrt(l))
            x = x.reshape(b, S, l // S, c)
        x = last(x, is_training=is_training)
        return self.Dense_0(x[:, 0].contiguous(), self.dtype)


# name -> (stage_sizes, num_heads, embed_dim); create_model.py:169-183, with the last width of cvt-13 /
# cvt-21 taken from the reference's cvt_test.py (384: see the module docstring)
CVT_CONFIGS = {
    "cvt-13": ((1, 2, 10), (1, 3, 6), (64, 192, 384)),
    "cvt-21": ((1, 4, 16), (1, 3, 6), (64, 192, 384)),
    "cvt-w24": ((2, 2, 20), (3, 12, 16), (192, 768, 1024)),
}


def create_cvt(model_name: str, num_classes: int = 1000, dtype: torch.dtype = torch.float32, device=None) -> CvT:
    """``create_model`` (models/create_model.py:169-183) for the CvT family."""
    if model_name not in CVT_CONFIGS:
        raise ValueError(f"unknown model {model_name!r}; CvT family: {sorted(CVT_CONFIGS)}")
    sizes, heads, dims = CVT_CONFIGS[model_name]
    return CvT(num_classes=num_classes, stage_sizes=sizes, num_heads=heads, embed_dim=dims, dtype=dtype, device=device)


def cvt_token_counts(img_size: int = 224, embed_strides=(4, 2, 2), sa_strides=(1, 2, 2)):
    """Per stage ``(query tokens, key / value tokens)`` of its blocks: the SAME-strided grid (plus the
    class token, zero-padded to a square, in the last stage) and its stride-2 projection."""
    out, side = [], img_size
    for i, s in enumerate(embed_strides):
        side = -(-side // s)
        g = side if i + 1 < len(embed_strides) else _grid_side(side * side + 1)
        out.append((g * g, (-(-g // sa_strides[1])) ** 2))
    return tuple(out)


def cvt_flops_per_image(model_name: str, img_size: int = 224, num_classes: int = 1000) -> float:
    """Forward FLOPs per image (2 per MAC): per stage the embedding convolution, and per block the
    three depthwise 3x3 + 1x1 projections (queries on the full grid, keys / values on the strided
    one), QK^T, AV, the output projection and the MLP; head.  Training = 3x."""
    sizes, _, dims = CVT_CONFIGS[model_name]
    counts = cvt_token_counts(img_size)
    ks, total, cin, side = (7, 3, 3), 0.0, 3, img_size
    for i, (C, (nq, nk)) in enumerate(zip(dims, counts)):
        side = -(-side // (4, 2, 2)[i])
        total += 2 * side * side * ks[i] * ks[i] * cin * C
        proj = 2 * 9 * C * (nq + 2 * nk) + 2 * C * C * (nq + 2 * nk)
        blk = proj + 2 * nq * nk * C * 2 + 2 * nq * C * C + 2 * nq * C * 4 * C * 2
        total += sizes[i] * blk
        cin = C
    return float(total + 2 * dims[-1] * num_classes)
