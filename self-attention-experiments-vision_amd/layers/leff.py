"""CeiT locally-enhanced feed-forward (models/layers/feedforwards/leff.py:9-63), MI355X path.

``LeFFBlock`` keeps the reference's fields, call signature ``(inputs [b, 1 + l, c], is_training)`` and
param tree (``Dense_0``, ``BatchNorm_0``, ``Conv_0``, ``BatchNorm_1``, ``Dense_1``, ``BatchNorm_2``; the
BatchNorm ``mean`` / ``var`` are buffers, Flax ``batch_stats``).  The class token passes through; the
l = S * S patch tokens go Dense -> BatchNorm -> GELU -> k x k convolution on the S x S grid ->
BatchNorm -> GELU -> Dense -> BatchNorm -> GELU.

HIP route: the two Dense layers are ``ops.dense``, the convolution (a full one, bias included) is
``ops.conv_tokens`` at stride 1, and each BatchNorm + GELU is one ``ops.bn_gelu`` (csrc/bn_rows.h).
No tensor is copied only to split off or re-attach the class token: ``Dense_0`` runs on all
b (1 + l) contiguous rows (one wasted row per sample), ``BatchNorm_0`` skips the class row of its
input (``x_lead = 1``), and ``BatchNorm_2`` writes the concatenated output, its row 0 read from
``inputs[:, :1]`` in place (``y_lead = 1``).  Calls the predicates refuse -- channel counts that are no
multiple of 8, k > 7, evaluation with a gradient wanted, an ``activation_fn`` other than the tanh-GELU
-- keep the framework route, ``LeFFBlock._framework_forward``.  Both routes return the compute dtype.
"""
from __future__ import annotations

import math
import types
from typing import Callable, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .attention import DenseGeneral
from .cvt import _BatchNorm, _Conv

__all__ = ["LeFFBlock"]


class LeFFBlock(nn.Module):
    """``LeFFBlock`` (leff.py:9-63).  ``activation_fn=None`` is the reference's default, Flax
    ``nn.gelu`` (the tanh form)."""

    def __init__(self, expand_ratio: Optional[float] = None, hidden_ch: Optional[int] = None, kernel_size: int = 5,
                 activation_fn: Optional[Callable] = None, bn_momentum: float = 0.9, bn_epsilon: float = 1e-5,
                 dtype: torch.dtype = torch.float32, *, in_ch: Optional[int] = None, device=None):
        super().__init__()
        if expand_ratio is None and hidden_ch is None:
            raise ValueError("Must provide one of expand_ratio or hidden_ch")
        self.expand_ratio, self.hidden_ch, self.kernel_size = expand_ratio, hidden_ch, kernel_size
        self.activation_fn = activation_fn
        self.bn_momentum, self.bn_epsilon, self.dtype = bn_momentum, bn_epsilon, dtype
        self._in_ch = None
        if in_ch is not None:
            self._build(in_ch, device)

    def _build(self, in_ch, device=None):
        hidden = self.hidden_ch if self.expand_ratio is None else max(1, int(self.expand_ratio * in_ch))
        self._in_ch, self._hidden = in_ch, hidden
        bn = lambda ch: _BatchNorm(ch, self.bn_momentum, self.bn_epsilon, device)
        self.Dense_0 = DenseGeneral((in_ch,), (hidden,), True, device)
        self.BatchNorm_0 = bn(hidden)
        self.Conv_0 = _Conv(self.kernel_size, hidden, hidden, True, device)
        self.BatchNorm_1 = bn(hidden)
        self.Dense_1 = DenseGeneral((hidden,), (in_ch,), True, device)
        self.BatchNorm_2 = bn(in_ch)

    def _hip_ok(self, inputs, is_training) -> bool:
        """Every predicate of the HIP route, from shapes alone (no tensor of the hidden width exists yet)."""
        if self.activation_fn is not None:
            return False
        B, R, C = inputs.shape
        hid, k, dt = self._hidden, self.kernel_size, self.dtype
        wants_grad = torch.is_grad_enabled() and (inputs.requires_grad or any(p.requires_grad for p in self.parameters()))
        rows = lambda ch: types.SimpleNamespace(is_cuda=inputs.is_cuda, shape=(B, R, ch))
        if not (ops.bn_gelu_ok(rows(hid), dt, is_training, wants_grad, x_lead=1)
                and ops.bn_gelu_ok(rows(C), dt, is_training, wants_grad, x_lead=1)):
            return False
        # ops.conv_tokens_ok for the [B, S, S, hidden] view of BatchNorm_0's (contiguous) output
        return 1 <= k <= 7 and hid % 8 == 0 and B * (R - 1) * ops.conv_window_cols(hid, k) < 2 ** 31

    def forward(self, inputs, is_training: bool):
        assert inputs.ndim == 3
        B, R, C = inputs.shape
        L = R - 1
        S = math.isqrt(max(L, 0))
        if L < 1 or S * S != L:
            raise ValueError(f"LeFFBlock: {L} patch tokens (after the class token) are no square grid")
        if self._in_ch is None:
            self._build(C, inputs.device)
        if not self._hip_ok(inputs, is_training):
            return self._framework_forward(inputs, is_training)
        dt, k, hid = self.dtype, self.kernel_size, self._hidden
        bn0, bn1, bn2 = self.BatchNorm_0, self.BatchNorm_1, self.BatchNorm_2
        x = inputs.to(dt)
        h = ops.dense(x, self.Dense_0.kernel, self.Dense_0.bias, dt)                 # [B, 1 + L, hidden]: class rows too
        h = ops.bn_gelu(h, bn0.scale, bn0.bias, bn0.mean, bn0.var, bn0.momentum, bn0.eps, is_training, dt, x_lead=1)
        h = ops.conv_tokens(h.view(B, S, S, hid), self.Conv_0.kernel, self.Conv_0.bias, k, 1, dt)   # [B, L, hidden]
        h = ops.bn_gelu(h, bn1.scale, bn1.bias, bn1.mean, bn1.var, bn1.momentum, bn1.eps, is_training, dt)
        h = ops.dense(h, self.Dense_1.kernel, self.Dense_1.bias, dt)                 # [B, L, C]
        return ops.bn_gelu(h, bn2.scale, bn2.bias, bn2.mean, bn2.var, bn2.momentum, bn2.eps, is_training, dt,
                           y_lead=1, lead=x[:, :1])

    def _framework_conv(self, h):
        """The convolution as ``F.conv2d`` on explicitly SAME-padded input, [B, S, S, hidden] ->
        [B, S, S, hidden] in dtype, rounding where ``ops.conv_tokens`` rounds (as
        ``ConvTokenEmbedBlock._framework_conv``): operands at the compute dtype, products and sums in
        fp32, the fp32 bias added, the output rounded once."""
        k, dt = self.kernel_size, self.dtype
        (pt, pb), (pl, pr) = ops.same_pads(h.shape[1], k, 1), ops.same_pads(h.shape[2], k, 1)
        hp = F.pad(h.to(dt).float().permute(0, 3, 1, 2), (pl, pr, pt, pb))           # NCHW
        w = self.Conv_0.kernel.to(dt).float().permute(3, 2, 0, 1)                    # [out, in, k, k]
        return F.conv2d(hp, w, self.Conv_0.bias.float()).permute(0, 2, 3, 1).to(dt)

    def _framework_forward(self, inputs, is_training: bool):
        """The same block as framework ops: every call the predicates refuse, and the A/B partner."""
        dt = self.dtype
        act = self.activation_fn if self.activation_fn is not None else (lambda t: F.gelu(t, approximate="tanh"))
        x = inputs.to(dt)
        cls, tokens = x[:, :1], x[:, 1:]
        B, L, C = tokens.shape
        S = math.isqrt(L)
        h = ops.dense(tokens, self.Dense_0.kernel, self.Dense_0.bias, dt)            # [B, L, hidden]
        h = act(self.BatchNorm_0(h.view(B, S, S, -1), is_training))
        h = act(self.BatchNorm_1(self._framework_conv(h), is_training))
        h = ops.dense(h.reshape(B, L, -1), self.Dense_1.kernel, self.Dense_1.bias, dt)
        h = act(self.BatchNorm_2(h.view(B, S, S, C), is_training)).view(B, L, C)
        return torch.cat([cls, h], dim=1)
