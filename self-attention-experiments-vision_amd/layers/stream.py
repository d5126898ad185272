"""The fp32 residual stream of every model here: its LayerNorm and its residual add, each on two routes,
and the one place that chooses between them.  HIP route: the LayerNorm kernels (``ops.layer_norm*``,
``ops.add_layer_norm*``, ``ops.cls_add_layer_norm``: the add, the addend's dropout or scale and the LayerNorm
in one HBM pass).  Framework route: the same operations as framework ops, for an fp32 compute dtype and every
stream ``ops.layer_norm_ok`` refuses.  ``fused`` decides; the stream's owner passes the value down as ``route``."""
import torch

from .. import ops


def fused(x: torch.Tensor, dtype: torch.dtype) -> bool:
    """The route of the stream ``x`` under the compute dtype: True for the HIP kernels."""
    return dtype == torch.bfloat16 and ops.layer_norm_ok(x)


def hidden_dropout(rate: float, is_training: bool, device):
    """``(rate, DropoutRng)`` for the ops' ``dropout=`` argument, or None (inference, rate 0)."""
    return (rate, ops.dropout_rng(device)) if is_training and rate > 0.0 else None


def scaled(delta, layerscale, rowscale, dtype):
    """``delta * layerscale[c] * rowscale[b]`` in ``dtype`` as ONE elementwise pass, the [B, 1, C] factor first."""
    f = layerscale.to(dtype)
    if rowscale is not None:
        f = f[None, None, :] * rowscale[:, None, None].to(dtype)
    return delta.to(dtype) * f


def norm(x, ln, dtype, route: bool):
    """``ln`` (a ``vit.LayerNorm``) of the stream, in ``dtype``."""
    return ops.layer_norm(x, ln.scale, ln.bias) if route else ln(x, dtype)


def norm_pass(x, ln, dtype, route: bool):
    """``(x, ln(x))``: on the HIP route the stream's gradient is added inside the LayerNorm backward kernel."""
    return ops.layer_norm_pass(x, ln.scale, ln.bias) if route else (x, ln(x, dtype))


def add_norm(x, delta, ln, dtype, route: bool, *, dropout=None, layerscale=None, rowscale=None, cls_only=False):
    """``(x', ln(x'))`` with ``x' = x + delta``, the addend under ``dropout = (rate, DropoutRng)`` (one stream id
    drawn here) or times ``layerscale`` and ``rowscale`` [B] or None (``scaled``).  ``ln=None``: no LayerNorm
    follows, so only the add runs, as framework ops on either route: ``(x', None)``.  ``cls_only``: ``(None,
    ln(x')[:, 0])``; the HIP route adds and normalises the token-0 rows alone, the framework route every row."""
    assert layerscale is None or (dropout is None and not cls_only), "the scaled form has no dropout / class-row form"
    if route and ln is not None:
        if layerscale is not None:
            return ops.add_layer_norm_scaled(x, delta, ln.scale, ln.bias, layerscale, rowscale)
        if cls_only:
            return None, ops.cls_add_layer_norm(x, delta, ln.scale, ln.bias, dropout=dropout)
        return ops.add_layer_norm(x, delta, ln.scale, ln.bias, dropout=dropout)
    if layerscale is not None:
        delta = scaled(delta, layerscale, rowscale, dtype)
    x = x + ops.dropout_rows(delta, dropout)            # fp32: the stream promotes the addend
    h = None if ln is None else ln(x, dtype)
    return (None, h[:, 0]) if cls_only else (x, h)
