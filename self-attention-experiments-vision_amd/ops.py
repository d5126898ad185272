"""Autograd operators over the C ABI (include/sae_attn.h).

Each ``torch.autograd.Function`` below is a thin host-side shim: it allocates outputs with
the framework's caching allocator, fills an ``sae_attn_desc`` with the tensors' element
strides, and calls the HIP library on the current stream.  Forward saves the log-sum-exp
rows, never the [B, H, Nq, Nk] probabilities (the reference materialises them:
models/layers/attentions/attention.py:41-58).  There is one Function per kernel family:
``_Attention`` and ``_TalkingHeads`` take q, k, v or one packed projection, ``_LayerNorm`` serves
every residual add + LayerNorm form; the public functions select its mode and outputs.

The public functions are the names in ``__all__``; each one's docstring cites the reference lines it
restates.  A Dense projection's routes are planned by ``dense_fwd_plan`` / ``dense_bwd_plan``.
"""
from __future__ import annotations

import contextlib
import ctypes
import dataclasses
import functools
import math
import os
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib as L

__all__ = ["attention", "attention_packed", "dense", "ff_block", "gemm_nt", "weight_cast", "forward_casts",
           "clear_weight_cache", "gemm_dw", "layer_norm", "add_layer_norm", "dropout_rows", "dropout_rows_mask",
           "add_layer_norm_scaled", "layer_norm_ok", "talking_heads_attention", "talking_heads_attention_packed",
           "relpos_bias", "rotary", "rotary_tables", "dtype_code", "KernelTimer", "set_kernel_timer",
           "DenseFacts", "dense_facts_of_shapes", "dense_fwd_plan", "dense_bwd_plan",
           "dwconv_bn", "dwconv_bn_ok", "same_pads", "conv_tokens", "conv_tokens_ok", "conv_window_matrix",
           "conv_window_scatter", "conv_window_cols", "bn_gelu", "bn_gelu_ok"]


class KernelTimer:
    """Brackets every C-ABI launch group with HIP events on the launch stream (used by
    bench.py to time the fused kernels inside the timed region of a training step)."""

    def __init__(self):
        self.events = {}

    def begin(self, name):
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.current_stream())
        return name, e0

    def end(self, token, work=None):
        name, e0 = token
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record(torch.cuda.current_stream())
        self.events.setdefault(name, []).append((e0, e1, work))

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, lst in self.events.items():
            ms = [a.elapsed_time(b) for a, b, _ in lst]
            out[name] = {"launches": len(ms), "total_ms": sum(ms), "mean_ms": sum(ms) / max(1, len(ms)),
                         "work": [w for _, _, w in lst]}
        return out


_TIMER = None


# The GradSinks (sinks.py) whose backward() window is open, or None: the only training-step state
# held here.  Sinks, written set, listener and weight-gradient side stream belong to that object.
_ACTIVE_SINKS = None


def _sinking(bwd):
    """Backward of an op that may write gradient sinks (sinks.GradSinks): once its kernels are enqueued,
    the active GradSinks reports every sink it claimed to its listener (the training step launches a
    bucket's all-reduce once all of its gradients are written, beside the rest of the backward)."""
    @functools.wraps(bwd)
    def wrapped(ctx, *grads):
        sinks = _ACTIVE_SINKS
        if sinks is None:
            return bwd(ctx, *grads)
        n0 = len(sinks.claimed)
        out = bwd(ctx, *grads)
        if len(sinks.claimed) > n0:
            sinks.report(n0)
        return out
    return wrapped


def _sink(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """The sink of parameter ``t`` in the open window (GradSinks.lookup); None outside one."""
    return None if _ACTIVE_SINKS is None else _ACTIVE_SINKS.lookup(t)


def _claim(sink: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """Mark a sink as written by this backward (GradSinks.claim: at most once per window)."""
    if sink is not None and _ACTIVE_SINKS is None:
        raise RuntimeError("gradient sink claimed outside the GradSinks.backward() window its forward ran in")
    return sink if sink is None else _ACTIVE_SINKS.claim(sink)


def _unsunk(g, sink):
    """The gradient autograd should see: None when it went into a sink."""
    return None if sink is not None else g


def _grad_out(sink: Optional[torch.Tensor], shape, device) -> torch.Tensor:
    """Where a backward kernel writes an fp32 parameter gradient: the claimed sink, or a fresh buffer."""
    return _claim(sink) if sink is not None else torch.empty(shape, dtype=torch.float32, device=device)


def occupy_cus(stream, workgroups: int, usec: float, threads: int = 256, lds_bytes: int = 64 * 1024) -> None:
    """Diagnostic (``sae_occupy_cus``): ``workgroups`` workgroups that hold their CUs for ``usec``
    microseconds on ``stream`` -- the CU footprint of an RCCL all-reduce's ring channels, for the
    one-GPU contention emulation of the data-parallel step (bench.py --emulate-rccl)."""
    lib = L.load()
    L.check(lib.sae_occupy_cus(ctypes.c_void_p(stream.cuda_stream), int(workgroups), int(threads), int(lds_bytes),
                               float(usec)))


def flag_bump(flags: torch.Tensor, index: int) -> None:
    """flags[index] += 1 on the current stream (``sae_flag_bump``; flags int32 on the GPU): a mark in
    a captured kernel chain that another stream can wait for (``stream_wait_flag``)."""
    lib = L.load()
    _require_gpu(flags)
    L.check(lib.sae_flag_bump(_stream(flags), ctypes.c_void_p(flags.data_ptr()), int(index)))


def stream_wait_flag(stream, flags: torch.Tensor, index: int, value: int) -> None:
    """Make ``stream`` wait until flags[index] >= value (``sae_stream_wait_flag``)."""
    lib = L.load()
    _require_gpu(flags)
    L.check(lib.sae_stream_wait_flag(ctypes.c_void_p(stream.cuda_stream),
                                     ctypes.c_void_p(flags.data_ptr() + 4 * int(index)), int(value) & 0xffffffff))


def set_kernel_timer(t):
    global _TIMER
    _TIMER = t


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.bfloat16:
        return L.SAE_DTYPE_BF16
    if dt == torch.float32:
        return L.SAE_DTYPE_F32
    raise TypeError(f"sae_vision_amd kernels take bfloat16 or float32, got {dt}")


def _require_gpu(*ts: torch.Tensor):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("sae_vision_amd attention runs on the GPU only (HIP kernels); "
                               f"got a tensor on {t.device}")


def _bnh(t: torch.Tensor):
    if t.dim() != 4:
        raise ValueError(f"expected a [B, N, H, D] tensor, got shape {tuple(t.shape)}")
    if t.stride(3) != 1:
        raise ValueError("head_dim must be the innermost (stride-1) dimension")
    return (t.stride(0), t.stride(1), t.stride(2))


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _make_desc(q, k, v, o, scale, dout=None, dq=None, dk=None, dv=None, grid=None) -> L.SaeAttnDesc:
    lib = L.load()
    B, Nq, H, D = q.shape
    Nk = k.shape[1]
    if k.shape != (B, Nk, H, D) or v.shape != (B, Nk, H, D):
        raise ValueError(f"q {tuple(q.shape)} / k {tuple(k.shape)} / v {tuple(v.shape)} mismatch")
    if not (q.dtype == k.dtype == v.dtype):
        raise TypeError("q, k and v must share a dtype")
    d = L.SaeAttnDesc()
    lib.sae_attn_desc_init(ctypes.byref(d), B, H, Nq, Nk, D, dtype_code(q.dtype), float(scale))
    d.q_stride, d.k_stride, d.v_stride = L.s3(_bnh(q)), L.s3(_bnh(k)), L.s3(_bnh(v))
    if o is not None:
        d.o_stride = L.s3(_bnh(o))
    if dout is not None:
        d.do_stride, d.dq_stride = L.s3(_bnh(dout)), L.s3(_bnh(dq))
        d.dk_stride, d.dv_stride = L.s3(_bnh(dk)), L.s3(_bnh(dv))
    if grid is not None:
        d.flags = L.SAE_FLAG_RELPOS
        d.rel_h, d.rel_w = int(grid[0]), int(grid[1])
    return d


def _rope_tabs(q, k, rope):
    """(sin, cos) fp32 [max(Nq, Nk), D / 2] for the fused-rotary entry points (``rope`` = base)."""
    return rotary_tables(max(q.shape[1], k.shape[1]), q.shape[-1], q.device, rope)


def _rope_route(route: str, ts) -> bool:
    """Whether the C ABI's own plan (``sae_attn_route`` / ``sae_th_attn_route``, rotary form) takes
    the [B, N, H, D] tensors ``ts`` = (q[, k[, v]]); a missing k / v has the layout of the last one."""
    if ts[0].dtype not in (torch.bfloat16, torch.float32) or any(t.dim() != 4 or t.stride(3) != 1 for t in ts):
        return False   # nothing a descriptor can say
    q, k, v = (tuple(ts) + (ts[-1],) * 2)[:3]
    lib = L.load()
    d = L.SaeAttnDesc()
    lib.sae_attn_desc_init(ctypes.byref(d), q.shape[0], q.shape[2], q.shape[1], k.shape[1], q.shape[3],
                           dtype_code(q.dtype), 1.0)
    d.q_stride, d.k_stride, d.v_stride = L.s3(_bnh(q)), L.s3(_bnh(k)), L.s3(_bnh(v))
    aligned = all(t.data_ptr() % 16 == 0 for t in ts)
    return getattr(lib, route)(ctypes.byref(d), L.SAE_PASS_FWD, L.SAE_FORM_ROTARY, int(aligned)) is not None


def rope_fused_ok(*ts: torch.Tensor) -> bool:
    """Whether the fused-rotary kernels take these [B, N, H, D] tensors (sae_attn_*_rotary)."""
    return _rope_route("sae_attn_route", ts)


# ------------------------------------------------------------------- attention dropout state
class DropoutRng:
    """Device state of the attention-probability dropout (``sae_attn_fwd_dropout``): a 2-element
    int64 tensor carrying the bit patterns of ``{seed, offset}``.  The kernels read it on the
    device, so a captured step replays with fresh masks once :meth:`advance` has run on the stream.
    Every attention call of a step draws its own ``stream_id`` from :meth:`next_stream` (a host
    counter since the last advance); the backward of a call passes the id its forward drew."""

    def __init__(self, seed: int, device):
        self.device = torch.device(device)
        self.state = torch.zeros(2, dtype=torch.int64, device=self.device)
        self.seed(seed)

    def seed(self, seed: int, offset: int = 0) -> None:
        """Set ``{seed, offset}`` (64-bit patterns) and restart the call counter."""
        def i64(x):
            x = int(x) & 0xFFFFFFFFFFFFFFFF
            return x - (1 << 64) if x >= (1 << 63) else x
        self.state.copy_(torch.tensor([i64(seed), i64(offset)], dtype=torch.int64))
        self._calls = 0

    def next_stream(self) -> int:
        sid = self._calls
        self._calls += 1
        return sid

    def advance(self, n: int = 1) -> None:
        """``offset += n`` on the current stream (``sae_dropout_advance``); restarts the call counter."""
        lib = L.load()
        _require_gpu(self.state)
        L.check(lib.sae_dropout_advance(_stream(self.state), _ptr(self.state), int(n)))
        self._calls = 0


_DROPOUT_RNGS = {}


def dropout_rng(device) -> DropoutRng:
    """The default :class:`DropoutRng` of ``device`` (seed 0 until :func:`seed_dropout`)."""
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    r = _DROPOUT_RNGS.get(dev)
    if r is None:
        r = _DROPOUT_RNGS[dev] = DropoutRng(0, dev)
    return r


def seed_dropout(seed: int) -> None:
    """Seed the default dropout state of every device that has one, and of the current device."""
    if torch.cuda.is_available():
        dropout_rng("cuda")
    for r in _DROPOUT_RNGS.values():
        r.seed(seed)


def dropout_mask(B: int, H: int, Nq: int, Nk: int, rate: float, rng: DropoutRng, stream_id: int) -> torch.Tensor:
    """uint8 ``keep[B, H, Nq, Nk]`` exactly as the dropout attention kernels apply it
    (``sae_attn_dropout_mask``)."""
    lib = L.load()
    _require_gpu(rng.state)
    keep = torch.empty((B, H, Nq, Nk), dtype=torch.uint8, device=rng.state.device)
    L.check(lib.sae_attn_dropout_mask(_stream(keep), B, H, Nq, Nk, float(rate), _ptr(rng.state), int(stream_id),
                                      _ptr(keep)))
    return keep


def _draw(dropout):
    """``(rate, rng)`` of the public ops -> ``(rate, state tensor, stream_id)`` of one call."""
    if dropout is None:
        return None
    rate, rng = dropout
    if not 0.0 <= float(rate) < 1.0:
        raise ValueError(f"dropout rate {rate} is outside [0, 1)")
    return (float(rate), rng.state, rng.next_stream())


def _drop_args(drop):
    """The three C arguments (rate, state pointer, stream id) of a drawn dropout triple."""
    return drop[0], _ptr(drop[1]), drop[2]


# ------------------------------------------------------------------- hidden-state dropout
def dropout_rows_mask(M: int, C: int, rate: float, rng: DropoutRng, stream_id: int, row0: int = 0,
                      row_step: int = 1) -> torch.Tensor:
    """uint8 ``keep[M, C]`` of the hidden-state dropout (``sae_dropout_rows_mask``): what
    :func:`dropout_rows` and the ``dropout=`` forms of ``add_layer_norm``, ``cls_add_layer_norm``,
    ``encoder_tokens`` and ``ff_block`` apply for rows ``row0 + i * row_step``."""
    lib = L.load()
    _require_gpu(rng.state)
    keep = torch.empty((M, C), dtype=torch.uint8, device=rng.state.device)
    L.check(lib.sae_dropout_rows_mask(_stream(keep), M, C, float(rate), _ptr(rng.state), int(stream_id), int(row0),
                                      int(row_step), _ptr(keep)))
    return keep


def _dropout_rows_call(x2, y2, drop):
    lib = L.load()
    M, C = x2.shape
    L.check(lib.sae_dropout_rows(_stream(x2), M, C, dtype_code(x2.dtype), _ptr(x2), x2.stride(0), _ptr(y2),
                                 y2.stride(0), *_drop_args(drop), 0, 1))


class _DropoutRows(torch.autograd.Function):
    """y = x * keep / pk over the rows of x viewed as [M, C] (C = the last dimension); the backward
    is the same kernel on the gradient with the stream id the forward drew."""

    @staticmethod
    def forward(ctx, x, drop):
        x2 = x.reshape(-1, x.shape[-1])
        if x2.stride(1) != 1:
            x2 = x2.contiguous()
        y2 = torch.empty_like(x2, memory_format=torch.contiguous_format)
        _dropout_rows_call(x2, y2, drop)
        ctx.drop = drop
        return y2.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        d2 = dy.reshape(-1, dy.shape[-1])
        if d2.stride(1) != 1:
            d2 = d2.contiguous()
        dx = torch.empty_like(d2, memory_format=torch.contiguous_format)
        _dropout_rows_call(d2, dx, ctx.drop)
        return dx.view(dy.shape), None


def dropout_rows(x: torch.Tensor, dropout=None) -> torch.Tensor:
    """Hidden-state dropout ``x * keep / pk`` (``sae_dropout_rows``; bf16 or fp32) of ``x`` [.., C]
    viewed as rows x C, with ``dropout = (rate, DropoutRng)``; ``None`` returns ``x``.  One stream id
    is drawn per call.  The paths the fused ``dropout=`` forms do not take."""
    if dropout is None:
        return x
    _require_gpu(x)
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"dropout_rows: dtype {x.dtype} is not float32 / bfloat16")
    return _DropoutRows.apply(x, _draw(dropout))


# ---------------------------------------------------------------------------- attention core
def _fwd(q, k, v, scale, bias_h=None, bias_w=None, grid=None, rope=None, drop=None):
    lib = L.load()
    B, Nq, H, D = q.shape
    o = torch.empty((B, Nq, H, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
    d = _make_desc(q, k, v, o, scale, grid=grid)
    tok = _TIMER.begin("attn_fwd") if _TIMER is not None else None
    if rope is not None:   # q / k un-rotated: the kernels rotate them while staging
        sin, cos = _rope_tabs(q, k, rope)
        L.check(lib.sae_attn_fwd_rotary(_stream(q), ctypes.byref(d), _ptr(q), _ptr(k), _ptr(v), _ptr(sin),
                                        _ptr(cos), _ptr(o), _ptr(lse)))
    elif drop is not None:
        L.check(lib.sae_attn_fwd_dropout(_stream(q), ctypes.byref(d), _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(lse),
                                         *_drop_args(drop)))
    else:
        L.check(lib.sae_attn_fwd(_stream(q), ctypes.byref(d), _ptr(q), _ptr(k), _ptr(v), _ptr(bias_h),
                                 _ptr(bias_w), _ptr(o), _ptr(lse)))
    if tok is not None:
        _TIMER.end(tok, (B, Nq, k.shape[1], H, D))
    return o, lse


def _bwd(q, k, v, o, lse, do, dq, dk, dv, scale, bias_h=None, bias_w=None, grid=None, rope=None, drop=None):
    lib = L.load()
    d = _make_desc(q, k, v, o, scale, do, dq, dk, dv, grid=grid)
    ws = torch.empty(lib.sae_attn_bwd_workspace_bytes(ctypes.byref(d)), dtype=torch.uint8, device=q.device)
    dbh = dbw = None
    if grid is not None:
        dbh, dbw = torch.empty_like(bias_h), torch.empty_like(bias_w)
    tok = _TIMER.begin("attn_bwd") if _TIMER is not None else None
    if rope is not None:   # dq / dk for the un-rotated q / k
        sin, cos = _rope_tabs(q, k, rope)
        L.check(lib.sae_attn_bwd_rotary(_stream(q), ctypes.byref(d), _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(lse),
                                        _ptr(do), _ptr(sin), _ptr(cos), _ptr(dq), _ptr(dk), _ptr(dv), _ptr(ws)))
    elif drop is not None:
        L.check(lib.sae_attn_bwd_dropout(_stream(q), ctypes.byref(d), _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(lse),
                                         _ptr(do), _ptr(dq), _ptr(dk), _ptr(dv), _ptr(ws), *_drop_args(drop)))
    else:
        L.check(lib.sae_attn_bwd(_stream(q), ctypes.byref(d), _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(lse),
                                 _ptr(do), _ptr(bias_h), _ptr(bias_w), _ptr(dq), _ptr(dk), _ptr(dv), _ptr(dbh),
                                 _ptr(dbw), _ptr(ws)))
    if tok is not None:
        _TIMER.end(tok, tuple(q.shape[:2]) + (k.shape[1],) + tuple(q.shape[2:]))
    return dbh, dbw


def _grad_in(g: torch.Tensor) -> torch.Tensor:
    return g if g.stride(-1) == 1 else g.contiguous()


def _split(q, k, v):
    """(q, k, v) of a call: three tensors, or -- ``k`` and ``v`` None -- the three views of ``q``, a
    packed projection [B, N, 3, H, D]."""
    return (q[:, :, 0], q[:, :, 1], q[:, :, 2]) if k is None else (q, k, v)


def _qkv_grads(q, k, v):
    """Where a backward writes dq / dk / dv, and what autograd gets back for (q, k, v): three
    tensors, or ONE buffer for a packed projection, written through the strides of its three views
    (no per-view gradient accumulation passes)."""
    if k is None:
        dqkv = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        return _split(dqkv, None, None), (dqkv, None, None)
    grads = tuple(torch.empty(t.shape, dtype=t.dtype, device=t.device) for t in (q, k, v))
    return grads, grads


class _Attention(torch.autograd.Function):
    """The attention core on q, k, v [B, N, H, D], or on a packed projection ``q`` [B, N, 3, H, D]
    with ``k`` and ``v`` None."""

    @staticmethod
    def forward(ctx, q, k, v, scale, bias_h, bias_w, grid, rope, drop):
        _require_gpu(q, k, v)
        o, lse = _fwd(*_split(q, k, v), scale, bias_h, bias_w, grid, rope, drop)
        ctx.save_for_backward(q, k, v, o, lse, bias_h, bias_w)
        ctx.scale, ctx.grid, ctx.rope, ctx.drop = scale, grid, rope, drop
        return o

    @staticmethod
    @_sinking
    def backward(ctx, do):
        q, k, v, o, lse, bias_h, bias_w = ctx.saved_tensors
        do = _grad_in(do)
        grads, ret = _qkv_grads(q, k, v)
        dbh, dbw = _bwd(*_split(q, k, v), o, lse, do, *grads, ctx.scale, bias_h, bias_w, ctx.grid, ctx.rope, ctx.drop)
        return (*ret, None, dbh, dbw, None, None, None)


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: Optional[float] = None,
              bias: Optional[Tuple[torch.Tensor, torch.Tensor, Tuple[int, int]]] = None,
              rotary: Optional[float] = None, dropout=None) -> torch.Tensor:
    """softmax(scale * q k^T [+ relpos bias]) v on token-major [B, N, H, D] tensors.

    ``scale`` defaults to the reference's 1/sqrt(head_ch) (attention.py:39).  ``bias`` is
    ``(bias_h, bias_w, (Hs, Ws))`` from :func:`relpos_bias` (BoTNet).  ``rotary`` (a base, e.g.
    10000.0): q and k are rotated first (position_embed.py:8-20) -- inside the kernels' staging
    where they take it (:func:`rope_fused_ok`), else by the standalone rotary pass.  ``dropout`` is
    ``(rate, DropoutRng)``: the probabilities are dropped inside the kernels (attention.py:54-58;
    the rate is quantised to n / 256, below 1 / 512 nothing is dropped); rotary then runs as the
    standalone pass, and relative logits are not supported with it."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if dropout is not None and bias is not None:
        raise NotImplementedError("attention dropout with relative logits is not implemented")
    if rotary is not None and (dropout is not None or bias is not None or not rope_fused_ok(q, k, v)):
        q, k = _Rotary.apply(q, float(rotary)), _Rotary.apply(k, float(rotary))   # the standalone pass
        rotary = None
    bh, bw, grid = (None, None, None) if bias is None else (bias[0], bias[1], tuple(bias[2]))
    return _Attention.apply(q, k, v, float(scale), bh, bw, grid, None if rotary is None else float(rotary),
                            _draw(dropout))


def attention_packed(qkv: torch.Tensor, scale: Optional[float] = None, rotary: Optional[float] = None,
                     dropout=None) -> torch.Tensor:
    """Self-attention on a packed projection ``qkv`` [B, N, 3, H, D] (one fused QKV GEMM output);
    ``rotary`` and ``dropout`` as in :func:`attention`."""
    if qkv.dim() != 5 or qkv.shape[2] != 3:
        raise ValueError(f"expected qkv [B, N, 3, H, D], got {tuple(qkv.shape)}")
    if scale is None:
        scale = 1.0 / math.sqrt(qkv.shape[-1])
    if rotary is not None and (dropout is not None or not rope_fused_ok(qkv[:, :, 0])):
        return attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], scale, rotary=rotary, dropout=dropout)
    return _Attention.apply(qkv, None, None, float(scale), None, None, None, None if rotary is None else float(rotary),
                            _draw(dropout))


# ----------------------------------------------------------------------------- talking heads
def _th_fwd(q, k, v, th1, th2, scale, rope=None):
    lib = L.load()
    B, Nq, H, D = q.shape
    th1c = th1.detach().to(torch.float32).contiguous()
    th2c = th2.detach().to(torch.float32).contiguous()
    o = torch.empty((B, Nq, H, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
    d = _make_desc(q, k, v, o, scale)
    tok = _TIMER.begin("th_attn_fwd") if _TIMER is not None else None
    if rope is not None:
        sin, cos = _rope_tabs(q, k, rope)
        L.check(lib.sae_th_attn_fwd_rotary(_stream(q), ctypes.byref(d), _ptr(q), _ptr(k), _ptr(v), _ptr(th1c),
                                           _ptr(th2c), _ptr(sin), _ptr(cos), _ptr(o), _ptr(lse)))
    else:
        L.check(lib.sae_th_attn_fwd(_stream(q), ctypes.byref(d), _ptr(q), _ptr(k), _ptr(v), _ptr(th1c),
                                    _ptr(th2c), _ptr(o), _ptr(lse)))
    if tok is not None:
        _TIMER.end(tok, (B, Nq, k.shape[1], H, D))
    return o, lse, th1c, th2c


def _th_bwd(q, k, v, th1, th2, lse, do, dq, dk, dv, scale, rope=None, dth1=None, dth2=None):
    """dT1 / dT2 go into ``dth1`` / ``dth2`` when given (fp32 [H, H]: the transforms' gradient
    sinks -- the reduce kernel writes them whole), else into fresh tensors."""
    lib = L.load()
    dth1 = torch.empty_like(th1) if dth1 is None else dth1
    dth2 = torch.empty_like(th2) if dth2 is None else dth2
    d = _make_desc(q, k, v, None, scale, do, dq, dk, dv)
    ws = torch.empty(lib.sae_th_attn_bwd_workspace_bytes(ctypes.byref(d)), dtype=torch.uint8, device=q.device)
    tok = _TIMER.begin("th_attn_bwd") if _TIMER is not None else None
    if rope is not None:
        sin, cos = _rope_tabs(q, k, rope)
        L.check(lib.sae_th_attn_bwd_rotary(_stream(q), ctypes.byref(d), _ptr(q), _ptr(k), _ptr(v), _ptr(th1),
                                           _ptr(th2), _ptr(lse), _ptr(do), _ptr(sin), _ptr(cos), _ptr(dq), _ptr(dk),
                                           _ptr(dv), _ptr(dth1), _ptr(dth2), _ptr(ws)))
    else:
        L.check(lib.sae_th_attn_bwd(_stream(q), ctypes.byref(d), _ptr(q), _ptr(k), _ptr(v), _ptr(th1), _ptr(th2),
                                    _ptr(lse), _ptr(do), _ptr(dq), _ptr(dk), _ptr(dv), _ptr(dth1), _ptr(dth2),
                                    _ptr(ws)))
    if tok is not None:
        _TIMER.end(tok, tuple(q.shape))
    return dth1, dth2


def _th_sinks(th1, th2):
    """Gradient sinks of the two transforms (fp32 contiguous parameters only: the reduce kernel
    writes fp32 [H, H] in place), or None each."""
    ok = lambda t: t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0
    s1 = _sink(th1) if ok(th1) else None
    s2 = _sink(th2) if ok(th2) else None
    if s1 is not None and s2 is not None and s1.data_ptr() == s2.data_ptr():
        # one parameter used as both transforms: autograd adds the two gradients.  Sink neither:
        # a sink counts as final the moment its kernel is enqueued (the overlapped all-reduce
        # launches its bucket then), so sinking dT1 while autograd still adds dT2 into the same
        # view would race the bucket's all-reduce; the post-accumulate hook marks it ready instead
        s1 = s2 = None
    return s1, s2


class _TalkingHeads(torch.autograd.Function):
    """Talking-heads attention on q, k, v [B, N, H, D], or on a packed projection ``q``
    [B, N, 3, H, D] with ``k`` and ``v`` None."""

    @staticmethod
    def forward(ctx, q, k, v, th1, th2, scale, rope):
        _require_gpu(q, k, v, th1, th2)
        o, lse, th1c, th2c = _th_fwd(*_split(q, k, v), th1, th2, scale, rope)
        ctx.save_for_backward(q, k, v, th1c, th2c, lse)
        ctx.scale, ctx.rope = scale, rope
        ctx.th_dtypes = (th1.dtype, th2.dtype)
        ctx.sinks = _th_sinks(th1, th2)
        return o

    @staticmethod
    @_sinking
    def backward(ctx, do):
        q, k, v, th1, th2, lse = ctx.saved_tensors
        do = _grad_in(do)
        grads, ret = _qkv_grads(q, k, v)
        s1, s2 = ctx.sinks
        dth1, dth2 = _th_bwd(*_split(q, k, v), th1, th2, lse, do, *grads, ctx.scale, ctx.rope,
                             _grad_out(s1, th1.shape, th1.device), _grad_out(s2, th2.shape, th2.device))
        return (*ret, _unsunk(dth1.to(ctx.th_dtypes[0]), s1), _unsunk(dth2.to(ctx.th_dtypes[1]), s2), None, None)


def _th_rope_ok(q, k, v) -> bool:
    return _rope_route("sae_th_attn_route", (q, k, v))


def talking_heads_attention_packed(qkv, th1, th2, scale: Optional[float] = None, rotary: Optional[float] = None):
    """Talking-heads self-attention on a packed projection ``qkv`` [B, N, 3, H, D]; ``rotary`` as
    in :func:`attention`."""
    if qkv.dim() != 5 or qkv.shape[2] != 3:
        raise ValueError(f"expected qkv [B, N, 3, H, D], got {tuple(qkv.shape)}")
    if scale is None:
        scale = 1.0 / math.sqrt(qkv.shape[-1])
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    if rotary is not None and not _th_rope_ok(q, k, v):
        return talking_heads_attention(q, k, v, th1, th2, scale, rotary)
    return _TalkingHeads.apply(qkv, None, None, th1, th2, float(scale), None if rotary is None else float(rotary))


def talking_heads_attention(q, k, v, th1, th2, scale: Optional[float] = None, rotary: Optional[float] = None):
    """Talking-heads attention (attention.py:41-58, talking_heads.py:9-14); th1/th2 are the
    fp32 [H, H] ``talking_heads_transform`` params of TalkingHeadsBlock_0 / _1; ``rotary`` as in
    :func:`attention`."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if rotary is not None and not _th_rope_ok(q, k, v):
        q, k = _Rotary.apply(q, float(rotary)), _Rotary.apply(k, float(rotary))
        rotary = None
    return _TalkingHeads.apply(q, k, v, th1, th2, float(scale), None if rotary is None else float(rotary))


# ------------------------------------------------------------------------ relative logits
class _RelposBias(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qhat, emb_h, emb_w, Hs, Ws):
        _require_gpu(qhat, emb_h, emb_w)
        lib = L.load()
        B, N, H, D = qhat.shape
        if N != Hs * Ws:
            raise ValueError(f"relpos grid {Hs}x{Ws} does not match {N} tokens")
        eh = emb_h.detach().to(torch.float32).contiguous()
        ew = emb_w.detach().to(torch.float32).contiguous()
        bh = torch.empty((B, H, N, Hs), dtype=torch.float32, device=qhat.device)
        bw = torch.empty((B, H, N, Ws), dtype=torch.float32, device=qhat.device)
        L.check(lib.sae_relpos_bias_fwd(_stream(qhat), B, H, Hs, Ws, D, dtype_code(qhat.dtype), _ptr(qhat),
                                        L.s3(_bnh(qhat)), _ptr(eh), _ptr(ew), _ptr(bh), _ptr(bw)))
        ctx.save_for_backward(qhat, eh, ew)
        ctx.grid = (Hs, Ws)
        ctx.emb_dtypes = (emb_h.dtype, emb_w.dtype)
        return bh, bw

    @staticmethod
    @_sinking
    def backward(ctx, dbh, dbw):
        qhat, eh, ew = ctx.saved_tensors
        lib = L.load()
        Hs, Ws = ctx.grid
        B, N, H, D = qhat.shape
        dbh = dbh.contiguous() if dbh is not None else torch.zeros((B, H, N, Hs), device=qhat.device)
        dbw = dbw.contiguous() if dbw is not None else torch.zeros((B, H, N, Ws), device=qhat.device)
        dq = torch.empty((B, N, H, D), dtype=qhat.dtype, device=qhat.device)
        deh, dew = torch.empty_like(eh), torch.empty_like(ew)
        ws = torch.empty(lib.sae_relpos_bias_bwd_workspace_bytes(B, Hs, Ws, D), dtype=torch.uint8,
                         device=qhat.device)
        L.check(lib.sae_relpos_bias_bwd(_stream(qhat), B, H, Hs, Ws, D, dtype_code(qhat.dtype), _ptr(qhat),
                                        L.s3(_bnh(qhat)), _ptr(eh), _ptr(ew), _ptr(dbh), _ptr(dbw), None, _ptr(dq),
                                        L.s3(_bnh(dq)), _ptr(deh), _ptr(dew), _ptr(ws)))
        return dq, deh.to(ctx.emb_dtypes[0]), dew.to(ctx.emb_dtypes[1]), None, None


def relpos_bias(qhat, emb_h, emb_w, grid: Tuple[int, int]):
    """BoTNet RelativeLogits (botnet.py:113-141) as two fp32 tables per query row:
    bias_h [B,H,N,Hs], bias_w [B,H,N,Ws]; the attention kernel adds
    ``bias_h[q, k // Ws] + bias_w[q, k % Ws]`` to the score tile."""
    return _RelposBias.apply(qhat, emb_h, emb_w, int(grid[0]), int(grid[1]))


# ---------------------------------------------------------------------------------- rotary
_TABLES = {}


def rotary_tables(n: int, dim: int, device, base: float = 10000.0):
    """fp32 sin/cos tables [n, dim/2] computed in float64 on the host (exact angles for the
    long CvT sequences; device sinf at |theta| ~ 3e3 would lose ~1e-4)."""
    key = (n, dim, float(base), str(device))
    t = _TABLES.get(key)
    if t is None:
        i = torch.arange(dim // 2, dtype=torch.float64)
        inv_freq = base ** (-2.0 * i / dim)
        ang = torch.arange(n, dtype=torch.float64)[:, None] * inv_freq[None, :]
        t = (torch.sin(ang).float().to(device), torch.cos(ang).float().to(device))
        _TABLES[key] = t
    return t


def _rotary_call(x, y, sin, cos, inverse):
    lib = L.load()
    B, N, H, D = x.shape
    L.check(lib.sae_rotary(_stream(x), B, N, H, D, dtype_code(x.dtype), _ptr(x), L.s3(_bnh(x)), _ptr(y),
                           L.s3(_bnh(y)), _ptr(sin), _ptr(cos), 1 if inverse else 0))


class _Rotary(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, base):
        _require_gpu(x)
        B, N, H, D = x.shape
        if D % 2:
            raise ValueError("rotary needs an even head_dim")
        sin, cos = rotary_tables(N, D, x.device, base)
        y = torch.empty((B, N, H, D), dtype=x.dtype, device=x.device)
        _rotary_call(x, y, sin, cos, False)
        ctx.base = base
        return y

    @staticmethod
    @_sinking
    def backward(ctx, dy):
        dy = _grad_in(dy)
        B, N, H, D = dy.shape
        sin, cos = rotary_tables(N, D, dy.device, ctx.base)
        dx = torch.empty((B, N, H, D), dtype=dy.dtype, device=dy.device)
        _rotary_call(dy, dx, sin, cos, True)
        return dx, None


def rotary(x: torch.Tensor, base: float = 10000.0) -> torch.Tensor:
    """GPT-J interleaved rotary on [B, N, H, D] (position_embed.py:8-20; build-defined base
    10000, survey D6)."""
    return _Rotary.apply(x, float(base))


# ------------------------------------------------------------------------------ projections
def gemm_dw(x2: torch.Tensor, dy2: torch.Tensor, dw: torch.Tensor, db: Optional[torch.Tensor] = None,
            accumulate: bool = False, jblock: int = 0, offload: bool = False) -> None:
    """dw (+)= x2^T dy2 and db (+)= colsum(dy2) in fp32 through ``sae_gemm_dw`` (split over the
    token axis, fixed-order reduction).  x2 [M, I], dy2 [M, J] bf16 with unit column stride.
    ``jblock`` > 0: dw is [J / jblock, I, jblock] (contiguous column blocks).  ``offload``: dw / db
    are gradient sinks nobody reads before the step's join, so the GEMM may run on the
    weight-gradient side stream of the open sink window (GradSinks.wgrad_stream; none outside one)."""
    lib = L.load()
    _require_gpu(x2, dy2, dw)
    M, I = x2.shape
    J = dy2.shape[1]
    side = _ACTIVE_SINKS.wgrad_stream if (offload and _ACTIVE_SINKS is not None) else None
    if side is not None:
        side.wait_stream(torch.cuda.current_stream(x2.device))   # x2 / dy2 are written on the main stream
        x2.record_stream(side)    # ... and stay allocated until the side stream has read them
        dy2.record_stream(side)
    with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
        ws = torch.empty(lib.sae_gemm_dw_workspace_bytes(M, I, J), dtype=torch.uint8, device=x2.device)
        tok = _TIMER.begin("gemm_dw") if _TIMER is not None else None
        if jblock:
            L.check(lib.sae_gemm_dw_blocked(_stream(x2), M, I, J, int(jblock), _ptr(x2), x2.stride(0), _ptr(dy2),
                                            dy2.stride(0), _ptr(dw), _ptr(db), int(accumulate), _ptr(ws)))
        else:
            L.check(lib.sae_gemm_dw(_stream(x2), M, I, J, _ptr(x2), x2.stride(0), _ptr(dy2), dy2.stride(0),
                                    _ptr(dw), dw.stride(0), _ptr(db), int(accumulate), _ptr(ws)))
        if tok is not None:
            _TIMER.end(tok, (M, I, J))


def gemm_f32(a: torch.Tensor, b: torch.Tensor, bias: Optional[torch.Tensor] = None,
             out: Optional[torch.Tensor] = None, colsum: Optional[torch.Tensor] = None,
             accumulate: bool = False) -> torch.Tensor:
    """``a @ b (+ bias)`` in exact fp32 through ``sae_gemm_f32`` (f32-input MFMA).  ``a`` [M, K] and
    ``b`` [K, N] are fp32 views with a unit stride along one dimension each (a transposed view is
    read in place: ``x.t()`` for a weight gradient, ``w.t()`` for an input gradient).  ``colsum``
    (fp32 [N]) also receives the column sums of ``b`` (a bias gradient); ``accumulate`` adds into
    ``out`` / ``colsum``."""
    lib = L.load()
    _require_gpu(a, b)
    M, K = a.shape
    N = b.shape[1]
    if b.shape[0] != K:
        raise ValueError(f"gemm_f32: a {tuple(a.shape)} and b {tuple(b.shape)} disagree on K")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    elif (out.dtype != torch.float32 or tuple(out.shape) != (M, N) or out.stride(1) != 1
          or out.device != a.device):
        raise ValueError(f"gemm_f32: out must be fp32 [{M}, {N}] with unit column stride on {a.device}")
    if colsum is not None and (colsum.dtype != torch.float32 or colsum.dim() != 1 or colsum.numel() < N
                               or colsum.stride(0) != 1 or colsum.device != a.device):
        # the kernel writes colsum[0 .. N) as fp32: anything else would be corrupted silently
        raise ValueError(f"gemm_f32: colsum must be a unit-stride fp32 vector of >= {N} elements on {a.device}")
    if bias is not None:
        bias = bias.float().contiguous()
    nbytes = lib.sae_gemm_f32_workspace_bytes(M, N, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=a.device) if nbytes else None
    tok = _TIMER.begin("gemm_f32") if _TIMER is not None else None
    L.check(lib.sae_gemm_f32(_stream(a), M, N, K, _ptr(a), a.stride(0), a.stride(1), _ptr(b), b.stride(0),
                             b.stride(1), _ptr(bias), _ptr(out), out.stride(0), _ptr(colsum), int(accumulate),
                             _ptr(ws)))
    if tok is not None:
        _TIMER.end(tok, (M, K, N))
    return out


def _f32_operand_ok(t: torch.Tensor) -> bool:
    """A view sae_gemm_f32 reads in place: fp32, unit stride along one dim, 16-byte aligned, the
    other stride and the contiguous extent multiples of 4."""
    if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.data_ptr() % 16:
        return False
    r, c = t.shape
    if t.stride(1) == 1:
        return t.stride(0) % 4 == 0 and c % 4 == 0 and t.stride(0) >= c
    if t.stride(0) == 1:
        return t.stride(1) % 4 == 0 and r % 4 == 0 and t.stride(1) >= r
    return False


def _rows_ok(t: torch.Tensor) -> bool:
    """A 2-D operand sae_gemm_nt / sae_gemm_dw read in place: bf16 on the GPU, unit column stride,
    width and row pitch multiples of 8, 16-byte aligned."""
    return (t.is_cuda and t.dtype == torch.bfloat16 and t.shape[1] % 8 == 0 and t.stride(1) == 1
            and t.stride(0) % 8 == 0 and t.data_ptr() % 16 == 0)


def _nt_ok(a2: torch.Tensor, N: int) -> bool:
    return N % 8 == 0 and _rows_ok(a2)


def _dw_ok(x2: torch.Tensor, dy2: torch.Tensor) -> bool:
    return _rows_ok(x2) and _rows_ok(dy2)


def _pitched(t: torch.Tensor, align: bool = True) -> torch.Tensor:
    """``t`` [M, K] with a unit column stride, a row pitch that is a multiple of 8 elements and
    (``align``) a 16-byte-aligned base, as the GEMM kernels read it in place: copied only if it is not."""
    if t.stride(1) != 1 or t.stride(0) % 8 or (align and t.data_ptr() % 16):
        return t.contiguous()
    return t


# ------------------------------------------------------------ registry of the bf16 weight copies
# A group is a list of fp32 2-D Dense kernels [K, n_j] of one K, stacked along columns; its bf16
# [K, sum n_j] copy and the transpose are served from ONE registry, keyed by the weights' data
# pointers and checked against their version counters.  A per-forward entry (owner None) is cast by
# ``forward_casts`` at the start of an encoder's forward and taken out when it returns (the next
# optimizer step changes the fp32 weights).  A persistent entry belongs to an optimizer that writes
# the copies as it updates (FusedAdamW with cast_groups, sae_adamw_step_cast): the forward neither
# casts nor allocates for it.  That update goes through raw pointers (no version bump); an in-place
# change of a weight OUTSIDE it (load_state_dict, a copy_) bumps the version counter, and the next
# lookup or ``refresh_persistent_casts`` re-casts into the same buffers.
@dataclasses.dataclass
class _CastEntry:
    versions: tuple        # the weights' version counters when the copies were written
    w16: torch.Tensor      # bf16 [K, N]
    wt16: torch.Tensor     # bf16 [N, K]
    weights: list          # the fp32 kernels (held: their addresses cannot be reused while registered)
    owner: object = None   # who keeps the copies current; None: a per-forward entry


_CASTS = {}


def _cast_key(ws):
    return tuple(w.data_ptr() for w in ws)


def _versions(ws):
    return tuple(w._version for w in ws)


def _run_casts(entries) -> None:
    """Cast every entry's fp32 weights into its bf16 buffers, all in one launch."""
    items = []
    for e in entries:
        K, N = e.w16.shape
        col = 0
        for w in e.weights:
            items.append(L.WeightCastItem(w.data_ptr(), e.w16.data_ptr(), e.wt16.data_ptr(), K, w.shape[1], N, K, col))
            col += w.shape[1]
        e.versions = _versions(e.weights)
    if items:
        arr = (L.WeightCastItem * len(items))(*items)
        L.check(L.load().sae_weight_cast_multi(_stream(entries[0].weights[0]), len(items), arr))


@contextlib.contextmanager
def forward_casts(groups):
    """For the ``with`` body (one encoder forward), serve each of ``groups`` a bf16 copy cast here, in one
    launch.  A group that is not 2-D fp32 contiguous with one K is skipped (its projections cast for
    themselves), as is one an optimizer already serves.  On exit only the entries added here go."""
    added = []
    for ws in groups:
        K = ws[0].shape[0]
        if any(w.dim() != 2 or w.shape[0] != K or w.dtype != torch.float32 or not w.is_contiguous() for w in ws):
            continue
        key = _cast_key(ws)
        if key in _CASTS and _CASTS[key].owner is not None:   # the optimizer keeps this group's copies
            continue
        N = sum(w.shape[1] for w in ws)
        e = _CASTS[key] = _CastEntry((), torch.empty((K, N), dtype=torch.bfloat16, device=ws[0].device),
                                     torch.empty((N, K), dtype=torch.bfloat16, device=ws[0].device), list(ws))
        added.append((key, e))
    try:
        _run_casts([e for _, e in added])
        yield
    finally:
        for key, e in added:
            if _CASTS.get(key) is e:
                del _CASTS[key]


def clear_weight_cache() -> None:
    """Drop every per-forward entry now, an open ``forward_casts`` block's included (a reset for callers)."""
    for key in [k for k, e in _CASTS.items() if e.owner is None]:
        del _CASTS[key]


def register_persistent_casts(groups, w16s, wt16s, owner) -> None:
    """Serve ``groups``' bf16 copies from ``w16s`` / ``wt16s``, kept current from now on by ``owner``
    (the optimizer that writes them; not None), and cast the weights' present values into them.
    A later registration of the same weights takes over."""
    if owner is None:
        raise ValueError("register_persistent_casts: a persistent entry needs an owner")
    entries = [_CastEntry((), w16, wt16, list(ws), owner) for ws, w16, wt16 in zip(groups, w16s, wt16s)]
    _CASTS.update((_cast_key(e.weights), e) for e in entries)
    _run_casts(entries)


def unregister_persistent_casts(owner) -> None:
    """Stop serving the copies ``owner`` registered (and still owns: not those taken over since)."""
    for key in [k for k, e in _CASTS.items() if e.owner is owner]:
        del _CASTS[key]


def release_persistent_casts(params) -> None:
    """Drop every persistent group holding one of ``params`` (an optimizer that now updates them
    without writing those copies takes them over: the copies would go stale)."""
    ids = {p.data_ptr() for p in params}
    for key in [k for k, e in _CASTS.items()
                if e.owner is not None and any(w.data_ptr() in ids for w in e.weights)]:
        del _CASTS[key]


def refresh_persistent_casts(groups, only_if_stale: bool = False) -> None:
    """Re-cast the persistent copies of ``groups`` from their fp32 weights (one launch); with
    ``only_if_stale`` only when a weight of one was changed in place since (its version moved)."""
    entries = [e for e in (_CASTS.get(_cast_key(ws)) for ws in groups) if e is not None and e.owner is not None]
    if not only_if_stale or any(e.versions != _versions(e.weights) for e in entries):
        _run_casts(entries)


def persistent_cast_entries(groups) -> tuple:
    """Per group, the persistent entry serving it (None: none does).  A captured forward reads the
    copies it was captured with: its owner keeps this tuple (and with it the buffers) and captures
    again when an entry is no longer the same object."""
    ents = (_CASTS.get(_cast_key(ws)) for ws in groups)
    return tuple(e if e is not None and e.owner is not None else None for e in ents)


def _cast_lookup(ws):
    """(bf16 [K, N], bf16 [N, K]) of the group ``ws`` from the registry, or None."""
    e = _CASTS.get(_cast_key(ws))
    if e is None:
        return None
    if e.versions != _versions(e.weights):
        if e.owner is None:   # a per-forward entry whose weight moved: stale, the caller casts
            return None
        _run_casts([e])
    return e.w16, e.wt16


def _cast(ws, dt):
    """bf16 [K, N] and [N, K] of the column-stacked fp32 weights ``ws`` (cached, or one launch)."""
    hit = _cast_lookup(ws) if dt == torch.bfloat16 else None
    if hit is not None:
        return hit
    w = ws[0] if len(ws) == 1 else torch.cat(ws, dim=1)
    if dt == torch.bfloat16 and w.dtype == torch.float32 and w.is_cuda:
        return weight_cast(w)
    return w.to(dt), None


# ------------------------------------------------------------- Dense: facts, plans, executors
# Every bf16 projection on aligned operands whose widths are multiples of 8 runs forward and input gradient
# on sae_gemm_nt (the C ABI picks the kernel: gemm.hip nt_plan) and its weight gradient on sae_gemm_dw: every
# width in create_model.py:6-215 (ViT-B/L, DeiT, CaiT 192-768, CeiT, CvT 64/192/368/1024, TNT 24/40/384/640);
# tests/test_routing_cpu.py pins it on the plans below.  GEMM_LIB = True sends forward and input gradient to
# the library GEMM (A/B runs only).
GEMM_LIB = False
# Calls of at most SMALL_M rows (classifier heads, CLS-token projections): while GEMM_LIB is on they keep
# their forward on sae_gemm_nt (with it off the bound decides nothing there), and only they take "dw_t".
SMALL_M = 4096


class DenseFacts(NamedTuple):
    """What the route of one Dense call depends on.  The layout fields are the results of _nt_ok /
    _dw_ok / _f32_operand_ok (false off the GPU); the three about dY are known in the backward only."""
    M: int                 # rows
    I: int                 # input features
    widths: tuple          # output features per column block (J = their sum)
    dtype: torch.dtype     # compute dtype
    on_gpu: bool
    nt_x: bool             # x2 is an sae_gemm_nt operand for J output features
    nt_dy: bool            # dy2 ... for I output features
    dw: bool               # x2 and dy2 are sae_gemm_dw operands
    dw_t: bool             # J % 8 != 0 (no sae_gemm_nt), and a fresh dY^T [J, M] and the bf16 W^T [J, I] are
    f32_x: bool            # x2 and W are sae_gemm_f32 operands
    f32_dy: bool           # dy2 is
    has_wt: bool           # a bf16 W^T exists
    has_bias: bool
    sinks_w: tuple         # per column block: its kernel has a gradient sink
    sink_b: bool
    adjacent: bool         # every block has a sink and they lie back to back: one [nb, I, n] buffer
    gemm_lib: bool         # GEMM_LIB


def _dense_facts(x2, wd, wt, has_bias, sw, sb, widths) -> DenseFacts:
    """The facts of a call from its tensors, as the forward knows them (dY: see _Dense.backward)."""
    (M, I), J = x2.shape, wd.shape[1]
    adjacent = sw[0] is not None and (len(sw) == 1 or all(   # (read for equal-width blocks only)
        t is not None and t.data_ptr() == sw[0].data_ptr() + k * I * widths[0] * 4 for k, t in enumerate(sw)))
    # dY has y's dtype and device and M rows, so its contiguous transpose [J, M] (J > 1: a fresh,
    # allocator-aligned copy of pitch M) is an sae_gemm_dw operand exactly when M % 8 == 0
    dw_t = wt is not None and J % 8 != 0 and J > 1 and M % 8 == 0 and _rows_ok(wt)
    f32_x = wd.dtype == torch.float32 and _f32_operand_ok(x2) and _f32_operand_ok(wd)
    return DenseFacts(M, I, widths, wd.dtype, x2.is_cuda, nt_x=_nt_ok(x2, J), nt_dy=False, dw=False, dw_t=dw_t,
                      f32_x=f32_x, f32_dy=False, has_wt=wt is not None, has_bias=has_bias,
                      sinks_w=tuple(t is not None for t in sw), sink_b=sb is not None, adjacent=adjacent,
                      gemm_lib=GEMM_LIB)


def dense_facts_of_shapes(M, I, widths, dtype=torch.bfloat16, has_bias=True, sinks_w=None, sink_b=False,
                          adjacent=True, on_gpu=True) -> DenseFacts:
    """The facts of a call on contiguous, aligned operands with fp32 parameters and a contiguous dY (what a
    model's Dense sees), from shapes alone.  ``adjacent``: the sinks, if every block has one, lie back to back."""
    J = sum(widths)
    sinks_w = tuple(sinks_w) if sinks_w is not None else (False,) * len(widths)
    rows = on_gpu and dtype == torch.bfloat16 and I % 8 == 0   # x2 [M, I] and W^T [J, I] are row operands
    nt = rows and J % 8 == 0
    f32 = on_gpu and dtype == torch.float32 and J % 4 == 0
    return DenseFacts(M, I, tuple(widths), dtype, on_gpu, nt_x=nt, nt_dy=nt, dw=nt,
                      dw_t=rows and J % 8 != 0 and J > 1 and M % 8 == 0, f32_x=f32 and I % 4 == 0, f32_dy=f32,
                      has_wt=on_gpu and dtype == torch.bfloat16, has_bias=has_bias, sinks_w=sinks_w,
                      sink_b=sink_b, adjacent=adjacent and all(sinks_w), gemm_lib=GEMM_LIB)


def _dx_reads_wt(f: DenseFacts) -> bool:
    """The "dw_t" input gradient can run (so the forward keeps the bf16 W^T for it): a small-M call whose J is
    no multiple of 8 (a classifier head of e.g. 10 classes), which sae_gemm_nt cannot reduce over."""
    return f.dw_t and f.M <= SMALL_M


def dense_fwd_plan(f: DenseFacts):
    """(route, keep_wt): "f32" exact fp32 on sae_gemm_f32, "nt" sae_gemm_nt, "lib" the library GEMM;
    ``keep_wt``: save the bf16 W^T for the backward."""
    if f.f32_x:
        route = "f32"
    elif f.has_wt and f.nt_x and (not f.gemm_lib or f.M <= SMALL_M):
        route = "nt"
    else:
        route = "lib"
    return route, _dx_reads_wt(f)


def dense_bwd_plan(f: DenseFacts):
    """(dx, dw, offload).  dx: "f32", "nt", "dw_t" (sae_gemm_dw over the rows of dY^T and W^T), "lib".
    dw: "f32"; on sae_gemm_dw "dw_blocks_sunk" (equal-width blocks, adjacent sinks: one blocked launch into
    the first), "dw_blocks" (equal-width blocks into a fresh [nb, I, n]), "dw_sunk" (one kernel into its
    sink), "dw" (one kernel, fresh buffer), "dw_stacked" (unequal blocks: a fresh [I, J], then slices);
    "lib".  ``offload``: the launch writes sinks only, so it may run on the weight-gradient side stream."""
    if f.f32_x and f.f32_dy:
        return "f32", "f32", False
    if f.dtype == torch.bfloat16 and f.nt_dy and not f.gemm_lib:
        dx = "nt"
    else:
        dx = "dw_t" if _dx_reads_wt(f) else "lib"
    nb, n = len(f.widths), f.widths[0]
    if not f.dw:
        dw = "lib"
    elif nb == 1:
        dw = "dw_sunk" if f.sinks_w[0] else "dw"
    elif len(set(f.widths)) == 1 and n % 4 == 0:   # one contiguous [I, n] gradient per block: no slice copies
        dw = "dw_blocks_sunk" if f.adjacent else "dw_blocks"
    else:
        dw = "dw_stacked"
    return dx, dw, dw in ("dw_sunk", "dw_blocks_sunk") and (f.sink_b or not f.has_bias)


def _dx_dw_t(dy2, wd, wt):
    # the reduction runs over the ROWS of dY^T [J, M] and W^T [J, I], i.e. on the weight-gradient
    # kernel: dx[m][i] = sum_j dY^T[j][m] W^T[j][i], fp32 then the activation dtype
    dxf = torch.empty((dy2.shape[0], wd.shape[0]), dtype=torch.float32, device=dy2.device)
    gemm_dw(dy2.t().contiguous(), wt, dxf)
    return dxf


_DX = {"f32": lambda dy2, wd, wt: gemm_f32(dy2, wd.t()), "nt": lambda dy2, wd, wt: gemm_nt(dy2, wd),
       "dw_t": _dx_dw_t, "lib": lambda dy2, wd, wt: dy2 @ wd.t()}


# A weight-gradient executor returns (db, [dW per column block]) as autograd sees them: None for a
# gradient that went into its sink (flat-buffer sinks of the multi-rank step, written in place).
def _db_out(ctx, dy2, sink):
    return _grad_out(sink, (dy2.shape[1],), dy2.device) if ctx.has_b else None


def _col_blocks(ctx, dw):
    return [g.to(wdt) for g, (_, wdt) in zip(dw.split([n for n, _ in ctx.wmeta], dim=1), ctx.wmeta)]


def _dw_f32(ctx, x2, dy2, offload):
    # per column block dW_k = X^T dY[:, block], that block's db slice as the ones-row column sum
    db = _db_out(ctx, dy2, ctx.sink_b)
    dws, col = [], 0
    for (n, wdt), sw in zip(ctx.wmeta, ctx.sinks_w):
        dst = _grad_out(sw, (x2.shape[1], n), x2.device)
        dyb = dy2[:, col:col + n]
        if not _f32_operand_ok(dyb):
            dyb = dyb.contiguous()
        gemm_f32(x2.t(), dyb, out=dst, colsum=db[col:col + n] if db is not None else None)
        dws.append(None if sw is not None else dst.to(wdt))
        col += n
    return _unsunk(db, ctx.sink_b), dws


def _dw_blocks(ctx, x2, dy2, offload, sunk=False):
    nb, n, I = len(ctx.wmeta), ctx.wmeta[0][0], x2.shape[1]
    db = _db_out(ctx, dy2, ctx.sink_b)
    if sunk:
        for t in ctx.sinks_w:
            _claim(t)
        dwb = ctx.sinks_w[0].as_strided((nb, I, n), (I * n, n, 1))
    else:
        dwb = _grad_out(None, (nb, I, n), x2.device)
    gemm_dw(x2, dy2, dwb, db, jblock=n, offload=offload)
    return _unsunk(db, ctx.sink_b), [None] * nb if sunk else [dwb[k].to(wdt) for k, (_, wdt) in enumerate(ctx.wmeta)]


def _dw_whole(ctx, x2, dy2, offload, sunk=False, bias_sink=True):
    # "dw_stacked" (bias_sink False) writes db into a fresh buffer although the bias may have a sink:
    # autograd then adds it into the sink.  Kept as found (open questions).
    sb = ctx.sink_b if bias_sink else None
    db = _db_out(ctx, dy2, sb)
    dw = _claim(ctx.sinks_w[0]) if sunk else _grad_out(None, (x2.shape[1], dy2.shape[1]), x2.device)
    gemm_dw(x2, dy2, dw, db, offload=offload)
    return _unsunk(db, sb), [None] if sunk else _col_blocks(ctx, dw)


def _dw_lib(ctx, x2, dy2, offload):
    dw = (x2.t() @ dy2).float()
    return dy2.sum(0, dtype=torch.float32) if ctx.has_b else None, _col_blocks(ctx, dw)


_DW = {"f32": _dw_f32, "dw_blocks_sunk": functools.partial(_dw_blocks, sunk=True), "dw_blocks": _dw_blocks,
       "dw_sunk": functools.partial(_dw_whole, sunk=True), "dw": _dw_whole,
       "dw_stacked": functools.partial(_dw_whole, bias_sink=False), "lib": _dw_lib}


class _Dense(torch.autograd.Function):
    """y = x @ W (+ b): Flax ``Dense`` / ``DenseGeneral`` semantics (input and fp32 kernel cast to
    the compute dtype).  ``W`` may be given as column blocks (the queries / keys / values kernels of
    one stacked projection): their gradients come back as the matching column slices.  The routes of
    forward, dX = dY W^T and dW / db (fp32) are named by dense_fwd_plan / dense_bwd_plan."""

    @staticmethod
    def forward(ctx, x, b, dt, *ws):
        x2 = x.to(dt).reshape(-1, ws[0].shape[0])
        wd, wt = _cast(ws, dt)
        widths = tuple(w.shape[1] for w in ws)
        ctx.wmeta = [(w.shape[1], w.dtype) for w in ws]
        ctx.sinks_w, ctx.sink_b = [_sink(w) for w in ws], _sink(b)
        ctx.facts = f = _dense_facts(x2, wd, wt, b is not None, ctx.sinks_w, ctx.sink_b, widths)
        route, keep_wt = dense_fwd_plan(f)
        if route == "f32":
            y = gemm_f32(x2, wd, b)                       # exact fp32 on the f32 MFMA, bias in the epilogue
        elif route == "nt":
            y = gemm_nt(x2, wt, b)                        # bias in the epilogue
        else:
            # bias rides in the library GEMM's epilogue (addmm) instead of a separate pass
            y = torch.addmm(b.to(dt), x2, wd) if b is not None else x2 @ wd
        ctx.save_for_backward(x2, wd, wt if keep_wt else None)   # version-checked
        ctx.has_b, ctx.xshape, ctx.xdtype = b is not None, x.shape, x.dtype
        return y.view(*x.shape[:-1], wd.shape[1])

    @staticmethod
    @_sinking
    def backward(ctx, dy):
        x2, wd, wt = ctx.saved_tensors
        I, J = wd.shape
        dy2 = _pitched(dy.reshape(-1, J), align=False)   # (a misaligned dY is not copied: the library routes)
        dx_route, dw_route, offload = dense_bwd_plan(ctx.facts._replace(
            nt_dy=_nt_ok(dy2, I), dw=_dw_ok(x2, dy2), f32_dy=_f32_operand_ok(dy2)))
        dx = _DX[dx_route](dy2, wd, wt).view(ctx.xshape).to(ctx.xdtype)
        db, dws = _DW[dw_route](ctx, x2, dy2, offload)
        return (dx, db, None, *dws)


def dense(x: torch.Tensor, w, b: Optional[torch.Tensor], dtype: torch.dtype) -> torch.Tensor:
    """Projection of the hot path: ``x @ w (+ b)`` in ``dtype`` with fp32 parameter gradients.
    ``w`` is a 2-D kernel [in, out] or a list of them stacked along the output axis."""
    ws = list(w) if isinstance(w, (list, tuple)) else [w]
    return _Dense.apply(x, b, dtype, *ws)


# ------------------------------------------------------------------------- patch embedding
def _patch_desc(images: torch.Tensor, patch: Tuple[int, int], embed: int, layout: str) -> L.SaePatchDesc:
    if layout == "NHWC":
        B, H, W, C = images.shape
        code = L.SAE_LAYOUT_NHWC
    elif layout == "HWCN":
        H, W, C, B = images.shape
        code = L.SAE_LAYOUT_HWCN
    else:
        raise ValueError(f"patch_embed: layout must be 'NHWC' or 'HWCN', got {layout!r}")
    return L.SaePatchDesc(B, H, W, C, int(patch[0]), int(patch[1]), int(embed), code, dtype_code(images.dtype))


# HWCN images (the train-step feed): write the patch matrix once (sae_patch_gather) and run the
# embedding and its weight gradient on the LDS-DMA GEMMs -- DeiT-S 59 + 56 us of fused HWCN
# gathers against the gather + gemm8 + gemm_dw8 (profiles/r05af_patch_gather_ab.txt).  False: the
# fused loaders (no patch copy; A/B runs).
PATCH_GATHER = os.environ.get("SAE_PATCH_GATHER", "1") != "0"


class _PatchEmbed(torch.autograd.Function):
    """patch_embed.py:15-26 in bf16: the patch gather fused into the GEMM's operand staging
    (``sae_patch_embed_fwd``), weight / bias gradients by the same gather (``sae_patch_embed_bwd``);
    for HWCN images the patch matrix is written once (``sae_patch_gather``) and both products run on
    ``sae_gemm_nt`` / ``sae_gemm_dw``.  The images take no gradient (they are the batch,
    train.py:80-82)."""

    @staticmethod
    def forward(ctx, images, w, b, patch, layout):
        lib = L.load()
        E = w.shape[1]
        desc = _patch_desc(images, patch, E, layout)
        _, wt = _cast([w], torch.bfloat16)
        Lp = (desc.height // desc.patch_h) * (desc.width // desc.patch_w)
        K = desc.patch_h * desc.patch_w * desc.channels
        bias = b.float().contiguous() if b is not None else None
        tok = _TIMER.begin("patch_embed") if _TIMER is not None else None
        gathered = layout == "HWCN" and PATCH_GATHER and E % 8 == 0
        if gathered:
            pm = torch.empty((desc.batch * Lp, K), dtype=torch.bfloat16, device=images.device)
            L.check(lib.sae_patch_gather(_stream(images), ctypes.byref(desc), _ptr(images), _ptr(pm)))
            out = gemm_nt(pm, wt, bias).view(desc.batch, Lp, E)
            ctx.save_for_backward(pm)
        else:
            out = torch.empty((desc.batch, Lp, E), dtype=torch.bfloat16, device=images.device)
            L.check(lib.sae_patch_embed_fwd(_stream(images), ctypes.byref(desc), _ptr(images), _ptr(wt),
                                            _ptr(bias), _ptr(out)))
            ctx.save_for_backward(images)
        if tok is not None:
            _TIMER.end(tok, (desc.batch * Lp, w.shape[0], E))
        ctx.desc, ctx.wshape, ctx.wdtype, ctx.has_b = desc, tuple(w.shape), w.dtype, b is not None
        ctx.gathered = gathered
        ctx.sinks = (_sink(w), _sink(b))
        return out

    @staticmethod
    @_sinking
    def backward(ctx, dout):
        lib = L.load()
        (saved,) = ctx.saved_tensors
        desc = ctx.desc
        dout = dout.to(torch.bfloat16).contiguous()
        sw, sb = ctx.sinks   # flat-buffer sinks (multi-rank step): written in place
        dw = _grad_out(sw, ctx.wshape, dout.device)
        db = _grad_out(sb, (ctx.wshape[1],), dout.device) if ctx.has_b else None
        if ctx.gathered:   # dW = P^T dY, db = colsum(dY) on the weight-gradient kernel
            gemm_dw(saved, dout.view(-1, ctx.wshape[1]), dw, db)
        else:
            ws = torch.empty(lib.sae_patch_embed_bwd_workspace_bytes(ctypes.byref(desc)), dtype=torch.uint8,
                             device=dout.device)
            L.check(lib.sae_patch_embed_bwd(_stream(dout), ctypes.byref(desc), _ptr(saved), _ptr(dout), _ptr(dw),
                                            _ptr(db), 0, _ptr(ws)))
        return None, None if sw is not None else dw.to(ctx.wdtype), _unsunk(db, sb), None, None


def patch_embed(images: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], patch: Tuple[int, int],
                layout: str = "NHWC") -> torch.Tensor:
    """``PatchEmbedBlock`` (patch_embed.py:15-26) in bf16: tokens [B, L, E] of ``images`` (bf16 or
    fp32; ``layout`` "NHWC" [B, H, W, C] or the train-step feed "HWCN" [H, W, C, B], train.py:80)
    times the fp32 Dense kernel ``w`` [ph * pw * C, E] (+ ``b``).  The images take no gradient."""
    _require_gpu(images, w)
    if images.requires_grad:
        raise NotImplementedError("patch_embed: the images take no gradient on this path (train.py:80-82)")
    if images.dtype not in (torch.bfloat16, torch.float32):
        images = images.float()
    if not images.is_contiguous() or images.data_ptr() % 16:
        images = images.contiguous()
    if w.dtype != torch.float32 or w.dim() != 2:
        raise ValueError("patch_embed: w must be the fp32 Dense kernel [ph * pw * C, E]")
    return _PatchEmbed.apply(images, w, b, tuple(int(p) for p in patch), layout)


def patch_embed_ok(images: torch.Tensor, w: torch.Tensor, patch: Tuple[int, int], layout: str = "NHWC") -> bool:
    """Shapes the fused kernel takes (sae_patch_embed_fwd's requirements, include/sae_attn.h)."""
    if images.dim() != 4 or not images.is_cuda:
        return False
    H, W, C, B = images.shape if layout == "HWCN" else (images.shape[1], images.shape[2], images.shape[3],
                                                        images.shape[0])
    ph, pw = patch
    K = ph * pw * C
    return (H % ph == 0 and W % pw == 0 and K % 64 == 0 and (pw * C) % 8 == 0 and w.shape[1] % 8 == 0
            and w.shape[0] == K and (layout != "HWCN" or B % 8 == 0))


# ------------------------------------------------- forward / input-gradient GEMMs (sae_gemm_nt)
EPI_NONE, EPI_GELU, EPI_DGELU = 0, 1, 2
# the FF block's pair (include/sae_attn.h): the forward saves g = gelu'(h) instead of h, the
# input-gradient epilogue multiplies by it
EPI_GELU_GRAD, EPI_MUL_AUX = 3, 4
FF_GELU_GRAD = os.environ.get("SAE_FF_GELU_GRAD", "1") != "0"   # (False: save h, GELU' epilogue; A/B)


def weight_cast(w: torch.Tensor, plain: bool = True, transposed: bool = True):
    """fp32 Dense kernel [K, N] -> (bf16 [K, N] or None, bf16 [N, K] or None) in one HIP pass."""
    lib = L.load()
    _require_gpu(w)
    K, N = w.shape
    w = w.contiguous()
    w16 = torch.empty((K, N), dtype=torch.bfloat16, device=w.device) if plain else None
    wt16 = torch.empty((N, K), dtype=torch.bfloat16, device=w.device) if transposed else None
    L.check(lib.sae_weight_cast(_stream(w), K, N, _ptr(w), _ptr(w16), _ptr(wt16)))
    return w16, wt16


def gemm_nt(a2: torch.Tensor, bt: torch.Tensor, bias: Optional[torch.Tensor] = None, epilogue: int = EPI_NONE,
            aux: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, drop=None):
    """``epi(a2 @ bt^T (+ bias))`` through ``sae_gemm_nt``: a2 [M, K], bt [N, K] bf16.  Returns c,
    or (c, h) for the GELU epilogue (c = gelu(h), h = the bf16 pre-activation), or (c, g) for
    EPI_GELU_GRAD (g = bf16(gelu'(h)), the aux of a later EPI_MUL_AUX call).  ``drop`` (a drawn
    ``(rate, state, stream_id)``, EPI_GELU_GRAD only): c and g times keep / pk of the hidden-state
    dropout over [M, N] (``sae_gemm_nt_gelu_dropout``)."""
    lib = L.load()
    _require_gpu(a2, bt)
    M, K = a2.shape
    N = bt.shape[0]
    if bt.shape[1] != K:
        raise ValueError(f"gemm_nt: a2 {tuple(a2.shape)} and bt {tuple(bt.shape)} disagree on K")
    if bt.stride(1) != 1:
        bt = bt.contiguous()
    if out is not None:
        if out.dtype != torch.bfloat16 or out.dim() != 2 or tuple(out.shape) != (M, N) or out.stride(1) != 1:
            raise ValueError(f"gemm_nt: out must be bf16 [{M}, {N}] with unit column stride")
        c = out
    else:
        c = torch.empty((M, N), dtype=torch.bfloat16, device=a2.device)
    # the kernel writes c2 with c's row stride (ldc): give it the same layout
    two = epilogue in (EPI_GELU, EPI_GELU_GRAD)
    c2 = torch.empty_strided((M, N), (c.stride(0), 1), dtype=torch.bfloat16, device=a2.device) if two else None
    if epilogue in (EPI_DGELU, EPI_MUL_AUX):
        if aux is None or aux.dtype != torch.bfloat16 or tuple(aux.shape) != (M, N):
            raise ValueError(f"gemm_nt: the GELU-derivative epilogue needs a bf16 aux [{M}, {N}]")
    if aux is not None and aux.stride(1) != 1:
        aux = aux.contiguous()
    if bias is not None:
        bias = bias.float().contiguous()
    if drop is not None:
        if epilogue != EPI_GELU_GRAD:
            raise ValueError("gemm_nt: dropout rides in the EPI_GELU_GRAD epilogue only")
        L.check(lib.sae_gemm_nt_gelu_dropout(_stream(a2), M, N, K, _ptr(a2), a2.stride(0), _ptr(bt), bt.stride(0),
                                             _ptr(bias), _ptr(c), c.stride(0), _ptr(c2), *_drop_args(drop)))
        return c, c2
    L.check(lib.sae_gemm_nt(_stream(a2), M, N, K, _ptr(a2), a2.stride(0), _ptr(bt), bt.stride(0), _ptr(bias),
                            _ptr(c), c.stride(0), int(epilogue), _ptr(aux), aux.stride(0) if aux is not None else 0,
                            _ptr(c2)))
    return (c, c2) if two else c


class _FFBlock(torch.autograd.Function):
    """ff.py:8-34 in bf16: ``Dense_1(gelu(Dense_0(x)))`` with the GELU fused into Dense_0's GEMM
    epilogue (saving gelu'(h) of the pre-activation h, EPI_GELU_GRAD) and the product with it fused
    into the epilogue of Dense_1's input-gradient GEMM (EPI_MUL_AUX); weight / bias gradients
    through ``sae_gemm_dw``."""

    @staticmethod
    def forward(ctx, x, w0, b0, w1, b1, drop=None):
        I, Hd = w0.shape
        x2 = _pitched(x.to(torch.bfloat16).reshape(-1, I))
        w0p, w0t = _cast([w0], torch.bfloat16)
        w1p, w1t = _cast([w1], torch.bfloat16)
        gg = FF_GELU_GRAD or drop is not None   # the hidden dropout rides in the saved gelu'(h)
        a, h = gemm_nt(x2, w0t, b0, EPI_GELU_GRAD if gg else EPI_GELU, drop=drop)   # h: gelu'(pre-activation)
        y = gemm_nt(a, w1t, b1)                                   # Dense_1 forward
        ctx.save_for_backward(x2, h, a, w0p, w1p)
        ctx.gg = gg
        ctx.xshape, ctx.xdtype, ctx.has_b = x.shape, x.dtype, (b0 is not None, b1 is not None)
        ctx.sinks = [_sink(t) for t in (w0, b0, w1, b1)]
        return y.view(*x.shape[:-1], w1.shape[1])

    @staticmethod
    @_sinking
    def backward(ctx, dy):
        x2, h, a, w0p, w1p = ctx.saved_tensors
        I, Hd = w0p.shape
        O = w1p.shape[1]
        dy2 = _pitched(dy.to(torch.bfloat16).reshape(-1, O))
        dh = gemm_nt(dy2, w1p, None, EPI_MUL_AUX if ctx.gg else EPI_DGELU, aux=h)   # dA W1^T, times gelu'(h)
        sw0, sb0, sw1, sb1 = ctx.sinks   # flat-buffer sinks (multi-rank step): written in place
        dev = dy2.device
        dw1 = _grad_out(sw1, (Hd, O), dev)
        db1 = _grad_out(sb1, (O,), dev) if ctx.has_b[1] else None
        gemm_dw(a, dy2, dw1, db1, offload=sw1 is not None and (sb1 is not None or not ctx.has_b[1]))
        dx = gemm_nt(dh, w0p)                                     # dH W0^T
        dw0 = _grad_out(sw0, (I, Hd), dev)
        db0 = _grad_out(sb0, (Hd,), dev) if ctx.has_b[0] else None
        gemm_dw(x2, dh, dw0, db0, offload=sw0 is not None and (sb0 is not None or not ctx.has_b[0]))
        ret = [_unsunk(g, sk) for sk, g in zip(ctx.sinks, (dw0, db0, dw1, db1))]
        return (dx.view(ctx.xshape).to(ctx.xdtype), *ret, None)


FF_FUSED = True   # tools/ab_step.py flips this to A/B against the library GEMM + torch GELU path


def ff_block_ok(x: torch.Tensor, w0: torch.Tensor, w1: torch.Tensor) -> bool:
    if not FF_FUSED:
        return False
    I, Hd = w0.shape
    O = w1.shape[1]
    return (x.is_cuda and w0.dtype == w1.dtype == torch.float32 and I % 8 == 0 and Hd % 8 == 0 and O % 8 == 0
            and w1.shape[0] == Hd)


def ff_block(x: torch.Tensor, w0: torch.Tensor, b0: Optional[torch.Tensor], w1: torch.Tensor,
             b1: Optional[torch.Tensor], dropout=None) -> torch.Tensor:
    """Flax FFBlock (ff.py:8-34) in bf16 with fp32 params: x [.., I] -> [.., O].  ``dropout =
    (rate, DropoutRng)``: the hidden dropout after the GELU (ff.py:30), inside Dense_0's GEMM
    epilogue; the output dropout (ff.py:32) belongs to the caller's residual add."""
    _require_gpu(x, w0, w1)
    return _FFBlock.apply(x, w0, b0, w1, b1, _draw(dropout))


# ------------------------------------------------------------------ residual add + LayerNorm
LN_EPS = 1e-6   # Flax nn.LayerNorm default (models/vit.py:19,26,57)


def layer_norm_ok(x: torch.Tensor) -> bool:
    """The fused kernels cover the encoder's fp32 residual stream with C % 4 == 0, C <= 1024."""
    C = x.shape[-1]
    return x.is_cuda and x.dtype == torch.float32 and C % 4 == 0 and C <= 1024 and x.is_contiguous()


def _f32c(t: torch.Tensor) -> torch.Tensor:
    """fp32 contiguous view/copy of a LayerNorm operand (the kernels read raw fp32)."""
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def _bf16c(t: torch.Tensor) -> torch.Tensor:
    """bf16 contiguous copy of a LayerNorm operand (the kernels read raw bf16)."""
    if t.dtype != torch.bfloat16:
        t = t.to(torch.bfloat16)
    return t if t.is_contiguous() else t.contiguous()


class _LnScale(NamedTuple):
    """The scaled (CaiT) form of the residual add, ``x + delta * bf16(ls[c]) * rowscale[row // rpb]``."""
    ls: torch.Tensor                       # fp32 contiguous copy of the LayerScale parameter
    rowscale: Optional[torch.Tensor]       # fp32 [B], or None
    rpb: int                               # rows per sample
    delta: Optional[torch.Tensor] = None   # backward: the bf16 addend the forward read
    sink: Optional[torch.Tensor] = None    # backward: the LayerScale gradient's sink


def _ln_fwd(x, delta, gamma, beta, eps, drop=None, rows=(0, 1), scaled: Optional[_LnScale] = None):
    """sae_layernorm_fwd, its dropout form (the addend dropped as it is added, with the mask of rows
    rows[0] + i * rows[1]) or its scaled form -> ``(x + delta, y, mean, rstd)``; without an addend the
    first is None."""
    if drop is not None and scaled is not None:
        raise NotImplementedError("layer norm: the dropout form has no LayerScale")
    lib = L.load()
    x, gamma, beta = _f32c(x), _f32c(gamma), _f32c(beta)
    if delta is not None:
        delta = _bf16c(delta)
    C = x.shape[-1]
    M = x.numel() // C
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    mean = torch.empty(M, dtype=torch.float32, device=x.device)
    rstd = torch.empty(M, dtype=torch.float32, device=x.device)
    xout = torch.empty_like(x) if delta is not None else None
    args = (_stream(x), M, C, _ptr(x), _ptr(delta), _ptr(xout), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(mean),
            _ptr(rstd), float(eps))
    if drop is not None:
        L.check(lib.sae_layernorm_fwd_dropout(*args, *_drop_args(drop), int(rows[0]), int(rows[1])))
    elif scaled is not None:
        L.check(lib.sae_layernorm_fwd_scaled(*args, _ptr(scaled.ls), _ptr(scaled.rowscale), int(scaled.rpb)))
    else:
        L.check(lib.sae_layernorm_fwd(*args))
    return xout, y, mean, rstd


def _ln_bwd(xs, mean, rstd, gamma, dy, dxin, want_ddelta, sinks=(None, None), drop=None, rows=(0, 1),
            scaled: Optional[_LnScale] = None):
    """sae_layernorm_bwd, its dropout form (ddelta = bf16(dx * keep / pk): the forward's mask) or its
    scaled form -> ``(dx, ddelta, dgamma, dbeta, dlayerscale)``; ``dxin`` (the residual stream's
    gradient, added into dx) may be None, ddelta is None unless wanted, dlayerscale unless scaled."""
    if drop is not None and scaled is not None:
        raise NotImplementedError("layer norm: the dropout form has no LayerScale")
    lib = L.load()
    C = xs.shape[-1]
    M = xs.numel() // C
    xs, gamma = _f32c(xs), _f32c(gamma)
    dy = _bf16c(dy)
    dx = torch.empty_like(xs)
    ddelta = torch.empty(xs.shape, dtype=torch.bfloat16, device=xs.device) if want_ddelta else None
    dg = _grad_out(sinks[0], (C,), xs.device)
    db = _grad_out(sinks[1], (C,), xs.device)
    dls = _grad_out(scaled.sink, (C,), xs.device) if scaled is not None else None
    ws = torch.empty(lib.sae_layernorm_bwd_workspace_bytes(M, C), dtype=torch.uint8, device=xs.device)
    if dxin is not None:
        dxin = _f32c(dxin)
    args = (_stream(xs), M, C, _ptr(xs), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(dy), _ptr(dxin), _ptr(dx),
            _ptr(ddelta), _ptr(dg), _ptr(db), _ptr(ws))
    if drop is not None:
        L.check(lib.sae_layernorm_bwd_dropout(*args, *_drop_args(drop), int(rows[0]), int(rows[1])))
    elif scaled is not None:
        L.check(lib.sae_layernorm_bwd_scaled(*args, _ptr(scaled.delta), _ptr(scaled.ls), _ptr(scaled.rowscale),
                                             int(scaled.rpb), _ptr(dls)))
    else:
        L.check(lib.sae_layernorm_bwd(*args))
    return dx, ddelta, dg, db, dls


def _cls_rows(rows: torch.Tensor, shape, dtype) -> torch.Tensor:
    """Zeros of ``shape`` [B, N, E] whose class-token rows [:, 0] are ``rows`` [B, E]."""
    out = torch.zeros(shape, dtype=dtype, device=rows.device)
    out[:, 0] = rows
    return out


class _LayerNorm(torch.autograd.Function):
    """The one LayerNorm of the fp32 residual stream: ``(stream, y)`` with y = LN(stream) in bf16 and
    stream = x, or x + delta for a bf16 addend (dropped as it is added under ``drop``; times
    ``ls[c] * rowscale[sample]``, the CaiT blocks' LayerScale and stochastic-depth factor, when ``ls`` is
    given).  Returning the stream lets the backward add the residual gradient inside the LayerNorm
    backward kernel (dx = dstream + LN'^T dy) instead of autograd summing the two paths in a separate
    pass; a caller that has no use for it says ``stream=False`` and gets None in its place, and the
    kernel then runs with dxin = NULL.  ``cls``: the class-token rows of x, delta [B, N, E] only -> y
    [B, E] (ViT's head reads token 0, vit.py:95; LayerNorm is row-wise, so those rows' values equal the
    full pass's, and under dropout they take their slice, rows b * N, of the full tensor's mask); the
    backward writes the class rows of dx and ddelta, the other rows take no gradient from here."""

    @staticmethod
    def forward(ctx, x, delta, gamma, beta, ls, rowscale, eps, drop, cls, stream):
        ctx.full_shape, ctx.rows = (x.shape, (0, x.shape[1])) if cls else (None, (0, 1))
        ctx.delta_dtype, ctx.ls_dtype = (None if t is None else t.dtype for t in (delta, ls))
        scaled = None
        if ls is not None:
            # the reference casts the LayerScale parameter to the compute dtype (layerscale.py:22): the
            # kernels round the fp32 parameter to bf16 as they load it (no cast launches here)
            scaled = _LnScale(_f32c(ls.detach()), rowscale, x.shape[1])
        xin, din = (x[:, 0], delta[:, 0]) if cls else (x, delta)
        if din is not None:
            din = _bf16c(din)
        xout, y, mean, rstd = _ln_fwd(xin, din, gamma, beta, eps, drop, ctx.rows, scaled)
        xs = xin if din is None else xout
        ctx.save_for_backward(xs, mean, rstd, gamma, *(() if scaled is None else (din, scaled.ls, rowscale)))
        ctx.drop = drop
        ctx.sinks = (_sink(gamma), _sink(beta), _sink(ls) if ctx.ls_dtype == torch.float32 else None)
        return (xs if stream else None), y

    @staticmethod
    @_sinking
    def backward(ctx, dstream, dy):
        # autograd hands an unused tensor output's gradient over as zeros (y unused: dx = 0 * rstd +
        # dstream) and None for the stream that was not returned
        xs, mean, rstd, gamma, *rest = ctx.saved_tensors
        sg, sb, sls = ctx.sinks
        scaled = _LnScale(rest[1], rest[2], xs.shape[1], rest[0], sls) if rest else None
        dx, ddelta, dg, db, dls = _ln_bwd(xs, mean, rstd, gamma, dy, dstream, ctx.delta_dtype is not None, (sg, sb),
                                          ctx.drop, ctx.rows, scaled)
        if ctx.full_shape is not None:
            dx, ddelta = _cls_rows(dx, ctx.full_shape, dx.dtype), _cls_rows(ddelta, ctx.full_shape, ctx.delta_dtype)
        if ddelta is not None:
            ddelta = ddelta.to(ctx.delta_dtype)
        if dls is not None:
            dls = _unsunk(dls.to(ctx.ls_dtype), sls)
        return dx, ddelta, _unsunk(dg, sg), _unsunk(db, sb), dls, None, None, None, None, None


def layer_norm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = LN_EPS) -> torch.Tensor:
    """Flax ``nn.LayerNorm(dtype=bfloat16)`` of an fp32 residual stream: bf16 output (HIP kernel)."""
    _require_gpu(x)
    return _LayerNorm.apply(x, None, gamma, beta, None, None, eps, None, False, False)[1]


def layer_norm_pass(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = LN_EPS):
    """``(x, LayerNorm(x))``: the encoder's first LayerNorm, returning its input as the residual stream
    (see _LayerNorm)."""
    _require_gpu(x, gamma, beta)
    return _LayerNorm.apply(x, None, gamma, beta, None, None, eps, None, False, True)


def add_layer_norm(x: torch.Tensor, delta: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                   eps: float = LN_EPS, dropout=None):
    """``x + delta`` (fp32 residual add, models/vit.py:24,31) and its LayerNorm in bf16, one kernel;
    returns ``(x + delta, LN(x + delta))``.  ``dropout = (rate, DropoutRng)``: the hidden dropout of
    the addend (the attention-output / FF-output dropout of vit.py:22,29) applied as it is added,
    ``x + delta * keep / pk``."""
    _require_gpu(x, delta)
    return _LayerNorm.apply(x, delta, gamma, beta, None, None, eps, _draw(dropout), False, True)


def add_layer_norm_scaled(x: torch.Tensor, delta: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                          layerscale: torch.Tensor, rowscale: Optional[torch.Tensor] = None,
                          eps: float = LN_EPS):
    """CaiT residual add ``x + delta * layerscale * rowscale[sample]`` (layerscale.py:21-23 and the
    stochastic-depth factor mask / keep, stochastic_depth.py:19-28) with its LayerNorm, one kernel;
    returns ``(x_out, LN(x_out))``.  ``rowscale`` [B] fp32 or None; x [B, N, C] fp32."""
    _require_gpu(x, delta)
    if rowscale is not None:
        rowscale = rowscale.float().contiguous()
    return _LayerNorm.apply(x, delta, gamma, beta, layerscale, rowscale, eps, None, False, True)


def cls_add_layer_norm(x: torch.Tensor, delta: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                       eps: float = LN_EPS, dropout=None) -> torch.Tensor:
    """bf16 LayerNorm(x[:, 0] + delta[:, 0]) of the [B, N, E] residual stream: the encoder's final
    residual add and LayerNorm on the class-token rows only (see _LayerNorm).  ``dropout``: as
    :func:`add_layer_norm`, with the class rows' slice of the full tensor's mask."""
    _require_gpu(x, delta, gamma, beta)
    return _LayerNorm.apply(x, delta, gamma, beta, None, None, eps, _draw(dropout), True, False)[1]


# ------------------------------------------------------------------------------ training loss
class _CrossEntropy(torch.autograd.Function):
    """The training loss: label-smoothed softmax cross entropy, mean over rows (train.py:77-90:
    optax.smooth_labels + jnp.mean(optax.softmax_cross_entropy)) against the targets ``ratio
    onehot(labels) + (1 - ratio) onehot(mix_labels)`` -- ``mix_labels`` / ``ratio`` None: one label per
    row, the plain smoothed loss -- and, with ``metrics``, the top-1 / top-5 fractions of
    utils.topk_correct from the same pass.  Three HIP launches (sae_mixed_ce_fwd / _bwd); dlogits come
    back in the logits' dtype.  Returns ``(loss, top, row_loss, rank)``: only the loss is
    differentiable; ``top`` [2], ``row_loss`` [R] and ``rank`` [R] feed the metrics and the evaluation
    accumulator (``top`` / ``rank`` empty without metrics)."""

    @staticmethod
    def forward(ctx, logits, labels, mix_labels, ratio, alpha, metrics):
        lib = L.load()
        R, K = logits.shape
        dev = logits.device
        lse = torch.empty(R, dtype=torch.float32, device=dev)
        row_loss = torch.empty(R, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        rank = torch.empty(R if metrics else 0, dtype=torch.int32, device=dev)
        top = torch.empty(2 if metrics else 0, dtype=torch.float32, device=dev)
        L.check(lib.sae_mixed_ce_fwd(_stream(logits), R, K, _ptr(logits), logits.stride(0), dtype_code(logits.dtype),
                                     _ptr(labels), _ptr(mix_labels), _ptr(ratio), float(alpha), _ptr(lse),
                                     _ptr(row_loss), _ptr(rank) if metrics else None, _ptr(loss),
                                     _ptr(top) if metrics else None))
        ctx.save_for_backward(logits, labels, lse, *(() if mix_labels is None else (mix_labels, ratio)))
        ctx.alpha = float(alpha)
        ctx.mark_non_differentiable(top, row_loss, rank)
        return loss, top, row_loss, rank

    @staticmethod
    @_sinking
    def backward(ctx, gloss, *_unused):
        lib = L.load()
        logits, labels, lse, *mix = ctx.saved_tensors
        mix_labels, ratio = mix if mix else (None, None)
        R, K = logits.shape
        g = gloss.float().contiguous()
        dx = torch.empty((R, K), dtype=logits.dtype, device=logits.device)
        L.check(lib.sae_mixed_ce_bwd(_stream(logits), R, K, _ptr(logits), logits.stride(0), dtype_code(logits.dtype),
                                     _ptr(labels), _ptr(mix_labels), _ptr(ratio), ctx.alpha, _ptr(lse), _ptr(g),
                                     _ptr(dx), dx.stride(0)))
        return dx, None, None, None, None, None


def _ce_args(logits, labels, mix_labels, ratio):
    """What the loss kernels take: GPU logits as [R, K] rows of unit column stride (a row-strided view
    is read in place), int64 labels [R] and, together or not at all, int64 ``mix_labels`` [R] and
    fp32 ``ratio`` [R]."""
    _require_gpu(logits, labels, mix_labels, ratio)
    if (mix_labels is None) != (ratio is None):
        raise ValueError("mixed_cross_entropy: mix_labels and ratio go together (both or neither)")
    if logits.dim() != 2 or logits.stride(1) != 1:
        logits = logits.reshape(-1, logits.shape[-1]).contiguous()
    R = logits.shape[0]
    labels = labels.to(torch.int64).contiguous()
    if mix_labels is not None:
        mix_labels = mix_labels.to(torch.int64).contiguous()
        ratio = ratio.to(torch.float32).contiguous()
        if mix_labels.numel() != R or ratio.numel() != R:
            raise ValueError(f"mixed_cross_entropy: mix_labels / ratio need one entry per row ({R})")
    if labels.numel() != R:
        raise ValueError(f"mixed_cross_entropy: labels need one entry per row ({R})")
    return logits, labels, mix_labels, ratio


def mixed_cross_entropy_rows(logits, labels, mix_labels=None, ratio=None, alpha=0.1, metrics=True):
    """``mixed_cross_entropy`` with its per-row results: ``(loss, top [2], row_loss [R], rank [R])``, what
    the evaluation accumulator (``ce_accumulate``) and ``train.topk_correct`` read."""
    return _CrossEntropy.apply(*_ce_args(logits, labels, mix_labels, ratio), alpha, bool(metrics))


def mixed_cross_entropy(logits: torch.Tensor, labels: torch.Tensor, mix_labels: Optional[torch.Tensor] = None,
                        ratio: Optional[torch.Tensor] = None, alpha: float = 0.1, metrics: bool = False):
    """The smoothed cross entropy of [R, K] GPU logits (bf16 or fp32) against the targets
    ``ratio onehot(labels) + (1 - ratio) onehot(mix_labels)`` (``mix_labels`` int [R], ``ratio`` float
    [R]; both None: one label per row, ``smoothed_cross_entropy``).  ``metrics=True``
    returns ``(loss, top1, top5)``: the fractions of rows whose first label is among the 1 / 5 largest
    logits in stable-argsort order (0-d device tensors, not differentiable)."""
    loss, top, _, _ = mixed_cross_entropy_rows(logits, labels, mix_labels, ratio, alpha, metrics)
    return (loss, top[0], top[1]) if metrics else loss


def smoothed_cross_entropy(logits: torch.Tensor, labels: torch.Tensor, alpha: float = 0.1) -> torch.Tensor:
    """mean_r [lse_r - (1 - alpha) x[r, y_r] - (alpha / K) sum_c x[r, c]] of [R, K] GPU logits (bf16 or
    fp32) against int64 labels [R]: ``mixed_cross_entropy`` with one label per row."""
    return mixed_cross_entropy(logits, labels, alpha=alpha)


def ce_accumulate(row_loss: torch.Tensor, rank: torch.Tensor, acc: torch.Tensor) -> None:
    """Add one batch's ``row_loss`` (fp32 [R]) and ``rank`` (int32 [R]) into the evaluation accumulator
    ``acc`` (4 x int64 on the GPU holding {double loss_sum; int64 top1, top5, samples}:
    ``sae_ce_accumulate``), on the current stream."""
    _require_gpu(row_loss, rank, acc)
    if (acc.dtype != torch.int64 or acc.numel() * 8 != L.SAE_CE_ACCUM_BYTES or not acc.is_contiguous()
            or row_loss.dtype != torch.float32 or rank.dtype != torch.int32 or rank.numel() != row_loss.numel()
            or not row_loss.is_contiguous() or not rank.is_contiguous()):
        raise ValueError("ce_accumulate: row_loss fp32 [R], rank int32 [R], acc int64 [4], all contiguous")
    L.check(L.load().sae_ce_accumulate(_stream(row_loss), row_loss.numel(), _ptr(row_loss), _ptr(rank), _ptr(acc)))


def ce_accumulator_fields(acc: torch.Tensor):
    """The two fields of an evaluation accumulator (int64 [4] holding {double loss_sum; int64 top1,
    top5, samples}) as views of it: ``(loss_sum float64 [1], counts int64 [3])``.  The one place
    that knows the layout on the Python side."""
    return acc[:1].view(torch.float64), acc[1:]


def read_ce_accumulator(acc: torch.Tensor):
    """``(loss_sum, top1, top5, samples)`` of an evaluation accumulator, on the host (one sync)."""
    loss_sum, counts = ce_accumulator_fields(acc.cpu())
    return (float(loss_sum[0]), *(int(c) for c in counts))


# ------------------------------------------------------------------------ encoder input tokens
class _EncoderTokens(torch.autograd.Function):
    """concat(cls, float(tokens)) + pos (models/vit.py:82-85,46; position_embed.py:48) in one HIP
    pass each way (sae_tokens_fwd / _bwd); cls / pos gradients go into their sinks when the
    multi-rank step registered them."""

    @staticmethod
    def forward(ctx, tokens, cls, pos, drop=None):
        lib = L.load()
        B, Lt, E = tokens.shape
        x = torch.empty((B, Lt + 1, E), dtype=torch.float32, device=tokens.device)
        if drop is not None:
            L.check(lib.sae_tokens_fwd_dropout(_stream(tokens), B, Lt, E, _ptr(tokens), _ptr(cls), _ptr(pos), _ptr(x),
                                               *_drop_args(drop)))
        else:
            L.check(lib.sae_tokens_fwd(_stream(tokens), B, Lt, E, _ptr(tokens), _ptr(cls), _ptr(pos), _ptr(x)))
        ctx.shape, ctx.drop = (B, Lt, E), drop
        ctx.sinks = (_sink(cls), _sink(pos))
        ctx.meta = (cls.shape, pos.shape)
        return x

    @staticmethod
    @_sinking
    def backward(ctx, dx):
        lib = L.load()
        B, Lt, E = ctx.shape
        dx = _f32c(dx)
        dtok = torch.empty((B, Lt, E), dtype=torch.bfloat16, device=dx.device)
        scls, spos = ctx.sinks
        dcls = _grad_out(scls, ctx.meta[0], dx.device)
        dpos = _grad_out(spos, ctx.meta[1], dx.device)
        if ctx.drop is not None:
            L.check(lib.sae_tokens_bwd_dropout(_stream(dx), B, Lt, E, _ptr(dx), _ptr(dtok), _ptr(dcls), _ptr(dpos),
                                               *_drop_args(ctx.drop)))
        else:
            L.check(lib.sae_tokens_bwd(_stream(dx), B, Lt, E, _ptr(dx), _ptr(dtok), _ptr(dcls), _ptr(dpos)))
        return dtok, _unsunk(dcls, scls), _unsunk(dpos, spos), None


def encoder_tokens_ok(tokens: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor) -> bool:
    """Inputs sae_tokens_fwd takes: bf16 [B, L, E] tokens, fp32 contiguous cls [.., E] and pos [1, L+1, E]."""
    if not (tokens.is_cuda and tokens.dtype == torch.bfloat16 and tokens.dim() == 3 and tokens.is_contiguous()):
        return False
    B, Lt, E = tokens.shape
    return (E % 4 == 0 and E <= 4096 and tokens.data_ptr() % 8 == 0
            and cls.dtype == torch.float32 and cls.is_contiguous() and cls.numel() == E and cls.data_ptr() % 16 == 0
            and pos.dtype == torch.float32 and pos.is_contiguous() and pos.numel() == (Lt + 1) * E
            and pos.data_ptr() % 16 == 0)


def encoder_tokens(tokens: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, dropout=None) -> torch.Tensor:
    """fp32 [B, L+1, E] encoder input = concat(cls, float(tokens)) + pos (see _EncoderTokens).
    ``dropout = (rate, DropoutRng)``: the encoder-input dropout of vit.py:47 in the same pass."""
    _require_gpu(tokens, cls, pos)
    if not encoder_tokens_ok(tokens, cls, pos):
        raise ValueError("encoder_tokens: needs bf16 contiguous tokens [B, L, E] (E % 4 == 0) and fp32 "
                         "contiguous cls [E] / pos [L+1, E]")
    return _EncoderTokens.apply(tokens, cls, pos, _draw(dropout))


# ------------------------------------------------- CvT projection: depthwise 3x3 conv + BatchNorm
def same_pads(n: int, k: int, s: int) -> Tuple[int, int]:
    """Flax ``SAME`` padding (low, high) of an axis of length ``n`` for kernel ``k``, stride ``s``:
    output ceil(n / s), total max((out - 1) s + k - n, 0), the smaller half in front."""
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return total // 2, total - total // 2


def dwconv_bn_ok(x, kernel_size: int, stride: int, dtype: torch.dtype, training: bool = True,
                 needs_grad: Optional[bool] = None) -> bool:
    """Host predicate of :func:`dwconv_bn` (``sae_dwconv_bn_*``): a GPU tensor [B, H, W, C], a 3 x 3
    kernel, stride 1 or 2, bf16 with C % 8 == 0 or fp32 with C % 4 == 0.  The evaluation form has no
    backward: with a gradient wanted (``needs_grad``; default: ``x.requires_grad`` under grad mode)
    it is not taken."""
    if not getattr(x, "is_cuda", False) or len(x.shape) != 4:
        return False
    if kernel_size != 3 or stride not in (1, 2) or dtype not in (torch.bfloat16, torch.float32):
        return False
    if x.shape[-1] % (8 if dtype == torch.bfloat16 else 4) or min(x.shape) < 1:
        return False
    if x.shape[0] * x.shape[1] * x.shape[2] > 1 << 30:
        return False
    if needs_grad is None:
        needs_grad = torch.is_grad_enabled() and bool(x.requires_grad)
    return bool(training) or not needs_grad


def _dwconv_desc(x, stride, momentum, eps, training) -> L.SaeDwconvDesc:
    B, H, W, C = x.shape
    return L.SaeDwconvDesc(B, H, W, C, int(stride), dtype_code(x.dtype), 1 if training else 0, float(momentum),
                           float(eps))


class _DwConvBn(torch.autograd.Function):
    """``sae_dwconv_bn_fwd`` / ``_bwd``: saves the conv output t and the batch mean / rstd; the running
    buffers are advanced by the forward's kernels (stream-ordered, no host read)."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, run_mean, run_var, stride, momentum, eps, training):
        lib = L.load()
        B, H, W, C = x.shape
        d = _dwconv_desc(x, stride, momentum, eps, training)
        Ho, Wo = -(-H // stride), -(-W // stride)
        y = torch.empty((B, Ho, Wo, C), dtype=x.dtype, device=x.device)
        t = mean = rstd = ws = None
        if training:
            t = torch.empty_like(y)
            mean = torch.empty(C, dtype=torch.float32, device=x.device)
            rstd = torch.empty(C, dtype=torch.float32, device=x.device)
            ws = torch.empty(lib.sae_dwconv_bn_workspace_bytes(B, H, W, C, int(stride)), dtype=torch.uint8,
                             device=x.device)
        tok = _TIMER.begin("dwconv_bn_fwd") if _TIMER is not None else None
        L.check(lib.sae_dwconv_bn_fwd(_stream(x), ctypes.byref(d), _ptr(x), _ptr(w), _ptr(gamma), _ptr(beta),
                                      _ptr(run_mean), _ptr(run_var), _ptr(t), _ptr(y), _ptr(mean), _ptr(rstd),
                                      _ptr(ws)))
        if tok is not None:
            _TIMER.end(tok, (B, H, W, C, stride))
        ctx.training = training
        if training:
            ctx.save_for_backward(x, w, gamma, t, mean, rstd)
            ctx.desc = d
        return y

    @staticmethod
    def backward(ctx, dy):
        if not ctx.training:
            raise RuntimeError("dwconv_bn: the evaluation form has no backward (dwconv_bn_ok refuses it)")
        lib = L.load()
        x, w, gamma, t, mean, rstd = ctx.saved_tensors
        d = ctx.desc
        B, H, W, C = x.shape
        dy = dy.to(x.dtype).contiguous()
        dx = torch.empty_like(x)
        dw = torch.empty((3, 3, 1, C), dtype=torch.float32, device=x.device)
        dg = torch.empty(C, dtype=torch.float32, device=x.device)
        db = torch.empty(C, dtype=torch.float32, device=x.device)
        ws = torch.empty(lib.sae_dwconv_bn_workspace_bytes(B, H, W, C, d.stride), dtype=torch.uint8, device=x.device)
        tok = _TIMER.begin("dwconv_bn_bwd") if _TIMER is not None else None
        L.check(lib.sae_dwconv_bn_bwd(_stream(x), ctypes.byref(d), _ptr(x), _ptr(w), _ptr(gamma), _ptr(t), _ptr(mean),
                                      _ptr(rstd), _ptr(dy), _ptr(dx), _ptr(dw), _ptr(dg), _ptr(db), _ptr(ws)))
        if tok is not None:
            _TIMER.end(tok, (B, H, W, C, d.stride))
        return dx, dw, dg, db, None, None, None, None, None, None


def dwconv_bn(x: torch.Tensor, w: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, run_mean: torch.Tensor,
              run_var: torch.Tensor, stride: int, momentum: float, eps: float, training: bool,
              dtype: torch.dtype) -> torch.Tensor:
    """Depthwise 3 x 3 convolution (Flax SAME padding, ``stride`` 1 or 2) + BatchNorm of ``x``
    [B, H, W, C] in the compute dtype ``dtype`` -> [B, ceil(H / s), ceil(W / s), C]
    (cvt_attention.py:21-36).  ``w`` is the Flax depthwise kernel [3, 3, 1, C] (fp32; used at
    ``dtype``), ``gamma`` / ``beta`` the BatchNorm scale / bias, ``run_mean`` / ``run_var`` its fp32
    batch_stats buffers: training normalises with the biased batch statistics and moves the buffers in
    place (ra = momentum * ra + (1 - momentum) * batch), evaluation reads them.  Gradients of x, w,
    gamma, beta.  No host synchronisation: the call can be captured into a graph."""
    _require_gpu(x, w, gamma, beta, run_mean, run_var)
    if not dwconv_bn_ok(x, w.shape[0], stride, dtype):
        raise ValueError(f"dwconv_bn: unsupported call (x {tuple(x.shape)}, kernel {tuple(w.shape)}, stride {stride}, "
                         f"{dtype}); see dwconv_bn_ok")
    if run_mean.dtype != torch.float32 or run_var.dtype != torch.float32 or not run_mean.is_contiguous() \
            or not run_var.is_contiguous():
        raise ValueError("dwconv_bn: run_mean / run_var must be contiguous fp32 buffers (they are updated in place)")
    x = x.to(dtype)
    x = x if x.is_contiguous() else x.contiguous()
    return _DwConvBn.apply(x, _f32c(w), _f32c(gamma), _f32c(beta), run_mean, run_var, int(stride),
                           float(momentum), float(eps), bool(training))


# ------------------------------------------- CeiT LeFF: BatchNorm over token rows + tanh-GELU
def bn_gelu_ok(x, dtype: torch.dtype, training: bool = True, needs_grad: Optional[bool] = None,
               x_lead: int = 0) -> bool:
    """Host predicate of :func:`bn_gelu` (``sae_bn_gelu_*``): a GPU tensor [B, L + x_lead, C] with
    B, L >= 1, bf16 with C % 8 == 0 or fp32 with C % 4 == 0, and B (L + 1) C < 2^31 (element offsets of
    either layout fit 31 bits).  The evaluation form has no backward: with a gradient wanted
    (``needs_grad``; default: ``x.requires_grad`` under grad mode) it is not taken."""
    if not getattr(x, "is_cuda", False) or len(x.shape) != 3 or x_lead not in (0, 1):
        return False
    if dtype not in (torch.bfloat16, torch.float32):
        return False
    B, R, C = x.shape
    if B < 1 or R - x_lead < 1 or C < 1 or C % (8 if dtype == torch.bfloat16 else 4):
        return False
    if B * (R - x_lead + 1) * C >= 2 ** 31:
        return False
    if needs_grad is None:
        needs_grad = torch.is_grad_enabled() and bool(x.requires_grad)
    return bool(training) or not needs_grad


def _aligned_rows(t: torch.Tensor) -> torch.Tensor:
    """``t`` as a contiguous, 16-byte-aligned tensor (itself when it already is one)."""
    if not t.is_contiguous():
        t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


class _BnGelu(torch.autograd.Function):
    """``sae_bn_gelu_fwd`` / ``_bwd``: saves x and the batch mean / rstd, nothing else (z is recomputed);
    the running buffers are advanced by the forward's kernels (stream-ordered, no host read)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, lead, run_mean, run_var, momentum, eps, training, x_lead, y_lead):
        lib = L.load()
        B, R, C = x.shape
        Lt = R - x_lead
        d = L.SaeBnrowsDesc(B, Lt, C, x_lead, y_lead, dtype_code(x.dtype), 1 if training else 0, float(momentum),
                            float(eps))
        y = torch.empty((B, Lt + y_lead, C), dtype=x.dtype, device=x.device)
        mean = rstd = ws = None
        if training:
            mean = torch.empty(C, dtype=torch.float32, device=x.device)
            rstd = torch.empty(C, dtype=torch.float32, device=x.device)
            ws = torch.empty(lib.sae_bn_gelu_workspace_bytes(B, Lt, C), dtype=torch.uint8, device=x.device)
        tok = _TIMER.begin("bn_gelu_fwd") if _TIMER is not None else None
        L.check(lib.sae_bn_gelu_fwd(_stream(x), ctypes.byref(d), _ptr(x), _ptr(gamma), _ptr(beta), _ptr(run_mean),
                                    _ptr(run_var), _ptr(lead), lead.stride(0) if lead is not None else 0, _ptr(y),
                                    _ptr(mean), _ptr(rstd), _ptr(ws)))
        if tok is not None:
            _TIMER.end(tok, (B, Lt, C, x_lead, y_lead))
        ctx.training = training
        if training:
            ctx.save_for_backward(x, gamma, beta, mean, rstd)
            ctx.desc = d
        return y

    @staticmethod
    def backward(ctx, dy):
        if not ctx.training:
            raise RuntimeError("bn_gelu: the evaluation form has no backward (bn_gelu_ok refuses it)")
        lib = L.load()
        x, gamma, beta, mean, rstd = ctx.saved_tensors
        d = ctx.desc
        B, _, C = x.shape
        dy = _aligned_rows(dy.to(x.dtype))
        dx = torch.empty_like(x)   # (its skipped lead rows are written as zeros by the kernel)
        dg = torch.empty(C, dtype=torch.float32, device=x.device)
        db = torch.empty(C, dtype=torch.float32, device=x.device)
        ws = torch.empty(lib.sae_bn_gelu_workspace_bytes(B, d.tokens, C), dtype=torch.uint8, device=x.device)
        tok = _TIMER.begin("bn_gelu_bwd") if _TIMER is not None else None
        L.check(lib.sae_bn_gelu_bwd(_stream(x), ctypes.byref(d), _ptr(x), _ptr(gamma), _ptr(beta), _ptr(mean),
                                    _ptr(rstd), _ptr(dy), _ptr(dx), _ptr(dg), _ptr(db), _ptr(ws)))
        if tok is not None:
            _TIMER.end(tok, (B, d.tokens, C, d.x_lead, d.y_lead))
        dlead = dy[:, :1] if d.y_lead and ctx.needs_input_grad[3] else None   # a view: no kernel
        return dx, dg, db, dlead, None, None, None, None, None, None, None


def bn_gelu(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, run_mean: torch.Tensor, run_var: torch.Tensor,
            momentum: float, eps: float, training: bool, dtype: torch.dtype, x_lead: int = 0, y_lead: int = 0,
            lead: Optional[torch.Tensor] = None) -> torch.Tensor:
    """BatchNorm over the token rows followed by the tanh-GELU (leff.py:40-41, 52-53, 58-59) of ``x``
    [B, L + x_lead, C] in the compute dtype ``dtype`` -> [B, L + y_lead, C].  ``x_lead`` (0 or 1)
    leading rows per sample -- the class token -- take no part and are not read; with ``y_lead = 1``
    row 0 of every sample of the output is ``lead`` ([B, 1, C] or [B, C], e.g. ``inputs[:, :1]``: a view
    is read in place through its sample stride), so the last BatchNorm of the block writes the
    concatenated output.  ``gamma`` / ``beta`` are the BatchNorm scale / bias, ``run_mean`` /
    ``run_var`` its fp32 batch_stats buffers: training normalises with the biased batch statistics and
    moves the buffers in place (ra = momentum * ra + (1 - momentum) * batch), evaluation reads them.
    Gradients of x (zero in its lead rows), gamma, beta and lead.  No host synchronisation: the call
    can be captured into a graph."""
    _require_gpu(x, gamma, beta, run_mean, run_var, lead)
    x_lead, y_lead = int(x_lead), int(y_lead)
    if not bn_gelu_ok(x, dtype, x_lead=x_lead) or y_lead not in (0, 1):
        raise ValueError(f"bn_gelu: unsupported call (x {tuple(x.shape)}, x_lead {x_lead}, y_lead {y_lead}, {dtype}); "
                         "see bn_gelu_ok")
    if run_mean.dtype != torch.float32 or run_var.dtype != torch.float32 or not run_mean.is_contiguous() \
            or not run_var.is_contiguous():
        raise ValueError("bn_gelu: run_mean / run_var must be contiguous fp32 buffers (they are updated in place)")
    B, _, C = x.shape
    if (lead is not None) != bool(y_lead):
        raise ValueError("bn_gelu: lead is given exactly when y_lead = 1")
    if lead is not None:
        if tuple(lead.shape) not in ((B, 1, C), (B, C)):
            raise ValueError(f"bn_gelu: lead must be [{B}, 1, {C}] or [{B}, {C}], got {tuple(lead.shape)}")
        lead = lead.to(dtype).reshape(B, 1, C) if lead.dim() == 2 else lead.to(dtype)
        V = 8 if dtype == torch.bfloat16 else 4
        if lead.stride(2) != 1 or lead.stride(0) % V or lead.data_ptr() % 16:
            lead = _aligned_rows(lead)
    x = _aligned_rows(x.to(dtype))
    return _BnGelu.apply(x, _f32c(gamma), _f32c(beta), lead, run_mean, run_var, float(momentum), float(eps),
                         bool(training), x_lead, y_lead)


# --------------------------------------------- CvT token embedding: k x k convolution, stride < k
def _convtok_desc(shape, kernel_size: int, stride: int, in_dtype: torch.dtype, dtype: torch.dtype) -> L.SaeConvtokDesc:
    B, H, W, C = shape
    return L.SaeConvtokDesc(int(B), int(H), int(W), int(C), int(kernel_size), int(stride), dtype_code(in_dtype),
                            dtype_code(dtype))


def conv_window_cols(channels: int, kernel_size: int) -> int:
    """Columns of the window matrix: ``kernel_size^2 * channels`` rounded up to a multiple of 8."""
    return -(-(kernel_size * kernel_size * channels) // 8) * 8


def conv_window_matrix(x: torch.Tensor, kernel_size: int, stride: int, dtype: torch.dtype) -> torch.Tensor:
    """The window matrix ``P`` [B * Ho * Wo, Kp] of ``x`` [B, H, W, Cin] (bf16 or fp32, contiguous) in
    the compute dtype ``dtype`` (``sae_conv_window_gather``): row (b, oy, ox), column
    ``(ky * k + kx) * Cin + c`` holds ``x[b, oy * s - pad_top + ky, ox * s - pad_left + kx, c]`` with the
    Flax SAME pads of :func:`same_pads`; taps outside the image and the columns past ``k * k * Cin``
    are zero.  fp32 values are rounded to bf16 as they are staged."""
    lib = L.load()
    _require_gpu(x)
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError("conv_window_matrix: x must be a contiguous [B, H, W, Cin] tensor")
    d = _convtok_desc(x.shape, kernel_size, stride, x.dtype, dtype)
    B, H, W, C = x.shape
    M = B * -(-H // stride) * -(-W // stride)
    P = torch.empty((M, conv_window_cols(C, kernel_size)), dtype=dtype, device=x.device)
    tok = _TIMER.begin("conv_window_gather") if _TIMER is not None else None
    L.check(lib.sae_conv_window_gather(_stream(x), ctypes.byref(d), _ptr(x), _ptr(P)))
    if tok is not None:
        _TIMER.end(tok, (M, P.shape[1]))
    return P


def conv_window_scatter(dP: torch.Tensor, x_shape, kernel_size: int, stride: int) -> torch.Tensor:
    """The transpose of :func:`conv_window_matrix` (``sae_conv_window_scatter``): ``dX`` [B, H, W, Cin]
    in ``dP``'s dtype, each element the fp32 sum, in a fixed order, of the entries of ``dP``
    [B * Ho * Wo, Kp] that read it.  No atomics: two calls give the same bits."""
    lib = L.load()
    _require_gpu(dP)
    B, H, W, C = (int(n) for n in x_shape)
    M = B * -(-H // stride) * -(-W // stride)
    if tuple(dP.shape) != (M, conv_window_cols(C, kernel_size)) or not dP.is_contiguous():
        raise ValueError(f"conv_window_scatter: dP must be contiguous [{M}, {conv_window_cols(C, kernel_size)}], "
                         f"got {tuple(dP.shape)}")
    d = _convtok_desc((B, H, W, C), kernel_size, stride, dP.dtype, dP.dtype)
    dX = torch.empty((B, H, W, C), dtype=dP.dtype, device=dP.device)
    tok = _TIMER.begin("conv_window_scatter") if _TIMER is not None else None
    L.check(lib.sae_conv_window_scatter(_stream(dP), ctypes.byref(d), _ptr(dP), _ptr(dX)))
    if tok is not None:
        _TIMER.end(tok, (B, H, W, C))
    return dX


def conv_tokens_ok(x, w, kernel_size: int, stride: int, dtype: torch.dtype) -> bool:
    """Host predicate of :func:`conv_tokens`: a contiguous, 16-byte-aligned GPU tensor [B, H, W, Cin]
    (bf16 or fp32), the Flax kernel [k, k, Cin, E] with k <= 7 and E % 8 == 0, stride >= 1, compute
    dtype bf16 or fp32, and extents whose element offsets fit 31 bits."""
    if not getattr(x, "is_cuda", False) or x.dim() != 4 or min(x.shape) < 1:
        return False
    if dtype not in (torch.bfloat16, torch.float32) or x.dtype not in (torch.bfloat16, torch.float32):
        return False
    k, s = int(kernel_size), int(stride)
    B, H, W, C = x.shape
    if not 1 <= k <= 7 or s < 1 or tuple(w.shape[:3]) != (k, k, C) or w.dim() != 4 or w.shape[3] % 8:
        return False
    if not x.is_contiguous() or x.data_ptr() % 16:
        return False
    M = B * -(-H // s) * -(-W // s)
    return x.numel() < 2 ** 31 and M * conv_window_cols(C, k) < 2 ** 31


class _ConvTokens(torch.autograd.Function):
    """models/cvt.py:28-33 as GEMMs on the window matrix P (``sae_conv_window_gather``): y = P W + b on
    ``sae_gemm_nt`` (bf16) or ``sae_gemm_f32``; dW = P^T dY and db on ``sae_gemm_dw`` / ``sae_gemm_f32``
    (into their gradient sinks inside a sink window); for an input that takes a gradient, and only
    then, dP = dY W^T on the same GEMMs and ``sae_conv_window_scatter``.  P is saved."""

    @staticmethod
    def forward(ctx, x, w, b, k, s, dt):
        K, E = k * k * x.shape[3], w.shape[3]
        B, H, W, _ = x.shape
        L_out = -(-H // s) * -(-W // s)
        tok = _TIMER.begin("conv_tokens_fwd") if _TIMER is not None else None
        P = conv_window_matrix(x, k, s, dt)
        Kp = P.shape[1]
        w2 = w.detach().reshape(K, E)
        if w2.dtype != torch.float32 or not w2.is_contiguous():
            w2 = w2.float().contiguous()
        if Kp != K:   # zero rows for the pad columns of P
            w2 = torch.nn.functional.pad(w2, (0, 0, 0, Kp - K))
        bias = b.detach().float().contiguous() if b is not None else None
        if dt == torch.bfloat16:
            wk, wt = weight_cast(w2)          # [Kp, E] for dP, [E, Kp] for the forward
            y = gemm_nt(P, wt, bias)
        else:
            wk = w2
            y = gemm_f32(P, wk, bias)
        if tok is not None:
            _TIMER.end(tok, (B * L_out, K, E))
        ctx.save_for_backward(P, wk)
        ctx.geom = (tuple(x.shape), k, s, K, E)
        ctx.wshape, ctx.wdtype, ctx.has_b, ctx.xdtype = tuple(w.shape), w.dtype, b is not None, x.dtype
        ctx.sinks = (_sink(w), _sink(b))
        return y.view(B, L_out, E)

    @staticmethod
    @_sinking
    def backward(ctx, dy):
        P, wk = ctx.saved_tensors
        xshape, k, s, K, E = ctx.geom
        Kp, dt, dev = P.shape[1], P.dtype, P.device
        dy2 = dy.to(dt).reshape(-1, E)
        if not dy2.is_contiguous() or dy2.data_ptr() % 16:
            dy2 = dy2.contiguous()
        sw, sb = ctx.sinks   # flat-buffer sinks (the training step): written in place
        tok = _TIMER.begin("conv_tokens_bwd") if _TIMER is not None else None
        db = _grad_out(sb, (E,), dev) if ctx.has_b else None
        # K == Kp: the kernel's gradient (or its sink) is the GEMM's output; else the first K rows of it
        direct = Kp == K
        dwp = _grad_out(sw.view(K, E) if sw is not None else None, (K, E), dev) if direct else \
            torch.empty((Kp, E), dtype=torch.float32, device=dev)
        if dt == torch.bfloat16:
            gemm_dw(P, dy2, dwp, db)
        else:
            gemm_f32(P.t(), dy2, out=dwp, colsum=db)
        if direct:
            dw = None if sw is not None else dwp.view(ctx.wshape).to(ctx.wdtype)
        elif sw is not None:
            _claim(sw).view(K, E).copy_(dwp[:K])
            dw = None
        else:
            dw = dwp[:K].reshape(ctx.wshape).to(ctx.wdtype)
        dx = None
        if ctx.needs_input_grad[0]:
            tok2 = _TIMER.begin("conv_tokens_dp") if _TIMER is not None else None
            dP = gemm_nt(dy2, wk) if dt == torch.bfloat16 else gemm_f32(dy2, wk.t())
            if tok2 is not None:
                _TIMER.end(tok2, (dy2.shape[0], E, Kp))
            dx = conv_window_scatter(dP, xshape, k, s).to(ctx.xdtype)
        if tok is not None:
            _TIMER.end(tok, (dy2.shape[0], K, E))
        return dx, dw, _unsunk(db, sb), None, None, None


def conv_tokens(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], kernel_size: int, stride: int,
                dtype: torch.dtype) -> torch.Tensor:
    """The convolution of ``ConvTokenEmbedBlock`` (models/cvt.py:28-33): ``x`` [B, H, W, Cin] (bf16 or
    fp32) with the Flax kernel ``w`` [k, k, Cin, E] (+ ``b``), stride ``stride``, SAME padding, in the
    compute dtype ``dtype`` -> tokens [B, Ho * Wo, E].  Gradients of w and b always, of x only when it
    requires one (the first stage's input is the image batch).  See :func:`conv_tokens_ok`."""
    _require_gpu(x, w)
    if x.dtype not in (torch.bfloat16, torch.float32) or (x.dtype == torch.bfloat16 and dtype == torch.float32):
        x = x.to(dtype)
    if not x.is_contiguous() or x.data_ptr() % 16:
        x = x.contiguous()
    if not conv_tokens_ok(x, w, kernel_size, stride, dtype):
        raise ValueError(f"conv_tokens: unsupported call (x {tuple(x.shape)}, kernel {tuple(w.shape)}, stride {stride}, "
                         f"{dtype}); see conv_tokens_ok")
    return _ConvTokens.apply(x, w, b, int(kernel_size), int(stride), dtype)
