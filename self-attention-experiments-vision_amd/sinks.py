"""Gradient sinks of one training step (the flat data-parallel gradient buffer, train.py).

Left to autograd, each parameter gradient would be computed into a fresh tensor and then ADDED into
its zeroed view of the flat buffer (one extra elementwise kernel per parameter, ~150 per DeiT-S
step).  A sink is that flat view: the backward kernels of ``ops`` (weight / bias GEMMs, LayerNorm
dgamma / dbeta, patch embedding) write the gradient straight into it and hand autograd None for
that parameter.  A parameter may feed at most one such op per backward (each Dense / LayerNorm of
the models is applied once per step); a second write raises instead of silently overwriting.
"""
from __future__ import annotations

import contextlib
import weakref
from typing import Optional

import torch

from . import ops

__all__ = ["GradSinks"]


class GradSinks:
    """``views[i]`` (fp32, contiguous, shaped like ``params[i]``) is the gradient sink of
    ``params[i]``; the ops see it only inside this object's :meth:`backward` window (outside every
    window a backward keeps autograd's accumulate semantics).  ``listener(data_ptr)`` is called for
    every sink once the kernel that writes it has been enqueued (the training step launches a
    bucket's all-reduce from it).  ``wgrad_stream``: a weight gradient that goes into a sink is off
    the backward's critical path, so its GEMM (``ops.gemm_dw(offload=True)``) runs on this stream
    beside the input-gradient chain; the owner joins it (:meth:`join`) before it reads the gradients."""

    def __init__(self, params, views, listener=None, wgrad_stream=None):
        self._by_id = {}      # id(param) -> (weakref(param), view)
        for p, v in zip(params, views):
            if v.dtype != torch.float32 or not v.is_contiguous() or v.shape != p.shape:
                raise ValueError("GradSinks: a sink must be an fp32 contiguous view shaped like its parameter")
            self._by_id[id(p)] = (weakref.ref(p), v)
        self.listener = listener
        self.wgrad_stream = wgrad_stream
        self.written = set()  # data pointers of the sinks written in the last window
        self.claimed = []     # ... of those claimed by the backward function now running

    @contextlib.contextmanager
    def backward(self):
        """The sink window of one forward + backward: every sink may be written once.  One window
        at a time; ``written`` stays readable after it closes, until the next one opens."""
        if ops._ACTIVE_SINKS is not None:
            raise RuntimeError("GradSinks.backward: a sink window is already open")
        self.written.clear()
        del self.claimed[:]
        ops._ACTIVE_SINKS = self
        try:
            yield self
        finally:
            ops._ACTIVE_SINKS = None

    def lookup(self, t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        """The sink of parameter ``t`` (or of the parameter ``t`` is a full reshape view of), viewed
        as ``t``'s shape; None when it has none."""
        if t is None or not t.requires_grad:
            return None
        base = t if t._base is None else t._base
        e = self._by_id.get(id(base))
        if e is None or e[0]() is not base or t.numel() != base.numel():
            return None
        g = base.grad   # a sink is live only while it is still the parameter's .grad (not replaced / reset)
        if g is None or g.data_ptr() != e[1].data_ptr():
            return None
        return e[1].view(t.shape)

    def claim(self, sink: torch.Tensor) -> torch.Tensor:
        """Mark ``sink`` as written by the backward function now running (at most once per window)."""
        key = sink.data_ptr()
        if key in self.written:
            raise RuntimeError("gradient sink written twice in one backward: a parameter feeds two ops")
        self.written.add(key)
        self.claimed.append(key)
        return sink

    def report(self, n0: int) -> None:
        """Tell the listener about the sinks claimed since ``claimed`` had ``n0`` entries: their
        kernels are enqueued (``ops._sinking`` calls this when a backward function returns)."""
        done = self.claimed[n0:]
        del self.claimed[n0:]
        if self.listener is None:
            return
        side = self.wgrad_stream
        if side is not None:
            # a sink may have been written on the weight-gradient stream: the listener's
            # collective waits on that stream, which first picks up the main stream's work
            side.wait_stream(torch.cuda.current_stream(side.device))
        with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
            for ptr in done:
                self.listener(ptr)

    def join(self) -> None:
        """Make the current stream wait for every weight-gradient GEMM enqueued on the side stream."""
        if self.wgrad_stream is not None:
            torch.cuda.current_stream(self.wgrad_stream.device).wait_stream(self.wgrad_stream)
