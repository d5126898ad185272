"""The bucketed all-reduce of one training step's flat gradient buffer (train.py).

The flat buffer is cut into buckets along parameter boundaries in the order the backward finishes
them; a ``GradReducer`` tracks, inside its :meth:`GradReducer.window`, which parameters' gradients
are final and launches a bucket's SUM all-reduce the moment its last one is.  The bookkeeping needs
neither a process group nor a GPU: only :meth:`GradReducer.launch` (and ``between`` /
``issue_flagged``) touch ``torch.distributed``.
"""
from __future__ import annotations

import contextlib

import torch
import torch.distributed as dist

from . import ops

__all__ = ["cut_buckets", "parse_emulate_rccl", "GradReducer"]


def cut_buckets(offs, total, cap_elems):
    """Buckets of a flat buffer of ``total`` elements whose parameters start at ``offs``: they tile
    [0, total) from the end along parameter boundaries, in reverse registration order (the order
    the backward finishes the parameters); a bucket closes once it holds >= ``cap_elems`` elements
    and what remains at the front is the last bucket.  Returns (ranges, members): per bucket its
    (lo, hi) and the indices of its parameters, last parameter first."""
    ranges, members = [], []
    hi, ms = total, []
    for i in reversed(range(len(offs))):
        ms.append(i)
        lo = offs[i]
        if hi - lo >= cap_elems:
            ranges.append((lo, hi))
            members.append(ms)
            hi, ms = lo, []
    if ms:
        ranges.append((0, hi))
        members.append(ms)
    return ranges, members


def parse_emulate_rccl(text):
    """``SAE_EMULATE_RCCL="channels,busbw_GBps,world[,lds_KiB[,threads]]"`` (bench.py
    --emulate-rccl) as (channels, busbw, world, lds_bytes, threads), LDS defaulting to 64 KiB and
    threads to 256; None for the empty string.  The one-GPU contention emulation of an N-GPU node:
    beside each bucket's (one-rank) all-reduce, ``channels`` workgroups of ``threads`` threads
    holding ``lds_KiB`` of LDS occupy CUs on the communication stream for the ring time the bucket
    would take at ``world`` GPUs, 2 (world - 1) / world x bytes / busbw -- the CU footprint of
    RCCL's ring channels on the compute units the backward is using."""
    if not text:
        return None
    f = [float(x) for x in text.split(",")]
    if not 3 <= len(f) <= 5:
        raise ValueError(f"SAE_EMULATE_RCCL ({text!r}): channels,busbw_GBps,world[,lds_KiB[,threads]]")
    lds_kib = f[3] if len(f) > 3 else 64.0
    threads = f[4] if len(f) > 4 else 256.0
    return int(f[0]), f[1], int(f[2]), int(lds_kib * 1024), int(threads)


class GradReducer:
    """The buckets of ``flat`` (parameters at ``offs``, cut at ``cap_elems``) and their all-reduce
    in collective ``mode``:

    "overlap": inside :meth:`window` (one forward + backward) a parameter's gradient is final when
    the kernel writing its sink has been enqueued (:meth:`on_sink`, the ``GradSinks`` listener) or,
    for gradients autograd accumulates, after its accumulation (:meth:`on_ready`, the
    post-accumulate-grad hook); the bucket holding it is launched once all of its parameters are
    final, and the window's end launches the rest and joins.  On the GPU (``comm_stream``) the
    all-reduce runs on a communication stream beside the rest of the backward; on the CPU as an
    async work the window's end waits for.

    ``flagged`` (graph steps with the overlapped collective on the GPU): the captured forward +
    backward stays ONE linear kernel chain -- at each bucket's ready point it bumps a device flag
    (sae_flag_bump) instead of forking the all-reduce onto the communication stream inside the
    graph -- and after each replay the host enqueues, on the communication stream, every bucket's
    wait for its flag (hipStreamWaitValue32) followed by its RCCL all-reduce
    (:meth:`issue_flagged`), so the rings still run beside the rest of the backward.  A branch
    inside a replayed HIP graph costs the whole replay 0.13-0.4 ms on this runtime (the multi-queue
    launch path, measured with one-rank RCCL + a stand-in kernel per bucket:
    profiles/r06e_graph_fork.txt, r06d_rccl_emulation.txt); a linear graph keeps the single-queue
    fast path.  Outside a capture a flagged reducer launches like an unflagged one.

    "between" / "host": no tracking; :meth:`between` all-reduces the whole buffer between the
    forward + backward and the optimizer.

    ``group``: the process group of the gradient all-reduces (None: the default group).  On the GPU
    it is a group of its own, created with an eager communicator (device_id) and given no eager
    work before the capture (:meth:`paused` covers the warm-up steps): RCCL's watchdog thread then
    never holds an event recorded on that group's internal stream, which joins the step's capture
    (an event query on a capturing stream is hipErrorCapturedEvent, fatal in the watchdog).
    ``emulate``: a ``parse_emulate_rccl`` tuple or None."""

    def __init__(self, flat, offs, cap_elems, mode="overlap", group=None, comm_stream=False, flagged=False,
                 emulate=None):
        self.flat, self.mode, self.group, self.flagged, self.emulate = flat, mode, group, flagged, emulate
        self.buckets, self.members = cut_buckets(offs, flat.numel(), cap_elems)
        self.bucket_of = {i: b for b, ms in enumerate(self.members) for i in ms}
        # a sink is its parameter's view of the flat buffer: the listener is told its address
        self.ptr_to_idx = {flat.data_ptr() + 4 * off: i for i, off in enumerate(offs)}
        self.comm = torch.cuda.Stream(device=flat.device) if comm_stream else None
        self.enabled = True    # False: the capture's warm-up steps, no collective (paused)
        self.armed = False     # True inside a window
        self.ready, self.remaining, self.launched, self.works = set(), [], [], []
        if flagged:
            # one int32 counter per bucket, bumped once per replay of the forward + backward graph
            self.flags = torch.zeros(len(self.buckets), dtype=torch.int32, device=flat.device)
            self.flag_order = []   # bucket order of the captured bumps (the host's issue order)
            self.epoch = 0

    # ---- ready tracking
    @contextlib.contextmanager
    def window(self):
        """One forward + backward: armed inside; a normal exit launches every bucket not launched
        yet (buckets holding a parameter that got no gradient) and joins the collectives; any exit
        disarms."""
        self.ready = set()
        self.remaining = [len(ms) for ms in self.members]
        self.launched = [False] * len(self.buckets)
        self.works = []
        self.armed = True
        try:
            yield self
            self.armed = False
            for b in range(len(self.buckets)):
                if not self.launched[b]:
                    self._release(b)
            self._join()
        finally:
            self.armed = False

    def on_sink(self, ptr):
        i = self.ptr_to_idx.get(ptr)
        if i is not None:
            self.on_ready(i)

    def on_ready(self, i):
        if not self.armed or i in self.ready:
            return
        self.ready.add(i)
        b = self.bucket_of[i]
        self.remaining[b] -= 1
        if self.remaining[b] == 0:
            self._release(b)

    def _release(self, b):
        self.launched[b] = True
        if self.enabled:
            self.launch(b)

    @contextlib.contextmanager
    def paused(self):
        """No collective inside: buckets are only marked launched and :meth:`between` does nothing."""
        self.enabled = False
        try:
            yield
        finally:
            self.enabled = True

    # ---- the collectives
    def _marking(self):
        """Capturing the flagged graph: a bucket is a mark on the captured chain, its collective
        is issued after each replay."""
        return self.flagged and torch.cuda.is_current_stream_capturing()

    def launch(self, b):
        """Bucket ``b`` is final: its all-reduce (or, capturing the flagged graph, its flag bump)."""
        lo, hi = self.buckets[b]
        t = self.flat[lo:hi]
        if self._marking():
            ops.flag_bump(self.flags, b)
            self.flag_order.append(b)
        elif self.comm is not None:
            # the comm stream picks up everything enqueued so far on the compute stream (this
            # bucket's gradient kernels included) and runs the RCCL all-reduce beside the rest of
            # the backward; inside a graph capture this is a fork of the captured graph
            self.comm.wait_stream(torch.cuda.current_stream(t.device))
            self._allreduce_on_comm(t)
        else:
            self.works.append(dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group, async_op=True))

    def _allreduce_on_comm(self, t):
        """The SUM all-reduce of bucket ``t`` on the communication stream, which the caller has made
        wait for the bucket's gradients; under the RCCL emulation, the occupancy kernel behind it."""
        with torch.cuda.stream(self.comm):
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
            if self.emulate is not None:
                ch, bw, wd, lds, thr = self.emulate
                usec = 2.0 * (wd - 1) / wd * t.numel() * 4 / (bw * 1e3)
                ops.occupy_cus(self.comm, ch, usec, threads=thr, lds_bytes=lds)

    def _join(self):
        if self.comm is None:
            for w in self.works:
                w.wait()
        elif not self._marking():
            torch.cuda.current_stream(self.flat.device).wait_stream(self.comm)
        self.works = []

    def between(self, replayed=False):
        """The collectives between the forward + backward and the optimizer: the whole buffer's
        all-reduce ("between" / "host"), the flagged collectives after a replay of the flagged
        graph (``replayed``); nothing otherwise ("overlap" ran them inside the backward)."""
        if replayed and self.flagged:
            self.issue_flagged()
        elif not self.enabled:
            pass
        elif self.mode == "host":
            # rehearsal of the multi-rank step on fewer GPUs (SAE_DIST_BACKEND=gloo): one explicit
            # host round trip (gloo's own CUDA path stalled for seconds behind the graph replays)
            host = self.flat.cpu()
            dist.all_reduce(host, op=dist.ReduceOp.SUM)
            self.flat.copy_(host)
        elif self.mode == "between":
            # every bucket in flight at once on the process group's stream; the optimizer's graph
            # replay waits for them on the compute stream (no host synchronisation)
            works = [dist.all_reduce(self.flat[lo:hi], op=dist.ReduceOp.SUM, group=self.group, async_op=True)
                     for lo, hi in self.buckets]
            for w in works:
                w.wait()

    def issue_flagged(self):
        """After a replay of the flagged forward + backward graph: on the communication stream, each
        bucket's wait for its flag (bumped by this replay) and its all-reduce, in the captured order;
        the compute stream joins the communication stream before the optimizer's graph."""
        self.epoch += 1
        for b in self.flag_order:
            lo, hi = self.buckets[b]
            ops.stream_wait_flag(self.comm, self.flags, b, self.epoch)
            self._allreduce_on_comm(self.flat[lo:hi])
        torch.cuda.current_stream(self.flat.device).wait_stream(self.comm)

    def reset_flag_order(self):
        """Before the flagged graph is captured: its bumps are recorded afresh."""
        if self.flagged:
            self.flag_order = []

    def close(self):
        """Destroy the gradient group (after the graphs that hold its collectives)."""
        if self.group is not None and dist.is_initialized():
            dist.destroy_process_group(self.group)
        self.group = None
