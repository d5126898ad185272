"""Data-parallel training step (train.py:77-109 of the reference, rebuilt for MI355X).

One process per GPU, ``torch.distributed`` with backend ``nccl`` (= RCCL on ROCm) over
xGMI.  The reference's ``jax.pmap(train_step)`` + ``lax.pmean(grads)`` (train.py:94-96,230)
becomes: every parameter's gradient is a 16-byte-aligned view into ONE flat fp32 buffer, cut
into buckets along parameter boundaries in the order the backward finishes them; the backward
kernels write the gradients straight into their views (gradient sinks, sinks.GradSinks), and
as soon as the last gradient of a bucket is written its SUM all-reduce (of the gradients of
loss / world = the global-batch mean) is launched on a communication stream, overlapping the
rest of the backward; the compute stream joins that stream before the one-launch AdamW.  On the
GPU the whole step -- forward, loss, backward with the overlapped bucket all-reduces, AdamW -- is
ONE HIP graph (RCCL collectives are graph-capturable: tools/probe/rccl_graph.py), so a step costs
one host call.  Survey D9 decisions: standard descent (the reference's optax chain ascends), the
gradient is the global batch mean (the reference divides the loss by device_count *and*
pmean's), no wandb call inside the step.

Collective modes (``TrainStep.collective``): "overlap" (default whenever there is a process group:
bucket all-reduces launched from inside the backward), "between" (``two_graphs=True``: forward +
backward graph, the bucket all-reduces, optimizer graph), "host" (gloo with CUDA tensors, the
multi-rank rehearsal on one GPU: an explicit host round trip between two graphs), "none" (no
process group).  ``SAE_WORLD1_RCCL=1`` (bench.py ``--world1-rccl``) creates a world-size-1 RCCL
group so the overlapped collective path runs on a one-GPU box.

Structure: ``step_facts`` gathers what a step's structure depends on (the process group, where
the parameters live, the constructor's arguments, ``SAE_FLAGGED`` / ``SAE_WG_STREAM``) and
``step_plan``, a pure function, decides it once: flat or per-parameter gradients, the optimizer,
the collective mode, one graph or two, flag-gated or not, which process groups, streams, hooks
and sinks exist.  ``TrainStep.__init__`` builds what the plan names.  The buckets and their
all-reduce are a ``reducer.GradReducer`` (``TrainStep.reducer``, None without a process group).

Loss: one-hot -> optax.smooth_labels(0.1) -> softmax cross-entropy, mean (train.py:83-92); with
``mix=True`` the one-hot is the default augmentation's mixup / cutmix target ``ratio onehot(labels) +
(1 - ratio) onehot(mix_labels)`` and ``metrics=True`` adds utils.topk_correct of the step's logits
(``step.top1`` / ``step.top5``), both from one HIP loss (ops.mixed_cross_entropy).  ``EvalStep`` is the
reference's eval_step (train.py:112-120) with a device accumulator.
Optimizer: the reference's chain (train.py:22-27,214-220): clip_by_global_norm(``clip_grad``),
Adam, decoupled weight decay 1e-4, scale by the schedule.  ``lr_schedule=None`` keeps the constant
rate 5e-4 * batch/512 and ``clip_grad=None`` no clip (the defaults, which launch exactly what a step
without the feature launched); a ``WarmupCosine`` (``reference_schedule`` builds the reference's) and
a clip norm put the learning rate and the clip factor into device memory, computed per step by
``sae_adamw_prepare`` (csrc/adamw.h), so the captured graph replays with each step's own values.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import os
import weakref
from dataclasses import dataclass
from typing import NamedTuple, Optional

import torch
import torch.distributed as dist
import torch.nn.functional as F

from . import _lib as L
from . import ops
from .reducer import GradReducer, parse_emulate_rccl
from .sinks import GradSinks

__all__ = ["smoothed_cross_entropy", "mixed_cross_entropy", "topk_correct", "label_ranks", "TrainStep", "EvalStep",
           "init_distributed", "FusedAdamW", "WarmupCosine", "reference_schedule", "StepFacts", "StepPlan",
           "step_facts", "step_facts_of_values", "step_plan"]


@dataclass(frozen=True)
class WarmupCosine:
    """optax.warmup_cosine_decay_schedule (reference train.py:215-220): linear from ``init_value``
    to ``peak_value`` over ``warmup_steps`` updates, then a cosine from ``peak_value`` to
    ``end_value`` that ends at update ``decay_steps`` (counted from 0, warm-up included) and stays
    there.  ``value(count)``: the rate of the update after ``count`` updates, as optax counts."""
    init_value: float
    peak_value: float
    warmup_steps: int
    decay_steps: int
    end_value: float = 0.0

    def __post_init__(self):
        if not (self.peak_value > 0 and math.isfinite(self.peak_value)):
            raise ValueError(f"WarmupCosine: peak_value ({self.peak_value}) must be > 0 and finite")
        if self.warmup_steps < 0 or self.decay_steps <= self.warmup_steps:
            raise ValueError(f"WarmupCosine: need 0 <= warmup_steps ({self.warmup_steps}) < decay_steps "
                             f"({self.decay_steps})")
        if not (0 <= self.init_value < math.inf and 0 <= self.end_value < math.inf):
            raise ValueError("WarmupCosine: init_value and end_value must be >= 0 and finite")

    def value(self, count: int) -> float:
        if count < self.warmup_steps:
            return self.init_value + (self.peak_value - self.init_value) * count / self.warmup_steps
        D = self.decay_steps - self.warmup_steps
        c = min(count - self.warmup_steps, D)
        alpha = self.end_value / self.peak_value
        return self.peak_value * ((1 - alpha) * 0.5 * (1 + math.cos(math.pi * c / D)) + alpha)


def reference_schedule(lr: float, global_batch: int, steps_per_epoch: int) -> WarmupCosine:
    """The reference's schedule (train.py:214-220): from 0 to lr * batch/512 over 5 epochs, cosine
    to 1e-5 at epoch 30."""
    return WarmupCosine(0.0, lr * (global_batch / 512), 5 * steps_per_epoch, 30 * steps_per_epoch, 1e-5)


def _check_clip(clip_grad):
    if clip_grad is not None and not float(clip_grad) > 0:   # (NaN included)
        raise ValueError(f"clip_grad ({clip_grad}) must be > 0 (None: no clip)")
    return None if clip_grad is None else float(clip_grad)


def _label_ranks_cpu(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """``label_ranks`` of CPU tensors: the rule the loss kernel counts by, in torch ops."""
    x = logits.detach().float().reshape(-1, logits.shape[-1])
    K = x.shape[1]
    y = labels.reshape(-1).to(torch.int64)
    ok = (y >= 0) & (y < K)
    yc = y.clamp(0, K - 1)[:, None]
    xy = x.gather(1, yc)
    nx, ny = x.isnan(), xy.isnan()
    cls = torch.arange(K)[None, :]
    above = ((x > xy) | (nx & ~ny) | (((x == xy) | (nx & ny)) & (cls > yc))).sum(1)
    return torch.where(ok, above, torch.full_like(above, K)).to(torch.int32)


def _cross_entropy_rows(logits, labels, mix_labels=None, ratio=None, smoothing=0.1, metrics=False):
    """The one loss of this module, ``(loss, top, row_loss, rank)`` as ops.mixed_cross_entropy_rows
    returns them: train.py:83-90 (the targets ``ratio onehot(labels) + (1 - ratio) onehot(mix_labels)``,
    or one label per row when ``mix_labels`` / ``ratio`` are None; optax.smooth_labels; mean softmax
    cross entropy) and, with ``metrics``, the per-row losses, the first label's ranks (``label_ranks``)
    and ``top`` = the mean top-1 / top-5 of train.py:98-99.  GPU logits take the HIP loss; CPU tensors
    (the multi-process gloo tests' small models) take torch's cross entropy, which computes the same
    quantity: index targets without a partner, probability targets with one.  The HIP loss gives a
    label outside [0, K) no target term; the CPU branch with a partner refuses one (ValueError).
    Without ``metrics`` the CPU branch returns None for the other three."""
    if logits.is_cuda:
        return ops.mixed_cross_entropy_rows(logits, labels, mix_labels, ratio, smoothing, metrics)
    if (mix_labels is None) != (ratio is None):
        raise ValueError("mixed_cross_entropy: mix_labels and ratio go together (both or neither)")
    x = logits.float()
    target = labels.to(torch.int64)
    if mix_labels is not None:
        K = x.shape[-1]
        for name, y in (("labels", labels), ("mix_labels", mix_labels)):
            if bool(((y < 0) | (y >= K)).any()):
                raise ValueError(f"mixed_cross_entropy (CPU): {name} outside [0, {K})")
        rho = ratio.to(x.dtype)[:, None]
        partner = F.one_hot(mix_labels.to(torch.int64), K).to(x.dtype)
        target = rho * F.one_hot(target, K).to(x.dtype) + (1.0 - rho) * partner
    loss = F.cross_entropy(x, target, label_smoothing=smoothing)
    if not metrics:
        return loss, None, None, None
    row_loss = F.cross_entropy(x, target, label_smoothing=smoothing, reduction="none")
    rank = _label_ranks_cpu(logits, labels)
    return loss, torch.stack([(rank < 1).float().mean(), (rank < 5).float().mean()]), row_loss, rank


def smoothed_cross_entropy(logits: torch.Tensor, labels: torch.Tensor, smoothing: float = 0.1) -> torch.Tensor:
    """train.py:77-90 (optax.smooth_labels + mean softmax cross entropy): ``mixed_cross_entropy`` with
    one label per row and no metrics."""
    return _cross_entropy_rows(logits, labels, None, None, smoothing, False)[0]


def label_ranks(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """Per row, the number of classes a stable ascending argsort of the row (jnp.argsort of
    utils.topk_correct) places above the row's label: class c is above label y iff x[c] > x[y], or
    x[c] is NaN and x[y] is not, or they compare equal (-0 == +0; both NaN) and c > y.  A label
    outside [0, K) ranks K.  GPU logits: the rank the loss kernel counts (sae_mixed_ce_fwd); CPU
    tensors: the same rule in torch ops (alone: torch's cross entropy refuses a label outside the
    classes).  int32 [R]."""
    logits = logits.reshape(-1, logits.shape[-1])
    if logits.is_cuda:
        return _cross_entropy_rows(logits.detach(), labels, None, None, 0.0, True)[3]
    return _label_ranks_cpu(logits, labels)


def topk_correct(logits: torch.Tensor, labels: torch.Tensor, topk=(1, 5)):
    """utils.topk_correct (train.py:98-99): per k of ``topk`` a float32 [R] tensor, 1 where the row's
    label is among the last k classes of the row's stable ascending argsort (ties go to the higher
    class index, NaN sorts last), else 0."""
    rank = label_ranks(logits, labels)
    return tuple((rank < int(k)).float() for k in topk)


def mixed_cross_entropy(logits: torch.Tensor, labels: torch.Tensor, mix_labels: Optional[torch.Tensor] = None,
                        ratio: Optional[torch.Tensor] = None, smoothing: float = 0.1, metrics: bool = False):
    """train.py:83-90 with the default augmentation's mixup / cutmix targets: ``ratio onehot(labels) +
    (1 - ratio) onehot(mix_labels)``, optax.smooth_labels, mean softmax cross entropy.  ``mix_labels``
    and ``ratio`` go together; both None is the one-label loss, ``smoothed_cross_entropy``.
    ``metrics=True`` returns ``(loss, top1, top5)`` with the mean of ``topk_correct`` on the first label
    (train.py:98-99).  Devices and refusals: ``_cross_entropy_rows``."""
    loss, top, _, _ = _cross_entropy_rows(logits, labels, mix_labels, ratio, smoothing, metrics)
    return (loss, top[0], top[1]) if metrics else loss


def init_distributed():
    """Initialise the process group from torchrun's env (RANK/WORLD_SIZE/LOCAL_RANK/MASTER_*).
    ``SAE_WORLD1_RCCL=1`` at world size 1 (GPU): a one-rank RCCL group, so the training step's
    collective path (the overlapped bucket all-reduces captured in the step's HIP graph) runs."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # SAE_DIST_BACKEND=gloo rehearses the multi-rank path on fewer GPUs than ranks (ranks share
    # devices round-robin; gloo all-reduces the CUDA gradients through host memory)
    backend = os.environ.get("SAE_DIST_BACKEND") or ("nccl" if torch.cuda.is_available() else "gloo")
    if torch.cuda.is_available():
        local = local % max(1, torch.cuda.device_count()) if backend == "gloo" else local
    world1 = world == 1 and os.environ.get("SAE_WORLD1_RCCL", "0") == "1" and torch.cuda.is_available()
    if backend == "nccl" or world1:
        # Peer connections at communicator creation, not at a communicator's first collective:
        # RCCL (2.26 bundled with torch, 2.27 in /opt/rocm; both read NCCL_RUNTIME_CONNECT) by
        # default connects the ring / tree peers lazily, inside the first collective that needs
        # them -- for the gradient group that first collective is issued INSIDE the step's graph
        # capture (TrainStep.reducer.group), where the connection setup's allocations and host
        # handshakes would run in a capturing context.  With 0 every communicator -- the default one created
        # by init_process_group(device_id=) and the gradient group's by new_group(device_id=) --
        # is fully connected when its creation returns, so the captured collectives only enqueue
        # kernels.  A value the user exported wins.
        os.environ.setdefault("NCCL_RUNTIME_CONNECT", "0")
    if (world > 1 or world1) and not dist.is_initialized():
        if torch.cuda.is_available():
            torch.cuda.set_device(local)
        if world1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            if "MASTER_PORT" not in os.environ:
                import socket
                with socket.socket() as sk:
                    sk.bind(("127.0.0.1", 0))
                    os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
            dist.init_process_group(backend="nccl", rank=0, world_size=1, device_id=torch.device("cuda", local))
        elif backend == "nccl":
            # device_id: the communicator is created now (eagerly), not by the first collective
            dist.init_process_group(backend=backend, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend=backend)
    elif torch.cuda.is_available():
        torch.cuda.set_device(local)
    return rank, world, local


def agree_all_ranks(ok: bool, group) -> bool:
    """True iff ``ok`` holds on every rank of ``group`` (a MIN all-reduce of one flag over a
    host-side gloo group).  TrainStep decides with it whether the captured graph is used: at
    world > 1 one rank's capture failure turns the graph off on every rank, so that all ranks
    issue the same collectives in the same order."""
    flag = torch.tensor([1 if ok else 0], dtype=torch.int32)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
    return bool(flag.item())


def flat_layout(params, align: int = 4):
    """Offsets of ``params`` in one flat fp32 buffer, each rounded up to ``align`` elements (16
    bytes): every gradient view starts 16-byte aligned, as the vector stores of the kernels that
    write them in place (gemm_dw, patch_embed_bwd, tokens_bwd) require.  Returns (offsets, total)."""
    offs, off = [], 0
    for p in params:
        offs.append(off)
        off += -(-p.numel() // align) * align
    return offs, off


class _Slot(NamedTuple):
    """One parameter of FusedAdamW: its index and the addresses of its gradient view and moments."""
    index: int
    param: torch.Tensor
    grad: int
    m: int
    v: int


class FusedAdamW:
    """AdamW (optax.adamw of train.py:25-27,229-233, torch.optim.AdamW's update order) for fp32 GPU
    parameters whose gradients live in one flat buffer: every parameter in one HIP launch
    (``sae_adamw_step``, csrc/adamw.h) instead of torch's multi-tensor launches.  The moments are
    two more flat buffers laid out like the gradients; the step counter stays on the device, so the
    update can be captured in a HIP graph and replayed.

    ``cast_groups``: column-stacked groups of 2-D fp32 Dense kernels (the ``ops.forward_casts``
    groups; each kernel a whole parameter, possibly reshaped) whose bf16 compute copies the
    update writes as it goes (``sae_adamw_step_cast``): the forward then reads persistent copies
    (``ops.register_persistent_casts``) instead of casting every weight at its start.  Parameter
    values are bit-identical either way.

    ``clip_grad`` (optax.clip_by_global_norm's max_norm), ``lr_schedule`` (a ``WarmupCosine``; None:
    the constant ``lr``) and ``monitor_norm`` (the norm without a clip): with any of them ``step()``
    is ``sae_adamw_prepare`` (global norm of the WHOLE flat buffer, clip factor, this step's rate,
    counter tick) followed by ``sae_adamw_step_dev`` on the current stream, so the norm always sits
    directly before the update wherever ``step()`` is captured.  ``lr_now`` and ``grad_norm`` are
    device views of the ``hyper`` buffer those kernels share (no sync; None without the feature).
    With all three at their defaults ``step()`` makes exactly the calls it made without them."""

    def __init__(self, params, flat_grad: torch.Tensor, lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, cast_groups=None, clip_grad: Optional[float] = None,
                 lr_schedule: Optional[WarmupCosine] = None, monitor_norm: bool = False):
        self.lib = L.load()
        self.params = list(params)
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), tuple(betas), float(eps), float(weight_decay)
        dev = flat_grad.device
        self.m = torch.zeros_like(flat_grad)
        self.v = torch.zeros_like(flat_grad)
        self.step_count = torch.zeros(1, dtype=torch.int32, device=dev)
        self.clip_grad, self.lr_schedule = _check_clip(clip_grad), lr_schedule
        if lr_schedule is not None and not isinstance(lr_schedule, WarmupCosine):
            raise TypeError("FusedAdamW: lr_schedule must be a WarmupCosine or None")
        self.hyper = None   # {lr_t, clip_scale, grad_norm, -} on the device, written by sae_adamw_prepare
        if self.clip_grad is not None or lr_schedule is not None or monitor_norm:
            if flat_grad.dtype != torch.float32 or not flat_grad.is_contiguous() or flat_grad.dim() != 1:
                raise ValueError("FusedAdamW: the flat gradient buffer must be 1-D contiguous fp32")
            self.hyper = torch.zeros(4, dtype=torch.float32, device=dev)
            s = lr_schedule
            self._sched = (L.LrSchedule(L.SAE_LR_CONSTANT, 0.0, self.lr, 0.0, 0, 0) if s is None else
                           L.LrSchedule(L.SAE_LR_WARMUP_COSINE, s.init_value, s.peak_value, s.end_value,
                                        int(s.warmup_steps), int(s.decay_steps)))
            # the norm runs over the whole flat buffer, alignment padding included: the padding is
            # zero when the buffer is built and nothing ever writes it (TrainStep, flat_layout)
            self._norm_of, self._norm_ws = None, None
            if self.clip_grad is not None or monitor_norm:
                self._norm_of = flat_grad
                nbytes = int(self.lib.sae_adamw_prepare_workspace_bytes(flat_grad.numel()))
                self._norm_ws = torch.zeros(nbytes // 8, dtype=torch.float64, device=dev)
        # copies an earlier optimizer over these parameters registered would go stale under this
        # one (it updates the weights through raw pointers): they stop being served
        ops.release_persistent_casts(self.params)
        slot = {}
        for i, p in enumerate(self.params):
            g = p.grad
            if (p.dtype != torch.float32 or not p.is_contiguous() or g is None or g.dtype != torch.float32
                    or not g.is_contiguous() or g.data_ptr() < flat_grad.data_ptr()):
                raise ValueError("FusedAdamW: fp32 contiguous parameters with views of the flat gradient buffer")
            off = (g.data_ptr() - flat_grad.data_ptr()) // 4
            slot[p.data_ptr()] = _Slot(i, p, g.data_ptr(), self.m.data_ptr() + 4 * off, self.v.data_ptr() + 4 * off)
        # the Dense kernels whose copies the update writes: whole parameters, shapes / alignment
        # the tile path takes (K, N, column offsets multiples of 4)
        self.cast_groups, self.copies = [], []
        tiles_in = []   # per kernel: (slot, K, n, w16, wt16, N of its group, its first column)
        claimed = set()
        for ws in (cast_groups or []):
            K = ws[0].shape[0]
            ent = [slot.get(w.data_ptr()) for w in ws]
            if (any(e is None or e.param.numel() != w.numel() for e, w in zip(ent, ws))
                    or any(e.index in claimed for e in ent)          # a parameter is updated once
                    or len({e.index for e in ent}) != len(ent)
                    or any(w.dim() != 2 or w.shape[0] != K for w in ws)
                    or K % 4 or any(w.shape[1] % 4 for w in ws)
                    or any(e.grad % 16 or e.m % 16 or e.v % 16 or e.param.data_ptr() % 16 for e in ent)):
                continue
            claimed.update(e.index for e in ent)
            N = sum(w.shape[1] for w in ws)
            w16 = torch.empty((K, N), dtype=torch.bfloat16, device=dev)
            wt16 = torch.empty((N, K), dtype=torch.bfloat16, device=dev)
            col = 0
            for e, w in zip(ent, ws):
                tiles_in.append((e, K, w.shape[1], w16, wt16, N, col))
                col += w.shape[1]
            self.cast_groups.append(list(ws))
            self.copies.append((w16, wt16))
        self._plan_chunks([p for i, p in enumerate(self.params) if i not in claimed], slot, dev)
        self.n_tiles, self.tiles = 0, None
        if tiles_in:
            self._plan_cast_tiles(tiles_in, dev)
            # the owner token: unregistering (close, finalizer) removes only this optimizer's
            # entries; registering casts the initial weights into the copies
            self._owner = object()
            ops.register_persistent_casts(self.cast_groups, [c[0] for c in self.copies], [c[1] for c in self.copies],
                                          self._owner)
            # the registry holds the weights (their addresses cannot be reused while registered);
            # it lets go of them with the optimizer
            weakref.finalize(self, ops.unregister_persistent_casts, self._owner)

    def _plan_chunks(self, params, slot, dev):
        """The device chunk table of ``params``, which the flat path updates (``sae_adamw_plan``), built once."""
        n = len(params)
        arr = lambda t: (t * max(1, n))()
        P, G, M, V = (arr(ctypes.c_void_p) for _ in range(4))
        Nn = arr(ctypes.c_int64)
        for j, p in enumerate(params):
            s = slot[p.data_ptr()]
            P[j], G[j], M[j], V[j], Nn[j] = p.data_ptr(), s.grad, s.m, s.v, p.numel()
        cap = sum(-(-p.numel() // L.SAE_ADAMW_CHUNK) for p in params)
        table = (L.AdamwChunk * max(1, cap))()
        cnt = ctypes.c_int64(0)
        L.check(self.lib.sae_adamw_plan(n, P, G, M, V, Nn, table, cap, ctypes.byref(cnt)))
        self.n_chunks = int(cnt.value)
        self.table = torch.frombuffer(bytearray(table), dtype=torch.uint8).to(dev)

    def _plan_cast_tiles(self, tiles_in, dev):
        """The device 64 x 64 tile table of the kernels whose bf16 copies the update writes, built once."""
        k = len(tiles_in)
        arr = lambda t: (t * k)()
        P, G, M, V, W16, WT = (arr(ctypes.c_void_p) for _ in range(6))
        Kx, Nx, LD, LT, C0 = (arr(ctypes.c_int32) for _ in range(5))
        for j, (e, K, Nw, w16, wt16, Ntot, col) in enumerate(tiles_in):
            P[j], G[j], M[j], V[j] = e.param.data_ptr(), e.grad, e.m, e.v
            W16[j], WT[j] = w16.data_ptr(), wt16.data_ptr()
            Kx[j], Nx[j], LD[j], LT[j], C0[j] = K, Nw, Ntot, K, col
        cap = sum(-(-K // 64) * -(-Nw // 64) for _, K, Nw, *_ in tiles_in)
        ttab = (L.AdamwCastTile * cap)()
        cnt = ctypes.c_int64(0)
        L.check(self.lib.sae_adamw_cast_plan(k, P, G, M, V, Kx, Nx, W16, LD, WT, LT, C0, ttab, cap, ctypes.byref(cnt)))
        self.n_tiles = int(cnt.value)
        self.tiles = torch.frombuffer(bytearray(ttab), dtype=torch.uint8).to(dev)

    @property
    def lr_now(self):
        """The rate the last update used (0-d device view; None without clip / schedule / monitor)."""
        return None if self.hyper is None else self.hyper[0]

    @property
    def grad_norm(self):
        """The global gradient norm the last update saw, before clipping (0-d device view; 0 unless
        ``clip_grad`` or ``monitor_norm`` asked for the norm pass)."""
        return None if self.hyper is None else self.hyper[2]

    def step(self):
        b1, b2 = self.betas
        st = torch.cuda.current_stream(self.m.device).cuda_stream
        if self.hyper is not None:
            g = self._norm_of
            L.check(self.lib.sae_adamw_prepare(
                st, 0 if g is None else g.numel(), None if g is None else g.data_ptr(),
                math.inf if self.clip_grad is None else self.clip_grad, ctypes.byref(self._sched),
                self.step_count.data_ptr(), None if g is None else self._norm_ws.data_ptr(), self.hyper.data_ptr()))
            L.check(self.lib.sae_adamw_step_dev(st, self.n_chunks, self.table.data_ptr(), self.n_tiles,
                                                self.tiles.data_ptr() if self.n_tiles else None,
                                                self.step_count.data_ptr(), self.hyper.data_ptr(), b1, b2, self.eps,
                                                self.weight_decay))
        elif self.n_tiles:
            L.check(self.lib.sae_adamw_step_cast(st, self.n_chunks, self.table.data_ptr(), self.n_tiles,
                                                 self.tiles.data_ptr(), self.step_count.data_ptr(), self.lr, b1, b2,
                                                 self.eps, self.weight_decay))
        else:
            L.check(self.lib.sae_adamw_step(st, self.n_chunks, self.table.data_ptr(), self.step_count.data_ptr(),
                                            self.lr, b1, b2, self.eps, self.weight_decay))

    def refresh_casts(self, only_if_stale: bool = False):
        """Re-cast the copies after the parameters were overwritten outside the update; with
        ``only_if_stale`` only if a weight's version moved since (a replayed step graph holds no cast:
        a load_state_dict after the capture would otherwise reach the forward one update late)."""
        if self.cast_groups:
            ops.refresh_persistent_casts(self.cast_groups, only_if_stale)

    def close(self):
        """Stop serving the copies (the forward casts per call again)."""
        if self.cast_groups:
            ops.unregister_persistent_casts(self._owner)
            self.cast_groups = []

    def state_tensors(self):
        return [self.m, self.v, self.step_count] + ([] if self.hyper is None else [self.hyper])


class StepFacts(NamedTuple):
    """What the structure of a training step depends on (``step_plan``), and nothing else."""
    pg: bool                     # there is a default process group
    backend: Optional[str]       # ... its backend ("nccl" / "gloo")
    world: int
    on_gpu: bool                 # every parameter is on the GPU
    fp32_contiguous: bool        # every parameter is fp32 and contiguous
    cuda: bool                   # torch.cuda.is_available()
    graph: bool                  # the arguments of TrainStep, as given ...
    flat_grads: Optional[bool]
    grad_sinks: bool
    two_graphs: Optional[bool]
    wgrad_stream: bool           # ... (None resolved from SAE_WG_STREAM)
    clip_or_schedule: bool       # clip_grad or lr_schedule is set
    flagged_on: bool             # SAE_FLAGGED != "0"


def step_facts(params, graph, flat_grads, grad_sinks, two_graphs, wgrad_stream, clip_or_schedule) -> StepFacts:
    """The facts of a step over ``params`` from TrainStep's arguments and the live process state (the
    default process group, the devices, SAE_FLAGGED, SAE_WG_STREAM: read here and nowhere else)."""
    pg = dist.is_initialized()
    if wgrad_stream is None:
        wgrad_stream = os.environ.get("SAE_WG_STREAM", "0") == "1"
    return StepFacts(pg=pg, backend=dist.get_backend() if pg else None, world=dist.get_world_size() if pg else 1,
                     on_gpu=all(p.is_cuda for p in params),
                     fp32_contiguous=all(p.dtype == torch.float32 and p.is_contiguous() for p in params),
                     cuda=torch.cuda.is_available(), graph=bool(graph), flat_grads=flat_grads,
                     grad_sinks=bool(grad_sinks), two_graphs=two_graphs, wgrad_stream=bool(wgrad_stream),
                     clip_or_schedule=bool(clip_or_schedule),
                     flagged_on=os.environ.get("SAE_FLAGGED", "1") != "0")


def step_facts_of_values(pg=False, backend=None, world=1, on_gpu=True, fp32_contiguous=True, cuda=True, graph=True,
                         flat_grads=None, grad_sinks=True, two_graphs=None, wgrad_stream=False,
                         clip_or_schedule=False, flagged_on=True) -> StepFacts:
    """The facts from plain values; the defaults are bench.py's step on one GPU (fp32 GPU parameters,
    graph=True, no process group, no environment switch set)."""
    return StepFacts(pg, backend, world, on_gpu, fp32_contiguous, cuda, graph, flat_grads, grad_sinks, two_graphs,
                     wgrad_stream, clip_or_schedule, flagged_on)


class StepPlan(NamedTuple):
    """The structure of a training step: what TrainStep.__init__ builds and its step runs."""
    graph: bool            # the step is captured as HIP graph(s)
    flat: bool             # one flat gradient buffer (else per-parameter gradients)
    fused: bool            # the one-launch FusedAdamW (else torch.optim.AdamW)
    collective: str        # "none" | "host" | "between" | "overlap"
    flagged: bool          # the overlapped all-reduces are flag-gated outside a linear graph (GradReducer)
    two_graphs: bool       # forward + backward graph, optimizer graph (else one graph)
    grad_group: bool       # create the RCCL gradient group
    agree_group: bool      # create the gloo group of the all-ranks capture decision
    hooks: bool            # arm the post-accumulate-grad hooks
    comm_stream: bool      # the communication stream
    sinks: bool            # gradient sinks
    sink_listener: bool    # ... that tell the reducer
    wgrad_stream: bool     # the weight-gradient side stream
    capturable: bool       # torch.optim.AdamW(capturable=True) (read for the torch optimizer only)
    capture_mode: str      # "thread_local" | "global"


def step_plan(f: StepFacts) -> StepPlan:
    """The structure of the step with facts ``f`` (pure); ValueError for the two configurations
    TrainStep refuses."""
    graph = f.graph and f.cuda
    # flat gradients by default on the GPU and whenever there is a process group: written in place
    # by the backward kernels (gradient sinks), stepped by the one-launch FusedAdamW if it can
    flat = (f.pg or f.on_gpu) if f.flat_grads is None else bool(f.flat_grads)
    fused = flat and f.on_gpu and f.fp32_contiguous
    if graph and not fused and f.clip_or_schedule:
        raise ValueError("TrainStep: clip_grad / lr_schedule with graph=True need the one-launch FusedAdamW "
                         "(fp32 contiguous GPU parameters, flat gradients); torch.optim.AdamW applies them "
                         "eagerly from the host")
    if not f.pg:
        collective = "none"
    elif f.on_gpu and f.backend == "gloo":
        collective = "host"
    elif f.two_graphs:
        collective = "between"
    else:
        collective = "overlap"
    if collective != "none" and not flat:
        raise ValueError("TrainStep: the collective path needs the flat gradient buffer")
    overlap = collective == "overlap"
    # flagged: the default for graph steps with the overlapped collective on the GPU; SAE_FLAGGED=0
    # keeps the round-3 structure (the all-reduces forked inside the one graph)
    flagged = overlap and graph and f.on_gpu and f.flagged_on
    sinks = flat and f.grad_sinks
    return StepPlan(
        graph=graph, flat=flat, fused=fused, collective=collective, flagged=flagged,
        two_graphs=collective in ("between", "host") or (collective == "none" and bool(f.two_graphs)) or flagged,
        grad_group=(overlap or collective == "between") and f.on_gpu,
        agree_group=f.world > 1 and graph,
        hooks=flat and overlap, comm_stream=flat and overlap and f.on_gpu,
        sinks=sinks, sink_listener=sinks and overlap,
        wgrad_stream=f.wgrad_stream and sinks and f.on_gpu,
        capturable=graph,
        # thread_local: RCCL's watchdog thread keeps querying the events of the default group's
        # eager work (the parameter broadcast) while the capture runs; a "global" capture would
        # refuse those queries (hipErrorStreamCaptureUnsupported, fatal in the watchdog)
        capture_mode="thread_local" if f.pg else "global")


class TrainStep:
    """``step(images, labels)`` = forward (bf16 compute) + loss + backward (+ bucketed all-reduce of
    the flat gradient when there is a process group) + optimizer update.  No host sync.

    graph=True (GPU): the whole step is one HIP graph (collective "overlap" or "none"); with
    ``two_graphs=True`` (collective "between") or the gloo rehearsal ("host"): graph 1 = forward +
    loss + backward, the bucket all-reduces, graph 2 = AdamW.

    ``clip_grad`` / ``lr_schedule``: the reference's clip_by_global_norm and warm-up-cosine schedule
    (train.py:22-27,214-220).  ``lr_schedule=None`` keeps the constant ``lr * global_batch / 512``; a
    ``WarmupCosine`` is taken as given (``reference_schedule`` builds the reference's).  The clip
    sees the gradient the update consumes -- after the all-reduce in every collective mode: the
    norm is part of the optimizer step, which every mode runs behind its join with the collectives.
    With the one-launch FusedAdamW both live on the device (graph-replayable); with
    ``torch.optim.AdamW`` (CPU or non-fp32 parameters) the same semantics run eagerly in torch ops
    and ``graph=True`` is refused.  ``lr_now`` / ``grad_norm``: the last update's rate and norm.

    ``mix=True``: ``step(images, labels, mix_labels, ratio)``, both extra arguments on every call (the
    captured step copies them into static buffers, ``mix_buffers()``); with ``mix=False`` they are
    refused.  ``metrics=True``: ``top1`` / ``top5``, the fractions of the last step's rank-local batch
    whose first label is among the 1 / 5 largest logits (0-d device tensors, no sync)."""

    def __init__(self, model: torch.nn.Module, global_batch: int, lr: float = 5e-4, weight_decay: float = 1e-4,
                 label_smoothing: float = 0.1, bucket_cap_mb: float = 25.0, device: Optional[torch.device] = None,
                 graph: bool = False, input_layout: str = "NHWC", flat_grads: Optional[bool] = None,
                 grad_sinks: bool = True, two_graphs: Optional[bool] = None, persistent_casts: bool = True,
                 wgrad_stream: Optional[bool] = None, clip_grad: Optional[float] = None,
                 lr_schedule: Optional[WarmupCosine] = None, mix: bool = False, metrics: bool = False):
        self.clip_grad = _check_clip(clip_grad)
        if lr_schedule is not None and not isinstance(lr_schedule, WarmupCosine):
            raise TypeError("TrainStep: lr_schedule must be a WarmupCosine or None")
        # mix: every call carries the batch's mixup / cutmix partner labels and ratios; metrics: the
        # loss kernel also ranks the labels (top1 / top5).  Neither is part of the step's structure
        # (step_plan); with both off the step launches exactly what it launched without them.
        self.mix, self.metrics = bool(mix), bool(metrics)
        self._top1 = self._top5 = None
        self._mix_labels = self._ratio = None
        self.lr_schedule = lr_schedule
        # input_layout "HWCN": the batch arrives as the reference's train-step feed [H, W, C, N]
        # (train.py:80, input_pipeline.py:187-191) and the model's patch GEMM gathers from it
        self.input_layout = input_layout
        self.model = model
        params = [p for p in model.parameters() if p.requires_grad]
        self._params = params
        facts = step_facts(params, graph, flat_grads, grad_sinks, two_graphs, wgrad_stream,
                           self.clip_grad is not None or lr_schedule is not None)
        plan = self.plan = step_plan(facts)   # (a refused configuration raises here: no collective issued yet)
        self.pg, self.world = facts.pg, facts.world
        self.graph, self.flat, self.collective = plan.graph, plan.flat, plan.collective
        self._flagged, self.two_graphs = plan.flagged, plan.two_graphs
        self._g = self._g_opt = None
        # the flat ranges _zero_grad clears (None: the whole buffer); _note_sunk narrows them
        self._zero_ranges = None
        if self.world > 1:
            self._broadcast_from_rank0([t for t in model.state_dict().values() if torch.is_tensor(t)])
        dev = params[0].device
        # the gradient all-reduces run on a process group of their own (GradReducer)
        grad_pg = dist.new_group(backend="nccl", device_id=dev) if plan.grad_group else None
        # world > 1: whether the step runs as a graph is decided by ALL ranks together (a host-side
        # gloo group carries the one flag all-reduce): a rank whose capture fails must not run the
        # eager step while its peers replay graphs -- their collective sequences would differ
        self._flag_pg = dist.new_group(backend="gloo") if plan.agree_group else None
        self.reducer = None
        if plan.flat:
            self._build_flat(dev, max(1, int(bucket_cap_mb * 2 ** 20 / 4)), grad_pg)
        # the sink-bound weight-gradient GEMMs run on a side stream beside the input-gradient chain
        # (GradSinks.wgrad_stream), opt-in: SAE_WG_STREAM=1 or wgrad_stream=True.  Off by default: the
        # concurrent dW kernels push the persistent gemm8 tiles into a tail (DeiT-S 15,381 vs
        # 15,619 img/s, profiles/r05i_wgstream_rejected.txt)
        self._wg = torch.cuda.Stream(device=dev) if plan.wgrad_stream else None
        # the backward kernels write each parameter's gradient straight into its flat view (this step's
        # GradSinks, live inside _fwd_bwd's window) instead of autograd adding a fresh tensor into it
        self._sinks = None
        if plan.sinks:
            self._sinks = GradSinks(params, [p.grad for p in params], wgrad_stream=self._wg,
                                    listener=self.reducer.on_sink if plan.sink_listener else None)
        self.opt = self._build_optimizer(lr * (global_batch / 512), weight_decay, persistent_casts)
        self.smoothing = label_smoothing
        # dropout (attn_dropout_rate > 0 or dropout_rate > 0 on any module): the first operation
        # of each step bumps the device offset of the dropout state (ops.DropoutRng.advance), so
        # every step -- every replay of the captured graph included -- draws fresh masks.  With
        # rate 0 everywhere the step launches nothing for it.
        self._drop_rng = None
        if facts.on_gpu and any(getattr(m, "attn_dropout_rate", 0.0) > 0.0 or getattr(m, "dropout_rate", 0.0) > 0.0
                                for m in model.modules()):
            self._drop_rng = ops.dropout_rng(dev)

    def _build_flat(self, dev, cap_elems, grad_pg):
        """One flat fp32 gradient buffer, every .grad a 16-byte-aligned view into it (autograd
        accumulates into the views in place); with a collective, its buckets of >= ``cap_elems``
        elements and their all-reduce (GradReducer), told by hooks about the gradients autograd
        accumulates."""
        params, plan = self._params, self.plan
        self._offs, n = flat_layout(params)
        # zeros: the alignment padding between the views is never written by anything (the
        # kernels and autograd write the views, _zero_grad writes zeros, a SUM all-reduce of
        # zeros is zero), so it stays zero and the global norm may run over the whole buffer
        self._flat = torch.zeros(n, dtype=torch.float32, device=dev)
        for p, off in zip(params, self._offs):
            p.grad = self._flat[off:off + p.numel()].view_as(p)
        if plan.collective != "none":
            self.reducer = reducer = GradReducer(
                self._flat, self._offs, cap_elems, mode=plan.collective, group=grad_pg,
                comm_stream=plan.comm_stream, flagged=plan.flagged,
                emulate=parse_emulate_rccl(os.environ.get("SAE_EMULATE_RCCL", "")))
        if plan.hooks:
            for i, p in enumerate(params):
                p.register_post_accumulate_grad_hook(lambda _p, i=i: reducer.on_ready(i))

    def _build_optimizer(self, lr, weight_decay, persistent_casts):
        kw = dict(lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay)
        if self.plan.fused:
            # the bf16 Dense copies written by the update (models that name them, bf16 compute)
            model = self.model
            groups = model.cast_groups() if persistent_casts and hasattr(model, "cast_groups") else None
            return FusedAdamW(self._params, self._flat, cast_groups=groups, clip_grad=self.clip_grad,
                              lr_schedule=self.lr_schedule, **kw)
        # the torch optimizer: clip and schedule in torch ops before its step (_opt_step)
        self._count = 0
        self._lr_now = self._grad_norm = None
        if self.plan.capturable:
            kw["capturable"] = True   # step counters on the device: replayable
        try:
            return torch.optim.AdamW(self._params, fused=True, **kw)
        except (RuntimeError, TypeError):
            return torch.optim.AdamW(self._params, foreach=True, **kw)

    @staticmethod
    def _broadcast_from_rank0(tensors):
        """Once, at construction: every replica starts from rank 0's parameters and buffers (the
        reference's pmap replicates one host-initialised state, train.py:226-228), whatever seed
        each rank used.  One flat broadcast per dtype, not one per tensor."""
        by_dtype = {}
        for t in tensors:
            by_dtype.setdefault(t.dtype, []).append(t)
        for ts in by_dtype.values():
            flat = torch.cat([t.detach().reshape(-1) for t in ts])
            if flat.is_cuda and dist.get_backend() == "gloo":
                host = flat.cpu()
                dist.broadcast(host, src=0)
                flat.copy_(host)
            else:
                dist.broadcast(flat, src=0)
            off = 0
            with torch.no_grad():
                for t in ts:
                    t.copy_(flat[off:off + t.numel()].view_as(t))
                    off += t.numel()

    # ---- pieces of one step
    def _zero_grad(self):
        if self.flat:
            if self._zero_ranges is None:
                self._flat.zero_()
            else:   # only the gradients autograd accumulates (every sink is overwritten)
                for lo, hi in self._zero_ranges:
                    self._flat[lo:hi].zero_()
        else:
            self.opt.zero_grad(set_to_none=True)

    def _note_sunk(self):
        """After a graph-mode backward: the flat ranges of the parameters whose gradients did NOT
        go through a sink (autograd adds into those, so they need zeroing before the next
        backward).  Graph mode only: the captured step writes the same sinks on every replay."""
        ranges = []
        for p, off in zip(self._params, self._offs):
            n = p.numel()
            if p.grad is None or p.grad.data_ptr() not in self._sinks.written:
                if ranges and ranges[-1][1] == off:
                    ranges[-1] = (ranges[-1][0], off + n)
                else:
                    ranges.append((off, off + n))
        # many scattered ranges would cost more launches than the one full fill saves
        self._zero_ranges = ranges if len(ranges) <= 8 else None

    def _fwd_bwd(self, images: torch.Tensor, labels: torch.Tensor, mix_labels=None, ratio=None) -> torch.Tensor:
        if self._drop_rng is not None:
            self._drop_rng.advance()
        self._zero_grad()
        sinks = self._sinks
        # the sink window (this step's forward + backward only) and, inside it, the reducer's: its
        # end launches what is left and joins the collectives, after every weight gradient is written
        with sinks.backward() if sinks is not None else contextlib.nullcontext(), \
                self.reducer.window() if self.collective == "overlap" else contextlib.nullcontext():
            if self.input_layout == "NHWC":
                logits = self.model(images, is_training=True)
            else:
                logits = self.model(images, is_training=True, layout=self.input_layout)
            if self.mix or self.metrics:
                loss = mixed_cross_entropy(logits, labels, mix_labels, ratio, self.smoothing, self.metrics)
                if self.metrics:
                    loss, self._top1, self._top5 = loss
            else:   # the same loss (_cross_entropy_rows), named by the module global tools/ab_loss.sh replaces
                loss = smoothed_cross_entropy(logits, labels, self.smoothing)
            # world > 1: the SUM all-reduce of the per-rank gradients of loss / world is the
            # gradient of the global-batch mean (survey D9)
            (loss / self.world if self.world > 1 else loss).backward()
            if sinks is not None:
                sinks.join()   # every weight gradient written before the update
        if sinks is not None and self.graph and not torch.cuda.is_current_stream_capturing():
            self._note_sunk()
        return loss.detach()

    def _between(self, replayed: bool = False):
        """The collectives between the forward + backward and the optimizer (GradReducer.between)."""
        if self.reducer is not None:
            self.reducer.between(replayed)

    def _opt_step(self):
        """The optimizer step.  FusedAdamW clips and schedules on the device; for torch.optim.AdamW
        the same chain in torch ops: the global norm of every gradient (fp64 sum of squares), optax's
        clip factor multiplied into the gradients in place, the schedule's value at the number of
        updates applied written to the parameter groups."""
        if isinstance(self.opt, FusedAdamW) or (self.clip_grad is None and self.lr_schedule is None):
            self.opt.step()
            return
        if self.clip_grad is not None:
            grads = [p.grad for p in self._params if p.grad is not None]
            norm = torch.stack([g.double().square().sum() for g in grads]).sum().sqrt().float()
            scale = torch.where(norm < self.clip_grad, torch.ones_like(norm), self.clip_grad / norm)
            torch._foreach_mul_(grads, scale)   # a NaN norm reaches every gradient: nothing is skipped
            self._grad_norm = norm
        if self.lr_schedule is not None:
            self._lr_now = self.lr_schedule.value(self._count)
            for group in self.opt.param_groups:
                group["lr"] = self._lr_now
        self._count += 1
        self.opt.step()

    @property
    def lr_now(self):
        """The rate of the last update: a 0-d device tensor (FusedAdamW, no sync) or a float; None
        when neither clip_grad nor lr_schedule is set."""
        return self.opt.lr_now if isinstance(self.opt, FusedAdamW) else self._lr_now

    @property
    def grad_norm(self):
        """The global gradient norm (before clipping) of the last update, a 0-d tensor; None without
        clip_grad."""
        return self.opt.grad_norm if isinstance(self.opt, FusedAdamW) else self._grad_norm

    @property
    def top1(self):
        """The fraction of the last step's rank-local batch whose label had the largest logit (stable
        argsort order, utils.topk_correct): a 0-d device tensor, no sync; None without ``metrics``."""
        return self._top1

    @property
    def top5(self):
        """... whose label was among the five largest logits."""
        return self._top5

    def _eager(self, images: torch.Tensor, labels: torch.Tensor, mix_labels=None, ratio=None) -> torch.Tensor:
        loss = self._fwd_bwd(images, labels, mix_labels, ratio)
        self._between()
        self._opt_step()
        return loss

    def _opt_snapshot(self):
        """The optimizer's state: FusedAdamW's tensors, or torch.optim.AdamW's per-parameter dicts."""
        if isinstance(self.opt, FusedAdamW):
            return [t.clone() for t in self.opt.state_tensors()]
        return {id(p): {k: (v.clone() if torch.is_tensor(v) else v) for k, v in self.opt.state[p].items()}
                for p in self._params if p in self.opt.state and self.opt.state[p]}

    def _opt_restore(self, snap):
        if isinstance(self.opt, FusedAdamW):
            for t, v in zip(self.opt.state_tensors(), snap):
                t.copy_(v)
            self.opt.refresh_casts()   # the bf16 copies of the restored weights
            return
        for p in self._params:
            old = snap.get(id(p))
            for k, v in (self.opt.state.get(p) or {}).items():
                if not torch.is_tensor(v):
                    continue
                if old is not None and torch.is_tensor(old.get(k)):
                    v.copy_(old[k])
                else:   # state created by the warm-up: a fresh optimizer's zeros
                    v.zero_()

    def _warm_up(self):
        """Two eager steps on a side stream before the capture (allocator, library and optimizer
        state) with the collectives off -- the gradient group stays free of eager work until its
        collectives are captured (GradReducer) -- and then everything they changed put back, so that
        the first call performs exactly ONE update (the reference's one update per batch,
        train.py:94-100)."""
        dev = self._images.device
        snap = [p.detach().clone() for p in self._params]
        # buffers a training forward advances (the BatchNorm running statistics of a CvT; none in the
        # other models): put back too, so the first call moves them once
        bufs = list(self.model.buffers())
        snap_buf = [t.detach().clone() for t in bufs]
        snap_opt = self._opt_snapshot()
        snap_rng = self._drop_rng.state.clone() if self._drop_rng is not None else None
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with self.reducer.paused() if self.reducer is not None else contextlib.nullcontext():
            with torch.cuda.stream(s):
                for _ in range(2):
                    self._eager(self._images, self._labels, self._mix_labels, self._ratio)
        torch.cuda.current_stream(dev).wait_stream(s)
        with torch.no_grad():
            for p, v in zip(self._params, snap):
                p.copy_(v)
            for t, v in zip(bufs, snap_buf):
                t.copy_(v)
            if snap_rng is not None:   # the warm-up steps advanced the dropout offset
                self._drop_rng.state.copy_(snap_rng)
            self._opt_restore(snap_opt)
        if not self.flat:
            self.opt.zero_grad(set_to_none=True)

    def _capture(self, images: torch.Tensor, labels: torch.Tensor, mix_labels=None, ratio=None):
        self._images = images.clone()
        self._labels = labels.clone()
        if self.mix:
            self._mix_labels = mix_labels.clone()
            self._ratio = ratio.to(torch.float32).clone()
        self._warm_up()
        mode = self.plan.capture_mode
        try:
            if not self.two_graphs:     # the whole step (with the overlapped collectives) in one graph
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode=mode):
                    self._loss = self._eager(self._images, self._labels, self._mix_labels, self._ratio)
                self._g = g
            else:                 # the collectives stay outside: two graphs around them
                g, go = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
                if self.reducer is not None:
                    self.reducer.reset_flag_order()
                with torch.cuda.graph(g, capture_error_mode=mode):
                    self._loss = self._fwd_bwd(self._images, self._labels, self._mix_labels, self._ratio)
                with torch.cuda.graph(go, capture_error_mode=mode):
                    self._opt_step()
                self._g, self._g_opt = g, go
            ok = True
        except RuntimeError as e:   # an op that cannot be captured: stay eager, say so once
            import sys
            print(f"[train] HIP-graph capture failed ({e}); running the eager step", file=sys.stderr)
            ok = False
        self._settle_capture(ok)

    def _settle_capture(self, ok: bool):
        """Keep the captured graph(s) or go eager -- at world > 1 on every rank alike (one MIN flag
        all-reduce over the gloo group): a rank whose capture failed would otherwise run the eager
        step's collectives while its peers replay graphs."""
        if self._flag_pg is not None:
            ok = agree_all_ranks(ok, self._flag_pg)
        if not ok:
            self.graph = False
            self._g = self._g_opt = None
            if torch.cuda.is_available():
                torch.cuda.synchronize()

    def close(self):
        """Release the captured graphs and the optimizer's persistent bf16 copies.  With a process
        group, call it BEFORE destroy_process_group: a graph whose capture holds RCCL collectives
        keeps communicator resources that its destruction releases, so it must not outlive the
        communicator (left to the garbage collector, it was destroyed at an arbitrary later point)."""
        if self._g is not None or self._g_opt is not None:
            torch.cuda.synchronize()
        self._g = self._g_opt = None
        if self.reducer is not None:
            self.reducer.close()
        if self._flag_pg is not None and dist.is_initialized():
            dist.destroy_process_group(self._flag_pg)
            self._flag_pg = None
        if isinstance(self.opt, FusedAdamW):
            self.opt.close()

    def input_buffers(self):
        """(images, labels): the captured graph's static input buffers, once the first call has
        captured it (None otherwise).  A loader that writes each batch into them saves the copy a
        call with other tensors makes before the replay."""
        if self._g is None:
            return None
        return self._images, self._labels

    def mix_buffers(self):
        """(mix_labels, ratio): the captured graph's static buffers of a ``mix=True`` step, once the
        first call has captured it (None otherwise), for a loader to write into like ``input_buffers``."""
        if self._g is None or not self.mix:
            return None
        return self._mix_labels, self._ratio

    def __call__(self, images: torch.Tensor, labels: torch.Tensor, mix_labels: Optional[torch.Tensor] = None,
                 ratio: Optional[torch.Tensor] = None) -> torch.Tensor:
        if self.mix and (mix_labels is None or ratio is None):
            raise ValueError("TrainStep(mix=True): every call needs mix_labels and ratio")
        if not self.mix and (mix_labels is not None or ratio is not None):
            raise ValueError("TrainStep: mix_labels / ratio need mix=True")
        if not self.graph:
            return self._eager(images, labels, mix_labels, ratio)
        if self._g is None:
            self._capture(images, labels, mix_labels, ratio)
            if not self.graph:
                return self._eager(images, labels, mix_labels, ratio)
        if images.data_ptr() != self._images.data_ptr():
            self._images.copy_(images)
        if labels.data_ptr() != self._labels.data_ptr():
            self._labels.copy_(labels)
        if self.mix:
            if mix_labels.data_ptr() != self._mix_labels.data_ptr():
                self._mix_labels.copy_(mix_labels)
            if ratio.data_ptr() != self._ratio.data_ptr():
                self._ratio.copy_(ratio)
        if isinstance(self.opt, FusedAdamW):
            self.opt.refresh_casts(only_if_stale=True)
        self._g.replay()
        if self._g_opt is not None:
            self._between(replayed=True)
            self._g_opt.replay()
        return self._loss


class EvalStep:
    """``step(images, labels)`` = the reference's eval_step (train.py:112-120): a forward with
    ``is_training=False`` under ``torch.no_grad()`` and the plain one-hot cross entropy (the mixed loss
    with alpha = 0 and no partner labels), with the top-1 / top-5 ranks from the same kernel, added
    into a device accumulator {double loss_sum; int64 top1, top5, samples} (``sae_ce_accumulate``).
    Returns the batch's mean loss as a 0-d device tensor; no host sync.  It never advances the dropout
    state and never touches ``.grad``.

    graph=True (GPU): captured once and replayed with static ``images`` / ``labels``.  The graph reads
    the bf16 Dense copies a ``FusedAdamW`` keeps current (refreshed before a replay if a weight was
    changed in place outside the update); when no optimizer owns them it holds the casts from the
    current fp32 weights itself.  When the copies change hands (an optimizer is built or closed) the
    next call captures again.

    ``result()`` is the one sync: the accumulator, summed over the default process group when there is
    one, as per-sample means ``{"loss", "top_1_acc", "top_5_acc", "samples"}``.  (The reference sums
    per-batch mean losses and divides by the sample count, train.py:240-250; see DESIGN.)  ``reset()``
    zeroes the accumulator.  CPU tensors run the same steps in torch ops."""

    def __init__(self, model: torch.nn.Module, device: Optional[torch.device] = None, graph: bool = False,
                 input_layout: str = "NHWC"):
        self.model, self.input_layout = model, input_layout
        dev = torch.device(device) if device is not None else next(model.parameters()).device
        self.device = dev
        self.graph = bool(graph) and dev.type == "cuda" and torch.cuda.is_available()
        # {double loss_sum; int64 top1, top5, samples} (ops.ce_accumulator_fields)
        self._acc = torch.zeros(L.SAE_CE_ACCUM_BYTES // 8, dtype=torch.int64, device=dev)
        self._g = self._images = self._labels = self._loss = None
        self._cast_entries = ()

    def _groups(self):
        groups = self.model.cast_groups() if hasattr(self.model, "cast_groups") else None
        return groups or []

    def _step(self, images: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        with torch.no_grad():
            if self.input_layout == "NHWC":
                logits = self.model(images, is_training=False)
            else:
                logits = self.model(images, is_training=False, layout=self.input_layout)
            loss, _, row_loss, rank = _cross_entropy_rows(logits, labels, None, None, 0.0, True)
            if logits.is_cuda:
                ops.ce_accumulate(row_loss, rank, self._acc)
                return loss
            loss_sum, counts = ops.ce_accumulator_fields(self._acc)
            loss_sum += row_loss.double().sum()
            counts += torch.stack([(rank < 1).sum(), (rank < 5).sum(), torch.tensor(rank.numel())])
            return row_loss.mean()

    def _capture(self, images: torch.Tensor, labels: torch.Tensor):
        dev = self.device
        self._images, self._labels = images.clone(), labels.clone()
        # one eager step on a side stream (allocator, library state), its accumulation taken back
        snap = self._acc.clone()
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            self._step(self._images, self._labels)
        torch.cuda.current_stream(dev).wait_stream(s)
        self._acc.copy_(snap)
        self._cast_entries = ops.persistent_cast_entries(self._groups())
        try:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local" if dist.is_initialized() else "global"):
                self._loss = self._step(self._images, self._labels)
            self._g = g
        except RuntimeError as e:   # an op that cannot be captured: stay eager, say so once
            import sys
            print(f"[eval] HIP-graph capture failed ({e}); running the eager step", file=sys.stderr)
            self.graph, self._g = False, None
            torch.cuda.synchronize()

    def __call__(self, images: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        if not self.graph:
            return self._step(images, labels)
        groups = self._groups()
        now = ops.persistent_cast_entries(groups)
        if self._g is not None and (len(now) != len(self._cast_entries)
                                    or any(a is not b for a, b in zip(now, self._cast_entries))):
            torch.cuda.synchronize()
            self._g = None   # the copies the graph reads changed hands: capture again
        if self._g is None:
            self._capture(images, labels)
            if not self.graph:
                return self._step(images, labels)
        if images.data_ptr() != self._images.data_ptr():
            self._images.copy_(images)
        if labels.data_ptr() != self._labels.data_ptr():
            self._labels.copy_(labels)
        ops.refresh_persistent_casts(groups, only_if_stale=True)
        self._g.replay()
        return self._loss

    def input_buffers(self):
        """(images, labels): the captured graph's static input buffers (None before the capture)."""
        return None if self._g is None else (self._images, self._labels)

    def reset(self):
        self._acc.zero_()

    def result(self) -> dict:
        """The totals since the last ``reset()`` over every rank, as per-sample means (one host sync; the
        SUM all-reduce goes through the host for gloo)."""
        total = self._acc.clone()
        if dist.is_initialized() and dist.get_world_size() > 1:
            if total.is_cuda and dist.get_backend() == "gloo":
                total = total.cpu()
            for field in ops.ce_accumulator_fields(total):   # a double and three integers: one SUM each
                dist.all_reduce(field)
        loss_sum, top1, top5, n = ops.read_ce_accumulator(total)
        d = max(n, 1)
        return {"loss": loss_sum / d, "top_1_acc": top1 / d, "top_5_acc": top5 / d, "samples": n}

    def close(self):
        """Release the captured graph."""
        if self._g is not None:
            torch.cuda.synchronize()
        self._g = None
