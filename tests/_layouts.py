"""Strided, padded and misaligned layouts of the eight attention tensors (q, k, v, o, dout, dq, dk,
dv of ``sae_attn_desc``): arenas, views, guards and launch helpers shared by
``test_layouts_cpu.py`` (routing, coverage and self-tests, no device) and ``test_gpu_layouts.py``.

A *plan* places every tensor of a case as a ``[B, N, H, D]`` view with unit innermost stride inside
an *arena*: a flat buffer with a guard before the first and after the last element any view of it
touches.  The guard is at least the largest tensor extent of the case, and at least the extent of any
tensor addressed with any mix of the eight tensors' strides.  A kernel that takes another tensor's
stride, assumes a stride it was not given or overruns a ragged tile then lands inside an arena, where
``assert_guards_intact`` sees it, instead of outside the allocation.

Every arena is filled with ``SENTINEL[dtype]``, one fixed bit pattern that is a NaN in its dtype, before
the input values are written into the views: the padding rows and columns next to every input are
NaN (a result that depends on them cannot pass a parity check), and every element outside the output
views must still carry the pattern after a call (compared as integers, so NaN-safe).

Layouts (``epc`` = elements per 16 bytes: 8 for bf16, 4 for fp32):
  contig          the control: eight contiguous tensors (each in a guarded arena of its own)
  distinct        tensor i in its own arena, head stride D + epc*i, token stride H*head + epc*(i+1),
                  batch stride N*token + epc*(2i+1): all eight values differ in each stride position,
                  every stride a multiple of epc and every base 16-byte aligned (the vector route)
  kv_packed       k / v interleaved in one [B, Nk, 2, H, D] arena and dk / dv in another (the CvT /
                  class-attention projection form); q, o, dout, dq contiguous
  head_major      [B, H, N, D] buffers viewed as [B, N, H, D]: token stride D (the smallest legal
                  one), head stride N*D
  misaligned_ptr  the distinct strides with every base pointer one element past a 16-byte boundary
  odd_stride      the distinct strides with epc/2 added to the token stride of k and of dq
The last two fail the vector predicate (csrc/desc.h ``desc_vec``: pointers, strides) and take the
scalar v1 / ``th_*_scalar`` kernels; so does every layout of a case whose head_dim is no multiple of
epc.
"""
import ctypes

import numpy as np

from sae_vision_amd import _lib as L

TENSORS = ("q", "k", "v", "o", "dout", "dq", "dk", "dv")     # the descriptor's order
KEYED = ("k", "v", "dk", "dv")                               # [B, Nk, H, D]; the others [B, Nq, H, D]
INPUTS = ("q", "k", "v", "dout")
OUTPUTS = ("o", "dq", "dk", "dv")
LAYOUTS = ("contig", "distinct", "kv_packed", "head_major", "misaligned_ptr", "odd_stride")
SCALAR_LAYOUTS = ("misaligned_ptr", "odd_stride")
EPC = {"bf16": 8, "f32": 4}
# a NaN in its dtype (exponent all ones, mantissa != 0), as the signed integer of the element's width
SENTINEL = {"bf16": 0x7FA5, "f32": 0x7FA5A5A5}
GUARD_ALIGN = 64   # guards are whole multiples of this many elements, so aligned bases stay aligned

FWD, BWD = L.SAE_PASS_FWD, L.SAE_PASS_BWD
PLAIN, ROT, DROP = L.SAE_FORM_PLAIN, L.SAE_FORM_ROTARY, L.SAE_FORM_DROPOUT
BF16, F32 = L.SAE_DTYPE_BF16, L.SAE_DTYPE_F32
DTYPE_CODE = {"bf16": BF16, "f32": F32}
ROPE_BASE = 10000.0
DROP_RATE = 0.5      # T = 128

# why a scalar layout has no route (sae_last_error of the route query starts with it)
NO_ROTARY = "rotary: fused only on the bf16 path"
NO_TH_ROTARY = "rotary: fused only on the bf16 talking-heads path (aligned strides)"


def no_th_heads(H):
    return f"talking heads: {H} heads > 8 on the fp32 / unaligned path"


# ------------------------------------------------------------------ descriptors and route queries
def desc(lib, Nq, Nk, D, H=4, dtype=BF16, grid=None, B=2):
    """A contiguous descriptor (``sae_attn_desc_init``), with the relative-logit grid if given."""
    d = L.SaeAttnDesc()
    lib.sae_attn_desc_init(ctypes.byref(d), B, H, Nq, Nk, D, dtype, 0.125)
    if grid is not None:
        d.flags, d.rel_h, d.rel_w = L.SAE_FLAG_RELPOS, grid[0], grid[1]
    return d


def route(lib, fn, d, pas, form, aligned=1):
    """``sae_attn_route`` / ``sae_th_attn_route`` as a str, or None where the call is refused."""
    r = getattr(lib, fn)(ctypes.byref(d), pas, form, aligned)
    return None if r is None else r.decode()


# ------------------------------------------------------------------------------ route names
def pair(sfx):
    return f"bwd2_dq_{sfx}+bwd2_dkdv_{sfx}"


def v1(pas, dtype, dp, sfx="", scalar=False):
    """The v1 kernels' route of one pass (attn.hip ``plan_name``): dtype, padded head dim, scalar,
    then ``_rel`` / ``_drop``."""
    inst = f"_{dtype}_d{dp}" + ("_scalar" if scalar else "") + sfx
    return "v1_fwd" + inst if pas == FWD else f"v1_bwd_dq{inst}+v1_bwd_dkdv{inst}"


def th2_bwd(q, kv):
    return f"th2_bwd_q_{q}+th2_bwd_kv_{kv}+th_reduce"


def th_v1(pas, dtype, dp, scalar=False):
    inst = f"_{dtype}_d{dp}" + ("_scalar" if scalar else "")
    return "th_fwd" + inst if pas == FWD else f"th_bwd_q{inst}+th_bwd_kv{inst}+th_reduce"


def pad_dim(D):
    """The kernels' padded head dim (csrc ``pick_dp``)."""
    return 32 if D <= 32 else 64 if D <= 64 else 128


class Refused:
    """In place of a route: the entry point refuses the call; ``text`` starts its message."""

    def __init__(self, text):
        self.text = text

    def __repr__(self):
        return f"Refused({self.text!r})"


class Case:
    """One row of the layout matrix.  ``kind``: plain | rel | rot | drop | th | th_rot.  ``fwd`` /
    ``bwd`` are the routes the case is meant to serve on a vector layout, exactly as the route query
    names them; ``fwd_scalar`` / ``bwd_scalar`` the routes (or the ``Refused``) of a scalar layout."""

    def __init__(self, kind, D, fwd, bwd, fwd_scalar, bwd_scalar, H=3, Nq=150, Nk=70, dtype="bf16", grid=None, B=2):
        self.kind, self.B, self.Nq, self.Nk, self.H, self.D, self.dtype, self.grid = kind, B, Nq, Nk, H, D, dtype, grid
        self.fwd, self.bwd, self.fwd_scalar, self.bwd_scalar = fwd, bwd, fwd_scalar, bwd_scalar
        if grid is not None:
            assert Nk == grid[0] * grid[1]

    @property
    def id(self):
        g = "" if self.grid is None else f"_{self.grid[0]}x{self.grid[1]}"
        return f"{self.kind}_{self.dtype}_nq{self.Nq}_nk{self.Nk}_h{self.H}_d{self.D}{g}"

    @property
    def th(self):
        return self.kind in ("th", "th_rot")

    @property
    def form(self):
        return {"rot": ROT, "th_rot": ROT, "drop": DROP}.get(self.kind, PLAIN)

    @property
    def route_fn(self):
        return "sae_th_attn_route" if self.th else "sae_attn_route"

    @property
    def epc(self):
        return EPC[self.dtype]

    def shape(self, name):
        return (self.B, self.Nk if name in KEYED else self.Nq, self.H, self.D)

    def declared(self, pas, scalar):
        return {(FWD, False): self.fwd, (BWD, False): self.bwd,
                (FWD, True): self.fwd_scalar, (BWD, True): self.bwd_scalar}[(pas, bool(scalar))]

    def steps(self):
        """Every kernel instance one of the declared routes names."""
        return {s for r in (self.fwd, self.bwd, self.fwd_scalar, self.bwd_scalar)
                if not isinstance(r, Refused) for s in r.split("+")}


def is_scalar(case, layout):
    """Whether ``layout`` fails the 16-byte vector predicate for ``case`` (declared, not measured:
    ``test_layouts_cpu.py`` checks it against the plan's strides)."""
    return layout in SCALAR_LAYOUTS or case.D % case.epc != 0


def gpu_layouts(case):
    """The non-control layouts that run on the GPU for ``case``: all but the refused scalar ones."""
    return [lay for lay in LAYOUTS[1:]
            if not isinstance(case.declared(FWD, is_scalar(case, lay)), Refused)]


# ------------------------------------------------------------------------------------ plans
class View:
    """Where one tensor lives: ``arena`` (a key of ``Plan.arenas``), the element ``offset`` of
    [0, 0, 0, 0] in it, ``shape`` [B, N, H, D] and the (batch, token, head) element ``strides``."""

    def __init__(self, name, arena, offset, shape, strides):
        self.name, self.arena, self.offset, self.shape, self.strides = name, arena, offset, shape, tuple(strides)

    @property
    def extent(self):
        """One past the largest element offset (from ``offset``) the view touches."""
        B, N, H, D = self.shape
        sb, st, sh = self.strides
        return (B - 1) * sb + (N - 1) * st + (H - 1) * sh + D

    def indices(self):
        """The arena indices of every element, as an int64 numpy array [B, N, H, D]."""
        B, N, H, D = self.shape
        sb, st, sh = self.strides
        ix = np.arange
        return (self.offset + ix(B)[:, None, None, None] * sb + ix(N)[None, :, None, None] * st +
                ix(H)[None, None, :, None] * sh + ix(D)[None, None, None, :])


class Plan:
    def __init__(self, case, layout, views, arenas, guard):
        self.case, self.layout, self.views, self.arenas, self.guard = case, layout, views, arenas, guard

    @property
    def aligned(self):
        """Every base pointer 16-byte aligned (arenas themselves are, as every allocation is)."""
        return all(v.offset % self.case.epc == 0 for v in self.views.values())

    def strides(self, name):
        return self.views[name].strides

    def views_of(self, arena):
        return [v for v in self.views.values() if v.arena == arena]


def _contig(shape):
    B, N, H, D = shape
    return (N * H * D, H * D, D)


def _distinct(case, i, shape, extra_token=0):
    e = case.epc
    B, N, H, D = shape
    sh = D + e * i
    st = H * sh + e * (i + 1) + extra_token
    return (N * st + e * (2 * i + 1), st, sh)


def plan(case, layout):
    """Strides, offsets and arena sizes of the eight tensors of ``case`` under ``layout`` (integers
    only: no tensor is made)."""
    assert layout in LAYOUTS, layout
    e = case.epc
    st, lead, arena_of = {}, 0, {n: n for n in TENSORS}
    for i, n in enumerate(TENSORS):
        shape = case.shape(n)
        B, N, H, D = shape
        if layout in ("contig", "kv_packed"):
            st[n] = _contig(shape)
        elif layout == "head_major":
            st[n] = (H * N * D, D, N * D)
        elif layout == "odd_stride":
            st[n] = _distinct(case, i, shape, e // 2 if n in ("k", "dq") else 0)
        else:
            st[n] = _distinct(case, i, shape)
    if layout == "misaligned_ptr":
        lead = 1
    inner = {n: 0 for n in TENSORS}     # offset past the leading guard
    if layout == "kv_packed":
        B, Nk, H, D = case.shape("k")
        for a, b, arena in (("k", "v", "kv"), ("dk", "dv", "dkdv")):
            st[a] = st[b] = (Nk * 2 * H * D, 2 * H * D, D)
            inner[b] = H * D
            arena_of[a] = arena_of[b] = arena
    views = {n: View(n, arena_of[n], 0, case.shape(n), st[n]) for n in TENSORS}
    # the guard: the extent of the longest tensor, and one row more, under the largest stride of each
    # position, which no tensor's own extent exceeds -- nor does any tensor addressed with another
    # one's strides, nor a store one row past a ragged tile
    worst = View("", "", 0, (case.B, max(case.Nq, case.Nk) + 1, case.H, case.D),
                 [max(s[pos] for s in st.values()) for pos in range(3)])
    guard = -(-worst.extent // GUARD_ALIGN) * GUARD_ALIGN
    arenas = {}
    for n, v in views.items():
        v.offset = guard + lead + inner[n]
        arenas[v.arena] = max(arenas.get(v.arena, 0), v.offset + v.extent + guard)
    return Plan(case, layout, views, arenas, guard)


def plan_desc(lib, p):
    """The descriptor of a plan from its stride triples alone (all eight)."""
    c = p.case
    d = desc(lib, c.Nq, c.Nk, c.D, c.H, DTYPE_CODE[c.dtype], c.grid, c.B)
    for n, field in zip(TENSORS, ("q_stride", "k_stride", "v_stride", "o_stride", "do_stride", "dq_stride",
                                  "dk_stride", "dv_stride")):
        setattr(d, field, L.s3(p.strides(n)))
    return d


# -------------------------------------------------------------------------- arenas and guards
def _torch_dtypes(dtype):
    import torch
    return (torch.bfloat16, torch.int16) if dtype == "bf16" else (torch.float32, torch.int32)


def make_arena(numel, dtype, device):
    """A flat tensor of ``numel`` elements, every one the sentinel NaN."""
    import torch
    td, ti = _torch_dtypes(dtype)
    a = torch.empty(numel, dtype=td, device=device)
    a.view(ti).fill_(SENTINEL[dtype])
    return a


def materialise(p, device, values=None):
    """The arenas of plan ``p`` on ``device`` and the eight ``[B, N, H, D]`` views into them;
    ``values`` (name -> array [B, N, H, D]) are written through the views.  Returns (arenas, views)."""
    import torch
    td, _ = _torch_dtypes(p.case.dtype)
    arenas = {k: make_arena(n, p.case.dtype, device) for k, n in p.arenas.items()}
    views = {}
    for n, v in p.views.items():
        views[n] = torch.as_strided(arenas[v.arena], v.shape, v.strides + (1,), v.offset)
    for n, x in (values or {}).items():
        views[n].copy_(torch.as_tensor(np.asarray(x, np.float32)).to(device=device, dtype=td))
    return arenas, views


def assert_guards_intact(arena, *views):
    """Every element of ``arena`` outside ``views`` (tensors that are views of it) still carries the
    sentinel bit pattern: compared as integers, so NaN-safe."""
    import torch
    dtype = "bf16" if arena.dtype == torch.bfloat16 else "f32"
    _, ti = _torch_dtypes(dtype)
    assert arena.dim() == 1 and arena.is_contiguous()
    flat = torch.arange(arena.numel(), device=arena.device)
    inside = torch.zeros(arena.numel(), dtype=torch.bool, device=arena.device)
    for v in views:
        assert v.untyped_storage().data_ptr() == arena.untyped_storage().data_ptr(), "not a view of this arena"
        inside[torch.as_strided(flat, v.shape, v.stride(), v.storage_offset() - arena.storage_offset())] = True
    bad = torch.nonzero((arena.view(ti) != SENTINEL[dtype]) & ~inside).flatten()
    if bad.numel():
        first = int(inside.nonzero()[0]) if inside.any() else 0
        raise AssertionError(f"{bad.numel()} element(s) written outside the tensor, the first at arena offset "
                             f"{int(bad[0])} (the view starts at {first}, the arena holds {arena.numel()})")


def check_outputs_guards(p, arenas, views, names):
    """``assert_guards_intact`` for the arenas of the output tensors ``names``."""
    for arena in sorted({p.views[n].arena for n in names}):
        try:
            assert_guards_intact(arenas[arena], *(views[v.name] for v in p.views_of(arena)))
        except AssertionError as e:
            raise AssertionError(f"{p.case.id} / {p.layout}: arena '{arena}': {e}") from None


# ------------------------------------------------------------------------------ launch helpers
# The C entry points called as ops._fwd / ops._bwd / ops._th_fwd / ops._th_bwd call them, with the
# caller's own o (ops allocates a contiguous one).  ``t``: name -> view.  ``rope`` = (sin, cos) fp32
# tables, ``drop`` = (rate, state tensor, stream id), ``bias`` = (bias_h, bias_w), all contiguous.
def _call_args(t):
    import sae_vision_amd.ops as ops
    return L.load(), ops._stream(t["q"]), ops._ptr


def run_fwd(t, scale, bias=None, grid=None, rope=None, drop=None):
    """sae_attn_fwd / _rotary / _dropout into ``t['o']``; returns lse fp32 [B, H, Nq]."""
    import torch
    import sae_vision_amd.ops as ops
    lib, st, P = _call_args(t)
    q, k, v, o = t["q"], t["k"], t["v"], t["o"]
    lse = torch.empty((q.shape[0], q.shape[2], q.shape[1]), dtype=torch.float32, device=q.device)
    d = ops._make_desc(q, k, v, o, scale, grid=grid)
    if rope is not None:
        L.check(lib.sae_attn_fwd_rotary(st, ctypes.byref(d), P(q), P(k), P(v), P(rope[0]), P(rope[1]), P(o), P(lse)))
    elif drop is not None:
        L.check(lib.sae_attn_fwd_dropout(st, ctypes.byref(d), P(q), P(k), P(v), P(o), P(lse), drop[0], P(drop[1]),
                                         drop[2]))
    else:
        bh, bw = bias if bias is not None else (None, None)
        L.check(lib.sae_attn_fwd(st, ctypes.byref(d), P(q), P(k), P(v), P(bh), P(bw), P(o), P(lse)))
    return lse


def run_bwd(t, lse, scale, bias=None, grid=None, rope=None, drop=None):
    """sae_attn_bwd / _rotary / _dropout into ``t['dq'], t['dk'], t['dv']``; returns (dbias_h, dbias_w)
    (None without relative logits)."""
    import torch
    import sae_vision_amd.ops as ops
    lib, st, P = _call_args(t)
    q, k, v, o, do, dq, dk, dv = (t[n] for n in TENSORS)
    d = ops._make_desc(q, k, v, o, scale, do, dq, dk, dv, grid=grid)
    ws = torch.empty(lib.sae_attn_bwd_workspace_bytes(ctypes.byref(d)), dtype=torch.uint8, device=q.device)
    dbh = dbw = None
    if rope is not None:
        L.check(lib.sae_attn_bwd_rotary(st, ctypes.byref(d), P(q), P(k), P(v), P(o), P(lse), P(do), P(rope[0]),
                                        P(rope[1]), P(dq), P(dk), P(dv), P(ws)))
    elif drop is not None:
        L.check(lib.sae_attn_bwd_dropout(st, ctypes.byref(d), P(q), P(k), P(v), P(o), P(lse), P(do), P(dq), P(dk),
                                         P(dv), P(ws), drop[0], P(drop[1]), drop[2]))
    else:
        bh, bw = bias if bias is not None else (None, None)
        if bias is not None:
            dbh, dbw = torch.empty_like(bh), torch.empty_like(bw)
        L.check(lib.sae_attn_bwd(st, ctypes.byref(d), P(q), P(k), P(v), P(o), P(lse), P(do), P(bh), P(bw), P(dq),
                                 P(dk), P(dv), P(dbh), P(dbw), P(ws)))
    return dbh, dbw


def run_th_fwd(t, th1, th2, scale, rope=None):
    """sae_th_attn_fwd / _rotary into ``t['o']``; returns lse fp32 [B, H, Nq] (of the mixed logits)."""
    import torch
    import sae_vision_amd.ops as ops
    lib, st, P = _call_args(t)
    q, k, v, o = t["q"], t["k"], t["v"], t["o"]
    lse = torch.empty((q.shape[0], q.shape[2], q.shape[1]), dtype=torch.float32, device=q.device)
    d = ops._make_desc(q, k, v, o, scale)
    if rope is not None:
        L.check(lib.sae_th_attn_fwd_rotary(st, ctypes.byref(d), P(q), P(k), P(v), P(th1), P(th2), P(rope[0]),
                                           P(rope[1]), P(o), P(lse)))
    else:
        L.check(lib.sae_th_attn_fwd(st, ctypes.byref(d), P(q), P(k), P(v), P(th1), P(th2), P(o), P(lse)))
    return lse


def run_th_bwd(t, th1, th2, lse, scale, rope=None):
    """sae_th_attn_bwd / _rotary into ``t['dq'], t['dk'], t['dv']``; returns (dth1, dth2) fp32 [H, H]."""
    import torch
    import sae_vision_amd.ops as ops
    lib, st, P = _call_args(t)
    q, k, v, o, do, dq, dk, dv = (t[n] for n in TENSORS)
    dth1, dth2 = torch.empty_like(th1), torch.empty_like(th2)
    d = ops._make_desc(q, k, v, o, scale, do, dq, dk, dv)
    ws = torch.empty(lib.sae_th_attn_bwd_workspace_bytes(ctypes.byref(d)), dtype=torch.uint8, device=q.device)
    if rope is not None:
        L.check(lib.sae_th_attn_bwd_rotary(st, ctypes.byref(d), P(q), P(k), P(v), P(th1), P(th2), P(lse), P(do),
                                           P(rope[0]), P(rope[1]), P(dq), P(dk), P(dv), P(dth1), P(dth2), P(ws)))
    else:
        L.check(lib.sae_th_attn_bwd(st, ctypes.byref(d), P(q), P(k), P(v), P(th1), P(th2), P(lse), P(do), P(dq),
                                    P(dk), P(dv), P(dth1), P(dth2), P(ws)))
    return dth1, dth2
