"""The split-reduced gradient GEMMs (``sae_gemm_dw``, ``sae_gemm_dw_blocked`` and the split-K path of
``sae_gemm_f32``) checked bit for bit: the split plans restated in Python, exact integer inputs,
guarded arenas, a caller-owned sentinel-filled workspace and direct C-ABI callers, shared by
``test_splits_cpu.py`` (no device) and ``test_gpu_splits.py``.

Plans.  ``dw_plan`` / ``f32_plan`` restate the host rules of csrc/gemm.hip (``dw_plan``, the ``NG``
rule of ``gemm_dw_impl``, ``f32_plan``); ``test_splits_cpu.py`` holds them against the two host-only
workspace queries over a dense sweep.  A plan is invisible from outside except through the workspace:
a call must write exactly ``S`` partial planes (and ``S`` bias rows at ``bpart``) and nothing else, so
a workspace filled with one bit pattern beforehand pins ``S`` and ``NG`` and proves that every
partial element the reduce kernel reads was written by a split.

Exact inputs.  Operands are integers in [-3, 3] (exact in bf16 and fp32), ``dw0`` / ``db0`` / ``c0`` /
``bias`` integers in [-1000, 1000].  Every product, every partial sum in any order and every result
is then an integer below 2**24 in magnitude (``exact_bound`` is that condition, asserted on the CPU
for every case), fp32 accumulation is exact whatever the order, and the expected result is the
integer product: the comparison is ``torch.equal``, without a tolerance.  The product is computed in
float64 on the CPU -- exact for integers below 2**53 -- and converted to int64.

Arenas.  Every operand, output and workspace is a view of a flat buffer filled with the NaN pattern
of ``_layouts.SENTINEL``; the view of a [rows, cols] matrix with leading dimension ``ld`` owns the
tightest legal allocation, ``(rows - 1) * ld + cols`` elements, between two guards.  A read of a pad
column or past the last row pulls a NaN into the result; a write outside the view shows in the
guards or in the pad columns (``_layouts.assert_guards_intact``).
"""
import collections
import ctypes
import functools

import numpy as np

from _layouts import EPC, GUARD_ALIGN, SENTINEL, assert_guards_intact, make_arena
from sae_vision_amd import _lib as L

DW_T, DW_K, DW8_K, DW8_RING = 128, 64, 32, 4     # csrc/gemm_dw.h kDwT, kDwK; gemm_dw8.h kDw8K, kDw8NS
F32_T, F32_K = 128, 16                            # csrc/gemm_f32.h kF32T, kF32K
DW_RED_COLS, DW_RED_GROUPS, DW_RED_BLOCKS = 64, 4, 4096   # gemm_dw_reduce_kernel / dw_reduce
EXACT = 1 << 24                                   # integers below it are exact in fp32
OPERAND_LIM, ADDEND_LIM = 3, 1000
WS_SENTINEL = SENTINEL["f32"]                     # 0x7FA5A5A5, as int32
WS_GUARD = 1024                                   # floats on each side of a workspace


def cdiv(a, b):
    return -(-a // b)


def round256(n):
    return (n + 255) & ~255


# ------------------------------------------------------------------------------------- plans
def dw_tiles(I, J):
    return cdiv(I, DW_T) * cdiv(J, DW_T)


def dw_split(M, I, J, slots):
    """(S, chunk) of csrc/gemm.hip ``dw_plan`` with ``slots`` workgroups."""
    s = max(1, min(slots // dw_tiles(I, J), cdiv(M, 256)))
    chunk = cdiv(cdiv(M, s), DW_K) * DW_K
    return cdiv(M, chunk), chunk


DwPlan = collections.namedtuple("DwPlan", [
    "tiles", "NG", "S", "chunk",
    "last_rows",            # token rows of the last split
    "stages",               # 32-token stages of a full split (the first one)
    "group_stages",         # ... per wave group: every group runs ceil(stages / NG)
    "last_stages",          # 32-token stages of the last split
    "last_group_stages",
    "S512",                 # splits of the 512-slot plan, which sizes the workspace
    "plane_offsets",        # byte offset of every partial plane the call writes
    "bpart_offset",         # byte offset of the [S][J] bias partials
    "ws_bytes",             # sae_gemm_dw_workspace_bytes
    "reduce_groups",        # splits each of the four reduce groups sums
    "reduce_strides",       # whether the reduce kernel's grid-stride loop takes a second trip
])


def dw_plan(M, I, J):
    """What ``sae_gemm_dw(M, I, J)`` launches: two wave groups (256 slots) up to 64 output tiles, one
    (512 slots) above; the workspace query always plans with 512."""
    tiles = dw_tiles(I, J)
    NG = 2 if tiles <= 64 else 1
    S, chunk = dw_split(M, I, J, 512 // NG)
    S512, _ = dw_split(M, I, J, 512)
    last_rows = M - (S - 1) * chunk
    stages, last_stages = cdiv(min(chunk, M), DW8_K), cdiv(last_rows, DW8_K)
    per = cdiv(S, DW_RED_GROUPS)
    return DwPlan(
        tiles=tiles, NG=NG, S=S, chunk=chunk, last_rows=last_rows,
        stages=stages, group_stages=cdiv(stages, NG),
        last_stages=last_stages, last_group_stages=cdiv(last_stages, NG),
        S512=S512,
        plane_offsets=tuple(s * I * J * 4 for s in range(S)),
        bpart_offset=round256(S * I * J * 4),
        ws_bytes=round256(S512 * I * J * 4) + round256(S512 * J * 4),
        reduce_groups=tuple(max(0, min(S, (g + 1) * per) - g * per) for g in range(DW_RED_GROUPS)),
        reduce_strides=cdiv(I * J // 4, DW_RED_COLS) > DW_RED_BLOCKS)


F32Plan = collections.namedtuple("F32Plan", ["tiles", "S", "kchunk", "ws_bytes"])


def f32_plan(M, N, K):
    """csrc/gemm.hip ``f32_plan`` and ``sae_gemm_f32_workspace_bytes``."""
    tiles = cdiv(M, F32_T) * cdiv(N, F32_T)
    s = 1
    if tiles < 256 and K >= 2048:
        s = min(cdiv(512, tiles), K // 1024)
    s = max(1, min(s, 64))
    kchunk = cdiv(cdiv(K, s), F32_K) * F32_K
    S = cdiv(K, kchunk)
    return F32Plan(tiles, S, kchunk, S * (M + 1) * N * 4 if S > 1 else 0)


# ------------------------------------------------------------------------------- case tables
# sae_gemm_dw: (M, I, J) -> the plan properties the row is there for (fields of DwPlan)
DW_ROWS = [
    ((1, 8, 8), dict(NG=2, S=1, stages=1, group_stages=1)),            # group 1 reads only zeros
    ((31, 8, 8), dict(NG=2, S=1, stages=1, last_rows=31)),             # ragged single stage
    ((33, 136, 128), dict(NG=2, S=1, stages=2, group_stages=1, tiles=2)),   # ragged I tile
    ((65, 128, 136), dict(NG=2, S=1, stages=3, group_stages=2)),       # group 1's 2nd stage past the end
    ((97, 24, 40), dict(NG=2, S=1, stages=4, group_stages=2, tiles=1)),
    ((225, 256, 8), dict(NG=2, S=1, stages=8, group_stages=4)),        # ring wraps: 4 > 3 prefetched
    ((257, 8, 264), dict(NG=2, S=2, chunk=192, last_rows=65, last_stages=3)),
    ((1280, 8, 8), dict(NG=2, S=5, reduce_groups=(2, 2, 1, 0))),
    ((3328, 8, 16), dict(NG=2, S=13, reduce_groups=(4, 4, 4, 1))),
    ((65536, 8, 8), dict(NG=2, S=256, chunk=256)),                     # the most a plan gives
    ((2048, 1024, 1024), dict(NG=2, tiles=64, S=4, S512=8)),           # 4 used, 8 provisioned
    ((1, 520, 1544), dict(NG=1, tiles=65, S=1, stages=1)),
    ((97, 520, 1544), dict(NG=1, tiles=65, S=1, stages=4, group_stages=4)),   # ring wraps
    ((300, 1544, 520), dict(NG=1, tiles=65, S=2, chunk=192, last_rows=108)),
    ((700, 1160, 1160), dict(NG=1, tiles=100, S=3, reduce_strides=True)),
]
DW_BLOCKED = [((257, 8, 264), 4), ((257, 8, 264), 88), ((257, 8, 264), 264),
              ((300, 1544, 520), 8), ((300, 1544, 520), 260)]    # the last two straddle 128-column tiles
DW_GAUSS = (300, 1544, 520)

# sae_gemm_f32 operand layouts as (A k-contiguous, B k-contiguous): the kernel's <AK, BK>
FORWARD, INPUT_GRAD, WEIGHT_GRAD, FOURTH = (True, False), (True, True), (False, False), (False, True)
F32_LAYOUTS = {"fwd": FORWARD, "dgrad": INPUT_GRAD, "wgrad": WEIGHT_GRAD, "fourth": FOURTH}
# ((M, N, K), layout name) -> plan properties (fields of F32Plan)
F32_ROWS = (
    [(((8, 8, 2048), lay), dict(S=2, kchunk=1024)) for lay in F32_LAYOUTS] +
    [(((132, 136, 2052), lay), dict(S=2, kchunk=1040, tiles=4)) for lay in F32_LAYOUTS] +
    [(((128, 128, 3072), "fwd"), dict(S=3, tiles=1)),       # the ones row of colsum in a second tile row
     (((8, 12, 2047), "wgrad"), dict(S=1, ws_bytes=0)),     # below the threshold: no workspace, NULL
     (((12, 8, 70000), "wgrad"), dict(S=64, kchunk=1104)),  # the cap, a ragged last split
     (((4, 4, 65536), "wgrad"), dict(S=64, kchunk=1024)),
     (((1920, 2048, 2048), "fwd"), dict(S=2, tiles=240))])  # the other side of tiles < 256
F32_GAUSS = ((132, 136, 2052), "wgrad")


def dw_id(shape):
    return "m%d_i%d_j%d" % shape


def f32_id(key):
    return "m%d_n%d_k%d_%s" % (key[0] + (key[1],))


# ------------------------------------------------------------------------------ exact inputs
def _ints(rng, shape, lim):
    return rng.integers(-lim, lim + 1, size=shape).astype(np.float64)


def _as_int(x):
    r = np.rint(x).astype(np.int64)
    assert np.array_equal(r, x)
    return r


DwInputs = collections.namedtuple("DwInputs", ["x", "dy", "dw0", "db0", "prod", "colsum"])
F32Inputs = collections.namedtuple("F32Inputs", ["a", "b", "c0", "bias", "colsum0", "prod", "colsum"])


@functools.lru_cache(maxsize=2)
def dw_inputs(M, I, J):
    """x [M, I], dy [M, J] (float64 arrays of small integers), dw0 [I, J], db0 [J] and the int64
    references x^T dy and colsum(dy); cached, so the variants of a row share one reference."""
    rng = np.random.default_rng([M, I, J])
    x, dy = _ints(rng, (M, I), OPERAND_LIM), _ints(rng, (M, J), OPERAND_LIM)
    dw0, db0 = _ints(rng, (I, J), ADDEND_LIM), _ints(rng, (J,), ADDEND_LIM)
    return DwInputs(x, dy, _as_int(dw0), _as_int(db0), _as_int(x.T @ dy), _as_int(dy.sum(0)))


@functools.lru_cache(maxsize=2)
def f32_inputs(M, N, K):
    """a [M, K], b [K, N] (logical; the layout only decides how they are stored), c0 [M, N], bias [N],
    colsum0 [N] and the int64 references a b and colsum(b)."""
    rng = np.random.default_rng([M, N, K, 1])
    a, b = _ints(rng, (M, K), OPERAND_LIM), _ints(rng, (K, N), OPERAND_LIM)
    c0, bias, cs0 = _ints(rng, (M, N), ADDEND_LIM), _ints(rng, (N,), ADDEND_LIM), _ints(rng, (N,), ADDEND_LIM)
    return F32Inputs(a, b, _as_int(c0), _as_int(bias), _as_int(cs0), _as_int(a @ b), _as_int(b.sum(0)))


def exact_bound(depth):
    """The largest magnitude any partial sum of a ``depth``-deep product can reach, in any order of
    summation, with both addends (dw0 and a bias) included: it must stay below 2**24."""
    return OPERAND_LIM * OPERAND_LIM * depth + 2 * ADDEND_LIM


def dw_expected(inp, with_db, accumulate):
    dw = inp.prod + (inp.dw0 if accumulate else 0)
    db = (inp.colsum + (inp.db0 if accumulate else 0)) if with_db else None
    return dw, db


def f32_expected(inp, with_bias, with_colsum, accumulate):
    c = inp.prod + (inp.bias[None, :] if with_bias else 0) + (inp.c0 if accumulate else 0)
    cs = (inp.colsum + (inp.colsum0 if accumulate else 0)) if with_colsum else None
    return c, cs


# ------------------------------------------------------------------------------------ arenas
def arena_layout(rows, cols, ld, lead=0):
    """(numel, offset, guard) of the arena of a [rows, cols] view with row stride ``ld`` that starts
    ``lead`` elements past the leading guard: ``(rows - 1) * ld + cols`` elements, the tightest legal
    allocation, then the trailing guard.  The guards hold an overrun of a whole ragged 128-row tile."""
    assert rows >= 1 and 1 <= cols <= ld and lead >= 0
    extent = (rows - 1) * ld + cols
    guard = cdiv(max(256, min(extent, (DW_T + 1) * ld)), GUARD_ALIGN) * GUARD_ALIGN
    return guard + lead + extent + guard, guard + lead, guard


Placed = collections.namedtuple("Placed", ["arena", "view"])


def place(values, rows, cols, ld, dtype, device, lead=0):
    """A sentinel-filled arena and the [rows, cols] view of ``arena_layout`` in it; ``values`` (or
    None: the view keeps the NaN pattern, as an output that must be overwritten) go through the view."""
    import torch
    numel, offset, _ = arena_layout(rows, cols, ld, lead)
    arena = make_arena(numel, dtype, device)
    view = torch.as_strided(arena, (rows, cols), (ld, 1), offset)
    if values is not None:
        view.copy_(torch.as_tensor(np.asarray(values, np.float32)).to(device=device, dtype=arena.dtype))
    return Placed(arena, view)


def place_vec(values, n, device):
    p = place(None if values is None else np.asarray(values)[None, :], 1, n, n, "f32", device)
    return Placed(p.arena, p.view[0])


def make_workspace(nbytes, device, junk_seed=None):
    """A caller-owned workspace of exactly ``nbytes`` between two guards, every int32 of it the
    sentinel -- or, with ``junk_seed``, seeded random bits.  Returns Placed(arena, fp32 view), or
    Placed(None, None) for ``nbytes == 0`` (the call takes NULL)."""
    import torch
    if nbytes == 0:
        return Placed(None, None)
    assert nbytes % 4 == 0
    n = nbytes // 4
    arena = make_arena(WS_GUARD + n + WS_GUARD, "f32", device)
    ws = arena[WS_GUARD:WS_GUARD + n]
    if junk_seed is not None:
        g = torch.Generator(device=device).manual_seed(junk_seed)
        ws.view(torch.int32).copy_(torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), dtype=torch.int32, device=device,
                                                 generator=g))
    return Placed(arena, ws)


def assert_workspace(ws, written):
    """Of the workspace ``ws`` (``make_workspace`` without junk), exactly the float ranges ``written``
    ((offset, count) pairs, in floats) hold no sentinel; every other element and both guards still do."""
    import torch
    if ws.arena is None:
        assert not written
        return
    assert_guards_intact(ws.arena, ws.view)
    is_sent = ws.view.view(torch.int32) == WS_SENTINEL
    inside = torch.zeros_like(is_sent)
    for off, cnt in written:
        assert 0 <= off and off + cnt <= inside.numel(), (off, cnt, inside.numel())
        inside[off:off + cnt] = True
    unwritten = int((is_sent & inside).sum())
    stray = torch.nonzero(~is_sent & ~inside).flatten()
    assert unwritten == 0, f"{unwritten} partial element(s) the reduce reads were written by no split"
    assert stray.numel() == 0, (f"{stray.numel()} workspace element(s) written outside the plan's partials, "
                                f"the first at float {int(stray[0])}")


def dw_written(plan, I, J, with_db):
    w = [(0, plan.S * I * J)]
    if with_db:
        w.append((plan.bpart_offset // 4, plan.S * J))
    return w


def f32_written(plan, M, N, with_colsum):
    return [(0, plan.S * (M + (1 if with_colsum else 0)) * N)] if plan.S > 1 else []


# ------------------------------------------------------------------------- direct C-ABI callers
def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(t):
    import torch
    return torch.cuda.current_stream(t.device).cuda_stream


def call_dw(x, dy, dw, db, accumulate, ws, jblock=0):
    """sae_gemm_dw (``jblock`` > 0: sae_gemm_dw_blocked, dw the contiguous [J / jblock, I, jblock])
    on the views' own strides with the caller's workspace."""
    lib = L.load()
    (M, I), J = x.shape, dy.shape[1]
    if jblock:
        rc = lib.sae_gemm_dw_blocked(_stream(x), M, I, J, jblock, _p(x), x.stride(0), _p(dy), dy.stride(0), _p(dw),
                                     _p(db), int(accumulate), _p(ws))
    else:
        rc = lib.sae_gemm_dw(_stream(x), M, I, J, _p(x), x.stride(0), _p(dy), dy.stride(0), _p(dw), dw.stride(0),
                             _p(db), int(accumulate), _p(ws))
    L.check(rc)


def place_f32_operands(inp, layout, device, pad=4):
    """a and b stored as the layout wants them, leading dimensions padded by ``pad``: returns
    (a Placed, (sam, sak), b Placed, (sbk, sbn))."""
    ak, bk = layout
    M, K = inp.a.shape
    N = inp.b.shape[1]
    if ak:
        a, sa = place(inp.a, M, K, K + pad, "f32", device), (K + pad, 1)
    else:
        a, sa = place(inp.a.T, K, M, M + pad, "f32", device), (1, M + pad)
    if bk:
        b, sb = place(inp.b.T, N, K, K + pad, "f32", device), (1, K + pad)
    else:
        b, sb = place(inp.b, K, N, N + pad, "f32", device), (N + pad, 1)
    return a, sa, b, sb


def call_f32(shape, a, sa, b, sb, bias, c, colsum, accumulate, ws):
    """sae_gemm_f32 with explicit operand strides (sa = (sam, sak), sb = (sbk, sbn)), c a [M, N] view
    with unit column stride, and the caller's workspace (None: NULL)."""
    M, N, K = shape
    L.check(L.load().sae_gemm_f32(_stream(c), M, N, K, _p(a), sa[0], sa[1], _p(b), sb[0], sb[1], _p(bias), _p(c),
                                  c.stride(0), _p(colsum), int(accumulate), _p(ws)))


# ----------------------------------------------------------------------------- the four checks
# One exact case end to end, shared by test_gpu_splits.py (``call`` = the C ABI) and the self-tests of
# test_splits_cpu.py (``call`` = a plain-torch emulation of the split kernels, right or broken on
# purpose, which shows that each assertion below catches what it is there for).
NONE = Placed(None, None)
_OPERANDS = {}      # the read-only operands of the row in hand, placed once for all of its variants


def _operands(key, make):
    if key not in _OPERANDS:
        _OPERANDS.clear()
        _OPERANDS[key] = make()
    return _OPERANDS[key]


def forget_operands():
    _OPERANDS.clear()


def _sync(device):
    import torch
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def _dev_f32(ref, device):
    import torch
    return torch.as_tensor(ref).to(device=device, dtype=torch.float32)      # int64 below 2**24: exact


def _same_bits(a, b):
    import torch
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _guards(*placed):
    for p in placed:
        if p.arena is not None:
            assert_guards_intact(p.arena, p.view)


def dw_strides(shape, padded):
    """(ldx, ldy, ldw, lead of the bf16 views, lead of the fp32 views): the padded form starts every
    view 48 bytes into a wider arena."""
    M, I, J = shape
    return (I + 8, J + 24, J + 4, 3 * EPC["bf16"], 3 * EPC["f32"]) if padded else (I, J, J, 0, 0)


def blocked(dw, jb):
    """[I, J] -> the rows of the contiguous [J / jb, I, jb] that sae_gemm_dw_blocked writes."""
    I, J = dw.shape
    return dw.reshape(I, J // jb, jb).transpose(1, 0, 2).reshape(-1, jb)


def run_dw(device, shape, inp, with_db, acc, padded, jblock=0, junk=None, call=call_dw):
    M, I, J = shape
    ldx, ldy, ldw, lead16, lead32 = dw_strides(shape, padded)
    x, dy = _operands(("dw", shape, padded, str(device)),
                      lambda: (place(inp.x, M, I, ldx, "bf16", device, lead16),
                               place(inp.dy, M, J, ldy, "bf16", device, lead16)))
    if jblock:
        dw = place(blocked(inp.dw0, jblock) if acc else None, J // jblock * I, jblock, jblock, "f32", device, lead32)
    else:
        dw = place(inp.dw0 if acc else None, I, J, ldw, "f32", device, lead32)
    db = place_vec(inp.db0 if acc else None, J, device) if with_db else NONE
    nbytes = L.load().sae_gemm_dw_workspace_bytes(M, I, J)
    assert nbytes == dw_plan(M, I, J).ws_bytes
    ws = make_workspace(nbytes, device, junk)
    call(x.view, dy.view, dw.view, db.view, acc, ws.view, jblock)
    _sync(device)
    return x, dy, dw, db, ws


def check_dw(device, shape, with_db, acc, padded, jblock=0, claims=None, call=call_dw):
    import torch
    M, I, J = shape
    plan = dw_plan(M, I, J)
    for field, want in (claims or {}).items():
        assert getattr(plan, field) == want, (field, getattr(plan, field), want)
    inp = dw_inputs(M, I, J)
    want_dw, want_db = dw_expected(inp, with_db, acc)
    x, dy, dw, db, ws = run_dw(device, shape, inp, with_db, acc, padded, jblock, call=call)
    # 1. exact (a NaN pulled in from a pad column or a guard fails it too)
    if jblock:
        for k in range(J // jblock):
            assert torch.equal(dw.view[k * I:(k + 1) * I], _dev_f32(want_dw[:, k * jblock:(k + 1) * jblock], device)), \
                f"dw differs from the integer reference in column block {k}"
    else:
        assert torch.equal(dw.view, _dev_f32(want_dw, device)), "dw differs from the integer reference"
    if with_db:
        assert torch.equal(db.view, _dev_f32(want_db, device)), "db differs from the integer reference"
    # 2. pad columns and guards
    _guards(dw, db, x, dy)
    # 3. exactly the plan's partials were written
    assert_workspace(ws, dw_written(plan, I, J, with_db))
    # 4. nothing depends on what the workspace held
    _, _, dw2, db2, _ = run_dw(device, shape, inp, with_db, acc, padded, jblock, junk=M + I + J + 1, call=call)
    assert _same_bits(dw.view, dw2.view), "dw depends on what the workspace held before the call"
    assert not with_db or _same_bits(db.view, db2.view), "db depends on what the workspace held before the call"


def run_f32(device, key, inp, with_bias, with_colsum, acc, ldc_pad, junk=None, call=call_f32):
    (M, N, K), lay = key
    a, sa, b, sb = _operands(("f32", key, str(device)), lambda: place_f32_operands(inp, F32_LAYOUTS[lay], device))
    c = place(inp.c0 if acc else None, M, N, N + ldc_pad, "f32", device)
    bias = place_vec(inp.bias, N, device) if with_bias else NONE
    cs = place_vec(inp.colsum0 if acc else None, N, device) if with_colsum else NONE
    nbytes = L.load().sae_gemm_f32_workspace_bytes(M, N, K)
    assert nbytes == f32_plan(M, N, K).ws_bytes
    ws = make_workspace(nbytes, device, junk)
    call((M, N, K), a.view, sa, b.view, sb, bias.view, c.view, cs.view, acc, ws.view)
    _sync(device)
    return a, b, bias, c, cs, ws


def check_f32(device, key, with_bias, with_colsum, acc, ldc_pad, claims=None, call=call_f32):
    import torch
    (M, N, K), _ = key
    plan = f32_plan(M, N, K)
    for field, want in (claims or {}).items():
        assert getattr(plan, field) == want, (field, getattr(plan, field), want)
    inp = f32_inputs(M, N, K)
    want_c, want_cs = f32_expected(inp, with_bias, with_colsum, acc)
    a, b, bias, c, cs, ws = run_f32(device, key, inp, with_bias, with_colsum, acc, ldc_pad, call=call)
    assert (ws.view is None) == (plan.S == 1)
    assert torch.equal(c.view, _dev_f32(want_c, device)), "c differs from the integer reference"
    if with_colsum:
        assert torch.equal(cs.view, _dev_f32(want_cs, device)), "colsum differs from the integer reference"
    _guards(c, cs, bias, a, b)
    assert_workspace(ws, f32_written(plan, M, N, with_colsum))
    _, _, _, c2, cs2, _ = run_f32(device, key, inp, with_bias, with_colsum, acc, ldc_pad, junk=M + N + K + 1, call=call)
    assert _same_bits(c.view, c2.view), "c depends on what the workspace held before the call"
    assert not with_colsum or _same_bits(cs.view, cs2.view), "colsum depends on what the workspace held"
