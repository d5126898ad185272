"""The split plans of the gradient GEMMs, their CPU half: the Python restatement of ``dw_plan``, the
``NG`` rule and ``f32_plan`` (``_splits.py``) against the two host-only workspace queries over a dense
sweep; the plan properties every row of the GPU tables (``test_gpu_splits.py``) is there for; the
2**24 condition of the exact-integer method; the arena helper; and the host-side refusals of
``sae_gemm_dw``, ``sae_gemm_dw_blocked`` and ``sae_gemm_f32``, which return before any HIP call (no
call here passes validation, so none needs a device)."""
import ctypes

import numpy as np
import pytest
import torch

import _splits as S
from _layouts import SENTINEL, assert_guards_intact
from sae_vision_amd import _lib as L

DW_M = (list(range(1, 70)) + [95, 96, 97, 127, 128, 129, 191, 192, 193, 224, 225, 255, 256, 257, 258, 300, 511, 512,
                              513, 700, 767, 768, 769, 1279, 1280, 1281, 2048, 3000, 3328, 4616, 18464, 25216, 65535,
                              65536, 65537, 131072])
DW_IJ = [8, 16, 24, 40, 120, 128, 136, 256, 264, 384, 520, 768, 1000, 1024, 1032, 1152, 1160, 1536, 1544, 2304, 3072]
F32_MN = [1, 4, 5, 8, 12, 127, 128, 129, 132, 136, 384, 1152, 1920, 1921, 2047, 2048, 2049, 3072]
F32_K = [1, 4, 16, 1023, 1024, 2047, 2048, 2049, 2052, 2063, 2064, 2065, 3071, 3072, 3073, 4096, 25216, 65535, 65536,
         65537, 70000, 131072]


@pytest.fixture(scope="module")
def lib():
    return L.load()


# ------------------------------------------------------------------- plans against the queries
def test_dw_plan_matches_workspace_query(lib):
    """sae_gemm_dw_workspace_bytes = round256(S512 I J 4) + round256(S512 J 4); the 256-slot plan never
    gives more splits than the 512-slot one (``dw_plan``'s comment claims it; the bpart offset and the
    workspace bound of the two-group kernel rely on it)."""
    shapes = [(M, I, J) for M in DW_M for I in DW_IJ for J in DW_IJ] + [r[0] for r in S.DW_ROWS]
    for M, I, J in shapes:
        p = S.dw_plan(M, I, J)
        assert lib.sae_gemm_dw_workspace_bytes(M, I, J) == p.ws_bytes, (M, I, J)
        assert p.ws_bytes == S.round256(p.S512 * I * J * 4) + S.round256(p.S512 * J * 4)
        s256, _ = S.dw_split(M, I, J, 256)
        s512, _ = S.dw_split(M, I, J, 512)
        assert 1 <= s256 <= s512 == p.S512, (M, I, J)
        assert p.S == (s256 if p.NG == 2 else s512) and p.S <= p.S512
        # what the launch relies on: chunks of whole 64-token stages that cover M with no empty split
        assert p.chunk % S.DW_K == 0 and (p.S - 1) * p.chunk < M <= p.S * p.chunk
        assert 1 <= p.last_rows <= p.chunk and sum(p.reduce_groups) == p.S
        # the partials the call writes lie inside the queried workspace
        assert p.plane_offsets[-1] + I * J * 4 <= p.bpart_offset
        assert p.bpart_offset + p.S * J * 4 <= p.ws_bytes
    assert lib.sae_gemm_dw_workspace_bytes(0, 8, 8) == 0


def test_f32_plan_matches_workspace_query(lib):
    """sae_gemm_f32_workspace_bytes = S (M + 1) N 4 when the shape splits, else 0."""
    shapes = [(M, N, K) for M in F32_MN for N in F32_MN for K in F32_K] + [r[0][0] for r in S.F32_ROWS]
    for M, N, K in shapes:
        p = S.f32_plan(M, N, K)
        assert lib.sae_gemm_f32_workspace_bytes(M, N, K) == p.ws_bytes, (M, N, K)
        assert p.ws_bytes == (p.S * (M + 1) * N * 4 if p.S > 1 else 0)
        assert 1 <= p.S <= 64 and p.kchunk % S.F32_K == 0 and (p.S - 1) * p.kchunk < K <= p.S * p.kchunk
        assert p.S == 1 or (p.tiles < 256 and K >= 2048)
    assert lib.sae_gemm_f32_workspace_bytes(8, 8, 0) == 0


# -------------------------------------------------------------------------- the GPU case tables
@pytest.mark.parametrize("shape,claims", S.DW_ROWS, ids=[S.dw_id(r[0]) for r in S.DW_ROWS])
def test_dw_row_reaches_what_it_claims(shape, claims):
    p = S.dw_plan(*shape)
    for field, want in claims.items():
        assert getattr(p, field) == want, (shape, field, getattr(p, field), want)


def test_dw_rows_cover_the_plan_edges():
    """Together the rows reach: fewer than three stages to prefetch, an odd stage count under two
    groups, a ring that wraps under both NG, a ragged last stage, a short last split under both NG,
    empty reduce groups, the largest S and a provisioned-but-unused half of the workspace."""
    plans = [S.dw_plan(*r[0]) for r in S.DW_ROWS]
    shapes = [r[0] for r in S.DW_ROWS]
    assert any(p.group_stages < S.DW8_RING - 1 for p in plans)
    assert any(p.NG == 2 and p.last_stages % 2 == 1 and p.last_stages > 1 for p in plans)
    for ng in (1, 2):
        assert any(p.NG == ng and p.group_stages > S.DW8_RING - 1 for p in plans)
        assert any(p.NG == ng and p.S > 1 and p.last_rows < p.chunk for p in plans)
        assert any(p.NG == ng and p.S == 1 and p.stages == 1 for p in plans)
    assert any(M % S.DW8_K for M, _, _ in shapes)
    assert {1, 2, 3, 5} <= {p.S for p in plans} and max(p.S for p in plans) == 256
    assert any(0 in p.reduce_groups for p in plans) and any(p.S < p.S512 for p in plans)
    assert any(p.reduce_strides for p in plans)
    for (shape, jb) in S.DW_BLOCKED:
        assert shape in shapes and shape[2] % jb == 0 and jb % 4 == 0
    assert any(S.DW_T % jb and jb % S.DW_T for _, jb in S.DW_BLOCKED)    # blocks that straddle tiles


@pytest.mark.parametrize("key,claims", S.F32_ROWS, ids=[S.f32_id(r[0]) for r in S.F32_ROWS])
def test_f32_row_reaches_what_it_claims(key, claims):
    (M, N, K), lay = key
    p = S.f32_plan(M, N, K)
    for field, want in claims.items():
        assert getattr(p, field) == want, (key, field, getattr(p, field), want)
    ak, bk = S.F32_LAYOUTS[lay]
    # what the entry point asks of the layout (its k-contiguous operands need K % 4 == 0, ...)
    assert (K % 4 == 0) if (ak or bk) else True
    assert ak or M % 4 == 0
    assert bk or N % 4 == 0


def test_f32_rows_cover_the_plan_edges():
    keys = [r[0] for r in S.F32_ROWS]
    for shape in ((8, 8, 2048), (132, 136, 2052)):
        assert {lay for s, lay in keys if s == shape} == set(S.F32_LAYOUTS)
    plans = {k: S.f32_plan(*k[0]) for k in keys}
    assert {1, 2, 3, 64} <= {p.S for p in plans.values()}
    assert S.f32_plan(8, 12, 2047).S == 1 and S.f32_plan(8, 12, 2048).S == 2      # the K threshold
    assert S.f32_plan(1920, 2048, 2048).tiles == 240 and S.f32_plan(2048, 2048, 2048).S == 1   # tiles < 256
    assert any(K % p.kchunk for ((_, _, K), _), p in plans.items() if p.S > 1)    # a ragged last split
    assert any(K % S.F32_K for ((_, _, K), _) in keys)                            # a ragged last k tile


# ------------------------------------------------------------------------ the 2**24 condition
@pytest.mark.parametrize("shape", [r[0] for r in S.DW_ROWS], ids=S.dw_id)
def test_dw_case_is_exact_in_fp32(shape):
    """Every partial sum in any order is bounded by 9 M + 2000, and the reference itself (dw0 and db0
    included) stays below 2**24: fp32 accumulation of the case is exact."""
    M, I, J = shape
    assert S.exact_bound(M) < S.EXACT
    inp = S.dw_inputs(M, I, J)
    for arr in (inp.x, inp.dy):
        assert np.abs(arr).max() <= S.OPERAND_LIM and np.array_equal(arr, np.rint(arr))
    dw, db = S.dw_expected(inp, True, True)
    assert dw.dtype == np.int64 and db.dtype == np.int64
    assert max(np.abs(dw).max(), np.abs(db).max(), np.abs(inp.prod).max(), np.abs(inp.colsum).max()) < S.EXACT
    assert np.array_equal(dw.astype(np.float32).astype(np.int64), dw)
    if M * I * J <= 1 << 22:      # the float64 product against numpy's own integer product
        assert np.array_equal(inp.prod, inp.x.astype(np.int64).T @ inp.dy.astype(np.int64))


@pytest.mark.parametrize("shape", sorted({r[0][0] for r in S.F32_ROWS}), ids=lambda s: "m%d_n%d_k%d" % s)
def test_f32_case_is_exact_in_fp32(shape):
    M, N, K = shape
    assert S.exact_bound(K) < S.EXACT
    inp = S.f32_inputs(M, N, K)
    c, cs = S.f32_expected(inp, True, True, True)
    assert c.dtype == np.int64 and cs.dtype == np.int64
    assert max(np.abs(c).max(), np.abs(cs).max(), np.abs(inp.prod).max(), np.abs(inp.colsum).max()) < S.EXACT
    assert np.array_equal(c.astype(np.float32).astype(np.int64), c)
    if M * N * K <= 1 << 22:
        assert np.array_equal(inp.prod, inp.a.astype(np.int64) @ inp.b.astype(np.int64))


# ------------------------------------------------------------------------------ the arena helper
def _arena_cases():
    out = []
    for (M, I, J), _ in S.DW_ROWS:
        for pad, lead in ((0, 0), (1, 24)):
            out += [(M, I, I + 8 * pad, "bf16", lead), (M, J, J + 24 * pad, "bf16", lead),
                    (I, J, J + 4 * pad, "f32", lead // 2), (1, J, J, "f32", 0)]
    for ((M, N, K), _), _ in S.F32_ROWS:
        out += [(M, K, K + 4, "f32", 0), (K, M, M + 4, "f32", 0), (K, N, N + 4, "f32", 0), (N, K, K + 4, "f32", 0),
                (M, N, N, "f32", 0), (M, N, N + 4, "f32", 0)]
    return sorted(set(out))


def test_arena_layout_is_tight_and_guarded():
    """The view owns exactly (rows - 1) ld + cols elements between its guards, starts 16-byte aligned
    and is followed by nothing but the trailing guard."""
    for rows, cols, ld, dtype, lead in _arena_cases():
        numel, offset, guard = S.arena_layout(rows, cols, ld, lead)
        extent = (rows - 1) * ld + cols
        assert guard >= 256 and guard % 64 == 0 and offset == guard + lead
        assert offset % S.EPC[dtype] == 0
        assert numel == offset + extent + guard
        last = offset + (rows - 1) * ld + cols - 1
        assert guard <= offset and last == numel - guard - 1


@pytest.mark.parametrize("rows,cols,ld,dtype,lead", [(1, 8, 8, "f32", 0), (5, 8, 12, "f32", 4), (33, 136, 144, "bf16", 24),
                                                     (3, 8, 8, "bf16", 0)])
def test_place_puts_a_unit_stride_view_inside_the_guards(rows, cols, ld, dtype, lead):
    vals = np.arange(rows * cols).reshape(rows, cols) % 7 - 3
    p = S.place(vals, rows, cols, ld, dtype, "cpu", lead)
    numel, offset, guard = S.arena_layout(rows, cols, ld, lead)
    assert p.arena.numel() == numel and p.view.storage_offset() == offset and p.view.stride() == (ld, 1)
    assert np.array_equal(p.view.float().numpy(), vals)
    assert_guards_intact(p.arena, p.view)                 # pad columns and guards: still the NaN pattern
    ti = torch.int16 if dtype == "bf16" else torch.int32
    bits = p.arena.view(ti)
    assert (bits[:offset] == SENTINEL[dtype]).all() and (bits[numel - guard:] == SENTINEL[dtype]).all()
    if ld > cols and rows > 1:
        assert torch.isnan(p.arena[offset + cols].float())                 # a pad column reads NaN
        p.arena[offset + cols] = 0                                         # ... and a write there shows
        with pytest.raises(AssertionError, match="written outside"):
            assert_guards_intact(p.arena, p.view)
    empty = S.place(None, rows, cols, ld, dtype, "cpu", lead)
    assert torch.isnan(empty.view.float()).all()


def test_workspace_check_sees_holes_and_strays():
    ws = S.make_workspace(1024, "cpu")
    assert ws.view.numel() == 256 and (ws.arena.view(torch.int32) == S.WS_SENTINEL).all()
    assert ws.view.data_ptr() % 16 == 0
    ws.view[:100] = 1.0
    S.assert_workspace(ws, [(0, 100)])
    with pytest.raises(AssertionError, match="written by no split"):
        S.assert_workspace(ws, [(0, 101)])
    with pytest.raises(AssertionError, match="outside the plan"):
        S.assert_workspace(ws, [(0, 99)])
    ws.arena[S.WS_GUARD + 256] = 0.0
    with pytest.raises(AssertionError, match="written outside"):
        S.assert_workspace(ws, [(0, 100)])
    assert S.make_workspace(0, "cpu") == (None, None)


# ------------------------------------------------------------------------- host-side refusals
X, DY, DW, DB, WS = (ctypes.c_void_p(0x10000 * (i + 1)) for i in range(5))    # never dereferenced


def _refused(lib, rc, code, text):
    assert rc == code, (rc, lib.sae_last_error().decode())
    assert text in lib.sae_last_error().decode(), lib.sae_last_error().decode()


@pytest.mark.parametrize("kw,code,text", [
    (dict(ldw=32), L.SAE_EINVAL, "bad leading dimensions"),                  # ldw < J
    (dict(ldw=42), L.SAE_EINVAL, "bad leading dimensions"),                  # ldw % 4
    (dict(I=12, ldx=16), L.SAE_EUNSUPPORTED, "must be multiples of 8"),      # I % 8
    (dict(dw=ctypes.c_void_p(0x30004)), L.SAE_EINVAL, "16-byte aligned"),    # misaligned dw
    (dict(ws=None), L.SAE_EINVAL, "must be non-NULL"),
], ids=["ldw_lt_J", "ldw_mod_4", "I_mod_8", "dw_misaligned", "ws_null"])
def test_gemm_dw_refuses_on_the_host(lib, kw, code, text):
    a = dict(M=300, I=16, J=40, ldx=16, ldy=40, ldw=40, dw=DW, ws=WS)
    a.update(kw)
    rc = lib.sae_gemm_dw(None, a["M"], a["I"], a["J"], X, a["ldx"], DY, a["ldy"], a["dw"], a["ldw"], DB, 0, a["ws"])
    _refused(lib, rc, code, text)


@pytest.mark.parametrize("jblock", [0, 6, 16, 24, 80])     # 16 and 24 do not divide 40; 6 is no multiple of 4
def test_gemm_dw_blocked_refuses_jblock_on_the_host(lib, jblock):
    rc = lib.sae_gemm_dw_blocked(None, 300, 16, 40, jblock, X, 16, DY, 40, DW, DB, 0, WS)
    _refused(lib, rc, L.SAE_EINVAL, "must be a multiple of 4 dividing J")


@pytest.mark.parametrize("kw,code,text", [
    (dict(ldc=12), L.SAE_EINVAL, "ldc (12) < N (16)"),
    (dict(K=2050, sam=2052), L.SAE_EUNSUPPORTED, "A needs unit stride along k"),      # K % 4, A k-contiguous
    (dict(K=2050, sam=1, sak=8, sbk=1, sbn=2052), L.SAE_EUNSUPPORTED, "B needs unit stride along k"),
    (dict(ws=None), L.SAE_EINVAL, "this shape splits K"),                             # S = 2, NULL workspace
    (dict(ws=ctypes.c_void_p(0x50004)), L.SAE_EINVAL, "this shape splits K"),
], ids=["ldc_lt_N", "K_mod_4_on_A", "K_mod_4_on_B", "split_ws_null", "split_ws_misaligned"])
def test_gemm_f32_refuses_on_the_host(lib, kw, code, text):
    a = dict(M=8, N=16, K=2048, sam=2048, sak=1, sbk=16, sbn=1, ldc=16, ws=WS)
    a.update(kw)
    assert S.f32_plan(a["M"], a["N"], 2048).S == 2
    rc = lib.sae_gemm_f32(None, a["M"], a["N"], a["K"], X, a["sam"], a["sak"], DY, a["sbk"], a["sbn"], None, DW,
                          a["ldc"], None, 0, a["ws"])
    _refused(lib, rc, code, text)


# ------------------------------------------------------------- the four checks, on emulated kernels
# ``check_dw`` / ``check_f32`` are what every GPU case runs.  Here they run on the CPU against a plain
# torch emulation of the split kernels and the reduce (same plan, same workspace layout): the faithful
# emulation passes, and each deliberately broken one trips the assertion that is there for it.
def _emu_dw(slots=None, skip_short_groups=False, ld_is_J=False, no_last_bias=False, extra_plane=False):
    def call(x, dy, dw, db, acc, ws, jblock=0):
        (M, I), J = x.shape, dy.shape[1]
        p = S.dw_plan(M, I, J)
        n, chunk = (p.S, p.chunk) if slots is None else S.dw_split(M, I, J, slots)
        xs, ds = x.float(), dy.float()
        for s in range(n):                                       # the splits
            rows = slice(s * chunk, min(M, (s + 1) * chunk))
            ws[s * I * J:(s + 1) * I * J] = (xs[rows].T @ ds[rows]).flatten()
            if db is not None and not (no_last_bias and s == n - 1):
                o = S.round256(n * I * J * 4) // 4 + s * J
                ws[o:o + J] = ds[rows].sum(0)
        per = S.cdiv(n, S.DW_RED_GROUPS)                          # the reduce: four groups in order
        tot = torch.zeros(I * J)
        for g in range(S.DW_RED_GROUPS):
            s0, s1 = g * per, min(n, (g + 1) * per)
            if skip_short_groups and s1 - s0 < per:
                continue
            for s in range(s0, s1 + (1 if extra_plane and g == 0 else 0)):
                tot += ws[s * I * J:(s + 1) * I * J]
        tot = tot.view(I, J)
        if jblock:
            tot = torch.as_tensor(S.blocked(tot.numpy(), jblock))
        out = torch.as_strided(dw, dw.shape, (J, 1)) if ld_is_J and not jblock else dw
        out.copy_(out + tot if acc else tot)
        if db is not None:
            o = S.round256(n * I * J * 4) // 4
            totb = sum(ws[o + s * J:o + (s + 1) * J] for s in range(n))
            db.copy_(db + totb if acc else totb)
    return call


def _emu_f32(bias_on_ones_row=False, drop_k_tail=False, part_rows_M1=False):
    def call(shape, a, sa, b, sb, bias, c, colsum, acc, ws):
        M, N, K = shape
        p = S.f32_plan(M, N, K)
        A = a if sa[1] == 1 else a.T                              # [M, K]
        B = b if sb[1] == 1 else b.T                              # [K, N]
        Mx = M + (1 if colsum is not None or part_rows_M1 else 0)
        tot = torch.zeros(Mx, N)
        for z in range(p.S):
            k1 = min(K, (z + 1) * p.kchunk)
            if drop_k_tail:
                k1 -= k1 % S.F32_K
            ks = slice(z * p.kchunk, k1)
            part = torch.zeros(Mx, N)
            part[:M] = A[:, ks] @ B[ks]
            if Mx > M:
                part[M] = B[ks].sum(0)
            if p.S > 1:
                ws[z * Mx * N:(z + 1) * Mx * N] = part.flatten()
                part = ws[z * Mx * N:(z + 1) * Mx * N].view(Mx, N)
            tot += part
        r = tot[:M] + (bias if bias is not None else 0)
        c.copy_(c + r if acc else r)
        if colsum is not None:
            row = tot[M] + (bias if bias is not None and bias_on_ones_row else 0)
            colsum.copy_(colsum + row if acc else row)
    return call


SMALL_DW = [r for r in S.DW_ROWS if r[0][0] * r[0][1] * r[0][2] <= 1 << 24]
SMALL_F32 = [r for r in S.F32_ROWS if r[0][0][0] * r[0][0][1] * r[0][0][2] <= 1 << 24]


@pytest.mark.parametrize("shape,claims", SMALL_DW, ids=[S.dw_id(r[0]) for r in SMALL_DW])
def test_checks_pass_on_a_faithful_dw_emulation(shape, claims):
    for with_db, acc, padded in ((False, 0, False), (True, 1, True), (True, 0, False), (False, 1, True)):
        S.check_dw("cpu", shape, with_db, acc, padded, claims=claims, call=_emu_dw())
    for s, jb in S.DW_BLOCKED:
        if s == shape:
            S.check_dw("cpu", shape, True, 1, True, jblock=jb, call=_emu_dw())


@pytest.mark.parametrize("key,claims", SMALL_F32, ids=[S.f32_id(r[0]) for r in SMALL_F32])
def test_checks_pass_on_a_faithful_f32_emulation(key, claims):
    for combo in ((False, False, 0, 0), (True, True, 1, 4), (True, False, 0, 4), (False, True, 1, 0)):
        S.check_f32("cpu", key, *combo, claims=claims, call=_emu_f32())


@pytest.mark.parametrize("shape,variant,broken,match", [
    # a reduce group shorter than the others is skipped: only S = 5 (groups 2, 2, 1, 0) notices
    ((1280, 8, 8), (True, 0, False), dict(skip_short_groups=True), "dw differs"),
    # the reduce indexes dw with J for ldw: only a padded dw notices
    ((33, 136, 128), (False, 0, True), dict(ld_is_J=True), "differs|written outside"),
    # right numbers from the wrong plan (512 slots under two wave groups): only the workspace notices
    ((2048, 1024, 1024), (False, 0, False), dict(slots=512), "outside the plan's partials"),
    ((2048, 1024, 1024), (True, 1, False), dict(slots=128), "written by no split"),
    # the reduce reads a bias row no split wrote (a NaN from the sentinel); group 0 runs one plane on
    ((257, 8, 264), (True, 0, True), dict(no_last_bias=True), "db differs"),
    ((257, 8, 264), (False, 1, False), dict(extra_plane=True), "dw differs"),
], ids=["short_group", "ldw_is_J", "plan_512_slots", "plan_128_slots", "bias_row_unwritten", "plane_read_twice"])
def test_checks_catch_a_broken_dw_emulation(shape, variant, broken, match):
    S.check_dw("cpu", shape, *variant, call=_emu_dw())
    with pytest.raises(AssertionError, match=match):
        S.check_dw("cpu", shape, *variant, call=_emu_dw(**broken))


@pytest.mark.parametrize("key,variant,broken,match", [
    (((8, 8, 2048), "fwd"), (True, True, 0, 4), dict(bias_on_ones_row=True), "colsum differs"),
    (((132, 136, 2052), "dgrad"), (False, False, 1, 0), dict(drop_k_tail=True), "c differs"),
    (((128, 128, 3072), "fwd"), (True, False, 0, 4), dict(part_rows_M1=True), "outside the plan's partials"),
], ids=["bias_on_ones_row", "ragged_k_tile_dropped", "ones_row_without_colsum"])
def test_checks_catch_a_broken_f32_emulation(key, variant, broken, match):
    S.check_f32("cpu", key, *variant, call=_emu_f32())
    with pytest.raises(AssertionError, match=match):
        S.check_f32("cpu", key, *variant, call=_emu_f32(**broken))
