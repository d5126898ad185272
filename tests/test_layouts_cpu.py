"""The route x layout matrix, its CPU half: the case table shared with ``test_gpu_layouts.py``, the
route of every case under every layout of ``_layouts.py`` (``sae_attn_route`` / ``sae_th_attn_route``
need no device), the coverage of the kernel instance tables by the cases, and self-tests of the
arena / view / guard helpers.

Shapes.  Key tiles are 64 keys wide, a forward workgroup holds 128 query rows and the single-pass
backward (bwd3) ends at 256 keys: ``Nq 150, Nk 70`` gives a second, ragged workgroup and a six-key
tail tile; the two-pass backward runs at ``Nq 70, Nk 300``; talking heads at ``Nq 70, Nk 45``;
relative logits at Nq = Nk = the grid.  Batch 2 throughout, so a batch stride is used."""
import os
import re

import numpy as np
import pytest

import _layouts as Y
from _layouts import BWD, FWD, Case, Refused, pair, th2_bwd, th_v1, v1
from sae_vision_amd import _lib as L
from test_routing_cpu import (ATTN_BASELINE, TH_BASELINE, TH_KNOB_ROWS)


def _core(kind, D, fwd, bwd, sfx="", **kw):
    """A core-attention case: the scalar layouts take the v1 scalar kernels of the padded head dim
    (none with rotary)."""
    dt = kw.get("dtype", "bf16")
    if kind == "rot":
        fs = bs = Refused(Y.NO_ROTARY)
    else:
        fs, bs = (v1(p, dt, Y.pad_dim(D), sfx, scalar=True) for p in (FWD, BWD))
    return Case(kind, D, fwd, bwd, fs, bs, **kw)


def _v1_case(kind, D, sfx="", **kw):
    """A case the v1 kernels serve on every layout (fp32, wide relative tables, the dropout rest)."""
    dt = kw.get("dtype", "bf16")
    scalar = D % Y.EPC[dt] != 0
    return _core(kind, D, *(v1(p, dt, Y.pad_dim(D), sfx, scalar=scalar) for p in (FWD, BWD)), sfx=sfx, **kw)


def _th(kind, H, D, fwd, bwd, dtype="bf16"):
    """A talking-heads case (Nq 70, Nk 45): the scalar layouts take ``th_*_scalar`` up to 8 heads,
    never with rotary."""
    if kind == "th_rot":
        fs = bs = Refused(Y.NO_TH_ROTARY)
    elif H > 8:
        fs = bs = Refused(Y.no_th_heads(H))
    else:
        fs, bs = (th_v1(p, dtype, Y.pad_dim(D), scalar=True) for p in (FWD, BWD))
    return Case(kind, D, fwd, bwd, fs, bs, H=H, Nq=70, Nk=45, dtype=dtype)


LONG = dict(Nq=70, Nk=300)      # past bwd3's 256 keys: the two-pass backward
G57 = dict(Nq=35, Nk=35, grid=(5, 7))
G816 = dict(Nq=128, Nk=128, grid=(8, 16))
G333 = dict(Nq=99, Nk=99, grid=(3, 33))   # 36 table columns: past the lean kernels' 32

CASES = [
    # ---- plain bf16 core
    _core("plain", 32, "fwd2_d32", "bwd3_d32"),
    _core("plain", 40, "fwd2_d64_k3", "bwd3_d64_k3"),          # the last 16-byte chunk pair partly past D
    _core("plain", 56, "fwd2_d64", "bwd3_d64"),
    _core("plain", 64, "fwd2_d64", "bwd3_d64"),
    _core("plain", 96, "fwd2_d128", pair("d128_agpr")),
    _core("plain", 128, "fwd2_d128", pair("d128_agpr")),
    _core("plain", 32, "fwd2_d32", pair("d32"), **LONG),
    _core("plain", 48, "fwd2_d64_k3", pair("d64"), **LONG),
    _core("plain", 40, "cls_fwd_1", "cls_bwd_1", Nq=1, Nk=300),
    _core("plain", 72, "cls_fwd_2", "cls_bwd_2", Nq=1, Nk=70),
    # ---- relative logits
    _core("rel", 16, "fwd2_d32_rel", pair("d32_rel"), "_rel", **G57),
    _core("rel", 64, "fwd2_d64_rel", pair("d64_rel"), "_rel", **G57),
    _core("rel", 128, "fwd2_d128_rel", pair("d128_rel"), "_rel", **G57),
    _core("rel", 128, "fwd2_d128_rel", "bwd2_dq_d128_rel_agpr+bwd2_dkdv_d128_rel", "_rel", **G816),
    _v1_case("rel", 32, "_rel", **G333),
    _v1_case("rel", 64, "_rel", **G333),
    _v1_case("rel", 32, "_rel", dtype="f32", **G57),
    # ---- fused rotary
    _core("rot", 32, "fwd2_d32_rot", "bwd3_d32_rot"),
    _core("rot", 48, "fwd2_d64_rot", "bwd3_d64_rot"),
    _core("rot", 32, "fwd2_d32_rot", pair("d32_rot"), **LONG),
    _core("rot", 64, "fwd2_d64_rot", pair("d64_rot"), **LONG),
    # ---- attention-probability dropout, rate 0.5
    _core("drop", 32, "fwd2_d32_drop", "bwd3_d32_drop", "_drop"),
    _core("drop", 40, "fwd2_d64_k3_drop", "bwd3_d64_k3_drop", "_drop"),
    _core("drop", 64, "fwd2_d64_drop", "bwd3_d64_drop", "_drop"),
    _core("drop", 32, "fwd2_d32_drop", pair("d32_drop"), "_drop", **LONG),
    _core("drop", 64, "fwd2_d64_drop", pair("d64_drop"), "_drop", **LONG),
    _v1_case("drop", 128, "_drop"),
    _v1_case("drop", 48, "_drop", Nq=1),
    _v1_case("drop", 32, "_drop", Nq=1),
    _v1_case("drop", 32, "_drop", dtype="f32"),
    # ---- fp32: always v1
    _v1_case("plain", 64, dtype="f32"),
    _v1_case("plain", 128, dtype="f32"),
    _v1_case("plain", 10, dtype="f32"),                         # scalar by head_dim on every layout
    # ---- talking heads
    _th("th", 4, 32, "th2_fwd_d32", th2_bwd("d32", "d32")),
    _th("th", 9, 24, "th2_fwd_d32_h16", th2_bwd("d32_h16", "d32_h16")),
    _th("th", 8, 40, "th2_fwd_d64_k3", th2_bwd("d64_lean_k3", "d64")),
    _th("th", 8, 64, "th2_fwd_d64", th2_bwd("d64_lean", "d64")),
    _th("th", 12, 48, "th2_fwd_d64_h16", th2_bwd("d64_h16", "d64_h16")),
    _th("th_rot", 4, 32, "th2_fwd_d32_rot", th2_bwd("d32_rot", "d32_rot")),
    _th("th_rot", 16, 32, "th2_fwd_d32_rot_h16", th2_bwd("d32_rot_h16", "d32_rot_h16")),
    _th("th_rot", 8, 40, "th2_fwd_d64_rot_k3", th2_bwd("d64_rot_lean_k3", "d64_rot")),
    _th("th_rot", 8, 56, "th2_fwd_d64_rot", th2_bwd("d64_rot", "d64_rot")),
    _th("th_rot", 12, 48, "th2_fwd_d64_rot_h16", th2_bwd("d64_rot_h16", "d64_rot_h16")),
    _th("th_rot", 8, 64, "th2_fwd_d64_rot", th2_bwd("d64_rot", "d64_rot")),
    _th("th", 4, 48, th_v1(FWD, "f32", 64), th_v1(BWD, "f32", 64), dtype="f32"),
]
CASE_IDS = [c.id for c in CASES]
MATRIX = [(c, lay) for c in CASES for lay in Y.LAYOUTS]
MATRIX_IDS = [f"{c.id}-{lay}" for c, lay in MATRIX]


@pytest.fixture(scope="module")
def lib():
    return L.load()


def test_case_ids_are_unique():
    assert len(set(CASE_IDS)) == len(CASES)


# ------------------------------------------------------------------------------------ routing
@pytest.mark.parametrize("case,layout", MATRIX, ids=MATRIX_IDS)
def test_layout_route(lib, case, layout):
    """The descriptor of the stride triples alone validates, and its route is the one the case
    declares: the control's on a vector layout, the scalar kernels' (or the documented refusal) on a
    scalar one."""
    p = Y.plan(case, layout)
    d = Y.plan_desc(lib, p)
    scalar = Y.is_scalar(case, layout)
    if case.D % case.epc == 0:   # (head_dim 10: v of the packed pair starts 30 elements in)
        assert p.aligned == (layout != "misaligned_ptr")
    ctl = Y.plan_desc(lib, Y.plan(case, "contig"))
    for pas in (FWD, BWD):
        want = case.declared(pas, scalar)
        got = Y.route(lib, case.route_fn, d, pas, case.form, int(p.aligned))
        if isinstance(want, Refused):
            assert scalar and got is None, (got, want)
            assert lib.sae_last_error().decode().startswith(want.text)
            assert layout not in Y.gpu_layouts(case)
            continue
        assert got is not None, lib.sae_last_error().decode()
        assert got == want
        if not scalar:
            assert got == Y.route(lib, case.route_fn, ctl, pas, case.form, 1) == case.declared(pas, False)
        assert layout == "contig" or layout in Y.gpu_layouts(case)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_scalar_declaration_matches_the_strides(case):
    """``is_scalar`` restates csrc/desc.h ``desc_vec`` (head_dim, every stride, every pointer)."""
    for layout in Y.LAYOUTS:
        p = Y.plan(case, layout)
        vec = p.aligned and case.D % case.epc == 0 and all(s % case.epc == 0 for n in Y.TENSORS for s in p.strides(n))
        assert vec == (not Y.is_scalar(case, layout)), layout


# ----------------------------------------------------------------------------------- coverage
def _table_rows():
    csrc = os.path.join(os.path.dirname(L.__file__), "csrc")
    rows = set()
    for f in ("attn.hip", "bwd2_run.h", "th.hip"):
        rows |= set(re.findall(r"^  X\((\w+),", open(os.path.join(csrc, f)).read(), re.M))
    return rows


def _covered(cases):
    return {s for c in cases for s in c.steps()}


def _v1_names():
    """The v1 / th-v1 instances the routing pins name, plus the two the scalar layouts add."""
    pinned = [want for want, *_ in ATTN_BASELINE + TH_BASELINE]
    # test_unaligned_pointers_take_the_scalar_kernels
    pinned += ["v1_fwd_bf16_d64_scalar", "v1_bwd_dq_bf16_d64_scalar_drop+v1_bwd_dkdv_bf16_d64_scalar_drop",
               "th_fwd_bf16_d64_scalar"]
    pinned += [v1(p, "bf16", 128, scalar=True) for p in (FWD, BWD)] + [v1(p, "f32", 64, scalar=True) for p in (FWD, BWD)]
    return {s for want in pinned for s in want.split("+") if s.startswith("v1_") or re.match(r"th_(fwd|bwd)", s)}


def missing_rows(cases):
    """Instance-table rows and pinned v1 names no declared route of ``cases`` runs."""
    return sorted((_table_rows() - TH_KNOB_ROWS | _v1_names()) - _covered(cases))


def test_every_table_row_has_a_layout_case():
    """A row added to an instance table needs a case here as well as its routing pin."""
    rows = _table_rows()
    assert len(rows) >= 12 + 8 + 9 + 9 + 3 + 4 + 10 + 11 + 8, sorted(rows)   # the regex still finds the tables
    assert len(_v1_names()) >= 20, sorted(_v1_names())
    assert missing_rows(CASES) == []


def test_coverage_names_the_row_that_lost_its_case():
    lost = [c for c in CASES if not (c.kind == "rot" and c.D == 48)]
    assert missing_rows(lost) == ["bwd3_d64_rot"]
    lost = [c for c in CASES if not (c.kind == "plain" and c.dtype == "f32" and c.D == 64)]
    assert missing_rows(lost) == ["v1_bwd_dkdv_f32_d64", "v1_bwd_dkdv_f32_d64_scalar", "v1_bwd_dq_f32_d64",
                                  "v1_bwd_dq_f32_d64_scalar", "v1_fwd_f32_d64", "v1_fwd_f32_d64_scalar"]


# --------------------------------------------------------------------------- layout self-tests
def _np_values(case, seed=0):
    rng = np.random.default_rng(seed)
    return {n: rng.integers(-64, 64, case.shape(n)).astype(np.float32) for n in Y.TENSORS}   # exact in bf16


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_distinct_strides_are_pairwise_different(case):
    """In each stride position the eight values differ, so swapping any two tensors' strides moves an
    address; all are whole 16-byte chunks where head_dim is."""
    p = Y.plan(case, "distinct")
    for pos in range(3):
        vals = [p.strides(n)[pos] for n in Y.TENSORS]
        assert len(set(vals)) == 8, (pos, vals)
        if case.D % case.epc == 0:
            assert all(v % case.epc == 0 for v in vals)
    for n in Y.TENSORS:
        B, N, H, D = case.shape(n)
        sb, st, sh = p.strides(n)
        assert sh >= D and st > H * sh and sb > N * st and (sb - N * st) % case.epc == 0
    assert any(p.strides(n)[2] == case.D for n in Y.TENSORS) and any(p.strides(n)[2] > case.D for n in Y.TENSORS)


@pytest.mark.parametrize("case,layout", MATRIX, ids=MATRIX_IDS)
def test_a_foreign_stride_stays_inside_the_arena(case, layout):
    """A tensor addressed with another tensor's stride in any position (and with one row more than it
    has) stays inside its arena; under ``distinct`` its last element moves, so the slip is visible."""
    p = Y.plan(case, layout)
    for a in Y.TENSORS:
        va = p.views[a]
        B, N, H, D = va.shape
        for b in Y.TENSORS:
            for pos, size in enumerate((B, N, H)):
                s = list(va.strides)
                s[pos] = p.strides(b)[pos]
                slipped = Y.View(a, va.arena, va.offset, (B, N + 1, H, D), s)
                assert slipped.offset + slipped.extent <= p.arenas[va.arena], (a, b, pos)
                if layout == "distinct" and a != b and size > 1:
                    assert Y.View(a, va.arena, va.offset, va.shape, s).extent != va.extent, (a, b, pos)


@pytest.mark.parametrize("case,layout", MATRIX, ids=MATRIX_IDS)
def test_plan_geometry(case, layout):
    """Views of one arena do not overlap (nor does a view overlap itself), and each lies inside its
    arena with a guard of at least the largest tensor extent of the case on both sides."""
    p = Y.plan(case, layout)
    biggest = max(v.extent for v in p.views.values())
    assert p.guard >= biggest and p.guard % Y.GUARD_ALIGN == 0
    for arena, numel in p.arenas.items():
        ix = np.concatenate([v.indices().ravel() for v in p.views_of(arena)])
        assert len(np.unique(ix)) == len(ix), "views overlap"
        assert ix.min() >= p.guard and ix.max() < numel - p.guard
    if layout == "kv_packed":
        assert p.views["k"].arena == p.views["v"].arena and p.views["dk"].arena == p.views["dv"].arena
        assert p.views["dv"].offset - p.views["dk"].offset == case.H * case.D
        assert len(p.arenas) == 6
    else:
        assert len(p.arenas) == 8
    if layout == "head_major":
        for n in Y.TENSORS:
            N = case.shape(n)[1]
            assert p.strides(n) == (case.H * N * case.D, case.D, N * case.D)
    if layout == "odd_stride":
        q = Y.plan(case, "distinct")
        for n in Y.TENSORS:
            assert p.strides(n)[1] - q.strides(n)[1] == (case.epc // 2 if n in ("k", "dq") else 0)
    if layout == "misaligned_ptr":
        assert all(v.offset % case.epc == 1 for v in p.views.values())
        assert all(p.strides(n) == Y.plan(case, "distinct").strides(n) for n in Y.TENSORS)


SELF_TEST_CASES = [CASES[1], CASES[-1]]    # one bf16 (D 40), one fp32


@pytest.mark.parametrize("case", SELF_TEST_CASES, ids=[c.id for c in SELF_TEST_CASES])
@pytest.mark.parametrize("layout", Y.LAYOUTS)
def test_views_hold_the_values_and_the_declared_strides(case, layout):
    import torch
    vals = _np_values(case)
    p = Y.plan(case, layout)
    arenas, views = Y.materialise(p, "cpu", vals)
    for n in Y.TENSORS:
        assert tuple(views[n].shape) == case.shape(n)
        assert views[n].stride() == p.strides(n) + (1,)
        assert (views[n].data_ptr() % 16 == 0) == (layout != "misaligned_ptr")
        assert np.array_equal(views[n].float().numpy(), vals[n])                       # read back
        assert np.array_equal(arenas[p.views[n].arena].float().numpy()[p.views[n].indices()], vals[n])
    for arena in p.arenas:
        Y.assert_guards_intact(arenas[arena], *(views[v.name] for v in p.views_of(arena)))
        own = np.zeros(p.arenas[arena], bool)
        for v in p.views_of(arena):
            own[v.indices().ravel()] = True
        assert torch.isnan(arenas[arena][torch.as_tensor(~own)]).all()     # the padding is NaN


@pytest.mark.parametrize("case", SELF_TEST_CASES, ids=[c.id for c in SELF_TEST_CASES])
@pytest.mark.parametrize("layout", ["contig", "distinct", "kv_packed", "misaligned_ptr"])
def test_guard_check_is_not_vacuous(case, layout):
    """One planted element in the guard before a view, after it, or in the padding between its rows
    fails ``assert_guards_intact``; a write inside the view does not."""
    p = Y.plan(case, layout)
    for name in Y.OUTPUTS:
        v = p.views[name]
        mine = [v2.name for v2 in p.views_of(v.arena)]
        own = np.zeros(p.arenas[v.arena], bool)
        for v2 in p.views_of(v.arena):
            own[v2.indices().ravel()] = True
        spots = {"first element": 0, "just before the view": int(np.flatnonzero(own)[0]) - 1,
                 "just after the view": int(np.flatnonzero(own)[-1]) + 1, "last element": len(own) - 1}
        holes = np.flatnonzero(~own[p.guard:len(own) - p.guard])
        if len(holes):
            spots["padding inside the extent"] = p.guard + int(holes[len(holes) // 2])
        for what, at in spots.items():
            arenas, views = Y.materialise(p, "cpu")
            views[name].fill_(1.0)                    # inside the view: fine
            Y.assert_guards_intact(arenas[v.arena], *(views[m] for m in mine))
            arenas[v.arena][at] = 0.0                 # one element outside
            with pytest.raises(AssertionError, match="written outside the tensor"):
                Y.assert_guards_intact(arenas[v.arena], *(views[m] for m in mine))
        if layout == "kv_packed" and name == "dk":    # an overrun of dk lands in dv: seen only with dv left out
            arenas, views = Y.materialise(p, "cpu")
            views["dv"][0, 0, 0, 0] = 1.0
            Y.assert_guards_intact(arenas[v.arena], views["dk"], views["dv"])
            with pytest.raises(AssertionError, match="written outside the tensor"):
                Y.assert_guards_intact(arenas[v.arena], views["dk"])
