"""Projection and attention routing (CPU: the routing predicates only, no device needed).

Every forward and input-gradient GEMM of every attention encoder width in the reference's model
registry (models/create_model.py:6-215 -- ViT-B/L, CaiT XXS..M, CeiT, CvT, TNT inner / outer;
plus DeiT-Ti/S of SURVEY D10) must run on this repo's ``sae_gemm_nt``: the Dense plans
(``ops.dense_fwd_plan`` / ``dense_bwd_plan``) send it there, and ``sae_gemm_nt_route`` (the C ABI's
kernel choice, include/sae_attn.h) must name a HIP kernel for it.  The projections are
attention.py:29-37,60-63 and the FF block ff.py:8-34.
The rocprofv3 step profiles confirm on the GPU that no library GEMM runs (profiles/)."""
import pytest

import _gemm_rows as G   # one pinned call per gemm_nt instance row, shared with tests/test_gpu_gemm_nt.py
import sae_vision_amd.ops as ops
from _layouts import desc as _desc, route as _route   # one way to build a descriptor, shared with the layout matrix
from sae_vision_amd import _lib as L

NONE, TILE128, KTAIL, GEMM8, GEMM8X = 0, 1, 2, 3, 4

# (model, embed width C, FF hidden) -- create_model.py line cited per entry
WIDTHS = [
    ("vit_b (create_model.py:10-23)", 768, 3072),
    ("vit_l (create_model.py:24-37)", 1024, 4096),
    ("tnt_s outer (create_model.py:50-56)", 640, 2560),
    ("tnt_s inner (create_model.py:50-56)", 40, 160),
    ("tnt_b outer (create_model.py:57-63)", 384, 1536),
    ("tnt_b inner (create_model.py:57-63)", 24, 96),
    ("ceit_t (create_model.py:64-68)", 192, 768),
    ("ceit_s (create_model.py:69-73)", 384, 1536),
    ("ceit_b (create_model.py:74-78)", 768, 3072),
    ("cait_xxs (create_model.py:79-96)", 192, 768),
    ("cait_xs (create_model.py:97-114)", 288, 1152),
    ("cait_s (create_model.py:115-141)", 384, 1536),
    ("cait_m (create_model.py:142-168)", 768, 3072),
    ("cvt stage 1 (create_model.py:169-183)", 64, 256),
    ("cvt stage 2 (create_model.py:169-183)", 192, 768),
    ("cvt-13/21 stage 3 (create_model.py:169-178)", 368, 1472),
    ("cvt-w24 stage 3 (create_model.py:179-183)", 1024, 4096),
    ("deit_ti (SURVEY D10)", 192, 768),
    ("deit_s (SURVEY D10)", 384, 1536),
]


def _shapes(C, hidden):
    # (K, N, epilogue) of every forward / input-gradient GEMM of one encoder block
    return {
        "qkv_fwd": (C, 3 * C, 0), "qkv_dx": (3 * C, C, 0),
        "oproj_fwd": (C, C, 0), "oproj_dx": (C, C, 0),
        "ff0_fwd_gelu": (C, hidden, 1), "ff0_dx": (hidden, C, 0),
        "ff1_fwd": (hidden, C, 0), "ff1_dx_dgelu": (C, hidden, 2),
    }


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _dense_calls(C, hidden, M):
    # (I, column-block widths) of every ops.dense call of one encoder block, and the 1000-class head
    return {"qkv": (M, C, (C, C, C)), "kv": (M, C, (C, C)), "oproj": (M, C, (C,)), "Dense_0": (M, C, (hidden,)),
            "Dense_1": (M, hidden, (C,)), "head": (128, C, (1000,))}


@pytest.mark.parametrize("name,C,hidden", WIDTHS)
def test_every_width_routes_to_hip(lib, name, C, hidden):
    for M in (128, 197 * 32, 197 * 128):   # a classifier-head-sized call and two batch sizes
        for what, (rows, I, widths) in _dense_calls(C, hidden, M).items():
            f = ops.dense_facts_of_shapes(rows, I, widths)   # bf16, with a bias, no sinks
            sunk = f._replace(sinks_w=(True,) * len(widths), sink_b=True, adjacent=True)
            for f in (f, f._replace(has_bias=False), sunk):
                dx, dw, _ = ops.dense_bwd_plan(f)
                assert (ops.dense_fwd_plan(f), dx) == (("nt", False), "nt"), f"{name} {what} {f}: not on sae_gemm_nt"
                assert dw in ("dw", "dw_sunk", "dw_blocks", "dw_blocks_sunk", "dw_stacked"), f"{name} {what} {f}: {dw}"
        for what, (K, N, epi) in _shapes(C, hidden).items():
            r = lib.sae_gemm_nt_route(M, N, K, epi)
            assert r != NONE, f"{name} {what} (M={M}, K={K}, N={N}) has no HIP kernel"
            assert (r == KTAIL) == (K % 64 != 0), (name, what, r)


def test_baseline_shapes_take_the_persistent_kernels(lib):
    """The DeiT-S, ViT-B@384 and CaiT-S24 training shapes keep the round-4 kernel choice."""
    M_s, M_b = 128 * 197, 32 * 577
    for what, (K, N, epi) in _shapes(384, 1536).items():
        assert lib.sae_gemm_nt_route(M_s, N, K, epi) == GEMM8, what
    expect_b = {"qkv_fwd": GEMM8, "ff0_fwd_gelu": GEMM8, "ff1_dx_dgelu": TILE128,
                "qkv_dx": GEMM8X, "oproj_fwd": GEMM8X, "oproj_dx": GEMM8X, "ff0_dx": GEMM8X, "ff1_fwd": GEMM8X}
    for what, (K, N, epi) in _shapes(768, 3072).items():
        assert lib.sae_gemm_nt_route(M_b, N, K, epi) == expect_b[what], what
    # ViT-L: the 1024 / 4096-feature outputs at K >= 768 fill 256-wide tiles
    for K, N in ((1024, 1024), (4096, 1024), (3072, 1024), (1024, 4096)):
        assert lib.sae_gemm_nt_route(M_b, N, K, 0) == GEMM8X, (K, N)
    assert lib.sae_gemm_nt_route(M_b, 3072, 1024, 0) == GEMM8   # ViT-L QKV forward
    # small M (classifier head) and shallow K stay on the 128-row kernel
    assert lib.sae_gemm_nt_route(128, 1000, 384, 0) == TILE128
    assert lib.sae_gemm_nt_route(128, 384, 1000, 0) == KTAIL
    assert lib.sae_gemm_nt_route(M_s, 576, 192, 0) == TILE128


def test_unsupported_shapes(lib):
    assert lib.sae_gemm_nt_route(1024, 1000, 12, 0) == NONE
    assert lib.sae_gemm_nt_route(1024, 10, 384, 0) == NONE
    assert lib.sae_gemm_nt_route(0, 64, 64, 0) == NONE
    for I, J in ((12, 64), (64, 10)):
        f = ops.dense_facts_of_shapes(1024, I, (J,))
        assert ops.dense_fwd_plan(f)[0] == "lib" and ops.dense_bwd_plan(f)[0] != "nt", (I, J)


def test_library_switch():
    """ops.GEMM_LIB = True (A/B runs only) hands the projections to the library GEMM."""
    old = ops.GEMM_LIB
    try:
        ops.GEMM_LIB = True
        f = ops.dense_facts_of_shapes(25216, 768, (2304,))
        assert ops.dense_fwd_plan(f)[0] == "lib" and ops.dense_bwd_plan(f)[0] == "lib"
    finally:
        ops.GEMM_LIB = old
    f = ops.dense_facts_of_shapes(25216, 768, (2304,))
    assert ops.dense_fwd_plan(f)[0] == "nt" and ops.dense_bwd_plan(f)[0] == "nt"


# ``sae_gemm_nt_instance`` reports the row of gemm.hip's instance tables that nt_plan picks, by name
# (tile height, tile width, stage depth, epilogue, dropout: what the four-value route does not tell).
@pytest.mark.parametrize("M,K,N,epi,drop,want", G.NT_ROWS)
def test_gemm_nt_instance(lib, M, K, N, epi, drop, want):
    assert G.instance(lib, M, K, N, epi, drop) == want
    assert lib.sae_gemm_nt_route(M, N, K, epi) == G.route_of(want)


def test_every_gemm_nt_row_is_pinned(lib):
    """The library's row list (by index, NULL past the end) against the pins: a new row needs one."""
    rows = []
    while (name := lib.sae_gemm_nt_instance_name(len(rows))) is not None:
        rows.append(name.decode())
    assert lib.sae_gemm_nt_instance_name(-1) is None
    assert len(rows) == len(set(rows)) == 11 + 6 + 14 + 4
    assert set(rows) - G.PATCH_ROWS == {want for *_, want in G.NT_ROWS}
    assert G.PATCH_ROWS <= set(rows)


def test_gemm_nt_instance_baseline_and_refusals(lib):
    M_s, M_b = 128 * 197, 32 * 577
    # DeiT-S: 226 tiles of 224 rows on the 384-feature outputs and the QKV forward, the FF pair on 256 x 128
    assert G.instance(lib, M_s, 384, 384, G.NONE) == "g8_192_bm224_plain"
    assert G.instance(lib, M_s, 384, 1152, G.NONE) == "g8_192_bm224_plain"
    assert G.instance(lib, M_s, 384, 1536, G.GELU_GRAD) == "g8_128_wgm4_gelu"
    assert G.instance(lib, M_s, 384, 1536, G.GELU_GRAD, 1) == "g8_128_wgm4_gelu_drop"
    assert G.instance(lib, M_s, 384, 1536, G.MUL_AUX) == "g8_128_wgm4_dgelu"
    # ViT-B@384: the 768-feature outputs on gemm8x, the GELU' epilogue from h on the tall 128-row tile
    assert G.instance(lib, M_b, 3072, 768, G.NONE) == "g8x_bm224_plain"            # 249 tiles of 224 rows: one round
    assert G.instance(lib, M_b, 768, 3072, G.DGELU) == "nt128_tall_dgelu"
    assert G.instance(lib, M_b, 768, 3072, G.MUL_AUX) == "g8_192_bm256_dgelu"       # 5 rounds of 256 against 6 of 224
    for args, text in (((1024, 12, 1000, 0, 0), "gemm_nt: K (12) and N (1000) must be multiples of 8"),
                       ((0, 64, 64, 0, 0), "gemm_nt: M/N/K must be >= 1"),
                       ((128, 64, 64, 5, 0), "gemm_nt: unknown epilogue 5"),
                       ((128, 64, 64, G.GELU, 1), "gemm_nt: dropout rides on the SAE_EPI_GELU_GRAD epilogue only")):
        assert G.instance(lib, *args) is None
        assert lib.sae_last_error().decode().startswith(text)


# ------------------------------------------------------------------ attention routing
# ``sae_attn_route`` / ``sae_th_attn_route`` report the plan the entry points launch (attn.hip
# attn_plan, th.hip th_plan) by name: the rows of the instance tables, in launch order.  Every
# expectation below is derived from the dispatch cascade those plans replaced, not from their output.
FWD, BWD = L.SAE_PASS_FWD, L.SAE_PASS_BWD
PLAIN, ROT, DROP = L.SAE_FORM_PLAIN, L.SAE_FORM_ROTARY, L.SAE_FORM_DROPOUT
BF16, F32 = L.SAE_DTYPE_BF16, L.SAE_DTYPE_F32


def _pair(sfx):
    return f"bwd2_dq_{sfx}+bwd2_dkdv_{sfx}"


# (route, pass, form, descriptor arguments): one pin per row of the lean tables
ATTN_ROWS = [
    # forward: three waves per SIMD at dp <= 64 (NSU 3 at head_dim <= 48), MFMA row sum at dp 128
    ("fwd2_d32", FWD, PLAIN, dict(Nq=50, Nk=50, D=32)),
    ("fwd2_d64_k3", FWD, PLAIN, dict(Nq=50, Nk=50, D=48)),
    ("fwd2_d64", FWD, PLAIN, dict(Nq=50, Nk=50, D=64)),
    ("fwd2_d128", FWD, PLAIN, dict(Nq=50, Nk=50, D=128)),
    ("fwd2_d32_rot", FWD, ROT, dict(Nq=50, Nk=50, D=32)),
    ("fwd2_d64_rot", FWD, ROT, dict(Nq=50, Nk=50, D=64)),
    ("fwd2_d64_rot", FWD, ROT, dict(Nq=50, Nk=50, D=48)),      # rotary has no NSU 3 instance
    ("fwd2_d64_rot", FWD, ROT, dict(Nq=1, Nk=50, D=64)),       # and rides the lean kernel at Nq 1
    ("fwd2_d32_rel", FWD, PLAIN, dict(Nq=49, Nk=49, D=32, grid=(7, 7))),
    ("fwd2_d64_rel", FWD, PLAIN, dict(Nq=49, Nk=49, D=64, grid=(7, 7))),
    ("fwd2_d128_rel", FWD, PLAIN, dict(Nq=49, Nk=49, D=128, grid=(7, 7))),
    ("fwd2_d32_drop", FWD, DROP, dict(Nq=50, Nk=50, D=32)),
    ("fwd2_d64_k3_drop", FWD, DROP, dict(Nq=50, Nk=50, D=48)),
    ("fwd2_d64_drop", FWD, DROP, dict(Nq=50, Nk=50, D=64)),
    # backward, Nk <= 256 and dp <= 64: the single pass
    ("bwd3_d32", BWD, PLAIN, dict(Nq=50, Nk=256, D=32)),
    ("bwd3_d64_k3", BWD, PLAIN, dict(Nq=50, Nk=50, D=40)),
    ("bwd3_d64", BWD, PLAIN, dict(Nq=50, Nk=50, D=64)),
    ("bwd3_d32_rot", BWD, ROT, dict(Nq=50, Nk=50, D=32)),
    ("bwd3_d64_rot", BWD, ROT, dict(Nq=50, Nk=50, D=48)),
    ("bwd3_d32_drop", BWD, DROP, dict(Nq=50, Nk=50, D=32)),
    ("bwd3_d64_k3_drop", BWD, DROP, dict(Nq=50, Nk=50, D=48)),
    ("bwd3_d64_drop", BWD, DROP, dict(Nq=50, Nk=50, D=64)),
    # backward, longer key ranges: the dQ pass, then the dK / dV pass
    (_pair("d32"), BWD, PLAIN, dict(Nq=50, Nk=257, D=32)),
    (_pair("d64"), BWD, PLAIN, dict(Nq=50, Nk=300, D=48)),
    (_pair("d32_rot"), BWD, ROT, dict(Nq=50, Nk=300, D=32)),
    (_pair("d64_rot"), BWD, ROT, dict(Nq=50, Nk=300, D=64)),
    (_pair("d32_drop"), BWD, DROP, dict(Nq=50, Nk=300, D=32)),
    (_pair("d64_drop"), BWD, DROP, dict(Nq=50, Nk=300, D=48)),
    # relative logits never take bwd3
    (_pair("d32_rel"), BWD, PLAIN, dict(Nq=49, Nk=49, D=32, grid=(7, 7))),
    (_pair("d64_rel"), BWD, PLAIN, dict(Nq=49, Nk=49, D=64, grid=(7, 7))),
    (_pair("d128_rel"), BWD, PLAIN, dict(Nq=49, Nk=49, D=128, grid=(7, 7))),
    ("bwd2_dq_d128_rel_agpr+bwd2_dkdv_d128_rel", BWD, PLAIN, dict(Nq=128, Nk=128, D=128, grid=(8, 16))),
    (_pair("d128_agpr"), BWD, PLAIN, dict(Nq=50, Nk=50, D=128)),
    # a single query row without relative logits, before the lean kernels
    ("cls_fwd_1", FWD, PLAIN, dict(Nq=1, Nk=50, D=64)),
    ("cls_fwd_2", FWD, PLAIN, dict(Nq=1, Nk=50, D=72)),
    ("cls_bwd_1", BWD, PLAIN, dict(Nq=1, Nk=300, D=32)),
    ("cls_bwd_2", BWD, PLAIN, dict(Nq=1, Nk=50, D=128)),
]

ATTN_BASELINE = [
    ("fwd2_d64", FWD, PLAIN, dict(Nq=197, Nk=197, D=64, H=6)),              # DeiT-S
    ("bwd3_d64", BWD, PLAIN, dict(Nq=197, Nk=197, D=64, H=6)),
    (_pair("d64"), BWD, PLAIN, dict(Nq=577, Nk=577, D=64, H=12)),           # ViT-B@384
    ("cls_fwd_1", FWD, PLAIN, dict(Nq=1, Nk=197, D=48, H=8)),               # CaiT class attention
    ("cls_bwd_1", BWD, PLAIN, dict(Nq=1, Nk=197, D=48, H=8)),
    ("fwd2_d128", FWD, PLAIN, dict(Nq=196, Nk=196, D=128)),                 # BoTNet 14 x 14
    (_pair("d128_agpr"), BWD, PLAIN, dict(Nq=196, Nk=196, D=128)),
    ("fwd2_d128_rel", FWD, PLAIN, dict(Nq=196, Nk=196, D=128, grid=(14, 14))),
    ("bwd2_dq_d128_rel_agpr+bwd2_dkdv_d128_rel", BWD, PLAIN, dict(Nq=196, Nk=196, D=128, grid=(14, 14))),
    ("fwd2_d128", FWD, PLAIN, dict(Nq=49, Nk=49, D=128)),                   # BoTNet 7 x 7
    (_pair("d128_agpr"), BWD, PLAIN, dict(Nq=49, Nk=49, D=128)),
    ("fwd2_d128_rel", FWD, PLAIN, dict(Nq=49, Nk=49, D=128, grid=(7, 7))),
    (_pair("d128_rel"), BWD, PLAIN, dict(Nq=49, Nk=49, D=128, grid=(7, 7))),
    # a 40 x 40 grid: 80 table columns do not fit the lean kernels' 32
    ("v1_fwd_bf16_d64_rel", FWD, PLAIN, dict(Nq=1600, Nk=1600, D=64, grid=(40, 40))),
    ("v1_bwd_dq_bf16_d64_rel+v1_bwd_dkdv_bf16_d64_rel", BWD, PLAIN, dict(Nq=1600, Nk=1600, D=64, grid=(40, 40))),
    # head_dim 10 is no whole number of 16-byte chunks; fp32 always takes v1
    ("v1_fwd_bf16_d32_scalar", FWD, PLAIN, dict(Nq=50, Nk=50, D=10)),
    ("v1_bwd_dq_bf16_d32_scalar+v1_bwd_dkdv_bf16_d32_scalar", BWD, PLAIN, dict(Nq=50, Nk=50, D=10)),
    ("v1_fwd_f32_d64", FWD, PLAIN, dict(Nq=197, Nk=197, D=64, dtype=F32)),
    ("v1_bwd_dq_f32_d64+v1_bwd_dkdv_f32_d64", BWD, PLAIN, dict(Nq=1, Nk=197, D=64, dtype=F32)),
    # dropout: lean at dp <= 64 and Nq > 1 (pinned per row above at 32 / 48 / 64), else v1 DROP
    ("v1_fwd_bf16_d128_drop", FWD, DROP, dict(Nq=50, Nk=50, D=128)),
    ("v1_bwd_dq_bf16_d128_drop+v1_bwd_dkdv_bf16_d128_drop", BWD, DROP, dict(Nq=50, Nk=50, D=128)),
    ("v1_fwd_bf16_d64_drop", FWD, DROP, dict(Nq=1, Nk=197, D=48)),
    ("v1_bwd_dq_bf16_d32_drop+v1_bwd_dkdv_bf16_d32_drop", BWD, DROP, dict(Nq=1, Nk=197, D=32)),
    ("v1_fwd_f32_d32_drop", FWD, DROP, dict(Nq=50, Nk=50, D=32, dtype=F32)),
    ("v1_bwd_dq_bf16_d64_scalar_drop+v1_bwd_dkdv_bf16_d64_scalar_drop", BWD, DROP, dict(Nq=50, Nk=50, D=36)),
]


def _th_bwd(q, kv):
    return f"th2_bwd_q_{q}+th2_bwd_kv_{kv}+th_reduce"


TH_ROWS = [
    # forward: <= 8 heads LEAN (NSU 3 at 32 < head_dim <= 48), 9..16 heads two per wave
    ("th2_fwd_d32", FWD, PLAIN, dict(D=32, H=8)),
    ("th2_fwd_d32_h16", FWD, PLAIN, dict(D=24, H=9)),
    ("th2_fwd_d32_rot", FWD, ROT, dict(D=32, H=4)),
    ("th2_fwd_d32_rot_h16", FWD, ROT, dict(D=32, H=16)),
    ("th2_fwd_d64_k3", FWD, PLAIN, dict(D=48, H=8)),
    ("th2_fwd_d64", FWD, PLAIN, dict(D=64, H=8)),
    ("th2_fwd_d64_h16", FWD, PLAIN, dict(D=48, H=16)),
    ("th2_fwd_d64_rot_k3", FWD, ROT, dict(D=40, H=8)),
    ("th2_fwd_d64_rot", FWD, ROT, dict(D=56, H=8)),
    ("th2_fwd_d64_rot_h16", FWD, ROT, dict(D=48, H=12)),
    # backward: the query pass LEAN at dp 64 and <= 8 heads (with rotary at head_dim <= 48 only)
    (_th_bwd("d32", "d32"), BWD, PLAIN, dict(D=32, H=8)),
    (_th_bwd("d32_h16", "d32_h16"), BWD, PLAIN, dict(D=32, H=16)),
    (_th_bwd("d32_rot", "d32_rot"), BWD, ROT, dict(D=32, H=8)),
    (_th_bwd("d32_rot_h16", "d32_rot_h16"), BWD, ROT, dict(D=16, H=9)),
    (_th_bwd("d64_lean_k3", "d64"), BWD, PLAIN, dict(D=48, H=8)),
    (_th_bwd("d64_lean", "d64"), BWD, PLAIN, dict(D=64, H=4)),
    (_th_bwd("d64_rot_lean_k3", "d64_rot"), BWD, ROT, dict(D=48, H=8)),
    (_th_bwd("d64_h16", "d64_h16"), BWD, PLAIN, dict(D=48, H=16)),
    (_th_bwd("d64_rot", "d64_rot"), BWD, ROT, dict(D=64, H=8)),
    (_th_bwd("d64_rot_h16", "d64_rot_h16"), BWD, ROT, dict(D=48, H=16)),
]
# the one row no release call reaches: the query pass at one workgroup per CU without rotary is what
# SAE_TH_BWDQ_WIDE selects in the development library
TH_KNOB_ROWS = {"th2_bwd_q_d64"}

TH_BASELINE = [
    ("th2_fwd_d64_k3", FWD, PLAIN, dict(Nq=196, Nk=196, D=48, H=8)),        # CaiT-S24 trunk
    (_th_bwd("d64_lean_k3", "d64"), BWD, PLAIN, dict(Nq=196, Nk=196, D=48, H=8)),
    ("th_fwd_f32_d64", FWD, PLAIN, dict(D=48, H=8, dtype=F32)),             # fp32 / unaligned: v1
    ("th_bwd_q_bf16_d32_scalar+th_bwd_kv_bf16_d32_scalar+th_reduce", BWD, PLAIN, dict(D=12, H=4)),
]


def _args(kw):
    kw = dict(kw)
    kw.setdefault("Nq", 50)
    kw.setdefault("Nk", kw["Nq"])
    return kw


@pytest.mark.parametrize("want,pas,form,kw", ATTN_ROWS + ATTN_BASELINE)
def test_attention_route(lib, want, pas, form, kw):
    assert _route(lib, "sae_attn_route", _desc(lib, **kw), pas, form) == want


@pytest.mark.parametrize("want,pas,form,kw", TH_ROWS + TH_BASELINE)
def test_talking_heads_route(lib, want, pas, form, kw):
    assert _route(lib, "sae_th_attn_route", _desc(lib, **_args(kw)), pas, form) == want


def test_every_table_row_is_pinned():
    """A row added to an instance table needs its pin above (the tables are the X-macro lists)."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(L.__file__), "csrc")
    rows = set()
    for f in ("attn.hip", "bwd2_run.h", "th.hip"):
        rows |= set(re.findall(r"^  X\((\w+),", open(os.path.join(csrc, f)).read(), re.M))
    assert len(rows) >= 12 + 8 + 9 + 9 + 3 + 4 + 10 + 11 + 8, sorted(rows)   # the regex still finds the tables
    pinned = {step for want, *_ in ATTN_ROWS + TH_ROWS for step in want.split("+")}
    assert rows - pinned == TH_KNOB_ROWS, sorted(rows - pinned)


def test_unaligned_pointers_take_the_scalar_kernels(lib):
    d = _desc(lib, 50, 50, 64)
    assert _route(lib, "sae_attn_route", d, FWD, PLAIN, 0) == "v1_fwd_bf16_d64_scalar"
    assert _route(lib, "sae_attn_route", d, BWD, DROP, 0) == "v1_bwd_dq_bf16_d64_scalar_drop+v1_bwd_dkdv_bf16_d64_scalar_drop"
    d.k_stride[1] += 4   # a token stride that is no whole number of 16-byte chunks
    assert _route(lib, "sae_attn_route", d, FWD, PLAIN, 1) == "v1_fwd_bf16_d64_scalar"
    assert _route(lib, "sae_th_attn_route", d, FWD, PLAIN, 1) == "th_fwd_bf16_d64_scalar"


REFUSALS = [
    ("sae_attn_route", FWD, ROT, 1, dict(Nq=50, Nk=50, D=64, dtype=F32), "rotary: fused only on the bf16 path"),
    ("sae_attn_route", BWD, ROT, 1, dict(Nq=50, Nk=50, D=128),
     "rotary: fused rotary needs head_dim % 8 == 0 and <= 64 (got 128)"),
    ("sae_attn_route", FWD, ROT, 0, dict(Nq=50, Nk=50, D=64), "rotary: fused only on the bf16 path"),
    ("sae_attn_route", BWD, ROT, 1, dict(Nq=49, Nk=49, D=64, grid=(7, 7)), "rotary: fused only on the bf16 path"),
    ("sae_attn_route", FWD, DROP, 1, dict(Nq=49, Nk=49, D=64, grid=(7, 7)),
     "dropout: flags 0x1 are not supported (no relative logits)"),
    ("sae_attn_route", FWD, PLAIN, 1, dict(Nq=50, Nk=50, D=129), "head_dim 129 > 128 is not supported"),
    ("sae_th_attn_route", FWD, PLAIN, 1, dict(Nq=50, Nk=50, D=48, H=17),
     "talking heads needs heads <= 16 and head_dim <= 64"),
    ("sae_th_attn_route", BWD, PLAIN, 1, dict(Nq=50, Nk=50, D=48, H=9, dtype=F32),
     "talking heads: 9 heads > 8 on the fp32 / unaligned path"),
    ("sae_th_attn_route", FWD, ROT, 1, dict(Nq=50, Nk=50, D=48, H=8, dtype=F32),
     "rotary: fused only on the bf16 talking-heads path (aligned strides)"),
    ("sae_th_attn_route", BWD, ROT, 0, dict(Nq=50, Nk=50, D=48, H=8),
     "rotary: fused only on the bf16 talking-heads path (aligned strides)"),
    ("sae_th_attn_route", FWD, PLAIN, 1, dict(Nq=49, Nk=49, D=48, grid=(7, 7)), "talking heads takes no flags"),
]


@pytest.mark.parametrize("fn,pas,form,aligned,kw,text", REFUSALS)
def test_route_refusals(lib, fn, pas, form, aligned, kw, text):
    assert _route(lib, fn, _desc(lib, **kw), pas, form, aligned) is None
    assert lib.sae_last_error().decode().startswith(text)
