"""The Dense plans (ops.dense_fwd_plan / dense_bwd_plan) on the pinned rows of tests/_dense_rows.py: pure
functions of a call's facts, so no device is needed.  tests/test_gpu_dense_routes.py runs the same calls on
the GPU and asserts the launches."""
import pytest
import torch

import _dense_rows as D
import sae_vision_amd.ops as ops

DX = {"f32", "nt", "dw_t", "lib"}
DW = {"f32", "dw_blocks_sunk", "dw_blocks", "dw_sunk", "dw", "dw_stacked", "lib"}


@pytest.mark.parametrize("kw,gemm_lib,fwd,bwd", [r[1:] for r in D.ROWS], ids=[r[0] for r in D.ROWS])
def test_dense_plan(kw, gemm_lib, fwd, bwd):
    f = D.facts(kw, gemm_lib)
    assert ops.dense_fwd_plan(f) == fwd
    assert ops.dense_bwd_plan(f) == bwd


def test_every_route_is_pinned():
    assert {fwd[0] for *_, fwd, _ in D.ROWS} == {"f32", "nt", "lib"}
    assert {bwd[0] for *_, bwd in D.ROWS} == DX == set(ops._DX)
    assert {bwd[1] for *_, bwd in D.ROWS} == DW == set(ops._DW)


def test_wt_is_kept_exactly_for_dw_t():
    """The forward saves the bf16 W^T on exactly the rows whose input gradient reads it."""
    for name, kw, gemm_lib, *_ in D.ROWS:
        f = D.facts(kw, gemm_lib)
        assert ops.dense_fwd_plan(f)[1] == (ops.dense_bwd_plan(f)[0] == "dw_t"), name
    assert any(fwd[1] for *_, fwd, _ in D.ROWS)


def test_facts_read_the_switch_when_built():
    old = ops.GEMM_LIB
    try:
        ops.GEMM_LIB = True
        assert ops.dense_facts_of_shapes(64, 64, (64,)).gemm_lib
    finally:
        ops.GEMM_LIB = old
    assert not ops.dense_facts_of_shapes(64, 64, (64,)).gemm_lib


def test_facts_from_cpu_tensors_plan_the_library():
    """The tensor constructor on CPU operands (what tests/test_dense_cpu.py runs): every layout check is
    false off the GPU, so all three products go to the library."""
    x2, wd = torch.zeros(16, 64, dtype=torch.bfloat16), torch.zeros(64, 64, dtype=torch.bfloat16)
    f = ops._dense_facts(x2, wd, None, True, [None], None, (64,))
    assert (f.M, f.I, f.widths, f.dtype, f.on_gpu) == (16, 64, (64,), torch.bfloat16, False)
    assert ops.dense_fwd_plan(f) == ("lib", False) and ops.dense_bwd_plan(f) == ("lib", "lib", False)
