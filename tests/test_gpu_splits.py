"""The split-reduced gradient GEMMs on the GPU, bit for bit at every edge of their split plans:
``sae_gemm_dw`` / ``sae_gemm_dw_blocked`` (gemm_dw8_kernel<BIAS, NG> + gemm_dw_reduce_kernel) and the
split-K path of ``sae_gemm_f32`` (gemm_f32_kernel<AK, BK> + gemm_f32_reduce_kernel), called through
the C ABI with caller-owned strides and a caller-owned workspace (``_splits.py``; the tables and the
plan restatement are checked on the CPU by ``test_splits_cpu.py``).

Every exact case asserts, per call:
  1. the outputs are ``torch.equal`` to the integer reference (inputs are small integers, so fp32
     accumulation is exact in any order: no tolerance);
  2. the pad columns of dw / c and every guard of every arena still hold the NaN pattern, and no
     NaN reached an output (operands sit in the tightest legal allocation between NaN guards);
  3. in the workspace -- exactly ``*_workspace_bytes``, pre-filled with one int32 pattern -- exactly the
     plan's S partial planes (and S bias rows at the plan's bpart offset) lost the pattern: that pins
     S and NG from outside and proves every partial the reduce reads was written by a split;
  4. a second call on a workspace of seeded random bits gives the same bits.
Integer inputs never round; one Gaussian run per entry point keeps the project's fp32 bar
(``_util.TOL``) against the float64 product."""
import numpy as np
import pytest
import torch

import _splits as S
from _layouts import assert_guards_intact
from _util import TOL, rel_err

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------- sae_gemm_dw
# (the row is the bottom decorator, so it varies slowest: the variants of a row run back to back and
# share its operands and reference)
@pytest.mark.parametrize("with_db", [False, True], ids=["nodb", "db"])
@pytest.mark.parametrize("acc", [0, 1], ids=["write", "accumulate"])
@pytest.mark.parametrize("padded", [False, True], ids=["contig", "padded"])
@pytest.mark.parametrize("shape,claims", S.DW_ROWS, ids=[S.dw_id(r[0]) for r in S.DW_ROWS])
def test_gemm_dw_exact(dev, shape, claims, with_db, acc, padded):
    S.check_dw(dev, shape, with_db, acc, padded, claims=claims)


@pytest.mark.parametrize("acc", [0, 1], ids=["write", "accumulate"])
@pytest.mark.parametrize("shape,jblock", S.DW_BLOCKED, ids=[f"{S.dw_id(s)}_jb{jb}" for s, jb in S.DW_BLOCKED])
def test_gemm_dw_blocked_exact(dev, shape, jblock, acc):
    """dw in contiguous column blocks [J / jblock, I, jblock], each block against the reference (with
    db, padded operands)."""
    S.check_dw(dev, shape, True, acc, True, jblock=jblock)


def test_gemm_dw_gaussian(dev):
    """Rounding, which integers never exercise: Gaussian bf16 operands against the float64 product of
    the same bf16 values at the project's fp32 bar (NG 1, S 2, padded operands)."""
    M, I, J = S.DW_GAUSS
    rng = np.random.default_rng(5)
    x = torch.as_tensor(rng.standard_normal((M, I)).astype(np.float32)).to(torch.bfloat16)
    dy = torch.as_tensor(rng.standard_normal((M, J)).astype(np.float32)).to(torch.bfloat16)
    inp = S.DwInputs(x.float().numpy(), dy.float().numpy(), None, None, None, None)
    S.forget_operands()
    _, _, dw, db, _ = S.run_dw(dev, S.DW_GAUSS, inp, True, 0, True)
    S.forget_operands()
    assert rel_err(dw.view, x.double().numpy().T @ dy.double().numpy()) <= TOL["f32"]
    assert rel_err(db.view, dy.double().numpy().sum(0)) <= TOL["f32"]
    assert_guards_intact(dw.arena, dw.view)


# ------------------------------------------------------------------------------ sae_gemm_f32
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("with_colsum", [False, True], ids=["nocolsum", "colsum"])
@pytest.mark.parametrize("acc", [0, 1], ids=["write", "accumulate"])
@pytest.mark.parametrize("ldc_pad", [0, 4], ids=["ldcN", "ldcN4"])
@pytest.mark.parametrize("key,claims", S.F32_ROWS, ids=[S.f32_id(r[0]) for r in S.F32_ROWS])
def test_gemm_f32_exact(dev, key, claims, with_bias, with_colsum, acc, ldc_pad):
    S.check_f32(dev, key, with_bias, with_colsum, acc, ldc_pad, claims=claims)


def test_gemm_f32_gaussian(dev):
    """Gaussian fp32 operands through the split weight-gradient layout (S 2, ragged tiles and k tile,
    bias, the ones row, padded c) against the float64 product at the project's fp32 bar."""
    key = S.F32_GAUSS
    M, N, K = key[0]
    rng = np.random.default_rng(6)
    a, b = rng.standard_normal((M, K)).astype(np.float32), rng.standard_normal((K, N)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    inp = S.F32Inputs(a, b, None, bias, None, None, None)
    S.forget_operands()
    _, _, _, c, cs, _ = S.run_f32(dev, key, inp, True, True, 0, 4)
    S.forget_operands()
    assert rel_err(c.view, a.astype(np.float64) @ b.astype(np.float64) + bias) <= TOL["f32"]
    assert rel_err(cs.view, b.astype(np.float64).sum(0)) <= TOL["f32"]
    assert_guards_intact(c.arena, c.view)
