"""Exact-arithmetic check of the relative-logit indexing INSIDE the attention kernels.

``test_relpos_index_map_exact`` proves the index map of the standalone table kernel only; the
kernels that consume the tables redo ``bias_h[q][k // Ws] + bias_w[q][k % Ws]`` themselves -- as
one-hot key rows on the MFMA (``fwd2`` / ``bwd2`` / ``bwd_agpr``: ``rel_onehot8``, ``rel_qrow8``,
``rel_put_onehot``) or per score with ``(key * rel_magic) >> 20`` (v1) -- and random inputs at the
2e-2 bf16 bar would not see a slip on one row or column of one tile edge.  The inputs of
``_stress.relpos_pair_case`` make every rounding of the bf16 kernels exact (two winning keys per
row with P = 1/2 each, integer v, k = 0, table entries 0 / -64, power-of-two scales), so bf16 and
fp32 are both held to the fp32 bar ``TOL["f32"] = 1e-5`` against float64 and an index slip moves a
result by O(1).  ``test_stress_inputs_cpu.py`` shows on the CPU that the bar is reachable.

Measured worst errors on an MI355X (every bar is 1e-5; o and dq are exact in every case):
  lean bf16 (fwd2 / bwd2 / bwd_agpr: 7x7, 5x7 D 64, 16x16, 1x31, 3x29, 14x14)
      lse 1.9e-9, dk 2.0e-8, dv 4.9e-31, dbias_h / dbias_w 4.0e-8
  bf16 v1 (16x17, 2x64, 5x7 at D 12)     lse 1.9e-9, dk 2.0e-8, dv 1.5e-30, dbias 7.8e-27
  fp32 v1 (7x7, 16x17, 2x64)             lse 1.9e-9, dk 3.2e-28, dv 4.0e-34, dbias 7.8e-27
  chained through relpos_bias            o exact (0) for all six cases
(1.9e-9 is fp32 ln 2; 2.0e-8 / 4.0e-8 the fp32 round trip of lse through log2 e in the backward's
P = 2^(S - lse).)  Tried once against a scratch build with bit 31 of the one-hot mask dropped in
``rel_onehot8``: the 16x16, 1x31 and 3x29 cases (all Hs + Ws = 32) fail here while
``test_botnet_relpos``, ``test_botmhsa_module`` and the golden fixtures still pass.
"""
import numpy as np
import pytest

import _stress as S
from _util import TOL, rel_err, to_np

pytestmark = pytest.mark.gpu

BAR = TOL["f32"]


def _td(mode):
    import torch
    return torch.bfloat16 if mode == "bf16" else torch.float32


@pytest.mark.parametrize("Hs,Ws,D,mode,pair,scale", S.RELPOS_CASES)
def test_relpos_pair_exact(dev, Hs, Ws, D, mode, pair, scale):
    import torch
    import sae_vision_amd.ops as ops

    c, ref = S.relpos_case_and_reference(Hs, Ws, D, pair, scale)
    td = _td(mode)
    tq, tk, tv = (torch.tensor(c[n], device=dev, dtype=td, requires_grad=True) for n in ("q", "k", "v"))
    bh, bw = (torch.tensor(c[n], device=dev, requires_grad=True) for n in ("bh", "bw"))
    o = ops.attention(tq, tk, tv, scale=scale, bias=(bh, bw, (Hs, Ws)))
    o.backward(torch.tensor(c["dout"], device=dev, dtype=td))
    with torch.no_grad():
        _, lse = ops._fwd(tq, tk, tv, scale, bh, bw, (Hs, Ws))
    torch.cuda.synchronize()

    e_h, e_w = S.table_errs(to_np(bh.grad), to_np(bw.grad), ref["dbh"], ref["dbw"])
    errs = dict(o=rel_err(o, ref["o"]), lse=float(np.abs(to_np(lse) - S.LN2).max()),
                dq=float(np.abs(to_np(tq.grad)).max()), dk=rel_err(tk.grad, ref["dk"]),
                dv=rel_err(tv.grad, ref["dv"]), dbias_h=e_h, dbias_w=e_w)
    print(f"relpos pair {Hs}x{Ws} D{D} {mode} {pair} scale {scale}: " +
          " ".join(f"{n} {x:.2e}" for n, x in errs.items()))
    assert errs["o"] <= BAR
    assert errs["lse"] <= BAR
    assert errs["dq"] == 0
    for n in ("dk", "dv", "dbias_h", "dbias_w"):
        assert errs[n] <= BAR, f"{n}: {errs[n]:.3e}"


@pytest.mark.parametrize("Hs,Ws,D", S.RELPOS_CHAIN_GRIDS)
@pytest.mark.parametrize("dx,dy", S.RELPOS_CHAIN_OFFSETS)
def test_relpos_chain_exact(dev, Hs, Ws, D, dx, dy):
    """Tables from ``ops.relpos_bias`` (embeddings that select relative offset (dx, dy)) into the
    fused kernels: query (x, y) returns v of key (x + dx, y + dy) wherever that key exists."""
    import torch
    import sae_vision_amd.ops as ops

    c = S.relpos_chain_case(Hs, Ws, S.RELPOS_HEADS, D, dx, dy)
    tq, tk, tv = (torch.tensor(c[n], device=dev, dtype=torch.bfloat16) for n in ("qhat", "k", "v"))
    teh, tew = (torch.tensor(c[n], device=dev) for n in ("eh", "ew"))
    bh, bw = ops.relpos_bias(tq, teh, tew, (Hs, Ws))
    o = to_np(ops.attention(tq, tk, tv, scale=1.0, bias=(bh, bw, (Hs, Ws))))
    ins = c["inside"]
    err = rel_err(o[:, ins], c["v"][:, c["target"][ins]])
    print(f"relpos chain {Hs}x{Ws} D{D} ({dx},{dy}): o {err:.2e}")
    assert err <= BAR
