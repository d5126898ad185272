"""CPU guards for the stress inputs of ``test_gpu_relpos_exact.py`` and ``test_gpu_th_stress.py``:
the GPU tests must be neither satisfiable nor unsatisfiable by construction.

* Relative logits: on every case the oracle's own program in the case's dtype equals float64
  within 1e-6 (so the fp32 bar is reachable in bf16), lse is ln 2, and the backward with the bf16
  kernels' operand roundings (``_stress.relpos_rounded_bwd``) still meets 1e-5.
* Talking heads: on every case the emulation of the kernels' documented arithmetic
  (``_stress.th_emulate``) meets the bar the GPU test applies to that case.

Emulation figures (CPU, not GPU measurements): talking-heads forward in bf16 <= 0.0161 at H 4
(tg 4, gain 2) and 0.0096 at H 12 against a bar of 0.02 on every case, fp32 <= 7.2e-7; backward
<= 0.0093 in bf16 and 3.1e-6 in fp32.  The GPU figures are in the two GPU modules' docstrings."""
import numpy as np
import pytest

import _stress as S
import attention_ref as R
from _util import TOL, rel_err


@pytest.mark.parametrize("Hs,Ws,D,mode,pair,scale", S.RELPOS_CASES)
def test_relpos_pair_inputs(Hs, Ws, D, mode, pair, scale):
    c, ref = S.relpos_case_and_reference(Hs, Ws, D, pair, scale)
    N = Hs * Ws
    # the construction: two winners per row, in one key row / one key column, wrapping
    full = S.relpos_full_bias(c["bh"], c["bw"], Ws)
    assert ((full == 0).sum(-1) == 2).all() and (full[full != 0] <= S.NEG).all()
    assert (np.take_along_axis(full, c["t1"][..., None], -1) == 0).all()
    assert (np.take_along_axis(full, c["t2"][..., None], -1) == 0).all()
    same = c["t1"] // Ws == c["t2"] // Ws if pair == "row" else c["t1"] % Ws == c["t2"] % Ws
    assert same.all() and (c["t1"] != c["t2"]).all()
    assert {int(t) for t in c["t1"][:, 0, 0]} == {s % N for s in S.relpos_shifts(Hs, Ws)}

    # what the inputs produce
    v = c["v"].astype(np.float64)
    bi, hi = np.arange(v.shape[0])[:, None, None], np.arange(v.shape[2])[None, :, None]
    o_exact = 0.5 * (v[bi, c["t1"], hi] + v[bi, c["t2"], hi]).transpose(0, 2, 1, 3)
    assert rel_err(ref["o"], o_exact) <= 1e-12
    assert np.abs(ref["lse"] - S.LN2).max() <= 1e-12
    assert not ref["dq"].any()
    assert np.abs(ref["dbh"] if pair == "row" else ref["dbw"]).max() <= 1e-20     # that table's sums cancel
    assert 0.5 <= max(np.abs(ref["dbh"]).max(), np.abs(ref["dbw"]).max()) <= 1.5
    assert 0 < np.abs(ref["dk"]).max() <= 6 and 0 < np.abs(ref["dv"]).max() <= 2 + 1e-9

    # the oracle's own program in this dtype: exact
    o_own, aux = R.attention_core_fwd(c["q"], c["k"], c["v"], mode, scale=scale, bias=full, return_aux=True)
    assert rel_err(o_own, ref["o"]) <= 1e-6
    assert np.abs(aux["lse"] - S.LN2).max() <= 1e-6

    # the kernels' bf16 operand roundings change nothing
    e = S.relpos_rounded_bwd(c, scale)
    assert not e["dq"].any()
    assert rel_err(e["dk"], ref["dk"]) <= 1e-5 and rel_err(e["dv"], ref["dv"]) <= 1e-5
    assert max(S.table_errs(e["dbh"], e["dbw"], ref["dbh"], ref["dbw"])) <= 1e-5
    # ... and every exact result is a bf16 value (the fp32 bar is reachable by a bf16 store)
    for n in ("dk", "dv"):
        assert rel_err(R.round_bf16(ref[n].astype(np.float32)), ref[n]) <= 1e-6, n
    assert rel_err(R.round_bf16(o_exact.astype(np.float32)), o_exact) == 0


@pytest.mark.parametrize("Hs,Ws,D", S.RELPOS_CHAIN_GRIDS)
@pytest.mark.parametrize("dx,dy", S.RELPOS_CHAIN_OFFSETS)
def test_relpos_chain_inputs(Hs, Ws, D, dx, dy):
    c = S.relpos_chain_case(Hs, Ws, S.RELPOS_HEADS, D, dx, dy)
    assert c["inside"].sum() == (Hs - abs(dx)) * (Ws - abs(dy))
    bh, bw = R.relpos_bias_tables(c["qhat"].astype(np.float64), c["eh"].astype(np.float64),
                                  c["ew"].astype(np.float64), Hs, Ws)
    full = S.relpos_full_bias(bh, bw, Ws)
    ins = c["inside"]
    assert (full[:, :, ins].argmax(-1) == c["target"][ins]).all()
    assert ((full[:, :, ins] == 0).sum(-1) == 1).all() and (full[full != 0] <= S.NEG).all()
    o = R.attention_core_fwd(c["qhat"], c["k"], c["v"], "bf16", scale=1.0, bias=full)
    assert rel_err(o[:, ins], c["v"][:, c["target"][ins]]) <= 1e-6


@pytest.mark.parametrize("H,mode", S.TH_VARIANTS)
@pytest.mark.parametrize("tg,gain", S.TH_FWD)
def test_th_spike_inputs(H, mode, tg, gain):
    c, ref = S.th_case_and_reference(H, tg, gain, mode)
    bwd = (tg, gain) in S.TH_BWD
    e = S.th_emulate(c, mode, backward=bwd)
    err = rel_err(e["o"], ref["o"])
    print(f"th emu H{H} {mode} tg{tg} gain{gain}: o {err:.3e} (bar {ref['fwd_bar']:.3e})", end="")
    assert err <= ref["fwd_bar"]
    if bwd:
        errs = {n: rel_err(e[n], ref[n]) for n in ("dq", "dk", "dv", "dth1", "dth2")}
        print("", {n: f"{x:.2e}" for n, x in errs.items()}, end="")
        assert max(errs.values()) <= TOL[mode], errs
    print()


def test_th_spike_is_peaked():
    """The inputs do what they are for: mixed logits far outside the unit-normal range of
    ``test_talking_heads`` and a softmax that saturates."""
    c, _ = S.th_case_and_reference(4, 4.0, 2.0, "bf16")
    _, aux = R.attention_core_fwd(c["q"], c["k"], c["v"], "f64", th1=c["th1"], th2=c["th2"], return_aux=True)
    print(f"|s1| max {np.abs(aux['s1']).max():.1f}, P max {aux['p'].max():.6f}")
    assert np.abs(aux["s1"]).max() > 50 and aux["p"].max() > 0.999      # (test_talking_heads: |s1| < 7)
    c, _ = S.th_case_and_reference(4, 1.0, 2.0, "bf16")
    _, aux = R.attention_core_fwd(c["q"], c["k"], c["v"], "f64", th1=c["th1"], th2=c["th2"], return_aux=True)
    assert aux["p"].max() > 0.999
