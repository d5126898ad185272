"""The route x layout matrix on the GPU: every attention route (``test_layouts_cpu.CASES``: one
case per row of the kernel instance tables and per pinned v1 instance) under every layout of
``_layouts.py`` that the route accepts -- distinct strides for all eight tensors, k / v and dk / dv
interleaved, head-major buffers, base pointers one element off a 16-byte boundary, a token stride
that is no whole number of 16-byte chunks -- with a caller-owned, strided ``o``.

Each test is one forward and one backward through the C entry points and asserts
  * parity of o, lse, dq, dk, dv (and dbias_h / dbias_w, dth1 / dth2) with the float64 oracle at the
    project's ``TOL`` (fp32 1e-5, bf16 2e-2; lse at the atol of ``test_lse_matches_oracle``), the same
    for every layout, and for the contiguous control run too;
  * bit identity with the control run wherever the layout's route is the control's: strides change
    addresses only and the kernels are deterministic, so this is exact;
  * that every element of every arena outside the tensors still carries the sentinel after each call
    (a wrong store bound or a swapped stride lands in a guard);
  * nothing of the result depends on bytes outside the tensors: the arenas are NaN wherever no tensor
    element lives (the control's too, before and after each tensor), so a padding row or column that
    reaches a result through a multiply in place of a select fails the parity check.

The control of a case runs once; the backward of every layout takes the control's o and lse.

Measured on an MI355X (45 controls + 201 case x layout pairs, 4.4 s for the file): every assertion
holds on the kernels as they are.  Worst errors -- bf16 0.0113 (dq, talking heads H 4 D 32), bf16 lse
0.0080 (talking heads with rotary, H 8 D 56), fp32 1.4e-6 (dq, D 128), fp32 lse 7.7e-7; the scalar
layouts stay below the vector ones (bf16 talking heads H 8 D 64: dk 2.7e-3 scalar, 7.0e-3 vector)."""
import math

import numpy as np
import pytest

import _dropout_ref as DR
import _layouts as Y
import attention_ref as R
from _util import TOL, randn, rel_err, to_np
from test_layouts_cpu import CASE_IDS, CASES

pytestmark = pytest.mark.gpu

SEED = 1234
LSE_ATOL = {"f32": 1e-4, "bf16": 2e-2}     # test_gpu_core.py::test_lse_matches_oracle
GPU_MATRIX = [(c, lay) for c in CASES for lay in Y.gpu_layouts(c)]
GPU_IDS = [f"{c.id}-{lay}" for c, lay in GPU_MATRIX]

_CONTEXT = {}   # case id -> inputs, side tensors and the float64 reference
_CONTROL = {}   # case id -> outputs of the contiguous run (or the exception it raised)


class _Ctx:
    pass


def _context(case, dev):
    """Inputs, the contiguous side tensors (relative tables, rotary tables, dropout state, transforms)
    and the float64 reference of ``case``: made once."""
    import torch
    import sae_vision_amd.ops as ops
    if case.id in _CONTEXT:
        return _CONTEXT[case.id]
    x = _Ctx()
    B, Nq, Nk, H, D, mode = case.B, case.Nq, case.Nk, case.H, case.D, case.dtype
    rng = np.random.default_rng(0)
    x.vals = {n: randn(rng, case.shape(n), mode) for n in ("q", "k", "v")}
    x.vals["dout"] = randn(np.random.default_rng(2), case.shape("dout"), mode)
    q, k, v, do = (x.vals[n] for n in ("q", "k", "v", "dout"))
    x.scale = 1.0 / math.sqrt(D)
    x.bias = x.rope = x.drop = x.th = None
    qr, kr, s, c = q, k, None, None
    if case.form == Y.ROT:
        n = max(Nq, Nk)
        x.rope = ops.rotary_tables(n, D, dev, Y.ROPE_BASE)
        s, c = R.rotary_sincos(n, D, Y.ROPE_BASE)
        qr = R.apply_rotary(q.astype(np.float64), s[:Nq], c[:Nq])
        kr = R.apply_rotary(k.astype(np.float64), s[:Nk], c[:Nk])
    if case.kind == "drop":
        state = ops.DropoutRng(SEED, dev)
        x.drop = (Y.DROP_RATE, state.state, 0)
        keep = ops.dropout_mask(B, H, Nq, Nk, Y.DROP_RATE, state, 0).cpu().numpy().astype(bool)
        o, lse = DR.fwd(q, k, v, keep, Y.DROP_RATE)
        x.ref = dict(DR.bwd(q, k, v, do, keep, Y.DROP_RATE), o=o, lse=lse)
    else:
        kw = {}
        if case.kind == "rel":
            Hs, Ws = case.grid
            trng = np.random.default_rng(3)
            bh = (0.5 * trng.standard_normal((B, H, Nq, Hs))).astype(np.float32)
            bw = (0.5 * trng.standard_normal((B, H, Nq, Ws))).astype(np.float32)
            x.bias = tuple(torch.tensor(t, device=dev) for t in (bh, bw))
            key = np.arange(Nk)
            kw["bias"] = bh.astype(np.float64)[..., key // Ws] + bw.astype(np.float64)[..., key % Ws]
        if case.th:
            trng = np.random.default_rng(7)
            th1, th2 = (np.linalg.qr(trng.standard_normal((H, H)))[0].astype(np.float32) for _ in range(2))
            x.th = tuple(torch.tensor(t, device=dev) for t in (th1, th2))
            kw.update(th1=th1, th2=th2)
        o, aux = R.attention_core_fwd(qr, kr, v, "f64", return_aux=True, **kw)
        g = R.attention_core_bwd(qr, kr, v, do, **kw)
        x.ref = dict(o=o, lse=aux["lse"], dq=g["dq"], dk=g["dk"], dv=g["dv"])
        if case.form == Y.ROT:   # gradients of the un-rotated q / k
            x.ref["dq"] = R.apply_rotary(g["dq"], -s[:Nq], c[:Nq])
            x.ref["dk"] = R.apply_rotary(g["dk"], -s[:Nk], c[:Nk])
        if case.kind == "rel":
            db = g["dbias"].reshape(B, H, Nq, Hs, Ws)
            x.ref.update(dbias_h=db.sum(-1), dbias_w=db.sum(-2))
        if case.th:
            x.ref.update(dth1=g["dth1"], dth2=g["dth2"])
    _CONTEXT[case.id] = x
    return x


def _run(case, layout, dev, x, ctl=None):
    """One forward and one backward of ``case`` under ``layout``; the guards of every arena are checked
    after each.  The backward reads the control's o and lse (``ctl``; its own for the control itself).
    Returns name -> contiguous copy of every output."""
    import torch
    p = Y.plan(case, layout)
    arenas, t = Y.materialise(p, dev, x.vals)
    grid = case.grid
    if case.th:
        lse = Y.run_th_fwd(t, x.th[0], x.th[1], x.scale, rope=x.rope)
    else:
        lse = Y.run_fwd(t, x.scale, bias=x.bias, grid=grid, rope=x.rope, drop=x.drop)
    torch.cuda.synchronize()
    Y.check_outputs_guards(p, arenas, t, Y.TENSORS)
    out = {"o": t["o"].clone(memory_format=torch.contiguous_format), "lse": lse}
    if ctl is not None:
        t["o"].copy_(ctl["o"])
    lse_in = lse if ctl is None else ctl["lse"]
    if case.th:
        out["dth1"], out["dth2"] = Y.run_th_bwd(t, x.th[0], x.th[1], lse_in, x.scale, rope=x.rope)
    else:
        dbh, dbw = Y.run_bwd(t, lse_in, x.scale, bias=x.bias, grid=grid, rope=x.rope, drop=x.drop)
        if x.bias is not None:
            out["dbias_h"], out["dbias_w"] = dbh, dbw
    torch.cuda.synchronize()
    Y.check_outputs_guards(p, arenas, t, Y.TENSORS)
    for n in ("dq", "dk", "dv"):
        out[n] = t[n].clone(memory_format=torch.contiguous_format)
    return out


def _control(case, dev):
    if case.id not in _CONTROL:
        try:
            _CONTROL[case.id] = _run(case, "contig", dev, _context(case, dev))
        except BaseException as e:   # its layouts fail with the same finding, without a second run
            _CONTROL[case.id] = e
    if isinstance(_CONTROL[case.id], BaseException):
        raise _CONTROL[case.id]
    return _CONTROL[case.id]


def _assert_parity(case, layout, out, ref):
    assert set(out) == set(ref), (sorted(out), sorted(ref))
    errs = {n: float(np.abs(to_np(out[n]) - ref[n]).max()) if n == "lse" else rel_err(out[n], ref[n]) for n in ref}
    print(f"{case.id} / {layout}: " + " ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    for n, e in errs.items():
        bar = LSE_ATOL[case.dtype] if n == "lse" else TOL[case.dtype]
        assert e <= bar, f"{n}: {e:.3e} > {bar:g} (NaN: a result read bytes outside the tensors)"


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_control(dev, case):
    """The contiguous run of every case against the float64 oracle (for several rows of the instance
    tables the first parity run at all), its inputs NaN-guarded like the layouts'."""
    _assert_parity(case, "contig", _control(case, dev), _context(case, dev).ref)


@pytest.mark.parametrize("case,layout", GPU_MATRIX, ids=GPU_IDS)
def test_layout(dev, case, layout):
    import torch
    x = _context(case, dev)
    ctl = _control(case, dev)
    out = _run(case, layout, dev, x, ctl)
    _assert_parity(case, layout, out, x.ref)
    if Y.is_scalar(case, layout) == Y.is_scalar(case, "contig"):   # the control's route: bit for bit
        for n in sorted(out):
            assert torch.equal(out[n], ctl[n]), f"{n} differs from the contiguous run of the same kernels"
