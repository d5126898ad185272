"""Stress inputs for the fused relative-logit kernels and the talking-heads kernels, with the
float64 references and two arithmetic emulations (numpy only: no GPU import).

Relative logits (``relpos_pair_case`` / ``relpos_chain_case``): inputs for which every rounding
inside the bf16 kernels is exact, so the bf16 path is held to the fp32 bar and an index slip on one
row, column or tile edge moves a result by O(1).  ``relpos_rounded_bwd`` is the backward with the
kernels' bf16 operands (dS for every gradient, P for dV) -- it must still equal float64.

Talking heads (``th_spike_case``): the spike inputs of ``test_softmax_spike`` under transforms of
gain ``tg``.  ``th_emulate`` restates the arithmetic of ``csrc/th2.h`` (bf16) / ``th_kernels.h``
(fp32) so that the CPU guards (``test_stress_inputs_cpu.py``) can show each GPU case to be neither
satisfied nor failed by construction.
"""
import functools
import math

import numpy as np

import attention_ref as R

LN2 = math.log(2.0)
NEG = -64.0                      # every losing table entry; -64 / scale is exact in bf16 for scale 1, 0.25

# (Hs, Ws, D, mode)                                what it covers
RELPOS_GRIDS = [
    (7, 7, 32, "bf16"),        # lean 32-wide tiles
    (7, 7, 32, "f32"),         # v1 in fp32
    (5, 7, 64, "bf16"),        # lean 64-wide tiles; dK/dV pass at one wave per SIMD
    (16, 16, 16, "bf16"),      # rel_h + rel_w == 32: bit 31 of the one-hot mask, four full key tiles
    (1, 31, 32, "bf16"),       # rel_h = 1; ragged single tile
    (3, 29, 128, "bf16"),      # head dim 128 with Nk = 87 < 128: two-wave bwd2; last tile of 23 keys
    (14, 14, 128, "bf16"),     # the AGPR unit with relative logits
    (16, 17, 32, "bf16"),      # 33 columns: first grid past the lean limit -> bf16 v1 fallback, 272 keys
    (16, 17, 32, "f32"),
    (2, 64, 64, "bf16"),       # rel_w at the validated maximum
    (2, 64, 64, "f32"),
    (5, 7, 12, "bf16"),        # head dim not a multiple of 8: unaligned bf16 path with relative logits
]
RELPOS_SCALES = (1.0, 0.25)
RELPOS_HEADS = 2


def relpos_pairs(Hs, Ws):
    """The ``pair`` values a grid admits ("col" needs two key rows, "row" two key columns)."""
    return [p for p in ("row", "col") if (p == "row" and Ws > 1) or (p == "col" and Hs > 1)]


RELPOS_CASES = [(Hs, Ws, D, mode, pair, scale) for (Hs, Ws, D, mode) in RELPOS_GRIDS
                for pair in relpos_pairs(Hs, Ws) for scale in RELPOS_SCALES]


def relpos_shifts(Hs, Ws):
    """Target offsets at the row-wrap edges of the key grid (one batch entry each)."""
    N = Hs * Ws
    return [0, 1, Ws - 1, Ws, Ws + 1, N // 2, N - 1]


def relpos_pair_case(Hs, Ws, H, D, shifts, pair, seed=0):
    """Two winning keys per score row, in one key row (``pair="row"``) or one key column ("col").

    k = 0, q integers in [-2, 2], v integers in [1, 4]; the fp32 tables hold -64 except the zeros
    that select, for batch b (shift s), head h and query n, the key t = (n + s + 3 h) mod N and its
    right ("row") or lower ("col") neighbour, wrapping.  dout[b, n, h, (n + h) % D] = 2.  Then
    P = 1/2, 1/2, o = (v[t1] + v[t2]) / 2, lse = ln 2, dS = +-(v[t1] - v[t2]) / 2 at one head-dim
    column, dq = 0 and every gradient is a small dyadic number.  Returns float32 arrays plus the
    winner indices ``t1`` / ``t2`` [B, H, N]."""
    assert pair in relpos_pairs(Hs, Ws), (Hs, Ws, pair)
    N, B = Hs * Ws, len(shifts)
    rng = np.random.default_rng(seed)
    q = rng.integers(-2, 3, (B, N, H, D)).astype(np.float32)
    k = np.zeros((B, N, H, D), np.float32)
    v = rng.integers(1, 5, (B, N, H, D)).astype(np.float32)
    bh = np.full((B, H, N, Hs), NEG, np.float32)
    bw = np.full((B, H, N, Ws), NEG, np.float32)
    dout = np.zeros((B, N, H, D), np.float32)
    t1 = np.zeros((B, H, N), np.int64)
    t2 = np.zeros((B, H, N), np.int64)
    for b, s in enumerate(shifts):
        for h in range(H):
            for n in range(N):
                t = (n + s + 3 * h) % N
                x, y = divmod(t, Ws)
                bh[b, h, n, x] = 0.0
                bw[b, h, n, y] = 0.0
                if pair == "row":
                    y2 = (y + 1) % Ws
                    bw[b, h, n, y2] = 0.0
                    u = x * Ws + y2
                else:
                    x2 = (x + 1) % Hs
                    bh[b, h, n, x2] = 0.0
                    u = x2 * Ws + y
                t1[b, h, n], t2[b, h, n] = t, u
                dout[b, n, h, (n + h) % D] = 2.0
    return dict(q=q, k=k, v=v, bh=bh, bw=bw, dout=dout, t1=t1, t2=t2, grid=(Hs, Ws))


def relpos_full_bias(bh, bw, Ws):
    """[B, H, N, Nk] logits of the two tables: R[q, k] = bh[q, k // Ws] + bw[q, k % Ws]."""
    Nk = bh.shape[-1] * Ws
    kk = np.arange(Nk)
    return np.asarray(bh, np.float64)[..., kk // Ws] + np.asarray(bw, np.float64)[..., kk % Ws]


def relpos_fold(dbias, Hs, Ws):
    """dbias [B, H, N, Nk] summed over key columns / key rows -> (dbias_h, dbias_w)."""
    d = dbias.reshape(dbias.shape[:-1] + (Hs, Ws))
    return d.sum(-1), d.sum(-2)


def relpos_reference(c, scale):
    """float64 truth of a pair case: o, lse and every gradient (dbias folded to the tables)."""
    Hs, Ws = c["grid"]
    full = relpos_full_bias(c["bh"], c["bw"], Ws)
    o, aux = R.attention_core_fwd(c["q"], c["k"], c["v"], "f64", scale=scale, bias=full, return_aux=True)
    g = R.attention_core_bwd(c["q"], c["k"], c["v"], c["dout"], scale=scale, bias=full)
    dbh, dbw = relpos_fold(g["dbias"], Hs, Ws)
    return dict(o=o, lse=aux["lse"], dq=g["dq"], dk=g["dk"], dv=g["dv"], dbh=dbh, dbw=dbw)


@functools.lru_cache(maxsize=None)
def relpos_case_and_reference(Hs, Ws, D, pair, scale):
    """One (inputs, float64 reference) per case, shared by the dtypes and the tests; read-only."""
    c = relpos_pair_case(Hs, Ws, RELPOS_HEADS, D, relpos_shifts(Hs, Ws), pair)
    ref = relpos_reference(c, scale)
    for a in list(c.values()) + list(ref.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c, ref


def _rb(x):
    """bf16 rounding of float32-representable values, returned as float64."""
    return R.round_bf16(np.asarray(x, np.float32)).astype(np.float64)


def relpos_rounded_bwd(c, scale):
    """Emulation 1 -- the backward with the bf16 kernels' operand roundings: dS rounded to bf16 for
    every gradient it feeds (dq, dk, dbias), P rounded to bf16 for dv; float64 sums."""
    Hs, Ws = c["grid"]
    q, k, v, do = (np.asarray(c[n], np.float64) for n in ("q", "k", "v", "dout"))
    s = scale * np.einsum("bqhd,bkhd->bhqk", q, k) + relpos_full_bias(c["bh"], c["bw"], Ws)
    e = np.exp(s - s.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    dp = np.einsum("bqhd,bkhd->bhqk", do, v)
    ds = _rb(p * (dp - (dp * p).sum(-1, keepdims=True)))
    dbh, dbw = relpos_fold(ds, Hs, Ws)
    return dict(dq=scale * np.einsum("bhqk,bkhd->bqhd", ds, k), dk=scale * np.einsum("bhqk,bqhd->bkhd", ds, q),
                dv=np.einsum("bhqk,bqhd->bkhd", _rb(p), do), dbh=dbh, dbw=dbw)


def table_errs(dbh, dbw, ref_h, ref_w):
    """Max abs error of each table over the larger of the two reference maxima (one of the two
    tables is ~0 by construction, so each cannot be normalised by its own maximum)."""
    den = max(np.abs(ref_h).max(), np.abs(ref_w).max())
    return (float(np.abs(np.asarray(dbh, np.float64) - ref_h).max() / den),
            float(np.abs(np.asarray(dbw, np.float64) - ref_w).max() / den))


# ---------------------------------------------------------------- chained through relpos_bias
RELPOS_CHAIN_GRIDS = [(7, 7, 32), (14, 14, 128)]        # (Hs, Ws, D), bf16
RELPOS_CHAIN_OFFSETS = [(0, 0), (1, 0), (0, -1)]


def relpos_chain_case(Hs, Ws, H, D, dx, dy, B=2, seed=1):
    """Inputs whose relative logits, built by the table kernel from embeddings, select key
    (x + dx, y + dy) for query (x, y): qhat[..., 0] = 1 and integers elsewhere, k = 0,
    emb_h[m, 0] = 0 at m = Hs - 1 + dx and -64 elsewhere (emb_w with dy), other embedding columns 0.
    ``target`` [N] is the winning key, ``inside`` [N] whether it lies in the grid (the other rows
    average a whole key row or column and are not exact)."""
    N = Hs * Ws
    rng = np.random.default_rng(seed)
    qhat = rng.integers(-2, 3, (B, N, H, D)).astype(np.float32)
    qhat[..., 0] = 1.0
    k = np.zeros((B, N, H, D), np.float32)
    v = rng.integers(1, 5, (B, N, H, D)).astype(np.float32)
    eh = np.zeros((2 * Hs - 1, D), np.float32)
    ew = np.zeros((2 * Ws - 1, D), np.float32)
    eh[:, 0] = NEG
    ew[:, 0] = NEG
    eh[Hs - 1 + dx, 0] = 0.0
    ew[Ws - 1 + dy, 0] = 0.0
    xs, ys = np.arange(N) // Ws + dx, np.arange(N) % Ws + dy
    inside = (xs >= 0) & (xs < Hs) & (ys >= 0) & (ys < Ws)
    target = np.where(inside, xs * Ws + ys, 0)
    return dict(qhat=qhat, k=k, v=v, eh=eh, ew=ew, target=target, inside=inside, grid=(Hs, Ws))


# ------------------------------------------------------------------------------ talking heads
TH_VARIANTS = [(4, "bf16"), (12, "bf16"), (4, "f32")]   # K-stacked single-MFMA mix, high/low two-MFMA mix, th_kernels.h
TH_FWD = [(tg, gain) for tg in (1.0, 4.0) for gain in (0.05, 0.6, 2.0)] + [(1.0, 4.0)]
TH_BWD = [(1.0, 0.05), (1.0, 0.6), (1.0, 2.0), (1.0, 4.0), (4.0, 0.05)]


def _orth(rng, h):
    a = rng.standard_normal((h, h))
    qm, r = np.linalg.qr(a)
    return (qm * np.sign(np.diag(r))).astype(np.float32)


def _randn(rng, shape, mode):
    x = rng.standard_normal(shape).astype(np.float32)
    return R.round_bf16(x) if mode == "bf16" else x


def th_spike_case(H, tg, gain, mode, N=70, Nk=70, D=48, seed=5):
    """``test_softmax_spike``'s inputs (q, v ~ N(0, 1), k ~ 0.3 N(0, 1); for three queries a key in
    a late tile at +gain q and one in the first tile at -gain q, in every head) with orthogonal
    transforms scaled by ``tg``: peaked MIXED logits, large |T|."""
    rng = np.random.default_rng(seed)
    q = _randn(rng, (1, N, H, D), mode)
    k = _randn(rng, (1, Nk, H, D), mode) * 0.3
    v = _randn(rng, (1, Nk, H, D), mode)
    for qi in (7, 40, N - 1):
        k[0, Nk - 1 - qi // 2] = gain * q[0, qi]
        k[0, qi % 32] = -gain * q[0, qi]
    if mode == "bf16":
        k = R.round_bf16(k)
    th1 = (tg * _orth(np.random.default_rng(3), H)).astype(np.float32)
    th2 = (tg * _orth(np.random.default_rng(4), H)).astype(np.float32)
    do = _randn(np.random.default_rng(2), (1, N, H, D), mode)
    return dict(q=q, k=k, v=v, th1=th1, th2=th2, do=do)


@functools.lru_cache(maxsize=None)
def th_case_and_reference(H, tg, gain, mode):
    """(inputs, float64 forward and backward, forward bar) of one case; read-only.  The forward bar
    is ``test_softmax_spike``'s rule: at least as close to float64 as the reference's own program
    in that dtype (with its fp32 mixes), and never tighter than the dtype's tolerance."""
    from _util import TOL, rel_err
    c = th_spike_case(H, tg, gain, mode)
    o64 = R.attention_core_fwd(c["q"], c["k"], c["v"], "f64", th1=c["th1"], th2=c["th2"])
    own = R.attention_core_fwd(c["q"], c["k"], c["v"], mode, th1=c["th1"], th2=c["th2"])
    g = R.attention_core_bwd(c["q"], c["k"], c["v"], c["do"], th1=c["th1"], th2=c["th2"])
    ref = dict(o=o64, fwd_bar=max(TOL[mode], rel_err(own, o64)), **g)
    for a in list(c.values()) + list(ref.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c, ref


def th_emulate(c, mode, backward=True):
    """Emulation 2 -- the talking-heads kernels' arithmetic in float32 numpy.

    bf16 (``csrc/th2.h``): the scores scale * (q k^T) rounded to bf16 into the exchange image; each
    transform as a bf16 high + low pair (~16 bits; T1 times log2 e before the split in the forward,
    so the mixed logits are in the log2 domain); fp32 softmax; P rounded to bf16 as the second
    mix's operand; P2 rounded to bf16 as the P V operand; bf16 output.  Backward: dP2 = dO V^T and
    dS1 rounded to bf16 into the images, delta from the fp32 P, dT2 from bf16 P and dP2, dT1 from the
    bf16 scores and dS1, dS = T1 dS1 rounded to bf16 for dQ / dK, bf16 P2 for dV, bf16 gradients.
    fp32 (``th_kernels.h``): the same program with no rounding."""
    f32 = np.float32
    rb = (lambda x: R.round_bf16(np.asarray(x, f32))) if mode == "bf16" else (lambda x: np.asarray(x, f32))

    def split16(t):
        t = np.asarray(t, f32)
        if mode != "bf16":
            return t
        hi = R.round_bf16(t)
        return hi + R.round_bf16(t - hi)

    q, k, v = (np.asarray(c[n], f32) for n in ("q", "k", "v"))
    th1, th2 = np.asarray(c["th1"], f32), np.asarray(c["th2"], f32)
    scale = f32(1.0 / math.sqrt(q.shape[-1]))
    s = rb(np.einsum("bqhd,bkhd->bhqk", q, k) * scale)
    s1 = np.einsum("hi,bhqk->biqk", split16(th1 * f32(math.log2(math.e))), s)     # log2 domain
    m = s1.max(-1, keepdims=True)
    lse2 = m + np.log2(np.exp2(s1 - m).sum(-1, keepdims=True, dtype=f32))
    p = np.exp2(s1 - lse2)
    pb = rb(p)
    t2 = split16(th2)
    p2 = rb(np.einsum("hi,bhqk->biqk", t2, pb))
    out = dict(o=rb(np.einsum("bhqk,bkhd->bqhd", p2, v)), lse=(lse2 * f32(LN2)).squeeze(-1))
    if not backward:
        return out
    do = np.asarray(c["do"], f32)
    dp2 = rb(np.einsum("bqhd,bkhd->bhqk", do, v))
    dp = np.einsum("hi,biqk->bhqk", t2, dp2)
    delta = (p * dp).sum(-1, keepdims=True, dtype=f32)
    ds1 = rb(p * (dp - delta))
    ds = rb(np.einsum("hi,biqk->bhqk", split16(th1), ds1))
    out.update(dth2=np.einsum("bhqk,biqk->hi", pb, dp2), dth1=np.einsum("bhqk,biqk->hi", s, ds1),
               dq=rb(np.einsum("bhqk,bkhd->bqhd", ds, k) * scale), dk=rb(np.einsum("bhqk,bqhd->bkhd", ds, q) * scale),
               dv=rb(np.einsum("bhqk,bqhd->bkhd", p2, do)))
    return out
