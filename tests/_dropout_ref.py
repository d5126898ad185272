"""Reference of the attention-probability dropout (include/sae_attn.h, csrc/dropout.h) in numpy:
Philox4x32-10, the keep mask as a pure function of (seed, offset, stream_id, b, h, q, k), and the
fp64 forward / backward of the attention core with a given mask."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
U32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Random123's Philox4x32-10 on arrays: ``ctr`` 4 and ``key`` 2 broadcastable uint32 arrays (or
    ints); returns the 4 output words as uint64 arrays holding 32-bit values."""
    c = [np.asarray(x, dtype=np.uint64) & U32 for x in ctr]
    k = [np.asarray(x, dtype=np.uint64) & U32 for x in key]
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & U32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & U32]
        k = [(k[0] + np.uint64(W0)) & U32, (k[1] + np.uint64(W1)) & U32]
    return c


def threshold(rate):
    """T = clamp(lrintf(rate * 256), 0, 255) (round half to even, in fp32) and pk = (256 - T) / 256."""
    t = int(np.clip(np.rint(np.float32(rate) * np.float32(256.0)), 0, 255))
    return t, (256 - t) / 256.0


def keep_mask(B, H, Nq, Nk, rate, seed, offset, stream_id):
    """bool keep[B, H, Nq, Nk] by the definition in sae_attn.h."""
    t, _ = threshold(rate)
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    k0, k1 = philox4x32_10((offset & U32, offset >> 32, stream_id, 0), (seed & U32, seed >> 32))[:2]
    kb = np.arange((Nk + 3) // 4, dtype=np.uint64)[None, None, :]
    qb = np.arange((Nq + 3) // 4, dtype=np.uint64)[None, :, None]
    bh = np.arange(B * H, dtype=np.uint64)[:, None, None]
    w = np.stack(philox4x32_10((kb, qb, bh, 0), (k0, k1)), axis=-1)          # [BH, Qb, Kb, word = q & 3]
    sh = (np.uint64(8) * np.arange(4, dtype=np.uint64))
    byte = (w[..., None] >> sh) & np.uint64(0xFF)                             # [BH, Qb, Kb, q & 3, k & 3]
    keep = (byte >= t).transpose(0, 1, 3, 2, 4).reshape(B * H, 4 * qb.shape[1], 4 * kb.shape[2])
    return np.ascontiguousarray(keep[:, :Nq, :Nk]).reshape(B, H, Nq, Nk)


def probs(q, k, scale=None):
    """fp64 softmax(scale q k^T) [B, H, Nq, Nk] and its log-sum-exp [B, H, Nq] (q, k token-major [B, N, H, D])."""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    scale = 1.0 / np.sqrt(q.shape[-1]) if scale is None else scale
    s = scale * np.einsum("bqhd,bkhd->bhqk", q, k)
    mx = s.max(-1, keepdims=True)
    e = np.exp(s - mx)
    l = e.sum(-1, keepdims=True)
    return e / l, (mx + np.log(l))[..., 0]


def fwd(q, k, v, keep, rate, scale=None):
    """o = (P o m) v with m = keep / pk; returns (o [B, Nq, H, D], lse of the undropped scores)."""
    _, pk = threshold(rate)
    p, lse = probs(q, k, scale)
    return np.einsum("bhqk,bkhd->bqhd", p * (keep / pk), np.asarray(v, np.float64)), lse


def bwd(q, k, v, do, keep, rate, scale=None):
    """dV = (P o m)^T dO, dS = P o (m o (dO V^T) - delta), delta = rowsum(dO o O), dQ = scale dS K,
    dK = scale dS^T Q."""
    q, k, v, do = (np.asarray(x, np.float64) for x in (q, k, v, do))
    scale = 1.0 / np.sqrt(q.shape[-1]) if scale is None else scale
    _, pk = threshold(rate)
    m = keep / pk
    p, _ = probs(q, k, scale)
    o = np.einsum("bhqk,bkhd->bqhd", p * m, v)
    dv = np.einsum("bhqk,bqhd->bkhd", p * m, do)
    dp = np.einsum("bqhd,bkhd->bhqk", do, v)
    delta = np.einsum("bqhd,bqhd->bhq", do, o)
    ds = p * (m * dp - delta[..., None])
    return {"dq": scale * np.einsum("bhqk,bkhd->bqhd", ds, k), "dk": scale * np.einsum("bhqk,bqhd->bkhd", ds, q),
            "dv": dv}
