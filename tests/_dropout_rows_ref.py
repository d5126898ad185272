"""Reference of the hidden-state dropout (include/sae_attn.h, csrc/drop_rows.h) in numpy: the keep
mask of a row-major activation as a pure function of (seed, offset, stream_id, row, col)."""
import numpy as np

from _dropout_ref import U32, philox4x32_10, threshold


def call_key(seed, offset, stream_id):
    """(k0, k1) of one call: the attention mask's derivation (drop_key)."""
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    return philox4x32_10((offset & U32, offset >> 32, stream_id, 0), (seed & U32, seed >> 32))[:2]


def keep_rows(M, C, rate, seed, offset, stream_id, row0=0, row_step=1):
    """bool keep[M, C]: rows row0 + i * row_step (64-bit) of the mask, columns 0 .. C - 1."""
    t, _ = threshold(rate)
    k0, k1 = call_key(seed, offset, stream_id)
    rows = (np.uint64(int(row0) & (2 ** 64 - 1)) + np.arange(M, dtype=np.uint64) * np.uint64(row_step))[:, None]
    blk = np.arange((C + 15) // 16, dtype=np.uint64)[None, :]
    w = np.stack(philox4x32_10((blk, rows & np.uint64(U32), rows >> np.uint64(32), 1), (k0, k1)), axis=-1)
    sh = np.uint64(8) * np.arange(4, dtype=np.uint64)
    byte = (w[..., None] >> sh) & np.uint64(0xFF)           # [M, block, word = (col >> 2) & 3, byte = col & 3]
    return np.ascontiguousarray((byte >= t).reshape(M, -1)[:, :C])
