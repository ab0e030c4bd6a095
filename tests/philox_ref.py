"""Pure-numpy Philox4x32-10 and the dropout mask the library's descriptor (seed, offset, p) stands for.

The definition (include/matgcn.h, "device-side dropout"): key = (lo32(seed), hi32(seed)); counter = (lo32(q), hi32(q),
lo32(offset), hi32(offset)) with q = idx >> 2 and idx = ((b*headT + t)*N + n)*64 + h the element's position in the logical
(B, headT, N, 64) mask; output word idx & 3 decides element idx: kept iff word >= floor((double)p * 2^32); a kept element is
multiplied by (float)(1 / (1 - (double)p)), a dropped one by 0.  Nothing here looks at the library.
"""
import math

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
LO = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: (..., 4) unsigned 32-bit words, key: two 32-bit words -> (..., 4) uint32 (Random123 order)"""
    c = np.asarray(counter, dtype=np.uint64) & LO
    c0, c1, c2, c3 = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                     # 32 x 32 -> 64 bits: no overflow in uint64
        n0 = (p1 >> S32) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> S32) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & LO, n2, p0 & LO
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def threshold(p) -> int:
    return int(math.floor(float(np.float32(p)) * 4294967296.0))


def keep_scale(p) -> np.float32:
    return np.float32(1.0 / (1.0 - float(np.float32(p))))


def keep_bits(batch, head_steps, nodes, seed, offset, p) -> np.ndarray:
    """(B, headT, N, 64) bool: which elements of the mask are kept"""
    quads = batch * head_steps * nodes * 16
    q = np.arange(quads, dtype=np.uint64)
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    ctr = np.stack([q & LO, q >> S32, np.full(quads, offset & 0xFFFFFFFF, dtype=np.uint64),
                    np.full(quads, offset >> 32, dtype=np.uint64)], -1)
    words = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    return (words >= np.uint32(threshold(p))).reshape(batch, head_steps, nodes, 64)


def mask(batch, head_steps, nodes, seed, offset, p) -> np.ndarray:
    """(B, headT, N, 64) float32 multipliers: 0 or 1/(1-p)"""
    keep = keep_bits(batch, head_steps, nodes, seed, offset, p)
    return np.where(keep, keep_scale(p), np.float32(0.0)).astype(np.float32)
