"""Philox4x32-10 in NumPy (uint64 arithmetic) and the fp32 value maps of the device's random streams.

The library documents three streams (include/locator_hip.h, "the random streams"): every value is one word of
philox(ctr_lo, ctr_hi, key) with
    counter words (lo32(ctr_lo), hi32(ctr_lo), lo32(ctr_hi), hi32(ctr_hi)),  key words (lo32(key), hi32(key)),
multipliers 0xD2511F53 / 0xCD9E8D57, Weyl increments 0x9E3779B9 / 0xBB67AE85, ten rounds (Salmon et al., "Parallel random
numbers: as easy as 1, 2, 3", SC11; the known answers of the Random123 distribution are in tests/test_references.py).

Nothing here imports the library: tests/test_gpu_random.py compares the device with it bit for bit.  Every step of the value
maps is one correctly rounded fp32 operation (uint32 -> fp32 conversion, one addition, a scaling by 2^-32, `2 u` exact, one
subtraction, one product), so a fused multiply-add on the device cannot change a result and equality is the bar."""
import math

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
LO = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
MASK64 = (1 << 64) - 1
MASK_STREAM = 0x6d61736b        # "mask": ctr_hi of the Dropout keep-mask stream


def philox4x32_10_words(c, k):
    """c: four counter words, k: two key words (integers or arrays of them, each < 2^32) -> uint32 [..., 4]."""
    c0, c1, c2, c3 = (np.asarray(w, dtype=np.uint64) for w in c)
    k0, k1 = (np.asarray(w, dtype=np.uint64) for w in k)
    assert all(int(np.max(w)) <= 0xFFFFFFFF for w in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0 = M0 * c0                     # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = M1 * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & LO, (p0 >> S32) ^ c3 ^ k1, p0 & LO
        k0, k1 = (k0 + W0) & LO, (k1 + W1) & LO
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def philox(ctr_lo, ctr_hi, key):
    """64-bit counter halves and key (integers below 2^64, or uint64 arrays) -> uint32 [..., 4]."""
    lo, hi, key = (np.asarray(v, dtype=np.uint64) for v in (ctr_lo, ctr_hi, key))
    return philox4x32_10_words((lo & LO, lo >> S32, hi & LO, hi >> S32), (key & LO, key >> S32))


def stream_words(first, n, ctr_hi, key):
    """Elements first .. first + n of the flat stream whose element i is word i % 4 of philox(i // 4, ctr_hi, key)
    (first % 4 == 0) -> uint32 [n]."""
    assert first % 4 == 0 and n >= 0
    blocks = np.uint64(first // 4) + np.arange((n + 3) // 4, dtype=np.uint64)
    return philox(blocks, ctr_hi, key).reshape(-1)[:n]


# ---------------------------------------------------------------- value maps, fp32 step by step
def u01(r):
    """uint32 -> (float32(r) + 0.5f) * 2^-32, in (0, 1]: conversion and addition round to nearest even, the scaling is
    exact."""
    f = np.asarray(r, dtype=np.uint32).astype(np.float32)
    return (f + np.float32(0.5)) * np.float32(2.0 ** -32)


def uniform_pm(r, limit):
    """(2 u01(r) - 1) * float32(limit)."""
    return (np.float32(2.0) * u01(r) - np.float32(1.0)) * np.float32(limit)


def glorot_limit(R, C):
    """float32(sqrt(6 / (R + C))), the square root taken in double."""
    return np.float32(math.sqrt(6.0 / (float(R) + float(C))))


def init_uniform_ref(n, limit, seed, stream_id):
    """loc_init_uniform: element i = word i % 4 of philox(i // 4, stream_id, seed) -> float32 [n]."""
    return uniform_pm(stream_words(0, n, stream_id, seed), limit)


def glorot_ref(R, C, seed, stream_id):
    """loc_init_glorot: logical element (r, c) = word 0 of philox(r * C + c, stream_id, seed) -> float32 [R, C], whatever
    the storage layout."""
    ctr = np.arange(R * C, dtype=np.uint64)
    return uniform_pm(philox(ctr, stream_id, seed)[:, 0], glorot_limit(R, C)).reshape(R, C)


def dropout_threshold(p):
    """uint32(float64(float32(p)) * 2^32): the rate reaches the library as a C float."""
    return int(float(np.float32(p)) * 4294967296.0)


def dropout_mask_ref(n, p, seed, offset):
    """loc_dropout_mask_fill: mask[i] = keep flag of element offset + i of the ONE stream keyed by seed (ctr_hi "mask"):
    keep iff the word >= the threshold -> uint8 [n]."""
    words = stream_words(offset, n, MASK_STREAM, seed & MASK64)
    return (words >= np.uint32(dropout_threshold(p))).astype(np.uint8)
