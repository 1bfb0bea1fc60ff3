"""The dropout mask of the UNet restated in numpy (the definition of include/diffulab_hip.h, dl_dropout): Philox4x32-10 and
``keep_mask``.  Shared by the host tests, the GPU tests and tests/golden/make_unet_dropout_golden.py; nothing here imports the
package under test."""

from __future__ import annotations

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
SHIFT32 = np.uint64(32)

# the fixture's case (tests/golden/unet_dropout.npz)
FIXTURE_SEED, FIXTURE_STEP, FIXTURE_P = 1234, 0, 0.3


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two ints -> four uint32 arrays"""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & MASK32 for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]  # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> SHIFT32) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> SHIFT32) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def threshold(p: float) -> int:
    """T = floor(p * 65536 + 0.5): an element is dropped iff its 16-bit half is below T"""
    return int(np.floor(np.float64(p) * 65536.0 + 0.5))


def scale_of(p: float) -> np.float32:
    return np.float32(1.0 / (1.0 - np.float64(p)))


def halves(n: int, seed: int, step: int, site: int) -> np.ndarray:
    """the 16-bit half of each of the first n elements (uint32 array [n])"""
    ng = (n + 7) // 8
    g = np.arange(ng, dtype=np.uint64)
    w = philox4x32_10((g & MASK32, g >> SHIFT32, site, step & 0xFFFFFFFF), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    h = np.empty((ng, 8), dtype=np.uint32)
    for j in range(4):
        h[:, 2 * j] = w[j] & np.uint32(0xFFFF)
        h[:, 2 * j + 1] = w[j] >> np.uint32(16)
    return h.reshape(-1)[:n]


def keep_mask(rows: int, cols: int, seed: int, step: int, site: int, p: float) -> np.ndarray:
    """bool [rows, cols]: True where element i = row * cols + col is kept"""
    return (halves(rows * cols, seed, step, site) >= threshold(p)).reshape(rows, cols)
