"""Host copy of the kernels' dropout stream (csrc/common.hip.h philox4x32 / philox_keep8), vectorised in numpy.

The kernels never store a dropout mask: every site regenerates it from (seed, site, element index).  This module computes the
same bits on the host so that the tests can (a) read a kernel's mask out of its output and compare it with an independent
derivation bit for bit, and (b) build fp64 references of the dropout-on paths with exactly the kernel's mask.

Philox4x32 with 7 rounds: counter = (idx lo, idx hi, site, 0x9E3779B9), key = the 64-bit seed (lo, hi), the key bumped by
(0x9E3779B9, 0xBB67AE85) after every round.  One call gives 4 x u32 = eight 16-bit slices (x lo, x hi, y lo, ... w hi); slice e
is element 8 idx + e, kept iff slice >= thr >> 16 with thr = drop_threshold(p).

Two element numberings:
  keep_rowmajor   element (m, n) of an [M, N] tensor is m N + n; groups of 8 may span rows.  The GEMM epilogues, the
                  LayerNorm forward / backward, row_normalize / row_apply_dropmask and the head's head_keep use it.
  keep_attention  attention_args.h attn_keep8: call ((bh Tq + i) NP + P) 4 + g covers query i and the keys 32 P + 4 g + r
                  (slices 0 - 3) and 32 P + 16 + 4 g + r (slices 4 - 7), NP = ceil(Tk / 32), bh = b heads + h.
"""
import numpy as np

from crct.lib import drop_threshold      # keep iff u32 >= thr; the kernels compare 16-bit slices with thr >> 16

PHILOX_ROUNDS = 7
_M32 = np.uint64(0xFFFFFFFF)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MUL0, _MUL1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)


def philox4x32(seed, site, idx, rounds=PHILOX_ROUNDS, counter_hi=(None, _W0)):
    """Four u32 words (each a uint64 array of idx's shape holding values < 2^32) of the Philox call at counter idx.
    rounds / counter_hi (words 2 and 3 of the counter; None = site) exist for the published test vectors only."""
    idx = np.asarray(idx, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w2, w3 = counter_hi
    c0 = idx & _M32
    c1 = idx >> np.uint64(32)
    c2 = np.full(idx.shape, (int(site) if w2 is None else w2) & 0xFFFFFFFF, dtype=np.uint64)
    c3 = np.full(idx.shape, w3, dtype=np.uint64)
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(rounds):
        p0 = c0 * _MUL0                   # < 2^64: exact in uint64
        p1 = c2 * _MUL1
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & _M32, n2, p0 & _M32
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def keep8(seed, site, idx8, p):
    """philox_keep8: bool [..., 8], element e of the call idx8 kept."""
    t = np.uint64(drop_threshold(p) >> 16)
    words = philox4x32(seed, site, idx8)
    sl = []
    for w in words:
        sl.append(w & np.uint64(0xFFFF))
        sl.append(w >> np.uint64(16))
    return np.stack(sl, axis=-1) >= t


def keep_rowmajor(seed, site, M, N, p):
    """bool [M, N]: element (m, n) = m N + n, group of 8 = (m N + n) >> 3."""
    total = int(M) * int(N)
    calls = np.arange((total + 7) // 8, dtype=np.uint64)
    return keep8(seed, site, calls, p).reshape(-1)[:total].reshape(int(M), int(N))


def keep_attention(seed, site, BH, Tq, Tk, p):
    """bool [BH, Tq, Tk]: the attention probabilities' mask of (batch * heads + head, query, key)."""
    NP = (int(Tk) + 31) // 32
    n = int(BH) * int(Tq) * NP * 4
    k = keep8(seed, site, np.arange(n, dtype=np.uint64), p)                    # [calls, 8]
    k = k.reshape(int(BH), int(Tq), NP, 4, 2, 4)                               # (.., P, g, slice >= 4, r)
    k = k.transpose(0, 1, 2, 4, 3, 5).reshape(int(BH), int(Tq), NP * 32)      # key 32 P + 16 hi + 4 g + r
    return np.ascontiguousarray(k[:, :, :int(Tk)])
