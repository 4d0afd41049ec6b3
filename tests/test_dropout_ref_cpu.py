"""The host copy of the dropout stream (tests/dropout_ref.py) on its own: the Philox round function against the published
Random123 known-answer vectors, determinism, keep rate, and the independence across seeds, sites, rows and heads that the GPU
tests rely on when they compare a kernel's mask with it.  CPU only."""
import math

import numpy as np

import dropout_ref as D
from crct import lib as L

SEED = (1 << 40) + 0x1234567        # the model's seeds reach 2^62


def _words(*a, **kw):
    return [int(w.reshape(-1)[0]) for w in D.philox4x32(*a, **kw)]


def test_philox_round_function_matches_the_published_vectors():
    # Random123 kat_vectors, philox4x32: (counter, key) -> output at 7 and 10 rounds.  The kernel's counter is
    # (idx lo, idx hi, site, 0x9E3779B9) and its key the seed (lo, hi)
    assert _words(0, 0, 0, rounds=7, counter_hi=(0, 0)) == [0x5f6fb709, 0x0d893f64, 0x4f121f81, 0x4f730a48]
    assert _words(0, 0, 0, rounds=10, counter_hi=(0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    pi = _words(0x299f31d0a4093822, 0, 0x85a308d3243f6a88, rounds=10, counter_hi=(0x13198a2e, 0x03707344))
    assert pi == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    # the default call IS that function with the kernel's counter words
    assert _words(SEED, 17, 12345) == _words(SEED, 0, 12345, counter_hi=(17, 0x9E3779B9))
    assert D.PHILOX_ROUNDS == 7


def test_keep8_slices_follow_the_threshold():
    idx = np.arange(4096, dtype=np.uint64)
    words = D.philox4x32(SEED, 3, idx)
    for p in (0.1, 0.5, 0.9):
        t = L.drop_threshold(p) >> 16
        k = D.keep8(SEED, 3, idx, p)
        for e in range(8):
            w = words[e // 2]
            sl = (w & np.uint64(0xFFFF)) if e % 2 == 0 else (w >> np.uint64(16))
            assert np.array_equal(k[:, e], sl >= np.uint64(t))
    assert D.keep8(SEED, 3, idx, 0.0).all()          # thr = 0: everything kept


def test_masks_are_deterministic():
    a = D.keep_rowmajor(SEED, 16, 37, 44, 0.1)
    assert np.array_equal(a, D.keep_rowmajor(SEED, 16, 37, 44, 0.1))
    b = D.keep_attention(SEED, 2, 6, 17, 45, 0.1)
    assert np.array_equal(b, D.keep_attention(SEED, 2, 6, 17, 45, 0.1))


def test_keep_rate_is_one_minus_the_threshold_within_binomial_error():
    for p in (0.1, 0.5):
        want = 1.0 - (L.drop_threshold(p) >> 16) / 65536.0
        for k in (D.keep_rowmajor(SEED, 1, 1000, 1001, p), D.keep_attention(SEED, 19, 64, 124, 124, p)):
            n = k.size
            assert abs(float(k.mean()) - want) < 5.0 * math.sqrt(want * (1 - want) / n), (p, k.shape)


def test_row_major_numbering_and_groups_spanning_rows():
    # M odd, N = 4 mod 8: the 8-element groups start mid-row; the [M, N] mask is the flat stream cut into rows
    M, N = 13, 36
    flat = D.keep8(SEED, 3, np.arange((M * N + 7) // 8, dtype=np.uint64), 0.5).reshape(-1)
    k = D.keep_rowmajor(SEED, 3, M, N, 0.5)
    assert np.array_equal(k.reshape(-1), flat[:M * N])
    assert np.array_equal(D.keep_rowmajor(SEED, 3, 1, M * N, 0.5).reshape(M, N), k)


def test_attention_numbering_follows_attn_keep8():
    BH, Tq, Tk, p = 3, 5, 70, 0.5
    k = D.keep_attention(SEED, 17, BH, Tq, Tk, p)
    NP = (Tk + 31) // 32
    for bh in range(BH):
        for i in range(Tq):
            for j in range(Tk):
                P, w = j // 32, j % 32
                call = ((bh * Tq + i) * NP + P) * 4 + (w % 16) // 4
                slice_ = 4 * (w // 16) + w % 4
                assert k[bh, i, j] == D.keep8(SEED, 17, np.array([call], dtype=np.uint64), p)[0, slice_]


def _differ(a, b):
    return float((a != b).mean())


def test_different_seed_site_pairs_give_different_masks():
    p = 0.5
    base = D.keep_rowmajor(SEED, 16, 64, 128, p)
    for seed, site in ((SEED + 1, 16), (SEED, 17), (SEED, 1), (SEED ^ (1 << 40), 16), (SEED + (1 << 32), 16), (SEED + (1 << 62), 16)):
        assert _differ(base, D.keep_rowmajor(seed, site, 64, 128, p)) > 0.4, (seed, site)     # independent masks differ in half


def test_seeds_above_two_to_the_32_change_the_mask():
    lo = SEED & 0xFFFFFFFF
    masks = [D.keep_rowmajor(lo | (hi << 32), 3, 32, 64, 0.5) for hi in (0, 1, 1 << 20, (1 << 30) - 1)]
    for i in range(len(masks)):
        for j in range(i):
            assert _differ(masks[i], masks[j]) > 0.4


def test_rows_and_heads_are_not_copies():
    p = 0.5
    k = D.keep_rowmajor(SEED, 2, 40, 64, p)
    for r in range(1, 40):
        assert _differ(k[0], k[r]) > 0.2
    a = D.keep_attention(SEED, 16, 8, 20, 36, p)              # B = 2 x 4 heads
    for bh in range(1, 8):
        assert _differ(a[0], a[bh]) > 0.4
    for i in range(1, 20):
        assert _differ(a[0, 0], a[0, i]) > 0.2
    # key pairs and lane groups are not copies of each other either
    assert _differ(a[:, :, :16], a[:, :, 16:32]) > 0.4 and _differ(a[:, :, :4], a[:, :, 4:8]) > 0.4
