"""Head size 128 without a GPU: the attention yardstick (tests/attention_ref.py) holds at d = 128 as it does at 32 / 48 / 64, the library's
host-side contract names 128 among the head sizes of the MFMA kernels, and the original ViLBERT config validates.

The yardstick part follows tests/test_attention_ref_cpu.py: the emulator of the kernels' documented arithmetic stays within 0.9 of the
derived budget, every mutant of attention_ref.MUTANTS leaves it.  The budget formulas contain d only through scale = 1 / sqrt(d)."""
import functools

import pytest

import attention_ref as AR
import dropout_ref as DR
from crct import config as C, lib as L

B, HEADS, D = 4, 2, 128                 # four batch rows: every mask_row kind of the 'masks' family
SHAPES = [(17, 36), (130, 49)]
PATHS = [("mfma", False), ("long", False), ("long", True)]
SEED, SITE = 4242, 9


@functools.lru_cache(maxsize=None)
def _case(family, Tq, Tk, p):
    q, k, v, dctx, km = AR.make_inputs(family, B, HEADS, Tq, Tk, D, seed=Tq + Tk)
    keep = DR.keep_attention(SEED, SITE, B * HEADS, Tq, Tk, p) if p > 0 else None
    return (q, k, v, km, dctx), keep, AR.reference(q, k, v, km, dctx, HEADS, D, keep=keep, p=p)


def _ratios(family, Tq, Tk, p, path, kept, mutate=None):
    (q, k, v, km, dctx), keep, r = _case(family, Tq, Tk, p)
    em = AR.emulate(q, k, v, km, dctx, HEADS, D, keep=keep, p=p, path=path, kept=kept, mutate=mutate)
    return {n: float(AR.ratio(em[n], r[n], AR.budget_of(r, n, kept)).max()) for n in AR.OUTPUTS}


@pytest.mark.parametrize("family", AR.FAMILIES)
def test_emulator_stays_within_nine_tenths_of_the_budget_at_head_size_128(family):
    """17 x 36 and 130 x 49 at d = 128, p in {0, 0.1}, paths mfma and long (recomputed and kept statistics): the same 0.9 of the budget
    tests/test_attention_ref_cpu.py holds the emulator to at the other head sizes.  (The emulator's 'mfma' arithmetic is defined for any
    length; the kernels take 130 x 49 on the long path.)"""
    worst = {}
    for Tq, Tk in SHAPES:
        for p in (0.0, 0.1):
            for path, kept in PATHS:
                got = _ratios(family, Tq, Tk, p, path, kept)
                key = path + ("/kept" if kept else "")
                for n, x in got.items():
                    worst.setdefault(key, {}).setdefault(n, 0.0)
                    worst[key][n] = max(worst[key][n], x)
                    assert x <= 0.9, "%s %dx%dx%d p=%g %s: %s at %.3f of the budget" % (family, Tq, Tk, D, p, key, n, x)
    for key, w in worst.items():
        print("%-10s %-10s " % (family, key) + " ".join("%s %.2f" % (n, w[n]) for n in AR.OUTPUTS))


# mutant -> (family, p, the outputs it must push over the budget, [(Tq, Tk, path, kept)]): the families and outputs of
# tests/test_attention_ref_cpu.py MUTANT_CASES, at this file's shapes
MUTANT_CASES = {
    "delta_dropped": ("flat", 0.1, ("dq", "dk"), [(17, 36, "mfma", False), (130, 49, "mfma", False), (17, 36, "long", False), (130, 49, "long", False)]),
    "no_rescale_last": ("late_max", 0.0, ("ctx",), [(17, 36, "long", False), (130, 49, "long", False)]),
    "dv_no_scale": ("flat", 0.1, ("dv",), [(17, 36, "mfma", False), (130, 49, "mfma", False), (17, 36, "long", False), (130, 49, "long", True)]),
    "ragged_last_key": ("flat", 0.0, ("ctx",), [(17, 36, "mfma", False), (130, 49, "mfma", False), (17, 36, "long", False), (130, 49, "long", False)]),
    "dk_last_qtile": ("flat", 0.0, ("dk",), [(17, 36, "mfma", False), (130, 49, "mfma", False), (17, 36, "long", False), (130, 49, "long", True)]),
    "pad_masked": ("masks", 0.0, ("ctx", "dv"), [(17, 36, "mfma", False), (130, 49, "mfma", False), (17, 36, "long", False), (130, 49, "long", True)]),
}


@pytest.mark.parametrize("mutant", AR.MUTANTS)
def test_every_mutant_exceeds_the_budget_at_head_size_128(mutant):
    family, p, outs, cases = MUTANT_CASES[mutant]
    low = {n: float("inf") for n in outs}
    for Tq, Tk, path, kept in cases:
        got = _ratios(family, Tq, Tk, p, path, kept, mutate=mutant)
        clean = _ratios(family, Tq, Tk, p, path, kept)
        for n in outs:
            low[n] = min(low[n], got[n])
            assert got[n] > 1.0, "%s %dx%dx%d %s%s: %s only at %.3f of the budget" % (mutant, Tq, Tk, D, path, "/kept" if kept else "", n, got[n])
            assert clean[n] <= 0.9
    print("%-16s " % mutant + " ".join("%s %.2f" % (n, low[n]) for n in outs))


def test_the_library_takes_head_size_128_at_every_length_and_the_abi_is_unchanged():
    lib = L.load()
    assert lib.crct_abi_version() == 7
    for Tq, Tk in ((44, 44), (124, 44), (44, 124), (257, 512), (512, 512)):
        assert lib.crct_attention_quant_ok(Tq, Tk, 128) == 1, (Tq, Tk)
    assert lib.crct_attention_quant_ok(124, 124, 40) == 0
    # every length in both directions (the diagonal and the two edges of the square)
    for T in range(1, 513):
        assert lib.crct_attention_quant_ok(T, T, 128) == 1 and lib.crct_attention_quant_ok(T, 512, 128) == 1 and lib.crct_attention_quant_ok(512, T, 128) == 1, T
    assert lib.crct_attention_quant_ok(513, 20, 128) == 0 and lib.crct_attention_quant_ok(20, 20, 96) == 0


def test_the_original_vilbert_config_has_head_sizes_64_128_128():
    c = C.vilbert_original_config()
    c.validate()
    assert (c.hidden_size // c.num_attention_heads, c.v_hidden_size // c.v_num_attention_heads,
            c.bi_hidden_size // c.bi_num_attention_heads) == (64, 128, 128)
    assert (c.num_attention_heads, c.v_num_attention_heads, c.bi_num_attention_heads, c.v_feature_size) == (12, 8, 8, 2048)
    base = C.vilbert_config()
    same = set(base.to_dict()) - {"num_attention_heads", "v_num_attention_heads", "bi_num_attention_heads", "v_feature_size"}
    assert all(getattr(c, k) == getattr(base, k) for k in same)
    assert C.vilbert_original_config(hidden_dropout_prob=0.0).hidden_dropout_prob == 0.0
