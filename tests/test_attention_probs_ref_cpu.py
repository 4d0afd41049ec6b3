"""The attention-map yardstick (tests/attention_probs_ref.py) proved on the CPU -- the emulator of the kernel's documented arithmetic stays
inside the derived budget, every named mutant leaves it -- and the C ABI of the feature: crct_attention_probs and
crct_engine_attention_probs are exported and bound, and crct_attention_probs refuses what it cannot take with a message naming the
limit before anything touches a GPU.  No GPU."""
import ctypes as C
import functools

import pytest
import torch

import attention_ref as AR
import attention_probs_ref as PR
import dropout_ref as DR
from crct import lib as L

B, HEADS = 4, 2                         # four batch rows: every mask_row kind of the 'masks' family
SHAPES = [(1, 1, 32), (17, 33, 48), (36, 20, 64), (44, 124, 32), (113, 113, 64), (257, 511, 64), (512, 512, 32)]
SEED, SITE = 4242, 9


@functools.lru_cache(maxsize=None)
def _case(family, Tq, Tk, d, p):
    q, k, _, _, km = AR.make_inputs(family, B, HEADS, Tq, Tk, d, seed=Tq + Tk)
    keep = DR.keep_attention(SEED, SITE, B * HEADS, Tq, Tk, p) if p > 0 else None
    return (q, k, km), keep, PR.reference(q, k, km, HEADS, d, keep=keep, p=p)


def _ratio(family, Tq, Tk, d, p, mutate=None):
    (q, k, km), keep, (ref, budget) = _case(family, Tq, Tk, d, p)
    em = PR.emulate(q, k, km, HEADS, d, keep=keep, p=p, mutate=mutate)
    return float(PR.ratio(em, ref, budget).max()), em, ref


@pytest.mark.parametrize("family", AR.FAMILIES)
def test_unmutated_emulator_stays_within_half_the_budget(family):
    """Every shape of SHAPES, p in {0, 0.1}: the largest |emulator - fp64| / budget over all elements is at most 0.50 (observed 0.49, in
    the fully masked rows of the masks family, where the fp32 spacing of x is 2^-10; flat 0.08, peaked 0.42, late_max 0.12, early_max 0.13); without dropout every row sums to
    1 within 6e-7; with it a dropped element is exactly 0."""
    worst = 0.0
    for Tq, Tk, d in SHAPES:
        for p in (0.0, 0.1):
            r, em, ref = _ratio(family, Tq, Tk, d, p)
            worst = max(worst, r)
            assert r <= 0.50, "%s %dx%dx%d p=%g: %.3f of the budget" % (family, Tq, Tk, d, p, r)
            if p == 0.0:
                dev = float((em.double().sum(-1) - 1.0).abs().max())
                assert dev <= 6e-7, "%s %dx%dx%d: a row sums to 1 + %.3g" % (family, Tq, Tk, d, dev)
            else:
                assert bool((em[ref == 0.0] == 0.0).all())
    print("%-10s largest |emulator - fp64| / budget %.2f" % (family, worst))


# mutant -> (family, p, shapes): applied where it has an effect -- pad_masked on shapes with Tk % 32 != 0, swapped_qk_lengths on Tq != Tk
MUTANT_CASES = {
    "pad_masked": ("masks", 0.0, [(17, 33, 48), (36, 20, 64), (44, 124, 32), (113, 113, 64), (257, 511, 64)]),
    "ragged_last_key": ("flat", 0.0, [(1, 1, 32), (17, 33, 48), (36, 20, 64), (44, 124, 32), (113, 113, 64), (257, 511, 64), (512, 512, 32)]),
    "no_dropout_scale": ("flat", 0.1, [(17, 33, 48), (36, 20, 64), (44, 124, 32), (113, 113, 64), (257, 511, 64), (512, 512, 32)]),
    "mask_of_batch0": ("masks", 0.0, [(17, 33, 48), (36, 20, 64), (44, 124, 32), (113, 113, 64), (257, 511, 64), (512, 512, 32)]),
    "swapped_qk_lengths": ("flat", 0.0, [(17, 33, 48), (36, 20, 64), (44, 124, 32), (257, 511, 64)]),
}


@pytest.mark.parametrize("mutant", PR.MUTANTS)
def test_every_mutant_exceeds_the_budget(mutant):
    """Each wrong kernel of attention_probs_ref.emulate leaves the budget at every shape listed for it (the issue asks for at least one),
    where the clean emulator stays inside."""
    family, p, shapes = MUTANT_CASES[mutant]
    low = float("inf")
    for Tq, Tk, d in shapes:
        got, _, _ = _ratio(family, Tq, Tk, d, p, mutate=mutant)
        clean, _, _ = _ratio(family, Tq, Tk, d, p)
        low = min(low, got)
        assert got > 1.0, "%s %dx%dx%d: only at %.3f of the budget" % (mutant, Tq, Tk, d, got)
        assert clean <= 0.50
    print("%-18s smallest of the largest ratios %.3g" % (mutant, low))


def test_the_mutant_shapes_are_where_the_mutants_act():
    assert all(Tk % 32 for _, Tk, _ in MUTANT_CASES["pad_masked"][2])
    assert all(Tq != Tk for Tq, Tk, _ in MUTANT_CASES["swapped_qk_lengths"][2])
    assert set(MUTANT_CASES) == set(PR.MUTANTS) and all(set(s) <= set(SHAPES) for _, _, s in MUTANT_CASES.values())


# ------------------------------------------------------------------------------------------- the C ABI, without a GPU
P = 64          # stands for a 16-byte aligned device address: a call that passes validation is never made here


def test_symbols_are_exported_and_bound():
    raw = C.CDLL(L.LIB_PATH)
    for name in ("crct_attention_probs", "crct_engine_attention_probs"):
        assert hasattr(raw, name), name
        assert name in L.PROTOTYPES, name
        assert L.PROTOTYPES[name][1][-1] is L.vp          # stream last
    assert L.PROTOTYPES["crct_attention_probs"][0] is C.c_int and len(L.PROTOTYPES["crct_attention_probs"][1]) == 16
    assert L.PROTOTYPES["crct_engine_attention_probs"][0] is L.c_i64 and len(L.PROTOTYPES["crct_engine_attention_probs"][1]) == 10
    assert L.load().crct_abi_version() == 7                 # new entry points only: no struct or prototype changed


def _call(lib, probs=P, Tq=20, Tk=36, d=32, ldq=3 * 64 + 8, ldk=3 * 64 + 8):
    return lib.crct_attention_probs(P, P, P, probs, 2, 2, Tq, Tk, d, ldq, ldk, 0, 1.0, 0, 0, None)


@pytest.mark.parametrize("kw, word", [
    (dict(Tk=513), b"must be in [1,512]"), (dict(Tq=513), b"must be in [1,512]"), (dict(Tk=0), b"must be in [1,512]"),
    (dict(d=72, ldq=3 * 144 + 8, ldk=3 * 144 + 8), b"multiple of 8 in [8,64]"), (dict(d=20), b"multiple of 8 in [8,64]"),
    (dict(probs=None), b"null output"), (dict(ldq=3 * 64 + 4), b"multiples of 8"), (dict(ldk=32), b"at least heads * d"),
])
def test_attention_probs_refuses_what_it_cannot_take(kw, word):
    lib = L.load()
    assert _call(lib, **kw) != 0
    msg = lib.crct_last_error()
    assert b"attention_probs" in msg and word in msg, msg


def test_engine_attention_probs_refuses_null_arguments():
    lib = L.load()
    assert lib.crct_engine_attention_probs(None, None, None, None, 0, 0, 0, None, 0, None) == -1
    assert b"engine_attention_probs: null argument" in lib.crct_last_error()


def test_python_surface_exists():
    from crct import ops
    from crct.engine import StepEngine
    assert callable(ops.attention_probs) and callable(StepEngine.attention_probs)
