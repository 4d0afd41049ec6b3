"""The attention yardstick (tests/attention_ref.py) proved on the CPU: the emulator of the kernels' documented arithmetic stays inside the
derived budget, every named mutant leaves it, and errors and budgets scale together.  No GPU."""
import functools

import pytest
import torch

import attention_ref as AR
import dropout_ref as DR

B, HEADS = 4, 2                         # four batch rows: every mask_row kind of the 'masks' family
SHAPES = [(20, 36, 32), (7, 5, 32), (100, 100, 64), (124, 44, 48), (300, 512, 64)]
SEED, SITE = 4242, 9


def _paths(Tq, Tk):
    """(path, kept statistics) an attention call of that shape can take"""
    short = [("mfma", False), ("valu", False)] if Tq <= 112 and Tk <= 112 else []
    return short + [("long", False), ("long", True)]


@functools.lru_cache(maxsize=None)
def _case(family, Tq, Tk, d, p):
    q, k, v, dctx, km = AR.make_inputs(family, B, HEADS, Tq, Tk, d, seed=Tq + Tk)
    keep = DR.keep_attention(SEED, SITE, B * HEADS, Tq, Tk, p) if p > 0 else None
    return (q, k, v, km, dctx), keep, AR.reference(q, k, v, km, dctx, HEADS, d, keep=keep, p=p)


def _ratios(family, Tq, Tk, d, p, path, kept, mutate=None, ops=None, ref=None):
    (q, k, v, km, dctx), keep, r = _case(family, Tq, Tk, d, p)
    if ops is not None:
        q, k, v, km, dctx = ops
        r = ref
    em = AR.emulate(q, k, v, km, dctx, HEADS, d, keep=keep, p=p, path=path, kept=kept, mutate=mutate)
    return {n: float(AR.ratio(em[n], r[n], AR.budget_of(r, n, kept)).max()) for n in AR.OUTPUTS}, em


@pytest.mark.parametrize("family", AR.FAMILIES)
def test_unmutated_emulator_stays_within_nine_tenths_of_the_budget(family):
    """Every shape of SHAPES, p in {0, 0.1}, every path the shape can take, recomputed and kept statistics: the largest
    |emulator - fp64| / (bf16 step + budget) over all elements of ctx, dq, dk, dv is at most 0.9.  Observed maxima over the families
    (the largest is 0.79: peaked, long, dq):
                     ctx    dq     dk     dv       worst family
        mfma         0.70   0.76   0.74   0.71     early_max / early_max / peaked / peaked
        valu         0.33   0.33   0.33   0.35     (nothing but the outputs is rounded)
        long         0.65   0.79   0.74   0.75     peaked
        long, kept   0.65   0.40   0.30   0.75     peaked (the kept form's budget holds the extra ctx-rounding term)
    """
    worst = {}
    for Tq, Tk, d in SHAPES:
        for p in (0.0, 0.1):
            for path, kept in _paths(Tq, Tk):
                got, _ = _ratios(family, Tq, Tk, d, p, path, kept)
                key = path + ("/kept" if kept else "")
                for n, x in got.items():
                    worst.setdefault(key, {}).setdefault(n, 0.0)
                    worst[key][n] = max(worst[key][n], x)
                    assert x <= 0.9, "%s %dx%dx%d p=%g %s: %s at %.3f of the budget" % (family, Tq, Tk, d, p, key, n, x)
    for key, w in worst.items():
        print("%-10s %-10s " % (family, key) + " ".join("%s %.2f" % (n, w[n]) for n in AR.OUTPUTS))


# mutant -> (family, p, the outputs it must push over the budget, [(Tq, Tk, d, path, kept)])
MUTANT_CASES = {
    "delta_dropped": ("flat", 0.1, ("dq", "dk"), [(300, 512, 64, "long", False), (124, 44, 48, "long", False), (100, 100, 64, "mfma", False),
                                                 (100, 100, 64, "valu", False)]),
    "no_rescale_last": ("late_max", 0.0, ("ctx",), [(100, 100, 64, "long", False), (300, 512, 64, "long", False), (20, 36, 32, "long", False)]),
    "dv_no_scale": ("flat", 0.1, ("dv",), [(20, 36, 32, "mfma", False), (100, 100, 64, "valu", False), (300, 512, 64, "long", False),
                                           (124, 44, 48, "long", True)]),
    "ragged_last_key": ("flat", 0.0, ("ctx",), [(20, 36, 32, "mfma", False), (100, 100, 64, "valu", False), (124, 44, 48, "long", False)]),
    "dk_last_qtile": ("flat", 0.0, ("dk",), [(20, 36, 32, "mfma", False), (100, 100, 64, "valu", False), (300, 512, 64, "long", False),
                                             (124, 44, 48, "long", True)]),
    "pad_masked": ("masks", 0.0, ("ctx", "dv"), [(20, 36, 32, "mfma", False), (100, 100, 64, "valu", False), (124, 44, 48, "long", False),
                                                  (124, 44, 48, "long", True)]),
}


@pytest.mark.parametrize("mutant", AR.MUTANTS)
def test_every_mutant_exceeds_the_budget(mutant):
    """Each wrong kernel of attention_ref.emulate leaves the budget on the family meant for it, at every listed shape and path.
    Observed ratios (per named output the SMALLEST over the listed cases of that case's largest ratio):
        delta_dropped    dq 4.77   dk 3.73        (p = 0.1: delta is off by the factor 1 / (1 - p))
        no_rescale_last  ctx 252.94
        dv_no_scale      dv 8.57
        ragged_last_key  ctx 50.20
        dk_last_qtile    dk 12.53
        pad_masked       ctx 15.08  dv 4.76       (the fully masked batch row of the masks family)
    """
    family, p, outs, cases = MUTANT_CASES[mutant]
    low = {n: float("inf") for n in outs}
    for Tq, Tk, d, path, kept in cases:
        got, _ = _ratios(family, Tq, Tk, d, p, path, kept, mutate=mutant)
        clean, _ = _ratios(family, Tq, Tk, d, p, path, kept)
        for n in outs:
            low[n] = min(low[n], got[n])
            assert got[n] > 1.0, "%s %dx%dx%d %s%s: %s only at %.3f of the budget" % (mutant, Tq, Tk, d, path, "/kept" if kept else "", n, got[n])
            assert clean[n] <= 0.9
    print("%-16s " % mutant + " ".join("%s %.2f" % (n, low[n]) for n in outs))


def test_errors_and_budgets_scale_with_dctx():
    """dctx * 2^-10: the gradients, their emulated bf16 values and their budgets all scale by exactly 2^-10 (powers of two commute with
    every rounding away from the subnormals), so the ratios do not move -- the budget has no absolute floor to hide behind."""
    Tq, Tk, d, p, f = 100, 100, 64, 0.1, 2.0 ** -10
    (q, k, v, km, dctx), keep, ref = _case("flat", Tq, Tk, d, p)
    small = AR.bf16(dctx.double() * f)
    ref_s = AR.reference(q, k, v, km, small, HEADS, d, keep=keep, p=p)
    for path, kept in _paths(Tq, Tk):
        r0, em0 = _ratios("flat", Tq, Tk, d, p, path, kept)
        r1, em1 = _ratios("flat", Tq, Tk, d, p, path, kept, ops=(q, k, v, km, small), ref=ref_s)
        for n in ("dq", "dk", "dv"):
            assert torch.equal(em1[n], em0[n] * f), (path, kept, n)
            torch.testing.assert_close(ref_s[n], ref[n] * f, rtol=1e-12, atol=0.0)
            torch.testing.assert_close(AR.budget_of(ref_s, n, kept), AR.budget_of(ref, n, kept) * f, rtol=1e-9, atol=0.0)
            assert abs(r1[n] - r0[n]) <= 1e-6 * r0[n], (path, kept, n, r0[n], r1[n])


def test_mask_rows_are_what_the_family_promises():
    import numpy as np
    g = np.random.default_rng(0)
    for Tk in (1, 5, 17, 36, 49, 65, 100, 113, 512):
        rows = [AR.mask_row(kind, Tk, g) for kind in range(4)]
        assert rows[0].any() and not rows[1].any()
        assert rows[2].sum() == 1 and rows[2].nonzero()[0][0] >= (Tk - 1) // 16 * 16
        if Tk >= 64:
            lo = rows[3].tolist().index(0)
            assert lo % 32 == 0 and 0 < lo and lo + 32 <= Tk and not rows[3][lo:lo + 32].any() and rows[3].sum() == Tk - 32
        assert Tk == 1 or rows[3].any()
