"""The weight-average yardstick (tests/ema_ref.py) proved on the CPU: the fp32 emulation of the kernel's two operations stays inside the
derived budget, and every mutant leaves it on every segment of the inputs the GPU tests use -- over the three steps of every optim_ref
family at every decay below 1, and on the tile-walked segments of optim_ref.shadow_fixture().  The latter is a condition on the INPUTS
(lr, the start of the average, the value families): it is asserted here so that the GPU tests cannot pass for want of contrast."""
import numpy as np
import pytest
import torch

import ema_ref as E
import optim_ref as R


def _steps(family, decay=0.999):
    """The trajectory the GPU test runs, on the host: (t, p before, p' after, e before) for t = 1, 2, 3 with the gradient t g; the
    average advances with the emulator at `decay` (each step is judged from its own stored inputs, as on the GPU)."""
    lay = E.Layout()
    (p, g, m, v), lr, wd, e = E.family_inputs(family, lay)
    lr_el, wd_el = lay.spread(lr), lay.spread(wd)
    out = []
    for t in (1, 2, 3):
        p1, m1, v1 = R.emulate(p, g * float(t), m, v, lr_el, wd_el, t)
        out.append((t, p, p1, e))
        e = E.emulate(e, p1, E.weight(decay))
        p, m, v = p1, m1, v1
    return lay, out


@pytest.mark.parametrize("family", R.FAMILIES)
def test_emulator_within_budget_and_mutants_outside(family):
    for decay in E.DECAYS:
        lay, steps = _steps(family, decay)
        segs = lay.segs()
        for t, p0, p1, e0 in steps:
            w = E.weight(decay)
            ref, budget = E.reference(e0, p1, w)
            got = E.emulate(e0, p1, w)
            ins = lay.inside
            E.assert_within(got[ins], ref[ins], budget[ins], "%s step %d decay %g" % (family, t, decay))
            if decay == 1.0:
                assert w == 0.0 and torch.equal(got.view(torch.int32), e0.view(torch.int32))       # fmaf(0, d, e) = e, bit for bit
                swapped = E.emulate(e0, p1, w, mutate="weights_swapped")
                for o, n, _ in segs:
                    assert not torch.equal(swapped[o:o + n].view(torch.int32), e0[o:o + n].view(torch.int32)), (family, t, o)
                continue
            for mutant in ("old_p", "weights_swapped", "no_tail"):
                bad = E.breaks(E.emulate(e0, p1, w, mutate=mutant, p_old=p0, segs=segs), ref, budget)
                for o, n, _ in segs:
                    if mutant == "no_tail":
                        if n % 4 == 0:        # no scalar tail: the mutant is the kernel there
                            assert not bool(bad[o:o + n].any())
                            continue
                        assert bool(bad[o + n - n % 4:o + n].all()), (family, t, decay, mutant, n)       # every tail element
                        assert not bool(bad[o:o + n - n % 4].any())
                    else:
                        assert bool(bad[o:o + n].any()), (family, t, decay, mutant, n)


@pytest.mark.parametrize("decay", [d for d in E.DECAYS if d < 1.0])
def test_plain_index_mutant_on_the_tile_walked_segments(decay):
    """shadow_fixture(): a tile-walked segment whose rows are longer than one tile (tin > 64) has a tile walk that differs from the
    plain chunk walk, and the mutant breaks the budget there; at tin = 64 the two walks are the same walk, and so are the results."""
    fx = R.shadow_fixture()
    segs = E.shadow_segs(fx)
    lr_el, wd_el = R.per_element(fx, fx["lr"]), R.per_element(fx, fx["wd"])
    p1, _, _ = R.emulate(fx["p"], fx["g"], fx["m"], fx["v"], lr_el, wd_el, 1)
    e0 = E.average_start(fx["total"], 9)
    w = E.weight(decay)
    ref, budget = E.reference(e0, p1, w)
    got = E.emulate(e0, p1, w)
    E.assert_within(got[fx["inside"]], ref[fx["inside"]], budget[fx["inside"]], "shadow fixture, decay %g" % decay)
    bad = E.breaks(E.emulate(e0, p1, w, mutate="plain_index", segs=segs), ref, budget)
    walked = 0
    for o, n, tin in segs:
        if tin > 64:
            walked += 1
            assert float(bad[o:o + n].double().mean()) > 0.5, (o, n, tin)
        else:
            ti, pi = E.tile_index(o, n, tin) if tin else (None, None)
            assert tin == 0 or bool((ti == pi).all())
            assert not bool(bad[o:o + n].any()), (o, n, tin)
    assert walked >= 5            # W_c, W_d and the three bands of the fused weight


def test_tile_index_is_a_permutation_of_the_segment():
    for n_out, tin in ((64, 192), (192, 128), (128, 64)):
        ti, pi = E.tile_index(640, n_out * tin, tin)
        assert sorted(ti.tolist()) == pi.tolist()


def test_budget_is_tight_enough_to_matter():
    """One ulp of the result is at most 2 U |ref|: a budget that typically allowed much more than an ulp or two would prove nothing
    (where e and w (p' - e) cancel, the rounding of the difference is large against the result, and the budget says so)."""
    lay, steps = _steps("init")
    _, _, p1, e0 = steps[0]
    for decay in (0.9, 0.9999):
        ref, budget = E.reference(e0, p1, E.weight(decay))
        ins = lay.inside & (ref.abs() > 1e-30)
        ulp = torch.from_numpy(np.spacing(np.abs(ref[ins].numpy().astype(np.float32))).astype(np.float64))
        assert float((budget[ins] / ulp).median()) <= 2.5


def test_subnormal_results_get_the_absolute_term():
    e = torch.tensor([2.0 ** -140, -2.0 ** -130, 2.0 ** -127])
    p = torch.tensor([2.0 ** -141, 2.0 ** -131, -2.0 ** -128])
    ref, budget = E.reference(e, p, E.weight(0.9))
    assert bool((budget >= E.SUBNORMAL).all())
    E.assert_within(E.emulate(e, p, E.weight(0.9)), ref, budget, "subnormal results")
