"""The optimizer yardstick (tests/optim_ref.py) proved on the CPU: the fp32 emulator of adamw_kernel's arithmetic stays inside the derived
budget, every arithmetic mutant leaves it, every shadow mutant differs in bits from the host model, the hand-written fp8 encoder is
torch's, and errors and budgets scale together.  No GPU."""
import functools

import numpy as np
import pytest
import torch

import optim_ref as R

N = 2048
# gradient scaling as the update can receive it: nothing, inv_scale_dev alone, amp.grad_scale alone, both (0.37 is not a power of two)
SCALINGS = (dict(), dict(inv_scale=0.37), dict(grad_scale=1024.0), dict(inv_scale=0.37, grad_scale=3.0))


@functools.lru_cache(maxsize=None)
def _inputs(family):
    return R.make_family(family, N, seed=1)


def _three_steps(family, lr, wd, scaling, device_step, mutate=None, t0=1):
    """Steps t0 .. t0 + 2; every step's reference starts from the emulator's own p, m, v of the step before.  Largest ratio per output."""
    p, g, m, v = _inputs(family)
    worst = dict.fromkeys(R.OUTPUTS, 0.0)
    for k in range(3):
        t = t0 + k
        gk = g * float(k + 1)
        ref = R.reference(p, gk, m, v, lr, wd, t, device_step=device_step, **scaling)
        p, m, v = R.emulate(p, gk, m, v, lr, wd, t, device_step=device_step, mutate=mutate, **scaling)
        for n, x in zip(R.OUTPUTS, (p, m, v)):
            worst[n] = max(worst[n], float(R.ratio(x, ref[n], ref["budget"][n]).max()))
    return worst


@pytest.mark.parametrize("family", R.FAMILIES)
def test_unmutated_emulator_stays_within_nine_tenths_of_the_budget(family):
    """All (lr, wd) pairs, all four gradient scalings, host and device step, steps 1-3 (and 10-12 on the device path): the largest
    |emulator - fp64| / budget is at most 0.9.  Observed maxima, host step / device step:
                   p              m              v
        p_zero     0.541 / 0.413  0.641 / 0.641  0.634 / 0.634
        init       0.821 / 0.811  0.648 / 0.648  0.640 / 0.640
        p_large    0.821 / 0.821  0.624 / 0.624  0.645 / 0.645
        sqrt_eps   0.816 / 0.809  0.645 / 0.645  0.656 / 0.656
        v_large    0.720 / 0.762  0.638 / 0.638  0.328 / 0.328
    The peak, p at 0.821, is the decayed weight alone (three roundings at |p|, the update far below them): that part of the budget is
    sharp, which is why a missing decay of lr wd = 1.5e-7 = 2.5 U sits at the budget and the pair (1e-3, 0.01) carries that mutant."""
    worst = {}
    for lr, wd in R.lr_wd_pairs():
        for sc in SCALINGS:
            for dev, t0 in ((False, 1), (True, 1), (True, 10)):
                got = _three_steps(family, lr, wd, sc, dev, t0=t0)
                for n, x in got.items():
                    key = "device" if dev else "host"
                    worst.setdefault(key, dict.fromkeys(R.OUTPUTS, 0.0))
                    worst[key][n] = max(worst[key][n], x)
                    assert x <= 0.9, "%s lr=%g wd=%g %s %s step, t0=%d: %s at %.3f of the budget" % (family, lr, wd, sc, key, t0, n, x)
    for key, w in worst.items():
        print("%-9s %-7s " % (family, key) + " ".join("%s %.3f" % (n, w[n]) for n in R.OUTPUTS))


# mutant -> (the output it must push over the budget, lr, wd, scaling)
MUTANT_CASES = {
    "no_decay": ("p", 1e-3, 0.01, {}),
    "l2_decay": ("p", 1e-3, 0.01, {}),
    "eps_in_sqrt": ("p", 1.5e-5, 0.0, {}),
    "bc2_no_sqrt": ("p", 1.5e-5, 0.01, {}),
    "no_bc1": ("p", 1.5e-5, 0.01, {}),
    "beta1_for_v": ("v", 1.5e-5, 0.01, {}),
    "gsc_m_only": ("v", 1.5e-5, 0.01, dict(inv_scale=0.37)),
    "grad_scale_multiplied": ("m", 1.5e-5, 0.01, dict(grad_scale=3.0)),
}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_arithmetic_mutant_exceeds_the_budget(mutant):
    """Each wrong kernel of optim_ref.emulate leaves the budget of the named output in at least one family (host step, steps 1-3; lr, wd
    and gradient scaling from MUTANT_CASES).  Observed largest ratio per family:
                                   p_zero   init     p_large  sqrt_eps v_large
        no_decay               p   38.7     56.1     56.2     55.9     56.3        <- the smallest: 56.3 is what the best family sees
        l2_decay               p   2.1e7    8.3e7    1.0e4    9.5e6    56.2
        eps_in_sqrt            p   1.3e6    8.8e5    57.8     1.2e6    0.31        (v' >> eps in v_large: nothing to see there)
        bc2_no_sqrt            p   1.2e6    9.1e5    75.7     1.2e6    19.5
        no_bc1                 p   1.1e6    8.5e5    70.5     1.1e6    17.9
        beta1_for_v            v   1.4e7    1.4e7    1.4e7    5.5e8    0.33        (g^2 is 1e-16 of v there)
        gsc_m_only             v   7.5e5    7.6e5    7.3e5    2.1e7    0.33
        grad_scale_multiplied  m   2.7e7    2.7e7    2.7e7    2.7e7    2.4e7"""
    out, lr, wd, sc = MUTANT_CASES[mutant]
    per_family = {f: _three_steps(f, lr, wd, sc, False, mutate=mutant)[out] for f in R.FAMILIES}
    clean = {f: _three_steps(f, lr, wd, sc, False)[out] for f in R.FAMILIES}
    print("%-22s %s " % (mutant, out) + " ".join("%s %.3g" % (f, per_family[f]) for f in R.FAMILIES))
    assert max(per_family.values()) > 1.0, (mutant, per_family)
    assert max(clean.values()) <= 0.9


# ------------------------------------------------------------------------------------------- bit-exact host models
def _fp8_probe():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(100000, generator=g) * torch.exp(torch.randn(100000, generator=g) * 4)
    edge = torch.tensor([448.0, 456.0, 464.0, 465.0, 480.0, 57344.0, 61439.0, 61440.0, 1e9, float("inf"), -float("inf"), 0.0, -0.0, 1e-30, -1e-30])
    return torch.cat([x, torch.tensor(R.PLANTED), edge]).float()


@pytest.mark.parametrize("kind,dtype,fmax", [("e4m3", torch.float8_e4m3fn, 448.0), ("e5m2", torch.float8_e5m2, 57344.0)])
def test_fp8_encoder_is_torchs_conversion(kind, dtype, fmax):
    """fp8_encode, written out bit by bit, against torch's round-to-nearest-even conversion: clamped (the kernels' form, `_q8` of
    tests/test_kernels_gpu.py) at several scales, and unclamped (what lies beyond becomes 0x7F / inf)."""
    x = _fp8_probe()
    for sc in (1.0, 37.0, 1e-3, 3000.0, 64.0):
        want = (x * torch.tensor(np.float32(sc))).clamp(-fmax, fmax).to(dtype).view(torch.uint8)
        got = R.q8(x, sc, kind)
        assert torch.equal(got, want), (kind, sc, x[got != want][:4])
        assert not bool(((got & 0x7F) == 0x7F).any()) if kind == "e4m3" else not bool(((got & 0x7F) > 0x7B).any())
    assert torch.equal(R.fp8_encode(x, kind, clamp=False), x.to(dtype).view(torch.uint8))
    # truncation differs from round-to-nearest-even exactly where the value is not representable and does not round down
    t, r = R.fp8_encode(x, kind, mode="trunc"), R.fp8_encode(x, kind)
    assert bool((t != r).any()) and bool(((t & 0x7F) <= (r & 0x7F)).all())


def test_bf16_model_rounds_to_nearest_even():
    x = torch.tensor([1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e38, 1e-40], dtype=torch.float32)       # ties at 1 + 2^-8 (down), 1 + 3 * 2^-8 (up)
    got = R.bf16_bits(x).view(torch.bfloat16).float()
    assert got.tolist()[:4] == [1.0, 1.0, 1.015625, -1.0]


@functools.lru_cache(maxsize=None)
def _shadow_step():
    fx = R.shadow_fixture()
    lr, wd = R.per_element(fx, fx["lr"]), R.per_element(fx, fx["wd"])
    p1, _, _ = R.emulate(fx["p"], fx["g"], fx["m"], fx["v"], lr, wd, 1)
    return fx, p1


def test_shadow_fixture_holds_what_it_promises():
    fx, p1 = _shadow_step()
    assert all(o % 64 == 0 for o in fx["off"]) and all(b % 64 == 0 for b in fx["t_base"])
    assert torch.equal(p1[fx["planted"]], fx["p"][fx["planted"]])                  # g = m = v = 0, wd = 0: p' = p, signed zeros included
    assert bool(torch.signbit(p1[fx["planted"]][torch.tensor(R.PLANTED * 2) == 0]).any())
    q, qt, amax = R.shadow_model(fx, p1)
    for sl in (1, 4):                                                              # the saturating slots: +-448 appear, never 0x7F / 0xFF
        seg = [i for i, s in enumerate(fx["slot"]) if s == sl]
        b = torch.cat([q[fx["off"][i]:fx["off"][i] + fx["len"][i]] for i in seg])
        x = torch.cat([p1[fx["off"][i]:fx["off"][i] + fx["len"][i]] for i in seg])
        assert bool((x.abs() * fx["scales"][sl] > 448.0).any()) and bool(((b & 0x7F) == 0x7E).any())
    assert not bool(((q[fx["inside"]] & 0x7F) == 0x7F).any())
    assert bool((q[~fx["inside"]] == R.SENTINEL_BYTE).all()) and bool((qt[~fx["inside"]] == R.SENTINEL_BYTE).all())
    # the transposed copy is the transposition per weight, the fused one included
    for off, out, cin, tr in fx["weights"]:
        blk = q[off:off + out * cin].reshape(out, cin)
        if tr:
            assert torch.equal(qt[off:off + out * cin].reshape(cin, out), blk.t())
        else:
            assert bool((qt[off:off + out * cin] == R.SENTINEL_BYTE).all())


@pytest.mark.parametrize("mutant", R.SHADOW_MUTANTS)
def test_every_shadow_mutant_differs_in_bits(mutant):
    fx, p1 = _shadow_step()
    q, qt, amax = R.shadow_model(fx, p1)
    q2, qt2, amax2 = R.shadow_model(fx, p1, p_old=fx["p"], mutate=mutant)
    diff = dict(q=int((q != q2).sum()), qt=int((qt != qt2).sum()), amax=int((amax != amax2).sum()))
    print("%-13s differs in %s" % (mutant, diff))
    where = dict(old_p="q", amax_old_p="amax", truncate="q", unclamped="q", tile_swapped="qt", band_base="qt")[mutant]
    assert diff[where] > 0, (mutant, diff)
    if mutant == "unclamped":
        assert bool(((q2 & 0x7F) == 0x7F).any())


# ------------------------------------------------------------------------------------------- scaling, and the reference itself
def test_errors_and_budgets_scale_together():
    """g, m and eps times 2^j with v times 4^j leave the update term alone and scale m', v' exactly; p and lr times 2^k (wd = 0) scale p'
    exactly.  Emulator, reference and budgets all follow, so no ratio moves: the budgets have no absolute floor to hide behind."""
    for family in ("init", "p_zero", "v_large"):
        p, g, m, v = _inputs(family)
        for j, k in ((-10, 7), (12, -9)):
            fj, fk = 2.0 ** j, 2.0 ** k
            lr, eps = 1e-3, 1e-8
            r0 = R.reference(p, g, m, v, lr, 0.0, 2, eps=eps)
            e0 = R.emulate(p, g, m, v, lr, 0.0, 2, eps=eps)
            lr1, eps1 = float(np.float32(lr)) * fk, float(np.float32(eps)) * fj
            args = (p * fk, g * fj, m * fj, v * fj * fj)
            r1 = R.reference(*args, lr1, 0.0, 2, eps=eps1)
            e1 = R.emulate(*args, lr1, 0.0, 2, eps=eps1)
            for n, x0, x1, f in zip(R.OUTPUTS, e0, e1, (fk, fj, fj * fj)):
                assert torch.equal(x1, x0 * f), (family, n, j, k)
                torch.testing.assert_close(r1[n], r0[n] * f, rtol=1e-12, atol=0.0)
                torch.testing.assert_close(r1["budget"][n], r0["budget"][n] * f, rtol=1e-9, atol=0.0)
                a, b = R.ratio(x0, r0[n], r0["budget"][n]), R.ratio(x1, r1[n], r1["budget"][n])
                assert float((a - b).abs().max()) <= 1e-6, (family, n, j, k)


def test_reference_against_torch_adamw():
    """The fp64 reference with fp32-valued betas against torch.optim.AdamW in fp64 with double betas, three steps: prints the relative
    difference in v' (expected (0.999 - fl32(0.999)) / 0.001 = 1.3e-5) and in p'; asserts only that the two are the same algorithm (1e-4)."""
    p, g, m, v = (x.double() for x in _inputs("init"))
    m, v = torch.zeros_like(m), torch.zeros_like(v)
    rp = p.clone().requires_grad_(True)
    opt = torch.optim.AdamW([rp], lr=1e-3, weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8)
    pp = p.clone()
    for t in (1, 2, 3):
        rp.grad = g * t
        opt.step()
        if t == 1:               # the fp64-state restatement below is reference()'s own arithmetic
            r = R.reference(pp, g, m, v, 1e-3, 0.01, 1)
            for a, b in zip(_reference64(pp, g, m, v, 1), (r["p"], r["m"], r["v"])):
                torch.testing.assert_close(a, b, rtol=1e-13, atol=0.0)
        pp, m, v = _reference64(pp, g * t, m, v, t)       # state kept in fp64: the difference printed is the betas' alone
    st = opt.state[rp]
    nz = g != 0
    dv = float(((v - st["exp_avg_sq"]).abs()[nz] / st["exp_avg_sq"][nz]).max())
    dp = float(((pp - rp.detach()).abs() / rp.detach().abs().clamp_min(1e-3)).max())
    print("reference (fp32-valued betas) against torch.optim.AdamW (double betas), 3 steps: v' differs by %.3g relative, p' by %.3g" % (dv, dp))
    assert dv < 1e-4 and dp < 1e-4


def _reference64(p, g, m, v, t):
    """optim_ref.reference's formulas on fp64 state (reference() itself takes fp32 state)"""
    b1, b2, ep, lr, wd = R.f32(0.9), R.f32(0.999), R.f32(1e-8), R.f32(1e-3), R.f32(0.01)
    m1 = b1 * m + (1 - b1) * g
    v1 = b2 * v + (1 - b2) * g * g
    p1 = p * (1 - lr * wd) - lr / (1 - b1 ** t) * m1 / (v1.sqrt() / (1 - b2 ** t) ** 0.5 + ep)
    return p1, m1, v1
