"""tests/poison_ref.py on launches whose footprint is known in closed form, the three mutants assert_footprint must catch, and what the
fp64 references say about the operations at which a non-finite value can disappear: the semantics the kernels are held to."""
import pytest
import torch

import gemm_ref as GR
import poison_ref as PR


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _matmul_case():
    a, b = _rand(9, 12, seed=1), _rand(7, 12, seed=2)
    ap, bp = PR.plant(a, (4, 11), PR.NAN), PR.plant(b, (5, 0), PR.INF)
    return GR.ref_nt, (a, b), (ap, bp)


def test_plant_leaves_the_source_alone_and_nonfinite_sees_every_kind():
    t = torch.zeros(3, 4)
    p = PR.plant(t, (1, 2), PR.NAN)
    assert bool(torch.isfinite(t).all()) and int(PR.nonfinite(p).sum()) == 1 and bool(PR.nonfinite(p)[1, 2])
    for dt in (torch.float64, torch.float32, torch.bfloat16, torch.float8_e4m3fn, torch.float8_e5m2):
        x = torch.tensor([1.0, PR.NAN, -2.0]).to(dt)
        assert PR.nonfinite(x).tolist() == [False, True, False], dt
    for dt in (torch.float32, torch.bfloat16, torch.float8_e5m2):      # e4m3fn has no inf
        assert PR.nonfinite(torch.tensor([PR.INF, 0.0, -PR.INF]).to(dt)).tolist() == [True, False, True], dt
    assert not bool((PR.bits(torch.tensor([0.0])) == PR.bits(torch.tensor([-0.0]))).any())
    assert bool((PR.bits(torch.tensor([PR.NAN])) == PR.bits(torch.tensor([PR.NAN]))).all())


def test_footprint_of_a_matmul_is_one_row_united_with_one_column():
    fn, clean, pois = _matmul_case()
    F = PR.footprint(fn, clean, pois)
    want = torch.zeros(9, 7, dtype=torch.bool)
    want[4, :] = True
    want[:, 5] = True
    assert torch.equal(F, want)
    PR.assert_footprint(fn(*clean), fn(*pois), F, "matmul")


def test_footprint_of_a_layernorm_is_one_row_of_every_output():
    def ln(x, g, b):
        mean = x.mean(-1)
        rstd = 1.0 / torch.sqrt(((x - mean[:, None]) ** 2).mean(-1) + 1e-12)
        return dict(y=g * (x - mean[:, None]) * rstd[:, None] + b, mean=mean, rstd=rstd)
    x, g, b = _rand(7, 96, seed=3), _rand(96, seed=4), _rand(96, seed=5)
    F = PR.footprint(ln, (x, g, b), (PR.plant(x, (2, 95), PR.NAN), g, b))
    rows = torch.zeros(7, dtype=torch.bool)
    rows[2] = True
    assert torch.equal(F["mean"], rows) and torch.equal(F["rstd"], rows) and torch.equal(F["y"], rows[:, None].expand(7, 96))
    PR.assert_footprint(ln(x, g, b), ln(PR.plant(x, (2, 95), PR.NAN), g, b), F, "layernorm")


def test_footprint_of_attention_probabilities_is_one_batch_and_head():
    def probs(q, k):         # [B, h, T, d]
        return torch.softmax(q @ k.transpose(-1, -2) / 4.0, -1)
    q, k = _rand(2, 3, 5, 16, seed=6), _rand(2, 3, 6, 16, seed=7)
    kp = PR.plant(k, (1, 1, 4, 0), PR.NAN)
    F = PR.footprint(probs, (q, k), (q, kp))
    want = torch.zeros(2, 3, 5, 6, dtype=torch.bool)
    want[1, 1] = True           # the softmax spreads the poisoned score over the row, every query row meets key 4
    assert torch.equal(F, want)
    qp = PR.plant(q, (1, 1, 2, 3), PR.INF)
    want = torch.zeros(2, 3, 5, 6, dtype=torch.bool)
    want[1, 1, 2] = True
    assert torch.equal(PR.footprint(probs, (q, k), (qp, k)), want)
    PR.assert_footprint(probs(q, k), probs(q, kp), F, "probs")


def test_footprint_refuses_a_reference_that_is_non_finite_when_clean():
    with pytest.raises(AssertionError, match="CLEAN"):
        PR.footprint(lambda x: x / 0.0, (torch.ones(3),), (torch.ones(3),))


# ------------------------------------------------------------------------------------------- the mutants
def test_mutant_one_element_of_the_footprint_finite_is_caught():
    fn, clean, pois = _matmul_case()
    F, yc = PR.footprint(fn, clean, pois), fn(*clean).float()
    yp = fn(*pois).float()
    yp[4, 3] = 0.0              # a relu that printed 0 for NaN
    with pytest.raises(AssertionError, match=r"R1 \(arrival\).*first at \(4, 3\)"):
        PR.assert_footprint(yc, yp, F, "mutant 1")


def test_mutant_one_ulp_outside_the_footprint_is_caught():
    fn, clean, pois = _matmul_case()
    F, yc = PR.footprint(fn, clean, pois), fn(*clean).float()
    yp = fn(*pois).float()
    yp[7, 2] = torch.nextafter(yp[7, 2], torch.tensor(PR.INF))
    assert abs(float(yp[7, 2]) - float(yc[7, 2])) <= 2.0 ** -22 * abs(float(yc[7, 2]))
    with pytest.raises(AssertionError, match=r"R2 \(containment\).*first at \(7, 2\)"):
        PR.assert_footprint(yc, yp, F, "mutant 2")
    # ... the same element within an atomic budget passes, a NaN there does not
    PR.assert_footprint(yc, yp, F, "mutant 2, budget", atomic=1e-5)
    yp[7, 2] = PR.NAN
    with pytest.raises(AssertionError, match=r"R2 \(containment\)"):
        PR.assert_footprint(yc, yp, F, "mutant 2, NaN under a budget", atomic=1e-5)
    yp = fn(*pois).float()
    yc2 = yc.clone()
    yc2[0, 0], yp[0, 0] = 0.0, -0.0                           # the sign of a zero is a bit too
    with pytest.raises(AssertionError, match=r"R2 \(containment\).*first at \(0, 0\)"):
        PR.assert_footprint(yc2, yp, F, "mutant 2, sign of zero")


def test_mutant_empty_or_full_footprint_is_caught():
    fn, clean, pois = _matmul_case()
    yc = fn(*clean).float()
    with pytest.raises(AssertionError, match="R3"):           # a reference that stopped propagating: nothing poisoned, nothing to see
        PR.assert_footprint(yc, yc.clone(), torch.zeros(9, 7, dtype=torch.bool), "mutant 3, empty")
    with pytest.raises(AssertionError, match="R3"):
        PR.assert_footprint(yc, torch.full_like(yc, PR.NAN), torch.ones(9, 7, dtype=torch.bool), "mutant 3, everything")
    # several outputs: one proper footprint is enough (all of dgamma, none of another problem's output)
    F = PR.footprint(fn, clean, pois)
    PR.assert_footprint(dict(y=yc, g=yc[0], o=yc), dict(y=fn(*pois).float(), g=torch.full_like(yc[0], PR.NAN), o=yc.clone()),
                        dict(y=F, g=torch.ones(7, dtype=torch.bool), o=torch.zeros(9, 7, dtype=torch.bool)), "three outputs")
    with pytest.raises(ValueError):
        PR.assert_footprint(yc, yc, F, "atomic=True", atomic=True)


# ------------------------------------------------------------------------------------------- what the references say
def test_reference_relu_keeps_nan_and_its_derivative_is_a_select():
    x = torch.tensor([-1.0, PR.NAN, 2.0, -PR.INF, PR.INF, -0.0], dtype=torch.float64)
    y = GR.ACTS["relu"](x)
    assert torch.isnan(y[1]) and y[[0, 2, 3, 5]].tolist() == [0.0, 2.0, 0.0, 0.0] and float(y[4]) == PR.INF
    assert torch.isnan(torch.relu(x)[1])                                   # what the oracle's torch.relu prints
    assert torch.isnan(GR.ACTS["leaky"](x)[1]) and torch.isnan(GR.ACTS["gelu"](x)[1]) and torch.isnan(GR.ACTS["tanh"](x)[1])
    # relu' / leaky' are selects on s > 0: a NaN in the saved output selects the `else` value, it does not propagate by itself
    assert GR.DACTS["relu"](x).tolist() == [0.0, 0.0, 1.0, 0.0, 1.0, 0.0]
    assert (GR.DACTS["leaky"](x) == 1.0).tolist() == [False, False, True, False, True, False] and not bool(PR.nonfinite(GR.DACTS["leaky"](x)).any())
    assert torch.isnan(GR.DACTS["gelu"](x)[1]) and torch.isnan(GR.DACTS["tanh"](x)[1])
    # ... through the epilogue: relu keeps the NaN of the accumulator, relu'(NaN) = 0 multiplies a finite accumulator to 0
    acc = torch.tensor([[1.0, PR.NAN, -3.0, 4.0]], dtype=torch.float64)
    assert PR.nonfinite(GR.epilogue(acc, act="relu")["y"]).tolist() == [[False, True, False, False]]
    src = torch.tensor([[1.0, 1.0, PR.NAN, 1.0]], dtype=torch.float64)
    r = GR.epilogue(acc, dact="relu", dact_src=src)["y"]
    assert PR.nonfinite(r).tolist() == [[False, True, False, False]] and float(r[0, 2]) == 0.0


def test_reference_dropout_zeroes_a_dropped_nan():
    acc = torch.tensor([[PR.NAN, PR.NAN, 1.0, PR.INF]], dtype=torch.float64)
    keep = torch.tensor([[True, False, True, False]])
    y = GR.epilogue(acc, keep=keep, drop_scale=2.0)["y"]
    assert PR.nonfinite(y).tolist() == [[True, False, False, False]] and y[0, 1:].tolist() == [0.0, 2.0, 0.0]
    # torch.nn.functional.dropout multiplies by the mask instead (0 * NaN = NaN): the kernels' select is the project's rule
    assert torch.isnan(torch.tensor(PR.NAN) * 0.0)


def test_reference_fp8_of_nan_is_nan_and_inf_saturates():
    x = torch.tensor([PR.NAN, PR.INF, -PR.INF, 1e6, -3.0], dtype=torch.float64)
    q4, q5 = GR.e4m3(x), GR.e5m2(x)
    assert torch.isnan(q4[0]) and q4[1:].tolist() == [448.0, -448.0, 448.0, -3.0]
    assert torch.isnan(q5[0]) and q5[1:].tolist() == [57344.0, -57344.0, 57344.0, -3.0]
    b4 = x.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    assert int(b4[0]) & 0x7F == 0x7F and int(b4[2]) == 0xFE                 # the NaN byte; -inf -> -448
    b5 = x.float().clamp(-57344.0, 57344.0).to(torch.float8_e5m2).view(torch.uint8)
    assert int(b5[0]) & 0x7F > 0x7C and int(b5[2]) == 0xFB                  # an e5m2 NaN (above the inf pattern 0x7C); -inf -> -57344
    r = GR.epilogue(torch.tensor([[PR.NAN, 2.0]], dtype=torch.float64), q_scale=4.0, q_kind="e4m3")
    assert torch.isnan(r["q"][0, 0]) and float(r["q"][0, 1]) == 8.0
