"""The masked-region head's two loss kernels (csrc/region_head.hip) alone, from given fp32 logits (-m gpu).  One wave holds a row: lane l
owns the float4 chunks l, l + 64, ... of it.  C in {17, 64, 130, 1601, 2048}: fewer columns than lanes, one float4 per 16 lanes ... exactly
one column per lane, a float4 tail, the real size (one past a multiple of 64: 7 chunks per lane, the last nearly empty) and the limit
(8 full chunks).  R in {1, 3, 4, 5, 64, 65}: a partial workgroup of four waves, a full one, one past it, the 64-row pad unit and one past.

Bounds against fp64 from the kernel's own fp32 logits x (nothing is fitted to what the kernels return).

Hard form -- those of tests/test_lm_head_kernels_gpu.py with C for V:

    |loss_r - ref| , |lse_r - ref| <= E_r := (C + 8) 2^-24 + 2^-22 (|max| + |lse|)     summation of terms in (0, 1], exp and log rounding
    |dL - ref|                    <= 2^-8 |ref| + (C + 8) 2^-24 |g| / n                 the bf16 store, and the forward's error on p

Soft form, loss_r = sum_j t_j (log t_j - x_j + lse), ref in fp64 from the fp32 targets t (exact in fp64):

  * lse enters every term with weight t_j: its error E_r counts s_r = sum_j t_j times;
  * a term is t_j * ((log t_j) - (x_j - lse)): one logf (<= 2 ulp), two subtractions and one product, each rounding at most 2^-24 of an
    operand no larger than |log t_j| + |x_j| + |lse|, so at most 5 * 2^-24 t_j (|log t_j| + |x_j| + |lse|);
  * the terms are added per lane in order (4 ceil(C / 256) <= 32 of them) and through a six-level tree: at most 4 ceil(C / 256) + 6
    roundings of partial sums that are bounded by sum_j |term_j| <= sum_j t_j (|log t_j| + |x_j| + |lse|).
  Together 4 ceil(C / 256) + 11 roundings, which is at most C + 8 for every C >= 7 (C = 17: 15 <= 25; C = 2048: 43 <= 2056):

    |loss_r - ref| <= s_r E_r + (C + 8) 2^-24 sum_j t_j (|log t_j| + |x_j| + |lse|)

  dL = (p_j s_r - t_j) g / n with p = exp(x - lse).  p carries the forward's error, (C + 8) 2^-24 absolute as in the hard form, times s_r;
  s_r is a sum of C non-negative fp32 numbers in the same lane-then-tree order, relative error (C + 8) 2^-24, times p_j <= 1; the
  product and the difference round once each, 2^-24 (p_j s_r) + 2^-24 max(p_j s_r, t_j); the scale and the bf16 store as before:

    |dL - ref| <= 2^-8 |ref| + ((C + 8) 2^-24 s_r (1 + p_j) + 2^-23 (p_j s_r + t_j)) |g| / n

A one-hot soft target must give the hard kernel's loss_r within the two loss bounds added together.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from crct import ops                               # noqa: E402

DEV = torch.device("cuda:0")
CS = (17, 64, 130, 1601, 2048)
RS = (1, 3, 4, 5, 64, 65)
CASES = [(C, R) for C in CS for R in RS]
EDGE = [(17, 5), (130, 65), (1601, 3), (2048, 4)]


def labels_for(x, C, seed):
    """int64 [R]: random, with 0, C - 1, one label shared by two rows and one row whose label is its argmax where R has room for them."""
    R = x.shape[0]
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, C, (R,), generator=g)
    if R >= 5:
        lab[0], lab[1], lab[2], lab[3] = 0, C - 1, 7, 7
    lab[R - 1] = int(x[R - 1, :C].argmax())
    return lab


def soft_for(R, C, seed):
    """fp32 [R, C] >= 0: about a third zeros; rows that sum to 1, one that sums to 0.5, one one-hot, where R has room."""
    g = torch.Generator().manual_seed(seed + 1000)
    t = torch.rand(R, C, generator=g)
    t[torch.rand(R, C, generator=g) < 0.3] = 0.0
    t[:, 0] += 1e-3                                                 # no all-zero row by accident
    t = (t / t.sum(1, keepdim=True)).float()
    if R >= 3:
        t[1] *= 0.5
        t[2] = 0.0
        t[2, C - 1] = 1.0
    return t


def padded(x, Rp, Cp, fill):
    out = torch.full((Rp, Cp), float(fill), dtype=torch.float32)
    out[:x.shape[0], :x.shape[1]] = x
    return out


def lse_bound(xd, ref_lse, C):
    return (C + 8) * 2.0 ** -24 + 2.0 ** -22 * (xd.max(1).values.abs() + ref_lse.abs())


def run_kernels(buf, R, C, gd, **kw):
    loss, lse, total = ops.region_ce_fwd(buf, R, C, 1.0 / R, **kw)
    dL = ops.region_ce_bwd(buf, lse, gd, 1.0 / R, R, C, **kw)
    return loss, lse, total, dL


def check(x, C, g, lab=None, t=None, fill=50.0):
    """x fp32 [R, C] (CPU): both kernels on a [Rp, Cp] buffer whose pad columns and rows hold `fill`, against fp64 over the C real columns.
    Hard with ``lab`` int64 [R]; soft with ``t`` fp32 [R, C], which goes to the device as rows of a LARGER [N, C] tensor whose other rows hold
    NaN and is read there by index.  Returns the per-row loss (fp64) and its bound."""
    R = x.shape[0]
    Rp, Cp = ops.pad64(R), ops.pad64(C)
    buf = padded(x, Rp, Cp, fill).to(DEV)
    gd = torch.tensor([g], dtype=torch.float32, device=DEV)
    if t is None:
        kw = dict(labels=lab.to(torch.int32).to(DEV))
        td = torch.zeros(R, C, dtype=torch.float64)
        td[torch.arange(R), lab] = 1.0
    else:
        gen = torch.Generator().manual_seed(R * 31 + C)
        N = 2 * R + 3
        where = torch.randperm(N, generator=gen)[:R]                 # unsorted: a row list is any list
        big = torch.full((N, C), float("nan"))
        big[where] = t
        kw = dict(targets=big.to(DEV), rows=where.to(torch.int32).to(DEV))
        td = t.double()
    loss, lse, total, dL = run_kernels(buf, R, C, gd, **kw)
    for a, b in zip((loss, lse, total, dL), run_kernels(buf, R, C, gd, **kw)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "second run differs"
    assert torch.isfinite(loss).all() and torch.isfinite(lse).all() and torch.isfinite(dL.float()).all()
    xd = x.double()
    ref_lse = torch.logsumexp(xd, 1)
    logp = xd - ref_lse[:, None]
    s = td.sum(1)
    ref_loss = (torch.xlogy(td, td) - torch.where(td > 0, td * logp, torch.zeros_like(td))).sum(1)
    E = lse_bound(xd, ref_lse, C)
    if t is None:
        b_loss = E
    else:
        mag = (torch.xlogy(td, td).abs() + td * (xd.abs() + ref_lse.abs()[:, None])).sum(1)      # sum_j t_j (|log t_j| + |x_j| + |lse|)
        b_loss = s * E + (C + 8) * 2.0 ** -24 * mag
    e_loss, e_lse = (loss.cpu().double() - ref_loss).abs(), (lse.cpu().double() - ref_lse).abs()
    print("C %d R %d %s: loss err / bound %.3f, lse err / bound %.3f" % (C, R, "hard" if t is None else "soft", float((e_loss / b_loss).max()),
                                                                       float((e_lse / E).max())))
    assert bool((e_loss <= b_loss).all()) and bool((e_lse <= E).all())
    e_tot = abs(float(total.cpu().double()) - float(ref_loss.mean()))
    assert tuple(total.shape) == (1, 1) and e_tot <= float(b_loss.max()) + (R + 8) * 2.0 ** -24 * float(ref_loss.abs().mean())
    p = torch.exp(logp)
    ref_dL = (p * s[:, None] - td) * (g / R)
    got = dL.cpu().double()
    e_dL = (got[:R, :C] - ref_dL).abs()
    if t is None:
        b_dL = 2.0 ** -8 * ref_dL.abs() + (C + 8) * 2.0 ** -24 * abs(g) / R
    else:
        b_dL = 2.0 ** -8 * ref_dL.abs() + ((C + 8) * 2.0 ** -24 * s[:, None] * (1.0 + p) + 2.0 ** -23 * (p * s[:, None] + td)) * abs(g) / R
    print("          dL err / bound %.3f" % float((e_dL / b_dL).max()))
    assert bool((e_dL <= b_dL).all())
    raw = dL.cpu().view(torch.int16)
    assert tuple(raw.shape) == (Rp, Cp)
    assert int(raw[:, C:].abs().max()) == 0 if Cp > C else True, "a pad column of dL is not +0"
    assert int(raw[R:].abs().max()) == 0 if Rp > R else True, "a pad row of dL is not +0"
    return loss.cpu().double(), b_loss


def logits_for(C, R, seed, scale=3.0):
    return torch.randn(R, C, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.mark.parametrize("C,R", CASES)
def test_hard_within_bounds_reproducible_and_zero_padded(C, R):
    x = logits_for(C, R, C * 7 + R)
    check(x, C, 1.0, lab=labels_for(x, C, R))


@pytest.mark.parametrize("C,R", CASES)
def test_soft_within_bounds_reproducible_and_read_by_row_index(C, R):
    x = logits_for(C, R, C * 11 + R)
    check(x, C, 1.0, t=soft_for(R, C, C + R))


@pytest.mark.parametrize("C,R", EDGE)
def test_one_hot_soft_target_is_the_hard_loss(C, R):
    x = logits_for(C, R, C * 13 + R)
    lab = labels_for(x, C, R)
    t = torch.zeros(R, C)
    t[torch.arange(R), lab] = 1.0
    hard, b_hard = check(x, C, 1.0, lab=lab)
    soft, b_soft = check(x, C, 1.0, t=t)
    assert bool(((hard - soft).abs() <= b_hard + b_soft).all())


@pytest.mark.parametrize("C,R", EDGE)
@pytest.mark.parametrize("soft", (False, True))
def test_pad_columns_and_rows_never_leak(C, R, soft):
    """Every real logit sits near -8 while the pad columns and pad rows of the buffer hold +50: one pad value read into the maximum, the sum
    or the gradient would move the loss by ~58 (C = 2048 has no pad column: its rows still do)."""
    x = (-8.0 + 0.05 * logits_for(C, R, C + R, 1.0)).float()
    if soft:
        check(x, C, 1024.0, t=soft_for(R, C, C - R), fill=50.0)
    else:
        check(x, C, 1024.0, lab=labels_for(x, C, R), fill=50.0)


@pytest.mark.parametrize("C,R", EDGE)
@pytest.mark.parametrize("soft", (False, True))
def test_a_column_at_plus_ninety_stays_finite(C, R, soft):
    x = logits_for(C, R, C - R, 1.0)
    x[:, 11] += 90.0
    if soft:
        check(x, C, 1.0, t=soft_for(R, C, C * 3 + R))
    else:
        check(x, C, 1.0, lab=labels_for(x, C, R))


def test_more_classes_than_a_wave_holds_and_mixed_target_forms_are_refused_without_a_launch():
    buf = torch.zeros(64, 2112, device=DEV)
    lab = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="region_ce_fwd"):
        ops.region_ce_fwd(buf, 1, 2049, 1.0, labels=lab)
    with pytest.raises(ValueError, match="either labels"):
        ops.region_ce_fwd(buf, 1, 17, 1.0)
    with pytest.raises(ValueError, match="either labels"):
        ops.region_ce_fwd(buf, 1, 17, 1.0, labels=lab, targets=torch.zeros(1, 17, device=DEV), rows=lab)
