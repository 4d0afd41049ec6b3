"""The masked-LM head's kernels (csrc/lm_head.hip) one by one (-m gpu), at H = 64 with vocabularies that exercise the padding -- 130 (a tail
of 2 past a multiple of 8 and of 64), 200 (a multiple of 8, not of 64), 192 (an exact fit) -- and R = 1, 5, 64, 65 masked rows (below,
at and past one 64-row pad unit).  Bounds against fp64 from the kernel's own fp32 logits:

    |loss_r - ref| , |lse_r - ref| <= (V + 8) 2^-24 + 2^-22 (|max| + |lse|)      sequential summation of terms in (0, 1], exp and log rounding
    |dL - ref|                    <= 2^-8 |ref| + (V + 8) 2^-24 |g| / n           the bf16 store, and the forward's error on the label column
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_ref as G                               # noqa: E402
from crct import ops                               # noqa: E402

DEV = torch.device("cuda:0")
H = 64
VS = (130, 200, 192)
RS = (1, 5, 64, 65)
CASES = [(V, R) for V in VS for R in RS]


def labels_for(logits, V, seed):
    """int64 [R]: random, with 0, V - 1, one label shared by two rows and one row whose label is its argmax where R has room for them."""
    R = logits.shape[0]
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, V, (R,), generator=g)
    if R >= 5:
        lab[0], lab[1], lab[2], lab[3] = 0, V - 1, 7, 7
    lab[R - 1] = int(logits[R - 1, :V].argmax())
    return lab


def padded(x, Rp, Vp, fill):
    out = torch.full((Rp, Vp), float(fill), dtype=torch.float32)
    out[:x.shape[0], :x.shape[1]] = x
    return out


def check_ce(x, lab, V, g, fill=50.0):
    """x fp32 [R, V] (CPU): both cross-entropy kernels on a [Rp, Vp] buffer whose pad columns and rows hold `fill`, against fp64 over V."""
    R = x.shape[0]
    Rp, Vp = ops.pad64(R), ops.pad64(V)
    buf = padded(x, Rp, Vp, fill).to(DEV)
    lab32 = lab.to(torch.int32).to(DEV)
    gd = torch.tensor([g], dtype=torch.float32, device=DEV)
    loss, lse, total = ops.lm_ce_fwd(buf, lab32, R, V, 1.0 / R)
    dL = ops.lm_ce_bwd(buf, lab32, lse, gd, 1.0 / R, R, V)
    again = ops.lm_ce_fwd(buf, lab32, R, V, 1.0 / R) + (ops.lm_ce_bwd(buf, lab32, lse, gd, 1.0 / R, R, V),)
    for a, b in zip((loss, lse, total, dL), again):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "second run differs"
    xd = x.double()
    ref_lse = torch.logsumexp(xd, 1)
    ref_loss = ref_lse - xd[torch.arange(R), lab]
    bound = (V + 8) * 2.0 ** -24 + 2.0 ** -22 * (xd.max(1).values.abs() + ref_lse.abs())
    e_loss, e_lse = (loss.cpu().double() - ref_loss).abs(), (lse.cpu().double() - ref_lse).abs()
    print("V %d R %d: loss err / bound %.3f, lse err / bound %.3f" % (V, R, float((e_loss / bound).max()), float((e_lse / bound).max())))
    assert torch.isfinite(loss).all() and torch.isfinite(lse).all() and torch.isfinite(dL.float()).all()
    assert bool((e_loss <= bound).all()) and bool((e_lse <= bound).all())
    e_tot = abs(float(total.cpu().double()) - float(ref_loss.mean()))
    assert e_tot <= float(bound.max()) + (R + 8) * 2.0 ** -24 * float(ref_loss.abs().mean())
    p = torch.exp(xd - ref_lse[:, None])
    p[torch.arange(R), lab] -= 1.0
    ref_dL = p * (g / R)
    got = dL.cpu().double()
    e_dL = (got[:R, :V] - ref_dL).abs()
    b_dL = 2.0 ** -8 * ref_dL.abs() + (V + 8) * 2.0 ** -24 * abs(g) / R
    print("          dL err / bound %.3f" % float((e_dL / b_dL).max()))
    assert bool((e_dL <= b_dL).all())
    raw = dL.cpu().view(torch.int16)
    assert int(raw[:, V:].abs().max()) == 0 if Vp > V else True, "a pad column of dL is not +0"
    assert int(raw[R:].abs().max()) == 0 if Rp > R else True, "a pad row of dL is not +0"


@pytest.mark.parametrize("V,R", CASES)
def test_gather_is_index_select_then_bf16_with_zero_pad_rows(V, R):
    g = torch.Generator().manual_seed(V * 100 + R)
    N = R + 9
    src = torch.randn(N, H, generator=g)
    rows = torch.randperm(N, generator=g)[:R].sort().values
    poisoned = [i for i in range(N) if i not in set(rows.tolist())][0]
    src[poisoned] = float("nan")                                    # an unselected row reaches nothing
    out = ops.lm_gather_rows(src.to(DEV), rows.to(torch.int32).to(DEV), R).cpu()
    Rp = ops.pad64(R)
    assert tuple(out.shape) == (Rp, H)
    assert torch.equal(out[:R].view(torch.int16), src.index_select(0, rows).bfloat16().view(torch.int16))
    assert int(out[R:].view(torch.int16).abs().max()) == 0 if Rp > R else True


@pytest.mark.parametrize("V", VS)
def test_padded_operands_and_the_logits_product_are_exact_on_integers(V):
    R, Rp, Vp = 65, 128, ops.pad64(V)
    z, table = G.operands(Rp, V, H, 15, 15, seed=V, extra=255)     # 64 * 15 * 15 + 255 < 2^24: fp32 accumulation is exact
    bias = G.unit_ints((V,), 255, V + 2, 1.0)
    table_pad, bias_pad = ops.lm_pad_operands(table.bfloat16().to(DEV), bias.float().to(DEV))
    assert tuple(table_pad.shape) == (Vp, H) and tuple(bias_pad.shape) == (Vp,)
    assert torch.equal(table_pad[:V].cpu().view(torch.int16), table.bfloat16().view(torch.int16))
    if Vp > V:
        assert int(table_pad[V:].cpu().view(torch.int16).abs().max()) == 0 and int(bias_pad[V:].cpu().view(torch.int32).abs().max()) == 0
    assert torch.equal(bias_pad[:V].cpu(), bias.float())
    logits = ops.gemm(z.bfloat16().to(DEV), table_pad, Rp, Vp, H, bias=bias_pad, out_f32=True).cpu().double()
    assert torch.equal(logits[:, :V], G.ref_nt(z, table) + bias[None, :])
    assert float(logits[:, V:].abs().max()) == 0.0 if Vp > V else True


@pytest.mark.parametrize("V,R", CASES)
def test_cross_entropy_within_bounds_and_reproducible(V, R):
    g = torch.Generator().manual_seed(V * 7 + R)
    x = torch.randn(R, V, generator=g) * 3.0
    check_ce(x, labels_for(x, V, R), V, g=1.0)


@pytest.mark.parametrize("V,R", [(130, 5), (200, 65), (192, 64)])
def test_pad_columns_never_leak(V, R):
    """Every real logit sits near -8 while the pad columns (and pad rows) of the buffer hold +50: one pad column read into the maximum,
    the sum or the gradient would move the loss by ~58."""
    g = torch.Generator().manual_seed(V + R)
    x = (-8.0 + 0.05 * torch.randn(R, V, generator=g)).float()
    check_ce(x, labels_for(x, V, R), V, g=1024.0, fill=50.0)


@pytest.mark.parametrize("V,R", [(130, 5), (192, 65)])
def test_a_column_at_plus_ninety_stays_finite(V, R):
    g = torch.Generator().manual_seed(V - R)
    x = torch.randn(R, V, generator=g)
    x[:, 11] += 90.0
    check_ce(x, labels_for(x, V, R), V, g=1.0)


@pytest.mark.parametrize("R", RS)
def test_scatter_is_exact_and_leaves_other_rows_zero(R):
    g = torch.Generator().manual_seed(R)
    N = R + 9
    src = torch.randn(ops.pad64(R), H, generator=g)
    rows = torch.randperm(N, generator=g)[:R].sort().values
    dst = torch.zeros(N, H, device=DEV)
    ops.lm_scatter_rows(src.to(DEV), rows.to(torch.int32).to(DEV), dst, R)
    want = torch.zeros(N, H)
    want[rows] = src[:R]
    assert torch.equal(dst.cpu(), want)


@pytest.mark.parametrize("V,R", [(130, 5), (200, 64), (192, 65), (130, 65)])
@pytest.mark.parametrize("accumulate", (True, False))
def test_decoder_weight_gradient_lands_on_v_rows_only(V, R, accumulate):
    """dL^T z in the exact regime (integers: the gemm_ref budget at K = Rp is zero), onto a [V, H] target with a sentinel behind it."""
    Rp, Vp = ops.pad64(R), ops.pad64(V)
    G.check_exact(Rp, 15, 15, extra=255)
    dL = torch.zeros(Rp, Vp, dtype=torch.float64)
    dL[:R, :V] = G.ints((R, V), 15, V + R)
    z = G.ints((Rp, H), 15, V + R + 1)
    prev = G.unit_ints((V, H), 255, V + R + 2, 1.0)
    buf = torch.full((V * H + 256,), -777.0)
    buf[:V * H] = prev.flatten().float()
    buf = buf.to(DEV)
    ops.lm_decoder_wgrad(dL.bfloat16().to(DEV), z.bfloat16().to(DEV), buf[:V * H].view(V, H), V, accumulate=accumulate)
    got = buf.cpu().double()
    want = G.ref_tt(dL[:, :V], z) + (prev if accumulate else 0.0)
    assert torch.equal(got[:V * H].view(V, H), want)
    assert bool((got[V * H:] == -777.0).all()), "rows at or past V were written"


def test_add_and_gelu_backward_helpers():
    g = torch.Generator().manual_seed(5)
    for n in (130, 64, 3):                                         # a tail past a multiple of 4, an exact fit, less than one vector
        dst, src = torch.randn(n + 8, generator=g), torch.randn(n + 8, generator=g)
        for acc in (True, False):
            d = dst.clone().to(DEV)
            ops.lm_add(d, src.to(DEV), n, acc)
            want = dst.clone()
            want[:n] = (dst[:n] + src[:n]) if acc else src[:n]
            assert torch.equal(d.cpu(), want)
    dy, pre = torch.randn(65, H, generator=g).bfloat16(), (2.0 * torch.randn(65, H, generator=g)).bfloat16()
    if dy.numel() % 8:
        dy, pre = dy[:64], pre[:64]
    got = ops.lm_gelu_bwd(dy.to(DEV).contiguous(), pre.to(DEV).contiguous()).cpu().double()
    ref = dy.double() * G.gelu_grad64(pre.double())
    # the bf16 store (2^-9 relative, 2^-8 allowed) and the kernels' erf (Abramowitz & Stegun 7.1.26: 1.5e-7 absolute on erf)
    assert bool(((got - ref).abs() <= 2.0 ** -8 * ref.abs() + 4e-7 * dy.double().abs()).all())
