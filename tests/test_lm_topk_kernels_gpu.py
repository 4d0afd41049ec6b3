"""``lm_topk_rows`` and ``lm_scores_grad_pack`` (csrc/lm_head.hip) on their own (-m gpu).

Top-k: V = 64 (an exact fit: no pad column, one float4 per thread at most), 130 (a tail of 2 past a multiple of 4 and of 64) and the BERT
vocabulary 30522 (120 columns per thread, padded to 30528) with R = 1, 5, 70 rows (30522: 5 rows), k = 1, 5, 8, ld = pad64(V), the pad
columns filled with +inf and NaN.  Every row content -- random normal, four distinct values with both zeros among them (ties everywhere),
all equal, a third of the entries -inf, one NaN -- runs at every (V, R); the labels cycle over column 0, column V - 1 and the first and the
last column of a tie group.  ``ids`` and ``label_rank`` are exactly those of tests/lm_scores_ref.py's order on the device's own fp32 logits;
``lse`` holds the bits of ``ops.lm_ce_fwd``'s; bounds against fp64, from tests/test_lm_head_kernels_gpu.py:

    |lse - ref|                         <= B = (V + 8) 2^-24 + 2^-22 (|max| + |lse|)
    |logprob - ref|, |label_logprob - ref| <= B + 2^-23 |ref|                          one more subtraction

A row with a NaN has lse = NaN in fp64 too (NaN there, and NaN for every log-probability); a -inf entry has log-probability -inf exactly.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lm_scores_ref as SR                         # noqa: E402
from crct import lib as L                          # noqa: E402
from crct import ops                               # noqa: E402

DEV = torch.device("cuda:0")
CASES = [(V, R) for V in (64, 130) for R in (1, 5, 70)] + [(30522, 5)]
KINDS = ("normal", "four_values", "all_equal", "neg_inf", "one_nan")
KS = (1, 5, 8)


def rows_of(kind, R, V, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, V, generator=g) * 3.0
    if kind == "four_values":
        x = torch.tensor([-1.5, -0.0, 0.0, 2.0])[torch.randint(0, 4, (R, V), generator=g)]
    elif kind == "all_equal":
        x = torch.full((R, V), 0.25)
    elif kind == "neg_inf":
        x[torch.rand(R, V, generator=g) < 1.0 / 3.0] = float("-inf")
        x[:, 9] = 1.0                                                # never a whole row
    elif kind == "one_nan":
        x[torch.arange(R), (7 * torch.arange(R) + 3) % V] = float("nan")
    return x.float()


def labels_of(x):
    """Row r: column 0, column V - 1, the first and the last column that holds the value of column (5 r + 1) % V, in turn."""
    R, V = x.shape
    key = SR.order_key(x.numpy())
    lab = []
    for r in range(R):
        group = np.nonzero(key[r] == key[r, (5 * r + 1) % V])[0]
        lab.append((0, V - 1, int(group[0]), int(group[-1]))[r % 4] if R > 1 else int(group[-1]))
    return torch.tensor(lab, dtype=torch.int64)


def padded(x, ld):
    buf = torch.empty(x.shape[0], ld)
    buf[:, 0::2], buf[:, 1::2] = float("inf"), float("nan")
    buf[:, :x.shape[1]] = x
    return buf


def close(got, ref, bound):
    """|got - ref| <= bound where ref is finite; the same infinity, or NaN for NaN, elsewhere."""
    got, ref = got.double(), ref.double()
    fin = torch.isfinite(ref)
    ok = torch.where(fin, (got - ref).abs() <= bound, (got == ref) | (torch.isnan(got) & torch.isnan(ref)))
    return bool(ok.all())


def bits(t):
    return t.contiguous().view(torch.uint8)


@pytest.mark.parametrize("V,R", CASES)
def test_topk_rows_is_the_reference_order_with_the_cross_entropy_kernels_lse(V, R):
    ld = ops.pad64(V)
    for n, kind in enumerate(KINDS):
        x = rows_of(kind, R, V, seed=V * 31 + R * 7 + n)
        lab = labels_of(x)
        buf = padded(x, ld).to(DEV)
        lab32 = lab.to(torch.int32).to(DEV)
        assert torch.equal(bits(buf[:, :V].cpu()), bits(x))                                  # the device's own logits are these
        xn, xd = x.numpy(), x.double()
        ce_lse = ops.lm_ce_fwd(buf, lab32, R, V, 1.0 / R)[1]
        ref_lse = torch.logsumexp(xd, 1)
        has_nan = torch.isnan(xd).any(1)
        vmax = torch.where(torch.isnan(xd), torch.full_like(xd, -float("inf")), xd).max(1).values
        B = (V + 8) * 2.0 ** -24 + 2.0 ** -22 * (vmax.abs() + ref_lse.abs())
        B = torch.where(has_nan, torch.zeros_like(B), B)
        want_rank = SR.label_rank(xn, lab.numpy())
        outs = {}
        for k in KS:
            ids, logprob, lse, lab_lp, lab_rank = outs[k] = ops.lm_topk_rows(buf, R, V, k, lab32)
            again = ops.lm_topk_rows(buf, R, V, k, lab32)
            for a, b in zip(outs[k], again):
                assert torch.equal(bits(a), bits(b)), "second launch differs (%s, k=%d)" % (kind, k)
            assert ids.dtype == torch.int32 and tuple(ids.shape) == (R, k) and tuple(logprob.shape) == (R, k) and lab_rank.dtype == torch.int32
            want_ids = SR.topk_ids(xn, k)
            assert np.array_equal(ids.cpu().numpy(), want_ids), (kind, k)
            assert np.array_equal(lab_rank.cpu().numpy(), want_rank), (kind, k)
            assert torch.equal(bits(lse), bits(ce_lse)), "lse is not lm_ce_fwd's (%s, k=%d)" % (kind, k)
            assert close(lse.cpu(), ref_lse, B), (kind, k)
            assert bool((torch.isnan(lse.cpu()) == has_nan).all())
            ref_lp = torch.gather(xd, 1, torch.from_numpy(want_ids)) - ref_lse[:, None]
            assert close(logprob.cpu(), ref_lp, B[:, None] + 2.0 ** -23 * ref_lp.abs().nan_to_num(0.0, 0.0, 0.0)), (kind, k)
            ref_ll = xd[torch.arange(R), lab] - ref_lse
            assert close(lab_lp.cpu(), ref_ll, B + 2.0 ** -23 * ref_ll.abs().nan_to_num(0.0, 0.0, 0.0)), (kind, k)
            # without labels: the same ids, log-probabilities and lse, and no label outputs
            bare = ops.lm_topk_rows(buf, R, V, k)
            assert bare[3] is None and bare[4] is None
            for a, b in zip(outs[k][:3], bare[:3]):
                assert torch.equal(bits(a), bits(b))
        for small in (1, 5):                                                                 # the common prefix of k = 1, 5, 8
            assert torch.equal(outs[8][0][:, :small], outs[small][0]) and torch.equal(bits(outs[8][1][:, :small]), bits(outs[small][1]))
            for j in (2, 3, 4):
                assert torch.equal(bits(outs[8][j]), bits(outs[small][j]))
        err = (outs[8][2].cpu().double() - ref_lse).abs()
        print("V %d R %d %-11s lse err / bound %.3f" % (V, R, kind, float((err / B)[~has_nan].max()) if bool((~has_nan).any()) else 0.0))


def test_rows_beyond_r_and_a_wider_buffer_are_left_alone():
    """More rows in the buffer than R and ld past pad64(V): only the first R rows are ranked, from their first V columns."""
    V, R = 130, 5
    x = rows_of("normal", R + 3, V, seed=1)
    buf = padded(x, 256).to(DEV)
    ids, logprob, lse, _, _ = ops.lm_topk_rows(buf, R, V, 5)
    assert tuple(ids.shape) == (R, 5) and np.array_equal(ids.cpu().numpy(), SR.topk_ids(x[:R].numpy(), 5))
    assert torch.equal(bits(lse), bits(ops.lm_ce_fwd(buf, torch.zeros(R, dtype=torch.int32, device=DEV), R, V, 1.0)[1]))
    empty = ops.lm_topk_rows(buf, 0, V, 5)
    assert tuple(empty[0].shape) == (0, 5) and tuple(empty[2].shape) == (0,)


def _launches(fn):
    """fn() with every kernel launch of the library counted (crct_prof_enable(2))."""
    lib = L.load()
    torch.cuda.synchronize()
    lib.crct_prof_reset()
    lib.crct_prof_enable(2)
    try:
        fn()
        torch.cuda.synchronize()
        return lib.crct_prof_stamp_count()
    finally:
        lib.crct_prof_enable(0)
        lib.crct_prof_reset()


def test_refusals_come_before_any_launch():
    buf = torch.randn(5, 64, device=DEV)
    assert _launches(lambda: ops.lm_topk_rows(buf, 5, 64, 5)) == 1                           # the counter sees this kernel

    def refused(fn, text):
        def run():
            with pytest.raises(RuntimeError, match=text):
                fn()
        assert _launches(run) == 0
    refused(lambda: ops.lm_topk_rows(buf, 5, 64, 3), "K=3")
    refused(lambda: ops.lm_topk_rows(buf, 5, 4, 5), "V >= K")
    refused(lambda: ops.lm_topk_rows(buf, 5, 7, 8), "V >= K")
    odd = torch.randn(5, 66, device=DEV)
    refused(lambda: ops.lm_topk_rows(odd, 5, 64, 5), "multiple of 4")
    refused(lambda: ops.lm_scores_grad_pack(odd, 5, 64, 64, 64, 1.0), "multiple of 4")


@pytest.mark.parametrize("V,R,ldg", [(64, 1, 64), (130, 5, 132), (130, 70, 192), (200, 70, 200), (30522, 5, 30524)])
def test_scores_grad_pack_is_torchs_cast_with_zero_padding(V, R, ldg):
    """bf16(c * g) against torch's cast of the fp32 product, bit for bit; pad rows and columns +0 by bit pattern; g with a row stride past V
    whose own pad columns hold NaN; sentinels behind the output."""
    c = 0.37
    Rp, Vp = ops.pad64(R), ops.pad64(V)
    g = torch.Generator().manual_seed(V + R)
    src = torch.full((R, ldg), float("nan"))
    src[:, :V] = torch.randn(R, V, generator=g) * 4.0
    src[0, 0], src[R - 1, V - 1] = 3.0e38, -1.0e-40                                          # overflows to inf with c > 1 only; a subnormal
    src = src.to(DEV)
    space = torch.full((Rp * Vp + 512,), 1.5, dtype=torch.bfloat16, device=DEV)
    out = ops.lm_scores_grad_pack(src[:, :V], R, Rp, V, Vp, c, out=space[:Rp * Vp].view(Rp, Vp))
    assert out.data_ptr() == space.data_ptr()
    want = (src[:, :V] * c).bfloat16()
    got = space[:Rp * Vp].view(Rp, Vp)
    assert torch.equal(got[:R, :V].contiguous().view(torch.int16), want.view(torch.int16))
    if Vp > V:
        assert int(got[:, V:].contiguous().view(torch.int16).abs().max()) == 0, "a pad column is not +0"
    if Rp > R:
        assert int(got[R:].contiguous().view(torch.int16).abs().max()) == 0, "a pad row is not +0"
    assert bool((space[Rp * Vp:] == 1.5).all()), "something behind the output was written"
    again = ops.lm_scores_grad_pack(src[:, :V], R, Rp, V, Vp, c)
    assert torch.equal(again.view(torch.int16), got.view(torch.int16))
    neg = ops.lm_scores_grad_pack(src[:, :V], R, Rp, V, Vp, -2.0)                            # c < 0: the pads stay +0, not -0
    assert int(neg[:, V:].contiguous().view(torch.int16).abs().max() if Vp > V else 0) == 0
    assert torch.equal(neg[:R, :V].contiguous().view(torch.int16), (src[:, :V] * -2.0).bfloat16().view(torch.int16))
