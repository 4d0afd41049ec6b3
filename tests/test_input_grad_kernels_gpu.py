"""The two kernels behind the input gradients (-m gpu), through crct.ops, per element against fp64 from their own inputs with the budgets of
tests/input_grad_ref.py (ratio <= 1; tests/test_input_grad_ref_cpu.py shows what the budgets admit and what they refuse).

  crct_softmax_bwd_rows     (M, F) = (1, 32) below one wave's vector width, (111, 1024) and (74, 2048) the project's widths in more than
                            one workgroup, (5, 36) a multiple of 4 only; fp32 and bf16 features; an almost one-hot row and a constant row
  crct_embed_input_grad     (M, H) = (1, 64), (111, 1024), (93, 768), (7, 96); p = 0 and 0.1 with the kernel's own mask (dropout_ref);
                            every combination of NULL outputs leaves the other outputs' bits alone; text rows without a box get an exact 0;
                            two runs give the same bits; d_sum rounded to bf16 is the d_sum crct_embed_image_bwd stores, bit for bit
"""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

import input_grad_ref as IG                         # noqa: E402
from crct import lib as L                          # noqa: E402
from crct import ops                               # noqa: E402

DEV = torch.device("cuda:0")


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", IG.SOFTMAX_CASES, ids=lambda c: "M%d_F%d" % c)
def test_softmax_backward_rows_match_fp64(case, bf16):
    """Worst ratios measured on MI355X: 0.001 - 0.018 over the eight cases (the budget carries the project's fp32 slack of 2^-16; the CPU
    emulator reads the same)."""
    x, g = IG.softmax_case(*case, bf16)
    ref, bud = IG.softmax_bwd_reference(x, g), IG.softmax_bwd_budget(x, g)
    xd = x.to(DEV, torch.bfloat16 if bf16 else torch.float32)
    got = ops.softmax_bwd_rows(xd, g.to(DEV))
    again = ops.softmax_bwd_rows(xd, g.to(DEV))
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == case and bool(torch.isfinite(got).all())
    r = IG.ratio(got, ref, bud)
    print("softmax backward", case, "bf16" if bf16 else "f32", "worst ratio %.3f" % float(r.max()))
    assert float(r.max()) <= 1.0, (case, bf16, float(r.max()), int((r > 1).sum()))
    assert torch.equal(got, again)
    # the kernel's rows sum to zero as far as fp32 sums of their terms can
    scale = (torch.softmax(x.double(), -1) * g.double().abs()).sum(-1)
    assert float((got.double().cpu().sum(-1).abs() / scale).max()) <= 2.0 ** -16


def test_softmax_backward_refuses_a_width_that_is_no_multiple_of_four():
    x = torch.zeros(2, 6, device=DEV)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.softmax_bwd_rows(x, torch.zeros(2, 6, device=DEV))


def _image_bwd_dsum(c, M, H):
    """The bf16 d_sum crct_embed_image_bwd stores for the same dy / sum / statistics / gamma / mask."""
    lib = L.load()
    d = lambda t: t.to(DEV).contiguous()
    nblk = lib.crct_layernorm_bwd_blocks(M)
    n_color = 5
    out = {k: torch.zeros(s, device=DEV) for k, s in dict(color=(n_color, H), w_loc=(H, 4), b_loc=(H,), b_img=(H,), gamma=(H,), beta=(H,)).items()}
    d_sum = torch.empty(M, H, device=DEV, dtype=torch.bfloat16)
    partials = torch.empty(7 * 4 * nblk * H, device=DEV)
    idx = torch.empty(M, dtype=torch.int32, device=DEV)
    rows = torch.empty(M, H, device=DEV)
    target = torch.zeros(M, dtype=torch.int64, device=DEV)
    dy, x, mean, rstd, gamma, loc = d(c["dy"]), d(c["x"]), d(c["mean"]), d(c["rstd"]), d(c["gamma"]), d(c["loc"])
    thr = L.drop_threshold(c["p"])
    L.check(lib.crct_embed_image_bwd(dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), loc.data_ptr(), target.data_ptr(),
                                     gamma.data_ptr(), d_sum.data_ptr(), out["color"].data_ptr(), out["w_loc"].data_ptr(), out["b_loc"].data_ptr(),
                                     out["b_img"].data_ptr(), out["gamma"].data_ptr(), out["beta"].data_ptr(), partials.data_ptr(), M, H,
                                     thr, 1.0 / (1.0 - c["p"]) if thr else 1.0, IG.ROW_SITE, IG.ROW_SEED, rows.data_ptr(), idx.data_ptr(),
                                     n_color, L.current_stream()), "embed_image_bwd")
    torch.cuda.synchronize()
    return d_sum


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("case", IG.ROW_CASES, ids=lambda c: "M%d_H%d" % c)
def test_embed_input_grad_rows_match_fp64(case, p):
    """Worst ratios measured on MI355X: d_loc and d_areas <= 0.002, d_sum <= 0.204 ((111, 1024) at p = 0.1; <= 0.09 elsewhere)."""
    M, H = case
    c = IG.rows_case(M, H, p)
    args = (c["dy"], c["x"], c["mean"], c["rstd"], c["gamma"], c["keep"], p, c["w_loc"], c["loc"], c["w_areas"])
    ref, bud = IG.rows_reference(*args), IG.rows_budget(*args)
    d = lambda t: t.to(DEV).contiguous()
    dev = dict(dy=d(c["dy"]), sum_saved=d(c["x"]), mean=d(c["mean"]), rstd=d(c["rstd"]), gamma=d(c["gamma"]), loc=d(c["loc"]),
               w_loc=d(c["w_loc"]), w_areas=d(c["w_areas"]))

    def run(want):
        o = ops.embed_input_grad(want=want, p_drop=p, site=IG.ROW_SITE, seed=IG.ROW_SEED, **dev)
        torch.cuda.synchronize()
        return dict(zip(("d_loc", "d_areas", "d_sum"), o))
    full = run(("d_loc", "d_areas", "d_sum"))
    worst = {}
    for k in ("d_loc", "d_areas", "d_sum"):
        assert bool(torch.isfinite(full[k]).all()), k
        r = IG.ratio(full[k], ref[k], bud[k])
        worst[k] = float(r.max())
        assert worst[k] <= 1.0, (case, p, k, worst[k], int((r > 1).sum()))
    print("embed_input_grad", case, p, "worst ratios", {k: round(v, 3) for k, v in worst.items()})
    # text rows without a box: an exact zero
    empty = (c["loc"].abs().sum(-1) == 0).to(DEV)
    assert bool(empty.any()) and float(full["d_loc"][empty].abs().max()) == 0.0
    assert M < 2 or float(full["d_loc"][~empty].abs().max()) > 0.0
    # every combination of NULL outputs (the empty one launches nothing): what is written has the bits of the full call; so has a second run
    for n in range(0, 4):
        for want in itertools.combinations(("d_loc", "d_areas", "d_sum"), n):
            o = run(want)
            for k in ("d_loc", "d_areas", "d_sum"):
                assert (o[k] is None) == (k not in want)
                assert o[k] is None or torch.equal(o[k], full[k]), (want, k)
    # the same arithmetic as the embedding backward: its bf16 d_sum is this row rounded once
    assert torch.equal(full["d_sum"].to(torch.bfloat16), _image_bwd_dsum(c, M, H))


def test_embed_input_grad_without_loc_masks_nothing():
    """Image rows pass no boxes to test against: every row gets its location gradient, the rows a text call would zero included."""
    M, H = 7, 96
    c = IG.rows_case(M, H, 0.0)
    d = lambda t: t.to(DEV).contiguous()
    kw = dict(dy=d(c["dy"]), sum_saved=d(c["x"]), mean=d(c["mean"]), rstd=d(c["rstd"]), gamma=d(c["gamma"]), w_loc=d(c["w_loc"]))
    with_loc = ops.embed_input_grad(want=("d_loc",), loc=d(c["loc"]), **kw)[0]
    without = ops.embed_input_grad(want=("d_loc",), **kw)[0]
    torch.cuda.synchronize()
    empty = (c["loc"].abs().sum(-1) == 0).to(DEV)
    assert torch.equal(with_loc[~empty], without[~empty]) and float(without[empty].abs().min()) > 0.0
    with pytest.raises(RuntimeError, match="w_areas"):
        ops.embed_input_grad(want=("d_areas",), **kw)
