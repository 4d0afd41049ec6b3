"""crct_head_loss_scores / crct_head_loss_variant_scores (-m gpu): the upstream gradients of the answer logits and of the regressed value
enter the head launch itself.  Every output element against the fp64 restatement of tests/score_grad_ref.py at its budgets (2^-16 of
the sum of the absolute terms for fp32, one bf16 step more for bf16, exactly 0 where nothing reaches), on the shapes B 1 / 7 / 300 x
Hb 64 / 1032, with dropout 0 / 0.1 at heads_ref.DROP_SEEDS, both fusions, L1 / SmoothL1, kind_l1 0 / 1, the three upstream kinds of
heads_ref.upstream crossed with {d_logits, d_value, both}, grad_scale 1 and 0.25.  Rows placed on purpose: label -1, every label -1,
needs = 0 under a non-zero d_value, |target| > 1 (the value's upstream still flows), z = 3 (1 - r^2 = 0.0099), ramps that cross 0.
Then the CE and NONE heads with d_logits, the snap with d_value (bit-identical to none), a NULL request (bit-identical to
crct_head_loss / crct_head_loss_variant on every output) and the three refusals.  Every test prints its largest |err| / budget."""
import ctypes as C
from unittest import mock

import pytest
import torch

import heads_ref as H
import score_grad_ref as SG
from test_heads_gpu import _stats_check
from test_kernels_gpu import DEV, L, _head_launch      # noqa: E402  (sets the import path of the package)

pytestmark = pytest.mark.gpu
CE = dict(regressor="ce", values=H.DVQA_FLOATS)
SNAP = dict(regressor="plotqa", values=H.DVQA_FLOATS, snap=1)
NONE = dict(regressor="none", null_reg=True)
OUTPUTS = ("logits", "reg", "stats", "scratch", "d_pt", "d_pv", "d_fh", "d_w_cls", "d_b_cls", "d_w6", "d_b6")


class _ScoresLib(object):
    """The library with crct_head_loss / crct_head_loss_variant routed through the new entry points with one request, so that
    test_kernels_gpu._head_launch -- its buffers, NaN fills and prefill draws -- serves these tests unchanged."""

    def __init__(self, lib, req):
        self._lib, self._req = lib, req

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def crct_head_loss(self, a, stream):
        return self._lib.crct_head_loss_scores(a, self._req, stream)

    def crct_head_loss_variant(self, a, stream):
        return self._lib.crct_head_loss_variant_scores(a, self._req, stream)


def _launch(inp, R, labels, hc, scores="plain", **kw):
    """scores: 'plain' = the old entry points; None = the new ones with a NULL request; (Gl, Gv) host tensors or None = a request."""
    if scores == "plain":
        return _head_launch(inp, R, labels, hc, **kw)
    req, keep = None, []
    if scores is not None:
        sg = L.ScoreGrads()
        for name, t in zip(("d_logits", "d_value"), scores):
            if t is not None:
                keep.append(t.to(DEV).float().contiguous())
                setattr(sg, name, keep[-1].data_ptr())
        req = C.byref(sg)
    with mock.patch.object(L, "load", lambda lib=L.load(): _ScoresLib(lib, req)):
        return _head_launch(inp, R, labels, hc, **kw)


def _same_bits(a, b, what, keys=OUTPUTS):
    for k in keys:
        if k in a or k in b:
            x, y = a[k], b[k]
            assert torch.equal(x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32),
                               y.view(torch.int16 if y.dtype == torch.bfloat16 else torch.int32)), "%s: %s differs" % (what, k)


def _setup(B, Hb, i):
    fusion_sum, p, use_l1, kind_l1, up, gs, lab_kind = SG.COMBOS[i]
    inp = SG.inputs(B, Hb, seed=B * 11 + Hb)
    hc = H.head_cfg(p=p, seed=H.DROP_SEEDS[i % 2] + B, fusion_sum=fusion_sum, use_l1=use_l1, kind_l1=kind_l1)
    R = SG.targets(inp, hc, seed=B)
    labels = H.make_labels(B, torch.Generator().manual_seed(B), lab_kind)
    return inp, hc, R, labels, H.host_keep(hc, B, Hb), H.upstream(up, B, gs), gs


def _dl64(ref, labels, gn64, Gl, c):
    B = ref["logits"].shape[0]
    valid = (labels != -1).double()[:, None]
    onehot = torch.nn.functional.one_hot(labels.clamp_min(0), 2).double()
    dl = (torch.softmax(ref["logits"], 1) - onehot) * valid * gn64 / max(int(valid.sum()), 1)
    return dl + (c * Gl.double() if Gl is not None else torch.zeros(B, 2, dtype=torch.float64))


def _fail(failed):
    assert not failed, failed


@pytest.mark.parametrize("B,Hb", SG.SHAPES)
def test_plotqa_head_with_score_gradients_against_fp64(B, Hb):
    """crct_head_loss_scores: logits, the five reg rows, stats (counts exact), dlogit0 / dlogit1 / dz of the scratch rows, the three bf16
    seeds and the four parameter gradients over a 0.3 randn prefill.  dz of the z = 3 row is held through d_fus_h, d_w_f6 and d_b_f6
    and not by itself: there the fp32 rounding of tanhf and of r^2 (about 1.5e-7 of 1) is already 2^-16 of 1 - r^2."""
    worst = {}
    for i in range(len(SG.COMBOS)):
        inp, hc, R, labels, keep, (g_loss, g_nsp, g_reg, gn64, gr64), gs = _setup(B, Hb, i)
        kinds, needs = inp["kinds"], R[:, 1] == 1
        for which in SG.WHICH:
            Gl, Gv = SG.score_upstream(B, which)
            out = _launch(inp, R, labels, hc, scores=(Gl, Gv), g_loss=g_loss, g_nsp=g_nsp, g_reg=g_reg, grad_scale=gs, prefill=0.3)
            ref, grads, mags = SG.plotqa_ref64(inp, R, labels, keep, hc, g_nsp=gn64, g_reg=gr64, Gl=Gl, Gv=Gv, c=gs)
            what = "B=%d Hb=%d combo %d %s" % (B, Hb, i, which)
            H.assert_within(out["logits"], ref["logits"], ref["logit_mag"], what + ": logits", worst=worst)
            for k in range(5):
                H.assert_within(out["reg"][k], ref["reg"][k], mags["reg"][k], what + ": reg[%d]" % k, worst=worst)
            _stats_check(out, ref, what, worst)
            H.assert_within(out["scratch"][:, :2], _dl64(ref, labels, gn64, Gl, gs), mags["dl"], what + ": dlogits", worst=worst)
            rows = torch.arange(B) != SG.BIG_ROW
            H.assert_within(out["scratch"][rows, 2], grads["dz"][rows], mags["dz"][rows], what + ": dz", worst=worst)
            _fail(SG.check_grads(out, grads, mags, out["prefill"], what, worst))
            assert float(out["reg"][0][~needs].abs().max() if bool((~needs).any()) else 0.0) == 0.0
            if bool((~needs).any()):                # needs = 0 under a non-zero d_value: nothing reaches the row
                assert float(out["scratch"][~needs, 2].abs().max()) == 0.0 and float(out["d_fh"][~needs].float().abs().max()) == 0.0
            big = (kinds == H._S_BIG) & needs
            if Gv is not None and bool(big.any()) and not hc["kind_l1"]:
                assert float(out["reg"][1][big].abs().max()) == 0.0 and float(out["scratch"][big, 2].abs().min()) > 0.0, what + ": |target| > 1"
            if SG.COMBOS[i][6] == "all_ignored" and Gl is not None:
                assert float(out["stats"][1]) == 0.0 and int(out["stats"][6]) == 0
                assert torch.equal(out["scratch"][:, :2], (torch.tensor(gs) * Gl).float()), what + ": the upstream is the whole seed"
    print("PlotQA head + scores B=%d Hb=%d worst |err| / budget: " % (B, Hb) + " ".join("%s %.4f" % kv for kv in sorted(worst.items())))


@pytest.mark.parametrize("B,Hb", [(7, 1032), (300, 64)])
def test_ce_and_none_heads_take_d_logits(B, Hb):
    """head_ce_rows_kernel and head_rows_kernel<HEAD_NONE> with d_logits: the classification half against fp64; everything of the
    regressor (reg, stats, ce_scratch, d_fus_h, the ce_fusion.6 gradients) bit-identical to the launch without a request."""
    worst = {}
    cinp, Rc = H.ce_inputs(B, Hb, seed=B * 7 + Hb)
    ninp = SG.inputs(B, Hb, seed=B * 11 + Hb)
    for i in range(len(SG.COMBOS)):
        fusion_sum, p, _, _, up, gs, lab_kind = SG.COMBOS[i]
        hc = H.head_cfg(p=p, seed=H.DROP_SEEDS[i % 2] + B, fusion_sum=fusion_sum)
        labels = H.make_labels(B, torch.Generator().manual_seed(B), lab_kind)
        keep = H.host_keep(hc, B, Hb)
        g_loss, g_nsp, g_reg, gn64, gr64 = H.upstream(up, B, gs)
        Gl, _ = SG.score_upstream(B, "logits")
        kw = dict(g_loss=g_loss, g_nsp=g_nsp, g_reg=g_reg, grad_scale=gs, prefill=0.3)
        cls_keys = ("d_pt", "d_pv", "d_w_cls", "d_b_cls")
        # CE
        out = _launch(cinp, Rc, labels, hc, scores=(Gl, None), variant=CE, **kw)
        base = _launch(cinp, Rc, labels, hc, variant=CE, **kw)
        ref, grads, mags = SG.ce_ref64(cinp, Rc, labels, keep, hc, g_nsp=gn64, g_reg=gr64, Gl=Gl, c=gs, values=H.DVQA_FLOATS)
        what = "CE B=%d Hb=%d combo %d" % (B, Hb, i)
        H.assert_within(out["scratch"][:, :2], _dl64(ref, labels, gn64, Gl, gs), mags["dl"], what + ": dlogits", worst=worst)
        _fail(SG.check_grads(out, grads, mags, out["prefill"], what, worst, keys=cls_keys))
        _same_bits(out, base, what, keys=("logits", "reg", "stats", "ce", "d_fh", "d_w6", "d_b6"))
        assert not torch.equal(out["d_pt"], base["d_pt"])
        # NONE
        Rn = SG.targets(ninp, hc, seed=B)
        out = _launch(ninp, Rn, labels, hc, scores=(Gl, None), variant=NONE, **kw)
        base = _launch(ninp, Rn, labels, hc, variant=NONE, **kw)
        ref, grads, mags = SG.none_ref64(ninp, Rn, labels, keep, hc, g_nsp=gn64, Gl=Gl, c=gs)
        what = "NONE B=%d Hb=%d combo %d" % (B, Hb, i)
        H.assert_within(out["scratch"][:, :2], _dl64(ref, labels, gn64, Gl, gs), mags["dl"], what + ": dlogits", worst=worst)
        _fail(SG.check_grads(out, grads, mags, out["prefill"], what, worst, keys=cls_keys))
        _same_bits(out, base, what, keys=("logits", "reg", "stats"))
        assert float(out["scratch"][:, 2].abs().max()) == 0.0
    print("CE / NONE + d_logits B=%d Hb=%d worst |err| / budget: " % (B, Hb) + " ".join("%s %.4f" % kv for kv in sorted(worst.items())))


@pytest.mark.parametrize("B,Hb", [(7, 64), (300, 1032)])
def test_snap_value_is_a_constant_and_a_null_request_changes_nothing(B, Hb):
    """The DVQA evaluation snap with d_value: every output bit-identical to the same launch without it (with and without d_logits), no
    regression gradient at all.  A NULL request, and a request with both members NULL, through the new entry points: every output of
    the PlotQA, snap, CE and NONE heads bit-identical to crct_head_loss / crct_head_loss_variant."""
    inp, hc, R, labels, keep, (g_loss, g_nsp, g_reg, gn64, gr64), gs = _setup(B, Hb, 2)
    kw = dict(g_loss=g_loss, g_nsp=g_nsp, g_reg=g_reg, grad_scale=gs, prefill=0.3)
    Gl, Gv = SG.score_upstream(B, "both")
    for gl in (None, Gl):
        with_v = _launch(inp, R, labels, hc, scores=(gl, Gv), variant=SNAP, **kw)
        without = _launch(inp, R, labels, hc, scores=(gl, None), variant=SNAP, **kw)
        _same_bits(with_v, without, "snap with d_value")
        assert float(with_v["d_fh"].float().abs().max()) == 0.0 and float(with_v["scratch"][:, 2].abs().max()) == 0.0
        assert torch.equal(with_v["d_w6"], with_v["prefill"]["d_w6"]) and torch.equal(with_v["d_b6"], with_v["prefill"]["d_b6"])
    plain = _launch(inp, R, labels, hc, variant=SNAP, **kw)
    assert not torch.equal(with_v["d_pt"], plain["d_pt"])          # d_logits did arrive
    cinp, Rc = H.ce_inputs(B, Hb, seed=B * 7 + Hb)
    for name, xi, xr, var in (("plotqa", inp, R, None), ("plotqa as a variant", inp, R, dict(regressor="plotqa", values=())), ("snap", inp, R, SNAP),
                              ("ce", cinp, Rc, CE), ("none", inp, R, NONE)):
        old = _launch(xi, xr, labels, hc, variant=var, **kw)
        for req in (None, (None, None)):
            _same_bits(_launch(xi, xr, labels, hc, scores=req, variant=var, **kw), old, "%s, request %r" % (name, req), keys=OUTPUTS + ("ce",))
        ev = _launch(xi, xr, None, hc, grads=False, variant=var)
        _same_bits(_launch(xi, xr, None, hc, scores=None, grads=False, variant=var), ev, name + ", evaluation", keys=OUTPUTS + ("ce",))


def test_non_finite_upstreams_arrive_in_the_gradients():
    B, Hb = 7, 64
    inp, hc, R, labels, keep, _, gs = _setup(B, Hb, 0)
    Gl, Gv = SG.score_upstream(B, "both")
    Gl[1, 0], Gv[0] = float("inf"), float("nan")
    out = _launch(inp, R, labels, hc, scores=(Gl, Gv), prefill=0.3)
    assert not bool(torch.isfinite(out["d_pt"][1].float()).all()) and bool(torch.isfinite(out["d_pt"][2].float()).all())
    assert bool(torch.isnan(out["d_fh"][0].float()).any()) and bool(torch.isfinite(out["d_fh"][2].float()).all())
    assert not bool(torch.isfinite(out["d_w_cls"]).all()) and bool(torch.isnan(out["d_b6"]).all())
    assert bool(torch.isfinite(out["logits"]).all()) and bool(torch.isfinite(out["stats"][:17]).all())


def test_the_three_refusals():
    """d_value with the CE regressor and without a regressor, and a request on a launch without gradient outputs."""
    B, Hb = 7, 64
    inp, hc, R, labels, keep, _, gs = _setup(B, Hb, 0)
    cinp, Rc = H.ce_inputs(B, Hb, seed=1)
    Gl, Gv = SG.score_upstream(B, "both")
    with pytest.raises(RuntimeError, match="d_value"):
        _launch(cinp, Rc, labels, hc, scores=(Gl, Gv), variant=CE)
    with pytest.raises(RuntimeError, match="d_value"):
        _launch(inp, R, labels, hc, scores=(None, Gv), variant=NONE)
    for var in (None, CE):
        with pytest.raises(RuntimeError, match="gradient outputs"):
            _launch(cinp if var else inp, Rc if var else R, labels, hc, scores=(Gl, None), grads=False, variant=var)
