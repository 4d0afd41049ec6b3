"""csrc/heads.hip through the C ABI, per element against the fp64 restatements of tests/heads_ref.py: the DVQA cross-entropy head
(head_ce_rows_kernel, head_ce_wgrad_kernel), the evaluation snap and the regressor-less head (head_rows_kernel<HEAD_SNAP / HEAD_NONE>),
the classification half that the source holds twice, and the answer selection (eval_select_kernel).  Bounds: heads_ref's budgets,
2^-16 of the sum of the absolute terms for fp32 outputs (no absolute floor), one bf16 step more for bf16 outputs, exactness for
counts, classes, table values and gathered values.  Every test prints its largest |err| / budget."""
import numpy as np
import pytest
import torch

import heads_ref as H
from test_kernels_gpu import DEV, L, _head_launch      # noqa: E402  (sets the import path of the package)

pytestmark = pytest.mark.gpu
F32 = np.float32
CE = dict(regressor="ce", values=H.DVQA_FLOATS)
ALL = torch.ones


def _cls_check(out, ref, cgrads, inp, labels, keep, hc, gn64, what, worst, grads=True):
    """The classification half of any head kind: logits, the per-row logit gradients (scratch[:, 0:2]), the bf16 seeds of the two
    poolers and the bi_seq_relationship gradients.  mag of dl_j = (softmax_j + [j == label]) g_nsp / n_valid, the two terms of the
    CE gradient; the seeds' and weight gradients' mags are the sums of |terms| built on it."""
    H.assert_within(out["logits"], ref["logits"], ref["logit_mag"], what + ": logits", worst=worst)
    if labels is None:
        assert float(out["scratch"][:, :2].abs().max()) == 0.0
        return
    valid = (labels != -1).double()[:, None]
    sm = torch.softmax(ref["logits"], 1)
    onehot = torch.nn.functional.one_hot(labels.clamp_min(0), 2).double()
    wq = gn64 / max(int(valid.sum()), 1)
    dl = (sm - onehot) * valid * wq
    dl_mag = (sm + onehot) * valid * abs(wq)
    H.assert_within(out["scratch"][:, :2], dl, dl_mag, what + ": dlogits", worst=worst)
    if not grads:
        return
    p = hc["p"]
    fd = (inp["pt"].double() + inp["pv"].double() if hc["fusion_sum"] else inp["pt"].double() * inp["pv"].double()) * keep / (1 - p)
    wa = inp["w_cls"].double().abs()
    df_mag = (dl_mag[:, :1] * wa[0] + dl_mag[:, 1:] * wa[1]) / (1 - p)
    H.assert_within(out["d_pt"], cgrads["d_pt"], df_mag * (1 if hc["fusion_sum"] else inp["pv"].double()), what + ": d_pooled_t", bf16=True, worst=worst)
    H.assert_within(out["d_pv"], cgrads["d_pv"], df_mag * (1 if hc["fusion_sum"] else inp["pt"].double()), what + ": d_pooled_v", bf16=True, worst=worst)
    for k, mag in (("d_w_cls", dl_mag.t() @ fd.abs()), ("d_b_cls", dl_mag.sum(0))):
        pre = out["prefill"][k].double()
        H.assert_within(out[k], pre + cgrads[k], mag + pre.abs(), what + ": " + k, worst=worst)


def _stats_check(out, ref, what, worst):
    st = out["stats"][:17].double()
    assert torch.equal(st[H.STAT_COUNTS], ref["stats"][H.STAT_COUNTS]), (what, st[H.STAT_COUNTS].tolist(), ref["stats"][H.STAT_COUNTS].tolist())
    H.assert_within(st[H.STAT_FLOATS], ref["stats"][H.STAT_FLOATS], ref["stats"][H.STAT_FLOATS].abs(), what + ": stats", worst=worst)


def _ce_check(out, ref, grads, mags, what, worst, with_grads=True):
    reg = out["reg"].double()
    for k in (0, 2, 4):                          # table values and their fp32 differences
        assert torch.equal(reg[k], ref["reg"][k]), "%s: reg[%d] %s" % (what, k, (reg[k] != ref["reg"][k]).nonzero().flatten().tolist()[:8])
    H.assert_within(reg[1], ref["reg"][1], mags["reg1"], what + ": reg[1]", worst=worst)
    H.assert_within(reg[3], ref["reg"][3], mags["reg3"], what + ": reg[3]", worst=worst)
    assert torch.equal(out["scratch"][:, 5] == 1, ref["ok"]) and torch.equal(out["scratch"][:, 6] == 1, ref["ok"]), what + ": right flags"
    H.assert_within(out["ce"], ref["dz"], mags["dz"], what + ": ce_scratch", worst=worst)
    _stats_check(out, ref, what, worst)
    if with_grads:
        H.assert_within(out["d_fh"], grads["d_fh"], mags["d_fh"], what + ": d_fus_h", bf16=True, worst=worst)
        for k in ("d_w6", "d_b6"):
            pre = out["prefill"][k].double()
            H.assert_within(out[k], pre + grads[k], mags[k] + pre.abs(), what + ": " + k, worst=worst)


@pytest.mark.parametrize("B,Hb", H.HEAD_SHAPES)
def test_ce_head_against_fp64(B, Hb):
    """Every output of the CE head (crct_head_loss_variant, regressor CE) for both fusions, p = 0 and 0.1 with the host mask, the three
    upstream-gradient forms with grad_scale != 1, labels with -1 rows and all -1, and the evaluation form.  Rows: right, wrong,
    needs = 0, R = [0, 0, 0, 0], fractional target, target -0.5, an exact argmax tie whose target is the later class; every class is
    a target at B >= 80.  Outputs start NaN, parameter gradients are pre-filled with 0.3 randn."""
    inp, R = H.ce_inputs(B, Hb, seed=B * 7 + Hb)
    worst = {}
    for i, (fusion_sum, p, up, gs, lab_kind) in enumerate(H.COMBOS):
        hc = H.head_cfg(p=p, seed=H.DROP_SEEDS[i % 2] + B, fusion_sum=fusion_sum)
        labels = H.make_labels(B, torch.Generator().manual_seed(B), lab_kind)
        keep = H.host_keep(hc, B, Hb)
        g_loss, g_nsp, g_reg, gn64, gr64 = H.upstream(up, B, gs)
        out = _head_launch(inp, R, labels, hc, g_loss=g_loss, g_nsp=g_nsp, g_reg=g_reg, grad_scale=gs, prefill=0.3, variant=CE)
        ref, grads, mags = H.ce_ref64(inp, R, labels, keep, hc, g_nsp=gn64, g_reg=gr64, values=H.DVQA_FLOATS)
        what = "B=%d Hb=%d combo %d" % (B, Hb, i)
        _cls_check(out, ref, grads, inp, labels, keep, hc, gn64, what, worst)
        _ce_check(out, ref, grads, mags, what, worst)
        for b in inp["tie_rows"]:
            assert float(out["reg"][0][b]) == H.DVQA_FLOATS[H.TIE_A] and float(out["scratch"][b, 5]) == 0.0, what + ": the tie row"
        if lab_kind == "all_ignored":
            st = out["stats"]
            assert float(st[1]) == 0.0 and float(st[10]) == 0.0 and int(st[6]) == 0
        assert B < 7 or 0 < int(out["stats"][4]) < int(out["stats"][3])
    hc = H.head_cfg()
    out = _head_launch(inp, R, None, hc, grads=False, variant=CE)            # evaluation: no labels, NULL gradient pointers
    _, _, _, gn64, gr64 = H.upstream("default", B, 1.0)
    ref, grads, mags = H.ce_ref64(inp, R, None, ALL(B, Hb, dtype=torch.bool), hc, g_nsp=gn64, g_reg=gr64, values=H.DVQA_FLOATS)
    _cls_check(out, ref, grads, inp, None, None, hc, gn64, "eval", worst, grads=False)
    _ce_check(out, ref, grads, mags, "eval", worst, with_grads=False)
    assert float(out["stats"][0]) == 0.0 and float(out["stats"][8]) == 0.0
    print("CE head B=%d Hb=%d worst |err| / budget: " % (B, Hb) + " ".join("%s %.4f" % kv for kv in sorted(worst.items())))


def test_ce_head_refuses_out_of_range_targets():
    """Targets -1, 65, 1e9 and NaN, in a launch of their own: that row's loss is NaN, its d_fus_h and ce_scratch rows exactly 0, the
    ce_fusion.6 gradients bit-equal to those of the same batch with that row's needs cleared, stats[2] NaN; everything else as fp64."""
    B, Hb = 80, 64
    inp, R0 = H.ce_inputs(B, Hb, seed=B * 7 + Hb)
    rows = [b for b in range(B) if inp["kinds"][b] in (H._RIGHT, H._WRONG)][:len(H.BAD_TARGETS)]
    R, R_off = R0.clone(), R0.clone()
    for b, t in zip(rows, H.BAD_TARGETS):
        R[b, 0] = t
        R_off[b, 1] = 0.0
    hc = H.head_cfg()
    labels = H.make_labels(B, torch.Generator().manual_seed(B))
    out = _head_launch(inp, R, labels, hc, prefill=0.3, variant=CE)
    off = _head_launch(inp, R_off, labels, hc, prefill=0.3, variant=CE)
    assert bool(torch.isnan(out["reg"][1][rows]).all()) and bool(torch.isnan(out["stats"][2]))
    assert float(out["d_fh"][rows].float().abs().max()) == 0.0 and float(out["ce"][rows].abs().max()) == 0.0
    assert float(out["reg"][2][rows].abs().max()) == 0.0 and float(out["scratch"][rows, 5:7].abs().max()) == 0.0
    assert torch.equal(out["d_w6"], off["d_w6"]) and torch.equal(out["d_b6"], off["d_b6"])
    assert not torch.equal(out["d_w6"], out["prefill"]["d_w6"])
    _, _, _, gn64, gr64 = H.upstream("default", B, 1.0)
    ref, grads, mags = H.ce_ref64(inp, R, labels, ALL(B, Hb, dtype=torch.bool), hc, g_nsp=gn64, g_reg=gr64, values=H.DVQA_FLOATS)
    worst = {}
    _ce_check(out, ref, grads, mags, "out of range", worst)
    print("CE head, out-of-range targets: " + " ".join("%s %.4f" % kv for kv in sorted(worst.items())))


def test_head_variant_refusals():
    """n_values != 65 and a NULL ce_scratch for the CE regressor, n_values = 0 for the snap."""
    B, Hb = 7, 64
    inp, R = H.ce_inputs(B, Hb, seed=1)
    with pytest.raises(RuntimeError, match="65 table values"):
        _head_launch(inp, R, None, H.head_cfg(), grads=False, variant=dict(regressor="ce", values=H.DVQA_FLOATS[:64]))
    with pytest.raises(RuntimeError, match="ce_scratch"):
        _head_launch(inp, R, None, H.head_cfg(), grads=False, variant=dict(CE, no_ce_scratch=True))
    sinp = H.snap_inputs(B, Hb, seed=1)
    with pytest.raises(RuntimeError, match="value table"):
        _head_launch(sinp, torch.zeros(B, 4), None, H.head_cfg(), grads=False, variant=dict(regressor="plotqa", values=(), snap=1))


# ------------------------------------------------------------------------------------------- snap, NONE
@pytest.mark.parametrize("B,Hb", [(1, 64), (7, 64), (80, 1032), (300, 64)])
def test_snap_against_fp64(B, Hb):
    """head_rows_kernel<HEAD_SNAP> from the kernel's own r (a probe launch: reg[3] depends on neither R nor the table): the DVQA table,
    the same shuffled, tables of one and three entries and four tables with an exact distance tie on one row (either order, at the head of the table
    and inside it: the first entry wins); rows ordinary, needs = 0, target 0 with an r that snaps to 0.0 (both0: right, d5 = 0, where the unsnapped launch says
    wrong) and |target| > 1 with kind_l1 = 0; both loss kinds.  With labels and gradient pointers: no regression gradient at all and
    the PlotQA head's classification gradients."""
    inp = H.snap_inputs(B, Hb, seed=B * 11 + Hb)
    probe = _head_launch(inp, torch.zeros(B, 4), None, H.head_cfg(use_l1=True, kind_l1=True), grads=False)
    r = probe["reg"][3].numpy()
    worst = {}
    probe_R = torch.cat([torch.zeros(B, 1), torch.ones(B, 1), torch.zeros(B, 1), inp["scale"][:, None]], 1)
    tb, tables = H.snap_tables(r, inp)
    sb = F32(inp["scale"][tb])
    for name, table, win in tables:
        var = dict(regressor="plotqa", values=table, snap=1)
        for use_l1, kind_l1 in ((False, False), (True, True)):
            hc = H.head_cfg(use_l1=use_l1, kind_l1=kind_l1)
            rp, _, _ = H.snap_nearest(r, probe_R, table)
            R = H.snap_targets(inp, rp, hc, seed=B)
            out = _head_launch(inp, R, None, hc, grads=False, variant=var)
            ref, _, reg_mag = H.snap_ref64(inp, R, None, ALL(B, Hb, dtype=torch.bool), hc, g_nsp=1.0, r=r, table=table)
            what = "B=%d Hb=%d %s l1=%d" % (B, Hb, name, use_l1)
            if win is not None:
                H.check_tie_table(table, F32(F32(r[tb]) * sb), win)          # both fp32 distances equal, smaller than every other entry's
                assert int(ref["idx"][tb]) == win
                assert float(out["reg"][0][tb]) == float(F32(F32(F32(table[win]) / sb) * sb)), what + ": the later entry of a tie won"
            assert torch.equal(out["reg"][3], probe["reg"][3]), what + ": reg[3] is not the PlotQA launch's"
            for k in range(5):
                H.assert_within(out["reg"][k], ref["reg"][k], reg_mag[k], what + ": reg[%d]" % k, worst=worst)
            tail = ref["tail"]
            assert torch.equal(out["scratch"][:, 5] == 1, tail["ok5"]) and torch.equal(out["scratch"][:, 6] == 1, tail["okt"]), what
            assert torch.equal(out["scratch"][:, 7] == 1, tail["needs"]) and float(out["scratch"][:, 2].abs().max()) == 0.0
            _stats_check(out, ref, what, worst)
            H.assert_within(out["logits"], ref["logits"], ref["logit_mag"], what + ": logits", worst=worst)
            if name == "dvqa" and B >= 7:
                zr = inp["kinds"] == H._S_SNAP0
                plain = _head_launch(inp, R, None, hc, grads=False)
                assert bool((plain["scratch"][zr, 5] == 0).all()) and bool((out["scratch"][zr, 5] == 1).all())
                assert float(out["reg"][4][zr].abs().max()) == 0.0 and float(out["reg"][0][zr].abs().max()) == 0.0
    # labels and gradient pointers: the snapped value is a constant
    hc = H.head_cfg(p=0.1, seed=H.DROP_SEEDS[0] + B)
    labels = H.make_labels(B, torch.Generator().manual_seed(B))
    rp, _, _ = H.snap_nearest(r, probe_R, H.DVQA_FLOATS)
    R = H.snap_targets(inp, rp, hc, seed=B)
    out = _head_launch(inp, R, labels, hc, prefill=0.3, variant=dict(regressor="plotqa", values=H.DVQA_FLOATS, snap=1))
    plain = _head_launch(inp, R, labels, hc, prefill=0.3)
    assert float(out["d_fh"].float().abs().max()) == 0.0
    assert torch.equal(out["d_w6"], out["prefill"]["d_w6"]) and torch.equal(out["d_b6"], out["prefill"]["d_b6"])
    for k in ("d_pt", "d_pv", "d_w_cls", "d_b_cls", "logits"):
        assert torch.equal(out[k], plain[k]), k
    assert torch.equal(out["reg"][3], plain["reg"][3])
    keep = H.host_keep(hc, B, Hb)
    ref, cgrads, _ = H.snap_ref64(inp, R, labels, keep, hc, g_nsp=1.0, r=r, table=H.DVQA_FLOATS)
    _cls_check(out, ref, cgrads, inp, labels, keep, hc, 1.0, "snap with labels", worst)
    print("snap B=%d Hb=%d worst |err| / budget: " % (B, Hb) + " ".join("%s %.4f" % kv for kv in sorted(worst.items())))


@pytest.mark.parametrize("B,Hb", [(7, 64), (300, 1032)])
def test_none_head_against_fp64(B, Hb):
    """head_rows_kernel<HEAD_NONE>: reg all zero, the needs count in stats[3] / stats[14], the other regression stats 0, the
    classification half as fp64; fus_h / w_f6 / b_f6 and their gradient pointers NULL once, sentinel-filled once (untouched)."""
    inp = H.snap_inputs(B, Hb, seed=B * 13 + Hb)
    R = H.snap_targets(inp, H.emu_tanh_r(inp), H.head_cfg(), seed=B)
    assert set(R[:, 1].tolist()) == {0.0, 1.0}
    hc = H.head_cfg(p=0.1, seed=H.DROP_SEEDS[1] + B, fusion_sum=1)
    labels = H.make_labels(B, torch.Generator().manual_seed(B))
    keep = H.host_keep(hc, B, Hb)
    g_nsp = torch.tensor([1.3])
    ref, cgrads = H.none_ref64(inp, R, labels, keep, hc, g_nsp=float(F32(1.3)) * 0.5)
    worst = {}
    sent = -1.5 * 2.0 ** 100
    for var in (dict(regressor="none", null_reg=True), dict(regressor="none", sentinel=sent)):
        out = _head_launch(inp, R, labels, hc, g_nsp=g_nsp, g_reg=torch.linspace(-0.5, 1.5, B), grad_scale=0.5, prefill=0.3, variant=var)
        assert float(out["reg"].abs().max()) == 0.0
        _stats_check(out, ref, "none", worst)
        n = int((R[:, 1] == 1).sum())
        assert float(out["stats"][3]) == n == float(out["stats"][14]) and float(out["stats"][[2, 4, 5, 11, 12, 15, 16]].abs().max()) == 0.0
        assert torch.equal(out["scratch"][:, 7] == 1, R[:, 1] == 1) and float(out["scratch"][:, [2, 5, 6]].abs().max()) == 0.0
        _cls_check(out, ref, cgrads, inp, labels, keep, hc, float(F32(1.3)) * 0.5, "none", worst)
        if "sentinel" in var:
            for k in ("d_fh", "d_w6", "d_b6"):
                assert bool((out[k].float() == sent).all()), k + " was written"
    print("NONE B=%d Hb=%d worst |err| / budget: " % (B, Hb) + " ".join("%s %.4f" % kv for kv in sorted(worst.items())))


# ------------------------------------------------------------------------------------------- one classification half
SHARED = ("logits", "d_pt", "d_pv", "d_w_cls", "d_b_cls")


@pytest.mark.parametrize("B,Hb", [(7, 1032), (300, 64)])
def test_the_four_head_kinds_share_one_classification_half(B, Hb):
    """head_rows_kernel and head_ce_rows_kernel each hold the logits, NSP terms, dropout mask and pooler seeds: CE, SNAP, NONE and
    crct_head_loss on the same inputs (p = 0.1, both fusions, g_nsp_dev given) agree bit for bit in logits, d_pooled_t / _v, d_w_cls,
    d_b_cls, scratch[:, 0:2] and stats[1, 6, 10]; the zeros of the CE kernel's d_pooled_t are the host mask."""
    cinp, Rc = H.ce_inputs(B, Hb, seed=B + Hb)
    sinp = H.snap_inputs(B, Hb, seed=B + Hb)
    for k in ("pt", "pv"):                       # strictly positive pooler outputs, a valid label on every row: no other zero
        cinp[k] = (cinp[k].float().abs() + 0.05).to(torch.bfloat16)
    sinp.update({k: cinp[k] for k in ("pt", "pv", "w_cls", "b_cls")})
    Rs = H.snap_targets(sinp, H.emu_tanh_r(sinp), H.head_cfg(), seed=B)
    labels = torch.arange(B) % 2
    for fusion_sum in (0, 1):
        hc = H.head_cfg(p=0.1, seed=H.DROP_SEEDS[fusion_sum] + B, fusion_sum=fusion_sum)
        kw = dict(g_nsp=torch.tensor([1.3]), g_reg=torch.linspace(-0.5, 1.5, B), grad_scale=0.5, prefill=0.3)
        outs = dict(ce=_head_launch(cinp, Rc, labels, hc, variant=CE, **kw),
                    snap=_head_launch(sinp, Rs, labels, hc, variant=dict(regressor="plotqa", values=H.DVQA_FLOATS, snap=1), **kw),
                    none=_head_launch(sinp, Rs, labels, hc, variant=dict(regressor="none", null_reg=True), **kw),
                    plotqa=_head_launch(sinp, Rs, labels, hc, **kw))
        base = outs["plotqa"]
        assert float(base["d_w_cls"].abs().max()) > 0 and not bool(torch.isnan(base["logits"]).any())
        for name in ("ce", "snap", "none"):
            o = outs[name]
            for k in SHARED:
                assert torch.equal(o[k], base[k]), "%s differs from crct_head_loss in %s (fusion_sum %d)" % (name, k, fusion_sum)
            assert torch.equal(o["scratch"][:, :2], base["scratch"][:, :2]), name
            assert torch.equal(o["stats"][[1, 6, 10]], base["stats"][[1, 6, 10]]), name
        keep = H.host_keep(hc, B, Hb)
        assert torch.equal(outs["ce"]["d_pt"] != 0, keep), int(((outs["ce"]["d_pt"] != 0) != keep).sum())
        assert torch.equal(outs["ce"]["d_pv"] != 0, keep)


# ------------------------------------------------------------------------------------------- answer selection
SENT = -1.5 * 2.0 ** 100


def _select(logits, reg_out, reg_err, reg_terr, num_ans, forced=None, N=None, prob0=True):
    """crct_eval_select called directly; N may be smaller than the rows the questions claim.  Outputs start as sentinels."""
    d = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dt).contiguous()      # noqa: E731
    rows = logits.shape[0]
    N = rows if N is None else N
    lg, ro, re_, rt = d(logits, torch.float32), d(reg_out, torch.float32), d(reg_err, torch.float32), d(reg_terr, torch.float32)
    na = d(num_ans, torch.int64)
    fz = d(forced, torch.int64) if forced is not None else None
    Q = na.numel()
    ans = torch.full((Q,), -77, dtype=torch.int64, device=DEV)
    so, se, st = (torch.full((Q,), SENT, device=DEV) for _ in range(3))
    p0 = torch.full((max(rows, 1),), SENT, device=DEV) if prob0 else None
    L.check(L.load().crct_eval_select(L.ptr(lg), L.ptr(ro), L.ptr(re_), L.ptr(rt), L.ptr(na), L.ptr(fz), Q, N, L.ptr(p0), L.ptr(ans),
                                      L.ptr(so), L.ptr(se), L.ptr(st), L.current_stream()), "eval_select")
    torch.cuda.synchronize()
    return ans.cpu().numpy(), so.cpu().numpy(), se.cpu().numpy(), st.cpu().numpy(), (p0.cpu().numpy()[:rows] if prob0 else None)


def _select_check(got, kw, what, worst):
    ref = H.select_ref64(**kw)
    for a, b, n in zip(got[:4], ref[:4], ("answers", "sel_out", "sel_err", "sel_terr")):
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, "%s: %s differs at questions %s: got %s, expected %s" % (what, n, bad[:6].tolist(), a[bad[:6]].tolist(), b[bad[:6]].tolist())
    p, p64 = got[4].astype(np.float64), ref[4]
    lg = np.asarray(kw["logits"], np.float64)
    N = kw.get("N", lg.shape[0])
    owned = np.arange(lg.shape[0]) < min(N, int(np.sum(kw["num_ans"])))
    assert np.all(got[4][~owned] == F32(SENT)), what + ": prob0 written on rows no question owns"
    d = lg[:, 0] - lg[:, 1]
    drawn = owned & (np.abs(d) <= 6)
    rel = np.abs(p[drawn] - p64[drawn]) / (2.0 ** -20 * p64[drawn])
    worst["prob0"] = max(worst.get("prob0", 0.0), float(rel.max()) if rel.size else 0.0)
    assert np.all(rel <= 1.0), what + ": prob0 %.3g of its budget" % float(rel.max())
    assert np.all(p[owned & (d >= 40)] == 1.0) and np.all(p[owned & (d <= -120)] == 0.0), what
    nan = owned & np.isnan(d)
    assert np.all(np.isnan(p[nan])), what


def test_eval_select_one_question():
    case = H.select_inputs(1, seed=1)
    kw = dict(logits=case["logits"], reg_out=case["reg_out"], reg_err=case["reg_err"], reg_terr=case["reg_terr"], num_ans=case["num_ans"])
    worst = {}
    _select_check(_select(**kw), kw, "Q=1", worst)
    assert _select(prob0=False, **kw)[0].tolist() == [0]


def test_eval_select_against_fp64():
    """Q = 150 questions of 0, 1, 2, 63, 64, 65 and 200 candidates (the offset sum strides, a lane holds up to four rows): answers and
    the three gathered values exactly, prob0 within 2^-20 relative.  Ties (bit-exact and shifted copies of the best row in the same
    lane, the next lane, and before it), questions saturated at p0 = 1 and p0 = 0, NaN scores (the first NaN row is the answer, as for
    torch.argmax: one NaN row that is not the numeric best, every row NaN, NaN rows in the same and in an earlier lane), N smaller than
    the rows the questions claim (a straddling question, questions wholly beyond N), forced answers in range, equal to n, -1 and on
    empty questions, and prob0 = NULL."""
    case = H.select_inputs(150, seed=150)
    worst = {}
    for v in H.select_variants(case):
        name, kw = v[0], v[1]
        got = _select(**kw)
        _select_check(got, kw, name, worst)
        if name == "nan":
            for q, a in v[2].items():
                assert int(got[0][q]) == a
        if name == "forced":
            assert np.array_equal(got[0], kw["forced"])
        if name == "short_N":
            N = kw["N"]
            offs = np.concatenate([[0], np.cumsum(case["num_ans"])])
            beyond = [q for q in range(150) if offs[q] >= N and case["num_ans"][q] > 0]
            assert beyond and all(got[0][q] == 0 and got[1][q] == 0 and np.isposinf(got[2][q]) and np.isposinf(got[3][q]) for q in beyond)
        if name == "plain":
            null = _select(prob0=False, **kw)
            assert all(np.array_equal(a, b) for a, b in zip(null[:4], got[:4]))
            for kind, (q, j) in case["special"].items():
                assert int(got[0][q]) == j, kind
    print("eval_select worst |err| / budget: prob0 %.4f" % worst["prob0"])
