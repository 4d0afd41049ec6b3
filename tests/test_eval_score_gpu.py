"""Evaluation scoring of every dataset on the GPU (-m gpu): ``crct_eval_score`` (selection, flags and the accuracy tables of one
batch in one launch) against the numpy restatement tests/eval_ref.py -- integer and compare work, so everything but the last bit
of prob0 is exact -- and bit for bit against ``crct_eval_select``; ``crct.evaluation.evaluate`` on the DVQA / FigureQA fixtures
(tests/golden/evalscore_*.npz) and on the PlotQA one (tiny_evalscore.npz) against the path of the Python helpers."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import eval_ref as ER                               # noqa: E402
from crct import config as C                        # noqa: E402
from crct import evaluation as EV                   # noqa: E402
from crct import lib as L                           # noqa: E402
from crct import synthetic as S                     # noqa: E402
from test_eval_scoring import _load as load_tiny    # noqa: E402  (tiny_evalscore.npz: z, meta, batches)

DEV = torch.device("cuda:0")
F32 = np.float32
UP = lambda v: np.nextafter(F32(v), F32(np.inf))    # noqa: E731
# relative errors on every histogram edge, just above it, inside every bin, in no bin (0, NaN) and beyond the last
ERRS = np.array([0.0, F32(0.05), UP(0.05), 0.1, UP(0.1), 0.2, UP(0.2), 1.0, UP(1.0), np.inf, np.nan, 0.03, 0.07, 0.12, 0.17, 0.25, 0.3,
                 0.35, 0.45, 0.55, 0.65, 0.75, 0.85, 0.95, 7.0, F32(0.15), UP(0.15), 0.9, UP(0.9)], dtype=F32)
TERRS = np.array([0.005, 0.01, 0.05, 0.1, 0.3, UP(0.05), np.inf], dtype=F32)
TOLS = np.array([0.01, 0.05, 0.2, 0.0], dtype=F32)


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def dev(x, dtype=None):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype)


def run_kernel(case, tables=None, outputs=True):
    """One crct_eval_score call on a case dict (numpy inputs).  Outputs start as sentinels."""
    t = {k: dev(case.get(k)) for k in ("logits", "reg_out", "reg_err", "reg_terr", "num_ans", "forced", "labels", "gt_id", "tolerance", "cats")}
    t["needs_reg"] = dev(case["needs_reg"].astype(np.uint8))
    Q, N = case["Q"], case["N"]
    o = dict(answers=torch.full((Q,), -77, dtype=torch.int64, device=DEV))
    if outputs:
        o.update(sel_out=torch.full((Q,), 123.0, device=DEV), sel_err=torch.full((Q,), 123.0, device=DEV),
                 sel_terr=torch.full((Q,), 123.0, device=DEV), flags=torch.full((Q,), 0xEE, dtype=torch.uint8, device=DEV),
                 prob0=torch.full((N,), -5.0, device=DEV))
    tables = torch.zeros(L.EVAL_TABLE_WORDS, dtype=torch.int64, device=DEV) if tables is None else tables
    a = L.EvalScoreArgs()
    for k, v in list(t.items()) + list(o.items()):
        setattr(a, k, L.ptr(v))
    a.tables, a.N, a.Q, a.mode, a.with_histogram = tables.data_ptr(), N, Q, case["mode"], int(case["with_histogram"])
    L.check(L.load().crct_eval_score(ctypes.byref(a), L.current_stream()), "eval_score")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}, tables


def reference(case, tables=None):
    return ER.score_batch(case["mode"], case["logits"], case.get("reg_out"), case.get("reg_err"), case.get("reg_terr"), case.get("num_ans"),
                          case.get("forced"), case.get("labels"), case["gt_id"], case["needs_reg"], case["tolerance"], case.get("cats"),
                          case["with_histogram"], tables)


def check(case, got, tables, ref):
    for k in ("answers", "flags", "sel_out", "sel_err", "sel_terr"):
        assert np.array_equal(bits(got[k]), bits(ref[k])), (k, got[k], ref[k])
    n = len(ref["prob0"]) if case["mode"] else min(case["N"], int(np.sum(case["num_ans"])))
    assert np.allclose(got["prob0"][:n], ref["prob0"][:n], atol=1e-6, rtol=0, equal_nan=True)      # expf against np.exp: the last bit
    assert (got["prob0"][n:] == -5.0).all()                     # rows no question owns are not written
    assert np.array_equal(tables.cpu().numpy(), ref["tables"]), (tables.cpu().numpy(), ref["tables"])


def common_fields(g, Q):
    needs = g.rand(Q) < 0.6
    c = dict(Q=Q, needs_reg=needs, tolerance=g.choice(TOLS, size=Q).astype(F32), with_histogram=True)
    c["cats"] = np.stack([g.randint(1, 5, size=Q), np.where(needs, 2, g.randint(0, 3, size=Q)), g.randint(0, 3, size=Q)], 1).astype(np.int32)
    return c


def mode0_case(num_ans, seed, short=0):
    """Candidate rows whose p0 differ by more than 1e-4 inside a question: l0 - l1 are distinct multiples of 0.05 within +-3.25
    (sigmoid' >= 0.035 there: neighbours differ by 1.7e-3), so a last-bit difference of expf cannot change a selection."""
    g = np.random.RandomState(seed)
    num_ans = np.asarray(num_ans, dtype=np.int64)
    Q, total = len(num_ans), int(num_ans.sum())
    N = total - short
    l1 = g.uniform(-2, 2, size=total).astype(F32)
    d = np.zeros(total, dtype=F32)
    off = 0
    for n in num_ans:
        d[off:off + n] = (g.permutation(131)[:n] - 65) * F32(0.05)
        off += n
    logits = np.stack([l1 + d, l1], 1).astype(F32)
    c = common_fields(g, Q)
    c.update(mode=0, N=N, num_ans=num_ans, reg_out=g.uniform(-50, 50, size=total).astype(F32), reg_err=g.choice(ERRS, size=total).astype(F32),
             reg_terr=g.choice(TERRS, size=total).astype(F32))
    c["logits_full"] = logits
    return c, g


def finish_mode0(c, g, forced=None):
    """Cut the rows to N, then labels from the expected answers: right on two questions of three."""
    N = c["N"]
    for k in ("reg_out", "reg_err", "reg_terr"):
        c[k] = c[k][:N].copy()
    c["logits"] = c.pop("logits_full")[:N].copy()
    c["forced"] = forced
    c["gt_id"] = np.zeros(c["Q"], dtype=np.int64)
    ans = reference(c)["answers"]
    c["gt_id"] = np.where(np.arange(c["Q"]) % 3 == 2, ans + 1, ans).astype(np.int64)
    return c


def offsets(num_ans):
    return np.concatenate([[0], np.cumsum(num_ans)[:-1]]).astype(np.int64)


MODE0_SHAPES = {
    "q1": [5],
    "q70": ([0, 1, 64, 65, 130, 3, 2] * 10),             # the offset sum takes two lane passes; one, two and three rows per lane
    "mixed": [130, 0, 65, 1, 64, 7, 0, 2],
}


@pytest.mark.parametrize("shape", sorted(MODE0_SHAPES))
def test_mode0_kernel_matches_the_restatement_exactly(shape):
    num_ans = MODE0_SHAPES[shape]
    c, g = mode0_case(num_ans, seed=len(num_ans))
    off = offsets(c["num_ans"])
    lg = c["logits_full"]
    if shape != "q1":
        big = sorted([q for q, n in enumerate(c["num_ans"]) if n >= 64][:3], key=lambda q: -c["num_ans"][q])      # 130, 65, 64 rows
        q = big[0]                                       # first-maximum tie: the same bits on three rows, in three lane passes
        for j in (9 + 64, 9, 1 + 128):
            lg[off[q] + j] = (F32(4.0), F32(0.5))
        q = big[1]                                       # one NaN row wins over every number
        lg[off[q] + 40] = (F32(np.nan), F32(0.0))
        q = big[2]                                       # two NaN rows: the first one
        lg[off[q] + 63] = (F32(0.0), F32(np.nan))
        lg[off[q] + 17] = (F32(np.nan), F32(np.nan))
    c["needs_reg"][0] = False                            # a question that needs no regression, with a non-zero error on every row
    c["reg_err"][off[0]:off[0] + max(int(c["num_ans"][0]), 1)] = F32(0.07)
    c = finish_mode0(c, g)
    ref = reference(c)
    got, tables = run_kernel(c)
    check(c, got, tables, ref)
    if shape != "q1":
        assert ref["answers"][big[0]] == 9 and ref["answers"][big[1]] == 40 and ref["answers"][big[2]] == 17
        assert ref["tables"][ER.HISTOGRAM:ER.HISTOGRAM + 13].any() and ref["tables"][ER.BREAKDOWN:ER.BREAKDOWN + 180].any()
    # a second call into the same tables adds; outputs left NULL are simply not produced
    got2, tables = run_kernel(c, tables=tables, outputs=False)
    assert np.array_equal(got2["answers"], ref["answers"])
    assert np.array_equal(tables.cpu().numpy(), 2 * ref["tables"])
    # without a histogram and without categories: only the totals
    c2 = dict(c, with_histogram=False, cats=None)
    got3, t3 = run_kernel(c2)
    ref3 = reference(c2)
    check(c2, got3, t3, ref3)
    assert not ref3["tables"][ER.BREAKDOWN:].any() and np.array_equal(ref3["tables"][:12], ref["tables"][:12])


@pytest.mark.parametrize("what", ["forced", "short", "short_forced"])
def test_mode0_forced_answers_and_missing_rows(what):
    num_ans = MODE0_SHAPES["mixed"] + [3, 70, 4]
    c, g = mode0_case(num_ans, seed=11, short=72 if what != "forced" else 0)      # N ends inside the 70-row question: it and the last have rows beyond N
    forced = None
    if what != "short":
        n = c["num_ans"]
        forced = np.array([3, 0, -1, 0, 64, 7, 5, 1, 2, 69, 0], dtype=np.int64)    # in range; -1; == n (64, 7); > n on an empty question
        assert len(forced) == len(n) and forced[4] == n[4] and forced[5] == n[5]
    c = finish_mode0(c, g, forced)
    ref = reference(c)
    got, tables = run_kernel(c)
    check(c, got, tables, ref)
    if what != "short":
        assert np.isinf(ref["sel_err"][[2, 4, 5, 6]]).all() and (ref["sel_out"][[2, 4, 5, 6]] == 0).all()
    if what == "short":
        assert ref["answers"][-1] == 0 and np.isinf(ref["sel_err"][-1])             # no row below N: answers 0, infinite errors
        assert ref["answers"][-2] in (0, 1)                                           # the partly missing question answers one of its two rows below N
    if what == "short_forced":
        assert np.isinf(ref["sel_err"][-2]) and np.isinf(ref["sel_terr"][-2])         # forced onto a row beyond N


def mode1_case(Q, seed):
    g = np.random.RandomState(seed)
    l1 = g.uniform(-2, 2, size=Q).astype(F32)
    k = g.randint(1, 300, size=Q) * g.choice([-1, 1], size=Q)
    logits = np.stack([l1 + (k * F32(0.01)).astype(F32), l1], 1).astype(F32)          # |l0 - l1| >= 0.01: |p0 - 0.5| >= 2.4e-3
    c = common_fields(g, Q)
    if Q > 3:
        logits[1, 0] = logits[1, 1]                                                    # p0 = 0.5 exactly: answers 0
        logits[Q - 2, 0] = logits[Q - 2, 1] = F32(-1.25)
        logits[2] = (F32(np.nan), F32(0.0))
    c.update(mode=1, N=Q, logits=logits, labels=g.randint(0, 2, size=Q).astype(np.int64), gt_id=g.randint(0, 2, size=Q).astype(np.int64))
    return c


@pytest.mark.parametrize("Q", [1, 64, 65, 300])
def test_mode1_binary_answers_match_the_restatement_exactly(Q):
    c = mode1_case(Q, seed=Q)
    ref = reference(c)
    got, tables = run_kernel(c)
    check(c, got, tables, ref)
    assert (got["sel_out"] == 0).all() and (got["sel_err"] == 0).all() and (got["sel_terr"] == 0).all()
    if Q > 3:
        assert got["prob0"][1] == 0.5 and got["answers"][1] == 0 and got["answers"][Q - 2] == 0
        assert got["answers"][2] == -1 and not got["flags"][2] & 1
        assert set(c["labels"].tolist()) == {0, 1} and set(got["answers"].tolist()) == {-1, 0, 1}
        assert 0 < ref["tables"][0] < Q - 1
    # the regression rows are not read in this mode: the same results with them given
    c2 = dict(c, reg_out=np.full(Q, 3.0, F32), reg_err=np.full(Q, 0.5, F32), reg_terr=np.full(Q, 0.5, F32))
    got2, t2 = run_kernel(c2)
    check(c2, got2, t2, ref)


def test_histogram_edges():
    """One candidate per question, its relative error on / just above every edge: bins are open below and closed above with fp32
    edges, 0 and NaN fall in none, and a question that needs no regression is not counted whatever its error."""
    Q = len(ERRS) + 1
    c, g = mode0_case([1] * Q, seed=2)
    c["reg_err"] = np.concatenate([ERRS, [F32(0.07)]]).astype(F32)
    c["needs_reg"] = np.arange(Q) < Q - 1
    c = finish_mode0(c, g)
    ref = reference(c)
    got, tables = run_kernel(c)
    check(c, got, tables, ref)
    h = tables.cpu().numpy()[ER.HISTOGRAM:ER.HISTOGRAM + 13]
    # by hand: (0, .05] 0.05 0.03 | (.05, .1] 0.05+ 0.1 0.07 | (.1, .15] 0.1+ 0.12 0.15 | (.15, .2] 0.2 0.17 0.15+ | (.2, .3] 0.2+ 0.25 0.3 |
    # 0.35 | 0.45 | 0.55 | 0.65 | 0.75 | 0.85 | (.9, 1] 1.0 0.95 0.9+ | > 1: 1.0+ inf 7.0; 0, NaN and 0.9 -> (.8, .9]
    assert h.tolist() == [2, 3, 3, 3, 3, 1, 1, 1, 1, 1, 2, 3, 3], h
    assert h.sum() == len(ERRS) - 2


def test_out_of_range_categories_are_counted_not_stored():
    c, g = mode0_case([3, 1, 4, 2, 5, 2, 3, 1], seed=4)
    c = finish_mode0(c, g)
    good = reference(c)
    bad = c["cats"].copy()
    bad[1, 0], bad[3, 0], bad[4, 1], bad[6, 2], bad[7, 1] = 0, 5, 3, -1, -1
    cb = dict(c, cats=bad)
    ref = reference(cb)
    got, tables = run_kernel(cb)
    check(cb, got, tables, ref)
    t = tables.cpu().numpy()
    assert t[ER.ERRORS] == 5
    assert t[ER.BREAKDOWN:ER.BREAKDOWN + 180].sum() < good["tables"][ER.BREAKDOWN:ER.BREAKDOWN + 180].sum()
    assert np.array_equal(t[:12], good["tables"][:12]) and np.array_equal(t[ER.HISTOGRAM:ER.HISTOGRAM + 13], good["tables"][ER.HISTOGRAM:ER.HISTOGRAM + 13])
    # every question bad: the breakdown stays untouched
    allbad = dict(c, cats=np.full_like(bad, 7))
    _, t2 = run_kernel(allbad)
    t2 = t2.cpu().numpy()
    assert not t2[ER.BREAKDOWN:ER.BREAKDOWN + 180].any() and t2[ER.ERRORS] == c["Q"]


def _same_as_select(logits, ro, re_, rt, num_ans, forced, batch):
    tables = torch.zeros(L.EVAL_TABLE_WORDS, dtype=torch.int64, device=DEV)
    a1 = EV.select_answers(logits, ro, re_, rt, num_ans, forced)
    ans, so, se, st, flags, p0 = EV.score_batch(logits, ro, re_, rt, batch, tables, forced=forced, want_prob0=True)
    torch.cuda.synchronize()
    for x, y in zip(a1, (ans, so, se, st, p0)):
        x, y = x.cpu().numpy(), y.cpu().numpy()
        assert np.array_equal(bits(x), bits(y)), (x, y)


def test_mode0_equals_eval_select_bit_for_bit():
    for shape in ("q70", "mixed"):
        c, g = mode0_case(MODE0_SHAPES[shape], seed=3)
        off = offsets(c["num_ans"])
        q = [i for i, n in enumerate(c["num_ans"]) if n >= 64][0]
        c["logits_full"][off[q] + 3] = c["logits_full"][off[q] + 50] = (F32(4.0), F32(0.5))
        c["logits_full"][off[q + 2] + 11] = (F32(np.nan), F32(1.0))
        c = finish_mode0(c, g)
        batch = dict(gt_id=torch.from_numpy(c["gt_id"]), needs_reg=torch.from_numpy(c["needs_reg"]), tolerance_margin=torch.from_numpy(c["tolerance"]),
                     num_ans=torch.from_numpy(c["num_ans"]))
        forced = torch.from_numpy(np.where(np.arange(c["Q"]) % 4 == 0, -1, c["gt_id"]))
        for f in (None, forced):
            _same_as_select(dev(c["logits"]), dev(c["reg_out"]), dev(c["reg_err"]), dev(c["reg_terr"]), batch["num_ans"], f, batch)
    z, meta, batches = load_tiny()
    for bi, b in enumerate(batches):
        rows = [dev(z["b%d.%s" % (bi, k)]) for k in ("nsp_scores", "reg0", "reg4", "reg2")]
        for f in (None, b["gt_id"]):
            _same_as_select(rows[0], rows[1], rows[2], rows[3], b["num_ans"], f, b)


# ---------------------------------------------------------------- the loop
class _Dataset(object):
    def __init__(self, ans_type=None):
        self.ans_type = ans_type or {}

    def cut_batch_padding(self, item):
        pass

    def get_ans_type(self, qa_ind):
        return self.ans_type[int(qa_ind)]


def fixture_model(meta):
    """The model of an evalscore_* fixture, as make_golden_evalscore_variants.build makes the reference's: test_eval_scoring.py's
    build_model, then the seeded weights at meta['weight_std'], the widened answer head and the CE bias bump."""
    from test_step_gpu import build_model
    cfg = C.BertConfig.from_dict(meta["cfg"])
    model, params = build_model(cfg, dict(meta["params"]), seed=meta["weight_seed"])
    sd = model.state_dict()
    S.seeded_fill_(sd, base_seed=meta["weight_seed"], std=meta["weight_std"])
    with torch.no_grad():
        sd["bert_pretrained.cls.bi_seq_relationship.weight"].mul_(meta["head_scale"])
        sd["bert_pretrained.cls.bi_seq_relationship.bias"][1] += meta["head_shift"]
        if meta.get("ce_bias_bump"):
            c, v = meta["ce_bias_bump"]
            sd["bert_pretrained.regressor.ce_fusion.6.bias"][c] += v
    model.bert_pretrained._invalidate_shadow()
    params["ddp"] = False
    return model, params


def _own_rows(model, params, batches, ebs):
    model.eval()
    rows = {}
    with torch.no_grad():
        for bi, b in enumerate(batches):
            s, o, e, t = EV.score_rows(model, dict(b), params, ebs)
            rows[bi] = (s.float().cpu().numpy(), o.cpu().numpy(), t.cpu().numpy(), e.cpu().numpy())       # nsp, reg0, reg2, reg4
    model.train()
    return rows


@pytest.mark.parametrize("case", ER.VARIANT_CASES)
def test_evaluate_on_the_variant_fixtures(case):
    z, meta, batches = ER.load_fixture(case)
    model, params = fixture_model(meta)
    ebs = int(z["eval_batch_size"])
    assert model.training
    total, breakdown, hist = EV.evaluate([dict(b) for b in batches], _Dataset(), params, ebs, model)
    assert model.training                                                   # restored (evaluation.py:384)
    assert total.dtype == torch.float64 and breakdown.dtype == torch.float64 and hist.dtype == torch.int64
    assert tuple(total.shape) == (6, 2) and tuple(breakdown.shape) == (5, 4, 3, 3) and tuple(hist.shape) == (13,)
    rows = _own_rows(model, params, batches, ebs)
    tables, _ = ER.fixture_tables(meta, batches, lambda bi, b: rows[bi])
    total = total.cpu().numpy()
    print(case, "total", total.tolist(), "reference", z["total_correct"].tolist())
    assert np.array_equal(total, tables[:12].reshape(6, 2).astype(np.float64)), (total, tables[:12])
    assert float(breakdown.abs().sum()) == 0.0 and int(hist.sum()) == 0     # PlotQA only (evaluation.py:331)
    ref_total = z["total_correct"]
    assert np.array_equal(total[:, 1], ref_total[:, 1])                     # counts are data properties
    assert np.abs(total[:, 0] - ref_total[:, 0]).max() <= 2                 # a bf16 forward may flip a near tie (meta['near_ties'] <= 2)


def _helpers_evaluate(batches, dataset, params, ebs, model, with_histogram=True, forced_mode=False):
    """The loop on the Python helpers (select_answers, correctness, the three reduce_*): the path before crct_eval_score."""
    model.eval()
    dev_ = torch.device(params["device"])
    breakdown = torch.zeros(5, 4, 3, 3, dtype=torch.float64, device=dev_)
    total = torch.zeros(6, 2, dtype=torch.float64, device=dev_)
    histogram = torch.zeros(13, dtype=torch.int64, device=dev_)
    per_batch = []
    with torch.no_grad():
        for batch in batches:
            batch = dict(batch)
            scores, out, err, terr = EV.score_rows(model, batch, params, ebs)
            forced = batch["gt_id"] if forced_mode else None
            answers, so, se, st, _ = EV.select_answers(scores, out, err, terr, batch["num_ans"], forced)
            nsp_right, reg_right, reg_t_right, needs = EV.correctness(answers, se, st, batch)
            EV.reduce_total_acc(total, needs, nsp_right, reg_right, reg_t_right, None)
            correct = nsp_right & (needs.logical_not() | reg_right)
            correct_t = nsp_right & (needs.logical_not() | reg_t_right)
            EV.reduce_breakdown_table(dataset.get_ans_type, None, params, breakdown, batch, correct, correct_t, needs)
            if with_histogram:
                EV.reduce_histogram(histogram, se[needs].view(-1), None)
            per_batch.append((answers, so, se, st))
    model.train()
    return total, breakdown, histogram, per_batch


@pytest.fixture(scope="module")
def tiny_plotqa():
    from test_step_gpu import build_model
    z, meta, batches = load_tiny()
    model, params = build_model(C.BertConfig.from_dict(meta["cfg"]), dict(meta["params"]), seed=meta["weight_seed"])
    params["ddp"] = False
    ans_type = {}
    for bi, b in enumerate(batches):
        for i, t in zip(b["id"].view(-1).tolist(), z["b%d.ans_type" % bi].tolist()):
            ans_type[i] = t
    return z, batches, model, params, _Dataset(ans_type), int(z["eval_batch_size"])


def _equal3(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y) for x, y in zip(a[:3], b[:3]))


def test_evaluate_equals_the_helper_path_on_plotqa(tiny_plotqa):
    z, batches, model, params, dataset, ebs = tiny_plotqa
    fresh = lambda: [dict(b) for b in batches]                                # noqa: E731
    for wh in (True, False):
        old = _helpers_evaluate(batches, dataset, params, ebs, model, with_histogram=wh)
        new = EV.evaluate(fresh(), dataset, params, ebs, model, with_histogram=wh)
        assert _equal3(new, old), (wh, new, old)
        assert _equal3(EV.plotqa_evaluate(fresh(), dataset, params, ebs, model, with_histogram=wh), old)
        assert (int(new[2].sum()) > 0) == wh and float(new[1].sum()) > 0
    assert model.training
    # '_REGS' question files: the answers are forced to gt_id (evaluation.py:288-289)
    p2 = dict(params, qa_file="qa_REGS_val")
    old = _helpers_evaluate(batches, dataset, p2, ebs, model, forced_mode=True)
    new = EV.evaluate(fresh(), dataset, p2, ebs, model, return_predictions=True)
    assert _equal3(new, old) and float(new[0][0, 0]) == float(new[0][0, 1])   # every forced answer is the right candidate
    assert not torch.equal(new[0], EV.evaluate(fresh(), dataset, params, ebs, model)[0])
    # the prediction records (evaluation.py:316-321)
    assert len(new[3]) == len(batches)
    for b, rec, (answers, so, se, st) in zip(batches, new[3], old[3]):
        needs = b["needs_reg"].view(-1).bool()
        rec = rec.cpu()
        assert tuple(rec.shape) == (b["id"].shape[0], 8) and rec.is_floating_point()
        cols = [b["id"].view(-1), b["gt_id"].view(-1), answers.cpu(), b["gt"].view(-1), so.cpu(), b["reg_target"].view(-1), se.cpu(), st.cpu()]
        for j, col in enumerate(cols):
            if j < 3:
                assert torch.equal(rec[:, j], col.to(rec.dtype)), j
            else:
                assert torch.equal(rec[needs, j], col[needs].to(rec.dtype)), j
                assert bool(torch.isnan(rec[~needs, j]).all()), j
        assert bool(needs.any()) and bool((~needs).any())
    # a category out of range is an error that names the ranges
    class Bad(_Dataset):
        def get_ans_type(self, qa_ind):
            return 3
    with pytest.raises(ValueError, match="answer kind 0..2"):
        EV.evaluate(fresh(), Bad(), params, ebs, model)
    assert model.training


def test_evaluate_under_a_single_process_gloo_group(tiny_plotqa, tmp_path):
    import torch.distributed as dist
    z, batches, model, params, dataset, ebs = tiny_plotqa
    alone = EV.evaluate([dict(b) for b in batches], dataset, params, ebs, model)
    assert not dist.is_initialized()
    dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "rendezvous"), rank=0, world_size=1)
    try:
        grouped = EV.evaluate([dict(b) for b in batches], dataset, dict(params, ddp=True), ebs, model, group=dist.group.WORLD)
        default = EV.evaluate([dict(b) for b in batches], dataset, dict(params, ddp=True), ebs, model)
    finally:
        dist.destroy_process_group()
    assert _equal3(grouped, alone) and _equal3(default, alone)
