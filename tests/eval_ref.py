"""numpy restatement of ONE evaluation batch's scoring as ``crct_eval_score`` computes it (test infrastructure only).

It follows CRCT/evaluation.py ``plotqa_evaluate_DDP`` through oracle/eval_oracle.py (softmax, flags :303-311, the tables
:465-484, :492-519, :528-543) and adds what the oracle does not state: the ``binary_answers`` branch (:280-285), the guards
of the selection kernel (a forced answer out of range, fewer rows than the questions claim, a question without candidates)
and the layout of the one int64 buffer the kernel adds into.
"""
import json
import os

import numpy as np
import torch

from oracle import eval_oracle as EO

TOTAL, BREAKDOWN, HISTOGRAM, ERRORS, TABLE_WORDS = 0, 12, 192, 205, 206        # CRCT_EVAL_* of include/crct_hip.h
_FIG_NAME = {v: k for k, v in EO.FIG_INDEX.items()}
_QID_OF_CAT = {0: "S0", 1: "D0", 2: "A0"}                                      # one question id per category (evaluation.py:437-449)


def binary_answers(p0, labels):
    """evaluation.py:280-285: answers = round(p0) (half to even, np.round as torch.round), right when equal to 1 - label.
    A NaN p0 answers -1 and is never right."""
    p0 = np.asarray(p0, dtype=np.float32)
    nan = np.isnan(p0)
    answers = np.where(nan, -1, np.round(np.where(nan, 0, p0))).astype(np.int64)
    return answers, ~nan & (answers == 1 - np.asarray(labels).reshape(-1))


def select_rows(p0, reg_out, reg_err, reg_terr, num_ans, forced=None):
    """evaluation.py:281-292 (oracle ``select_answers``) with the kernel's guards: rows at or beyond N score 0 and are never
    read; an answer outside its question's rows, or on a row beyond N, gives value 0 and infinite errors; a question without
    candidates answers 0."""
    N = len(p0)
    answers, out, err, terr = [], [], [], []
    off = 0
    for q, n in enumerate(np.asarray(num_ans).reshape(-1)):
        n = int(n)
        if forced is not None:
            a = int(np.asarray(forced).reshape(-1)[q])
        elif n > 0:
            rows = np.zeros(n, dtype=np.float32)
            m = max(0, min(n, N - off))
            rows[:m] = p0[off:off + m]
            a = int(np.argmax(rows))                      # first maximum; the first NaN when there is one
        else:
            a = 0
        ok = 0 <= a < n and off + a < N
        answers.append(a)
        out.append(reg_out[off + a] if ok else np.float32(0))
        err.append(reg_err[off + a] if ok else np.float32(np.inf))
        terr.append(reg_terr[off + a] if ok else np.float32(np.inf))
        off += n
    return (np.array(answers, dtype=np.int64), np.array(out, dtype=np.float32), np.array(err, dtype=np.float32),
            np.array(terr, dtype=np.float32))


def tally(tables, needs, nsp_right, reg_right, reg_t_right, sel_err, cats=None, with_histogram=False):
    """One batch's increments of the int64 [206] buffer: total, breakdown (with ``cats`` [Q, 3]), histogram, error count."""
    correct = nsp_right & (~needs | reg_right)
    correct_t = nsp_right & (~needs | reg_t_right)
    tables[TOTAL:TOTAL + 12] += EO.total_acc_increment(needs, nsp_right, reg_right, reg_t_right).astype(np.int64).reshape(-1)
    if with_histogram:
        with np.errstate(invalid="ignore"):
            tables[HISTOGRAM:HISTOGRAM + 13] += EO.histogram_increment(np.asarray(sel_err, dtype=np.float32)[needs])
    if cats is not None:
        cats = np.asarray(cats).reshape(-1, 3)
        good = (cats[:, 0] >= 1) & (cats[:, 0] <= 4) & (cats[:, 1] >= 0) & (cats[:, 1] <= 2) & (cats[:, 2] >= 0) & (cats[:, 2] <= 2)
        tables[ERRORS] += int((~good).sum())
        g = np.nonzero(good)[0]
        inc = EO.breakdown_increment([_QID_OF_CAT[int(cats[i, 2])] for i in g], [_FIG_NAME[int(cats[i, 0])] for i in g],
                                     [int(cats[i, 1]) for i in g], needs[g], correct[g], correct_t[g])
        tables[BREAKDOWN:BREAKDOWN + 180] += inc.astype(np.int64).reshape(-1)
    return tables


def score_batch(mode, logits, reg_out=None, reg_err=None, reg_terr=None, num_ans=None, forced=None, labels=None, gt_id=None,
                needs_reg=None, tolerance=None, cats=None, with_histogram=False, tables=None):
    """What one ``crct_eval_score`` call leaves: dict(prob0, answers, sel_out, sel_err, sel_terr, flags, tables)."""
    logits = np.asarray(logits, dtype=np.float32).reshape(-1, 2)
    p0 = EO.softmax_p0(logits) if len(logits) else np.zeros(0, dtype=np.float32)
    needs = np.asarray(needs_reg).reshape(-1).astype(bool)
    Q = needs.shape[0]
    if mode == 1:
        answers, nsp_right = binary_answers(p0, labels)
        out = err = terr = np.zeros(Q, dtype=np.float32)
    else:
        answers, out, err, terr = select_rows(p0, reg_out, reg_err, reg_terr, num_ans, forced)
        nsp_right = answers == np.asarray(gt_id).reshape(-1)
    with np.errstate(invalid="ignore"):
        reg_right = (err <= np.float32(0.05)) & needs
        reg_t_right = (terr <= np.asarray(tolerance, dtype=np.float32).reshape(-1)) & needs
    flags = (nsp_right * 1 + reg_right * 2 + reg_t_right * 4).astype(np.uint8)
    tables = np.zeros(TABLE_WORDS, dtype=np.int64) if tables is None else tables
    tally(tables, needs, nsp_right, reg_right, reg_t_right, err, cats, with_histogram)
    return dict(prob0=p0, answers=answers, sel_out=out, sel_err=err, sel_terr=terr, flags=flags, tables=tables)


def categories(qids, qa_types, ans_types):
    """int32 [Q, 3] (figure kind, answer kind, question category), as crct.evaluation.question_categories builds it."""
    return np.array([[EO.FIG_INDEX[t], int(a), EO.qcat_of_qid(q)] for q, t, a in zip(qids, qa_types, ans_types)], dtype=np.int32).reshape(-1, 3)


# ---------------------------------------------------------------- the committed evaluation fixtures
VARIANT_CASES = ("evalscore_figureqa", "evalscore_dvqa", "evalscore_dvqa_ce", "evalscore_dvqa_cls")


def load_fixture(name):
    """(z, meta, batches) of tests/golden/<name>.npz in the schema of tiny_evalscore.npz; the image features of the variant
    fixtures are drawn again from meta['feat_seed'] + batch index (the variant models never read them)."""
    from helpers import GOLDEN
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    batches = []
    for bi in range(int(z["n_batches"])):
        pre = "b%d.in." % bi
        b = {k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre)}
        if "image_feat" not in b:
            g = torch.Generator().manual_seed(int(meta["feat_seed"]) + bi)
            B, V = b["image_target"].shape
            b["image_feat"] = torch.randn(B, V, int(meta["cfg"]["v_feature_size"]), generator=g, dtype=torch.float32).half().float()
        if "b%d.qid" % bi in z.files:
            b["qid"] = [str(x) for x in z["b%d.qid" % bi]]
            b["qa_type"] = [str(x) for x in z["b%d.qa_type" % bi]]
        batches.append(b)
    return z, meta, batches


def fixture_tables(meta, batches, rows_of, ans_types=None, with_histogram=True):
    """The int64 [206] buffer of a whole evaluation from per-row scores: ``rows_of(bi, batch)`` -> (nsp_scores, reg0, reg2, reg4).
    Follows the loop: binary mode under params['binary_answers'], breakdown / histogram only for PlotQA."""
    params = meta["params"]
    binary = bool(params.get("binary_answers"))
    plotqa = "plotqa" in params["dataset"]
    tables = np.zeros(TABLE_WORDS, dtype=np.int64)
    per_batch = []
    for bi, b in enumerate(batches):
        nsp, r0, r2, r4 = rows_of(bi, b)
        cats = categories(b["qid"], b["qa_type"], ans_types[bi]) if plotqa else None
        per_batch.append(score_batch(1 if binary else 0, nsp, r0, r4, r2, num_ans=b["num_ans"].numpy(),
                                     labels=b["next_sentence_labels"].numpy(), gt_id=b["gt_id"].numpy(), needs_reg=b["needs_reg"].numpy(),
                                     tolerance=b["tolerance_margin"].numpy(), cats=cats, with_histogram=plotqa and with_histogram,
                                     tables=tables))
    return tables, per_batch
