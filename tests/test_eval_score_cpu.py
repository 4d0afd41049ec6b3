"""Evaluation scoring of every dataset, CPU part: the numpy restatement (tests/eval_ref.py) reproduces the accuracy tables the
REFERENCE's own evaluation loop returned for the DVQA / FigureQA fixtures (tests/golden/evalscore_*.npz, made by
tests/golden/make_golden_evalscore_variants.py), and the C boundary of ``crct_eval_score`` (symbol, struct mirror, host checks)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import eval_ref as ER
from crct import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", ER.VARIANT_CASES)
def test_eval_ref_reproduces_the_reference_totals(case):
    z, meta, batches = ER.load_fixture(case)
    assert len(batches) == 3 and all(8 <= b["num_ans"].shape[0] <= 12 for b in batches)
    assert meta["near_ties"] <= 2
    tables, per_batch = ER.fixture_tables(meta, batches, lambda bi, b: (z["b%d.nsp_scores" % bi], z["b%d.reg0" % bi], z["b%d.reg2" % bi], z["b%d.reg4" % bi]))
    total = tables[ER.TOTAL:ER.TOTAL + 12].reshape(6, 2)
    ref = z["total_correct"]
    assert np.array_equal(total.astype(np.float64), ref), (total, ref)
    assert not tables[ER.BREAKDOWN:].any()                    # breakdown, histogram: PlotQA only (evaluation.py:331); no error
    # every branch populated: some right, some wrong.  The regression rows exist only where the model has a regressor.
    rows = range(6) if case in ("evalscore_dvqa", "evalscore_dvqa_ce") else (0, 4)
    for r in rows:
        assert 0 < ref[r, 0] < ref[r, 1], (r, ref)
    if case in ("evalscore_dvqa", "evalscore_dvqa_ce"):
        flags = np.concatenate([p["flags"] for p in per_batch])
        needs = np.concatenate([b["needs_reg"].numpy().reshape(-1) for b in batches])
        seen = set(int(f) for f in flags[needs])
        assert {7, 5, 3, 6} <= seen, seen      # both measures right; tick only; 5 % only; a fine regression on the wrong candidate
        assert ref[4, 0] < ref[0, 0]
    else:
        assert (ref[1:4] == 0).all()
    if meta["params"]["binary_answers"]:
        answers = np.concatenate([p["answers"] for p in per_batch])
        assert set(answers.tolist()) == {0, 1}                # both answers occur


def test_binary_answers_round_half_to_even_and_nan():
    p0 = np.array([0.5, 0.50000006, 0.49999997, 1.0, 0.0, np.nan], dtype=np.float32)
    ans, right = ER.binary_answers(p0, np.array([1, 0, 0, 0, 1, 2]))
    assert ans.tolist() == [0, 1, 0, 1, 0, -1]
    assert right.tolist() == [True, True, False, True, True, False]     # a NaN is never right, not even against label 2


def _header_struct(name):
    text = open(os.path.join(ROOT, "include", "crct_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        m = re.match(r"(const\s+)?(\w+)\s*(\*?)\s*(.*)$", decl)
        kind, star, names = m.group(2), m.group(3), m.group(4)
        for n in names.split(","):
            n = n.strip()
            size = 8 if (star or n.startswith("*")) else {"int64_t": 8, "int32_t": 4, "float": 4}[kind]
            fields.append((n.lstrip("* "), size))
    return fields


def test_eval_score_symbol_struct_and_host_checks():
    assert "crct_eval_score" in L.PROTOTYPES
    raw = C.CDLL(L.LIB_PATH)
    assert hasattr(raw, "crct_eval_score") and hasattr(raw, "crct_eval_select")
    lib = L.load()
    assert lib.crct_abi_version() == 7
    fields = _header_struct("CrctEvalScoreArgs")
    assert [n for n, _ in fields] == [n for n, _ in L.EvalScoreArgs._fields_]
    size = sum(s for _, s in fields)
    assert C.sizeof(L.EvalScoreArgs) == (size + 7) // 8 * 8 == 18 * 8 + 8 + 3 * 4 + 4
    assert (L.EVAL_TOTAL, L.EVAL_BREAKDOWN, L.EVAL_HISTOGRAM, L.EVAL_ERRORS, L.EVAL_TABLE_WORDS) == (0, 12, 12 + 180, 12 + 180 + 13, 206)
    assert (ER.TOTAL, ER.BREAKDOWN, ER.HISTOGRAM, ER.ERRORS, ER.TABLE_WORDS) == (0, 12, 192, 205, 206)

    def args(**kw):
        a = L.EvalScoreArgs()
        for n, _ in L.EvalScoreArgs._fields_[:18]:
            setattr(a, n, 16)                  # never dereferenced: every call below fails on the host
        a.N, a.Q, a.mode, a.with_histogram = 8, 4, 0, 1
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    bad = [(args(mode=2), b"mode 2"), (args(mode=-1), b"mode -1"), (args(mode=1), b"one row per question"),
           (args(mode=1, N=4, labels=None), b"labels"), (args(num_ans=None), b"num_ans"), (args(Q=-1), b"sizes"), (args(N=-1), b"sizes"),
           (args(logits=None), b"null"), (args(gt_id=None), b"null"), (args(needs_reg=None), b"null"), (args(tolerance=None), b"null"),
           (args(answers=None), b"null"), (args(tables=None), b"null"), (args(reg_err=None), b"reg_err")]
    for a, needle in bad:
        assert lib.crct_eval_score(C.byref(a), None) == 2, needle
        msg = lib.crct_last_error()
        assert b"eval_score" in msg and needle in msg, (needle, msg)
    assert lib.crct_eval_score(None, None) == 2 and b"eval_score" in lib.crct_last_error()
    # no question: nothing to launch, whatever else is given
    assert lib.crct_eval_score(C.byref(args(Q=0, N=0)), None) == 0
    assert lib.crct_eval_score(C.byref(args(Q=0, N=0, mode=1)), None) == 0
