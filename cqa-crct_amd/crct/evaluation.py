"""Evaluation scoring path on the MI355X step engine.

Mirror of the scoring half of CRCT/evaluation.py ``plotqa_evaluate_DDP`` (:199-386) and its helpers
(``reduce_total_acc`` :492-525, ``reduce_histogram`` :528-549, ``reduce_breakdown_table`` :465-489,
``get_qcat_by_qid`` :437-449): the evaluation batch holds, per question, ``num_ans`` candidate answers as consecutive
rows; the rows are scored by chunked evaluation forwards (dropout off, ``'L1'`` regression kind), every question picks
the candidate with the highest answer probability, and regression questions count as right when the chosen candidate's
value is within 5 % (or within the chart's tick tolerance).

What is different from the reference is only HOW: the reference walks the questions in a Python loop with one
``.item()`` host sync each (:281-292) and moves every intermediate to the CPU; here the selection is one HIP launch
(``crct_eval_select``, one wave per question) and all flags / tables stay on the device until the caller reads them.
``evaluate`` is the loop for every dataset (PlotQA, DVQA, and FigureQA's ``binary_answers`` branch :280-285): there the
selection, the flags and the three tables of a batch are one launch together (``crct_eval_score``).
Logging, CSV dumps and plots of the reference are not rebuilt.
"""
import ctypes

import numpy as np
import torch
import torch.distributed as dist

from . import lib as L
from .step_adapter import forward as step_forward

# fig_dataloader.py:27-32: per-candidate tensors, padded to [Q, 120, ...] by the collate step
PADDING_TXT = ["tokens", "segments", "sep_indices", "mask", "next_sentence_labels", "hist_len", "loc", "legend_belonging_t"]
PADDING_VIS = ["image_feat", "image_loc", "image_mask", "image_target", "image_label", "legend_belonging_v", "R"]
FIG_INDEX = {"Total": 0, "line": 1, "vbar": 2, "hbar": 3, "dot": 4}                # evaluation.py:467


def cut_batch_padding(batch, keys=None):
    """fig_dataloader.py:697-702: keep the first ``num_ans[i]`` candidate rows of question i and concatenate."""
    n = batch["num_ans"].reshape(-1).tolist()
    for k in (keys if keys is not None else PADDING_VIS + PADDING_TXT):
        if k in batch:
            x = batch[k]
            batch[k] = torch.cat([x[i, :n[i], ...] for i in range(x.shape[0])], dim=0)
    return batch


def get_qcat_by_qid(qid):
    """evaluation.py:437-449: ('s', 0) structural S0..S17, ('d', 1) data retrieval D0..D15 except D6, ('r', 2) reasoning."""
    num = qid[1:]
    if qid[:1] == "S" and num.isdigit() and 0 <= int(num) <= 17:
        return "s", 0
    if qid[:1] == "D" and num.isdigit() and 0 <= int(num) <= 15 and int(num) != 6:
        return "d", 1
    return "r", 2


def score_rows(dialog_encoder, batch, params, eval_batch_size):
    """evaluation.py:233-266: chunked evaluation forwards over all candidate rows.
    Returns device tensors (nsp_scores [N, 2], reg_output [N], reg_err [N], reg_t_err [N])."""
    N = batch["tokens"].shape[0]
    scores, out, err, terr = [], [], [], []
    for j in range(int(np.ceil(N / eval_batch_size))):
        lo, hi = j * eval_batch_size, min((j + 1) * eval_batch_size, N)
        _, _, _, _, nsp_scores, regression = step_forward(dialog_encoder, batch, params, output_nsp_scores=True,
                                                          evaluation=True, sample_ids=np.arange(lo, hi))
        assert nsp_scores.shape[-1] == 2                                           # :252
        scores.append(nsp_scores)
        out.append(regression[0]); err.append(regression[4]); terr.append(regression[2])
    return torch.cat(scores, 0), torch.cat(out, 0), torch.cat(err, 0), torch.cat(terr, 0)


def select_answers(nsp_scores, reg_out, reg_err, reg_terr, num_ans, forced=None):
    """evaluation.py:281-302 as ONE launch.  Returns (answers [Q] int64, out [Q], err [Q], t_err [Q], prob0 [N])."""
    dev = nsp_scores.device
    if dev.type != "cuda":
        raise RuntimeError("select_answers runs on an MI355X only (no CPU fallback)")
    na = num_ans.reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
    Q, N = na.numel(), nsp_scores.shape[0]
    f = lambda t: t.reshape(-1).to(device=dev, dtype=torch.float32).contiguous()   # noqa: E731
    logits = nsp_scores.to(torch.float32).contiguous()
    ro, re_, rt = f(reg_out), f(reg_err), f(reg_terr)
    fz = forced.reshape(-1).to(device=dev, dtype=torch.int64).contiguous() if forced is not None else None
    answers = torch.empty(Q, dtype=torch.int64, device=dev)
    so, se, st = (torch.empty(Q, device=dev) for _ in range(3))
    p0 = torch.empty(N, device=dev)
    L.check(L.load().crct_eval_select(L.ptr(logits), L.ptr(ro), L.ptr(re_), L.ptr(rt), L.ptr(na), L.ptr(fz), Q, N, L.ptr(p0),
                                      L.ptr(answers), L.ptr(so), L.ptr(se), L.ptr(st), L.current_stream()), "eval_select")
    return answers, so, se, st, p0


def correctness(answers, sel_err, sel_terr, batch):
    """evaluation.py:303-311 on the device."""
    dev = answers.device
    gt_id = batch["gt_id"].reshape(-1).to(dev)
    needs = batch["needs_reg"].reshape(-1).to(dev).bool()
    tol = batch["tolerance_margin"].reshape(-1).to(dev).float()
    nsp_right = answers == gt_id
    reg_right = (sel_err <= 0.05) & needs
    reg_t_right = (sel_terr <= tol) & needs
    return nsp_right, reg_right, reg_t_right, needs


def reduce_total_acc(total_correct_tensor, needs_regression, nsp_right, reg_right, reg_t_right, group=None):
    """evaluation.py:492-525: the [6, 2] (hits, count) table; all-reduced when a process group is up."""
    t = torch.zeros_like(total_correct_tensor)
    n = nsp_right.shape[0]
    not_needed = needs_regression.logical_not()
    t[0, 0], t[0, 1] = nsp_right.sum(), n
    t[1, 0], t[1, 1] = (nsp_right & needs_regression).sum(), needs_regression.sum()
    t[2, 0], t[2, 1] = reg_right.sum(), needs_regression.sum()
    t[3, 0], t[3, 1] = reg_t_right.sum(), needs_regression.sum()
    t[4, 0], t[4, 1] = (nsp_right & (not_needed | reg_right)).sum(), n
    t[5, 0], t[5, 1] = (nsp_right & (not_needed | reg_t_right)).sum(), n
    if dist.is_available() and dist.is_initialized():
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    total_correct_tensor += t
    return total_correct_tensor


def reduce_histogram(histogram, reg_5_dist, group=None):
    """evaluation.py:528-549: 13 bins of the relative regression error."""
    d = reg_5_dist
    h = torch.zeros_like(histogram)
    k = 0
    for i in range(4):
        h[k] = (((i / 20) < d) & (d <= ((i + 1) / 20))).sum()
        k += 1
    for i in range(2, 10):
        h[k] = (((i / 10) < d) & (d <= ((i + 1) / 10))).sum()
        k += 1
    h[k] = (1 < d).sum()
    if dist.is_available() and dist.is_initialized():
        dist.all_reduce(h, op=dist.ReduceOp.SUM, group=group)
    histogram += h
    return histogram


def reduce_breakdown_table(get_ans_type, group, params, breakdown_tensor, batch, correct, correct_t, needs):
    """evaluation.py:465-489.  The string / dataset look-ups of the questions run on the host (they are host data);
    the table itself is built by one scatter-add on the device."""
    dev = breakdown_tensor.device
    ids = batch["id"].reshape(-1).tolist()
    qc = [get_qcat_by_qid(q)[1] for q in batch["qid"]]
    fig = [FIG_INDEX[t] for t in batch["qa_type"]]
    ans = [int(get_ans_type(i)) for i in ids]
    qc_t, fig_t, ans_t = (torch.tensor(v, dtype=torch.int64, device=dev) for v in (qc, fig, ans))
    t = torch.zeros_like(breakdown_tensor)
    one = torch.ones(len(ids), dtype=t.dtype, device=dev)
    c5, ct = correct.to(t.dtype), correct_t.to(t.dtype)
    nd = needs.to(t.dtype)
    last = torch.full_like(ans_t, breakdown_tensor.shape[1] - 1)
    for f in (torch.zeros_like(fig_t), fig_t):
        for col, val in ((0, c5), (1, ct), (2, one)):
            c = torch.full_like(fig_t, col)
            t.index_put_((f, ans_t, qc_t, c), val, accumulate=True)
            t.index_put_((f, last, qc_t, c), val * nd, accumulate=True)
    if params.get("ddp") and dist.is_available() and dist.is_initialized():
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)                      # :485-488
    breakdown_tensor += t       # the reference accumulates only under DDP (its evaluation never runs without it)
    return breakdown_tensor


def question_categories(batch, get_ans_type):
    """The breakdown indices of a batch's questions (evaluation.py:471-474) as one host int32 [Q, 3] tensor: figure kind 1..4
    (FIG_INDEX), answer kind (``get_ans_type``), question category (``get_qcat_by_qid``).  Unknown figure kinds become -1 and
    are counted by the kernel as errors."""
    ids = batch["id"].reshape(-1).tolist()
    rows = [[FIG_INDEX.get(t, -1), int(get_ans_type(i)), get_qcat_by_qid(q)[1]] for i, q, t in zip(ids, batch["qid"], batch["qa_type"])]
    return torch.tensor(rows, dtype=torch.int32).reshape(len(ids), 3)


def score_batch(nsp_scores, reg_out, reg_err, reg_terr, batch, tables, binary=False, forced=None, cats=None, with_histogram=False,
                want_prob0=False):
    """Selection, flags and tables of one batch as ONE launch (``crct_eval_score``; evaluation.py:280-311, :465-543).
    ``tables`` (int64 [lib.EVAL_TABLE_WORDS], on the device) is added into in place.  ``cats``: int32 [Q, 3] from
    ``question_categories`` (host or device; one copy) or None for no breakdown.  The regression rows may be None with
    ``binary``.  Returns (answers [Q] int64, sel_out, sel_err, sel_terr [Q] fp32, flags [Q] uint8, prob0 [N] or None)."""
    dev = nsp_scores.device
    if dev.type != "cuda":
        raise RuntimeError("score_batch runs on an MI355X only (no CPU fallback)")
    if tables.device != dev or tables.dtype != torch.int64 or tables.numel() != L.EVAL_TABLE_WORDS or not tables.is_contiguous():
        raise ValueError("score_batch: tables must be a contiguous int64 [%d] tensor on %s" % (L.EVAL_TABLE_WORDS, dev))
    i64 = lambda t: None if t is None else t.reshape(-1).to(device=dev, dtype=torch.int64).contiguous()      # noqa: E731
    f32 = lambda t: None if t is None else t.reshape(-1).to(device=dev, dtype=torch.float32).contiguous()    # noqa: E731
    logits = nsp_scores.to(torch.float32).contiguous()
    N = logits.shape[0]
    gt_id = i64(batch["gt_id"])
    Q = gt_id.numel()
    keep = [logits, gt_id, f32(reg_out), f32(reg_err), f32(reg_terr),
            i64(batch["next_sentence_labels"]) if binary else None, None if binary else i64(batch["num_ans"]), i64(forced),
            batch["needs_reg"].reshape(-1).to(device=dev, dtype=torch.uint8).contiguous(), f32(batch["tolerance_margin"]),
            None if cats is None else cats.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()]
    answers = torch.empty(Q, dtype=torch.int64, device=dev)
    so, se, st = (torch.empty(Q, device=dev) for _ in range(3))
    flags = torch.empty(Q, dtype=torch.uint8, device=dev)
    p0 = torch.empty(N, device=dev) if want_prob0 else None
    a = L.EvalScoreArgs()
    (a.logits, a.gt_id, a.reg_out, a.reg_err, a.reg_terr, a.labels, a.num_ans, a.forced, a.needs_reg, a.tolerance,
     a.cats) = (L.ptr(t) for t in keep)
    a.answers, a.sel_out, a.sel_err, a.sel_terr, a.flags, a.prob0, a.tables = (L.ptr(t) for t in (answers, so, se, st, flags, p0, tables))
    a.N, a.Q, a.mode, a.with_histogram = N, Q, 1 if binary else 0, 1 if with_histogram else 0
    L.check(L.load().crct_eval_score(ctypes.byref(a), L.current_stream()), "eval_score")
    return answers, so, se, st, flags, p0


def prediction_record(batch, answers, sel_out, sel_err, sel_terr):
    """evaluation.py:316-321: [Q, 8] float64 rows (id, gt_id, answer, gt, regressed value, target, relative error, tick error) on the
    device, NaN from column 3 on where the question needs no regression."""
    dev = answers.device
    col = lambda k: batch[k].reshape(-1).to(dev).to(torch.float64)               # noqa: E731
    rec = torch.stack([col("id"), col("gt_id"), answers.double(), col("gt"), sel_out.double(), col("reg_target"), sel_err.double(), sel_terr.double()], 1)
    rec[batch["needs_reg"].reshape(-1).to(dev).bool().logical_not(), 3:] = float("nan")
    return rec


def evaluate(dataloader, dataset, params, eval_batch_size, dialog_encoder, group=None, with_histogram=True, return_predictions=False):
    """The evaluation loop of every dataset the model knows (evaluation.py:199-386 without logging / CSV / plots): candidate
    rows for PlotQA and DVQA, ``params['binary_answers']`` (:280-285) for FigureQA, forced answers for '_REGS' question files;
    the breakdown and the histogram only for PlotQA (:331).  Everything after the forwards is one launch per batch
    (``score_batch``) into one int64 buffer, which is all-reduced ONCE after the loop when a process group is up (integer sums:
    the same totals as the reference's per-batch reductions).
    ``dataset`` needs ``get_ans_type(qa_id)`` for PlotQA and may provide ``cut_batch_padding``.
    Returns (total_correct_tensor [6, 2] float64, breakdown_tensor [5, 4, 3, 3] float64, histogram [13] int64) on the device,
    and with ``return_predictions`` a list of ``prediction_record`` tensors, one per batch, as a fourth value."""
    was_training = dialog_encoder.training
    dialog_encoder.eval()
    dev = torch.device(params["device"])
    tables = torch.zeros(L.EVAL_TABLE_WORDS, dtype=torch.int64, device=dev)
    binary = bool(params.get("binary_answers"))
    plotqa = "plotqa" in params["dataset"]
    forced_mode = "_REGS" in str(params.get("qa_file", ""))
    records = []
    try:
        with torch.no_grad():
            for batch in dataloader:
                (dataset.cut_batch_padding if hasattr(dataset, "cut_batch_padding") else cut_batch_padding)(batch)
                if batch["id"].shape[0] == 0:
                    continue
                scores, out, err, terr = score_rows(dialog_encoder, batch, params, eval_batch_size)
                assert batch["tokens"].shape[0] == scores.shape[0] == out.shape[0] == err.shape[0] == terr.shape[0]   # :269
                cats = question_categories(batch, dataset.get_ans_type) if plotqa else None
                forced = batch["gt_id"] if forced_mode and not binary else None
                answers, so, se, st, _, _ = score_batch(scores, out, err, terr, batch, tables, binary=binary, forced=forced, cats=cats,
                                                        with_histogram=plotqa and with_histogram)
                if return_predictions:
                    records.append(prediction_record(batch, answers, so, se, st))
    finally:
        if was_training:
            dialog_encoder.train()
    if dist.is_available() and dist.is_initialized():
        if dist.get_backend(group) == "gloo":              # 1.6 KB, once per evaluation: through the host where the backend has no device path
            host = tables.cpu()
            dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
            tables.copy_(host)
        else:
            dist.all_reduce(tables, op=dist.ReduceOp.SUM, group=group)
    if int(tables[L.EVAL_ERRORS]) != 0:
        raise ValueError("evaluate: %d questions with a category outside figure kind 1..4 (%s) / answer kind 0..2 / question category "
                         "0..2" % (int(tables[L.EVAL_ERRORS]), ", ".join(k for k in FIG_INDEX if k != "Total")))
    total = tables[L.EVAL_TOTAL:L.EVAL_TOTAL + 12].to(torch.float64).reshape(6, 2)
    breakdown = tables[L.EVAL_BREAKDOWN:L.EVAL_BREAKDOWN + 180].to(torch.float64).reshape(5, 4, 3, 3)
    histogram = tables[L.EVAL_HISTOGRAM:L.EVAL_HISTOGRAM + 13].clone()
    if return_predictions:
        return total, breakdown, histogram, records
    return total, breakdown, histogram


def plotqa_evaluate(dataloader, dataset, params, eval_batch_size, dialog_encoder, group=None, with_histogram=True):
    """The PlotQA evaluation loop under its earlier name: ``evaluate``.
    Returns (total_correct_tensor [6, 2], breakdown_tensor [5, 4, 3, 3], histogram [13]) on the device."""
    return evaluate(dataloader, dataset, params, eval_batch_size, dialog_encoder, group=group, with_histogram=with_histogram)


def masked_lm_evaluate(dataloader, params, encoder, topk=(1, 5), eval_batch_size=None, group=None):
    """Masked-token accuracy, loss and perplexity of the LM head over the tokens that carry a label (``batch['mask']``, -1 = none): per batch,
    in chunks of ``eval_batch_size`` rows like ``evaluate`` (None: the whole batch), an evaluation forward and then
    ``lm_predict(labels=mask, k=max(topk))`` on the labelled rows.  The token count, the count of ``label_rank < k`` for every k (int64) and the
    sum of ``-label_logprob`` (fp64) are accumulated on the device with stock torch reductions over the [R] vectors -- no host sync inside
    the loop with the labels on the host, where the loader leaves them -- then all-reduced once when a process group is up and read with one
    transfer.  Returns ``dict(n, loss, perplexity, acc={k: ...})``; without any labelled token n = 0 and the rest is NaN.  max(topk) must be
    1, 5 or 8; every k <= max(topk)."""
    import math
    topk = tuple(int(k) for k in topk)
    kmax = max(topk)
    core = getattr(encoder, "module", encoder).bert_pretrained
    dev = torch.device(params["device"])
    counts = torch.zeros(1 + len(topk), dtype=torch.int64, device=dev)        # n, hits per k
    nll = torch.zeros(1, dtype=torch.float64, device=dev)
    was_training = encoder.training
    encoder.eval()
    try:
        with torch.no_grad():
            for batch in dataloader:
                N = batch["tokens"].shape[0]
                step = N if eval_batch_size is None else int(eval_batch_size)
                for lo in range(0, N, max(step, 1)):
                    hi = min(lo + step, N)
                    step_forward(encoder, batch, params, evaluation=True, sample_ids=None if (lo, hi) == (0, N) else np.arange(lo, hi))
                    pred = core.lm_predict(labels=batch["mask"][lo:hi], k=kmax)
                    if pred.rows.numel() == 0:
                        continue
                    counts[0] += int(pred.rows.numel())
                    for i, k in enumerate(topk):
                        counts[1 + i] += (pred.label_rank < k).sum()
                    nll += (-pred.label_logprob.double()).sum()
    finally:
        if was_training:
            encoder.train()
    packed = torch.cat([counts.double(), nll])                                    # counts below 2^53: exact in fp64
    if dist.is_available() and dist.is_initialized():
        if dist.get_backend(group) == "gloo":
            host = packed.cpu()
            dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
            packed = host
        else:
            dist.all_reduce(packed, op=dist.ReduceOp.SUM, group=group)
    host = packed.cpu().tolist()
    n = int(host[0])
    loss = host[-1] / n if n else float("nan")
    try:
        ppl = math.exp(loss)
    except OverflowError:
        ppl = float("inf")
    return dict(n=n, loss=loss, perplexity=ppl, acc={k: (host[1 + i] / n if n else float("nan")) for i, k in enumerate(topk)})
