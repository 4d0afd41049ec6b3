"""Masked-LM predictions (-m gpu): ``return_lm_scores`` / ``output_lm_scores`` (prediction_scores_t in slot 4 of the training tuple and slot 0 of
the inference tuple, differentiable under grad), ``CrctModel.lm_predict`` and ``evaluation.masked_lm_evaluate``.  The tiny config of
tests/test_lm_loss_gpu.py: vocab_size = 130, B 4, T 12, 5 visual elements, dropout off; one case at the BERT vocabulary (30522 -> 30528).

Off (passes without the feature too): both slots None, nothing on the model, the launches of a training step unchanged.  On: the scores
against tests/lm_scores_ref.py computed from the step's OWN sequence_output_t and weights, within its budget, and bit-identical between the
ways to ask for them; their gradients (head tensors, the word table's decoder term, d / d sequence_output_t) within the same reference's
budget; predictions exactly the reference order on the scores the same forward returned.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lm_head_ref as R                            # noqa: E402
import lm_scores_ref as SR                         # noqa: E402
from crct import config as C                       # noqa: E402
from crct import synthetic as S                    # noqa: E402
from crct.model import SequenceMask                # noqa: E402
from crct.step_adapter import forward as step_forward   # noqa: E402
from helpers import ATOMIC_GRADS                   # noqa: E402
from test_lm_loss_gpu import B, COEFF, HEAD, REF_KEY, T, VOCAB, WORD, grads, head_weights, make   # noqa: E402
from test_lm_topk_kernels_gpu import _launches     # noqa: E402
from test_seq_outputs_gpu import _logged           # noqa: E402
from test_step_gpu import build_model              # noqa: E402

DEV = torch.device("cuda:0")
H = 64


def core_call(core, batch, train=True):
    """The model called as the step adapter calls it (crct/step_adapter.py), returning the model's OWN tuple: 8 values in the training
    branch (slot 4 = prediction_scores_t), 7 in the inference branch (slot 0)."""
    kw = dict(sep_indices=batch["sep_indices"], sep_len=batch["hist_len"] + 1, token_type_ids=batch["segments"], masked_lm_labels=batch["mask"],
              attention_mask=SequenceMask(batch["sep_indices"], batch["hist_len"], batch["tokens"].shape[1]),
              next_sentence_label=batch["next_sentence_labels"] if train else None, image_attention_mask=batch["image_mask"],
              image_label=batch["image_label"] if train else None, image_target=batch["image_target"],
              gt_reg=[batch["R"], "L1_smooth" if train else "L1"])
    return core(batch["tokens"], batch["loc"], batch["image_feat"], batch["image_loc"], **kw)


def upstream(shape=(B, T, VOCAB), seed=21):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def seq_rows(core):
    return core.sequence_output_t.detach().double().cpu().reshape(-1, core.config.hidden_size)


def bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


# ------------------------------------------------------------------------------------------------ off
@pytest.mark.parametrize("coeff", [None, COEFF])
def test_off_both_slots_are_none_and_the_step_launches_what_it_launched(coeff):
    cfg, model, params, core, batch = make(coeff)
    core.return_lm_scores = False
    out = core_call(core, batch)
    assert len(out) == 8 and out[4] is None and getattr(core, "prediction_scores_t", None) is None
    model.eval()
    with torch.no_grad():
        ev = core_call(core, batch, train=False)
    assert len(ev) == 7 and ev[0] is None and getattr(core, "prediction_scores_t", None) is None
    model.train()
    _, model2, params2, core2, _ = make(coeff)                                          # never touches the attribute

    def step(m, p, c):
        def run():
            c.zero_flat_grads()
            c._calls = 0
            step_forward(m, batch, p)[0].backward()
        return _logged(run)[1:]
    step(model, params, core), step(model2, params2, core2)                             # (first calls build caches)
    assert step(model, params, core) == step(model2, params2, core2)
    a, b = grads(core), grads(core2)
    for n in a:
        if n not in ATOMIC_GRADS:
            assert (a[n] is None and b[n] is None) or torch.equal(bits(a[n]), bits(b[n])), n


# ------------------------------------------------------------------------------------------------ on: values
@pytest.mark.parametrize("coeff", [0.0, COEFF])
def test_on_scores_in_every_branch_against_the_reference_from_the_steps_own_states(coeff):
    cfg, model, params, core, batch = make(coeff)
    core.return_lm_scores = True
    core.return_sequence_outputs = True
    out = core_call(core, batch)
    scores = out[4]
    assert scores is not None and scores is core.prediction_scores_t
    assert tuple(scores.shape) == (B, T, VOCAB) and scores.dtype == torch.float32 and scores.requires_grad
    assert not scores.is_contiguous() and scores.stride() == (T * 192, 192, 1)          # a view of the padded [64, 192] logits
    w, x = head_weights(core), seq_rows(core)
    ref, bud = SR.reference(w, x)["scores"], SR.budget(w, x)["scores"]
    err = (scores.detach().double().cpu().reshape(-1, VOCAB) - ref).abs()
    print("coeff %s: scores worst |error| / budget %.3f" % (coeff, float((err / bud).max())))
    assert bool((err <= bud).all())
    assert float(ref.abs().max()) > 8.0 * float(bud.max())
    kept = scores.detach().clone()
    # slot 3 is return_sequence_outputs' alone: without it the scores are the same and slot 3 stays None
    core.return_sequence_outputs = False
    out = core_call(core, batch)
    assert out[3] is None and core.sequence_output_t is None and torch.equal(bits(out[4].detach()), bits(kept))
    with torch.no_grad():                                                               # the training branch, forward only
        out = core_call(core, batch)
    assert not out[4].requires_grad and torch.equal(bits(out[4]), bits(kept))
    assert (float(out[0]) > 0.0) == (coeff > 0.0)
    ev = core_call(core, batch, train=False)                                            # the inference tuple (dropout is off: the same text states)
    assert len(ev) == 7 and ev[0] is core.prediction_scores_t and not ev[0].requires_grad and torch.equal(bits(ev[0]), bits(kept))
    model.eval()
    with torch.no_grad():
        ev = core_call(core, batch, train=False)
    assert torch.equal(bits(ev[0]), bits(kept))
    model.train()
    # VisualDialogEncoder(output_lm_scores=True): the flag for that call only, the appended element is the tensor
    core.return_lm_scores = False
    kw = dict(sep_indices=batch["sep_indices"], sep_len=batch["hist_len"] + 1, token_type_ids=batch["segments"], masked_lm_labels=batch["mask"],
              attention_mask=SequenceMask(batch["sep_indices"], batch["hist_len"], T), next_sentence_label=batch["next_sentence_labels"],
              image_attention_mask=batch["image_mask"], image_label=batch["image_label"], image_target=batch["image_target"],
              gt_reg=[batch["R"], "L1_smooth"])
    enc = model(batch["tokens"], batch["loc"], batch["image_feat"], batch["image_loc"], output_lm_scores=True, **kw)
    assert len(enc) == 7 and torch.equal(bits(enc[4].detach()), bits(kept)) and enc[4].requires_grad and core.return_lm_scores is False
    assert len(model(batch["tokens"], batch["loc"], batch["image_feat"], batch["image_loc"], **kw)) == 6 and core.prediction_scores_t is None
    # the step adapter: its tuples keep their lengths, the tensor is left on the core
    tr = step_forward(model, batch, params, output_lm_scores=True)
    assert len(tr) == 7 and torch.equal(bits(core.prediction_scores_t.detach()), bits(kept))
    model.eval()
    ev = step_forward(model, batch, params, output_lm_scores=True, evaluation=True)
    assert len(ev) == 6 and ev[0] is None and torch.equal(bits(core.prediction_scores_t), bits(kept))
    model.train()
    step_forward(model, batch, params)
    assert core.prediction_scores_t is None


def test_on_the_loss_and_every_gradient_keep_their_bits():
    got = []
    for on in (False, True):
        cfg, model, params, core, batch = make()
        core.return_lm_scores = on
        core.zero_flat_grads()
        out = step_forward(model, batch, params)
        out[0].backward()
        torch.cuda.synchronize()
        got.append((out[1].detach().clone(), out[0].detach().clone(), grads(core)))
        assert (core.prediction_scores_t is not None) == on
    assert torch.equal(bits(got[0][0]), bits(got[1][0])) and torch.equal(bits(got[0][1]), bits(got[1][1]))
    for n, g in got[0][2].items():
        if n not in ATOMIC_GRADS:
            assert torch.equal(bits(g), bits(got[1][2][n])), n


# ------------------------------------------------------------------------------------------------ on: gradients
def scores_pass(coeff, scale=None, with_loss=False, only_loss=False, **cfg_over):
    """One forward with the scores on and one backward of (scores * G).sum() (optionally scaled / with the adapter's loss / the loss alone).
    Returns (core, batch, G, gradients of every used tensor, d / d sequence_output_t as autograd accumulated it on that output)."""
    cfg, model, params, core, batch = make(coeff, **cfg_over)
    core.return_lm_scores = True
    core.return_sequence_outputs = True
    out = step_forward(model, batch, params)
    scores, seq = core.prediction_scores_t, core.sequence_output_t
    seq.retain_grad()
    G = upstream()
    core.zero_flat_grads()
    target = out[0] if only_loss else (scores * G).sum() + (out[0] if with_loss else 0.0)
    (target if scale is None else scale.scale(target)).backward()
    torch.cuda.synchronize()
    return core, batch, G, grads(core), seq.grad.detach().clone()


def test_gradients_of_the_scores_against_the_reference():
    core, batch, G, got, d_seq = scores_pass(COEFF)
    w, x = head_weights(core), seq_rows(core)
    G64 = G.double().cpu().reshape(-1, VOCAB)
    ref, bud = SR.reference(w, x, G64), SR.budget(w, x, G64)
    mine = {REF_KEY[n]: got[n].double().cpu() for n in HEAD}
    mine["d_seq"] = d_seq.double().cpu().reshape(-1, H)
    worst = {k: float(((v - ref[k]).abs() / bud[k]).max()) for k, v in mine.items()}
    print("worst |error| / budget:", {k: round(v, 3) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst
    assert all(float(ref[k].abs().max()) > 4.0 * float(bud[k].max()) for k in mine)
    # the word table = the decoder term + what the encoder hands down from d_seq: the latter from a model without the head, given the same
    # upstream on sequence_output_t (tests/test_lm_loss_gpu.py does the same for the loss)
    _, model0, params0, core0, _ = make(None)
    core0.return_sequence_outputs = True
    step_forward(model0, batch, params0)
    assert torch.equal(core0.sequence_output_t, core.sequence_output_t.detach())
    core0.zero_flat_grads()
    (d_seq * core0.sequence_output_t).sum().backward()
    torch.cuda.synchronize()
    word_on, word_off = got[WORD].double().cpu(), grads(core0, [WORD])[WORD].double().cpu()
    err = (word_on - word_off - ref["decoder"]).abs()
    bound = bud["decoder"] + 2.0 ** -21 * (word_off.abs() + ref["decoder"].abs())
    print("word table: worst |error| / bound %.3f" % float((err / bound).max()))
    assert bool((err <= bound).all())
    assert float(ref["decoder"].abs().max()) > 4.0 * float(bound.max())


def test_with_the_loss_off_only_d_seq_and_the_word_table_flow():
    core, batch, G, got, d_seq = scores_pass(0.0)
    byname = dict(core.named_parameters())
    assert all(byname[n].grad is None for n in HEAD) and all(not core._entries[n].used for n in HEAD)
    w, x = head_weights(core), seq_rows(core)
    G64 = G.double().cpu().reshape(-1, VOCAB)
    ref, bud = SR.reference(w, x, G64), SR.budget(w, x, G64)
    err = (d_seq.double().cpu().reshape(-1, H) - ref["d_seq"]).abs()
    print("d_seq worst |error| / budget %.3f" % float((err / bud["d_seq"]).max()))
    assert bool((err <= bud["d_seq"]).all())
    # ... and the same bits as with the loss on: the head tensors' gradients are no part of d_seq
    assert torch.equal(bits(d_seq), bits(scores_pass(COEFF)[4]))
    assert float(got[WORD].abs().max()) > 0.0


def test_scores_and_fused_loss_in_one_pass_add_up():
    """(loss + (scores * G).sum()).backward() against the two separate passes added.  On the head tensors and on sequence_output_t the two
    nodes' terms are the same launches in both forms, added in fp32: the closed forms' budgets (both references') hold with room."""
    core, batch, G, both, d_both = scores_pass(COEFF, with_loss=True)
    _, _, _, g_scores, d_scores = scores_pass(COEFF)
    _, _, _, g_loss, d_loss = scores_pass(COEFF, only_loss=True)
    w, x = head_weights(core), seq_rows(core)
    G64, labels = G.double().cpu().reshape(-1, VOCAB), batch["mask"].reshape(-1)
    bs, bl = SR.budget(w, x, G64), R.budget(w, x, labels, g=COEFF)
    for n in HEAD:
        err = (both[n] - (g_scores[n] + g_loss[n])).double().cpu().abs()
        assert bool((err <= bs[REF_KEY[n]] + bl[REF_KEY[n]]).all()), n
        assert float(g_loss[n].abs().max()) > 0.0 and float(g_scores[n].abs().max()) > 0.0
    err = (d_both - (d_scores + d_loss)).double().cpu().reshape(-1, H).abs()
    assert bool((err <= bs["d_seq"] + bl["d_seq"]).all())
    assert torch.isfinite(both[WORD]).all() and not torch.equal(both[WORD], g_scores[WORD])


def test_a_grad_scaler_scales_the_gradients_exactly_and_a_frozen_word_table_gets_nothing():
    _, _, _, one, d_one = scores_pass(COEFF)
    _, _, _, scaled, d_scaled = scores_pass(COEFF, scale=torch.amp.GradScaler("cuda", init_scale=1024.0))
    for n in HEAD:                                                                      # powers of two all the way
        assert torch.equal(scaled[n], 1024.0 * one[n]), n
    assert torch.equal(d_scaled, 1024.0 * d_one)
    core, _, _, got, _ = scores_pass(COEFF, fixed_t_layer=1)
    byname = dict(core.named_parameters())
    assert byname[WORD].grad is None and WORD in core.tensors_without_grad
    assert all(float(got[n].abs().max()) > 0.0 for n in HEAD)


# ------------------------------------------------------------------------------------------------ lm_predict
def test_lm_predict_is_the_reference_order_on_the_scores_of_the_same_forward():
    cfg, model, params, core, batch = make()
    with pytest.raises(RuntimeError, match="forward pass"):
        core.lm_predict(labels=batch["mask"])
    core.return_lm_scores = True
    core.return_sequence_outputs = True
    step_forward(model, batch, params)
    scores = core.prediction_scores_t.detach().cpu().reshape(-1, VOCAB)
    labels = batch["mask"].reshape(-1)
    rows = (labels >= 0).nonzero().flatten()
    xs = scores[rows].contiguous().numpy()
    preds = {k: core.lm_predict(labels=batch["mask"], k=k) for k in (1, 5, 8)}
    for k, p in preds.items():
        assert torch.equal(p.rows.cpu().long(), rows) and tuple(p.ids.shape) == (rows.numel(), k)
        assert np.array_equal(p.ids.cpu().numpy(), SR.topk_ids(xs, k)), k
        assert np.array_equal(p.label_rank.cpu().numpy(), SR.label_rank(xs, labels[rows].numpy())), k
        want = torch.from_numpy(xs).double()
        lp = torch.gather(want, 1, p.ids.cpu().long()) - torch.logsumexp(want, 1)[:, None]
        assert float((p.logprobs.cpu().double() - lp).abs().max()) <= (VOCAB + 8) * 2.0 ** -24 + 2.0 ** -21 * float(want.abs().max() + lp.abs().max())
    # labels from the device: the same result; rows=: the same ids, no label outputs
    dev = core.lm_predict(labels=batch["mask"].to(DEV), k=5)
    for a, b in zip(dev, preds[5]):
        assert torch.equal(bits(a), bits(b))
    by_rows = core.lm_predict(rows=rows, k=5)
    assert by_rows.label_logprob is None and by_rows.label_rank is None
    for a, b in zip(by_rows[:3], preds[5][:3]):
        assert torch.equal(bits(a), bits(b))
    assert torch.equal(core.lm_predict(rows=[47, 0], k=1).ids.cpu().long().flatten(), torch.from_numpy(SR.topk_ids(scores[[47, 0]].numpy(), 1)).flatten())
    # no row: empty tensors and no launch; bad arguments
    none = torch.full((B, T), -1, dtype=torch.int64)
    empty = []
    assert _launches(lambda: empty.append(core.lm_predict(labels=none, k=5))) == 0
    e = empty[0]
    assert tuple(e.ids.shape) == (0, 5) and tuple(e.logprobs.shape) == (0, 5) and e.rows.numel() == e.label_rank.numel() == e.label_logprob.numel() == 0
    assert core.lm_predict(rows=[], k=8).label_rank is None
    for kw in (dict(), dict(labels=batch["mask"], rows=rows)):
        with pytest.raises(ValueError, match="exactly one"):
            core.lm_predict(**kw)
    with pytest.raises(ValueError, match="1, 5 or 8"):
        core.lm_predict(labels=batch["mask"], k=3)
    with pytest.raises(ValueError, match="rows must lie"):
        core.lm_predict(rows=[B * T], k=1)


def test_lm_predict_against_the_fp64_reference_where_it_separates_the_winner():
    """The fp64 reference's top-k from the step's own states, compared only on rows whose reference gap between the k-th and the (k + 1)-th
    value exceeds twice the budget (the row's largest: either side may move by one budget, so on such a row the top-k SET is determined);
    at most a quarter of the rows may be left out.  At this size -- 130 scores of standard deviation 0.16 per row against a budget of
    0.005 .. 0.012 -- the rule keeps most rows only at k = 1: measured over model seeds 1, 2, 3, 7 and two batches, it leaves out 4 to 18 of
    the 48 rows at k = 1 and 24 to 39 at k = 5, so no seed meets the cap at k = 5 and the comparison runs at k = 1, on all 48 rows (rows=),
    with model seed 1 (4 of 48 left out for this batch).  k = 5 and 8 are pinned exactly against the scores of the same forward above.
    The emulation alone (bf16 storage, no kernel) picks the reference's winner on the kept rows too."""
    cfg = C.tiny_config(vocab_size=VOCAB)
    model, params = build_model(cfg, C.default_params(categories=9, L1=True), weights=None, seed=1)
    model.train()
    core = model.bert_pretrained
    batch = S.make_batch(B, T, 5, cfg.v_feature_size, categories=9, vocab_size=VOCAB, seed=11)
    core.return_sequence_outputs = True
    step_forward(model, batch, params)
    pred = core.lm_predict(rows=torch.arange(B * T), k=1)
    w, x = head_weights(core), seq_rows(core)
    ref, emu, bud = SR.reference(w, x)["scores"], SR.emulate(w, x)["scores"], SR.budget(w, x)["scores"]
    top = torch.sort(ref, 1, descending=True).values
    keep = (top[:, 0] - top[:, 1]) > 2.0 * bud.max(1).values
    left_out = int((~keep).sum())
    print("k 1: %d of %d rows left out" % (left_out, B * T))
    assert 4 * left_out <= B * T
    want = ref.argmax(1)
    assert torch.equal(pred.ids.cpu().long().flatten()[keep], want[keep])
    assert torch.equal(emu.argmax(1)[keep], want[keep])
    lp = (top[:, 0] - torch.logsumexp(ref, 1))[keep]                                    # the winner's log-probability: one budget on the value, at most one on lse
    assert bool(((pred.logprobs.cpu().double().flatten()[keep] - lp).abs() <= 2.0 * bud.max(1).values[keep]).all())


# ------------------------------------------------------------------------------------------------ masked_lm_evaluate
def test_masked_lm_evaluate_counts_and_loss():
    from crct.evaluation import masked_lm_evaluate
    cfg, model, params, core, batch = make()
    batches = [batch]
    for seed in (5, 6):
        g = torch.Generator().manual_seed(seed)
        b = dict(S.make_batch(B, T, 5, cfg.v_feature_size, categories=9, vocab_size=VOCAB, seed=30 + seed))
        b["mask"] = torch.where(torch.rand(B, T, generator=g) < 0.3, torch.randint(0, VOCAB, (B, T), generator=g), torch.full((B, T), -1))
        batches.append(b)
    batches[1]["mask"] = torch.full((B, T), -1, dtype=torch.int64)                      # a batch without a label
    params = dict(params, device=DEV)
    res = masked_lm_evaluate(batches, params, model, topk=(1, 5))
    assert model.training                                                               # the mode is put back
    # the same sums from per-batch lm_predict results
    model.eval()
    n, hits, nll = 0, {1: 0, 5: 0}, torch.zeros(1, dtype=torch.float64, device=DEV)
    tol, train_sum = 0.0, 0.0
    core.return_lm_scores = True
    with torch.no_grad():
        for b in batches:
            step_forward(model, b, params, evaluation=True)
            p = core.lm_predict(labels=b["mask"], k=5)
            if p.rows.numel() == 0:
                continue
            n += p.rows.numel()
            for k in hits:
                hits[k] += int((p.label_rank < k).sum())
            nll += (-p.label_logprob.double()).sum()
            # the training tuple's lm_loss of the same batch in eval() (dropout off: the same states), and what the two may differ by: per
            # row the cross-entropy kernel's bound B for loss_r, B + 2^-23 |value| for label_logprob, plus the fp32 mean of the R losses
            lm = step_forward(model, b, params)[1]
            xs = core.prediction_scores_t.double().cpu().reshape(-1, VOCAB)[p.rows.cpu().long()]
            lse = torch.logsumexp(xs, 1)
            bound = (VOCAB + 8) * 2.0 ** -24 + 2.0 ** -22 * (xs.max(1).values.abs() + lse.abs())
            Rb = p.rows.numel()
            tol += float((2.0 * bound + 2.0 ** -23 * p.label_logprob.double().cpu().abs()).sum()) + (Rb + 8) * 2.0 ** -24 * abs(float(lm)) * Rb
            train_sum += float(lm.double()) * Rb
    model.train()
    assert res["n"] == n and n > 0
    loss = float(nll.cpu()) / n
    assert res["loss"] == loss and res["perplexity"] == math.exp(loss)
    assert res["acc"] == {k: hits[k] / n for k in (1, 5)} and res["acc"][5] >= res["acc"][1]
    print("n %d, loss %.6f against the training tuple's %.6f (tolerance %.2e)" % (n, loss, train_sum / n, tol / n))
    assert abs(loss - train_sum / n) <= tol / n
    # in chunks of three rows: the same tokens and hits; the loss up to the order of the fp64 additions
    core.return_lm_scores = False
    chunked = masked_lm_evaluate(batches, params, model, topk=(1, 5), eval_batch_size=3)
    assert chunked["n"] == n and chunked["acc"] == res["acc"] and abs(chunked["loss"] - loss) <= 1e-12 * abs(loss)
    empty = masked_lm_evaluate([batches[1]], params, model, topk=(1,))
    assert empty["n"] == 0 and math.isnan(empty["loss"]) and math.isnan(empty["acc"][1])


# ------------------------------------------------------------------------------------------------ the real vocabulary
def test_the_bert_vocabulary_end_to_end():
    """vocab_size = 30522 (padded to 30528) at the tiny hidden size, B 2, T 8: scores, predictions and a backward through the scores."""
    V, b, t = 30522, 2, 8
    cfg = C.tiny_config(vocab_size=V)
    model, params = build_model(cfg, C.default_params(categories=9, L1=True), weights=None, seed=7)
    model.train()
    core = model.bert_pretrained
    batch = S.make_batch(b, t, 5, cfg.v_feature_size, categories=9, vocab_size=V, seed=11)
    g = torch.Generator().manual_seed(4)
    batch["mask"] = torch.where(torch.rand(b, t, generator=g) < 0.4, torch.randint(0, V, (b, t), generator=g), torch.full((b, t), -1))
    batch["mask"][0, 0], batch["mask"][1, 7] = 0, V - 1
    core.return_lm_scores = True
    core.return_sequence_outputs = True
    step_forward(model, batch, params)
    scores, seq = core.prediction_scores_t, core.sequence_output_t
    assert tuple(scores.shape) == (b, t, V) and scores.stride() == (t * 30528, 30528, 1)
    # the device's own logits: a second evaluation of the head on the same states gives the same bits, and the view stops at column V
    logits, _ = core.text_head.logits(seq.detach(), torch.arange(b * t, dtype=torch.int32, device=DEV), b * t)
    assert tuple(logits.shape) == (64, 30528) and torch.equal(bits(logits[:b * t, :V]), bits(scores.detach().reshape(-1, V)))
    xs = scores.detach().cpu().reshape(-1, V)
    labels = batch["mask"].reshape(-1)
    rows = (labels >= 0).nonzero().flatten()
    p = core.lm_predict(labels=batch["mask"], k=5)
    assert np.array_equal(p.ids.cpu().numpy(), SR.topk_ids(xs[rows].numpy(), 5))
    assert np.array_equal(p.label_rank.cpu().numpy(), SR.label_rank(xs[rows].numpy(), labels[rows].numpy()))
    assert int(p.ids.max()) < V and int(p.label_rank.max()) < V
    seq.retain_grad()
    core.zero_flat_grads()
    G = upstream((b, t, V), seed=8)
    (scores * G).sum().backward()
    torch.cuda.synchronize()
    w, x = head_weights(core), seq.detach().double().cpu().reshape(-1, H)
    G64 = G.double().cpu().reshape(-1, V)
    ref, bud = SR.reference(w, x, G64), SR.budget(w, x, G64)
    err = (seq.grad.double().cpu().reshape(-1, H) - ref["d_seq"]).abs()
    print("V 30522: d_seq worst |error| / budget %.3f" % float((err / bud["d_seq"]).max()))
    assert bool((err <= bud["d_seq"]).all())
