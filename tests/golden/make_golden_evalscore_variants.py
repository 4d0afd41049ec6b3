"""Generate the DVQA / FigureQA evaluation-scoring fixtures by RUNNING THE REFERENCE's evaluation loop (build container only).

The recipe of ``make_golden.eval_scoring_case`` (CRCT/evaluation.py ``plotqa_evaluate_DDP`` :199-386 on synthetic candidate
batches; ``pytorch_transformers`` shim, single-process gloo group, ``.cuda()`` as the identity) for the model variants:

  evalscore_figureqa     dataset 'figure_qa', binary_answers (:280-285): one row per question, answer = round(p0)
  evalscore_dvqa         dataset 'dvqa', PlotQA regressor, evaluation snap to dvqa_floats (vilbert.py:1619-1625)
  evalscore_dvqa_ce      dataset 'dvqa', CE_REG (vilbert.py:1603-1615), ce_fusion.6 bias bump as in make_golden_variants.py
  evalscore_dvqa_cls     dataset 'dvqa', a '_cls' question file: no regressor (vilbert.py:1518), no regression question

Each case: 3 batches of 8 to 12 questions.  The labels are designed from the model's own predictions so that every branch of
the scoring is hit (right / wrong class, both error measures right, one right and the other wrong, wrong candidate with a fine
regression).  Every file holds the inputs (without the image features, which the variant models never read: drawn again from
``meta['feat_seed']`` + batch index), the per-row ``nsp_scores`` / ``reg0`` / ``reg2`` / ``reg4``, the ``total_correct`` the
reference returned, and the meta.

A bf16 forward may move a logit by up to 3e-2, so the GPU tests allow 2 differing questions per table row against the
reference.  So that this allowance cannot hide a scoring error, ``meta['near_ties']`` counts the questions a bounded forward
error could flip -- a top-two p0 gap (as a logit-difference gap) below 6e-2, for binary answers |l0 - l1| below 6e-2, a
designed regression margin below 1 % of the threshold's scale, a DVQA snap closer than 3e-2 * scale to a midpoint of the value
table, a CE top-two logit gap below 6e-2 -- and the seeds below are chosen so that it is at most 2 (asserted).

    python tests/golden/make_golden_evalscore_variants.py
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG                    # noqa: E402  (sys.path set up there: crct, oracle)
import make_golden_variants as MV           # noqa: E402
from crct import config as C                # noqa: E402
from crct import synthetic as S             # noqa: E402

LOGIT_BOUND = 3e-2                           # documented bound of a bf16 forward on the nsp logits (tests/test_variants_gpu.py)
CE_BUMP = (17, 4.0)
# The seeded weights of the other fixtures (N(0, 0.02)) give a tiny model whose logits hardly depend on the row (l0 - l1 within 1e-3
# of each other): every question would be a near tie.  These fixtures draw the weights at WEIGHT_STD (rows then differ by some 0.25 in
# l0 - l1, the tanh regressor stays unsaturated), widen the answer head by HEAD_SCALE and, for the binary case, shift its bias so that
# both answers occur.  meta carries all three; the tests build the model the same way.
WEIGHT_STD, HEAD_SCALE = 0.08, 10.0
#        name                   kind       batch seed, feat seed, head bias[1] shift
CASES = [("evalscore_figureqa", "figureqa", 412, 4100, 1.6),
         ("evalscore_dvqa", "dvqa", 421, 4200, 0.0),
         ("evalscore_dvqa_ce", "dvqa_ce", 432, 4300, 0.0),
         ("evalscore_dvqa_cls", "dvqa_cls", 444, 4400, 0.0)]


def import_evaluation():
    pt = types.ModuleType("pytorch_transformers")
    tb = types.ModuleType("pytorch_transformers.tokenization_bert")
    tb.BertTokenizer = type("BertTokenizer", (), {})
    pt.tokenization_bert = tb
    sys.modules["pytorch_transformers"] = pt
    sys.modules["pytorch_transformers.tokenization_bert"] = tb
    sys.modules.setdefault("pandas", __import__("pandas"))
    import importlib
    return importlib.import_module("evaluation")


def make_batches(kind, cfg, seed, feat_seed, n_batches=3):
    """Evaluation batches after cut_batch_padding: candidate rows concatenated, per-question tensors [Q, 1]."""
    g = np.random.RandomState(seed)
    batches = []
    qa = 5000
    for bi in range(n_batches):
        Q = int(g.randint(8, 13))
        num_ans = np.ones(Q, dtype=np.int64) if kind == "figureqa" else g.randint(1, 5, size=Q).astype(np.int64)
        N = int(num_ans.sum())
        b = dict(S.make_batch(N, 7, 5, cfg.v_feature_size, categories=9, vocab_size=cfg.vocab_size, seed=seed + 1 + bi))
        b["image_feat"] = MV.variant_features(N, 5, cfg.v_feature_size, feat_seed + bi)
        ga = torch.Generator().manual_seed(seed + 50 + bi)
        b["areas"] = torch.rand(N, 5, 1, generator=ga, dtype=torch.float32) * 2.0
        b["R"] = torch.zeros(N, 4)
        b["num_ans"] = torch.from_numpy(num_ans).view(Q, 1)
        b["id"] = torch.arange(qa, qa + Q, dtype=torch.int64).view(Q, 1)
        b["gt_id"] = torch.zeros(Q, 1, dtype=torch.int64)
        b["needs_reg"] = torch.zeros(Q, 1, dtype=torch.bool)
        b["tolerance_margin"] = torch.zeros(Q, 1)
        b["gt"] = torch.zeros(Q, 1)
        b["reg_target"] = torch.zeros(Q, 1)
        qa += Q
        batches.append(b)
    return batches


def clone(b):
    return {k: (v.clone() if torch.is_tensor(v) else list(v)) for k, v in b.items()}


def snap_margin(x, values):
    """Distance of x to the nearest midpoint between two neighbouring table values."""
    v = np.sort(np.asarray(values, dtype=np.float64))
    return float(np.abs((v[1:] + v[:-1]) / 2 - x).min())


def design(kind, b, model, ed, params, case, ce_logits):
    """Set the labels / regression targets of batch b from the model's predictions; returns (next case number, near ties)."""
    N, Q = b["tokens"].shape[0], b["num_ans"].shape[0]
    vals = params.get("dvqa_floats")
    near = 0
    probe = clone(b)
    regress = kind in ("dvqa", "dvqa_ce")
    probe["R"] = torch.tensor([[0.0 if kind == "dvqa_ce" else 1.0, 1.0 if regress else 0.0, 0.0, 1.0]]).repeat(N, 1)
    model.train()                                  # no snap (vilbert.py:1621): reg[0] is the raw tanh output; the tiny config has no dropout
    del ce_logits[:]
    with torch.no_grad():
        out = ed.forward(model, probe, params, output_nsp_scores=True, evaluation=True)
    logits = out[4]
    p0 = torch.softmax(logits, dim=1)[:, 0]
    r_raw = out[5][0]
    off = 0
    for q in range(Q):
        n = int(b["num_ans"][q])
        kinds = 2 if not regress else 6
        k = case % kinds
        case += 1
        needs, tol, scale, target = False, 0.0, 0.0, 0.0
        if kind == "figureqa":
            a = int(torch.round(p0[off]))
            b["next_sentence_labels"][off, 0] = (1 - a) if k == 0 else a            # right / wrong
            gt_id = a
            near += int(abs(float(logits[off, 0] - logits[off, 1])) < 2 * LOGIT_BOUND)
        else:
            a = int(torch.argmax(p0[off:off + n]))
            d = (logits[off:off + n, 0] - logits[off:off + n, 1]).numpy()           # p0 is monotone in l0 - l1
            near += int(n > 1 and float(np.sort(d)[-1] - np.sort(d)[-2]) < 2 * LOGIT_BOUND)
            gt_id = a
            if k in (1, 5):
                gt_id = (a + 1) % n if n > 1 else a                                 # wrong candidate (k 5: with a fine regression)
            if kind == "dvqa" and k >= 2:
                raw = float(r_raw[off + a])
                scale = float(np.float32(1.0 / abs(raw)))                           # raw * scale = +-1: a table value, 0.5 from the next midpoint
                near += int(snap_margin(raw * scale, vals) < LOGIT_BOUND * scale)
                r = float(np.float32(np.sign(raw)) / np.float32(scale))             # the snapped prediction in normalised units
                needs = True
                if k == 2:
                    target, tol = r * 1.02, 0.5                                     # both measures right
                elif k == 3:
                    target, tol = r * 1.03, abs(r) * 0.001                          # 5 % right, tick tolerance wrong
                elif k == 4:
                    target, tol = r * 1.5, abs(r) + 1.0                             # 5 % wrong, tick tolerance right
                else:
                    target, tol = r * 1.01, 0.5
                gt, reg_target, r0 = target * scale, target, target * scale
            elif kind == "dvqa_ce" and k >= 2:
                z = ce_logits[0][off + a].numpy()
                chosen = int(np.argmax(z))
                near += int(float(np.sort(z)[-1] - np.sort(z)[-2]) < 2 * LOGIT_BOUND)
                needs, scale = True, 1.0
                cls = chosen
                if k == 2:
                    tol = 0.5                                                       # both measures right (errors are 0)
                elif k == 3:
                    tol = -1.0                                                      # 5 % right, tick tolerance wrong
                elif k == 4:
                    cls, tol = chosen + 1, 2.0                                      # 5 % wrong (|value difference| = 1), tick tolerance right
                else:
                    tol = 0.5
                gt, reg_target, r0 = vals[cls], float(cls), float(cls)              # R[:, 0] is the class index (fig_dataloader.py:628-629)
        if needs:
            b["R"][off:off + n] = torch.tensor([r0, 1.0, tol, scale])
            b["gt"][q, 0], b["reg_target"][q, 0] = gt, reg_target
        b["gt_id"][q, 0] = gt_id
        b["needs_reg"][q, 0] = needs
        b["tolerance_margin"][q, 0] = tol
        off += n
    return case, near


def build(kind, vilbert, ed, head_shift):
    """The reference model of a case: seeded weights at WEIGHT_STD, the answer head widened (HEAD_SCALE, head_shift), CE bump."""
    cfg = C.tiny_config()
    extra = dict(categories=9, L1=True, ddp=True, world_size=1, rank=0, save_path="/tmp", eval_set="val", start_checkpoint="none/tiny.ckpt")
    if kind == "dvqa_cls":
        extra.update(qa_file="qa_cls", BOT_MODE=False)          # no regressor to call (vilbert.py:1518, 1598)
    params = MV.variant_params("dvqa" if kind == "dvqa_cls" else kind, **extra)
    params["device"] = torch.device("cpu")
    model = MG.build_reference_model(vilbert, ed, cfg, params)
    S.seeded_fill_(model.state_dict(), base_seed=7, std=WEIGHT_STD)
    core = model.bert_pretrained
    bump = CE_BUMP if kind == "dvqa_ce" else None
    ce_logits = []
    with torch.no_grad():
        core.cls.bi_seq_relationship.weight *= HEAD_SCALE
        core.cls.bi_seq_relationship.bias[1] += head_shift
        if bump:
            core.regressor.ce_fusion[6].bias[bump[0]] += bump[1]
    if bump:
        core.regressor.ce_fusion[6].register_forward_hook(lambda m, i, o: ce_logits.append(o.detach().clone()))
    return cfg, params, model, bump, ce_logits


def run_case(name, kind, seed, feat_seed, head_shift, vilbert, ed, evaluation):
    import torch.distributed as dist
    cfg, params, model, bump, ce_logits = build(kind, vilbert, ed, head_shift)
    batches = make_batches(kind, cfg, seed, feat_seed)
    case, near = 0, 0
    for b in batches:
        case, n = design(kind, b, model, ed, params, case, ce_logits)
        near += n
    model.train()

    class Dataset(object):
        def cut_batch_padding(self, item):
            pass

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29573")
    dist.init_process_group(backend="gloo", rank=0, world_size=1)
    old_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        total, breakdown = evaluation.plotqa_evaluate_DDP([clone(b) for b in batches], Dataset(), params, 5, model, progress=False, csv=False)
    finally:
        torch.Tensor.cuda = old_cuda
        dist.destroy_process_group()
    assert float(breakdown.abs().sum()) == 0.0                     # built for PlotQA only (:331)
    rec = {"total_correct": total.numpy(), "n_batches": np.array(len(batches)), "eval_batch_size": np.array(5)}
    model.eval()
    for bi, b in enumerate(batches):
        with torch.no_grad():
            out = ed.forward(model, clone(b), params, output_nsp_scores=True, evaluation=True)
        rec["b%d.nsp_scores" % bi] = out[4].numpy()
        for j in (0, 2, 4):
            rec["b%d.reg%d" % (bi, j)] = out[5][j].numpy()
        for k, v in b.items():
            if torch.is_tensor(v) and k != "image_feat":
                rec["b%d.in.%s" % (bi, k)] = v.numpy()
        # designed regression margins: the chosen row's two errors against their thresholds (1 % as in make_golden.eval_scoring_case)
        p0 = torch.softmax(out[4], dim=1)[:, 0]
        off = 0
        for q in range(b["num_ans"].shape[0]):
            n = int(b["num_ans"][q])
            if bool(b["needs_reg"][q]):
                a = off + int(torch.argmax(p0[off:off + n]))
                near += int(abs(float(out[5][4][a]) - 0.05) < 0.01 or abs(float(out[5][2][a]) - float(b["tolerance_margin"][q])) < 0.01 * abs(float(b["reg_target"][q])))
            off += n
    assert near <= 2, "%s: %d questions inside the forward's error bound: choose another seed" % (name, near)
    meta = dict(cfg=cfg.to_dict(), params={k: v for k, v in params.items() if k != "device"}, weight_seed=7, ce_bias_bump=bump,
                feat_seed=feat_seed, near_ties=near, logit_bound=LOGIT_BOUND, weight_std=WEIGHT_STD, head_scale=HEAD_SCALE,
                head_shift=head_shift)
    rec["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **rec)
    print("  wrote %s (%.1f KB); near ties %d; total_correct =\n%s" % (path, os.path.getsize(path) / 1024, near, total.numpy()))


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    vilbert, ed = MG.import_reference()
    evaluation = import_evaluation()
    for name, kind, seed, feat_seed, head_shift in CASES:
        run_case(name, kind, seed, feat_seed, head_shift, vilbert, ed, evaluation)


if __name__ == "__main__":
    main()
