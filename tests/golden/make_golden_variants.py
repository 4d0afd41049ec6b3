"""Generate the DVQA / FigureQA variant fixtures by RUNNING THE REFERENCE (build container only).

Same recipe as make_golden.py -- the reference model imported on CPU, name-keyed seeded weights (crct.synthetic.seeded_fill_),
seeded synthetic batches fed through the reference's own ``encoder_decorator.forward`` + ``loss.backward()`` -- for the model
variants the oracle does not restate (vilbert.py:1459-1537, 1596-1625; regressor.py:45-79):

  variant_tiny_dvqa_ce        dataset 'dvqa', CE_REG, with areas: every gradient (1024-element samples of tensors above 4 K)
  variant_tiny_dvqa           dataset 'dvqa', PlotQA regressor, SmoothL1, with areas: the same
  variant_tiny_dvqa_eval      the same model in evaluation mode (the snap to dvqa_floats)
  variant_tiny_figureqa       dataset 'figure_qa', binary_answers (no regressor), with areas: the same
  variant_full_dvqa_ce        config/vilbert.json at DVQA's shape (B 4, V 30, T 124): 64-element gradient samples
  variant_full_figureqa       config/vilbert.json at FigureQA's shape (B 4, V 70, T 64): 64-element gradient samples

The image features are not stored: the variants never read them (vilbert.py:1481-1483), so they are drawn from
``meta['feat_seed']`` by ``variant_features`` and the tests draw them again; the gradient samples sit at ``sample_index``
positions, which the tests recompute too.  That keeps every file under 1 MB.  Every file's ``meta`` also carries the reference's ``named_parameters()`` and ``state_dict()`` key lists with shapes.  The CE
draws add ``meta['ce_bias_bump']`` to one class's ce_fusion.6 bias (applied again after the seeded fill by the tests), so that the top-2 probability margin is clear and bf16
rounding cannot flip the argmax.

    python tests/golden/make_golden_variants.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG              # noqa: E402  (sys.path set up there: crct, oracle)
from crct import config as C          # noqa: E402
from crct import synthetic as S       # noqa: E402

DVQA_FLOATS = [-9.0, -8.0, -7.0, -6.0, -5.0, -4.0, -3.0, -2.0, -1.0] + [float(v) for v in range(0, 42)] + \
              [43.0, 50.0, 60.0, 70.0, 80.0, 90.0, 100.0, 1000.0, 10000.0, 100000.0, 1000000.0, 10000000.0, 100000000.0, 1000000000.0]
assert len(DVQA_FLOATS) == 65


def variant_params(kind, **kw):
    if kind.startswith("dvqa"):
        p = C.default_params(dataset="dvqa", categories=62, max_seq_len=124, max_vis_features=30, binary_answers=False,
                             CE_REG=(kind == "dvqa_ce"), dvqa_floats=list(DVQA_FLOATS))
    else:
        p = C.default_params(dataset="figure_qa", categories=258, max_seq_len=64, max_vis_features=70, binary_answers=True,
                             max_previews=10, BOT_MODE=False)
    p.update(kw)
    return p


def variant_features(B, V, F_v, seed):
    """The image features of a variant fixture (never read by the variant models): N(0, 1), fp16-exact."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, V, F_v, generator=g, dtype=torch.float32).half().float()


def sample_index(numel, n):
    """n evenly spaced element positions of a flattened tensor (first and last included)."""
    n = min(numel, n)
    return (torch.arange(n, dtype=torch.int64) * (numel - 1)) // max(n - 1, 1)


def add_areas(batch, seed):
    B, V, F_v = batch["image_feat"].shape
    batch["image_feat"] = variant_features(B, V, F_v, seed + 1000)    # meta['feat_seed'] of run_variant
    g = torch.Generator().manual_seed(seed)
    B, V = batch["image_target"].shape
    # spread over [0, 2): the areas Linear's weight gradient is an areas-weighted column sum, and a narrow spread leaves it close to
    # a multiple of the bias gradient plus bf16 noise (a [0, 0.5) draw gave cosine 0.979 on the tiny CE case, 0.9998 under autocast)
    batch["areas"] = torch.rand(B, V, 1, generator=g, dtype=torch.float32) * 2.0
    return batch


def run_variant(name, cfg, params, batch, vilbert, ed, save_weights, evaluation=False, ce_bump=None, feat_seed=None):
    params = dict(params)
    params["device"] = torch.device("cpu")
    model = MG.build_reference_model(vilbert, ed, cfg, params)
    S.seeded_fill_(model.state_dict(), base_seed=7)
    if ce_bump is not None:
        with torch.no_grad():
            model.bert_pretrained.regressor.ce_fusion[6].bias[ce_bump[0]] += ce_bump[1]
    if evaluation:
        model.eval()
    sd = {k[len("bert_pretrained."):]: v for k, v in model.named_parameters()}
    out = ed.forward(model, {k: v.clone() for k, v in batch.items()}, params, evaluation=evaluation)
    if evaluation:
        loss, lm, nsp, img, scores, reg = out
    else:
        loss, lm, nsp, img, scores, reg, leg = out
        loss.backward()
    rec = {"in." + k: v.numpy() for k, v in batch.items() if k != "image_feat"}
    rec["out.nsp_scores"] = scores.detach().numpy()
    rec["out.reg_pred"] = reg[0].detach().numpy()
    rec["out.reg_loss"] = reg[1].detach().numpy()
    rec["out.reg_l1"] = reg[2].detach().numpy()
    rec["out.reg_right"] = np.array(reg[3], dtype=np.int64)
    rec["out.reg_dist5"] = reg[4].detach().numpy()
    if not evaluation:
        rec["out.loss"] = np.array(float(loss), dtype=np.float64)
        rec["out.nsp_loss"] = nsp.detach().numpy()
        for k, p in sd.items():
            if p.grad is None:
                rec["gradnorm." + k] = np.array(-1.0)
                continue
            g = p.grad
            rec["gradnorm." + k] = np.array(float(g.double().norm()))
            if save_weights and g.numel() <= 4096:
                rec["grad." + k] = g.numpy()
            else:             # tiny cases: 1024 evenly spaced elements of the larger tensors (keeps a file under 1 MB)
                flat = g.reshape(-1)
                rec["gradsample." + k] = flat[sample_index(flat.numel(), 1024 if save_weights else 64)].numpy()
    meta = dict(cfg=cfg.to_dict(), params={k: v for k, v in params.items() if k != "device"}, evaluation=evaluation, weight_seed=7,
                cls_dropout=0.0, ce_bias_bump=ce_bump, feat_seed=feat_seed,
                named_parameters=[[k, list(p.shape)] for k, p in sd.items()],
                state_dict=[[k, list(v.shape)] for k, v in model.bert_pretrained.state_dict().items()])
    rec["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **rec)
    print("  wrote %s (%.1f KB)  loss %s  reg_right %s" % (path, os.path.getsize(path) / 1024,
                                                        "-" if evaluation else "%.6f" % float(loss), tuple(reg[3])))


def ce_targets(batch, chosen, seed):
    """Class targets in R[:, 0] (fig_dataloader.py:628-629): half the rows on the bumped class (right), the rest elsewhere."""
    g = torch.Generator().manual_seed(seed)
    B = batch["R"].shape[0]
    t = torch.randint(0, 65, (B,), generator=g).float()
    t[t == chosen] = (chosen + 1) % 65
    t[::2] = float(chosen)
    batch["R"][:, 0] = t
    batch["R"][:, 1] = 1.0
    batch["R"][1, 1] = 0.0
    batch["needs_reg"] = (batch["R"][:, 1:2] == 1)
    return batch


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    vilbert, ed = MG.import_reference()
    tiny = C.tiny_config()
    # ---- DVQA, CE_REG (L1 loss kind for the SmoothL1 / L1 choice is irrelevant to CE), areas
    p = variant_params("dvqa_ce", categories=9)
    b = add_areas(S.make_batch(4, 7, 5, tiny.v_feature_size, categories=9, vocab_size=tiny.vocab_size, seed=21), seed=22)
    b = ce_targets(b, 17, seed=23)
    b["next_sentence_labels"][2, 0] = -1
    run_variant("variant_tiny_dvqa_ce", tiny, p, b, vilbert, ed, save_weights=True, ce_bump=(17, 4.0), feat_seed=1022)
    # ---- DVQA with the PlotQA regressor (SmoothL1), areas; and its evaluation (snap)
    p = variant_params("dvqa", categories=9, L1=False)
    b = add_areas(S.make_batch(4, 7, 5, tiny.v_feature_size, categories=9, vocab_size=tiny.vocab_size, seed=31), seed=32)
    b["R"][:, 1] = torch.tensor([1.0, 1.0, 0.0, 1.0])
    b["R"][:, 3] = 40.0
    b["R"][:, 0] = torch.tensor([12.0, 3.0, 7.0, 30.0])
    b["needs_reg"] = (b["R"][:, 1:2] == 1)
    run_variant("variant_tiny_dvqa", tiny, p, b, vilbert, ed, save_weights=True, feat_seed=1032)
    run_variant("variant_tiny_dvqa_eval", tiny, p, b, vilbert, ed, save_weights=False, evaluation=True, feat_seed=1032)
    # ---- FigureQA: binary answers (no regressor module, no regression rows), areas
    p = variant_params("figureqa", categories=9)
    b = add_areas(S.make_batch(4, 7, 5, tiny.v_feature_size, categories=9, vocab_size=tiny.vocab_size, seed=41), seed=42)
    b["R"][:, 1] = 0.0
    b["needs_reg"] = (b["R"][:, 1:2] == 1)
    run_variant("variant_tiny_figureqa", tiny, p, b, vilbert, ed, save_weights=True, feat_seed=1042)
    # ---- full config at each dataset's own shape
    cfg = C.vilbert_config(v_feature_size=1024, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                           v_hidden_dropout_prob=0.0, v_attention_probs_dropout_prob=0.0)
    p = variant_params("dvqa_ce")
    b = add_areas(S.make_batch(4, 124, 30, 1024, categories=62, seed=51, lengths=[124, 80, 101, 117], n_vis=[30, 21, 27, 30]), seed=52)
    b = ce_targets(b, 40, seed=53)
    run_variant("variant_full_dvqa_ce", cfg, p, b, vilbert, ed, save_weights=False, ce_bump=(40, 4.0), feat_seed=1052)
    p = variant_params("figureqa")
    # seed 71: seed 61 was a cancelling draw for the visual pooler (its bias gradient 3.2 % / cosine 0.985 off under the reference's
    # own bf16 autocast), the situation make_golden.py describes for the PlotQA T = 124 fixture
    b = add_areas(S.make_batch(4, 64, 70, 1024, categories=258, seed=71, lengths=[64, 40, 57, 61], n_vis=[70, 48, 66, 70]), seed=72)
    b["R"][:, 1] = 0.0
    b["needs_reg"] = (b["R"][:, 1:2] == 1)
    run_variant("variant_full_figureqa", cfg, p, b, vilbert, ed, save_weights=False, feat_seed=1072)


if __name__ == "__main__":
    main()
