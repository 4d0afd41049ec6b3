"""What the masked-LM predictions cost at the reference's PlotQA shape (B 80, V 44, T 124, F_v 1024; BERT vocabulary): with 15 % of the real
tokens labelled (``lm_predict(labels=...)``) and over all B * T rows (``return_lm_scores``).  One process, forms alternated (--rounds times
--steps launches each), one JSON line per measurement:

  rows      ``lm_topk_rows`` at k = 1, 5, 8 beside ``lm_ce_fwd`` on the SAME fp32 logits [Rp, Vp] (both sweep the row twice), and stock
            ``torch.topk`` + ``torch.logsumexp`` on them; with the bytes/s of the two row kernels counted as ONE read of the R x V logits
            (the second sweep of a 122 KB row comes from L2) -- at R = the labelled rows and at R = B * T
  predict   the whole ``lm_predict(labels=..., k)`` call after an evaluation forward (gather, two GEMMs, LayerNorm, top-k; host side included)
  forward   the evaluation forward with and without ``return_lm_scores``, and the bytes the full scores take

    python tools/lm_predict_time.py [--mask-prob 0.15] [--steps 20] [--warmup 3] [--rounds 4]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cqa-crct_amd"))

from crct import config as C                       # noqa: E402
from crct import ops                               # noqa: E402
from crct import synthetic as S                    # noqa: E402
from crct.heads import lm_rows                     # noqa: E402
from crct.model import VisualDialogEncoder         # noqa: E402
from crct.step_adapter import forward as step_forward   # noqa: E402

B, V, T, FV = 80, 44, 124, 1024


def timed(fn, n):
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n


def alternate(forms, args):
    """{name: [ms per round]} of the callables in ``forms``, warmed up and then timed in alternation."""
    for fn in forms.values():
        for _ in range(args.warmup):
            fn()
    ms = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k, fn in forms.items():
            ms[k].append(timed(fn, args.steps))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mask-prob", type=float, default=0.15)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = C.vilbert_config(v_feature_size=FV)
    vocab = cfg.vocab_size
    host = S.make_batch(B, T, V, FV, seed=17)
    gen = torch.Generator().manual_seed(5)
    real = torch.arange(T)[None, :] < (host["sep_indices"][:, 0] + 1)[:, None]
    pick = (torch.rand(B, T, generator=gen) < args.mask_prob) & real
    labels = torch.where(pick, host["tokens"], torch.full((B, T), -1))
    batch = {k: v.to(dev) for k, v in host.items()}
    batch["mask"] = labels                          # on the host, as the loader leaves them
    params = C.default_params(device=dev, quiet_init=True, max_vis_features=V, max_seq_len=T)
    model = VisualDialogEncoder(params, config=cfg)
    S.seeded_fill_(model.state_dict(), base_seed=7)
    core = model.bert_pretrained
    core._invalidate_shadow()
    model.eval()

    def say(**kw):
        print(json.dumps(kw), flush=True)

    with torch.no_grad():
        # ---- forward with and without the scores
        def fwd(on):
            core.return_lm_scores = on
            step_forward(model, batch, params, evaluation=True)
        ms = alternate({"off": lambda: fwd(False), "on": lambda: fwd(True)}, args)
        fwd(True)
        scores = core.prediction_scores_t
        buf_bytes = scores.stride(0) * 4 * B if scores is not None else 0
        for k in ms:
            say(what="forward", return_lm_scores=k, B=B, T=T, vocab=vocab, ms=[round(v, 3) for v in ms[k]], ms_min=round(min(ms[k]), 3),
                scores_bytes=B * T * vocab * 4 if k == "on" else 0, padded_buffer_bytes=buf_bytes if k == "on" else 0)
        # ---- the row kernels on the same logits: the labelled rows, then all rows
        job = core.text_head.upload(lm_rows(labels, vocab))
        seq_t = core._engine.sequence_outputs(visual=False)[0]
        for name, rows, lab, R in (("labelled", job.rows, job.labels, job.R),
                                   ("all", torch.arange(B * T, dtype=torch.int32, device=dev), batch["tokens"].reshape(-1).to(torch.int32), B * T)):
            logits, _ = core.text_head.logits(seq_t, rows, R)
            forms = {"lm_ce_fwd": lambda: ops.lm_ce_fwd(logits, lab, R, vocab, 1.0 / R)}
            for k in (1, 5, 8):
                forms["lm_topk_rows k=%d" % k] = lambda k=k: ops.lm_topk_rows(logits, R, vocab, k, lab)

            def stock(k=5):
                x = logits[:R, :vocab]
                return torch.topk(x, k, dim=1), torch.logsumexp(x, 1)
            forms["torch.topk(5) + logsumexp"] = stock
            ms = alternate(forms, args)
            for k in ms:
                best = min(ms[k])
                say(what="rows", rows=name, R=R, vocab=vocab, kernel=k, ms=[round(v, 4) for v in ms[k]], ms_min=round(best, 4),
                    logits_gb_per_s=round(R * vocab * 4 / best / 1e6, 1))
            del logits
        # ---- the whole lm_predict call
        core.return_lm_scores = False
        step_forward(model, batch, params, evaluation=True)
        ms = alternate({k: (lambda k=k: core.lm_predict(labels=labels, k=k)) for k in (1, 5, 8)}, args)
        for k in ms:
            say(what="predict", k=k, R=job.R, ms=[round(v, 3) for v in ms[k]], ms_min=round(min(ms[k]), 3))


if __name__ == "__main__":
    main()
