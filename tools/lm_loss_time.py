"""What ``params['lm_loss_coeff']`` costs: forward + backward of the training step with the option off and with ``lm_loss_coeff = 1`` at a
masking probability (``--mask-prob``, default 0.15: the labels sit on that share of the real tokens, drawn once per shape), at BASELINE
configs[1] (B 80, V 36, T 20, F_v 2048) or at the reference's own PlotQA shape (B 80, V 44, T 124, F_v 1024).  Resident batches except the
labels, which stay on the host as the reference's loader leaves them; dropout on, no optimizer.  The two forms are two models (the option
is read at construction) on the same seeded weights, timed in alternation (--rounds times --steps steps each); one JSON line per form with
R (the masked rows of the batch), every round's time and the smallest.  The "off" line is the one to hold against the same run of this
file on the parent commit (it knows no such option: ``--off-only`` runs there).

Under ``rocprofv3 --kernel-trace --stats -- python tools/lm_loss_time.py --steps 20`` the rows lm_*_kernel of the kernel statistics are
the device time of the head's own launches; its three vocabulary-sized GEMMs appear among the gemm kernels.

    python tools/lm_loss_time.py [--workload plotqa-real] [--mask-prob 0.15] [--steps 20] [--warmup 5] [--rounds 4] [--off-only]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cqa-crct_amd"))

from crct import config as C                       # noqa: E402
from crct import synthetic as S                    # noqa: E402
from crct.model import VisualDialogEncoder         # noqa: E402
from crct.step_adapter import forward as step_forward   # noqa: E402

SHAPES = {"configs[1]": (80, 36, 20, 2048), "plotqa-real": (80, 44, 124, 1024)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(SHAPES), default="plotqa-real")
    ap.add_argument("--mask-prob", type=float, default=0.15)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4, help="alternations of the forms")
    ap.add_argument("--off-only", action="store_true", help="only the form without the option (any commit runs it)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, V, T, Fv = SHAPES[args.workload]
    cfg = C.vilbert_config(v_feature_size=Fv)
    host = S.make_batch(B, T, V, Fv, seed=17)
    gen = torch.Generator().manual_seed(5)
    real = torch.arange(T)[None, :] < (host["sep_indices"][:, 0] + 1)[:, None]
    pick = (torch.rand(B, T, generator=gen) < args.mask_prob) & real
    labels = torch.where(pick, host["tokens"], torch.full((B, T), -1))
    batch = {k: v.to(dev) for k, v in host.items()}
    batch["mask"] = labels                          # on the host, as train.py leaves them (encoder_decorator.py:85)
    R = int(pick.sum())
    forms = {"off": {}} if args.off_only else {"off": {}, "on": dict(lm_loss_coeff=1.0)}
    runs = {}
    for form, extra in forms.items():
        params = C.default_params(device=dev, quiet_init=True, max_vis_features=V, max_seq_len=T, **extra)
        model = VisualDialogEncoder(params, config=cfg)
        S.seeded_fill_(model.state_dict(), base_seed=7)
        model.bert_pretrained._invalidate_shadow()
        runs[form] = (model, params)

    def step(form):
        model, params = runs[form]
        model.bert_pretrained.zero_flat_grads(lazy=True)
        step_forward(model, batch, params)[0].backward()

    def timed(form, n):
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(n):
            step(form)
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / n

    for form in forms:                                # warm up every form, then alternate them: clocks and neighbours drift
        for _ in range(args.warmup):
            step(form)
    ms = {form: [] for form in forms}
    for _ in range(args.rounds):
        for form in forms:
            step(form)
            ms[form].append(timed(form, args.steps))
    H, vocab = cfg.hidden_size, cfg.vocab_size
    for form in forms:
        print(json.dumps(dict(shape=args.workload, B=B, V=V, T=T, F_v=Fv, lm_loss=form, mask_prob=args.mask_prob, masked_rows=R,
                              vocab_gemm_tflop_estimate=round(3 * 2.0 * R * H * vocab / 1e12, 4) if form == "on" else 0.0,
                              steps=args.steps, rounds=args.rounds, fwd_bwd_ms=[round(v, 3) for v in ms[form]],
                              fwd_bwd_ms_min=round(min(ms[form]), 3))), flush=True)


if __name__ == "__main__":
    main()
