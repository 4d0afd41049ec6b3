"""What ``core.return_sequence_outputs`` costs: the four launches it adds to a training step -- two ln_rows_f32 (the fp32 final hidden
states rebuilt after the forward) and two hidden_grad_add (their upstream gradients added onto the hidden gradients in segment 0) -- at
BASELINE configs[1] (B 80, V 36, T 20, F_v 2048) and at the reference's own PlotQA shape (B 80, V 44, T 124, F_v 1024).  Resident batches,
dropout on, no optimizer.  The aux term is a fixed cotangent on both states, so backward receives a dense fp32 upstream for each.

Two ways to read it:
  * under ``rocprofv3 --kernel-trace --stats -- python tools/seq_outputs_time.py --steps 20``: the rows ln_rows_f32_kernel and
    hidden_grad_add_kernel of the kernel statistics are the device time of the launches themselves;
  * on its own: forward + backward time with the flag off, on with the outputs unused, and on with the aux term, timed in alternation
    (--rounds times --steps steps each); one JSON line per form with every round's time and the smallest.  "on + aux" includes the torch
    kernels of the aux term itself (a product and a sum per state).

    python tools/seq_outputs_time.py [--steps 20] [--warmup 5] [--rounds 4]
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
FORMS = ("off", "on, unused", "on + aux")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4, help="alternations of the three forms")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for shape, (B, V, T, Fv) in SHAPES.items():
        cfg = C.vilbert_config(v_feature_size=Fv)
        params = C.default_params(device=dev, quiet_init=True, max_vis_features=V, max_seq_len=T)
        model = VisualDialogEncoder(params, config=cfg)
        core = model.bert_pretrained
        S.seeded_fill_(model.state_dict(), base_seed=7)
        core._invalidate_shadow()
        batch = {k: v.to(dev) for k, v in S.make_batch(B, T, V, Fv, seed=17).items()}
        gen = torch.Generator().manual_seed(3)
        Ct = (torch.randn(B, T, cfg.hidden_size, generator=gen) * 1e-4).to(dev)
        Cv = (torch.randn(B, V, cfg.v_hidden_size, generator=gen) * 1e-4).to(dev)

        def step(form):
            core.return_sequence_outputs = form != "off"
            core.zero_flat_grads(lazy=True)
            loss = step_forward(model, batch, params)[0]
            if form == "on + aux":
                loss = loss + (Ct * core.sequence_output_t).sum() + (Cv * core.sequence_output_v).sum()
            loss.backward()

        def timed(form, n):
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(n):
                step(form)
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1) / n

        for form in FORMS:                            # warm up every form, then alternate them: clocks and neighbours drift
            for _ in range(args.warmup):
                step(form)
        ms = {form: [] for form in FORMS}
        for _ in range(args.rounds):
            for form in FORMS:
                step(form)
                ms[form].append(timed(form, args.steps))
        for form in FORMS:
            print(json.dumps(dict(shape=shape, B=B, V=V, T=T, F_v=Fv, sequence_outputs=form, steps=args.steps, rounds=args.rounds,
                                  fwd_bwd_ms=[round(v, 3) for v in ms[form]], fwd_bwd_ms_min=round(min(ms[form]), 3))), flush=True)
        core.return_sequence_outputs = False
        del model, core
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
