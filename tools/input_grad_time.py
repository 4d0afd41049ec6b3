"""What a request for input gradients costs: forward + backward time of the training step with and without ``image_feat`` /
``image_loc`` / ``loc`` requiring grad and ``keep_text_embedding_grad``, with every parameter trainable and with every parameter
frozen (backward then runs data gradients only), at BASELINE configs[1] (B 80, V 36, T 20, F_v 2048) and at the reference's own
PlotQA shape (B 80, V 44, T 124, F_v 1024).  Resident batches, dropout on, no optimizer: the optimizer's time does not depend on the
request.  The two forms of a setting are timed in alternation (--rounds times --steps steps each); one JSON line per form with
every round's time and the smallest.  The frozen runs without a request run no backward at all and are the forward's time.

    python tools/input_grad_time.py [--steps 20] [--warmup 5] [--rounds 4]
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
FLOAT_INPUTS = ("image_feat", "image_loc", "loc")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4, help="alternations of (without, with) a request per setting")
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

        def set_request(on):
            for k in FLOAT_INPUTS:
                batch[k] = batch[k].detach().requires_grad_(on)
            core.keep_text_embedding_grad = on

        def step():
            for k in FLOAT_INPUTS:
                batch[k].grad = None
            core.zero_flat_grads(lazy=True)
            step_forward(model, batch, params)[0].backward()

        def timed(n):
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(n):
                step()
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1) / n

        for frozen in (False, True):
            for p in core.parameters():
                p.requires_grad_(not frozen)
            for request in (False, True):             # warm up both forms, then alternate them: clocks and neighbours drift
                set_request(request)
                for _ in range(args.warmup):
                    step()
            ms = {False: [], True: []}
            for _ in range(args.rounds):
                for request in (False, True):
                    set_request(request)
                    step()
                    ms[request].append(timed(args.steps))
            for request in (False, True):
                print(json.dumps(dict(shape=shape, B=B, V=V, T=T, F_v=Fv, parameters="frozen" if frozen else "trainable", input_grads=request,
                                      steps=args.steps, rounds=args.rounds, fwd_bwd_ms=[round(v, 3) for v in ms[request]],
                                      fwd_bwd_ms_min=round(min(ms[request]), 3))), flush=True)
        core.keep_text_embedding_grad = False
        del model, core
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
