"""Step time (forward + backward + fused AdamW, overlap mode, dropout on) with ``fixed_t_layer`` 0 and 6, at BASELINE configs[1]
(B 80, V 36, T 20, 2048-d features) and at the plotqa-real shape (B 80, V 44, T 124, 1024-d).  ONE model and optimizer per shape;
the field is switched between timed windows, so the two settings alternate in one process on the same weights and batch
(pairs: 0, 6, 0, 6, ...).  One JSON line per window, then one summary line per shape with every pair's difference and the spread
of each setting over its windows.

    python tools/frozen_step_time.py [--pairs 5] [--window 100] [--warmup 10] [--levels 0,6] [--package DIR]

``--levels 0`` times the unfrozen step alone (every window the same setting: its run-to-run spread); ``--package DIR`` imports the
``crct`` package from ``DIR`` instead of this tree's, to time another build of the library with the same script.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"configs[1]": (80, 36, 20, 2048), "plotqa-real": (80, 44, 124, 1024)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--window", type=int, default=100, help="steps per timed window")
    ap.add_argument("--warmup", type=int, default=10, help="untimed steps per setting before the first window")
    ap.add_argument("--levels", default="0,6")
    ap.add_argument("--package", default=os.path.join(ROOT, "cqa-crct_amd"))
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    sys.path.insert(0, args.package)
    from crct import config as C
    from crct import synthetic as S
    from crct.model import VisualDialogEncoder
    from crct.optim import get_optimizer
    from crct.step_adapter import forward as step_forward

    levels = [int(x) for x in args.levels.split(",")]
    dev = torch.device("cuda:0")
    for name in args.shapes.split(","):
        B, V, T, F = SHAPES[name]
        cfg = C.vilbert_config(v_feature_size=F)
        params = C.default_params(device=dev, quiet_init=True, max_vis_features=V, max_seq_len=T)
        model = VisualDialogEncoder(params, config=cfg)
        S.seeded_fill_(model.state_dict(), base_seed=7)
        model.bert_pretrained._invalidate_shadow()
        opt = get_optimizer(params, model)
        opt.overlap = True
        batch = {k: v.to(dev) for k, v in S.make_batch(B, T, V, F, seed=17).items()}

        def window(level, steps):
            if cfg.fixed_t_layer != level:
                cfg.fixed_t_layer = level
                cfg.validate()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            for _ in range(steps):
                step_forward(model, batch, params)[0].backward()
                opt.step()
                opt.zero_grad()
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1) / steps

        for lv in levels:
            window(lv, args.warmup)
        times = {lv: [] for lv in levels}
        for pair in range(args.pairs):
            for lv in levels:
                ms = window(lv, args.window)
                times[lv].append(ms)
                print(json.dumps(dict(label=args.label, shape=name, B=B, V=V, T=T, pair=pair, fixed_t_layer=lv, steps=args.window,
                                      step_ms=round(ms, 4))), flush=True)
        summary = dict(label=args.label, shape=name, summary=True)
        for lv in levels:
            t = times[lv]
            summary["fixed_t_layer=%d" % lv] = dict(min_ms=round(min(t), 4), max_ms=round(max(t), 4), mean_ms=round(sum(t) / len(t), 4),
                                                    spread_ms=round(max(t) - min(t), 4))
        if len(levels) == 2:
            a, b = levels
            diffs = [x - y for x, y in zip(times[a], times[b])]
            summary["saved_ms_per_pair"] = [round(d, 4) for d in diffs]
            summary["faster_on_every_pair"] = all(d > 0 for d in diffs)
        print(json.dumps(summary), flush=True)
        del model, opt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
