"""What ``params['img_loss_coeff']`` costs, and what the one-wave-per-row loss kernels buy over the vocabulary kernels.

Part 1 (the step): forward + backward of the training step with the option off and with ``img_loss_coeff = 1`` at the reference's own PlotQA
shape (B 80, V 44, T 124, F_v 1024) or BASELINE configs[1]; ``image_label`` is 1 on ``--mask-prob`` (default 0.15) of the real regions
(never the <IMG> row), drawn once, on the host as the loader leaves it, with their features zeroed; hard targets in ``image_class``.
Resident batch otherwise; dropout on, no optimizer.  The two forms are two models (the option is read at construction) on the same seeded
weights, warmed up, then timed in alternation (--rounds windows of --steps steps each, device events around each window); one JSON line per
form with R (the masked rows), every window's time, the median and the spread (max - min).  The "off" line is the one to hold against the
same run of this file on the parent commit (it knows no such option: ``--off-only`` runs there).

Part 2 (``--kernels``): region_ce_fwd / region_ce_bwd (hard targets) against lm_ce_fwd / lm_ce_bwd -- the path one would otherwise have
used -- on the same fp32 logits at C = 1601 (Cp = 1664) and R = 528 and 3520 rows, each timed as --rounds windows of --launches back-to-back
launches between device events, the pairs in alternation; median, min and max per launch in microseconds and the bytes each must move.
The logits (3.5 MB at R = 528, 23 MB at 3520) stay in the 256 MB last-level cache between launches: these are warm-cache times, as in the
step, where the decoder GEMM has just written them.  A window also holds the host's enqueue cost (the same for both families), which
hides a kernel of a few microseconds: the kernels' own device times come from a run of their own under
``rocprofv3 --kernel-trace --stats -- python tools/img_loss_time.py --kernels --rows 528`` (one row count per run: the statistics are per
kernel name).

    python tools/img_loss_time.py [--workload plotqa-real] [--mask-prob 0.15] [--steps 20] [--warmup 5] [--rounds 5] [--off-only]
    python tools/img_loss_time.py --kernels [--rows 528 3520] [--launches 200] [--rounds 9]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cqa-crct_amd"))

from crct import config as C                       # noqa: E402
from crct import ops                               # noqa: E402
from crct import synthetic as S                    # noqa: E402
from crct.model import VisualDialogEncoder         # noqa: E402
from crct.step_adapter import forward as step_forward   # noqa: E402

SHAPES = {"configs[1]": (80, 36, 20, 2048), "plotqa-real": (80, 44, 124, 1024)}


def window(fn, n):
    """Milliseconds per call of ``fn`` over n back-to-back calls, between device events."""
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n


def summary(ms, scale=1.0, digits=3):
    return dict(median=round(statistics.median(ms) * scale, digits), min=round(min(ms) * scale, digits), max=round(max(ms) * scale, digits),
                spread=round((max(ms) - min(ms)) * scale, digits))


def step_times(args):
    dev = torch.device("cuda:0")
    B, V, T, Fv = SHAPES[args.workload]
    cfg = C.vilbert_config(v_feature_size=Fv)
    host = S.make_batch(B, T, V, Fv, seed=17)
    gen = torch.Generator().manual_seed(5)
    real = host["image_mask"] != 0
    real[:, 0] = False                                # the <IMG> row is never masked
    pick = (torch.rand(B, V, generator=gen) < args.mask_prob) & real
    label = torch.full((B, V), -1, dtype=torch.int64)
    label[:, 0] = 0
    label[pick] = 1
    host["image_feat"][pick] = 0.0
    batch = {k: v.to(dev) for k, v in host.items()}
    batch["image_label"] = label                      # on the host, as the loader leaves it
    batch["image_class"] = torch.randint(0, cfg.v_target_size, (B, V), generator=gen)
    R = int(pick.sum())
    forms = {"off": {}} if args.off_only else {"off": {}, "on": dict(img_loss_coeff=1.0)}
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

    for form in forms:                                # warm up every form, then alternate them: clocks and neighbours drift
        for _ in range(args.warmup):
            step(form)
    ms = {form: [] for form in forms}
    for _ in range(args.rounds):
        for form in forms:
            step(form)
            ms[form].append(window(lambda: step(form), args.steps))
    for form in forms:
        print(json.dumps(dict(shape=args.workload, B=B, V=V, T=T, F_v=Fv, img_loss=form, mask_prob=args.mask_prob, masked_rows=R,
                              classes=cfg.v_target_size, steps=args.steps, rounds=args.rounds, fwd_bwd_ms=[round(v, 3) for v in ms[form]],
                              **{"fwd_bwd_ms_" + k: v for k, v in summary(ms[form]).items()})), flush=True)


def kernel_times(args):
    dev = torch.device("cuda:0")
    Cn = 1601
    Cp = ops.pad64(Cn)
    for R in args.rows:
        Rp = ops.pad64(R)
        gen = torch.Generator().manual_seed(R)
        logits = (torch.randn(Rp, Cp, generator=gen) * 3.0).to(dev)
        labels = torch.randint(0, Cn, (R,), generator=gen).to(torch.int32).to(dev)
        g = torch.ones(1, device=dev)
        _, lse_new, _ = ops.region_ce_fwd(logits, R, Cn, 1.0 / R, labels=labels)
        _, lse_old, _ = ops.lm_ce_fwd(logits, labels, R, Cn, 1.0 / R)
        d_new, d_old = ops.region_ce_bwd(logits, lse_new, g, 1.0 / R, R, Cn, labels=labels), ops.lm_ce_bwd(logits, labels, lse_old, g, 1.0 / R, R, Cn)
        same_dL = bool(torch.equal(d_new.view(torch.int16), d_old.view(torch.int16)))
        lse_diff = float((lse_new - lse_old).abs().max())
        calls = {
            "region_ce_fwd": lambda: ops.region_ce_fwd(logits, R, Cn, 1.0 / R, labels=labels),
            "lm_ce_fwd": lambda: ops.lm_ce_fwd(logits, labels, R, Cn, 1.0 / R),
            "region_ce_bwd": lambda: ops.region_ce_bwd(logits, lse_new, g, 1.0 / R, R, Cn, labels=labels),
            "lm_ce_bwd": lambda: ops.lm_ce_bwd(logits, labels, lse_old, g, 1.0 / R, R, Cn),
        }
        for fn in calls.values():
            for _ in range(20):
                fn()
        ms = {k: [] for k in calls}
        for _ in range(args.rounds):
            for k, fn in calls.items():
                ms[k].append(window(fn, args.launches))
        # what a launch must move: fwd reads the R real rows (+ the mean launch's R floats); bwd reads them and writes bf16 [Rp, Cp]
        need = {"fwd": R * Cn * 4, "bwd": R * Cn * 4 + Rp * Cp * 2}
        for k in calls:
            s = summary(ms[k], 1e3, 2)
            print(json.dumps(dict(kernel=k, C=Cn, Cp=Cp, R=R, Rp=Rp, launches=args.launches, rounds=args.rounds, us_per_call=s,
                                  bytes_needed=need[k[-3:]], gb_per_s_at_median=round(need[k[-3:]] / (s["median"] * 1e-6) / 1e9, 1),
                                  note="each call = the launch(es) plus its output allocations on the host, the same for both families; fwd "
                                       "includes the one-workgroup mean launch", dL_bits_equal_lm=same_dL, lse_max_abs_diff_vs_lm=lse_diff)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(SHAPES), default="plotqa-real")
    ap.add_argument("--mask-prob", type=float, default=0.15)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=None, help="timed windows per form / kernel (default 5 for the step, 9 for --kernels)")
    ap.add_argument("--off-only", action="store_true", help="only the form without the option (any commit runs it)")
    ap.add_argument("--kernels", action="store_true", help="part 2: the loss kernels alone against the vocabulary kernels")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rows", type=int, nargs="+", default=[528, 3520], help="--kernels: the row counts R")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("img_loss_time: needs the GPU; there is no CPU path to time")
    if args.rounds is None:
        args.rounds = 9 if args.kernels else 5
    (kernel_times if args.kernels else step_times)(args)


if __name__ == "__main__":
    main()
