"""What the weight average in the AdamW launch costs a training step: ``FusedAdamW.enable_ema()`` adds 4 B read + 4 B written per
parameter to the update's 30 B (the bytes predict 38 / 30 of the AdamW launch, most of it hidden beside the next forward), and with the
average off nothing may change at all.  The step is bench.py's: forward + backward + overlapped FusedAdamW.step() + zero_grad() on
resident batches, at BASELINE configs[1] (B 80, V 36, T 20, F_v 2048) and at the reference's own PlotQA shape (B 80, V 44, T 124,
F_v 1024).

Method (one box, one call): every process times windows of ``--steps`` steps in alternation -- average off, average on, off, on, ... --
so that clock and neighbour drift hits both forms alike; a PAIR is one off window and the on window right behind it.  With
``--parent-lib`` (a libcrct_hip.so built from the parent commit) processes of this build and of the parent build alternate as well, the
parent's timing ``off`` windows only: the claim to confirm is that off equals the parent within the spread of the pairs.  The process
that starts the others never touches the GPU; every timing process is a fresh one.

    python tools/ema_step_time.py [--steps 100] [--pairs 4] [--rounds 3] [--parent-lib PATH] [--shapes configs[1],plotqa-real]

One JSON line per process and shape, then a summary per shape: the median and the range of the windows of each form, the on - off
difference pair by pair, and (with --parent-lib) this build's off against the parent's."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cqa-crct_amd"))

SHAPES = {"configs[1]": (80, 36, 20, 2048), "plotqa-real": (80, 44, 124, 1024)}


def worker(args):
    """One timing process: the windows of one build on one shape.  Prints one JSON line."""
    import torch                                   # first: torch must load ITS HIP runtime before any other library brings one
    from crct import lib as L
    if args.lib:                                   # another build of the library (the parent commit's): bind what it exports
        L.LIB_PATH = os.path.abspath(args.lib)
        raw = ctypes.CDLL(L.LIB_PATH)
        for name in [n for n in L.PROTOTYPES if not hasattr(raw, n)]:
            del L.PROTOTYPES[name]
    from crct import config as C
    from crct import synthetic as S
    from crct.model import VisualDialogEncoder
    from crct.optim import get_optimizer
    from crct.step_adapter import forward as step_forward

    dev = torch.device("cuda:0")
    B, V, T, Fv = SHAPES[args.shape]
    cfg = C.vilbert_config(v_feature_size=Fv)
    params = C.default_params(device=dev, quiet_init=True, max_vis_features=V, max_seq_len=T, batch_size=B)
    model = VisualDialogEncoder(params, config=cfg)
    core = model.bert_pretrained
    S.seeded_fill_(model.state_dict(), base_seed=7)
    core._invalidate_shadow()
    model.train()
    opt = get_optimizer(params, model)
    opt.overlap = True
    pool = [{k: v.to(dev) for k, v in S.make_batch(B, T, V, Fv, seed=1234 + 97 * i).items()} for i in range(4)]
    forms = args.forms.split(",")
    count = [0]

    def step():
        batch = pool[count[0] % len(pool)]
        count[0] += 1
        step_forward(model, batch, params)[0].backward()
        opt.step()
        opt.zero_grad()

    def set_form(form):
        opt.synchronize()
        torch.cuda.synchronize()
        if form == "on" and not opt.ema_enabled:
            opt.enable_ema(0.999)
        elif form == "off" and getattr(opt, "ema_enabled", False):
            opt.disable_ema()

    def timed(n):
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(n):
            step()
        opt.synchronize()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / n

    for form in forms:                             # warm up every form, then alternate them
        set_form(form)
        for _ in range(args.warmup):
            step()
    ms = {form: [] for form in forms}
    for _ in range(args.pairs):
        for form in forms:
            set_form(form)
            step()
            ms[form].append(round(timed(args.steps), 4))
    print(json.dumps(dict(shape=args.shape, B=B, V=V, T=T, F_v=Fv, build=args.label, steps=args.steps, step_ms=ms)), flush=True)


def describe(v):
    return "median %.3f  min %.3f  max %.3f  (n %d)" % (statistics.median(v), min(v), max(v), len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100, help="steps per window")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=4, help="off / on window pairs per process")
    ap.add_argument("--rounds", type=int, default=3, help="processes per build and shape")
    ap.add_argument("--shapes", default="configs[1],plotqa-real")
    ap.add_argument("--parent-lib", default=None, help="libcrct_hip.so of the parent commit: timed with the average off, in alternation with this build")
    ap.add_argument("--limit-s", type=float, default=240.0, help="time limit of one timing process")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--shape", default="configs[1]", help=argparse.SUPPRESS)
    ap.add_argument("--forms", default="off,on", help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--label", default="this", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    results = []
    for shape in args.shapes.split(","):
        for _ in range(args.rounds):
            builds = [("this", None, "off,on")] + ([("parent", args.parent_lib, "off")] if args.parent_lib else [])
            for label, lib, forms in builds:
                argv = [sys.executable, os.path.abspath(__file__), "--worker", "--shape", shape, "--forms", forms, "--label", label,
                        "--steps", str(args.steps), "--warmup", str(args.warmup), "--pairs", str(args.pairs if label == "this" else 2 * args.pairs)]
                if lib:
                    argv += ["--lib", lib]
                out = subprocess.run(argv, stdout=subprocess.PIPE, timeout=args.limit_s, check=True).stdout.decode()      # a failing process ends the run
                line = [ln for ln in out.splitlines() if ln.startswith("{")][-1]
                print(line, flush=True)
                results.append(json.loads(line))
    for shape in args.shapes.split(","):
        mine = [r for r in results if r["shape"] == shape and r["build"] == "this"]
        off = [v for r in mine for v in r["step_ms"]["off"]]
        on = [v for r in mine for v in r["step_ms"]["on"]]
        diff = [b - a for a, b in zip(off, on)]
        print("%s, step ms over %d-step windows" % (shape, args.steps))
        print("  average off : " + describe(off))
        print("  average on  : " + describe(on))
        print("  on - off, pair by pair : " + describe(diff))
        print("  spread of the off windows of this build (max - min): %.3f ms" % (max(off) - min(off)))
        parent = [v for r in results if r["shape"] == shape and r["build"] == "parent" for v in r["step_ms"]["off"]]
        if parent:
            print("  parent build: " + describe(parent))
            print("  off - parent (medians): %+.3f ms" % (statistics.median(off) - statistics.median(parent)))


if __name__ == "__main__":
    main()
