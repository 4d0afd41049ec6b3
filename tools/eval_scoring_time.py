"""What scoring one evaluation batch costs after the forwards (everything behind crct.evaluation.score_rows), on the GPU, for

  new     question_categories + score_batch: one crct_eval_score launch (selection, flags, the three tables)
  parent  select_answers + correctness + reduce_total_acc + reduce_breakdown_table + reduce_histogram: the crct_eval_select launch
          and the tensor operations of the Python helpers, as plotqa_evaluate ran them before crct_eval_score existed

No model: synthetic row scores for --questions questions (256) with 1 to 120 candidates each and PlotQA categories, the per-question
tensors on the host as a dataloader hands them over.  Each batch is timed with a device-event pair and a synchronise, the two paths
alternating batch by batch (the order swapping every batch); median over --batches (50) after --warmup (10), in a fresh child process
under a time limit.  Both paths' tables are compared on every warm-up batch.  A second child counts the device kernels and copies of
one batch of each path with torch.profiler (a run of its own: tracing slows the host).  One JSON line per result.

    python tools/eval_scoring_time.py > profiles/eval_scoring_time.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cqa-crct_amd"))

QIDS = ["S3", "S17", "D6", "D14", "D2", "A2", "M1", "CD7", "D15", "D16", "C5", "S0"]
FIGS = ["line", "vbar", "hbar", "dot"]


def make_batches(n, questions, dev, seed=0):
    import numpy as np
    import torch
    g = np.random.RandomState(seed)
    out = []
    for bi in range(n):
        Q = questions
        num_ans = g.randint(1, 121, size=Q).astype(np.int64)
        N = int(num_ans.sum())
        needs = g.rand(Q) < 0.5
        rows = dict(scores=torch.from_numpy(g.randn(N, 2).astype(np.float32)).to(dev),
                    out=torch.from_numpy(g.uniform(-50, 50, size=N).astype(np.float32)).to(dev),
                    err=torch.from_numpy(np.abs(g.randn(N) * 0.3).astype(np.float32)).to(dev),
                    terr=torch.from_numpy(np.abs(g.randn(N) * 0.1).astype(np.float32)).to(dev))
        batch = dict(num_ans=torch.from_numpy(num_ans).view(Q, 1), id=torch.arange(bi * Q, (bi + 1) * Q).view(Q, 1),
                     gt_id=torch.from_numpy((g.rand(Q) * num_ans).astype(np.int64)).view(Q, 1), needs_reg=torch.from_numpy(needs).view(Q, 1),
                     tolerance_margin=torch.from_numpy(g.choice([0.01, 0.05, 0.2], size=Q).astype(np.float32)).view(Q, 1),
                     qid=[QIDS[i] for i in g.randint(len(QIDS), size=Q)], qa_type=[FIGS[i] for i in g.randint(4, size=Q)])
        ans_type = {int(i): (2 if nd else int(k)) for i, nd, k in zip(batch["id"].view(-1).tolist(), needs, g.randint(0, 3, size=Q))}
        out.append((rows, batch, ans_type))
    return out


def paths(dev):
    import torch
    from crct import evaluation as EV
    from crct import lib as L
    params = dict(ddp=False)

    def new(rows, batch, ans_type, state):
        cats = EV.question_categories(batch, ans_type.__getitem__)
        EV.score_batch(rows["scores"], rows["out"], rows["err"], rows["terr"], batch, state["tables"], cats=cats, with_histogram=True)

    def parent(rows, batch, ans_type, state):
        answers, so, se, st, _ = EV.select_answers(rows["scores"], rows["out"], rows["err"], rows["terr"], batch["num_ans"], None)
        nsp_right, reg_right, reg_t_right, needs = EV.correctness(answers, se, st, batch)
        EV.reduce_total_acc(state["total"], needs, nsp_right, reg_right, reg_t_right, None)
        correct = nsp_right & (needs.logical_not() | reg_right)
        correct_t = nsp_right & (needs.logical_not() | reg_t_right)
        EV.reduce_breakdown_table(ans_type.__getitem__, None, params, state["breakdown"], batch, correct, correct_t, needs)
        EV.reduce_histogram(state["histogram"], se[needs].view(-1), None)

    def fresh():
        return dict(tables=torch.zeros(L.EVAL_TABLE_WORDS, dtype=torch.int64, device=dev),
                    total=torch.zeros(6, 2, dtype=torch.float64, device=dev), breakdown=torch.zeros(5, 4, 3, 3, dtype=torch.float64, device=dev),
                    histogram=torch.zeros(13, dtype=torch.int64, device=dev))

    def same(state):
        t = state["tables"]
        return (torch.equal(t[:12].double().view(6, 2), state["total"]) and torch.equal(t[12:192].double().view(5, 4, 3, 3), state["breakdown"])
                and torch.equal(t[192:205], state["histogram"]) and int(t[205]) == 0)

    return dict(new=new, parent=parent), fresh, same


def measure(args):
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("eval_scoring_time.py measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    fns, fresh, same = paths(dev)
    pool = make_batches(8, args.questions, dev)
    times = dict(new=[], parent=[])
    state = fresh()
    for i in range(args.warmup + args.batches):
        rows, batch, ans_type = pool[i % len(pool)]
        for name in (("new", "parent") if i % 2 == 0 else ("parent", "new")):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fns[name](rows, batch, ans_type, state)
            e1.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                times[name].append(e0.elapsed_time(e1))
        if i < args.warmup and not same(state):
            raise RuntimeError("the two paths' tables differ on batch %d" % i)
    if not same(state):
        raise RuntimeError("the two paths' tables differ after the timed batches")
    rows_per_batch = [int(b["num_ans"].sum()) for _, b, _ in pool]
    for name in ("new", "parent"):
        t = sorted(times[name])
        print(json.dumps(dict(what="scoring of one batch, " + name + " path", device=torch.cuda.get_device_name(0), questions=args.questions,
                              rows_per_batch=[min(rows_per_batch), max(rows_per_batch)], batches=len(t), warmup=args.warmup,
                              median_ms=round(statistics.median(t), 4), min_ms=round(t[0], 4), p90_ms=round(t[int(0.9 * (len(t) - 1))], 4),
                              max_ms=round(t[-1], 4))), flush=True)
    print(json.dumps(dict(what="parent / new, medians", ratio=round(statistics.median(times["parent"]) / statistics.median(times["new"]), 2),
                          tables_equal=True)), flush=True)


def count(args):
    import torch
    from torch.profiler import ProfilerActivity, profile
    dev = torch.device("cuda:0")
    fns, fresh, _ = paths(dev)
    pool = make_batches(2, args.questions, dev)
    state = fresh()
    for name in ("new", "parent"):
        for rows, batch, ans_type in pool:                 # warm
            fns[name](rows, batch, ans_type, state)
        torch.cuda.synchronize()
        rows, batch, ans_type = pool[0]
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fns[name](rows, batch, ans_type, state)
            torch.cuda.synchronize()
        kernels = copies = 0
        for ev in prof.events():
            if ev.device_type == torch.autograd.DeviceType.CUDA:
                if "memcpy" in ev.name.lower() or "memset" in ev.name.lower():
                    copies += 1
                else:
                    kernels += 1
        print(json.dumps(dict(what="device activities of one batch, " + name + " path", kernels=kernels, copies_and_memsets=copies)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--questions", type=int, default=256)
    ap.add_argument("--batches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds each child process may take")
    ap.add_argument("--child", choices=["measure", "count"])
    args = ap.parse_args()
    if args.child:
        return (measure if args.child == "measure" else count)(args)
    print(json.dumps(dict(command="python tools/eval_scoring_time.py " + " ".join(sys.argv[1:]))), flush=True)
    rc = 0
    for child in ("measure", "count"):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", child, "--questions", str(args.questions), "--batches", str(args.batches),
               "--warmup", str(args.warmup)]
        try:
            r = subprocess.run(cmd, timeout=args.limit)
            if r.returncode != 0:
                print(json.dumps(dict(what=child, error="exit status %d" % r.returncode)), flush=True)
                rc = rc or r.returncode
                break                                      # nothing more on the device after a failed child
        except subprocess.TimeoutExpired:
            print(json.dumps(dict(what=child, error="no result within %.0f s" % args.limit)), flush=True)
            rc = 124
            break
    return rc


if __name__ == "__main__":
    sys.exit(main())
