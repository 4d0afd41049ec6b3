"""What FusedAdamW.clip_grad_norm_ costs at BASELINE configs[1] (vilbert.json, B 80, V 36 x 2048-d, T 20): three measurements in
one process on the GPU, one JSON line each.

  (a) the sum-of-squares pass alone (crct_grad_sumsq), device events around --reps launches after warm-up, fp32 and bf16 source,
      as GB/s of the bytes it reads (4 or 2 B per gradient element) -- beside the full crct_adamw_step launch timed the same way
      in the same process (30 B per parameter: the project's own yardstick for streaming these buffers);
  (b) the finalize launch alone (crct_grad_norm_finalize, per-tensor norms included);
  (c) the training step (forward + backward + overlapped AdamW + zero_grad) with and without clip_grad_norm_ in deferred mode
      and a max_norm that never clips: --pairs alternating pairs of windows of at least --window seconds each, mean difference
      and spread over the pairs.

    python tools/clip_norm_cost.py [--reps 100] [--pairs 5] [--window 2.0] > profiles/clip_grad_norm_cost.txt
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cqa-crct_amd"))

from crct import config as C                       # noqa: E402
from crct import ops                               # noqa: E402
from crct import synthetic as S                    # noqa: E402
from crct.model import VisualDialogEncoder         # noqa: E402
from crct.optim import get_optimizer               # noqa: E402
from crct.step_adapter import forward as step_forward   # noqa: E402


def timed(fn, reps, warmup=10):
    """Mean milliseconds per call of ``fn`` over ``reps`` back-to-back calls, device events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--window", type=float, default=2.0, help="seconds per timed window of (c), at least")
    ap.add_argument("--batch", type=int, default=80)
    args = ap.parse_args()
    if args.reps < 50:
        ap.error("--reps must be at least 50")
    if not torch.cuda.is_available():
        raise RuntimeError("clip_norm_cost.py measures on the GPU; there is none")
    print(json.dumps(dict(command="python tools/clip_norm_cost.py " + " ".join(sys.argv[1:]), device=torch.cuda.get_device_name(0))), flush=True)
    dev = torch.device("cuda:0")
    cfg = C.vilbert_config(v_feature_size=2048)
    params = C.default_params(device=dev, quiet_init=True)
    model = VisualDialogEncoder(params, config=cfg)
    core = model.bert_pretrained
    S.seeded_fill_(model.state_dict(), base_seed=7)
    core._invalidate_shadow()
    opt = get_optimizer(params, model)
    opt.overlap = True
    batch = {k: v.to(dev) for k, v in S.make_batch(args.batch, 20, 36, 2048, seed=17).items()}

    def step(clip):
        step_forward(model, batch, params)[0].backward()
        if clip:
            opt.clip_grad_norm_(1e30)
        opt.step()
        opt.zero_grad()

    for _ in range(5):
        step(False)
        step(True)
    opt.synchronize()
    torch.cuda.synchronize()

    # ---- (a), (b): the launches alone, on the gradients of a real backward pass
    step_forward(model, batch, params)[0].backward()
    torch.cuda.synchronize()
    elems = int(sum(e.numel for e in opt._segs))
    n_blk = int(opt._blk_seg.numel())
    tables = (opt._seg_off, opt._seg_len, opt._blk_seg, opt._blk_off)
    g32 = core.flat_grads
    g16 = g32.to(torch.bfloat16)
    partials = torch.empty(n_blk, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    ms_adamw = timed(lambda: opt._launch(0, n_blk, None, stream), args.reps)
    rate_adamw = 30.0 * elems / (ms_adamw * 1e-3) / 1e9
    print(json.dumps(dict(what="crct_adamw_step alone (yardstick)", elements=elems, chunks=n_blk, ms=round(ms_adamw, 4), bytes_per_element=30,
                          GBps=round(rate_adamw, 1))), flush=True)
    for name, g, width in (("fp32", g32, 4), ("bf16", g16, 2)):
        for kind in (0, 1):
            ms = timed(lambda: ops.grad_sumsq(g, *tables, partials=partials, norm_kind=kind), args.reps)
            rate = width * elems / (ms * 1e-3) / 1e9
            print(json.dumps(dict(what="(a) crct_grad_sumsq alone", source=name, norm_kind=kind, ms=round(ms, 4), bytes_per_element=width,
                                  GBps=round(rate, 1), share_of_adamw_rate=round(rate / rate_adamw, 3))), flush=True)
    ops.grad_sumsq(g32, *tables, partials=partials)
    ms = timed(lambda: ops.grad_norm_finalize(partials, opt._blk_seg, len(opt._segs), 1.0), args.reps)
    print(json.dumps(dict(what="(b) crct_grad_norm_finalize alone", chunks=n_blk, tensors=len(opt._segs), ms=round(ms, 4))), flush=True)
    one = torch.ones(1, device=dev)
    ms = timed(lambda: ops.scale_runs(g32, one, *tables), args.reps)
    print(json.dumps(dict(what="crct_scale_runs alone, coefficient 1 (no traffic)", ms=round(ms, 4))), flush=True)
    opt.zero_grad()

    # ---- (c): the training step with and without the clip call, alternating windows
    def window(clip):
        for _ in range(3):
            step(clip)
        opt.synchronize()
        torch.cuda.synchronize()
        n, t0 = 0, time.perf_counter()
        while True:
            for _ in range(20):
                step(clip)
            n += 20
            opt.synchronize()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if dt >= args.window:
                return dt / n * 1e3

    diffs, rows = [], []
    for pair in range(args.pairs):
        order = (False, True) if pair % 2 == 0 else (True, False)
        got = {clip: window(clip) for clip in order}
        diffs.append(got[True] - got[False])
        rows.append(dict(pair=pair, step_ms_without=round(got[False], 4), step_ms_with=round(got[True], 4), diff_ms=round(diffs[-1], 4)))
        print(json.dumps(rows[-1]), flush=True)
    mean = sum(diffs) / len(diffs)
    print(json.dumps(dict(what="(c) step with - without clip_grad_norm_ (deferred, never clipping)", pairs=args.pairs, window_s=args.window,
                          mean_diff_ms=round(mean, 4), min_diff_ms=round(min(diffs), 4), max_diff_ms=round(max(diffs), 4),
                          mean_step_ms_without=round(sum(r["step_ms_without"] for r in rows) / len(rows), 4))), flush=True)


if __name__ == "__main__":
    main()
