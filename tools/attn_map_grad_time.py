"""What ``core.attention_map_outputs`` costs: the training step (forward + backward + overlapped AdamW + zero_grad, resident batch,
dropout on) with 0 maps, with 1 co-attention map (("conn", 0, 0)) and with all co-attention maps (both directions of every connection
layer) requested AND used in the loss, at BASELINE configs[1] (B 80, V 36, T 20, F_v 2048) and at the reference's own PlotQA shape
(B 80, V 44, T 124, F_v 1024).  A used map adds one attention_probs launch to the forward and the two launches of
crct_attention_probs_bwd to the backward; the figures include the torch kernels of the aux term itself (a product and a sum per map,
and their backward).

Two comparisons, both in alternating windows of at least --window seconds (clocks and neighbours drift, so a pair is the unit):
  * the three forms against each other, in one process per shape;
  * with --parent DIR, the 0-map step of this tree against the step of another checkout of the project (the commit before the feature,
    built): one child process per window, this tree and DIR in alternation, so that the two libraries never share a process.  A 0-map
    step outside the other tree's run-to-run spread is a defect to find, not a number to record.

    python tools/attn_map_grad_time.py [--pairs 3] [--window 2.0] [--parent DIR] > profiles/attn_map_grad_time.txt
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"configs[1]": (80, 36, 20, 2048), "plotqa-real": (80, 44, 124, 1024)}
FORMS = ("0 maps", "1 map", "all co-attention maps")


def build(tree, shape):
    sys.path.insert(0, os.path.join(tree, "cqa-crct_amd"))
    import torch
    from crct import config as C
    from crct import synthetic as S
    from crct.model import VisualDialogEncoder
    from crct.optim import get_optimizer
    from crct.step_adapter import forward as step_forward
    if not torch.cuda.is_available():
        raise RuntimeError("attn_map_grad_time.py measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    B, V, T, Fv = SHAPES[shape]
    cfg = C.vilbert_config(v_feature_size=Fv)
    params = C.default_params(device=dev, quiet_init=True, max_vis_features=V, max_seq_len=T)
    model = VisualDialogEncoder(params, config=cfg)
    core = model.bert_pretrained
    S.seeded_fill_(model.state_dict(), base_seed=7)
    core._invalidate_shadow()
    opt = get_optimizer(params, model)
    opt.overlap = True
    batch = {k: v.to(dev) for k, v in S.make_batch(B, T, V, Fv, seed=17).items()}
    n_conn = len(cfg.v_biattention_id)
    maps = {"0 maps": [], "1 map": [("conn", 0, 0)], "all co-attention maps": [("conn", i, d) for i in range(n_conn) for d in (0, 1)]}
    gen = torch.Generator().manual_seed(3)
    nh = cfg.bi_num_attention_heads
    W = {0: (torch.randn(B, nh, T, V, generator=gen) * 1e-4).to(dev), 1: (torch.randn(B, nh, V, T, generator=gen) * 1e-4).to(dev)}

    def step(form):
        if maps[form] or hasattr(core, "attention_map_outputs"):      # a tree from before the feature has no attribute to clear
            core.attention_map_outputs = maps[form]
        loss = step_forward(model, batch, params)[0]
        for key in maps[form]:
            loss = loss + (W[key[2]] * core.attention_maps[key]).sum()
        loss.backward()
        opt.step()
        opt.zero_grad()

    def window(form, seconds):
        for _ in range(3):
            step(form)
        opt.synchronize()
        torch.cuda.synchronize()
        n, t0 = 0, time.perf_counter()
        while True:
            for _ in range(10):
                step(form)
            n += 10
            opt.synchronize()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if dt >= seconds:
                return dt / n * 1e3
    return step, window, torch.cuda.get_device_name(0), len(maps[FORMS[2]])


def child(tree, shape, seconds, forms):
    """The windows of one process: the checkout at `tree`, one shape; prints one JSON line of step times in ms."""
    step, window, name, n_all = build(tree, shape)
    for form in forms:
        for _ in range(5):
            step(form)
    print(json.dumps(dict(device=name, n_all=n_all, **{form: window(form, seconds) for form in forms})), flush=True)


def spread(v):
    return dict(mean=round(sum(v) / len(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--window", type=float, default=2.0, help="seconds per timed window, at least")
    ap.add_argument("--parent", default=None, help="root of a built checkout of the commit to compare the 0-map step against")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], args.window, args.child[2].split("|"))

    def run(tree, shape, forms):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, shape, "|".join(forms), "--window", str(args.window)],
                             check=True, stdout=subprocess.PIPE, text=True).stdout
        return json.loads(out.strip().splitlines()[-1])
    print(json.dumps(dict(command="python tools/attn_map_grad_time.py " + " ".join(sys.argv[1:]))), flush=True)
    for shape in args.shapes.split(","):
        rows = []
        for pair in range(args.pairs):                  # one process per pair: the forms alternate inside it, the order flips between pairs
            got = run(ROOT, shape, FORMS if pair % 2 == 0 else FORMS[::-1])
            rows.append(got)
            print(json.dumps(dict(shape=shape, pair=pair, device=got["device"], **{"step_ms " + f: round(got[f], 4) for f in FORMS})), flush=True)
        print(json.dumps(dict(what="attention_map_outputs used in the loss, training step", shape=shape, maps_in_all=rows[0]["n_all"],
                              zero_ms=spread([r[FORMS[0]] for r in rows]), one_minus_zero_ms=spread([r[FORMS[1]] - r[FORMS[0]] for r in rows]),
                              all_minus_zero_ms=spread([r[FORMS[2]] - r[FORMS[0]] for r in rows]))), flush=True)
        if args.parent:
            prow = []
            for pair in range(args.pairs):
                order = (ROOT, args.parent) if pair % 2 == 0 else (args.parent, ROOT)
                got = {tree: run(tree, shape, FORMS[:1])[FORMS[0]] for tree in order}
                prow.append((got[ROOT], got[args.parent]))
                print(json.dumps(dict(shape=shape, pair=pair, step_ms_this_tree_0_maps=round(got[ROOT], 4), step_ms_parent=round(got[args.parent], 4),
                                      diff_ms=round(got[ROOT] - got[args.parent], 4))), flush=True)
            print(json.dumps(dict(what="0 maps - parent commit, training step, one process per window", shape=shape,
                                  parent_ms=spread([p for _, p in prow]), this_tree_0_maps_ms=spread([t for t, _ in prow]),
                                  diff_ms=spread([t - p for t, p in prow]))), flush=True)


if __name__ == "__main__":
    main()
