"""Time the attention-map kernel (csrc/attention_probs.hip) at the shapes of the reference's PlotQA training batch (config/plotqa.json:
B 80, T 124, V 44; heads and head sizes of config/vilbert.json) and print microseconds and achieved write GB/s per shape next to the byte
count B * heads * Tq * Tk * 4.  Meant to run under the kernel tracer, in a process of its own:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/attention_probs_time.py [--reps 50]

The per-shape figures printed here come from HIP events around `reps` back-to-back launches (the tracer's table has one row per kernel
instantiation, and two of the shapes share one).  --flag-off runs, instead, one evaluation forward of the tiny model WITHOUT
output_all_attention_masks: its kernel list in the tracer's table is the parent commit's (no attn_probs_kernel in it)."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cqa-crct_amd"))

from crct import config as C      # noqa: E402
from crct import ops              # noqa: E402


def shapes(cfg, B, T, V):
    d_t, d_v, d_b = (cfg.hidden_size // cfg.num_attention_heads, cfg.v_hidden_size // cfg.v_num_attention_heads,
                     cfg.bi_hidden_size // cfg.bi_num_attention_heads)
    return [("text self", B, cfg.num_attention_heads, T, T, d_t), ("visual self", B, cfg.v_num_attention_heads, V, V, d_v),
            ("co-attention 1 (text over visual)", B, cfg.bi_num_attention_heads, T, V, d_b),
            ("co-attention 2 (visual over text)", B, cfg.bi_num_attention_heads, V, T, d_b)]


def time_shape(name, B, heads, Tq, Tk, d, reps, p):
    dev = "cuda"
    H = heads * d
    g = torch.Generator().manual_seed(Tq * 1000 + Tk)
    bufq = torch.randn(B, Tq, 3 * H, generator=g).to(torch.bfloat16).to(dev)       # the engine's fused qkv buffers
    bufk = torch.randn(B, Tk, 3 * H, generator=g).to(torch.bfloat16).to(dev)
    km = torch.ones(B, Tk, dtype=torch.uint8)
    for b in range(B):
        km[b, Tk - (b % 7):] = 0 if b % 7 else 1
    km = km.to(dev)
    q, k = bufq[:, :, :H], bufk[:, :, H:2 * H]
    out = torch.empty(B, heads, Tq, Tk, device=dev)
    for _ in range(3):
        ops.attention_probs(q, k, km, heads, d, p_drop=p, site=3, seed=5, out=out)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        ops.attention_probs(q, k, km, heads, d, p_drop=p, site=3, seed=5, out=out)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / reps
    nbytes = B * heads * Tq * Tk * 4
    dev_sum = float((out.double().sum(-1) - 1.0).abs().max()) if p == 0 else float("nan")
    print("%-36s B %3d heads %2d %3d x %3d d %2d p %.1f  %8.1f us  %7.2f MB written  %7.0f GB/s  (max |row sum - 1| %.1e)" % (
        name, B, heads, Tq, Tk, d, p, us, nbytes / 1e6, nbytes / us / 1e3, dev_sum))


def flag_off_forward():
    from crct import synthetic as S
    from crct.model import SequenceMask, VisualDialogEncoder
    dev = torch.device("cuda:0")
    cfg = C.tiny_config()
    params = C.default_params(categories=9, device=dev)
    model = VisualDialogEncoder(params, config=cfg)
    S.seeded_fill_(model.state_dict(), base_seed=7)
    model.bert_pretrained._invalidate_shadow()
    model.eval()
    b = S.make_batch(4, 9, 6, cfg.v_feature_size, categories=9, vocab_size=cfg.vocab_size, seed=5)
    with torch.no_grad():
        out = model.bert_pretrained(b["tokens"], b["loc"], b["image_feat"], b["image_loc"], token_type_ids=b["segments"],
                                    attention_mask=SequenceMask(b["sep_indices"], b["hist_len"], b["tokens"].shape[1]),
                                    image_attention_mask=b["image_mask"], image_target=b["image_target"], gt_reg=[b["R"], "L1"])
    torch.cuda.synchronize()
    assert out[4] is None
    print("evaluation forward without output_all_attention_masks: slot 4 is None")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=80)
    ap.add_argument("--tokens", type=int, default=124)
    ap.add_argument("--vis", type=int, default=44)
    ap.add_argument("--flag-off", action="store_true")
    ap.add_argument("--lib", default=None, help="another build of libcrct_hip.so to time (A/B of kernel variants)")
    a = ap.parse_args()
    if a.lib:
        from crct import lib as L
        L.LIB_PATH = os.path.abspath(a.lib)
        print("library: %s" % L.LIB_PATH)
    if a.flag_off:
        return flag_off_forward()
    cfg = C.vilbert_config()
    for p in (0.0, 0.1):
        for s in shapes(cfg, a.batch, a.tokens, a.vis):
            time_shape(*s, reps=a.reps, p=p)


if __name__ == "__main__":
    main()
