"""Generate the head-size-128 fixtures by RUNNING THE REFERENCE (build container only, on the CPU).

Same import shims, model construction and recording as ``make_golden.py`` (``run_case`` with ``save_weights=False, yardstick=True``:
inputs, outputs, activations at the heads, every gradient's norm and a 64-element sample, the bf16-autocast yardstick's norm ratios;
name-keyed seeded weights, none committed).  Two cases:

    head128_small_B3_V9_T130          ``small_long_config()`` with 2 text heads on 128 (head size 64) and 2 visual / co-attention heads on
                                      256 (head size 128); the batch of ``small_B3_V9_T130`` (lengths 130 / 97 / 113, 9 / 4 / 7 elements)
    head128_full_B4_V36_T20_F2048     ``vilbert_original_config`` (12 x 64, 8 x 128, 8 x 128) with all dropouts 0; the batch of
                                      ``full_B4_V36_T20_F2048`` (seed 1234, features rounded to fp16)

To keep every committed file below 1 MiB the written .npz is then slimmed (``slim``): ``out.emb_t`` / ``out.emb_v`` (the embeddings do not
depend on the head size; the existing fixtures pin them) are dropped; ``in.image_feat`` is stored as fp16 where its values are
fp16-representable (the full case; tests cast it back: lossless); the per-tensor scalars ``gradnorm.<name>`` / ``yardratio.<name>`` become
two arrays ``gradnorms`` / ``yardratios`` (NaN: none) in the order of the JSON list ``gradnames`` (a zip entry per scalar costs 250 bytes),
with ``yardcosines`` beside them: the yardstick's per-tensor gradient cosine against its fp32 self (``yardstick_cosines``);
``gradidx.<name>`` is dropped after checking that it is ``sample_index`` of the tensor's size -- ``gradsample.<name>`` stays as it is.

    python tests/golden/make_golden_head128.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G          # noqa: E402  (sets up sys.path for crct / oracle)
from crct import config as C     # noqa: E402
from crct import synthetic as S  # noqa: E402

SMALL = "head128_small_B3_V9_T130"
FULL = "head128_full_B4_V36_T20_F2048"


def small_head128_config():
    cfg = G.small_long_config()
    for k, v in dict(num_attention_heads=2, v_hidden_size=256, v_num_attention_heads=2, v_intermediate_size=256, bi_hidden_size=256,
                     bi_num_attention_heads=2).items():
        setattr(cfg, k, v)
    cfg.validate()
    return cfg


def sample_index(numel):
    """The positions of a tensor's committed gradient sample (run_case's rule): min(numel, 64) evenly spaced elements of the flat tensor."""
    n = min(numel, 64)
    return (torch.arange(n, dtype=torch.int64) * (numel - 1)) // max(n - 1, 1)


def yardstick_cosines(model, cfg, params, batch):
    """Per tensor the cosine between the oracle's gradient under torch's CPU bf16 autocast (run_case's yardstick) and its fp32 self, on the
    weights of the reference model run_case returned -- run_case records only the yardstick's norm ratios."""
    params = dict(params, device=torch.device("cpu"))
    out = {}
    grads = []
    for autocast in (False, True):
        sd = {k[len("bert_pretrained."):]: v.detach().clone().requires_grad_(True) for k, v in model.named_parameters()}
        if autocast:
            with torch.autocast("cpu", dtype=torch.bfloat16):
                o = G.O.oracle_step(sd, cfg, params, batch, training=True, cls_dropout=0.0)
        else:
            o = G.O.oracle_step(sd, cfg, params, batch, training=True, cls_dropout=0.0)
        o[0].float().backward()
        grads.append({k: v.grad for k, v in sd.items()})
    for k, g in grads[0].items():
        if g is None or grads[1][k] is None or float(g.norm()) < 1e-7:
            continue
        a, b = grads[1][k].double().flatten(), g.double().flatten()
        out[k] = float((a @ b) / (a.norm() * b.norm() + 1e-300))
    return out


def slim(name, yardcos):
    path = os.path.join(HERE, name + ".npz")
    z = np.load(path)
    names = [k[len("gradnorm."):] for k in z.files if k.startswith("gradnorm.")]
    rec = {k: z[k] for k in z.files if k not in ("out.emb_t", "out.emb_v") and not k.startswith(("gradnorm.", "gradidx.", "yardratio."))}
    for k in names:
        if "gradidx." + k in z.files:
            assert np.array_equal(z["gradidx." + k], sample_index(int(z["gradidx." + k][-1]) + 1).numpy()), k
    rec["gradnames"] = np.array(json.dumps(names))
    rec["gradnorms"] = np.array([float(z["gradnorm." + k]) for k in names], dtype=np.float64)
    rec["yardratios"] = np.array([float(z["yardratio." + k]) if "yardratio." + k in z.files else np.nan for k in names], dtype=np.float64)
    rec["yardcosines"] = np.array([yardcos.get(k, np.nan) for k in names], dtype=np.float64)
    ys = sorted(yardcos.values())
    print("  [%s] bf16-autocast yardstick: gradient cosine min %.4f, median %.4f" % (name, ys[0], ys[len(ys) // 2]))
    feat = rec["in.image_feat"]
    if np.array_equal(feat.astype(np.float16).astype(np.float32), feat):
        rec["in.image_feat"] = feat.astype(np.float16)
    np.savez_compressed(path, **rec)
    size = os.path.getsize(path)
    print("  slimmed %s: %.1f KB" % (path, size / 1024))
    assert size < (1 << 20)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    vilbert, ed = G.import_reference()
    small = small_head128_config()
    assert (small.hidden_size // small.num_attention_heads, small.v_hidden_size // small.v_num_attention_heads,
            small.bi_hidden_size // small.bi_num_attention_heads) == (64, 128, 128)
    b = S.make_batch(3, 130, 9, small.v_feature_size, categories=9, vocab_size=small.vocab_size, seed=21, lengths=[130, 97, 113], n_vis=[9, 4, 7])
    b["R"][0, 1] = 1.0
    b["R"][1, 1] = 0.0
    b["R"][2, 1] = 1.0
    b["needs_reg"] = (b["R"][:, 1:2] == 1)
    model = G.run_case(SMALL, small, C.default_params(categories=9), b, vilbert, ed, save_weights=False, yardstick=True)
    slim(SMALL, yardstick_cosines(model, small, C.default_params(categories=9), b))
    cfg = C.vilbert_original_config(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, v_hidden_dropout_prob=0.0,
                                    v_attention_probs_dropout_prob=0.0)
    batch = S.make_batch(4, 20, 36, 2048, seed=1234)
    batch["image_feat"] = batch["image_feat"].half().float()
    model = G.run_case(FULL, cfg, C.default_params(), batch, vilbert, ed, save_weights=False, yardstick=True)
    slim(FULL, yardstick_cosines(model, cfg, C.default_params(), batch))


if __name__ == "__main__":
    main()
