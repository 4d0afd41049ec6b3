"""The bits of the training step, for comparing two checkouts of the project: one SHA-256 per result over its raw bytes.

Each case below runs one training forward + backward at a fixed seed and call number, dropout on, on cleared gradients, and prints a
line per item: the flat gradient buffer, the step outputs [stats | reg | logits] as the forward and as the backward left them, every
requested input gradient, ``text_embedding_grad``, both sequence outputs and every requested attention map.  Run it in two trees and
diff the outputs: a host-side refactor of the step engine must leave every line as it was.

    python tools/step_bits.py [--tree DIR] [--cases a,b]        (DIR: root of a built checkout, default this one)

Three tensors of the flat gradient buffer -- the position, type and colour embedding tables -- are the ones tests/helpers.py lists
(ATOMIC_GRADS) as free to differ in their last bits between two runs of ONE tree, and the suite's bit-for-bit tests compare them to
rounding only.  Their ranges are cleared before the buffer is hashed; every other gradient has one fixed summation order.

Cases: tiny PlotQA plain / with every request at once / the same with key masks that mask keys out in both streams (a swapped mask in the
co-attention shows here) / tiny FigureQA with areas and one map / long attention (T 113, the shortest length served by
attention_long.hip, whose row statistics the maps' attention sites carry) / the fp8 step (e4m3 context copies, e5m2 dqkv copies).
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOMIC_GRADS = ("bert.embeddings.position_embeddings.weight", "bert.embeddings.plotqa_type_embeddings.weight",
                "bert.v_embeddings.color_emb.weight")
ALL_MAPS = [("text", 1), ("visual", 0), ("conn", 0, 0), ("conn", 0, 1)]


def sha(t):
    import torch
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--cases", default="plain,all,masks,figureqa,long,fp8")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.tree, "cqa-crct_amd"))
    import numpy as np
    import torch
    from crct import config as C
    from crct import synthetic as S
    from crct.model import VisualDialogEncoder
    from crct.step_adapter import forward as step_forward
    if not torch.cuda.is_available():
        raise RuntimeError("step_bits.py runs the step on the GPU; there is none")
    dev = torch.device("cuda:0")

    def build(cfg, params, seed, cls_dropout):
        params = dict(params, device=dev, quiet_init=True)
        model = VisualDialogEncoder(params, config=cfg)
        core = model.bert_pretrained
        core.cls_dropout = cls_dropout
        S.seeded_fill_(model.state_dict(), base_seed=seed)
        core._invalidate_shadow()
        model.train()
        return model, params, core

    def tiny(B=3, T=9, V=5, lengths=None, n_vis=None, **over):
        p = 0.1
        cfg = C.tiny_config(hidden_dropout_prob=p, attention_probs_dropout_prob=p, v_hidden_dropout_prob=p, v_attention_probs_dropout_prob=p, **over)
        model, params, core = build(cfg, C.default_params(categories=9, L1=True), 7, p)
        batch = S.make_batch(B, T, V, cfg.v_feature_size, categories=9, vocab_size=cfg.vocab_size, seed=11, lengths=lengths, n_vis=n_vis)
        return model, params, core, batch

    def step(case, model, params, core, batch, it=1, inputs=(), keep_emb=False, seq=False, scores=False, maps=()):
        """One forward + backward at call number `it` on cleared gradients, with a fixed loss term on every requested output."""
        b = dict(batch)
        for n in inputs:
            b[n] = batch[n].detach().clone().requires_grad_(True)
        core.zero_flat_grads()
        core._calls = it - 1
        core.keep_text_embedding_grad = keep_emb
        core.return_sequence_outputs = seq
        core.differentiable_scores = scores
        if maps or hasattr(core, "attention_map_outputs"):
            core.attention_map_outputs = list(maps)
        out = step_forward(model, b, params)
        torch.cuda.synchronize()
        items = [("outputs after forward", core._engine.out.clone())]
        gen = torch.Generator().manual_seed(1000 + it)

        def term(t, scale):          # a fixed cotangent: the gradient of the term with respect to t is W itself
            return ((torch.randn(t.shape, generator=gen) * scale).to(dev) * t).sum()
        loss = out[0]
        keys = [(tuple(k) + (0,))[:3] for k in maps]
        if seq:
            loss = loss + term(core.sequence_output_t, 1e-3) + term(core.sequence_output_v, 1e-3)
        if scores:
            loss = loss + term(out[4], 1e-2) + term(out[5][0], 1e-2)
        for k in keys:
            loss = loss + term(core.attention_maps[k], 1e-2)
        loss.backward()
        torch.cuda.synchronize()
        g = core.flat_grads.clone()
        for e in core.table:
            if e.name in ATOMIC_GRADS:
                g[e.offset:e.offset + e.numel] = 0
        items += [("flat gradients (atomic tables cleared)", g), ("outputs after backward", core._engine.out)]
        items += [("grad of " + n, b[n].grad) for n in inputs]
        if keep_emb:
            items.append(("text_embedding_grad", core.text_embedding_grad))
        if seq:
            items += [("sequence_output_t", core.sequence_output_t), ("sequence_output_v", core.sequence_output_v)]
        items += [("map %s %d %d" % k, core.attention_maps[k]) for k in keys]
        for name, t in items:
            print("%-10s %-40s %s %s" % (case, name, "x".join(str(s) for s in t.shape), sha(t)), flush=True)

    everything = dict(inputs=("image_feat", "image_loc", "loc"), keep_emb=True, seq=True, scores=True, maps=ALL_MAPS)
    for case in args.cases.split(","):
        if case == "plain":
            step(case, *tiny())
        elif case == "all":
            step(case, *tiny(), **everything)
        elif case == "masks":
            model, params, core, batch = tiny(lengths=[9, 6, 4], n_vis=[5, 3, 2])
            assert int((batch["image_mask"] == 0).sum()) >= 1
            step(case, model, params, core, batch, **everything)
        elif case == "figureqa":
            z = np.load(os.path.join(args.tree, "tests", "golden", "variant_tiny_figureqa.npz"), allow_pickle=False)
            meta = json.loads(str(z["meta"]))
            cfg = C.BertConfig.from_dict(meta["cfg"])
            batch = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in.")}
            Bv, Vv = batch["image_target"].shape
            gen = torch.Generator().manual_seed(int(meta["feat_seed"]))      # the fixture does not store the features: the variant never reads them
            batch["image_feat"] = torch.randn(Bv, Vv, cfg.v_feature_size, generator=gen, dtype=torch.float32).half().float()
            model, params, core = build(cfg, dict(meta["params"]), meta["weight_seed"], 0.0)
            step(case, model, params, core, batch, inputs=("areas",), maps=[("conn", len(cfg.v_biattention_id) - 1, 0)])
        elif case == "long":
            # beyond 112 keys the attention kernels need a head size of 32, 48, 64 or 128: the tiny config widened as the smoke run's
            # (head sizes 32 / 48 / 32), and with room for 113 positions
            wide = dict(hidden_size=128, num_attention_heads=4, intermediate_size=256, max_position_embeddings=160, v_hidden_size=192,
                        v_num_attention_heads=4, v_intermediate_size=192, bi_hidden_size=128, bi_num_attention_heads=4)
            step(case, *tiny(B=2, T=113, V=5, **wide), maps=[("text", 0), ("conn", 0, 1)])
        elif case == "fp8":
            # the fp8 step tests' smallest shape (tests/test_step_gpu.py: full widths, B 3, T 31, V 7); no maps: refused with fp8 data gradients.
            # The first backward pass calibrates the gradient scales (its GEMMs run in bf16), the second reads the e5m2 copies.
            p = 0.1
            cfg = C.vilbert_config(v_feature_size=2048, hidden_dropout_prob=p, attention_probs_dropout_prob=p, v_hidden_dropout_prob=p,
                                   v_attention_probs_dropout_prob=p)
            model, params, core = build(cfg, C.default_params(fp8=True, fp8_backward=True, fp8_wgrad=True), 11, p)
            assert core.fp8 and core.fp8_backward and core.fp8_wgrad
            batch = S.make_batch(3, 31, 7, 2048, seed=103)
            for it in (1, 2):
                step("fp8 pass %d" % it, model, params, core, batch, it=it)
        else:
            raise SystemExit("unknown case %r" % case)


if __name__ == "__main__":
    main()
