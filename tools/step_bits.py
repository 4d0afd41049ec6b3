"""The bits of the training step, for comparing two checkouts of the project: one SHA-256 per result over its raw bytes.

Each case below runs one training forward + backward at a fixed seed and call number, dropout on, on cleared gradients, and prints a
line per item: the flat gradient buffer, the step outputs [stats | reg | logits] as the forward and as the backward left them, every
requested input gradient, ``text_embedding_grad``, both sequence outputs and every requested attention map; with a prediction head on
also the two head losses, ``prediction_scores_t`` and every field of an ``lm_predict(labels=..., k=5)`` result; and for every case the
count of ALL kernel launches of the forward + backward (the kernel stamps) and their GEMM launch records (the launch log).  Run it in
two trees and diff the outputs: a host-side refactor of the step engine or of the heads must leave every line as it was.

    python tools/step_bits.py [--tree DIR] [--cases a,b]        (DIR: root of a built checkout, default this one)

Three tensors of the flat gradient buffer -- the position, type and colour embedding tables -- are the ones tests/helpers.py lists
(ATOMIC_GRADS) as free to differ in their last bits between two runs of ONE tree, and the suite's bit-for-bit tests compare them to
rounding only.  Their ranges are cleared before the buffer is hashed; every other gradient has one fixed summation order.

Cases: tiny PlotQA plain / with every request at once / the same with key masks that mask keys out in both streams (a swapped mask in the
co-attention shows here) / tiny FigureQA with areas and one map / long attention (T 113, the shortest length served by
attention_long.hip, whose row statistics the maps' attention sites carry) / the fp8 step (e4m3 context copies, e5m2 dqkv copies) / the
prediction heads on the tiny config, through the public surface only (params, the step adapter, public attributes, ``lm_predict``):
the masked-LM loss / the masked-region loss on class ids (``image_class``) / on soft targets / ``output_lm_scores`` with the loss off and
a cotangent on the scores / both losses, the scores and a requested image_feat gradient in one pass, then a second pass on a lazy clear.
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
    ap.add_argument("--cases", default="plain,all,masks,figureqa,long,fp8,lm,region,region_soft,lmscores,heads")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.tree, "cqa-crct_amd"))
    import ctypes
    import numpy as np
    import torch
    from crct import config as C
    from crct import lib as L
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
        coeffs = {k: over.pop(k) for k in list(over) if k.endswith("_loss_coeff")}      # params['lm_loss_coeff'] / ['img_loss_coeff']; the rest is config
        cfg = C.tiny_config(hidden_dropout_prob=p, attention_probs_dropout_prob=p, v_hidden_dropout_prob=p, v_attention_probs_dropout_prob=p, **over)
        model, params, core = build(cfg, C.default_params(categories=9, L1=True, **coeffs), 7, p)
        batch = S.make_batch(B, T, V, cfg.v_feature_size, categories=9, vocab_size=cfg.vocab_size, seed=11, lengths=lengths, n_vis=n_vis)
        return model, params, core, batch

    def label_tokens(batch, vocab):
        """masked_lm_labels on about a quarter of the tokens (tests/test_lm_loss_gpu.py): one sample without a label, both ends of the vocabulary."""
        B, T = batch["tokens"].shape
        g = torch.Generator().manual_seed(3)
        mask = torch.where(torch.rand(B, T, generator=g) < 0.25, torch.randint(0, vocab, (B, T), generator=g), torch.full((B, T), -1))
        mask[2] = -1
        mask[0, 1], mask[0, 2], mask[1, 3] = 0, vocab - 1, 7
        return dict(batch, mask=mask)

    def label_regions(batch, n_classes, soft):
        """image_label 1 on a few regions with zeroed features, their classes in image_class as ids or as distributions (tests/test_img_loss_gpu.py);
        the rows without a label hold values that must never be looked at."""
        B, V = batch["image_target"].shape
        g = torch.Generator().manual_seed(3)
        label = torch.full((B, V), -1, dtype=torch.int64)
        label[:, 0] = 0
        pick = torch.rand(B, V, generator=g) < 0.35
        pick[:, 0] = False
        pick[2] = False
        pick[0, 1] = pick[0, 2] = pick[1, 3] = True
        label[pick] = 1
        feat = batch["image_feat"].clone()
        feat[pick] = 0.0
        if soft:
            t = torch.rand(B, V, n_classes, generator=g)
            t[torch.rand(B, V, n_classes, generator=g) < 0.3] = 0.0
            t[..., 0] += 1e-3
            t = t / t.sum(-1, keepdim=True)
            t[0, 1] *= 0.5
            t[~pick] = -1.0
            cls = t.float()
        else:
            cls = torch.randint(0, n_classes, (B, V), generator=g)
            cls[0, 1], cls[0, 2], cls[1, 3] = 0, n_classes - 1, 7
            cls[~pick] = 10 ** 6
        return dict(batch, image_label=label, image_feat=feat, image_class=cls)

    def logged(fn):
        """fn() with every kernel launch counted and every GEMM launch recorded (tests/test_seq_outputs_gpu.py): (launches, records)."""
        lib = L.load()
        torch.cuda.synchronize()
        lib.crct_prof_reset()
        lib.crct_prof_enable(2)
        lib.crct_launch_log_enable(1)
        try:
            fn()
            torch.cuda.synchronize()
            n = lib.crct_prof_stamp_count()
            recs = []
            for i in range(lib.crct_launch_log_count()):
                r = L.LaunchRec()
                lib.crct_launch_log_read(i, ctypes.byref(r))
                recs.append((r.site, r.kind, r.M, r.N, r.K, r.cfg, r.n_problems))
        finally:
            lib.crct_launch_log_enable(0)
            lib.crct_prof_enable(0)
            lib.crct_prof_reset()
        return n, recs

    def step(case, model, params, core, batch, it=1, inputs=(), keep_emb=False, seq=False, scores=False, maps=(), heads=False, lm_scores=False,
             lazy_clear=False):
        """One forward + backward at call number `it` on cleared gradients, with a fixed loss term on every requested output."""
        b = dict(batch)
        for n in inputs:
            b[n] = batch[n].detach().clone().requires_grad_(True)
        core.zero_flat_grads(**(dict(lazy=True) if lazy_clear else {}))
        core._calls = it - 1
        core.keep_text_embedding_grad = keep_emb
        core.return_sequence_outputs = seq
        core.differentiable_scores = scores
        if maps or hasattr(core, "attention_map_outputs"):
            core.attention_map_outputs = list(maps)
        passes = {}

        def forward_pass():
            passes["out"] = step_forward(model, b, params, **(dict(output_lm_scores=True) if lm_scores else {}))
        n_fwd, rec_fwd = logged(forward_pass)
        out = passes["out"]
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
        if lm_scores:
            loss = loss + term(core.prediction_scores_t, 1e-2)
        n_bwd, rec_bwd = logged(loss.backward)
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
        if heads or lm_scores:
            items += [("lm_loss (slot 0)", out[1]), ("img_loss (slot 1)", out[3])]
            if lm_scores:
                items.append(("prediction_scores_t", core.prediction_scores_t))
            pred = core.lm_predict(labels=b["mask"], k=5)
            items += [("lm_predict " + f, getattr(pred, f)) for f in pred._fields]
        for name, t in items:
            print("%-10s %-40s %s %s" % (case, name, "x".join(str(s) for s in t.shape), sha(t)), flush=True)
        recs = repr(rec_fwd + rec_bwd).encode()
        print("%-10s %-40s %d+%d %s" % (case, "kernel launches forward+backward", n_fwd, n_bwd, "-"), flush=True)
        print("%-10s %-40s %d+%d %s" % (case, "GEMM launch records forward+backward", len(rec_fwd), len(rec_bwd), hashlib.sha256(recs).hexdigest()), flush=True)

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
        elif case == "lm":
            model, params, core, batch = tiny(lm_loss_coeff=0.5)
            step(case, model, params, core, label_tokens(batch, core.config.vocab_size), heads=True)
        elif case in ("region", "region_soft"):
            model, params, core, batch = tiny(img_loss_coeff=0.5)
            step(case, model, params, core, label_regions(batch, core.config.v_target_size, soft=case == "region_soft"), heads=True)
        elif case == "lmscores":
            model, params, core, batch = tiny()
            step(case, model, params, core, label_tokens(batch, core.config.vocab_size), lm_scores=True)
        elif case == "heads":
            model, params, core, batch = tiny(lm_loss_coeff=0.5, img_loss_coeff=0.5)
            batch = label_regions(label_tokens(batch, core.config.vocab_size), core.config.v_target_size, soft=False)
            for it, lazy in ((1, False), (2, True)):
                step("heads %s" % ("lazy" if lazy else "pass"), model, params, core, batch, it=it, inputs=("image_feat",), heads=True, lm_scores=True,
                     lazy_clear=lazy)
        else:
            raise SystemExit("unknown case %r" % case)


if __name__ == "__main__":
    main()
