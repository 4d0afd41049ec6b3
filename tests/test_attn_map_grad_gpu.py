"""Attention maps as differentiable outputs of the training step (-m gpu): ``core.attention_map_outputs = [("conn", 0, 0), ...]`` leaves the
requested maps in ``core.attention_maps`` after every forward, and in a training forward under grad they are outputs of the step's autograd
node: a loss written on a map trains the query / key projections and everything below them (csrc/attention_probs_bwd.hip behind each
layer's own attention backward, crct_engine_set_attention_map_grads).

* Values: ``core.attention_maps`` equals ``StepEngine.attention_probs`` bit for bit.
* Per layer, per element: the QKV weight gradients of a pass that differentiates ONE map alone (the heads get zero seeds, so the layer's
  dqkv scratch holds bf16 of the map's contribution and nothing else), minus those of the same pass without the request (exact zeros),
  against the fp64 contribution computed from the engine's own t<i>.qkv / v<i>.qkv / c<i>.qkv* taps and the layer's input tap.
* The whole step and the aux term alone against oracle_step under autograd, with O.sdpa wrapped from here to record the maps.
* Off means off: launch for launch and bit for bit.
* The surface: unused maps, GradScaler, FlatGradDDP on one rank, a frozen prefix, the FigureQA variant, the fp8 refusal.

The cotangents are seeded normal draws scaled ONCE, from the oracle alone, to AUX_GAIN times the norm of the oracle's own d loss / d map
(through the context), so that the aux term dominates; the oracle side asserts that this moved the gradients of the affected query / key
tensors (cosine with / without aux below 0.9 on at least half of them).  Checked on the CPU when this file was written: 10 of 10.
"""
import math
import os
from unittest import mock

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from crct import config as C                       # noqa: E402
from crct.step_adapter import forward as step_forward   # noqa: E402
from helpers import ATOMIC_GRADS, GOLDEN, load_case    # noqa: E402
from oracle import crct_oracle as O                # noqa: E402
import attention_ref as AR                         # noqa: E402
import attn_map_grad_ref as MR                     # noqa: E402
from test_input_grad_gpu import _tiny, bits        # noqa: E402
from test_seq_outputs_gpu import _logged, compare_grads, is_head      # noqa: E402
from test_step_gpu import build_model, cosine      # noqa: E402

DEV = torch.device("cuda:0")
AUX_GAIN = 4.0
# one text layer, one visual layer, both directions of one connection layer, and one direction of the other
MAPS = (("text", 1, 0), ("visual", 0, 0), ("conn", 0, 0), ("conn", 0, 1), ("conn", 1, 0))


def qk_names(key):
    """The query and key weight of a map: (query weight, key weight) parameter names."""
    kind, i, direction = key
    if kind == "text":
        p = "bert.encoder.layer.%d.attention.self." % i
        return p + "query.weight", p + "key.weight"
    if kind == "visual":
        p = "bert.encoder.v_layer.%d.attention.self." % i
        return p + "query.weight", p + "key.weight"
    p = "bert.encoder.c_layer.%d.biattention." % i          # stream 1 = visual, 2 = text; direction 0: text queries over visual keys
    return (p + "query2.weight", p + "key1.weight") if direction == 0 else (p + "query1.weight", p + "key2.weight")


def map_keys_in_call_order(cfg):
    """The (kind, index, direction) of every O.sdpa call of one oracle_step, in call order."""
    keys = []
    for kind, i in O.encoder_schedule(cfg):
        keys += [("text", i, 0)] if kind == "t" else [("visual", i, 0)] if kind == "v" else [("conn", i, 0), ("conn", i, 1)]
    return keys


def recording_sdpa(rec):
    """O.sdpa that also appends its (post-dropout) probabilities to `rec`."""
    def sdpa(q, k, v, add_mask, n_heads, p_drop, training):
        qh, kh, vh = O._heads(q, n_heads), O._heads(k, n_heads), O._heads(v, n_heads)
        s = torch.matmul(qh, kh.transpose(-1, -2)) / math.sqrt(qh.shape[-1]) + add_mask
        p = O._drop(torch.softmax(s, dim=-1), p_drop, training)
        rec.append(p)
        return O._merge(torch.matmul(p, vh))
    return sdpa


def _backward_into(sd, scalar):
    for v in sd.values():
        v.grad = None
    scalar.backward(retain_graph=True)
    return {k: (None if v.grad is None else v.grad.detach().clone()) for k, v in sd.items()}


def oracle_with_maps(sd_values, cfg, cpu_params, batch, maps=MAPS, live=None, share=None):
    """oracle_step with its maps recorded; gradients of loss, of loss + aux and of aux alone, aux = sum_maps (G o map).sum()."""
    sd = {k: (v.detach().clone().requires_grad_(True) if live is None or k in live else v.detach().clone()) for k, v in sd_values.items()}
    rec = []
    with mock.patch.object(O, "sdpa", recording_sdpa(rec)):
        out = O.oracle_step(sd, cfg, cpu_params, batch, cls_dropout=0.0)
    named = dict(zip(map_keys_in_call_order(cfg), rec))
    assert len(rec) == len(named)
    loss = out[0].float()
    if share is None:
        gen = torch.Generator().manual_seed(777)
        G = {}
        for key, gm in zip(maps, torch.autograd.grad(loss, [named[k] for k in maps], retain_graph=True)):
            g = torch.randn(named[key].shape, generator=gen)
            G[key] = g * (AUX_GAIN * float(gm.double().norm()) / float(g.double().norm()))
    else:
        G = share
    aux = sum((G[k] * named[k].float()).sum() for k in maps)
    r = dict(G=G, maps={k: named[k].detach().float() for k in maps}, loss=float(loss.detach()))
    trainable = {k: v for k, v in sd.items() if v.requires_grad}
    r["plain"], r["both"], r["aux"] = _backward_into(trainable, loss), _backward_into(trainable, loss + aux), _backward_into(trainable, aux)
    if live is None:
        qk = sorted({n for key in maps for n in qk_names(key)})
        moved = [cosine(r["both"][n].float(), r["plain"][n].float()) for n in qk]
        r["moved"] = (sum(c < 0.9 for c in moved), len(moved))
        print("oracle: aux moves %d of %d affected query / key gradients below cosine 0.9" % r["moved"])
        assert 2 * r["moved"][0] >= r["moved"][1] > 0, (r["moved"], moved)
    return r


_T = {}


def tiny():
    """tiny_L1 (dropout 0): the golden weights and batch, one model for the tests that only read it, and the oracle's passes."""
    if not _T:
        z, meta, cfg, params, batch = load_case("tiny_L1")
        zw = np.load(os.path.join(GOLDEN, "tiny_L1.npz"))
        model, params = build_model(cfg, params, weights=zw)
        model.train()
        core = model.bert_pretrained
        sd = {k[2:]: torch.from_numpy(zw[k]).clone() for k in zw.files if k.startswith("w.")}
        ref = oracle_with_maps(sd, cfg, dict(params, device=torch.device("cpu")), batch)
        _T.update(cfg=cfg, params=params, batch=batch, model=model, core=core, sd=sd, ref=ref, zw=zw)
    t = _T
    return t["cfg"], t["model"], t["params"], t["core"], t["batch"], t["sd"], t["ref"]


def run_step(model, params, core, batch, G, with_loss=True, it=1, scaler=None, zero=True, maps=None):
    """One training forward + backward of loss (with_loss) + sum_maps (G o map).sum(); returns (out, maps of the forward)."""
    core.attention_map_outputs = list(G) if maps is None else list(maps)
    try:
        if zero:
            core.zero_flat_grads()
        core._calls = it - 1
        out = step_forward(model, batch, params)
        got = dict(core.attention_maps)
        terms = ([out[0]] if with_loss else []) + [(g.to(DEV) * got[k]).sum() for k, g in G.items()]
        total = sum(terms[1:], terms[0])
        (total if scaler is None else scaler.scale(total)).backward()
        torch.cuda.synchronize()
    finally:
        core.attention_map_outputs = ()
    return out, got


# ------------------------------------------------------------------------------------------------ 1. values
def test_values_are_the_engines_own_maps_bit_for_bit():
    cfg, model, params, core, batch, sd, ref = tiny()
    B, T = batch["tokens"].shape
    V = batch["image_feat"].shape[1]
    assert core.attention_maps == {} or all(k in MAPS for k in core.attention_maps)
    core.attention_map_outputs = [("conn", 0, 0), ("text", 1), (1, 0, 0), ("conn", 0, 1), (2, 1, 0)]      # names or numbers, direction optional
    try:
        step_forward(model, batch, params)
        got = dict(core.attention_maps)
        assert set(got) == set(MAPS), sorted(got)
        shapes = {"text": (B, cfg.num_attention_heads, T, T), "visual": (B, cfg.v_num_attention_heads, V, V)}
        for key, m in got.items():
            want = shapes.get(key[0], (B, cfg.bi_num_attention_heads, V, T) if key[2] else (B, cfg.bi_num_attention_heads, T, V))
            assert m.dtype == torch.float32 and tuple(m.shape) == want and m.requires_grad, key
            assert torch.equal(bits(m), bits(core._engine.attention_probs(*key))), key
            err = float((m.detach().cpu() - ref["maps"][key]).abs().max())
            assert err < 2e-2, (key, err)
        # evaluation under no_grad: plain tensors, the same bits (dropout 0)
        model.eval()
        try:
            with torch.no_grad():
                step_forward(model, batch, params, evaluation=True)
            for key, m in core.attention_maps.items():
                assert not m.requires_grad and torch.equal(bits(m), bits(got[key])), key
        finally:
            model.train()
    finally:
        core.attention_map_outputs = ()
    step_forward(model, batch, params)
    assert core.attention_maps == {}


# ------------------------------------------------------------------------------------------------ 2. per layer, per element
def _qkv_tap(eng, name, B, T, V, rows, width):
    from crct import lib as L
    buf = torch.empty(B * rows * 3 * width, dtype=torch.bfloat16, device=DEV)
    n = eng.lib.crct_engine_tap(eng.handle, eng.workspace.data_ptr(), name.encode(), B, T, V, buf.data_ptr(), buf.numel(), L.current_stream())
    assert n == buf.numel(), (name, n, eng.lib.crct_last_error())
    return buf.view(B, rows, 3 * width).cpu()


def _layer_operands(eng, cfg, batch, key):
    """(q, k, keymask, heads, d, x_q, x_k) of a map from the engine's taps: q / k [B, T*, H] bf16, the inputs of the layer's query and key
    projections (the states the schedule step before it left)."""
    kind, i, direction = key
    B, T = batch["tokens"].shape
    V = batch["image_feat"].shape[1]
    km_t = O.text_key_mask(batch["sep_indices"], batch["hist_len"], T).to(torch.uint8)
    km_v = (batch["image_mask"] != 0).to(torch.uint8)
    sched = O.encoder_schedule(cfg)
    at = sched.index(({"text": "t", "visual": "v", "conn": "c"}[kind], i))
    assert at > 0, "the first schedule step reads the embeddings, which have no tap"
    prev = "%s%d" % sched[at - 1]
    xt, xv = eng.tap(prev + ".t", B, T, V).cpu(), eng.tap(prev + ".v", B, T, V).cpu()
    if kind == "text":
        H = cfg.hidden_size
        x = _qkv_tap(eng, "t%d.qkv" % i, B, T, V, T, H)
        return x[:, :, :H], x[:, :, H:2 * H], km_t, cfg.num_attention_heads, H // cfg.num_attention_heads, xt, xt
    if kind == "visual":
        H = cfg.v_hidden_size
        x = _qkv_tap(eng, "v%d.qkv" % i, B, T, V, V, H)
        return x[:, :, :H], x[:, :, H:2 * H], km_v, cfg.v_num_attention_heads, H // cfg.v_num_attention_heads, xv, xv
    H, nh = cfg.bi_hidden_size, cfg.bi_num_attention_heads
    x1, x2 = _qkv_tap(eng, "c%d.qkv1" % i, B, T, V, V, H), _qkv_tap(eng, "c%d.qkv2" % i, B, T, V, T, H)
    if direction == 0:
        return x2[:, :, :H], x1[:, :, H:2 * H], km_v, nh, H // nh, xt, xv
    return x1[:, :, :H], x2[:, :, H:2 * H], km_t, nh, H // nh, xv, xt


def _one_map_alone(model, params, core, batch, cfg, key, seed):
    """A pass that differentiates `key`'s map alone, against fp64 from the engine's own taps.  Returns the worst budget ratio."""
    core.attention_map_outputs = [key]
    try:
        core.zero_flat_grads()
        core._calls = 0
        out = step_forward(model, batch, params)
        m = core.attention_maps[key]
        G = torch.randn(m.shape, generator=torch.Generator().manual_seed(seed))
        # without the request: the same pass with a zero seed of the loss and the map unused -- every gradient an exact zero
        torch.autograd.backward([out[0]], [torch.zeros((), device=DEV)], retain_graph=True)
        torch.cuda.synchronize()
        without = {n: p.grad.detach().clone() for n, p in core.named_parameters() if p.grad is not None}
        assert all(float(g.abs().max()) == 0.0 for g in without.values())
        core.zero_flat_grads()
        m.backward(G.to(DEV))
        torch.cuda.synchronize()
    finally:
        core.attention_map_outputs = ()
    q, k, km, heads, d, xq, xk = _layer_operands(core._engine, cfg, batch, key)
    (cq, ck), (bq, bk) = MR.reference(q, k, km, G, 1.0, heads, d)          # c = CrctStepCfg.grad_scale = 1 outside a data-parallel group
    grads = dict(core.named_parameters())
    worst = 0.0
    for name, contrib, budget, x in zip(qk_names(key), (cq, ck), (bq, bk), (xq, xk)):
        # dqkv holds bf16(contribution): per element within budget + one bf16 step; the weight-gradient GEMM sums rows in fp32
        rows = contrib.reshape(-1, contrib.shape[-1])
        xa = x.double().reshape(-1, x.shape[-1])
        ref = rows.t() @ xa
        tol = (budget.reshape(rows.shape) + AR.bf16_step(rows)).t() @ xa.abs() + AR.S32 * (rows.abs().t() @ xa.abs())
        got = (grads[name].grad - without[name]).double().cpu()
        assert float(ref.abs().max()) > 0.0
        r = (got - ref).abs() / tol
        assert bool((r <= 1.0).all()), (key, name, float(r.max()), int((r > 1).sum()))
        worst = max(worst, float(r.max()))
    # nothing else enters this layer's QKV gradients: the value projection's stays an exact zero
    vname = qk_names(key)[0].replace("query", "value")
    assert float(grads[vname].grad.abs().max()) == 0.0, vname
    return worst


@pytest.mark.parametrize("key", MAPS[:4], ids=["text1", "visual0", "conn0_text_over_visual", "conn0_visual_over_text"])
def test_one_map_alone_against_fp64_from_the_engines_own_taps(key):
    cfg, model, params, core, batch, sd, ref = tiny()
    worst = _one_map_alone(model, params, core, batch, cfg, key, 31 + MAPS.index(key))
    print("map %s alone: largest |QKV weight gradient - fp64| / budget %.2f" % (key, worst))


# ------------------------------------------------------------------------------------------------ 3. the whole step and aux alone
def test_whole_step_with_aux_on_five_maps_matches_the_oracle():
    """tiny_L1, L = loss + sum_maps (G o map).sum(): every parameter gradient cosine >= 0.99, norm within 5 % (compare_grads)."""
    cfg, model, params, core, batch, sd, ref = tiny()
    out, got = run_step(model, params, core, batch, ref["G"])
    assert abs(float(out[0].detach()) - ref["loss"]) <= 2e-2 * abs(ref["loss"])
    n = compare_grads(core, ref["both"], "tiny_L1 loss + aux on maps")
    assert n > 60


def test_aux_alone_trains_what_lies_below_the_maps_and_leaves_the_heads_at_zero():
    cfg, model, params, core, batch, sd, ref = tiny()
    out, got = run_step(model, params, core, batch, ref["G"], with_loss=False)
    below = {k for k, _ in core.named_parameters() if not is_head(k)}
    n = compare_grads(core, ref["aux"], "tiny_L1 aux on maps alone", names=below)
    assert n > 30
    for k, p in core.named_parameters():
        if is_head(k):
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k


# ------------------------------------------------------------------------------------------------ 4. off means off
def test_off_means_off_launch_for_launch_and_bit_for_bit():
    """(a) a model whose attribute was never touched and one with it set to an empty list: the same launches and GEMM records in forward
    and backward, the same gradient bits.  (b) maps requested but not used in backward (None upstream): the forward launches exactly one
    kernel per map more, the backward none, same bits.  (c) used: two launches per map more in backward."""
    cfg, model, params, core, batch = _tiny()                 # dropout on
    assert core.attention_map_outputs == () and core.attention_maps == {}

    def fwd(it=1):
        core.zero_flat_grads()
        core._calls = it - 1
        return step_forward(model, batch, params)

    def step(use=None):
        out, nf, lf = _logged(fwd)
        total = out[0] if use is None else out[0] + sum((core.attention_maps[k] * 0.5).sum() for k in use)
        _, nb, lb = _logged(lambda: total.backward())
        return out, (nf, nb), (lf, lb), core.flat_grads.clone()
    fwd()[0].backward()                                       # builds the engine and refreshes the bf16 weight shadow: not part of a step
    ws0 = core._engine.workspace.numel()
    out0, n0, log0, g0 = step()
    core.attention_map_outputs = []
    out1, n1, log1, g1 = step()
    assert n1 == n0 and log1 == log0 and torch.equal(bits(out1[0].detach()), bits(out0[0].detach())) and core.attention_maps == {}
    core.attention_map_outputs = list(MAPS[:3])
    try:
        out2, n2, log2, g2 = step()
        assert n2 == (n0[0] + 3, n0[1]), (n0, n2)
        assert log2 == log0 and torch.equal(bits(out2[0].detach()), bits(out0[0].detach()))
        assert core._engine.workspace.numel() == ws0          # an unused request never reaches the engine
        out3, n3, log3, g3 = step(use=MAPS[:2])
        assert n3 == (n0[0] + 3, n0[1] + 4), (n0, n3)         # two launches per used map (the stamps count the library's kernels only)
        assert log3 == log0
    finally:
        core.attention_map_outputs = ()
    out4, n4, log4, g4 = step()
    assert n4 == n0 and log4 == log0
    for e in core.table:
        a = g0[e.offset:e.offset + e.numel]
        for g in (g1, g2, g4):
            b = g[e.offset:e.offset + e.numel]
            if e.name in ATOMIC_GRADS:
                assert torch.allclose(a, b, rtol=1e-3, atol=1e-6), e.name
            else:
                assert torch.equal(bits(a), bits(b)), e.name
    qn = qk_names(MAPS[0])[0]
    e = next(e for e in core.table if e.name == qn)
    assert not torch.equal(bits(g0[e.offset:e.offset + e.numel]), bits(g3[e.offset:e.offset + e.numel])), "the used map left no trace"


# ------------------------------------------------------------------------------------------------ 5. the surface
def _small_G(core, model, params, batch, maps, seed, std=0.05):
    core.attention_map_outputs = list(maps)
    try:
        with torch.no_grad():
            step_forward(model, batch, params)
        gen = torch.Generator().manual_seed(seed)
        return {k: torch.randn(core.attention_maps[k].shape, generator=gen) * std for k in maps}
    finally:
        core.attention_map_outputs = ()


def test_grad_scaler_unscales_to_the_plain_gradients():
    cfg, model, params, core, batch = _tiny()
    G = _small_G(core, model, params, batch, MAPS[:3], 5)
    run_step(model, params, core, batch, G)
    plain = core.flat_grads.clone()
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=10 ** 6)
    run_step(model, params, core, batch, G, scaler=scaler)
    unscaled = core.flat_grads / 1024.0                       # the unscale: a power of two, exact
    used = torch.cat([torch.arange(e.offset, e.offset + e.numel) for e in core.table if e.used and e.name not in ATOMIC_GRADS]).to(DEV)
    err = (unscaled[used] - plain[used]).abs().max() / plain[used].abs().max()
    print("GradScaler 1024 with aux on maps: max |unscaled - plain| / max |plain| = %.3g" % float(err))
    assert float(err) <= 1e-6


def test_flat_grad_ddp_at_world_one_gives_the_plain_bits():
    import torch.distributed as dist
    from crct.ddp import FlatGradDDP
    cfg, model, params, core, batch = _tiny()
    G = _small_G(core, model, params, batch, MAPS[:4], 6)
    run_step(model, params, core, batch, G)
    base = core.flat_grads.clone()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29571")
    torch.cuda.set_device(0)
    dist.init_process_group(backend="nccl", rank=0, world_size=1, device_id=DEV)
    try:
        ddp = FlatGradDDP(model, device_ids=[0], find_unused_parameters=True)
        run_step(ddp, params, core, batch, G)
        for e in core.table:
            if e.used and e.name not in ATOMIC_GRADS:
                assert torch.equal(bits(base[e.offset:e.offset + e.numel]), bits(core.flat_grads[e.offset:e.offset + e.numel])), e.name
    finally:
        core._ddp = None
        dist.destroy_process_group()


def test_a_frozen_prefix_and_a_map_in_a_segment_that_does_not_run():
    """fixed_t_layer = 1 with the text embeddings without gradient too: the segment of text layer 0 does not run, a requested map of it
    contributes nothing (the plain gradients, bit for bit), and the maps above it still match the oracle with the same tensors detached."""
    cfg0, _, _, _, batch, sd, ref = tiny()
    z, meta, _, params, _ = load_case("tiny_L1")
    cfg = C.BertConfig.from_dict(dict(meta["cfg"], fixed_t_layer=1))
    model, params = build_model(cfg, params, weights=_T["zw"])
    model.train()
    core = model.bert_pretrained
    for k, p in core.named_parameters():
        if k.startswith("bert.embeddings."):
            p.requires_grad_(False)
    G0 = _small_G(core, model, params, batch, [("text", 0, 0)], 9, std=1.0)
    run_step(model, params, core, batch, {})
    plain = core.flat_grads.clone()
    live = {k for k, p in core.named_parameters() if p.grad is not None}
    assert not any(k.startswith(("bert.encoder.layer.0.", "bert.embeddings.")) for k in live) and len(live) > 30
    plan = core._engine.backward_plan()
    seg_t0 = len(O.encoder_schedule(cfg)) - O.encoder_schedule(cfg).index(("t", 0))
    assert not plan[seg_t0][0], plan
    run_step(model, params, core, batch, G0)
    for e in core.table:
        if e.used and e.name in live and e.name not in ATOMIC_GRADS:
            assert torch.equal(bits(plain[e.offset:e.offset + e.numel]), bits(core.flat_grads[e.offset:e.offset + e.numel])), e.name
    # the maps above the frozen prefix, against the oracle with the same tensors detached (the cotangents of the unfrozen pass)
    fro = oracle_with_maps(sd, cfg0, dict(params, device=torch.device("cpu")), batch, live=live, share=ref["G"])
    run_step(model, params, core, batch, ref["G"])
    compare_grads(core, fro["both"], "tiny_L1 frozen prefix, loss + aux on maps", names=live)


def test_figureqa_variant_one_map_alone():
    """The tiny FigureQA fixture (binary answers, areas, no feature embedding) with its dropout set to 0: a co-attention map alone."""
    from test_variants_gpu import load_variant, variant_model
    z, meta, cfg, params, batch = load_variant("variant_tiny_figureqa")
    for k in ("hidden_dropout_prob", "attention_probs_dropout_prob", "v_hidden_dropout_prob", "v_attention_probs_dropout_prob"):
        setattr(cfg, k, 0.0)
    model, params = variant_model(meta, cfg, params)
    model.train()
    core = model.bert_pretrained
    assert core.variant[0] == "figure_qa", core.variant
    key = ("conn", len(cfg.v_biattention_id) - 1, 0)
    worst = _one_map_alone(model, params, core, batch, cfg, key, 77)
    print("FigureQA map %s alone: largest |QKV weight gradient - fp64| / budget %.2f" % (key, worst))


def test_refusals_fp8_backward_and_maps_out_of_range():
    z, meta, cfg, params, batch = load_case("tiny_L1")
    model, params = build_model(cfg, dict(params, fp8=True), weights=None, seed=3)
    core = model.bert_pretrained
    assert core.fp8 and core.fp8_backward
    core.attention_map_outputs = [("conn", 0, 0)]
    with pytest.raises(NotImplementedError, match="fp8_backward"):
        step_forward(model, batch, params)
    # the engine's own refusals
    _, model2, params2, core2, _, _, _ = tiny()
    step_forward(model2, batch, params2)
    eng = core2._engine
    g = torch.zeros(4, device=DEV)
    for bad, word in (((2, 5, 0, g), "connection layer 5 out of range"), ((0, 1, 1, g), "direction 1 belongs to connection layers"),
                      ((3, 0, 0, g), "unknown kind 3"), ((1, -1, 0, g), "visual layer -1 out of range")):
        with pytest.raises(RuntimeError, match=word):
            eng.set_attention_map_grads([bad])
    with pytest.raises(ValueError, match="contiguous fp32"):
        eng.set_attention_map_grads([(0, 0, 0, g.double())])
    with pytest.raises(ValueError, match="kind must be"):
        core2.attention_map_outputs = [("cross", 0)]
        try:
            step_forward(model2, batch, params2)
        finally:
            core2.attention_map_outputs = ()
