"""Frozen layers on the native step (-m gpu): ``fixed_t_layer`` / ``fixed_v_layer`` and ``requires_grad_(False)``.

Every comparison is against the same seeded weights and batch with nothing frozen, and bit for bit: above the cut the same kernels
read the same inputs (``no_grad`` does not turn dropout off, the forward is unchanged).  The one tolerance -- the clipped norm
against float64 -- is the bound tests/test_clip_grad_gpu.py derives (4e-6 relative).

Shapes: B 3, T 9, V 5 on the tiny configs (a frozen and a running self layer per stream, a co-attention step above them, row
counts off every tile multiple), and one full-depth run of ``vilbert_config()`` at B 2, V 36, T 20 with ``fixed_t_layer = 6``.
"""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from crct import config as C                       # noqa: E402
from crct import layout                            # noqa: E402
from crct import lib as L                          # noqa: E402
from crct import synthetic as S                    # noqa: E402
from crct.model import VisualDialogEncoder         # noqa: E402
from crct.step_adapter import forward as step_forward   # noqa: E402
from helpers import GOLDEN                         # noqa: E402

DEV = torch.device("cuda:0")
NORM_RTOL = 4e-6
SENTINEL = 0x5EA7BEE5            # an int32 bit pattern no kernel produces by accident (fp32 2.4e19)
HEADS = ("bert.t_pooler.", "bert.v_pooler.", "cls.bi_seq_relationship.", "regressor.")

with open(os.path.join(GOLDEN, "frozen_names.json")) as _f:
    FIXTURE = json.load(_f)
BASE = C.default_params(categories=9, L1=True)
DROP = dict(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, v_hidden_dropout_prob=0.1, v_attention_probs_dropout_prob=0.1)


def bits(t):
    return t.contiguous().view(torch.int32)


def build(cfg, dropout=False, base=BASE, seed=7):
    params = dict(base, device=DEV)
    model = VisualDialogEncoder(params, config=cfg)
    core = model.bert_pretrained
    core.cls_dropout = 0.1 if dropout else 0.0
    S.seeded_fill_(model.state_dict(), base_seed=seed)
    core._invalidate_shadow()
    return model, params, core


def tiny_batch(cfg):
    return S.make_batch(3, 9, 5, cfg.v_feature_size, categories=9, vocab_size=cfg.vocab_size, seed=11)


def used(core):
    byname = dict(core.named_parameters())
    return [(e, byname[e.name]) for e in core.table if e.used]


def step(model, params, core, batch, it=1, sentinel=(), before_backward=None):
    """One forward + backward at call number ``it`` (the dropout seed) on cleared gradients.  ``sentinel``: names whose range of the
    flat gradient buffer is filled with SENTINEL between forward and backward.  Returns outputs and cloned gradients."""
    core.zero_flat_grads()
    core._calls = it - 1
    out = step_forward(model, batch, params)
    ents = {e.name: e for e in core.table}
    for n in sentinel:
        e = ents[n]
        bits(core.flat_grads)[e.offset:e.offset + e.numel] = SENTINEL
    if before_backward is not None:
        before_backward()
    out[0].backward()
    torch.cuda.synchronize()
    grads = {e.name: (None if p.grad is None else p.grad.detach().clone()) for e, p in used(core)}
    return dict(loss=out[0].detach().clone(), logits=out[4].detach().clone(), reg=[r.detach().clone() for r in (out[5][0], out[5][1], out[5][2], out[5][4])],
                grads=grads)


def sentinel_intact(core, names):
    ents = {e.name: e for e in core.table}
    bad = [n for n in names if not bool((bits(core.flat_grads)[ents[n].offset:ents[n].offset + ents[n].numel] == SENTINEL).all())]
    return bad


def same_outputs(a, b):
    assert torch.equal(bits(a["loss"].reshape(1)), bits(b["loss"].reshape(1)))
    assert torch.equal(bits(a["logits"]), bits(b["logits"]))
    for x, y in zip(a["reg"], b["reg"]):
        assert torch.equal(bits(x.float()), bits(y.float()))


def same_grads(frozen, free, without):
    """Tensors in ``without`` have no gradient in ``frozen``; every other gradient has the unfrozen run's bits."""
    for n, g in frozen["grads"].items():
        if n in without:
            assert g is None, n
        else:
            assert g is not None and free["grads"][n] is not None, n
            assert torch.equal(bits(g), bits(free["grads"][n])), n


def frozen_used(core, names):
    """``names`` without the tensors that never receive a gradient anyway."""
    mine = {e.name for e in core.table if e.used}
    return [n for n in names if n in mine]


_FREE = {}


def unfrozen(case, dropout):
    """The reference run of a case: same config with both fields 0, computed once and left unchanged."""
    key = (case, dropout)
    if key not in _FREE:
        over = dict(FIXTURE[case]["config"], fixed_t_layer=0, fixed_v_layer=0)
        cfg = C.tiny_config(**dict(over, **(DROP if dropout else {})))
        model, params, core = build(cfg, dropout)
        _FREE[key] = step(model, params, core, tiny_batch(cfg))
    return _FREE[key]


def case_cfg(case, dropout):
    return C.tiny_config(**dict(FIXTURE[case]["config"], **(DROP if dropout else {})))


# ------------------------------------------------------------------------------------------------ checks 1 - 3: the config route
@pytest.mark.parametrize("dropout", [False, True])
@pytest.mark.parametrize("case", ["A", "B"])
def test_config_route_matches_the_unfrozen_step(case, dropout):
    cfg = case_cfg(case, dropout)
    model, params, core = build(cfg, dropout)
    names = frozen_used(core, FIXTURE[case]["grad_is_none"])
    assert names
    got = step(model, params, core, tiny_batch(cfg), sentinel=names)
    free = unfrozen(case, dropout)
    same_outputs(got, free)
    same_grads(got, free, set(names))
    assert core.tensors_without_grad == frozenset(names)
    # the config route does not flip requires_grad (the reference does not either)
    assert all(p.requires_grad for p in core.parameters())
    # every frozen tensor belongs to a step that does not run (or to an embedding half that does not): never written
    assert sentinel_intact(core, names) == []


def segment_of(eng, entry):
    for i, (lo, hi) in enumerate(eng.segments):
        if lo <= entry.offset < hi:
            return i
    raise AssertionError(entry.name)


@pytest.mark.parametrize("case", ["A", "B"])
def test_plan_names_the_segments_that_do_not_run(case):
    cfg = case_cfg(case, False)
    model, params, core = build(cfg)
    step(model, params, core, tiny_batch(cfg))
    eng = core._engine
    plan = eng.backward_plan()
    sched = layout.encoder_schedule(cfg)
    n = len(sched) + 2
    assert len(plan) == n == eng.n_segments
    frozen_steps = [("t", i) for i in range(cfg.fixed_t_layer)] + [("v", i) for i in range(cfg.fixed_v_layer)]
    for i, st in enumerate(sched):
        assert plan[len(sched) - i][0] == (st not in frozen_steps), (st, plan)          # segment of schedule step i
    assert plan[0] == (True, True, True, 0)
    # the embedding segment: each half follows its own stream
    assert plan[-1][1] == (cfg.fixed_t_layer == 0) and plan[-1][2] == (cfg.fixed_v_layer == 0)
    # the lowest running step of a frozen stream produces no input gradient
    first_conn = next(i for i, st in enumerate(sched) if st[0] == "c")
    pc = plan[len(sched) - first_conn]
    assert pc[0] and pc[1] == (cfg.fixed_t_layer == 0) and pc[2] == (cfg.fixed_v_layer == 0)
    assert all(p[3] == 0 for p in plan)


# ------------------------------------------------------------------------------------------------ check 4: launches
def count_launches(core, model, params, batch, segmented):
    """Stamped launches of one backward pass: per engine call (segment index, or -1 for the whole pass)."""
    lib = L.load()
    counts = {}
    core.zero_flat_grads()
    core._calls = 0
    out = step_forward(model, batch, params)
    eng = core._engine
    orig = eng.backward

    def counted(p32, p16, g32, tensors, st, seg=-1):
        torch.cuda.synchronize()
        lib.crct_prof_reset()
        orig(p32, p16, g32, tensors, st, seg)
        torch.cuda.synchronize()
        counts[int(seg)] = lib.crct_prof_stamp_count()

    eng.backward = counted
    core.force_segmented = bool(segmented)
    lib.crct_prof_enable(2)
    try:
        out[0].backward()
    finally:
        lib.crct_prof_enable(0)
        lib.crct_prof_reset()
        core.force_segmented = False
        del eng.backward
    torch.cuda.synchronize()
    return counts


def check_launches(free_model, frozen_model, batch, expect_idle):
    fm, fp, fc = free_model
    zm, zp, zc = frozen_model
    per_seg = count_launches(fc, fm, fp, batch, segmented=True)
    whole = count_launches(fc, fm, fp, batch, segmented=False)[-1]
    frozen = count_launches(zc, zm, zp, batch, segmented=False)[-1]
    plan = zc._engine.backward_plan()
    idle = [i for i, p in enumerate(plan) if not p[0]]
    assert idle == expect_idle, (idle, expect_idle)
    saved = sum(per_seg[i] for i in idle)
    print("launches: unfrozen %d (by segment %d), frozen %d, segments that do not run %s hold %d" % (whole, sum(per_seg.values()), frozen, idle, saved))
    assert all(per_seg[i] > 0 for i in idle)
    assert frozen <= whole - saved
    # a segment that does not run returns at once and issues nothing
    seg_counts = count_launches(zc, zm, zp, batch, segmented=True)
    assert all(seg_counts[i] == 0 for i in idle) and all(seg_counts[i] > 0 for i in range(len(plan)) if i not in idle)


@pytest.mark.parametrize("case", ["A", "B"])
def test_frozen_backward_issues_fewer_launches(case):
    cfg = case_cfg(case, False)
    free_cfg = C.tiny_config(**dict(FIXTURE[case]["config"], fixed_t_layer=0, fixed_v_layer=0))
    sched = layout.encoder_schedule(cfg)
    frozen_steps = [("t", i) for i in range(cfg.fixed_t_layer)] + [("v", i) for i in range(cfg.fixed_v_layer)]
    idle = sorted(len(sched) - i for i, st in enumerate(sched) if st in frozen_steps)
    if cfg.fixed_t_layer and cfg.fixed_v_layer:          # both embeddings frozen: the embedding segment does not run either
        idle.append(len(sched) + 1)
    check_launches(build(free_cfg), build(cfg), tiny_batch(cfg), idle)


def test_heads_only_runs_segment_zero_alone():
    cfg = C.tiny_config()
    batch = tiny_batch(cfg)
    free = build(cfg)
    model, params, core = build(cfg)
    for n, p in core.named_parameters():
        if not n.startswith(HEADS):
            p.requires_grad_(False)
    check_launches(free, (model, params, core), batch, list(range(1, len(layout.encoder_schedule(cfg)) + 2)))
    ref = step(*free, batch)
    names = [e.name for e, _ in used(core) if not e.name.startswith(HEADS)]
    got = step(model, params, core, batch, sentinel=names)
    same_outputs(got, ref)
    same_grads(got, ref, set(names))
    assert sentinel_intact(core, names) == []


# ------------------------------------------------------------------------------------------------ check 5: requires_grad_
@pytest.mark.parametrize("case", ["A", "B"])
def test_requires_grad_route_is_the_config_route_and_can_be_undone(case):
    free_cfg = C.tiny_config(**dict(FIXTURE[case]["config"], fixed_t_layer=0, fixed_v_layer=0))
    model, params, core = build(free_cfg)
    batch = tiny_batch(free_cfg)
    byname = dict(core.named_parameters())
    for n in FIXTURE[case]["grad_is_none"]:
        byname[n].requires_grad_(False)
    names = frozen_used(core, FIXTURE[case]["grad_is_none"])
    got = step(model, params, core, batch, sentinel=names)
    free = unfrozen(case, False)
    same_outputs(got, free)
    same_grads(got, free, set(names))
    assert sentinel_intact(core, names) == []
    cfg_model, cfg_params, cfg_core = build(case_cfg(case, False))
    step(cfg_model, cfg_params, cfg_core, batch)
    assert core._engine.backward_plan() == cfg_core._engine.backward_plan()
    # thawed: the next step is the unfrozen step again, and every gradient is a view of the flat buffer again
    for n in FIXTURE[case]["grad_is_none"]:
        byname[n].requires_grad_(True)
    again = step(model, params, core, batch)
    same_outputs(again, free)
    same_grads(again, free, set())
    assert core.tensors_without_grad == frozenset()
    lo, hi = core.flat_grads.data_ptr(), core.flat_grads.data_ptr() + 4 * core.flat_grads.numel()
    assert all(lo <= p.grad.data_ptr() < hi for _, p in used(core))
    assert all(p[0] and p[3] == 0 for p in core._engine.backward_plan())


# ------------------------------------------------------------------------------------------------ check 6: partial freezes
def partial(names, sentinel):
    cfg = C.tiny_config()
    batch = tiny_batch(cfg)
    key = ("plain", False)
    if key not in _FREE:
        _FREE[key] = step(*build(cfg), batch)
    model, params, core = build(cfg)
    byname = dict(core.named_parameters())
    for n in names:
        byname[n].requires_grad_(False)
    got = step(model, params, core, batch, sentinel=sentinel)
    same_outputs(got, _FREE[key])
    same_grads(got, _FREE[key], set(names))
    return core


def test_a_linear_weight_whose_bias_rides_elsewhere_loses_its_gemm():
    name = "bert.encoder.layer.1.attention.output.dense.weight"
    core = partial([name], [name])
    assert sentinel_intact(core, [name]) == []
    eng = core._engine
    plan = eng.backward_plan()
    seg = segment_of(eng, core._entries[name])
    assert all(p[0] and p[1] and p[2] for p in plan)
    assert [p[3] for p in plan] == [1 if i == seg else 0 for i in range(len(plan))]


def test_a_linear_weight_whose_bias_rides_on_its_gemm_keeps_it():
    core = partial(["bert.encoder.layer.1.intermediate.dense.weight"], [])
    assert all(p == (True, True, True, 0) for p in core._engine.backward_plan())
    # with its bias frozen too, nothing rides on the GEMM any more
    names = ["bert.encoder.layer.1.intermediate.dense.weight", "bert.encoder.layer.1.intermediate.dense.bias"]
    core = partial(names, names[:1])
    assert sentinel_intact(core, names[:1]) == []
    assert sum(p[3] for p in core._engine.backward_plan()) == 1


def test_a_fused_qkv_gemm_goes_only_with_all_three_weights_and_biases():
    pre = "bert.encoder.v_layer.0.attention.self."
    core = partial([pre + "query.weight", pre + "key.weight"], [])
    assert sum(p[3] for p in core._engine.backward_plan()) == 0
    names = [pre + "%s.%s" % (a, b) for a in ("query", "key", "value") for b in ("weight", "bias")]
    core = partial(names, [n for n in names if n.endswith("weight")])
    assert sentinel_intact(core, [n for n in names if n.endswith("weight")]) == []
    assert sum(p[3] for p in core._engine.backward_plan()) == 1


def test_the_word_table_alone_drops_its_scatter():
    name = "bert.embeddings.word_embeddings.weight"
    core = partial([name], [name])          # position / type / LayerNorm gradients: compared bit for bit in partial()
    assert sentinel_intact(core, [name]) == []
    assert all(p == (True, True, True, 0) for p in core._engine.backward_plan())


# ------------------------------------------------------------------------------------------------ check 7: optimizer
def opt_state(core, opt):
    opt.synchronize()
    torch.cuda.synchronize()
    return dict(p=bits(core.flat_params).clone(), m=bits(opt._m).clone(), v=bits(opt._v).clone(), s=bits(core.flat_shadow.float()).clone())


def ranges_equal(a, b, entries):
    return [e.name for e in entries if not torch.equal(a[e.offset:e.offset + e.numel], b[e.offset:e.offset + e.numel])]


def train(cfg, batch, overlap, steps, scaler=False):
    from crct.optim import get_optimizer
    model, params, core = build(cfg)
    opt = get_optimizer(dict(params, lr=1e-3, image_lr=2e-3, wd=0.01), model)
    opt.overlap = overlap
    sc = torch.amp.GradScaler("cuda", init_scale=1024.0) if scaler else None
    core._refresh_shadow()               # the bf16 shadow of the seeded weights (the first forward would write it)
    states = [opt_state(core, opt)]
    for it in range(1, steps + 1):
        core._calls = it - 1
        loss = step_forward(model, batch, params)[0]
        (sc.scale(loss) if sc else loss).backward()
        if sc:
            sc.step(opt)
            sc.update()
        else:
            opt.step()
        opt.zero_grad()
        states.append(opt_state(core, opt))
    return core, opt, states


@pytest.mark.parametrize("mode", ["default", "overlap", "scaler"])
def test_optimizer_updates_exactly_the_tensors_with_gradient(mode):
    cfg, free_cfg = case_cfg("A", False), C.tiny_config()
    batch = tiny_batch(cfg)
    steps = 1 if mode == "scaler" else 3
    core, opt, st = train(cfg, batch, mode == "overlap", steps, scaler=mode == "scaler")
    fcore, fopt, fst = train(free_cfg, batch, mode == "overlap", 1, scaler=mode == "scaler")
    without = core.tensors_without_grad
    assert without == frozenset(frozen_used(core, FIXTURE["A"]["grad_is_none"]))
    with_grad = [e for e, _ in used(core) if e.name not in without]
    no_grad = [e for e, _ in used(core) if e.name in without]
    # after step 1 the tensors with gradient are the unfrozen run's: weights, moments and bf16 shadow
    for k in "pmvs":
        assert ranges_equal(st[1][k], fst[1][k], with_grad) == [], k
    assert ranges_equal(st[1]["p"], st[0]["p"], with_grad[:1]) != []           # ... and they did move
    # the tensors without gradient keep weights, both moments and shadow over every step, bit for bit
    for s in st[1:]:
        for k in "pmvs":
            assert ranges_equal(s[k], st[0][k], no_grad) == [], k
    assert bool((st[-1]["m"][no_grad[0].offset:no_grad[0].offset + no_grad[0].numel] == 0).all())
    # the checkpoint layout is the reference's: one group per tensor, frozen or not
    assert len(opt.state_dict()["param_groups"]) == len(fopt.state_dict()["param_groups"])
    assert opt.covers_every_gradient()


# ------------------------------------------------------------------------------------------------ check 8: clipping
def test_clip_grad_norm_never_reads_a_range_without_gradient():
    cfg = case_cfg("A", False)
    from crct.optim import get_optimizer
    model, params, core = build(cfg)
    opt = get_optimizer(params, model)
    step(model, params, core, tiny_batch(cfg))
    for e, _ in used(core):
        if e.name in core.tensors_without_grad:
            core.flat_grads[e.offset:e.offset + e.numel] = float("nan")
    n = opt.clip_grad_norm_(float("inf"))
    per = opt.grad_norms()
    torch.cuda.synchronize()
    got = float(n)
    sq = {e.name: p.grad.double().pow(2).sum() for e, p in used(core) if p.grad is not None}
    ref = float(torch.stack(list(sq.values())).sum().sqrt())
    print("norm %.9g float64 %.9g rel %.3g" % (got, ref, abs(got - ref) / ref))
    assert got == got and got != float("inf") and ref > 0.0
    assert abs(got - ref) <= NORM_RTOL * ref
    for name, v in zip(opt.grad_norm_names, per.tolist()):
        if name in sq:
            assert abs(v - float(sq[name].sqrt())) <= NORM_RTOL * float(sq[name].sqrt()), name
        else:
            assert v == 0.0, name


# ------------------------------------------------------------------------------------------------ check 9: single-rank exchange
def test_single_rank_exchange_covers_the_ranges_with_gradient():
    import torch.distributed as dist
    from crct.ddp import FlatGradDDP
    from crct.optim import get_optimizer
    cfg = case_cfg("A", False)
    batch = tiny_batch(cfg)
    plain_core, plain_opt, plain = train(cfg, batch, False, 1)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(29600 + os.getpid() % 300))
    dist.init_process_group(backend="nccl", rank=0, world_size=1)
    cores = []
    try:
        for dtype in (torch.float32, torch.bfloat16):
            model, params, core = build(cfg)
            cores.append(core)
            opt = get_optimizer(dict(params, lr=1e-3, image_lr=2e-3, wd=0.01), model)
            ddp = FlatGradDDP(model, bucket_mb=0.05, broadcast=False, grad_dtype=dtype)
            ddp.force_exchange = True
            core._refresh_shadow()
            before = opt_state(core, opt)
            core._calls = 0
            step_forward(model, batch, params)[0].backward()          # the exchange hangs on the core's backward
            torch.cuda.synchronize()
            assert ddp.last_exchange is not None and len(ddp.last_exchange.issue_order) == len(ddp._buckets) > 1
            without = core.tensors_without_grad
            sent = torch.zeros(core.flat_grads.numel(), dtype=torch.bool)
            for _, lo, hi in ddp._buckets:
                assert not bool(sent[lo:hi].any())
                sent[lo:hi] = True
            for e, _ in used(core):
                inside = sent[e.offset:e.offset + e.numel]
                assert bool(inside.all()) if e.name not in without else not bool(inside.any()), e.name
            # events and callbacks at bucket ends agree with the engine's plan: every bucket ends on a segment the plan knows
            plan = core._engine.backward_plan()
            assert all(0 <= last < len(plan) for last, _, _ in ddp._buckets)
            assert ddp.segment_waits() is not None and len(ddp.segment_waits()) == len(plan)
            opt.step()
            after = opt_state(core, opt)
            no_grad = [e for e, _ in used(core) if e.name in without]
            for k in "pmvs":
                assert ranges_equal(after[k], before[k], no_grad) == [], k
            if dtype == torch.float32:          # the reference's payload: one step equals the plain frozen step
                for k in "pmvs":
                    assert torch.equal(after[k], plain[1][k]), k
            else:
                assert not torch.equal(after["p"], before["p"]) and bool(torch.isfinite(core.flat_params).all())
    finally:
        for core in cores:
            core._ddp = None
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------ check 10: fp8
def test_fp8_with_a_frozen_shadowed_weight_is_refused_before_the_step():
    cfg = C.tiny_config(hidden_size=128, intermediate_size=256, fixed_t_layer=1)
    model, params, core = build(cfg, base=dict(BASE, fp8=True))
    lib = L.load()
    lib.crct_prof_enable(2)
    lib.crct_prof_reset()
    try:
        with pytest.raises(NotImplementedError) as ei:
            step_forward(model, tiny_batch(cfg), params)
        launched = lib.crct_prof_stamp_count()
    finally:
        lib.crct_prof_enable(0)
        lib.crct_prof_reset()
    assert "fp8" in str(ei.value) and "bert.encoder.layer.0." in str(ei.value)
    assert launched == 0


# ------------------------------------------------------------------------------------------------ check 11: segment events
def test_segmented_backward_and_segment_events_on_a_frozen_model():
    cfg = case_cfg("B", False)
    batch = tiny_batch(cfg)
    free = unfrozen("B", False)
    # segment by segment (the data-parallel call pattern without the collectives)
    model, params, core = build(cfg)
    names = set(frozen_used(core, FIXTURE["B"]["grad_is_none"]))
    core.force_segmented = True
    same_grads(step(model, params, core, batch), free, names)
    # one call that records the four events of every segment, running or not
    model, params, core = build(cfg)
    core.record_segment_events = True
    got = step(model, params, core, batch)
    same_grads(got, free, names)
    evs = core.segment_done_events()
    assert len(evs) == 4 * core._engine.n_segments
    assert all(ev.query() for ev in evs)
    waits = core.take_segment_done_events()
    assert waits is not None and len(waits) == core._engine.n_segments
    # a second pass re-records them: nothing stale, nothing missing
    got = step(model, params, core, batch)
    same_grads(got, free, names)
    assert all(ev.query() for ev in core.segment_done_events())


# ------------------------------------------------------------------------------------------------ full depth
def test_full_depth_fixed_t_layer_6():
    """vilbert.json, B 2, V 36, T 20: the real word table and segment ranges.  One model: the unfrozen step first, then the same
    weights with ``fixed_t_layer = 6``."""
    cfg = C.vilbert_config()
    model, params, core = build(cfg, base=C.default_params(), seed=5)
    batch = S.make_batch(2, 20, 36, cfg.v_feature_size, seed=21)
    free = step(model, params, core, batch)
    launches_free = count_launches(core, model, params, batch, segmented=True)
    whole_free = count_launches(core, model, params, batch, segmented=False)[-1]
    cfg.fixed_t_layer = 6
    cfg.validate()
    names = [n for n in layout.frozen_names(cfg, params) if core._entries[n].used]
    assert len(names) == 7 + 6 * 16
    got = step(model, params, core, batch, sentinel=names)
    same_outputs(got, free)
    same_grads(got, free, set(names))
    assert sentinel_intact(core, names) == []
    plan = core._engine.backward_plan()
    sched = layout.encoder_schedule(cfg)
    idle = sorted(len(sched) - i for i, st in enumerate(sched) if st[0] == "t" and st[1] < 6)
    assert [i for i, p in enumerate(plan) if not p[0]] == idle and len(idle) == 6
    assert plan[-1][:3] == (True, False, True)
    whole_frozen = count_launches(core, model, params, batch, segmented=False)[-1]
    saved = sum(launches_free[i] for i in idle)
    print("launches: unfrozen %d, fixed_t_layer=6 %d, the six text segments hold %d" % (whole_free, whole_frozen, saved))
    assert whole_frozen <= whole_free - saved
    # the word table and six BERT layers: 66 M of the 238 M gradient elements are neither produced nor updated
    assert sum(core._entries[n].numel for n in names) > 60e6
