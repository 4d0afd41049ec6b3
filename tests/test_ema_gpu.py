"""FusedAdamW's weight average on the native step (-m gpu): enable_ema / ema_decay / swap_ema / the checkpoint entries.

Everything but the recurrence is a bit comparison: the average is an observer of the update (a run with it and a run without it have
the same losses, weights and moments in every launch mode), tensors no launch touches keep the weights they started from, and a
swap_ema() round trip leaves nothing behind.  The recurrence itself is held per element to the two-rounding budget of tests/ema_ref.py,
from the average before the step and the weights after it.

Shapes: the tiny config of the step tests at B 4, T 7, V 5; the fp8 runs use the smallest config the fp8 step runs at in this suite
(hidden 128 / 256, tests/golden/head128_small: B 3, T 130, V 9)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from crct import checkpoint as CK                  # noqa: E402
from crct import config as C                       # noqa: E402
from crct import synthetic as S                    # noqa: E402
from crct.model import VisualDialogEncoder         # noqa: E402
from crct.optim import WarmupLinearScheduleNonZero, get_optimizer   # noqa: E402
from crct.step_adapter import forward as step_forward   # noqa: E402
from helpers import GOLDEN, load_case              # noqa: E402
import ema_ref as E                                # noqa: E402

DEV = torch.device("cuda:0")
BASE = C.default_params(categories=9, L1=True)
INF = float("inf")


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def build(cfg, base=BASE, seed=7):
    params = dict(base, device=DEV)
    model = VisualDialogEncoder(params, config=cfg)
    core = model.bert_pretrained
    core.cls_dropout = 0.0
    S.seeded_fill_(model.state_dict(), base_seed=seed)
    core._invalidate_shadow()
    return model, params, core


def tiny_batch(cfg):
    return S.make_batch(4, 7, 5, cfg.v_feature_size, categories=9, vocab_size=cfg.vocab_size, seed=11)


def fp8_case():
    """The small fp8-capable config and its batch (every Linear a multiple of 64 wide: the update keeps the transposed shadow itself)."""
    z = np.load(os.path.join(GOLDEN, "head128_small_B3_V9_T130.npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    cfg = C.BertConfig.from_dict(meta["cfg"])
    batch = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in.")}
    batch["image_feat"] = batch["image_feat"].float()
    return cfg, dict(BASE, fp8=True), batch


def backward(model, params, core, batch, it, scaler=None):
    core._calls = it
    loss = step_forward(model, batch, params)[0]
    (loss if scaler is None else scaler.scale(loss)).backward()
    return loss.detach().clone()


def settle(opt):
    opt.synchronize()
    torch.cuda.synchronize()


def state(core, opt):
    settle(opt)
    return [bits(core.flat_params).clone(), bits(opt._m).clone(), bits(opt._v).clone()]


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def evaluate(model, params, batch):
    model.eval()
    try:
        with torch.no_grad():
            out = step_forward(model, batch, params, output_nsp_scores=True, evaluation=True)
    finally:
        model.train()
    return out[4].detach().float().clone(), out[5][0].detach().float().clone()


# ------------------------------------------------------------------------------------------------ the average is an observer
MODES = {"plain": {}, "overlap": dict(overlap=True), "overlap_groups": dict(overlap=True, launch_groups=3), "early": dict(overlap=True, early=True),
         "scaler": dict(scaler=True), "fuse_zero_grad": dict(overlap=True, fuse_zero_grad=True), "clip": dict(clip=True), "fp8": dict(fp8=True)}
HIGHER_LR = dict(lr=1e-3, image_lr=2e-3)


def run(mode, ema, steps=6, decay=0.9):
    """`steps` training steps in launch mode `mode`; returns (losses, state, per-step averages or None, the optimizer)."""
    kw = MODES[mode]
    if kw.get("fp8"):
        cfg, base, batch = fp8_case()
    else:
        cfg, base = C.tiny_config(), BASE
        batch = tiny_batch(cfg)
    model, params, core = build(cfg, dict(base, **HIGHER_LR))
    opt = get_optimizer(params, model)
    opt.overlap = bool(kw.get("overlap"))
    opt.launch_groups = kw.get("launch_groups", 0)
    opt.fuse_zero_grad = bool(kw.get("fuse_zero_grad"))
    if kw.get("early"):
        opt.set_early(True)
    if ema:
        opt.enable_ema(decay)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=10 ** 6) if kw.get("scaler") else None
    losses, avgs = [], []
    for it in range(steps):
        losses.append(bits(backward(model, params, core, batch, it, scaler).reshape(1)))
        if kw.get("clip"):
            opt.clip_grad_norm_(1e-3)                      # far below the norm of these gradients: every step is clipped
        if scaler is not None:
            if it == 2:
                core.flat_grads[5] = INF                   # the scaler skips this step, decided on the device
            scaler.step(opt)
            scaler.update()
        else:
            opt.step()
        opt.zero_grad()
        if ema:
            settle(opt)
            avgs.append(bits(opt._ema).clone())
    return losses, state(core, opt), avgs if ema else None, opt


@pytest.mark.parametrize("mode", list(MODES))
def test_average_on_against_off(mode):
    """Six steps with the average and six without: losses, weights and both moments bit-identical; the average moves on every real
    step and keeps every bit across the step a GradScaler skips."""
    l_off, s_off, _, _ = run(mode, ema=False)
    l_on, s_on, avgs, opt = run(mode, ema=True)
    assert all(torch.equal(a, b) for a, b in zip(l_off, l_on)), mode
    assert same(s_off, s_on), mode
    for it in range(1, len(avgs)):
        moved = not torch.equal(avgs[it], avgs[it - 1])
        assert moved == (not (mode == "scaler" and it == 2)), (mode, it)
    if mode == "scaler":
        assert int(opt._step_dev.item()) == 5
    assert bool(torch.isfinite(opt._ema).all())


# ------------------------------------------------------------------------------------------------ the recurrence
@pytest.mark.parametrize("mode", ["plain", "overlap"])
def test_recurrence_per_element(mode):
    """After every step: the average against ema_ref from the average before and the weights after, within the budget, over every
    tensor the optimizer updates; with a decay schedule on the host attribute (0.9, 0.999, 0.9999, 1.0 in turn)."""
    cfg = C.tiny_config()
    batch = tiny_batch(cfg)
    model, params, core = build(cfg, dict(BASE, **HIGHER_LR))
    opt = get_optimizer(params, model)
    opt.overlap = mode == "overlap"
    opt.enable_ema(0.5)
    upd = torch.zeros(core.flat_params.numel(), dtype=torch.bool)
    for e in opt._segs:
        upd[e.offset:e.offset + e.numel] = True
    worst = 0.0
    for it, decay in enumerate(E.DECAYS):
        opt.ema_decay = decay                               # read at every step()
        settle(opt)
        before = opt._ema.cpu()
        backward(model, params, core, batch, it)
        opt.step()
        opt.zero_grad()
        settle(opt)
        after, p_after = opt._ema.cpu(), core.flat_params.cpu()
        ref, budget = E.reference(before, p_after, E.weight(decay))
        worst = max(worst, E.assert_within(after[upd], ref[upd], budget[upd], "%s step %d decay %g" % (mode, it, decay)))
        assert torch.equal(bits(after[~upd]), bits(before[~upd]))
        if decay == 1.0:
            assert torch.equal(bits(after), bits(before))
        else:
            assert not torch.equal(after[upd], before[upd])
    print("recurrence (%s): worst |got - fp64| / budget %.3f" % (mode, worst))


# ------------------------------------------------------------------------------------------------ tensors no launch touches
def ranges_differ(a, b, entries):
    return [e.name for e in entries if not torch.equal(a[e.offset:e.offset + e.numel], b[e.offset:e.offset + e.numel])]


def train(model, params, core, opt, batch, steps):
    for it in range(steps):
        backward(model, params, core, batch, it)
        opt.step()
        opt.zero_grad()
    settle(opt)


def test_frozen_tensors_read_as_their_weights():
    """fixed_t_layer = 1 and one requires_grad_(False) tensor: after 4 steps their average is bit-identical to their weights (which never
    moved), as is the average of the tensors that receive no gradient at all; everything else trails its weights."""
    cfg = C.tiny_config(fixed_t_layer=1)
    batch = tiny_batch(cfg)
    model, params, core = build(cfg, dict(BASE, **HIGHER_LR))
    extra = "bert.encoder.layer.2.output.dense.weight"
    dict(core.named_parameters())[extra].requires_grad_(False)
    opt = get_optimizer(params, model)
    opt.enable_ema(0.9)
    p0 = bits(core.flat_params).clone()
    train(model, params, core, opt, batch, 4)
    without = core.tensors_without_grad
    assert extra in without and any(n.startswith("bert.encoder.layer.0.") for n in without)
    p, a = bits(core.flat_params), bits(opt._ema)
    still = [e for e in core.table if (not e.used) or e.name in without or e.name not in opt._group_of]
    moving = [e for e in core.table if e.used and e.name not in without and e.name in opt._group_of]
    assert still and moving
    assert ranges_differ(a, p, still) == [] and ranges_differ(p, p0, still) == []
    # ... and the rest trails its weights (all but the few tensors whose gradient is exactly zero, the key biases among them)
    assert len(ranges_differ(a, p, moving)) > len(moving) * 3 // 4


def test_an_optimizer_over_a_parameter_subset():
    """Only the head tensors are in the optimizer's groups: the average of every other tensor stays its weight, bit for bit."""
    from crct.optim import FusedAdamW
    cfg = C.tiny_config()
    batch = tiny_batch(cfg)
    model, params, core = build(cfg)
    heads = [(n, p) for n, p in core.named_parameters() if n.startswith(("bert.t_pooler.", "bert.v_pooler.", "cls.bi_seq_relationship.", "regressor."))]
    opt = FusedAdamW([{"params": [p], "lr": 1e-3, "weight_decay": 0.01} for _, p in heads], model, lr=1e-3)
    opt.enable_ema(0.9)
    assert not opt.covers_every_gradient()
    train(model, params, core, opt, batch, 4)
    p, a = bits(core.flat_params), bits(opt._ema)
    inside = [e for e in core.table if e.name in opt._group_of]
    outside = [e for e in core.table if e.name not in opt._group_of]
    assert inside and outside
    assert ranges_differ(a, p, outside) == []
    assert len(ranges_differ(a, p, inside)) > len(inside) // 2


def test_figureqa_without_areas_puts_the_average_back():
    """The FigureQA variant stepped without `areas`: areas_emp has no gradient, the update's blocks cover it all the same and its weights,
    moments, shadow AND average are put back behind the launch -- the average stays the weight, bit for bit."""
    z, meta, cfg, params, batch = load_case("variant_tiny_figureqa")
    B, V = batch["image_target"].shape
    g = torch.Generator().manual_seed(int(meta["feat_seed"]))
    batch["image_feat"] = torch.randn(B, V, cfg.v_feature_size, generator=g, dtype=torch.float32).half().float()
    model, params, core = build(cfg, dict(params, **HIGHER_LR), seed=meta["weight_seed"])
    opt = get_optimizer(params, model)
    opt.enable_ema(0.9)
    plain = {k: v for k, v in batch.items() if k != "areas"}
    assert core.optional_entries and opt._opt_blocks
    train(model, params, core, opt, plain, 4)
    p, a = bits(core.flat_params), bits(opt._ema)
    assert ranges_differ(a, p, core.optional_entries) == []
    loc = core._entries["bert.v_embeddings.new_loc_emb.weight"]
    assert ranges_differ(a, p, [loc]) == [loc.name]                       # everything else averages
    train(model, params, core, opt, batch, 1)                             # with areas the tensor trains and its average follows
    assert len(ranges_differ(bits(opt._ema), bits(core.flat_params), core.optional_entries)) == len(core.optional_entries)


# ------------------------------------------------------------------------------------------------ swap_ema
def shadows(core):
    out = [core.flat_shadow.view(torch.int16).clone()]
    st = core._fp8
    if st is not None:
        out += [st.q.clone(), st.qt.clone(), bits(st.weight.scale).clone(), bits(st.weight.amax).clone(), bits(st.act.scale).clone(),
                bits(st.act.amax).clone(), bits(st.grad.scale).clone(), bits(st.grad.amax).clone()]
    return out


@pytest.mark.parametrize("fp8", [False, True])
def test_swap_round_trip_and_evaluation(fp8):
    if fp8:
        cfg, base, batch = fp8_case()
    else:
        cfg, base = C.tiny_config(), BASE
        batch = tiny_batch(cfg)
    runs = {}
    for name in ("swapped", "twin"):
        model, params, core = build(cfg, dict(base, **HIGHER_LR))
        opt = get_optimizer(params, model)
        opt.overlap = True
        opt.enable_ema(0.9)
        for it in range(3):
            backward(model, params, core, batch, it)
            opt.step()
            opt.zero_grad()
        if name == "swapped":
            settle(opt)
            before = state(core, opt) + shadows(core) + [bits(opt._ema).clone()]
            want = opt.ema_state_dict()
            train_sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
            assert list(want.keys()) == list(train_sd.keys())
            assert "bert_pretrained.cls.predictions.decoder.weight" in want
            assert any(not torch.equal(want[k], train_sd[k]) for k in want)
            with opt.swap_ema():
                inside = model.state_dict()
                for k in want:
                    assert torch.equal(bits(inside[k]), bits(want[k])), k
                got = evaluate(model, params, batch)
                assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())
                if not fp8:
                    # the averaged weights in a model of their own: the same logits and regressed values, bit for bit.  (An fp8 model
                    # of its own calibrates its activation scales on its first pass, the swapped one keeps the training run's delayed
                    # ones: there the two evaluate alike, not bit for bit.)
                    fresh, fparams, fcore = build(cfg, base, seed=3)
                    fresh.load_state_dict(want)
                    ref = evaluate(fresh, fparams, batch)
                    assert torch.equal(bits(got[0]), bits(ref[0])) and torch.equal(bits(got[1]), bits(ref[1]))
                held = opt.ema_state_dict()                          # inside the context it still names the averaged weights
                assert all(torch.equal(held[k], want[k]) for k in want)
                with pytest.raises(RuntimeError, match="swap_ema"):
                    opt.step()
                with pytest.raises(RuntimeError, match="nest"):
                    with opt.swap_ema():
                        pass
            settle(opt)
            after = state(core, opt) + shadows(core) + [bits(opt._ema).clone()]
            assert len(before) == len(after)
            for i, (x, y) in enumerate(zip(before, after)):
                assert torch.equal(x, y), "buffer %d differs after the swap round trip" % i
            back = model.state_dict()
            assert all(torch.equal(bits(back[k]), bits(train_sd[k])) for k in train_sd)
        losses = []
        for it in range(3, 6):
            losses.append(bits(backward(model, params, core, batch, it).reshape(1)))
            opt.step()
            opt.zero_grad()
        runs[name] = (losses, state(core, opt) + shadows(core) + [bits(opt._ema).clone()])
    assert all(torch.equal(a, b) for a, b in zip(runs["swapped"][0], runs["twin"][0]))
    assert len(runs["swapped"][1]) == len(runs["twin"][1])
    for i, (x, y) in enumerate(zip(runs["swapped"][1], runs["twin"][1])):
        assert torch.equal(x, y), "buffer %d differs from the run that never swapped" % i


def test_swap_restores_on_an_exception_too():
    cfg = C.tiny_config()
    model, params, core = build(cfg)
    opt = get_optimizer(params, model)
    with pytest.raises(RuntimeError, match="enable_ema"):
        with opt.swap_ema():
            pass
    opt.enable_ema(0.9)
    train(model, params, core, opt, tiny_batch(cfg), 2)
    p0, a0 = bits(core.flat_params).clone(), bits(opt._ema).clone()
    with pytest.raises(ZeroDivisionError):
        with opt.swap_ema():
            assert torch.equal(bits(core.flat_params), a0) and torch.equal(bits(opt._ema), p0)
            1 / 0
    assert torch.equal(bits(core.flat_params), p0) and torch.equal(bits(opt._ema), a0)
    opt.step()                                                            # usable again


# ------------------------------------------------------------------------------------------------ checkpoints
def test_checkpoints_carry_the_average(tmp_path):
    cfg = C.tiny_config()
    batch = tiny_batch(cfg)
    base = dict(BASE, warmup=4, min_lr=1.3e-5, **HIGHER_LR)
    model, params, core = build(cfg, base)
    opt = get_optimizer(params, model)
    sched = WarmupLinearScheduleNonZero(opt, warmup_steps=4, t_total=10, min_lr=1.3e-5)
    off = CK.checkpoint_dict(model, opt, sched, 0)
    assert list(off.keys()) == ["model_state_dict", "scheduler_state_dict", "optimizer_state_dict", "iter_id"]      # the reference's keys
    opt.enable_ema(0.9)
    train(model, params, core, opt, batch, 3)
    path = CK.save_checkpoint(str(tmp_path), model, opt, sched, epoch=0, step_iter_id=2)
    back = torch.load(path, map_location="cpu", weights_only=False)
    assert list(back["ema_state_dict"].keys()) == list(back["model_state_dict"].keys())
    assert all(v.device.type == "cpu" and v.untyped_storage().nbytes() == v.numel() * 4 for v in back["ema_state_dict"].values())
    assert back["optimizer_state_dict"].keys() == off["optimizer_state_dict"].keys()
    # a new model and optimizer with the average enabled: resume restores it bit for bit
    model2, params2, core2 = build(cfg, base, seed=3)
    opt2 = get_optimizer(params2, model2)
    opt2.enable_ema(0.9)
    CK.resume(model2, opt2, path, params2, 1)
    settle(opt2)
    assert torch.equal(bits(opt2._ema), bits(opt._ema))
    assert torch.equal(bits(core2.flat_params), bits(core.flat_params))
    # ... and without it the entry is ignored
    model3, params3, core3 = build(cfg, base, seed=3)
    opt3 = get_optimizer(params3, model3)
    CK.resume(model3, opt3, path, params3, 1)
    assert not opt3.ema_enabled
    # the deployment path: the averaged weights into a bare encoder
    model4, params4, core4 = build(cfg, base, seed=4)
    n = CK.load_model_weights(model4, path, use_ema=True)
    assert n == len(back["ema_state_dict"])
    assert torch.equal(bits(core4.flat_params), bits(opt._ema))
    assert CK.load_model_weights(model4, path) == n and torch.equal(bits(core4.flat_params), bits(core.flat_params))
    opt.disable_ema()
    path_off = CK.save_checkpoint(str(tmp_path / "off"), model, opt, sched, epoch=0, step_iter_id=2)
    assert "ema_state_dict" not in torch.load(path_off, map_location="cpu", weights_only=False)
    with pytest.raises(KeyError, match="ema_state_dict"):
        CK.load_model_weights(model4, path_off, use_ema=True)


# ------------------------------------------------------------------------------------------------ other surface
def test_enable_after_some_steps_reset_and_disable():
    cfg = C.tiny_config()
    batch = tiny_batch(cfg)
    model, params, core = build(cfg, dict(BASE, **HIGHER_LR))
    opt = get_optimizer(params, model)
    opt.overlap = True
    with pytest.raises(RuntimeError, match="enable_ema"):
        opt.ema_state_dict()
    train(model, params, core, opt, batch, 2)
    torch.cuda.synchronize()
    base_mem = torch.cuda.memory_allocated()
    opt.enable_ema(0.99)
    assert opt.ema_enabled and opt.ema_decay == 0.99
    assert torch.cuda.memory_allocated() - base_mem >= 4 * core.flat_params.numel()
    settle(opt)
    assert torch.equal(bits(opt._ema), bits(core.flat_params))            # starts from the CURRENT weights, the overlapped update included
    train(model, params, core, opt, batch, 1)
    assert not torch.equal(bits(opt._ema), bits(core.flat_params))
    # load_state_dict on the model, then ema_reset(): the average is the loaded weights
    sd = {k: v.detach().clone() + 0.25 for k, v in model.state_dict().items()}
    model.load_state_dict(sd)
    opt.ema_reset()
    assert torch.equal(bits(opt._ema), bits(core.flat_params))
    # load_ema_state_dict is the reverse of ema_state_dict, by key intersection
    want = {k: v + 1.0 for k, v in opt.ema_state_dict().items()}
    some = dict(list(want.items())[:5], not_a_key=torch.zeros(1))
    assert opt.load_ema_state_dict(some) == 5
    got = opt.ema_state_dict()
    assert all(torch.equal(got[k], want[k]) for k in list(want)[:5]) and not torch.equal(got[list(want)[7]], want[list(want)[7]])
    del sd, want, some, got
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    opt.disable_ema()
    assert not opt.ema_enabled
    torch.cuda.synchronize()
    assert held - torch.cuda.memory_allocated() >= 4 * core.flat_params.numel()          # the buffer is returned
    train(model, params, core, opt, batch, 1)                             # ... and training goes on without it
