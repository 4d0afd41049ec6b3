"""params['img_loss_coeff']: the masked-region loss of the training step (-m gpu).  The tiny config (Hv = 96, C = v_target_size = 17), B 4,
V 9, image_label 1 on a few regions, 0 on the <IMG> row, -1 elsewhere, one sample without a labelled region.

Option off (these pass without the feature too): slot 1 is the cached zero, the six head tensors have no gradient, the segments are the
schedule's.  Option on: loss, the six head gradients and d sequence_output_v against tests/region_head_ref.py computed from the step's OWN
sequence_output_v and weights, within its budget, for hard and soft targets; the adapter's loss, alone and next to the masked-LM term;
no labelled region; refusals before any launch; image_class; accumulation; GradScaler; a frozen head tensor; a requested input gradient;
the fused optimizer, plain and overlapped, and its gradient norm; the data-parallel wrapper at world size 1; torch.no_grad(); a FigureQA
model and an fp8 one.

Measured on MI355X, the worst |error| / budget over the eight outputs (budget = region_head_ref.budget, nothing fitted; every test prints
its own line): hard 0.56 (dense.weight), soft 0.48 (d_seq), FigureQA 0.64 (decoder.weight), fp8 0.56; the loss itself 0.02 .. 0.10.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import lm_head_ref as LR                           # noqa: E402
import region_head_ref as R                        # noqa: E402
from crct import config as C                       # noqa: E402
from crct import synthetic as S                    # noqa: E402
from crct.layout import encoder_schedule           # noqa: E402
from crct.step_adapter import forward as step_forward   # noqa: E402
from helpers import ATOMIC_GRADS                   # noqa: E402
from test_step_gpu import build_model              # noqa: E402

DEV = torch.device("cuda:0")
COEFF = 0.5                                        # a power of two: coeff * gradient is exact in every format
P = "cls.imagePredictions."
HEAD = (P + "decoder.bias", P + "transform.dense.weight", P + "transform.dense.bias", P + "transform.LayerNorm.weight",
        P + "transform.LayerNorm.bias", P + "decoder.weight")
REF_KEY = dict(zip(HEAD, ("decoder.bias", "dense.weight", "dense.bias", "LayerNorm.weight", "LayerNorm.bias", "decoder.weight")))
LM_HEAD = ("cls.predictions.bias", "cls.predictions.transform.dense.weight", "cls.predictions.transform.dense.bias",
           "cls.predictions.transform.LayerNorm.weight", "cls.predictions.transform.LayerNorm.bias")
B, T, NV, NC = 4, 12, 9, 17


def label_regions(batch, soft=False, seed=3):
    """image_label as the loader writes it (1 = masked region with zeroed features, 0 = the <IMG> row, -1 elsewhere) and the true classes in
    batch['image_class'] (int64 [B, V], or float [B, V, C] with zeros); the unlabelled rows carry values that must never be looked at."""
    g = torch.Generator().manual_seed(seed)
    label = torch.full((B, NV), -1, dtype=torch.int64)
    label[:, 0] = 0
    pick = torch.rand(B, NV, generator=g) < 0.35
    pick[:, 0] = False
    pick[2] = False                                                 # one sample without a labelled region
    pick[0, 1] = pick[0, 2] = pick[1, 3] = pick[3, 4] = True
    label[pick] = 1
    feat = batch["image_feat"].clone()
    feat[pick] = 0.0
    batch = dict(batch, image_label=label, image_feat=feat)
    if soft:
        t = torch.rand(B, NV, NC, generator=g)
        t[torch.rand(B, NV, NC, generator=g) < 0.3] = 0.0
        t[..., 0] += 1e-3
        t = t / t.sum(-1, keepdim=True)
        t[0, 1] *= 0.5
        t[~pick] = -1.0                                             # unlabelled rows: never validated, never read into a result
        batch["image_class"] = t.float()
    else:
        ids = torch.randint(0, NC, (B, NV), generator=g)
        ids[0, 1], ids[0, 2], ids[1, 3], ids[3, 4] = 0, NC - 1, 7, 7
        ids[~pick] = 10 ** 6
        batch["image_class"] = ids
    return batch


def make(coeff=COEFF, soft=False, label=True, lm=None, params_over=None, **cfg_over):
    cfg = C.tiny_config(**cfg_over)
    assert cfg.v_hidden_size == 96 and (cfg.v_target_size == NC or "v_target_size" in cfg_over)
    extra = {} if coeff == "absent" else dict(img_loss_coeff=coeff)
    if lm is not None:
        extra["lm_loss_coeff"] = lm
    model, params = build_model(cfg, C.default_params(categories=9, L1=True, **dict(extra, **(params_over or {}))), weights=None, seed=7)
    model.train()
    batch = S.make_batch(B, T, NV, cfg.v_feature_size, categories=9, vocab_size=cfg.vocab_size, seed=11)
    if label:
        batch = label_regions(batch, soft)
    if lm is not None:
        g = torch.Generator().manual_seed(5)
        mask = torch.where(torch.rand(B, T, generator=g) < 0.25, torch.randint(0, cfg.vocab_size, (B, T), generator=g), torch.full((B, T), -1))
        mask[0, 1] = 3
        batch["mask"] = mask
    return cfg, model, params, model.bert_pretrained, batch


def grads(core, names=None):
    byname = dict(core.named_parameters())
    return {n: (None if byname[n].grad is None else byname[n].grad.detach().clone()) for n in (names or [e.name for e in core.table if e.used])}


def head_weights(core):
    p = {n: v.detach().double().cpu() for n, v in core.named_parameters() if n in HEAD}
    return dict(d=p[HEAD[0]], W=p[HEAD[1]], b=p[HEAD[2]], gamma=p[HEAD[3]], beta=p[HEAD[4]], D=p[HEAD[5]])


def ref_args(core, cfg, batch):
    x = core.sequence_output_v.detach().double().cpu().reshape(-1, cfg.v_hidden_size)
    tg = batch["image_class"]
    return head_weights(core), x, batch["image_label"].reshape(-1), tg.reshape(-1, NC).double() if torch.is_floating_point(tg) else tg.reshape(-1)


def check_head(core, cfg, batch, img, seq_grad, g=1.0, tag=""):
    """img_loss, the six head gradients and d sequence_output_v of ``g * img_loss`` within region_head_ref.budget of the fp64 reference."""
    args = ref_args(core, cfg, batch)
    ref, bud = R.reference(*args, g=g), R.budget(*args, g=g)
    got = {REF_KEY[n]: v.double().cpu() for n, v in grads(core, HEAD).items()}
    got["loss"], got["d_seq"] = img.detach().double().cpu().reshape(1), seq_grad.double().cpu().reshape(-1, cfg.v_hidden_size)
    worst = {k: float(((v - ref[k]).abs() / bud[k]).max()) for k, v in got.items()}
    print("%s worst |error| / budget:" % tag, {k: round(v, 3) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst
    off = (args[2] != 1).nonzero().flatten()
    assert float(got["d_seq"][off].abs().max()) == 0.0              # rows without label 1 get exactly nothing
    assert float(ref["d_seq"].abs().max()) > 0.0 and all(float(got[k].abs().max()) > 0.0 for k in got)


# ------------------------------------------------------------------------------------------------ option off
@pytest.mark.parametrize("coeff", ["absent", None, 0.0])
def test_option_off_is_the_stub(coeff):
    cfg, model, params, core, batch = make(coeff)
    out = step_forward(model, batch, params)
    assert out[3] is core._const_zeros[1] and float(out[3]) == 0.0 and tuple(out[3].shape) == (1, 1) and not out[3].requires_grad
    assert torch.equal(out[0], core.last_loss)
    out[0].backward()
    torch.cuda.synchronize()
    byname = dict(core.named_parameters())
    assert all(byname[n].grad is None for n in HEAD)
    assert core._engine.n_segments == len(encoder_schedule(cfg)) + 2
    assert all(not e.used for e in core.table if e.name in HEAD)
    # ... and the bits of a model that has never heard of the option, with the labels and image_class in the batch
    _, model0, params0, core0, _ = make("absent")
    out0 = step_forward(model0, {k: v for k, v in batch.items() if k != "image_class"}, params0)
    out0[0].backward()
    torch.cuda.synchronize()
    assert torch.equal(out0[0], out[0])
    for e in core.table:
        if e.used and e.name not in ATOMIC_GRADS:
            assert torch.equal(core.flat_grads[e.offset:e.offset + e.numel].view(torch.int32), core0.flat_grads[e.offset:e.offset + e.numel].view(torch.int32)), e.name


# ------------------------------------------------------------------------------------------------ option on
@pytest.mark.parametrize("soft", (False, True))
def test_loss_and_gradients_against_the_reference_from_the_steps_own_states(soft):
    cfg, model, params, core, batch = make(soft=soft)
    core.return_sequence_outputs = True
    out = step_forward(model, batch, params)
    img = out[3]
    assert tuple(img.shape) == (1, 1) and img.dtype == torch.float32 and float(img) > 0.0 and img.requires_grad
    assert core._engine.n_segments == len(encoder_schedule(cfg)) + 3
    lo, hi = core._engine.segments[0]
    assert sorted(e.name for e in core.table if e.used and lo <= e.offset < hi) == sorted(HEAD)
    assert torch.equal(out[0], core.last_loss + COEFF * img.sum())                      # the adapter's loss = fused + coeff * img_loss
    assert out[1] is core._const_zeros[0]                                               # the LM stub is untouched
    seq = core.sequence_output_v
    seq.retain_grad()
    core.zero_flat_grads()
    img.sum().backward()                                                                # the region term alone: g = 1
    torch.cuda.synchronize()
    check_head(core, cfg, batch, img, seq.grad, tag="soft" if soft else "hard")


def test_both_heads_together_each_within_its_budget():
    cfg, model, params, core, batch = make(lm=0.25)
    core.return_sequence_outputs = True
    out = step_forward(model, batch, params)
    lm, img = out[1], out[3]
    assert float(lm) > 0.0 and float(img) > 0.0
    assert torch.equal(out[0], (core.last_loss + 0.25 * lm.sum()) + COEFF * img.sum())
    assert core._engine.n_segments == len(encoder_schedule(cfg)) + 3                    # ONE segment for both heads
    lo, hi = core._engine.segments[0]
    assert sorted(e.name for e in core.table if e.used and lo <= e.offset < hi) == sorted(HEAD + LM_HEAD)
    seq_t, seq_v = core.sequence_output_t, core.sequence_output_v
    seq_t.retain_grad(), seq_v.retain_grad()
    core.zero_flat_grads()
    (lm.sum() + img.sum()).backward()
    torch.cuda.synchronize()
    check_head(core, cfg, batch, img, seq_v.grad, tag="region next to LM")
    p = {n: v.detach().double().cpu() for n, v in core.named_parameters()}
    w = dict(E=p["bert.embeddings.word_embeddings.weight"], bias=p[LM_HEAD[0]], W=p[LM_HEAD[1]], b=p[LM_HEAD[2]], gamma=p[LM_HEAD[3]], beta=p[LM_HEAD[4]])
    x = seq_t.detach().double().cpu().reshape(-1, cfg.hidden_size)
    ref, bud = LR.reference(w, x, batch["mask"].reshape(-1)), LR.budget(w, x, batch["mask"].reshape(-1))
    got = dict(zip(("bias", "dense.weight", "dense.bias", "LayerNorm.weight", "LayerNorm.bias"), (v.double().cpu() for v in grads(core, LM_HEAD).values())))
    got["loss"], got["d_seq"] = lm.detach().double().cpu().reshape(1), seq_t.grad.double().cpu().reshape(-1, cfg.hidden_size)
    worst = {k: float(((v - ref[k]).abs() / bud[k]).max()) for k, v in got.items()}
    print("LM next to region worst |error| / budget:", {k: round(v, 3) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst


def test_no_labelled_region_is_the_constant_zero():
    cfg, model, params, core, batch = make()
    batch = dict(batch, image_label=torch.where(batch["image_label"] == 1, torch.full_like(batch["image_label"], -1), batch["image_label"]))
    out = step_forward(model, batch, params)
    assert out[3] is core._const_zeros[1] and float(out[3]) == 0.0 and not out[3].requires_grad
    assert torch.equal(out[0], core.last_loss)
    core.zero_flat_grads()
    out[0].backward()
    torch.cuda.synchronize()
    assert all(float(g.abs().max()) == 0.0 for g in grads(core, HEAD).values())
    assert torch.isfinite(out[0]).all()


def test_bad_targets_are_refused_before_any_launch_and_only_on_labelled_rows():
    cfg, model, params, core, batch = make()
    calls = core._calls
    for bad in (NC, -1):
        b = dict(batch, image_class=batch["image_class"].clone())
        b["image_class"][0, 1] = bad
        with pytest.raises(ValueError, match=r"image_class: %d .*v_target_size = %d" % (bad, NC)):
            step_forward(model, b, params)
    b = {k: v for k, v in batch.items() if k != "image_class"}
    b["image_target"] = batch["image_target"].clone()
    b["image_target"][0, 1] = NC + 3                                                    # the default source names itself
    with pytest.raises(ValueError, match=r"image_target: %d " % (NC + 3)):
        step_forward(model, b, params)
    _, model_s, params_s, core_s, batch_s = make(soft=True)
    for bad in (-0.25, float("nan"), float("inf")):
        b = dict(batch_s, image_class=batch_s["image_class"].clone())
        b["image_class"][1, 3, 5] = bad
        with pytest.raises(ValueError, match="image_class.*negative or not finite"):
            step_forward(model_s, b, params_s)
    assert core._calls == calls and core_s._calls == 0                                  # no forward was started
    # the same values on rows without label 1 are what label_regions put there: accepted
    assert int(batch["image_class"].max()) == 10 ** 6 and float(batch_s["image_class"].min()) == -1.0
    assert float(step_forward(model, batch, params)[3]) > 0.0 and float(step_forward(model_s, batch_s, params_s)[3]) > 0.0
    with pytest.raises(NotImplementedError, match="2048"):
        make(v_target_size=4096)
    make("absent", v_target_size=4096)                                                  # without the option the size is nobody's business
    model.eval()
    ev = step_forward(model, batch, params, evaluation=True)                            # the inference branch is untouched
    assert ev[0] is None and ev[3] is None


def test_image_class_overrides_image_target_for_the_loss_only():
    cfg, model, params, core, batch = make()
    core.return_sequence_outputs = True
    plain = {k: v for k, v in batch.items() if k != "image_class"}                      # image_target (all 8 here) is the default target
    core._calls = 0
    a = step_forward(model, plain, params)
    seq_a = (core.sequence_output_t.clone(), core.sequence_output_v.clone())
    core._calls = 0
    b = step_forward(model, batch, params)
    assert torch.equal(seq_a[0], core.sequence_output_t) and torch.equal(seq_a[1], core.sequence_output_v)     # the forward states: bit-identical
    assert torch.equal(a[2], b[2])                                                      # ... and the answer loss with them
    assert float(a[3]) > 0.0 and float(b[3]) > 0.0 and not torch.equal(a[3], b[3])
    core._calls = 0
    c = step_forward(model, dict(plain, image_class=batch["image_target"]), params)     # the same ids by the other door: the same bits
    assert torch.equal(a[3], c[3])
    core._calls = 0
    d = step_forward(model, dict(batch, image_label=batch["image_label"].to(DEV), image_class=batch["image_class"].to(DEV)), params)
    assert torch.equal(b[3], d[3])                                                      # device tensors cost a copy, not an error


def one_step_grads(model, params, core, batch, passes=1, scaler=None):
    core.zero_flat_grads()
    for _ in range(passes):
        core._calls = 0
        loss = step_forward(model, batch, params)[0]
        (loss if scaler is None else scaler.scale(loss)).backward()
    torch.cuda.synchronize()
    return grads(core)


@pytest.mark.parametrize("soft", (False, True))
def test_accumulation_and_grad_scaler_are_exact(soft):
    cfg, model, params, core, batch = make(soft=soft)
    one = one_step_grads(model, params, core, batch)
    two = one_step_grads(model, params, core, batch, passes=2)
    scaled = one_step_grads(model, params, core, batch, scaler=torch.amp.GradScaler("cuda", init_scale=1024.0))
    assert all(float(one[n].abs().max()) > 0.0 for n in HEAD)
    for n in HEAD:                                                                      # the region path alone: powers of two all the way
        assert torch.equal(scaled[n], 1024.0 * one[n]), n
    for n, g in one.items():
        if n not in ATOMIC_GRADS:
            assert torch.equal(two[n], 2.0 * g), n


def test_a_frozen_decoder_weight_drops_that_product_only():
    cfg, model, params, core, batch = make()
    full = one_step_grads(model, params, core, batch)
    byname = dict(core.named_parameters())
    byname[HEAD[5]].requires_grad_(False)
    got = one_step_grads(model, params, core, batch)
    assert byname[HEAD[5]].grad is None and HEAD[5] in core.tensors_without_grad
    for n, g in full.items():
        if n != HEAD[5] and n not in ATOMIC_GRADS:
            assert torch.equal(got[n].view(torch.int32), g.view(torch.int32)), n


def test_requested_input_gradient_sees_the_region_term():
    seen = []
    for coeff in ("absent", COEFF):
        cfg, model, params, core, batch = make(coeff)
        b = dict(batch, image_feat=batch["image_feat"].to(DEV).requires_grad_(True))
        step_forward(model, b, params)[0].backward()
        torch.cuda.synchronize()
        seen.append(b["image_feat"].grad.clone())
    assert torch.isfinite(seen[1]).all() and not torch.equal(seen[0], seen[1])


def trained_weights(overlap=False, wrap=False, steps=2, clip=False):
    from crct.optim import get_optimizer
    cfg, model, params, core, batch = make()
    opt = get_optimizer(dict(params, lr=1e-3, image_lr=2e-3), model)
    opt.overlap = overlap
    runner = model
    if wrap:
        from crct.ddp import FlatGradDDP
        runner = FlatGradDDP(model, device_ids=[0], find_unused_parameters=True)
    start = core.flat_params.clone()
    norms = None
    for _ in range(steps):
        step_forward(runner, batch, params)[0].backward()
        if clip:
            total = opt.clip_grad_norm_(1e9)
            norms = (float(total), dict(zip(opt.grad_norm_names, opt.grad_norms().double().cpu().tolist())), grads(core, HEAD))
        opt.step()
        opt.zero_grad()
    if overlap:
        opt.synchronize()
    torch.cuda.synchronize()
    return core, start, core.flat_params.clone(), opt, norms


def test_fused_adamw_moves_the_head_at_image_lr_and_overlap_changes_no_bit():
    core, start, plain, opt, _ = trained_weights()
    for e in core.table:
        if e.name in HEAD:
            assert not torch.equal(start[e.offset:e.offset + e.numel], plain[e.offset:e.offset + e.numel]), e.name
            assert opt.param_groups[opt._group_of[e.name]]["lr"] == 2e-3 and not e.language, e.name
    _, _, over, opt, _ = trained_weights(overlap=True)
    for e in core.table:
        if e.used and e.name not in ATOMIC_GRADS:
            assert torch.equal(plain[e.offset:e.offset + e.numel].view(torch.int32), over[e.offset:e.offset + e.numel].view(torch.int32)), e.name
    with pytest.raises(RuntimeError, match="img_loss_coeff"):
        opt.set_early(True)


def test_clip_grad_norm_counts_the_head():
    core, _, _, opt, (total, per, head_grads) = trained_weights(steps=1, clip=True)
    for n in HEAD:
        want = float(head_grads[n].double().pow(2).sum().sqrt())
        assert n in per and want > 0.0 and abs(per[n] - want) <= 1e-5 * want, n
    assert total ** 2 >= sum(per[n] ** 2 for n in HEAD) * (1.0 - 1e-5)


def test_data_parallel_wrapper_at_world_size_one():
    import torch.distributed as dist
    _, _, plain, _, _ = trained_weights(steps=1)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29573")
    torch.cuda.set_device(0)
    dist.init_process_group(backend="nccl", rank=0, world_size=1, device_id=DEV)
    try:
        core, _, wrapped, _, _ = trained_weights(wrap=True, steps=1)
    finally:
        dist.destroy_process_group()
    for e in core.table:
        if e.used and e.name not in ATOMIC_GRADS:
            assert torch.equal(plain[e.offset:e.offset + e.numel].view(torch.int32), wrapped[e.offset:e.offset + e.numel].view(torch.int32)), e.name


@pytest.mark.parametrize("soft", (False, True))
def test_no_grad_in_the_training_branch_gives_the_same_bits_forward_only(soft):
    cfg, model, params, core, batch = make(soft=soft)
    core._calls = 0
    with_grad = step_forward(model, batch, params)[3]
    core._calls = 0
    with torch.no_grad():
        out = step_forward(model, batch, params)
    assert not out[3].requires_grad and torch.equal(out[3], with_grad.detach())


def test_figure_qa_model_meets_the_budgets():
    from test_variants_gpu import load_variant, variant_model
    z, meta, cfg, params, batch = load_variant("variant_tiny_figureqa")
    for k in ("hidden_dropout_prob", "attention_probs_dropout_prob", "v_hidden_dropout_prob", "v_attention_probs_dropout_prob"):
        setattr(cfg, k, 0.0)
    model, params = variant_model(meta, cfg, dict(params, img_loss_coeff=COEFF))
    model.train()
    core = model.bert_pretrained
    assert core.variant[0] == "figure_qa" and cfg.v_target_size == NC
    Bv, Vv = batch["image_feat"].shape[:2]
    g = torch.Generator().manual_seed(9)
    label = torch.full((Bv, Vv), -1, dtype=torch.int64)
    label[:, 0] = 0
    label[:, 1:][torch.rand(Bv, Vv - 1, generator=g) < 0.4] = 1
    label[0, 1] = 1
    batch = dict(batch, image_label=label, image_class=torch.randint(0, NC, (Bv, Vv), generator=g))
    core.return_sequence_outputs = True
    out = step_forward(model, batch, params)
    seq = core.sequence_output_v
    seq.retain_grad()
    core.zero_flat_grads()
    out[3].sum().backward()
    torch.cuda.synchronize()
    check_head(core, cfg, batch, out[3], seq.grad, tag="figure_qa")


def test_fp8_model_runs_the_head_in_bf16_within_the_budgets():
    cfg, model, params, core, batch = make(params_over=dict(fp8=True))
    assert core.fp8
    core.return_sequence_outputs = True
    out = step_forward(model, batch, params)
    seq = core.sequence_output_v
    seq.retain_grad()
    core.zero_flat_grads()
    out[3].sum().backward()
    torch.cuda.synchronize()
    check_head(core, cfg, batch, out[3], seq.grad, tag="fp8")
