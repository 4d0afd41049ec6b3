"""params['lm_loss_coeff']: the masked-LM loss of the training step (-m gpu).  The tiny config with vocab_size = 130 (a tail of 2 past a
multiple of 64), B 4, T 12, labels on about a quarter of the tokens and one sample with none.

Option off (these pass without the feature too): slot 0 is the cached zero, the five head tensors have no gradient, the segments are
the schedule's.  Option on: loss and gradients against tests/lm_head_ref.py computed from the step's OWN sequence_output_t and weights,
within its budget; the tied word table; the adapter's loss; no labels; accumulation; GradScaler; frozen text layers; a requested input
gradient; the fused optimizer, plain and overlapped; the data-parallel wrapper at world size 1.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import lm_head_ref as R                            # noqa: E402
from crct import config as C                       # noqa: E402
from crct import synthetic as S                    # noqa: E402
from crct.layout import encoder_schedule           # noqa: E402
from crct.step_adapter import forward as step_forward   # noqa: E402
from helpers import ATOMIC_GRADS                   # noqa: E402
from test_step_gpu import build_model              # noqa: E402

DEV = torch.device("cuda:0")
COEFF = 0.5                                        # a power of two: coeff * gradient is exact in every format
HEAD = ("cls.predictions.bias", "cls.predictions.transform.dense.weight", "cls.predictions.transform.dense.bias",
        "cls.predictions.transform.LayerNorm.weight", "cls.predictions.transform.LayerNorm.bias")
WORD = "bert.embeddings.word_embeddings.weight"
REF_KEY = dict(zip(HEAD, ("bias", "dense.weight", "dense.bias", "LayerNorm.weight", "LayerNorm.bias")))
B, T, NV, VOCAB = 4, 12, 5, 130


def make(coeff=COEFF, labels=True, **cfg_over):
    cfg = C.tiny_config(vocab_size=VOCAB, **cfg_over)
    extra = {} if coeff is None else dict(lm_loss_coeff=coeff)
    model, params = build_model(cfg, C.default_params(categories=9, L1=True, **extra), weights=None, seed=7)
    model.train()
    batch = S.make_batch(B, T, NV, cfg.v_feature_size, categories=9, vocab_size=VOCAB, seed=11)
    if labels:
        g = torch.Generator().manual_seed(3)
        mask = torch.where(torch.rand(B, T, generator=g) < 0.25, torch.randint(0, VOCAB, (B, T), generator=g), torch.full((B, T), -1))
        mask[2] = -1                                                # one sample without a label
        mask[0, 1], mask[0, 2], mask[1, 3], mask[3, 4] = 0, VOCAB - 1, 7, 7
        batch["mask"] = mask
    return cfg, model, params, model.bert_pretrained, batch


def grads(core, names=None):
    byname = dict(core.named_parameters())
    return {n: (None if byname[n].grad is None else byname[n].grad.detach().clone()) for n in (names or [e.name for e in core.table if e.used])}


def head_weights(core):
    p = {n: v.detach().double().cpu() for n, v in core.named_parameters() if n in HEAD or n == WORD}
    return dict(E=p[WORD], bias=p[HEAD[0]], W=p[HEAD[1]], b=p[HEAD[2]], gamma=p[HEAD[3]], beta=p[HEAD[4]])


# ------------------------------------------------------------------------------------------------ option off
@pytest.mark.parametrize("coeff", [None, 0.0])
def test_option_off_is_the_stub(coeff):
    cfg, model, params, core, batch = make(coeff)
    out = step_forward(model, batch, params)
    assert out[1] is core._const_zeros[0] and float(out[1]) == 0.0 and tuple(out[1].shape) == (1, 1) and not out[1].requires_grad
    out[0].backward()
    torch.cuda.synchronize()
    byname = dict(core.named_parameters())
    assert all(byname[n].grad is None for n in HEAD)
    assert core._engine.n_segments == len(encoder_schedule(cfg)) + 2
    assert all(not e.used for e in core.table if e.name in HEAD)


# ------------------------------------------------------------------------------------------------ option on
def test_loss_and_gradients_against_the_reference_from_the_steps_own_states():
    cfg, model, params, core, batch = make()
    core.return_sequence_outputs = True
    out = step_forward(model, batch, params)
    lm = out[1]
    assert tuple(lm.shape) == (1, 1) and lm.dtype == torch.float32 and float(lm) > 0.0 and lm.requires_grad
    assert core._engine.n_segments == len(encoder_schedule(cfg)) + 3
    lo, hi = core._engine.segments[0]
    assert sorted(e.name for e in core.table if e.used and lo <= e.offset < hi) == sorted(HEAD)
    assert torch.equal(out[0], core.last_loss + COEFF * lm.sum())                       # the adapter's loss = fused + coeff * lm_loss
    seq = core.sequence_output_t
    seq.retain_grad()
    core.zero_flat_grads()
    lm.sum().backward()                                                                 # the LM term alone: g = 1
    torch.cuda.synchronize()
    w = head_weights(core)
    labels = batch["mask"].reshape(-1)
    x = seq.detach().double().cpu().reshape(-1, cfg.hidden_size)
    ref, bud = R.reference(w, x, labels), R.budget(w, x, labels)
    got = {REF_KEY[n]: v.double().cpu() for n, v in grads(core, HEAD).items()}
    got["loss"], got["d_seq"] = lm.detach().double().cpu().reshape(1), seq.grad.double().cpu().reshape(-1, cfg.hidden_size)
    worst = {}
    for k, v in got.items():
        worst[k] = float(((v - ref[k]).abs() / bud[k]).max())
    print("worst |error| / budget:", {k: round(v, 3) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst
    nz = (labels < 0).nonzero().flatten()
    assert float(got["d_seq"][nz].abs().max()) == 0.0                                   # rows without a label get exactly nothing


def test_word_table_gradient_is_embedding_term_plus_decoder_term():
    cfg, model, params, core, batch = make()
    core.return_sequence_outputs = True
    out = step_forward(model, batch, params)
    seq = core.sequence_output_t
    seq.retain_grad()
    core.zero_flat_grads()
    out[0].backward()                                                                   # fused + COEFF * lm_loss
    torch.cuda.synchronize()
    word_on, d_seq = grads(core, [WORD])[WORD].double().cpu(), seq.grad.detach().clone()
    w, labels = head_weights(core), batch["mask"].reshape(-1)
    x = seq.detach().double().cpu().reshape(-1, cfg.hidden_size)
    ref, bud = R.reference(w, x, labels, g=COEFF), R.budget(w, x, labels, g=COEFF)
    # the same upstream on sequence_output_t into a model without the option: the embedding term alone (seq.grad above holds only the
    # LM head's share: the engine adds its own hidden gradient inside)
    _, model0, params0, core0, _ = make(None)
    core0.return_sequence_outputs = True
    out0 = step_forward(model0, batch, params0)
    assert torch.equal(core0.sequence_output_t, seq.detach())
    core0.zero_flat_grads()
    (out0[0] + (d_seq * core0.sequence_output_t).sum()).backward()
    torch.cuda.synchronize()
    word_off = grads(core0, [WORD])[WORD].double().cpu()
    err = (word_on - word_off - ref["decoder"]).abs()
    bound = bud["decoder"] + 2.0 ** -21 * (word_off.abs() + ref["decoder"].abs())      # + a few fp32 roundings of the sum
    print("word table: worst |error| / bound %.3f" % float((err / bound).max()))
    assert bool((err <= bound).all())
    assert float(ref["decoder"].abs().max()) > 4.0 * float(bound.max())               # the decoder term is what is being seen


def test_no_label_at_all_is_the_constant_zero():
    cfg, model, params, core, batch = make(labels=False)
    out = step_forward(model, batch, params)
    assert out[1] is core._const_zeros[0] and float(out[1]) == 0.0
    core.zero_flat_grads()
    out[0].backward()
    torch.cuda.synchronize()
    assert all(float(g.abs().max()) == 0.0 for g in grads(core, HEAD).values())
    assert torch.isfinite(out[0]).all()


def test_bad_labels_are_refused_before_any_launch():
    cfg, model, params, core, batch = make()
    for bad in (VOCAB, -2):
        b = dict(batch, mask=batch["mask"].clone())
        b["mask"][1, 1] = bad
        with pytest.raises(ValueError, match="masked_lm_labels"):
            step_forward(model, b, params)
    with torch.no_grad():                                                               # forward only; labels from the device cost a copy, not an error
        out = step_forward(model, dict(batch, mask=batch["mask"].to(DEV)), params)
    assert float(out[1]) > 0.0 and not out[1].requires_grad
    model.eval()
    ev = step_forward(model, batch, params, evaluation=True)                            # the inference branch is untouched
    assert ev[0] is None and ev[1] is None


def one_step_grads(model, params, core, batch, passes=1, scaler=None):
    core.zero_flat_grads()
    for _ in range(passes):
        core._calls = 0
        loss = step_forward(model, batch, params)[0]
        (loss if scaler is None else scaler.scale(loss)).backward()
    torch.cuda.synchronize()
    return grads(core)


def test_accumulation_and_grad_scaler_are_exact():
    cfg, model, params, core, batch = make()
    one = one_step_grads(model, params, core, batch)
    two = one_step_grads(model, params, core, batch, passes=2)
    scaled = one_step_grads(model, params, core, batch, scaler=torch.amp.GradScaler("cuda", init_scale=1024.0))
    assert all(float(one[n].abs().max()) > 0.0 for n in HEAD + (WORD,))
    for n in HEAD:                                                                      # the LM path alone: powers of two all the way
        assert torch.equal(scaled[n], 1024.0 * one[n]), n
    # the word table also holds the engine's embedding term, whose loss seeds the head kernel scales in fp32 (tests/test_seq_outputs_gpu.py)
    assert float((scaled[WORD] / 1024.0 - one[WORD]).abs().max()) <= 1e-6 * float(one[WORD].abs().max())
    for n, g in one.items():
        if n not in ATOMIC_GRADS and n != WORD:
            assert torch.equal(two[n], 2.0 * g), n
    # the word table sums TWO terms per pass, decoder d then embedding e: ((d + e) + d) + e against 2 (d + e) is three fp32 additions on
    # partial sums of at most 2 (|d| + |e|), so 3 * 2^-24 * 2 (|d| + |e|) < 2^-21 (|d| + |e|), with |e| <= |d + e| + |d| and |d| from the reference
    core.return_sequence_outputs = True
    step_forward(model, batch, params)
    x = core.sequence_output_t.detach().double().cpu().reshape(-1, cfg.hidden_size)
    d = R.reference(head_weights(core), x, batch["mask"].reshape(-1), g=COEFF)["decoder"].abs()
    err = (two[WORD] - 2.0 * one[WORD]).double().cpu().abs()
    assert bool((err <= 2.0 ** -21 * (2.0 * d * 1.01 + one[WORD].double().cpu().abs()) + 1e-12).all())


def test_frozen_text_layer_drops_the_decoder_product_only():
    cfg, model, params, core, batch = make(fixed_t_layer=1)
    got = one_step_grads(model, params, core, batch)
    byname = dict(core.named_parameters())
    assert byname[WORD].grad is None and WORD in core.tensors_without_grad
    assert all(float(got[n].abs().max()) > 0.0 for n in HEAD)
    # ... and a head tensor the caller freezes gets none while the others keep theirs
    byname[HEAD[1]].requires_grad_(False)
    got = one_step_grads(model, params, core, batch)
    assert byname[HEAD[1]].grad is None and all(float(got[n].abs().max()) > 0.0 for n in HEAD if n != HEAD[1])


def test_requested_input_gradient_sees_the_lm_term():
    seen = []
    for coeff in (None, COEFF):
        cfg, model, params, core, batch = make(coeff)
        b = dict(batch, image_feat=batch["image_feat"].to(DEV).requires_grad_(True))
        step_forward(model, b, params)[0].backward()
        torch.cuda.synchronize()
        seen.append(b["image_feat"].grad.clone())
    assert torch.isfinite(seen[1]).all() and not torch.equal(seen[0], seen[1])


def trained_weights(overlap=False, wrap=False, steps=2):
    from crct.optim import get_optimizer
    cfg, model, params, core, batch = make()
    opt = get_optimizer(dict(params, lr=1e-3, image_lr=1e-3), model)
    opt.overlap = overlap
    runner = model
    if wrap:
        from crct.ddp import FlatGradDDP
        runner = FlatGradDDP(model, device_ids=[0], find_unused_parameters=True)
    start = core.flat_params.clone()
    for _ in range(steps):
        step_forward(runner, batch, params)[0].backward()
        opt.step()
        opt.zero_grad()
    if overlap:
        opt.synchronize()
    torch.cuda.synchronize()
    return core, start, core.flat_params.clone(), opt


def test_fused_adamw_moves_the_head_and_overlap_changes_no_bit():
    core, start, plain, _ = trained_weights()
    for e in core.table:
        if e.name in HEAD:
            assert not torch.equal(start[e.offset:e.offset + e.numel], plain[e.offset:e.offset + e.numel]), e.name
    _, _, over, opt = trained_weights(overlap=True)
    for e in core.table:
        if e.used and e.name not in ATOMIC_GRADS:
            assert torch.equal(plain[e.offset:e.offset + e.numel].view(torch.int32), over[e.offset:e.offset + e.numel].view(torch.int32)), e.name
    with pytest.raises(RuntimeError, match="lm_loss_coeff"):
        opt.set_early(True)


def test_data_parallel_wrapper_at_world_size_one():
    import torch.distributed as dist
    _, _, plain, _ = trained_weights(steps=1)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29571")
    torch.cuda.set_device(0)
    dist.init_process_group(backend="nccl", rank=0, world_size=1, device_id=DEV)
    try:
        core, _, wrapped, _ = trained_weights(wrap=True, steps=1)
    finally:
        dist.destroy_process_group()
    for e in core.table:
        if e.used and e.name not in ATOMIC_GRADS:
            assert torch.equal(plain[e.offset:e.offset + e.numel].view(torch.int32), wrapped[e.offset:e.offset + e.numel].view(torch.int32)), e.name
