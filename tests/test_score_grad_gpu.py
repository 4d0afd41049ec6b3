"""The answer scores and the regressed value as differentiable outputs of the training step (-m gpu): with
``core.differentiable_scores = True`` the training tuple's ``seq_relationship_score`` (the step adapter's ``nsp_scores``) and, for a
PlotQA regressor, ``regression[0]`` carry a graph, and a loss written on them trains the model.

tiny_L1 (the golden weights and batch: B = 3, needs = rows 0 and 2, scale 100) against the oracle under autograd.  The oracle detaches
``reg[0]``, so its value is rebuilt here as where(needs, taps['reg_raw'] * R[:, 3], 0).  The cotangents are seeded draws
(Generator().manual_seed(4242)) scaled once, from the oracle alone: Cl to 4 x ||d loss / d logits||, Cv on the needs rows so that
Cv * R[:, 3] has 4 x ||d loss / d reg_raw||.

* Aux alone -- (Cl scores).sum() alone and (Cv value).sum() alone, the loss not differentiated: every gradient comes through the new
  path (the code before this feature raises); every parameter gradient at cosine >= 0.99, norm within 5 %, ~0 where the oracle has none
  (compare_grads of tests/test_seq_outputs_gpu.py, the rule of test_tiny_step_matches_reference), the head parameters included.
* loss + both terms at the same bounds, after the oracle side showed that the logits term moved the encoder's gradients.
* Values: bit-equal to the flag-off model's; regression[0] exactly 0 without needs.
* Off means off, launch for launch and bit for bit; used, the backward launches what it launched.
* Saliency of the answer, the autograd surface, the variants, an fp8 step.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from crct import config as C                       # noqa: E402
from crct import synthetic as S                    # noqa: E402
from crct.step_adapter import forward as step_forward   # noqa: E402
from helpers import ATOMIC_GRADS, GOLDEN, load_case    # noqa: E402
from oracle import crct_oracle as O                # noqa: E402
from test_input_grad_gpu import _tiny, bits, leaves    # noqa: E402
from test_seq_outputs_gpu import _backward_into, _logged, compare_grads, is_head    # noqa: E402
from test_step_gpu import build_model, cosine      # noqa: E402

DEV = torch.device("cuda:0")
GAIN = 4.0
_FIX = {}


def _oracle_terms(sd, cfg, cpu_params, batch, share=None, autocast=False):
    """oracle_step under autograd: (loss, logits, value, d loss / d logits, d loss / d reg_raw) with value rebuilt from the raw tap."""
    taps = {}
    if autocast:
        with torch.autocast("cpu", dtype=torch.bfloat16):
            out = O.oracle_step(sd, cfg, cpu_params, batch, taps=taps, cls_dropout=0.0)
    else:
        out = O.oracle_step(sd, cfg, cpu_params, batch, taps=taps, cls_dropout=0.0)
    R = batch["R"]
    needs = R[:, 1] == 1
    raw = taps["reg_raw"].float()
    value = torch.where(needs, raw * R[:, 3], torch.zeros_like(raw))
    return out[0].float(), out[4].float(), value, taps["reg_raw"], needs


def fixture():
    """tiny_L1: weights, batch, a flag-on model, and the oracle's passes (loss, each aux term alone, loss + logits term, loss + both)."""
    if not _FIX:
        z, meta, cfg, params, batch = load_case("tiny_L1")
        zw = np.load(os.path.join(GOLDEN, "tiny_L1.npz"))
        model, params = build_model(cfg, params, weights=zw)
        model.train()
        core = model.bert_pretrained
        core.differentiable_scores = True
        cpu_params = dict(params, device=torch.device("cpu"))
        sd = {k[2:]: torch.from_numpy(zw[k]).clone().requires_grad_(True) for k in zw.files if k.startswith("w.")}
        loss, logits, value, raw, needs = _oracle_terms(sd, cfg, cpu_params, batch)
        gl, gr = torch.autograd.grad(loss, [logits, raw], retain_graph=True)
        gen = torch.Generator().manual_seed(4242)
        Cl, Cv = torch.randn(logits.shape, generator=gen), torch.randn(value.shape, generator=gen)
        Cl = Cl * (GAIN * float(gl.double().norm()) / float(Cl.double().norm()))
        R3 = batch["R"][:, 3]
        Cv = Cv * (GAIN * float(gr.double().norm()) / float((Cv * R3)[needs].double().norm()))
        aux_l, aux_v = (Cl * logits).sum(), (Cv * value).sum()
        ref = dict(Cl=Cl, Cv=Cv, loss=float(loss.detach()), logits=logits.detach(), value=value.detach(), needs=needs,
                   plain=_backward_into(sd, loss), aux_l=_backward_into(sd, aux_l), aux_v=_backward_into(sd, aux_v),
                   with_l=_backward_into(sd, loss + aux_l), both=_backward_into(sd, loss + aux_l + aux_v))
        used = [k for k, g in ref["plain"].items() if g is not None]
        ref["reached"] = tuple(sum(ref[a][k] is not None and float(ref[a][k].double().norm()) >= 1e-7 for k in used) for a in ("aux_l", "aux_v"))
        enc = [k for k in used if k.startswith("bert.encoder.") and float(ref["plain"][k].double().norm()) >= 1e-7]
        moved = [cosine(ref["with_l"][k].float(), ref["plain"][k].float()) for k in enc]
        ref["moved"] = (sum(c < 0.9 for c in moved), len(moved), float(np.median(moved)))
        print("oracle tiny_L1: the logits / value term alone reaches %d / %d of %d used tensors; the logits term moves %d of %d encoder "
              "gradients below cosine 0.9 (median %.3f)" % (ref["reached"] + (len(used),) + ref["moved"]))
        _FIX.update(cfg=cfg, params=params, batch=batch, model=model, core=core, sd=sd, ref=ref, zw=zw, cpu_params=cpu_params)
    f = _FIX
    return f["cfg"], f["model"], f["params"], f["core"], f["batch"], f["sd"], f["ref"]


def run_step(model, params, core, batch, Cl=None, Cv=None, with_loss=True, it=1, scaler=None, zero=True):
    """One training forward + backward of loss (with_loss) + (Cl scores).sum() + (Cv value).sum(); returns the step's tuple."""
    if zero:
        core.zero_flat_grads()
    core._calls = it - 1
    out = step_forward(model, batch, params)
    terms = [out[0]] if with_loss else []
    if Cl is not None:
        terms.append((Cl.to(DEV) * out[4]).sum())
    if Cv is not None:
        terms.append((Cv.to(DEV) * out[5][0]).sum())
    total = sum(terms[1:], terms[0])
    (total if scaler is None else scaler.scale(total)).backward()
    torch.cuda.synchronize()
    return out


def same_bits(core, a, b, what, names=None):
    for e in core.table:
        if e.used and e.name not in ATOMIC_GRADS and (names is None or e.name in names):
            assert torch.equal(bits(a[e.offset:e.offset + e.numel]), bits(b[e.offset:e.offset + e.numel])), (what, e.name)


# ------------------------------------------------------------------------------------------------ 1. values
def test_values_are_the_flag_off_bits_and_carry_a_graph():
    cfg, model, params, core, batch, sd, ref = fixture()
    off_model, _ = build_model(cfg, params, weights=_FIX["zw"])
    off_model.train()
    off = off_model.bert_pretrained
    assert off.differentiable_scores is False
    off._calls = core._calls = 0
    o0 = step_forward(off_model, batch, params)
    o1 = step_forward(model, batch, params)
    assert not o0[4].requires_grad and not o0[5][0].requires_grad and o0[4].cpu().numpy().shape == (3, 2)
    assert o1[4].requires_grad and o1[5][0].requires_grad and o1[4].grad_fn is not None
    assert o1[4].dtype == o1[5][0].dtype == torch.float32 and tuple(o1[4].shape) == (3, 2) and tuple(o1[5][0].shape) == (3,)
    assert torch.equal(bits(o1[4]), bits(o0[4])) and torch.equal(bits(o1[5][0]), bits(o0[5][0]))
    assert o1[4].data_ptr() != core._engine.logits.data_ptr() and o1[4]._base is None and o1[5][0]._base is None
    needs = ref["needs"]
    assert needs.tolist() == [True, False, True] and float(o1[5][0].detach().cpu()[~needs].abs().max()) == 0.0
    assert float((o1[4].detach().cpu() - ref["logits"]).abs().max()) <= 3e-2
    assert float((o1[5][0].detach().cpu() - ref["value"]).abs().max()) <= 3e-2 * 100.0
    for k in (1, 2, 4):                            # the rest of regression stays plain
        assert not o1[5][k].requires_grad or k == 1
    with torch.no_grad():                          # without grad: plain tensors, the same bits
        o2 = step_forward(model, batch, params)
    assert not o2[4].requires_grad and not o2[5][0].requires_grad and torch.equal(bits(o2[4]), bits(o0[4]))


# ------------------------------------------------------------------------------------------------ 2. aux alone: the decisive comparison
def test_logits_term_alone_matches_the_oracle():
    """(Cl scores).sum() alone, the loss not differentiated: every parameter gradient, the heads' included, at cosine >= 0.99 and norm
    within 5 %; the regressor's exactly 0.  On the CPU the oracle's gradient of this term has norm >= 1e-7 on 153 of the 188 used tensors;
    measured on MI355X: 153 tensors compared, none outside the bounds."""
    cfg, model, params, core, batch, sd, ref = fixture()
    assert ref["reached"][0] >= 140, ref["reached"]
    run_step(model, params, core, batch, Cl=ref["Cl"], with_loss=False)
    n = compare_grads(core, ref["aux_l"], "tiny_L1 logits term alone")
    print("logits term alone: %d tensors compared" % n)
    assert n > 100
    for k, p in core.named_parameters():
        if k.startswith("regressor."):
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k


def test_value_term_alone_matches_the_oracle():
    """(Cv value).sum() alone: the same bounds; the classification half's gradients exactly 0.  The oracle's gradient of this term has norm
    >= 1e-7 on 160 of the 188 used tensors (144 of them >= 1e-6, which is where compare_grads starts to take cosines); measured on MI355X:
    144 tensors compared, none outside the bounds."""
    cfg, model, params, core, batch, sd, ref = fixture()
    assert ref["reached"][1] >= 140, ref["reached"]
    run_step(model, params, core, batch, Cv=ref["Cv"], with_loss=False)
    n = compare_grads(core, ref["aux_v"], "tiny_L1 value term alone")
    print("value term alone: %d tensors compared" % n)
    assert n > 100
    for k, p in core.named_parameters():
        if k.startswith(("cls.", "bert.t_pooler.", "bert.v_pooler.")):
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k


def test_loss_plus_both_terms_matches_the_oracle():
    cfg, model, params, core, batch, sd, ref = fixture()
    moved = ref["moved"]
    assert 2 * moved[0] >= moved[1] > 0, moved     # the logits term moved the oracle's encoder gradients: no pass on the loss alone
    out = run_step(model, params, core, batch, Cl=ref["Cl"], Cv=ref["Cv"])
    assert abs(float(out[0].detach()) - ref["loss"]) <= 2e-2 * abs(ref["loss"])
    assert compare_grads(core, ref["both"], "tiny_L1 loss + both terms") > 100


# ------------------------------------------------------------------------------------------------ 3. off means off
def test_off_means_off_launch_for_launch_and_bit_for_bit():
    """Flag never touched / set to False: the same launches, GEMM records, gradient bits and requires_grad.  Flag on, scores unused in
    backward: the same library launches (the two copies are torch's) and bits.  Flag on, scores used: the backward's launch list has
    the same length and GEMM records -- the upstream rides in the head launch -- and the gradients differ."""
    cfg, model, params, core, batch = _tiny()      # dropout on
    assert core.differentiable_scores is False

    def fwd(it=1):
        core.zero_flat_grads()
        core._calls = it - 1
        return step_forward(model, batch, params)

    def step(use=None):
        out, nf, lf = _logged(fwd)
        total = out[0] if use is None else out[0] + (use[0] * out[4]).sum() + (use[1] * out[5][0]).sum()
        _, nb, lb = _logged(lambda: total.backward())
        return out, (nf, nb), (lf, lb), core.flat_grads.clone()
    fwd()[0].backward()                            # builds the engine and refreshes the bf16 weight shadow: not part of a step
    out0, n0, log0, g0 = step()
    assert not out0[4].requires_grad and not out0[5][0].requires_grad
    core.differentiable_scores = False
    out1, n1, log1, g1 = step()
    assert n1 == n0 and log1 == log0 and not out1[4].requires_grad
    core.differentiable_scores = True
    out2, n2, log2, g2 = step()
    assert out2[4].requires_grad and out2[5][0].requires_grad
    assert n2 == n0 and log2 == log0, (n0, n2)
    for o in (out1, out2):
        assert torch.equal(bits(o[0].detach()), bits(out0[0].detach())) and torch.equal(bits(o[4].detach()), bits(out0[4]))
        assert torch.equal(bits(o[5][0].detach()), bits(out0[5][0]))
    for e in core.table:
        a = g0[e.offset:e.offset + e.numel]
        for g in (g1, g2):
            b = g[e.offset:e.offset + e.numel]
            if e.name in ATOMIC_GRADS:
                assert torch.allclose(a, b, rtol=1e-3, atol=1e-6), e.name
            else:
                assert torch.equal(bits(a), bits(b)), e.name
    gen = torch.Generator().manual_seed(3)
    use = (torch.randn(3, 2, generator=gen).to(DEV), torch.randn(3, generator=gen).to(DEV) * 0.01)
    out3, n3, log3, g3 = step(use)
    assert n3 == n0 and log3 == log0, (n0, n3)
    assert not torch.equal(bits(g3), bits(g0))
    assert core._engine._score_grads == (None, None)          # the request stood for that pass only


# ------------------------------------------------------------------------------------------------ 4. saliency of the answer
def test_answer_saliency_with_every_label_ignored():
    """image_feat.requires_grad_(True), every NSP label -1, backward of scores[:, 0].sum(): image_feat.grad against the oracle's at the
    bound of the input-gradient tests (1 - cos <= 1.6 x the bf16-autocast twin's + 0.004, norm within 5 %); loss.backward() on the same
    batch leaves no NSP contribution."""
    cfg, model, params, core, batch, sd, ref = fixture()
    b = dict(batch, next_sentence_labels=torch.full_like(batch["next_sentence_labels"], -1))
    gb = leaves(b, ("image_feat",))
    core.zero_flat_grads()
    core._calls = 0
    out = step_forward(model, gb, params)
    assert float(out[2].detach().abs().max()) == 0.0          # nsp_loss: no valid label
    out[4][:, 0].sum().backward()
    torch.cuda.synchronize()
    got = gb["image_feat"].grad.float().cpu()
    w = {k: v.detach() for k, v in sd.items()}
    want = {}
    for autocast in (False, True):
        ob = leaves(b, ("image_feat",))
        _, logits, _, _, _ = _oracle_terms(w, cfg, _FIX["cpu_params"], ob, autocast=autocast)
        logits[:, 0].sum().backward()
        want[autocast] = ob["image_feat"].grad.float()
    d, dy = 1.0 - cosine(got, want[False]), 1.0 - cosine(want[True], want[False])
    q = float(got.double().norm() / want[False].double().norm())
    print("answer saliency d scores[:, 0] / d image_feat: deficit %.5f (twin %.5f), norm ratio %.4f" % (d, dy, q))
    assert d <= 1.6 * dy + 0.004 and abs(q - 1.0) <= 0.05, (d, dy, q)
    # the loss on the same batch: the NSP term is 0 and seeds nothing
    core.zero_flat_grads()
    core._calls = 0
    out = step_forward(model, gb, params)
    out[0].backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[0].detach()))
    for k, p in core.named_parameters():
        if k.startswith(("cls.bi_seq_relationship.", "bert.t_pooler.", "bert.v_pooler.")):
            assert float(p.grad.abs().max()) == 0.0, k
    assert float(core.regressor.fusion._modules["6"].weight.grad.abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------ 5. the surface
def test_upstream_in_bf16_and_on_a_view_is_accepted():
    cfg, model, params, core, batch, sd, ref = fixture()
    Cl, Cv = ref["Cl"].bfloat16().float(), ref["Cv"].bfloat16().float()
    run_step(model, params, core, batch, Cl, Cv)
    base = core.flat_grads.clone()
    wide = torch.zeros(3, 7, dtype=torch.bfloat16, device=DEV)
    vl, vv = wide[:, 1:5:2], wide[:, 6]            # bf16, strided, unaligned
    vl.copy_(Cl.to(DEV))
    vv.copy_(Cv.to(DEV))
    assert not vl.is_contiguous() and not vv.is_contiguous()
    core.zero_flat_grads()
    core._calls = 0
    out = step_forward(model, batch, params)
    torch.autograd.backward([out[0], out[4], out[5][0]], [torch.ones((), device=DEV), vl, vv])
    torch.cuda.synchronize()
    same_bits(core, base, core.flat_grads, "bf16 views")


def test_grad_scaler_unscales_to_the_plain_gradients_and_sees_an_inf():
    from crct.optim import get_optimizer
    cfg, model, params, core, batch = _tiny()
    core.differentiable_scores = True
    gen = torch.Generator().manual_seed(5)
    Cl, Cv = torch.randn(3, 2, generator=gen), torch.randn(3, generator=gen) * 0.01
    run_step(model, params, core, batch, Cl, Cv)
    plain = core.flat_grads.clone()
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=10 ** 6)
    run_step(model, params, core, batch, Cl, Cv, scaler=scaler)
    unscaled = core.flat_grads / 1024.0
    used = torch.cat([torch.arange(e.offset, e.offset + e.numel) for e in core.table if e.used and e.name not in ATOMIC_GRADS]).to(DEV)
    err = (unscaled[used] - plain[used]).abs().max() / plain[used].abs().max()
    print("GradScaler 1024 with score terms: max |unscaled - plain| / max |plain| = %.3g" % float(err))
    assert float(err) <= 1e-6
    opt = get_optimizer(params, model)
    opt.overlap = False
    before = core.flat_params.clone()
    Cinf = Cl.clone()
    Cinf[1, 0] = float("inf")
    run_step(model, params, core, batch, Cinf, Cv, scaler=scaler)
    assert not bool(torch.isfinite(core.flat_grads).all())
    scaler.step(opt)
    scaler.update()
    torch.cuda.synchronize()
    assert torch.equal(bits(core.flat_params), bits(before)), "the step was taken on non-finite gradients"
    assert float(scaler.get_scale()) < 1024.0


def test_flat_grad_ddp_at_world_one_gives_the_plain_bits():
    import torch.distributed as dist
    from crct.ddp import FlatGradDDP
    cfg, model, params, core, batch = _tiny()
    core.differentiable_scores = True
    gen = torch.Generator().manual_seed(6)
    Cl, Cv = torch.randn(3, 2, generator=gen), torch.randn(3, generator=gen) * 0.01
    run_step(model, params, core, batch, Cl, Cv)
    base = core.flat_grads.clone()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29567")
    torch.cuda.set_device(0)
    dist.init_process_group(backend="nccl", rank=0, world_size=1, device_id=DEV)
    try:
        ddp = FlatGradDDP(model, device_ids=[0], find_unused_parameters=True)
        run_step(ddp, params, core, batch, Cl, Cv)
        same_bits(core, base, core.flat_grads, "FlatGradDDP, world 1")
        with ddp.no_sync():                        # batch_multiply: two accumulated passes are twice one
            run_step(ddp, params, core, batch, Cl, Cv)
        run_step(ddp, params, core, batch, Cl, Cv, zero=False)
        same_bits(core, 2 * base, core.flat_grads, "FlatGradDDP, two passes")
    finally:
        core._ddp = None
        dist.destroy_process_group()


def test_frozen_heads_leave_the_encoder_gradients_unchanged():
    """cls.bi_seq_relationship and the regressor without gradient: their .grad is None, every other gradient keeps its bits."""
    cfg, model, params, core, batch, sd, ref = fixture()
    run_step(model, params, core, batch, ref["Cl"], ref["Cv"])
    base = core.flat_grads.clone()
    frozen = [p for k, p in core.named_parameters() if k.startswith(("cls.bi_seq_relationship.", "regressor."))]
    try:
        for p in frozen:
            p.requires_grad_(False)
        run_step(model, params, core, batch, ref["Cl"], ref["Cv"])
        names = {k for k, p in core.named_parameters() if p.grad is not None}
        assert all(p.grad is None for p in frozen) and len(names) > 100
        same_bits(core, base, core.flat_grads, "frozen heads", names=names)
    finally:
        for p in frozen:
            p.requires_grad_(True)
        run_step(model, params, core, batch)        # the views come back


def test_composes_with_sequence_outputs_and_runs_in_eval_mode():
    cfg, model, params, core, batch, sd, ref = fixture()
    core.return_sequence_outputs = True
    try:
        core.zero_flat_grads()
        core._calls = 0
        out = step_forward(model, batch, params)
        st = core.sequence_output_t
        assert st is not None and st.requires_grad and out[4].requires_grad and out[5][0].requires_grad and tuple(out[4].shape) == (3, 2)
        gen = torch.Generator().manual_seed(9)
        Ct = (torch.randn(st.shape, generator=gen) * 1e-3).to(DEV)
        (out[0] + (Ct * st).sum() + (ref["Cl"].to(DEV) * out[4]).sum() + (ref["Cv"].to(DEV) * out[5][0]).sum()).backward()
        torch.cuda.synchronize()
        both = core.flat_grads.clone()
        run_step(model, params, core, batch, ref["Cl"], ref["Cv"])
        assert not torch.equal(bits(both), bits(core.flat_grads)) and bool(torch.isfinite(both).all())
        # the two requests are independent: the head parameters see the score terms alone
        same_bits(core, both, core.flat_grads, "heads beside a sequence-output term", names={e.name for e in core.table if e.name.startswith(("cls.", "regressor.fusion.6."))})
    finally:
        core.return_sequence_outputs = False
    # model.eval() in the training branch (labels given): dropout off, the same graph
    run_step(model, params, core, batch, ref["Cl"], ref["Cv"])
    train_bits = core.flat_grads.clone()
    model.eval()
    try:
        out = run_step(model, params, core, batch, ref["Cl"], ref["Cv"])
        assert out[4].requires_grad and out[5][0].requires_grad
        same_bits(core, train_bits, core.flat_grads, "eval() in the training branch (the fixture has no dropout)")
    finally:
        model.train()


# ------------------------------------------------------------------------------------------------ 6. the variants
@pytest.mark.parametrize("case", ["variant_tiny_figureqa", "variant_tiny_dvqa_ce"])
def test_variants_have_differentiable_logits_and_a_plain_value(case):
    """binary_answers (no regressor) and CE_REG (a table lookup): the logits carry a graph, regression[0] does not.  The oracle models
    the PlotQA variant only, so the logits term is held to what it implies in closed form and to linearity: d / d b_cls of
    (Cl scores).sum() is Cl.sum(0) exactly (fp32 sums of B terms), the regressor's gradients are exactly 0, and the gradients of
    loss + term are those of the loss plus those of the term alone (two passes through the same bf16 kernels: cosine >= 0.999,
    norm within 1 %, per tensor)."""
    from test_variants_gpu import load_variant, variant_model
    z, meta, cfg, params, batch = load_variant(case)
    for k in ("hidden_dropout_prob", "attention_probs_dropout_prob", "v_hidden_dropout_prob", "v_attention_probs_dropout_prob"):
        setattr(cfg, k, 0.0)
    model, params = variant_model(meta, cfg, params)
    model.train()
    core = model.bert_pretrained
    core.cls_dropout = 0.0
    core.differentiable_scores = True
    assert core.variant[1] != "plotqa"
    B = batch["tokens"].shape[0]
    Cl = torch.randn(B, 2, generator=torch.Generator().manual_seed(12))
    out = run_step(model, params, core, batch, Cl=Cl, with_loss=False)
    assert out[4].requires_grad and out[5][0].requires_grad is False
    alone = core.flat_grads.clone()
    bias = core.cls.bi_seq_relationship.bias.grad.cpu()
    assert torch.allclose(bias, Cl.sum(0), rtol=1e-6, atol=1e-6), (bias, Cl.sum(0))
    for k, p in core.named_parameters():
        if k.startswith("regressor.") and p.grad is not None:
            assert float(p.grad.abs().max()) == 0.0, k
    run_step(model, params, core, batch)
    plain = core.flat_grads.clone()
    run_step(model, params, core, batch, Cl=Cl)
    both = core.flat_grads
    n = 0
    for e in core.table:
        if not e.used or e.name in ATOMIC_GRADS:
            continue
        s = slice(e.offset, e.offset + e.numel)
        want, got = (plain[s] + alone[s]).double(), both[s].double()
        if float(want.norm()) < 1e-6:
            continue
        c, q = float(torch.dot(want, got) / (want.norm() * got.norm())), float(got.norm() / want.norm())
        assert c >= 0.999 and abs(q - 1) <= 0.01, (e.name, c, q)
        n += 1
    assert n > 60
    with pytest.raises(RuntimeError, match="d_value"):
        core._engine.set_score_grads(value=torch.zeros(B, device=DEV))
    with pytest.raises(ValueError, match="contiguous fp32"):
        core._engine.set_score_grads(logits=torch.zeros(B, 2, device=DEV, dtype=torch.bfloat16))
    assert core._engine._score_grads == (None, None)


# ------------------------------------------------------------------------------------------------ 7. fp8
def test_fp8_step_trains_on_a_score_term():
    """params['fp8'] = True at full width, B 3, a label-smoothing-like term on the scores and a term on the value in the loss: finite
    gradients, and the loss falls over a few AdamW steps."""
    from crct.optim import get_optimizer
    cfg = C.vilbert_config(v_feature_size=2048, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, v_hidden_dropout_prob=0.0,
                           v_attention_probs_dropout_prob=0.0)
    model, params = build_model(cfg, C.default_params(fp8=True), weights=None, seed=11)
    model.train()
    core = model.bert_pretrained
    core.cls_dropout = 0.0
    core.differentiable_scores = True
    batch = S.make_batch(3, 31, 37, 2048, seed=103)
    opt = get_optimizer(params, model)
    totals = []
    for it in range(1, 6):
        opt.zero_grad()
        core._calls = it - 1
        out = step_forward(model, batch, params)
        total = out[0] - 0.1 * torch.log_softmax(out[4], 1).mean() + 1e-4 * (out[5][0] ** 2).mean()
        total.backward()
        torch.cuda.synchronize()
        for k, p in core.named_parameters():
            if p.grad is not None:
                assert bool(torch.isfinite(p.grad).all()), (it, k)
        totals.append(float(total.detach()))
        opt.step()
    print("fp8 step with score terms, objective over 5 steps:", [round(t, 4) for t in totals])
    assert all(np.isfinite(totals)) and totals[-1] < totals[0], totals
