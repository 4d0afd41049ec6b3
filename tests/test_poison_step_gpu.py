"""A non-finite input element through the whole step engine (-m gpu): DESIGN.md, "Non-finite values".

Row 1 of a batch of three is poisoned (one NaN in image_feat[1], or one inf in loc[1]); the CPU oracle on the same poisoned batch says
which outputs must turn non-finite (R1), the clean batch's launch which bits rows 0 and 2 must keep (R2).  Under a GradScaler the
poisoned step must be skipped as a whole -- with nothing written into flat_grads by the test: the NaN has to travel from the input
through forward and backward into the gradients by itself -- and the model must afterwards train exactly like a twin that never saw
the batch.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from crct import config as C                       # noqa: E402
from crct import synthetic as S                    # noqa: E402
from crct.optim import get_optimizer               # noqa: E402
from crct.step_adapter import forward as step_forward   # noqa: E402
from oracle import crct_oracle as O                # noqa: E402
from helpers import ATOMIC_GRADS, seeded_weights   # noqa: E402
import poison_ref as PR                            # noqa: E402
from test_step_gpu import build_model, _oracle_threads   # noqa: E402

B, T, V = 3, 7, 5
ROW = 1


def _tiny():
    cfg = C.tiny_config()
    base = C.default_params(categories=9, L1=True)
    batch = S.make_batch(B, T, V, cfg.v_feature_size, categories=9, vocab_size=cfg.vocab_size, seed=11)
    assert bool(batch["image_mask"][ROW, 0]), "the poisoned visual position must be attended"
    return cfg, base, batch


def _poisoned(batch, key="image_feat", index=(ROW, 0, 3), value=PR.NAN):
    out = dict(batch)
    out[key] = PR.plant(batch[key].float(), index, value).to(batch[key].dtype)
    return out


def _oracle(cfg, base, batch, evaluation, seed=7):
    cpu = dict(base, device=torch.device("cpu"))
    sd = seeded_weights(cfg, cpu, base_seed=seed)
    out = O.oracle_step(sd, cfg, cpu, batch, evaluation=evaluation, training=not evaluation, cls_dropout=0.0)
    return sd, out


def _per_row(out):
    """The outputs of a step that carry one entry per batch row: answer scores and the regression's prediction, loss, l1 and d5."""
    reg = out[5]
    return dict(scores=out[4].detach().float(), reg_pred=reg[0].detach().float(), reg_loss=reg[1].detach().float(),
                reg_l1=reg[2].detach().float(), d5=reg[4].detach().float())


def test_evaluation_forward_keeps_a_poisoned_batch_row_to_itself():
    """Evaluation forward of the clean and of the poisoned batch: rows 0 and 2 of every per-row output carry the clean launch's bits;
    row 1 is non-finite wherever the oracle's is.  The one check that a batch row cannot reach another through the whole engine."""
    cfg, base, batch = _tiny()
    model, params = build_model(cfg, base, weights=None, seed=7)
    model.eval()
    for what, pb in (("NaN in image_feat", _poisoned(batch)), ("inf in loc", _poisoned(batch, "loc", (ROW, 0, 1), PR.INF))):
        with torch.no_grad():
            clean = _per_row(step_forward(model, batch, params, output_nsp_scores=True, evaluation=True))
            got = _per_row(step_forward(model, pb, params, output_nsp_scores=True, evaluation=True))
        torch.cuda.synchronize()
        ref = _per_row(_oracle(cfg, base, pb, True)[1])
        ref_clean = _per_row(_oracle(cfg, base, batch, True)[1])
        F = {}
        for k, v in ref.items():
            assert tuple(v.shape) == tuple(got[k].shape) and v.shape[0] == B, (k, tuple(v.shape), tuple(got[k].shape))
            assert not bool(PR.nonfinite(ref_clean[k]).any()), k
            F[k] = PR.nonfinite(v)
            assert not bool(F[k][0].any()) and not bool(F[k][2].any()), (what, k, "the oracle itself leaks across batch rows")
        assert bool(F["scores"][ROW].all()), what + ": the oracle's scores of the poisoned row are finite"
        PR.assert_footprint(clean, got, F, "evaluation forward, " + what)


def test_training_step_carries_the_poison_into_loss_and_gradients():
    """Training step without a scaler: the loss is non-finite iff the oracle's is, and every parameter tensor whose oracle gradient
    holds a non-finite value holds one in flat_grads too.  The input-gradient path: loc requires grad and the gradient at the text
    embedding is kept (core.keep_text_embedding_grad) -- both stay finite, with the clean step's bits, in rows 0 and 2."""
    cfg, base, batch = _tiny()
    torch.set_num_threads(_oracle_threads())
    for what, pb in (("NaN in image_feat", _poisoned(batch)), ("inf in loc", _poisoned(batch, "loc", (ROW, 0, 1), PR.INF))):
        model, params = build_model(cfg, base, weights=None, seed=7)
        core = model.bert_pretrained
        grads = {}
        for name, b in (("clean", batch), ("poisoned", pb)):
            core.zero_flat_grads()
            b = dict(b, loc=b["loc"].detach().clone().requires_grad_(True))
            core.keep_text_embedding_grad = True             # the gradient at the text embedding, for this pass
            loss = step_forward(model, b, params)[0]
            loss.backward()
            torch.cuda.synchronize()
            grads[name] = (float(loss.detach()), core.flat_grads.clone(), b["loc"].grad.detach().cpu().clone(),
                           core.text_embedding_grad.detach().cpu().reshape(B, T, -1).clone())
        sd, ref = _oracle(cfg, base, pb, False)
        ref[0].backward()
        assert torch.isfinite(torch.tensor(grads["clean"][0])) and bool(torch.isfinite(grads["clean"][1]).all())
        assert bool(torch.isfinite(ref[0])) == bool(torch.isfinite(torch.tensor(grads["poisoned"][0]))), (what, float(ref[0]), grads["poisoned"][0])
        assert not bool(torch.isfinite(ref[0])), what + ": the oracle's loss is finite: the case tests nothing"
        want = {k for k, p in sd.items() if p.grad is not None and bool(PR.nonfinite(p.grad).any())}
        have = {e.name for e in core.table if e.used and bool(PR.nonfinite(grads["poisoned"][1][e.offset:e.offset + e.numel]).any())}
        assert want, what
        assert want <= have, (what, sorted(want - have))
        lc, lp = grads["clean"][2], grads["poisoned"][2]
        rows = torch.zeros(lc.shape, dtype=torch.bool)
        rows[ROW] = True
        assert bool(torch.isfinite(lp[0]).all()) and bool(torch.isfinite(lp[2]).all())
        assert bool((PR.bits(lp)[~rows] == PR.bits(lc)[~rows]).all()), what + ": loc.grad of the clean rows changed"
        ec, ep = grads["clean"][3], grads["poisoned"][3]       # [B, T, H]: the poisoned batch row's gradient is non-finite, the others' bits stay
        assert bool(torch.isfinite(ec).all()) and bool(PR.nonfinite(ep[ROW]).any()), what + ": text_embedding_grad of the poisoned row"
        assert bool((PR.bits(ep)[[0, 2]] == PR.bits(ec)[[0, 2]]).all()), what + ": text_embedding_grad of the clean rows changed"


def _snapshot(core, opt):
    return dict(params=core.flat_params.clone(), shadow=core.flat_shadow.clone(), m=opt._m.clone(), v=opt._v.clone())


def _scaler_step(model, params, opt, scaler, batch):
    loss = step_forward(model, batch, params)[0]
    scaler.scale(loss).backward()
    scaler.step(opt)
    scaler.update()
    return loss


@pytest.mark.parametrize("poison", ["image_feat_nan", "loc_inf"])
@pytest.mark.parametrize("lazy", [False, True], ids=["eager_zero_grad", "lazy_zero_grad"])
def test_grad_scaler_skips_a_step_poisoned_in_the_forward_pass(lazy, poison):
    """The GradScaler loop of the reference (train.py:157, 208-212) on a batch with one NaN feature, nothing written into flat_grads
    by the test.  The step is skipped: weights, bf16 shadow, moments and the device step counter keep their bits and the scale halves;
    after zero_grad() the gradients are finite; the next clean step equals the same step of a twin model that never saw the batch,
    bit for bit outside helpers.ATOMIC_GRADS and within 2e-7 (test_grad_scaler_step_equals_plain_step's bound) there.

    zero_grad() in its two forms.  Eager (lazy_zero_grad = False): all of flat_grads is finite afterwards.  Lazy (the default): zero_grad
    clears the gradients backward ACCUMULATES into and leaves the Linear weight gradients, which the next backward pass overwrites, as
    they are (CrctModel.zero_flat_grads) -- so those still hold the skipped step's NaN (measured on the MI355X: with the lazy form
    flat_grads is NOT all finite after zero_grad()).  There the finiteness is asserted on the runs zero_grad() clears, and on the whole
    buffer behind the next backward pass, where it must also equal the twin's bit for bit."""
    cfg, base, batch = _tiny()
    pb = _poisoned(batch) if poison == "image_feat_nan" else _poisoned(batch, "loc", (ROW, 0, 1), PR.INF)
    models = []
    for twin in (False, True):
        model, params = build_model(cfg, base, weights=None, seed=7)
        core = model.bert_pretrained
        opt = get_optimizer(params, model)
        opt.overlap = False
        opt.lazy_zero_grad = lazy
        if not twin:
            scaler = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=10 ** 6)
            loss = step_forward(model, pb, params)[0]
            scaler.scale(loss).backward()
            torch.cuda.synchronize()
            before = _snapshot(core, opt)                    # behind the forward pass, which is what builds the bf16 shadow
            scaler.step(opt)
            scaler.update()
            opt.synchronize()
            torch.cuda.synchronize()
            assert not bool(torch.isfinite(loss.detach())), "the NaN did not reach the loss"
            assert not bool(torch.isfinite(core.flat_grads).all()), "the NaN did not reach flat_grads"
            after = _snapshot(core, opt)
            for k in before:
                assert torch.equal(PR.bits(before[k]), PR.bits(after[k])), "a skipped step changed " + k
            assert int(opt._step_dev.item()) == 0, "a skipped step was counted"
            assert float(scaler.get_scale()) == 512.0
            opt.zero_grad()
            torch.cuda.synchronize()
            cleared = torch.ones_like(core.flat_grads, dtype=torch.bool)
            if lazy:
                plan = core._lazy_zero_plan()
                assert plan is not None, "one backward pass has run: the lazy form must be in force"
                cleared.zero_()
                for o, n in zip(plan[0].tolist(), plan[1].tolist()):
                    cleared[o:o + n] = True
                assert bool(cleared.any()) and not bool(cleared.all())
            assert bool(torch.isfinite(core.flat_grads[cleared]).all()), "zero_grad() left non-finite gradients behind"
        else:
            scaler = torch.amp.GradScaler("cuda", init_scale=512.0, growth_interval=10 ** 6)
        core._calls = 1
        loss = _scaler_step(model, params, opt, scaler, batch)
        opt.synchronize()
        torch.cuda.synchronize()
        assert int(opt._step_dev.item()) == 1 and float(scaler.get_scale()) == 512.0
        models.append((core, opt, float(loss), core.flat_grads.clone()))
    (ca, oa, la, ga), (cb, ob, lb, gb) = models
    assert la == lb, (la, lb)
    assert bool(torch.isfinite(ga).all()), "the backward pass after the skipped step left non-finite gradients"
    for e in ca.table:
        if not e.used:
            continue
        sl = slice(e.offset, e.offset + e.numel)
        if any(a in e.name for a in ATOMIC_GRADS):
            assert torch.allclose(ca.flat_params[sl], cb.flat_params[sl], rtol=0, atol=2e-7), e.name
            continue
        assert torch.equal(PR.bits(ga[sl]), PR.bits(gb[sl])), e.name + ": gradient of the step after the skipped one"
        for x, y, what in ((ca.flat_params, cb.flat_params, "weights"), (ca.flat_shadow, cb.flat_shadow, "bf16 shadow"), (oa._m, ob._m, "m"), (oa._v, ob._v, "v")):
            assert torch.equal(PR.bits(x[sl]), PR.bits(y[sl])), "%s: %s differ from the twin's" % (e.name, what)


def test_fp8_grad_scaler_skips_a_step_poisoned_in_the_forward_pass():
    """The same loop in fp8 mode at full depth and the odd shape of test_fp8_mode_through_the_training_loop_paths (B = 3, 31 tokens, 7
    visual elements).  Skipped as a whole: weights, the e4m3 shadow, its transposed copy and the weight scales as before; no activation
    or gradient scale non-finite or zero afterwards (the NaN reached their amax words, crct_fp8_update_scales kept the scales); the
    following clean step's loss and scores within that test's bounds (5e-2 of the oracle's loss, 2e-2 on the scores)."""
    torch.set_num_threads(_oracle_threads())
    cfg = C.vilbert_config(v_feature_size=2048, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                           v_hidden_dropout_prob=0.0, v_attention_probs_dropout_prob=0.0)
    Bf, Tf, Vf = 3, 31, 7
    batch = S.make_batch(Bf, Tf, Vf, 2048, seed=103)
    assert bool(batch["image_mask"][ROW, 0])
    pb = _poisoned(batch)
    model, params = build_model(cfg, C.default_params(fp8=True), weights=None, seed=11)
    core = model.bert_pretrained
    cpu_params = dict(C.default_params(), device=torch.device("cpu"))
    ref = O.oracle_step(seeded_weights(cfg, cpu_params, base_seed=11), cfg, cpu_params, batch, cls_dropout=0.0)
    for _ in range(2):                  # calibration passes, as that test makes them
        core.zero_flat_grads()
        out = step_forward(model, batch, params, output_nsp_scores=True)
        out[0].backward()
    torch.cuda.synchronize()
    scores0 = out[4].detach().float().clone()
    opt = get_optimizer(params, model)
    scaler = torch.amp.GradScaler("cuda", init_scale=256.0, growth_interval=10 ** 6)
    st = core._fp8
    opt.zero_grad()
    q0, qt0, ws0, p0 = st.q.clone(), st.qt.clone(), st.weight.scale.clone(), core.flat_params.clone()
    flags0 = (st.calibrated, st.scaled, st.bwd_calibrated)
    loss = _scaler_step(model, params, opt, scaler, pb)
    opt.synchronize()
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(loss.detach())) and not bool(torch.isfinite(core.flat_grads).all())
    assert torch.equal(core.flat_params, p0) and torch.equal(st.q, q0) and torch.equal(st.qt, qt0) and torch.equal(st.weight.scale, ws0)
    assert (st.calibrated, st.scaled, st.bwd_calibrated) == flags0 and float(scaler.get_scale()) == 128.0
    opt.zero_grad()
    out = step_forward(model, batch, params, output_nsp_scores=True)       # the next clean step (its forward updates the activation scales)
    scaler.scale(out[0]).backward()
    scaler.step(opt)
    scaler.update()
    opt.synchronize()
    torch.cuda.synchronize()
    for name, ss in (("activation", st.act), ("gradient", st.grad), ("weight", st.weight)):
        sc = ss.scale[:ss.n]
        assert bool(torch.isfinite(sc).all()) and bool((sc != 0).all()), name + " scales after the poisoned step"
        assert bool(torch.isfinite(ss.amax).all()), name + " amax words after the clean step"
    assert abs(float(out[0]) - float(ref[0])) <= 5e-2 * abs(float(ref[0])), (float(out[0]), float(ref[0]))
    assert float((out[4].detach().float() - scores0).abs().max()) <= 2e-2
    assert not torch.equal(core.flat_params, p0) and bool(torch.isfinite(core.flat_params).all()) and float(scaler.get_scale()) == 128.0
