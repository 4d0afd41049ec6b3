"""Sequence outputs of the training step as differentiable outputs (-m gpu): ``core.return_sequence_outputs = True`` puts
``sequence_output_t`` into slot 3 of the model's tuples (vilbert.py:1659, :1661), leaves it and ``sequence_output_v`` on the model, and
under grad both are outputs of the step's autograd node: whatever a caller hangs on them trains the encoder.

* Values against the oracle's taps and, bit for bit once rounded, against the engine's own bf16 states; evaluation under no_grad too.
* Segment 0 per element from the engine's own values: the hidden gradients with a request are bf16(float(without) + c C) on every row.
* The whole step and the aux term alone against the oracle under autograd (``loss + (Ct seq_t).sum() + (Cv seq_v).sum()``).
* Off means off: launch for launch and bit for bit.
* The autograd surface: dtypes and views of the upstream, input gradients beside it, GradScaler, FlatGradDDP, frozen tensors, fp8.

The cotangents Ct, Cv are seeded normal draws scaled ONCE, from the oracle alone, to AUX_GAIN times the norm of the oracle's own
d loss / d seq_t and d loss / d seq_v, so that the aux term dominates the gradient that enters the encoder from above; each oracle-side
helper asserts that this moved the oracle's encoder gradients (cosine with / without aux < 0.9 on at least half of them), so that no
comparison below can pass on the heads' gradient alone.  Checked on the CPU when this file was written: tiny_L1 135 of 135 encoder
tensors below 0.9 (median cosine 0.385).
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from crct import config as C                       # noqa: E402
from crct import lib as L                          # noqa: E402
from crct import synthetic as S                    # noqa: E402
from crct.step_adapter import forward as step_forward   # noqa: E402
from helpers import ATOMIC_GRADS, GOLDEN, load_case, seeded_weights    # noqa: E402
from oracle import crct_oracle as O                # noqa: E402
from test_input_grad_gpu import _tiny, bits, full_model, leaves    # noqa: E402
from test_layers_gpu import _SegmentTaps           # noqa: E402
from test_step_gpu import build_model, cosine      # noqa: E402

DEV = torch.device("cuda:0")
AUX_GAIN = 4.0
HEADS = ("bert.t_pooler.", "bert.v_pooler.", "cls.", "regressor.")


def is_head(name):
    return name.startswith(HEADS)


# ------------------------------------------------------------------------------------------------ the oracle side, once per fixture
_ORACLE = {}


def _backward_into(sd, scalar):
    for v in sd.values():
        v.grad = None
    scalar.backward(retain_graph=True)
    return {k: (None if v.grad is None else v.grad.detach().clone()) for k, v in sd.items()}


def oracle_with_aux(key, sd_values, cfg, cpu_params, batch, autocast=False, share=None):
    """oracle_step on (weights, batch) with taps; gradients of loss, of loss + aux and of aux alone, the taps and the cotangents.
    `share`: the (Ct, Cv) of another pass on the same draw (the bf16-autocast twin takes the fp32 pass's)."""
    if key in _ORACLE:
        return _ORACLE[key]
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in sd_values.items()}
    taps = {}
    if autocast:
        with torch.autocast("cpu", dtype=torch.bfloat16):
            out = O.oracle_step(sd, cfg, cpu_params, batch, taps=taps, cls_dropout=0.0)
    else:
        out = O.oracle_step(sd, cfg, cpu_params, batch, taps=taps, cls_dropout=0.0)
    seq_t, seq_v = taps["seq_t"], taps["seq_v"]
    loss = out[0].float()
    if share is None:
        gt, gv = torch.autograd.grad(loss, [seq_t, seq_v], retain_graph=True)
        gen = torch.Generator().manual_seed(4242)
        Ct, Cv = torch.randn(seq_t.shape, generator=gen), torch.randn(seq_v.shape, generator=gen)
        Ct = Ct * (AUX_GAIN * float(gt.double().norm()) / float(Ct.double().norm()))
        Cv = Cv * (AUX_GAIN * float(gv.double().norm()) / float(Cv.double().norm()))
    else:
        Ct, Cv = share
    aux = (Ct * seq_t.float()).sum() + (Cv * seq_v.float()).sum()
    r = dict(Ct=Ct, Cv=Cv, seq_t=seq_t.detach().float(), seq_v=seq_v.detach().float(), loss=float(loss.detach()),
             plain=_backward_into(sd, loss), both=_backward_into(sd, loss + aux), aux=_backward_into(sd, aux))
    enc = [k for k in sd if k.startswith("bert.encoder.") and r["plain"][k] is not None and float(r["plain"][k].double().norm()) >= 1e-7]
    moved = [cosine(r["both"][k].float(), r["plain"][k].float()) for k in enc]
    r["moved"] = (sum(c < 0.9 for c in moved), len(moved), float(np.median(moved)))
    if not autocast:
        print("oracle %s: aux moves %d of %d encoder gradients below cosine 0.9 (median cosine %.3f)" % ((key,) + r["moved"]))
        assert 2 * r["moved"][0] >= r["moved"][1] > 0, r["moved"]
    _ORACLE[key] = r
    return r


_TINY = {}


def tiny_golden():
    """tiny_L1: the golden weights and batch, one model for every test that only reads it (flag on), and the oracle's passes."""
    if not _TINY:
        z, meta, cfg, params, batch = load_case("tiny_L1")
        zw = np.load(os.path.join(GOLDEN, "tiny_L1.npz"))
        model, params = build_model(cfg, params, weights=zw)
        model.train()
        core = model.bert_pretrained
        core.return_sequence_outputs = True
        sd = {k[2:]: torch.from_numpy(zw[k]).clone() for k in zw.files if k.startswith("w.")}
        ref = oracle_with_aux("tiny_L1", sd, cfg, dict(params, device=torch.device("cpu")), batch)
        _TINY.update(cfg=cfg, params=params, batch=batch, model=model, core=core, sd=sd, ref=ref)
    t = _TINY
    return t["cfg"], t["model"], t["params"], t["core"], t["batch"], t["sd"], t["ref"]


def run_step(model, params, core, batch, Ct=None, Cv=None, with_loss=True, it=1, scaler=None, zero=True):
    """One training forward + backward of loss (with_loss) + (Ct seq_t).sum() + (Cv seq_v).sum(); returns (out, seq_t, seq_v)."""
    if zero:
        core.zero_flat_grads()
    core._calls = it - 1
    out = step_forward(model, batch, params)
    st, sv = core.sequence_output_t, core.sequence_output_v
    terms = [out[0]] if with_loss else []
    if Ct is not None:
        terms.append((Ct.to(DEV) * st).sum())
    if Cv is not None:
        terms.append((Cv.to(DEV) * sv).sum())
    total = sum(terms[1:], terms[0])
    (total if scaler is None else scaler.scale(total)).backward()
    torch.cuda.synchronize()
    return out, st, sv


def compare_grads(core, ref, what, names=None, cos_min=0.99, norm_tol=0.05):
    """Every parameter gradient against `ref` ({name: tensor or None}): cosine >= cos_min and norm within norm_tol where the reference
    has a gradient worth the name (test_tiny_step_matches_reference's rule and bounds), ~0 where it has not."""
    bad, n = [], 0
    for k, p in core.named_parameters():
        if names is not None and k not in names:
            continue
        r = ref.get(k)
        if r is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k          # never-used tensors
            continue
        assert p.grad is not None, k
        g, rn = p.grad.float().cpu(), float(r.double().norm())
        if rn < 1e-6:
            assert float(g.norm()) < 1e-3, (k, float(g.norm()))
            continue
        c, q = cosine(g, r.float()), float(g.double().norm()) / rn
        n += 1
        if c < cos_min or abs(q - 1) > norm_tol:
            bad.append((k, round(c, 5), round(q, 4), rn))
    assert n > 0 and not bad, (what, len(bad), bad[:10])
    return n


# ------------------------------------------------------------------------------------------------ 1. values
def test_values_match_the_oracle_and_round_to_the_engines_own_states():
    cfg, model, params, core, batch, sd, ref = tiny_golden()
    B, T = batch["tokens"].shape
    V = batch["image_feat"].shape[1]
    kw = dict(sep_indices=batch["sep_indices"], sep_len=batch["hist_len"] + 1, token_type_ids=batch["segments"],
              image_attention_mask=batch["image_mask"], image_target=batch["image_target"])
    from crct.model import SequenceMask
    kw["attention_mask"] = SequenceMask(batch["sep_indices"], batch["hist_len"], T)

    def check(slot3, training):
        st, sv = core.sequence_output_t, core.sequence_output_v
        assert slot3 is st
        assert st.dtype == sv.dtype == torch.float32 and tuple(st.shape) == (B, T, cfg.hidden_size) and tuple(sv.shape) == (B, V, cfg.v_hidden_size)
        for got, name in ((st, "seq_t"), (sv, "seq_v")):
            r = ref[name]
            err = float((got.detach().cpu() - r).abs().max() / (r.abs().max() + 1e-9))
            print("sequence output %s (%s): max error / max |oracle| %.4f" % (name, "training" if training else "evaluation", err))
            assert err < 4e-2, (name, err)
            tap = core._engine.tap(name, B, T, V)
            assert torch.equal(bits(got.detach().bfloat16()), bits(tap)), name
    # the training branch under grad: slot 3 of the 8-tuple, part of the graph
    out = core(batch["tokens"], batch["loc"], batch["image_feat"], batch["image_loc"], masked_lm_labels=batch["mask"],
               next_sentence_label=batch["next_sentence_labels"], gt_reg=[batch["R"], "L1_smooth"], **kw)
    assert len(out) == 8 and out[3].requires_grad and core.sequence_output_v.requires_grad and out[4] is None
    check(out[3], True)
    first = out[3]
    # evaluation under no_grad: slot 3 of the 7-tuple, a plain tensor of its own
    model.eval()
    try:
        with torch.no_grad():
            out = core(batch["tokens"], batch["loc"], batch["image_feat"], batch["image_loc"], gt_reg=[batch["R"], "L1"], **kw)
        assert len(out) == 7 and not out[3].requires_grad and out[3] is not first
        check(out[3], False)
        assert torch.equal(bits(out[3]), bits(first.detach()))          # dropout 0: evaluation computes the training forward's states
    finally:
        model.train()
    # the training branch without grad: plain tensors
    with torch.no_grad():
        out = core(batch["tokens"], batch["loc"], batch["image_feat"], batch["image_loc"], masked_lm_labels=batch["mask"],
                   next_sentence_label=batch["next_sentence_labels"], gt_reg=[batch["R"], "L1_smooth"], **kw)
    assert len(out) == 8 and not out[3].requires_grad and torch.equal(bits(out[3]), bits(first.detach()))


# ------------------------------------------------------------------------------------------------ 2. segment 0 per element
def _segment0(model, params, core, batch, cfg):
    B, T = batch["tokens"].shape
    V = batch["image_target"].shape[1]
    gen = torch.Generator().manual_seed(99)
    Ct = torch.randn(B, T, cfg.hidden_size, generator=gen) * 0.02
    Cv = torch.randn(B, V, cfg.v_hidden_size, generator=gen) * 0.02
    runs = []
    for req in (False, True):
        runner = _SegmentTaps(B, T, V)
        core._ddp = runner
        try:
            run_step(model, params, core, batch, Ct if req else None, Cv if req else None)
        finally:
            core._ddp = None
        runs.append(runner)
    plain, aux = runs
    c = 1.0                                              # CrctStepCfg.grad_scale of a pass outside a data-parallel group
    for name, a, b, Cx in (("grad.t", plain.gt[0], aux.gt[0], Ct), ("grad.v", plain.gv[0], aux.gv[0], Cv)):
        want = (a.float() + torch.tensor(c, dtype=torch.float32) * Cx).bfloat16()
        got = b.bfloat16()                               # the taps are bf16 values held as fp32
        assert torch.equal(got.float(), b), name
        wrong = (bits(got) != bits(want)).nonzero()
        assert wrong.numel() == 0, (name, wrong[:5].tolist())
        assert float(a[:, 1:].abs().max()) == 0.0 and float(a[:, 0].abs().max()) > 0.0, name      # the heads seed row 0 alone ...
        assert float(b[:, 1:].abs().max()) > 0.0, name                                             # ... the request every row
    assert torch.equal(bits(plain.grads[0]), bits(aux.grads[0])), "a head parameter gradient changed with the request"
    assert float(plain.grads[0].abs().max()) > 0.0
    return plain, aux


def test_segment0_adds_the_upstream_onto_the_heads_gradient_plotqa():
    """tiny config, dropout 0, PlotQA heads (the regressor pipes write row 0 last): every element of grad.t / grad.v after segment 0."""
    cfg, model, params, core, batch = _tiny(dropout=False)
    core.return_sequence_outputs = True
    _segment0(model, params, core, batch, cfg)


def test_segment0_adds_the_upstream_onto_the_heads_gradient_binary_answers():
    """The tiny FigureQA fixture (binary_answers: heads_bwd leaves right after the poolers) with its dropout set to 0."""
    from test_variants_gpu import load_variant, variant_model
    z, meta, cfg, params, batch = load_variant("variant_tiny_figureqa")
    for k in ("hidden_dropout_prob", "attention_probs_dropout_prob", "v_hidden_dropout_prob", "v_attention_probs_dropout_prob"):
        setattr(cfg, k, 0.0)
    model, params = variant_model(meta, cfg, params)
    model.train()
    core = model.bert_pretrained
    assert core.variant[1] not in ("plotqa", "ce"), core.variant
    core.return_sequence_outputs = True
    _segment0(model, params, core, batch, cfg)


def test_segment0_on_the_golden_tiny_fixture():
    cfg, model, params, core, batch, sd, ref = tiny_golden()
    _segment0(model, params, core, batch, cfg)


# ------------------------------------------------------------------------------------------------ 3. the whole step against the oracle
def test_tiny_step_with_aux_matches_the_oracle():
    """tiny_L1, L = loss + (Ct seq_t).sum() + (Cv seq_v).sum(): every parameter gradient cosine >= 0.99, norm within 5 %."""
    cfg, model, params, core, batch, sd, ref = tiny_golden()
    out, st, sv = run_step(model, params, core, batch, ref["Ct"], ref["Cv"])
    assert abs(float(out[0].detach()) - ref["loss"]) <= 2e-2 * abs(ref["loss"])
    n = compare_grads(core, ref["both"], "tiny_L1 loss + aux")
    assert n > 60


def test_full_width_step_with_aux_matches_the_oracle():
    """One full-width draw (B 3, V 37, T 31, dropout 0, the seeded weights, batch seed 103) with the rule of
    tests/test_input_grad_gpu.py::_whole_step per parameter tensor: 1 - cos <= 1.6 (1 - cos of the oracle's bf16-autocast twin on the
    same draw and cotangents) + 0.004, norm within 8 % of the fp32 oracle's (the twin's own norm ratios are printed beside it).
    Measured on MI355X over the 494 tensors with a gradient (printed by this test): deficit max / median 0.00543 / 0.00010 against the
    twin's 0.00522 / 0.00007 (worst: regressor.vis_pipe.2.weight, 0.00543 against 0.00522); norm ratios 0.9929 .. 1.0052, the twin's
    0.9901 .. 1.0051.  On the oracle the aux term moves 450 of 450 encoder gradients below cosine 0.9 (median 0.139)."""
    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
    cfg, model, params = full_model(0.0)
    core = model.bert_pretrained
    cpu_params = dict(params, device=torch.device("cpu"))
    sd = seeded_weights(cfg, cpu_params, base_seed=11, requires_grad=False)
    batch = S.make_batch(3, 31, 37, 2048, seed=103)
    ref = oracle_with_aux("full_103", sd, cfg, cpu_params, batch)
    yard = oracle_with_aux("full_103_bf16", sd, cfg, cpu_params, batch, autocast=True, share=(ref["Ct"], ref["Cv"]))
    core.return_sequence_outputs = True
    try:
        run_step(model, params, core, batch, ref["Ct"], ref["Cv"])
    finally:
        core.return_sequence_outputs = False
    rows, bad = [], []
    for k, p in core.named_parameters():
        r = ref["both"].get(k)
        if r is None or float(r.double().norm()) < 1e-7:
            continue
        g, y = p.grad.float().cpu(), yard["both"][k].float()
        d, dy = 1.0 - cosine(g, r), 1.0 - cosine(y, r)
        q, qy = float(g.double().norm() / r.double().norm()), float(y.double().norm() / r.double().norm())
        rows.append((d, dy, q, qy, k))
        if d > 1.6 * dy + 0.004 or abs(q - 1.0) > 0.08:
            bad.append((k, round(d, 5), round(dy, 5), round(q, 4), round(qy, 4)))
    ds, dys = sorted(r[0] for r in rows), sorted(r[1] for r in rows)
    print("full width B3 seed 103, loss + aux, %d tensors: deficit max / median %.5f / %.5f, twin's %.5f / %.5f, norm ratio %.4f .. %.4f, twin's %.4f .. %.4f"
          % (len(rows), ds[-1], ds[len(ds) // 2], dys[-1], dys[len(dys) // 2], min(r[2] for r in rows), max(r[2] for r in rows),
             min(r[3] for r in rows), max(r[3] for r in rows)), " worst", [(r[4], round(r[0], 5), round(r[1], 5)) for r in sorted(rows, reverse=True)[:3]])
    assert len(rows) > 450 and not bad, (len(bad), bad[:10])


# ------------------------------------------------------------------------------------------------ 4. the aux term alone
def test_aux_only_backward_trains_the_encoder_and_leaves_the_heads_at_zero():
    cfg, model, params, core, batch, sd, ref = tiny_golden()
    core.zero_flat_grads()
    core._calls = 0
    out = step_forward(model, batch, params)
    torch.autograd.backward([core.sequence_output_t, core.sequence_output_v], [ref["Ct"].to(DEV), ref["Cv"].to(DEV)])
    torch.cuda.synchronize()
    below = {k for k, _ in core.named_parameters() if not is_head(k)}
    n = compare_grads(core, ref["aux"], "tiny_L1 aux alone", names=below)
    assert n > 50
    heads = [(k, p) for k, p in core.named_parameters() if is_head(k)]
    assert len(heads) > 20
    for k, p in heads:
        assert p.grad is None or float(p.grad.abs().max()) == 0.0, (k, float(p.grad.abs().max()))
    assert out[0].grad_fn is not None


# ------------------------------------------------------------------------------------------------ 5. off means off
def _logged(fn):
    """fn() with every kernel launch counted (crct_prof_enable(2): the stamps of ALL kernels) and every GEMM launch recorded
    (crct_launch_log_*, which logs the GEMM kernels only): (result, launches, [(site, kind, M, N, K, cfg, n_problems)])."""
    import ctypes as CT
    lib = L.load()
    torch.cuda.synchronize()
    lib.crct_prof_reset()
    lib.crct_prof_enable(2)
    lib.crct_launch_log_enable(1)
    try:
        res = fn()
        torch.cuda.synchronize()
        n = lib.crct_prof_stamp_count()
        recs = []
        for i in range(lib.crct_launch_log_count()):
            r = L.LaunchRec()
            lib.crct_launch_log_read(i, CT.byref(r))
            recs.append((r.site, r.kind, r.M, r.N, r.K, r.cfg, r.n_problems))
    finally:
        lib.crct_launch_log_enable(0)
        lib.crct_prof_enable(0)
        lib.crct_prof_reset()
    return res, n, recs


def test_off_means_off_launch_for_launch_and_bit_for_bit():
    """(a) a model whose flag was never touched and one with the flag set to False: the same launches and GEMM records in forward and in
    backward, the same gradient bits.  (b) flag on, outputs not used in backward: the forward launches exactly two kernels more, the
    backward none, same bits.  (c) evaluation with the flag off launches what it launched before.  The launch log records GEMM launches
    only, so the counts come from the kernel stamps and the log pins the GEMM sequence."""
    cfg, model, params, core, batch = _tiny()                 # dropout on
    assert core.return_sequence_outputs is False

    def fwd(it=1):
        core.zero_flat_grads()
        core._calls = it - 1
        return step_forward(model, batch, params)

    def step():
        out, nf, lf = _logged(fwd)
        _, nb, lb = _logged(lambda: out[0].backward())
        return out, (nf, nb), (lf, lb), core.flat_grads.clone()
    fwd()[0].backward()                                       # builds the engine and refreshes the bf16 weight shadow: not part of a step
    out0, n0, log0, g0 = step()
    assert core.sequence_output_t is None and core.sequence_output_v is None
    model.eval()
    _, ne_0, le_0 = _logged(lambda: step_forward(model, batch, params, evaluation=True))
    model.train()
    eval0 = (ne_0, le_0)
    core.return_sequence_outputs = False                      # set, to what it was
    out1, n1, log1, g1 = step()
    assert n1 == n0 and log1 == log0 and torch.equal(bits(out1[0].detach()), bits(out0[0].detach()))
    core.return_sequence_outputs = True
    out2, n2, log2, g2 = step()
    assert core.sequence_output_t is not None and core.sequence_output_t.requires_grad
    assert n2 == (n0[0] + 2, n0[1]), (n0, n2)
    assert log2 == log0 and torch.equal(bits(out2[0].detach()), bits(out0[0].detach()))
    for e in core.table:
        a = g0[e.offset:e.offset + e.numel]
        for g in (g1, g2):
            b = g[e.offset:e.offset + e.numel]
            if e.name in ATOMIC_GRADS:
                assert torch.allclose(a, b, rtol=1e-3, atol=1e-6), e.name
            else:
                assert torch.equal(bits(a), bits(b)), e.name
    # evaluation: the flag on adds its two launches, the flag off (again) launches what the untouched model launched
    model.eval()
    try:
        _, ne_on, le_on = _logged(lambda: step_forward(model, batch, params, evaluation=True))
        assert core.sequence_output_t is not None and not core.sequence_output_t.requires_grad
        core.return_sequence_outputs = False
        _, ne_off, le_off = _logged(lambda: step_forward(model, batch, params, evaluation=True))
        assert core.sequence_output_t is None
        assert (ne_off, le_off) == eval0 and ne_on == ne_off + 2 and le_on == le_off, (ne_on, ne_off, eval0[0])
    finally:
        model.train()


# ------------------------------------------------------------------------------------------------ 6. the surface
def test_upstream_in_bf16_and_on_a_view_is_accepted():
    cfg, model, params, core, batch, sd, ref = tiny_golden()
    Ct = ref["Ct"].bfloat16().float()                         # representable in bf16: both routes see the same values
    run_step(model, params, core, batch, Ct, None)
    base = core.flat_grads.clone()
    B, T, H = Ct.shape
    wide = torch.zeros(B, T, 2 * H + 3, dtype=torch.bfloat16, device=DEV)
    view = wide[:, :, 3:3 + 2 * H:2]                          # bf16, strided, offset by 6 bytes
    view.copy_(Ct.to(DEV))
    assert not view.is_contiguous()
    core.zero_flat_grads()
    core._calls = 0
    step_forward(model, batch, params)
    torch.autograd.backward([core.last_loss, core.sequence_output_t], [torch.ones((), device=DEV), view])
    torch.cuda.synchronize()
    for e in core.table:
        if e.name not in ATOMIC_GRADS:
            assert torch.equal(bits(base[e.offset:e.offset + e.numel]), bits(core.flat_grads[e.offset:e.offset + e.numel])), e.name


def test_input_gradients_compose_with_output_gradients():
    cfg, model, params, core, batch, sd, ref = tiny_golden()
    b = leaves(batch, ("image_feat", "image_loc"))
    run_step(model, params, core, b, ref["Ct"], ref["Cv"])
    compare_grads(core, ref["both"], "tiny_L1 loss + aux with input gradients")
    # the oracle's input gradients of the same scalar
    w = {k: v.detach() for k, v in sd.items()}
    ob = leaves(batch, ("image_feat", "image_loc"))
    taps = {}
    oout = O.oracle_step(w, cfg, dict(params, device=torch.device("cpu")), ob, taps=taps, cls_dropout=0.0)
    (oout[0] + (ref["Ct"] * taps["seq_t"]).sum() + (ref["Cv"] * taps["seq_v"]).sum()).backward()
    for k in ("image_feat", "image_loc"):
        g, r = b[k].grad, ob[k].grad
        assert g is not None and tuple(g.shape) == tuple(r.shape)
        c, q = cosine(g.float().cpu(), r), float(g.double().norm() / r.double().norm())
        print("input gradient beside the aux term", k, "cosine %.5f norm ratio %.4f" % (c, q))
        assert c >= 0.99 and abs(q - 1) <= 0.05, (k, c, q)


def test_grad_scaler_unscales_to_the_plain_gradients_and_sees_an_inf():
    from crct.optim import get_optimizer
    cfg, model, params, core, batch = _tiny()
    core.return_sequence_outputs = True
    gen = torch.Generator().manual_seed(5)
    Ct = torch.randn(3, 9, cfg.hidden_size, generator=gen) * 0.01
    Cv = torch.randn(3, 5, cfg.v_hidden_size, generator=gen) * 0.01
    run_step(model, params, core, batch, Ct, Cv)
    plain = core.flat_grads.clone()
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=10 ** 6)
    run_step(model, params, core, batch, Ct, Cv, scaler=scaler)
    unscaled = core.flat_grads / 1024.0                       # the unscale: a power of two, exact
    used = torch.cat([torch.arange(e.offset, e.offset + e.numel) for e in core.table if e.used and e.name not in ATOMIC_GRADS]).to(DEV)
    err = (unscaled[used] - plain[used]).abs().max() / plain[used].abs().max()
    print("GradScaler 1024 with aux: max |unscaled - plain| / max |plain| = %.3g" % float(err))
    assert float(err) <= 1e-6
    # an inf in Ct reaches the gradients, and the scaler skips the step
    opt = get_optimizer(params, model)
    opt.overlap = False
    before = core.flat_params.clone()
    Cinf = Ct.clone()
    Cinf[1, 2, 3] = float("inf")
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
    core.return_sequence_outputs = True
    gen = torch.Generator().manual_seed(6)
    Ct = torch.randn(3, 9, cfg.hidden_size, generator=gen) * 0.01
    Cv = torch.randn(3, 5, cfg.v_hidden_size, generator=gen) * 0.01
    run_step(model, params, core, batch, Ct, Cv)
    base = core.flat_grads.clone()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29563")
    torch.cuda.set_device(0)
    dist.init_process_group(backend="nccl", rank=0, world_size=1, device_id=DEV)
    try:
        ddp = FlatGradDDP(model, device_ids=[0], find_unused_parameters=True)
        run_step(ddp, params, core, batch, Ct, Cv)
        for e in core.table:
            if e.used and e.name not in ATOMIC_GRADS:
                assert torch.equal(bits(base[e.offset:e.offset + e.numel]), bits(core.flat_grads[e.offset:e.offset + e.numel])), e.name
        # no_sync() / batch_multiply: two accumulated passes are twice one
        with ddp.no_sync():
            run_step(ddp, params, core, batch, Ct, Cv)
        run_step(ddp, params, core, batch, Ct, Cv, zero=False)
        for e in core.table:
            if e.used and e.name not in ATOMIC_GRADS:
                assert torch.equal(bits(2 * base[e.offset:e.offset + e.numel]), bits(core.flat_grads[e.offset:e.offset + e.numel])), e.name
    finally:
        core._ddp = None
        dist.destroy_process_group()


def test_frozen_tensors_keep_the_remaining_gradients_right():
    """fixed_t_layer = 1 and every head parameter requires_grad_(False): the gradients that remain match the oracle's with the same
    tensors detached; and with the whole text stream without gradient (and no input request) d_seq_t is moot and the pass runs."""
    z, meta, cfg0, params, batch = load_case("tiny_L1")
    zw = np.load(os.path.join(GOLDEN, "tiny_L1.npz"))
    cfg = C.BertConfig.from_dict(dict(meta["cfg"], fixed_t_layer=1))
    model, params = build_model(cfg, params, weights=zw)
    model.train()
    core = model.bert_pretrained
    core.return_sequence_outputs = True
    for k, p in core.named_parameters():
        if is_head(k):
            p.requires_grad_(False)
    _, _, _, _, _, sd, ref = tiny_golden()
    run_step(model, params, core, batch, ref["Ct"], ref["Cv"])
    live = {k for k, p in core.named_parameters() if p.grad is not None}
    dead = {k for k, p in core.named_parameters() if p.grad is None}
    assert all(k in dead for k, _ in core.named_parameters() if is_head(k) or k.startswith("bert.encoder.layer.0."))
    assert not any(is_head(k) for k in live) and len(live) > 30
    # the oracle with the same tensors detached
    osd = {k: (v.detach().clone().requires_grad_(True) if k in live else v.detach().clone()) for k, v in sd.items()}
    taps = {}
    oout = O.oracle_step(osd, cfg0, dict(params, device=torch.device("cpu")), batch, taps=taps, cls_dropout=0.0)
    (oout[0] + (ref["Ct"] * taps["seq_t"]).sum() + (ref["Cv"] * taps["seq_v"]).sum()).backward()
    compare_grads(core, {k: osd[k].grad for k in live}, "tiny_L1 frozen, loss + aux", names=live)
    # nothing below the heads has a gradient (both streams, no input request): the heads run, the upstream gradients have nowhere to go --
    # the pass does not fail, launches no add, and the heads' gradients are those of the pass without aux
    for k, p in core.named_parameters():
        p.requires_grad_(is_head(k))
    run_step(model, params, core, batch, None, None)
    plan0 = core._engine.backward_plan()[0]
    assert plan0[0] and not plan0[1] and not plan0[2], plan0
    without = core.flat_grads.clone()
    run_step(model, params, core, batch, ref["Ct"], ref["Cv"])
    left = {k for k, p in core.named_parameters() if p.grad is not None}
    assert left and all(is_head(k) for k in left), sorted(left)[:5]
    for e in core.table:
        if is_head(e.name) and e.used:
            assert torch.equal(bits(without[e.offset:e.offset + e.numel]), bits(core.flat_grads[e.offset:e.offset + e.numel])), e.name


def test_fp8_step_runs_with_the_flag_on_and_aux_in_the_loss():
    """params['fp8'] = True at full width, B 3: finite gradients everywhere (fidelity of the fp8 modes is bounded elsewhere)."""
    cfg = C.vilbert_config(v_feature_size=2048, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, v_hidden_dropout_prob=0.0,
                           v_attention_probs_dropout_prob=0.0)
    model, params = build_model(cfg, C.default_params(fp8=True), weights=None, seed=11)
    model.train()
    core = model.bert_pretrained
    core.return_sequence_outputs = True
    batch = S.make_batch(3, 31, 37, 2048, seed=103)
    gen = torch.Generator().manual_seed(8)
    Ct = torch.randn(3, 31, cfg.hidden_size, generator=gen) * 1e-3
    Cv = torch.randn(3, 37, cfg.v_hidden_size, generator=gen) * 1e-3
    for it in (1, 2):                                         # the first backward pass calibrates the gradient scales
        out, st, sv = run_step(model, params, core, batch, Ct, Cv, it=it)
    assert st.dtype == torch.float32 and bool(torch.isfinite(st).all()) and bool(torch.isfinite(sv).all())
    assert torch.equal(bits(st.detach().bfloat16()), bits(core._engine.tap("seq_t", 3, 31, 37)))
    n = 0
    for k, p in core.named_parameters():
        if p.grad is not None:
            assert bool(torch.isfinite(p.grad).all()), k
            n += int(float(p.grad.abs().max()) > 0)
    assert n > 450
