"""The score-gradient yardstick (tests/score_grad_ref.py) proved on the CPU: the fp32 emulator of heads.hip's order, extended by the two
additions (c Gl onto dlogit, c Gv R3 (1 - r^2) onto dz), stays within a quarter of every budget on the cases
tests/test_score_grad_kernels_gpu.py runs; every named mutant leaves a budget; the fp64 restatement agrees with plain autograd on an
independent statement of the objective; the shared inputs meet their conditions.  No GPU."""
import functools

import numpy as np
import pytest
import torch

import heads_ref as H
import score_grad_ref as SG

F32 = np.float32


@functools.lru_cache(maxsize=None)
def _case(B, Hb):
    return SG.inputs(B, Hb, seed=B * 11 + Hb)


def _setup(B, Hb, i):
    fusion_sum, p, use_l1, kind_l1, up, gs, lab_kind = SG.COMBOS[i]
    inp = _case(B, Hb)
    hc = H.head_cfg(p=p, seed=H.DROP_SEEDS[i % 2] + B, fusion_sum=fusion_sum, use_l1=use_l1, kind_l1=kind_l1)
    R = SG.targets(inp, hc, seed=B)
    labels = H.make_labels(B, torch.Generator().manual_seed(B), lab_kind)
    keep = H.host_keep(hc, B, Hb)
    return inp, hc, R, labels, keep, H.upstream(up, B, gs), gs


def _run(B, Hb, i, which, mutate=None, mode="plotqa", worst=None, frac=0.25):
    inp, hc, R, labels, keep, (g_loss, g_nsp, g_reg, gn64, gr64), gs = _setup(B, Hb, i)
    Gl, Gv = SG.score_upstream(B, which)
    pre = SG.prefill(B, Hb)
    what = "B=%d Hb=%d combo %d %s" % (B, Hb, i, which)
    emu = SG.emu_scores(inp, R, labels, keep, hc, gs, g_loss, g_nsp, g_reg, Gl, None if mode == "none" else Gv, prefill=pre, mode=mode, mutate=mutate)
    if mode == "none":
        _, grads, mags = SG.none_ref64(inp, R, labels, keep, hc, g_nsp=gn64, Gl=Gl, c=gs)
        return SG.check_grads(emu, grads, mags, pre, what, worst, frac, keys=("d_pt", "d_pv", "d_w_cls", "d_b_cls"))
    snap = dict(snap_table=H.DVQA_FLOATS, r32=H.emu_tanh_r(inp)) if mode == "snap" else {}
    out, grads, mags = SG.plotqa_ref64(inp, R, labels, keep, hc, g_nsp=gn64, g_reg=gr64, Gl=Gl, Gv=Gv, c=gs, **snap)
    failed = SG.check_grads(emu, grads, mags, pre, what, worst, frac)
    try:
        H.assert_within(emu["logits"], out["logits"], out["logit_mag"], what + ": logits", worst=worst, frac=frac)
        H.assert_within(emu["dl"], _dl64(out, labels, gn64, Gl, gs), mags["dl"], what + ": dlogits", worst=worst, frac=frac)
    except AssertionError as e:
        failed.append(str(e))
    return failed


def _dl64(out, labels, gn64, Gl, c):
    B = out["logits"].shape[0]
    dl = torch.zeros(B, 2, dtype=torch.float64)
    if labels is not None:
        valid = (labels != -1).double()[:, None]
        onehot = torch.nn.functional.one_hot(labels.clamp_min(0), 2).double()
        dl = (torch.softmax(out["logits"], 1) - onehot) * valid * gn64 / max(int(valid.sum()), 1)
    return dl + (c * Gl.double() if Gl is not None else 0)


@pytest.mark.parametrize("B,Hb", SG.SHAPES)
def test_emulator_stays_within_a_quarter_of_every_budget(B, Hb):
    """Every shape, setting and upstream of the GPU test, PlotQA, snap and NONE: |emulator - fp64| <= 0.25 budget for the fp32 outputs;
    the bf16 seeds are held to 0.51, since a correctly rounded bf16 lies up to half a step from fp64 whatever came before it."""
    worst = {}
    for i in range(len(SG.COMBOS)):
        for which in SG.WHICH:
            assert not _run(B, Hb, i, which, worst=worst)
        assert not _run(B, Hb, i, "logits", mode="none", worst=worst)
        assert not _run(B, Hb, i, "both", mode="snap", worst=worst)
    print("B=%d Hb=%d " % (B, Hb) + " ".join("%s %.4f" % kv for kv in sorted(worst.items())))


@pytest.mark.parametrize("mutant", SG.MUTANTS)
def test_every_mutant_is_caught_at_the_budget(mutant):
    """B = 7, Hb = 64 suffices: each mutant leaves the full budget of some gradient in some combination."""
    B, Hb = 7, 64
    mode = "snap" if mutant == "snap_not_constant" else "plotqa"
    caught = []
    for i in range(len(SG.COMBOS)):
        caught += _run(B, Hb, i, "both", mutate=mutant, mode=mode, frac=1.0)
    assert caught, "mutant %s passes every check" % mutant
    print(mutant, "caught by", sorted({c.split(": ")[1].split(":")[0] for c in caught}))


def test_restatement_against_plain_autograd():
    """The objective written out once more without heads_ref: logits = dropout(fuse(pt, pv)) W^T + b, value = tanh(fh . w6 + b6) R3 on the
    needs rows; the gradients of sum(Gl logits) + sum(Gv value) alone (zero loss seeds) equal the restatement's."""
    B, Hb = 7, 64
    inp, hc, R, labels, keep, _, _ = _setup(B, Hb, 0)
    Gl, Gv = SG.score_upstream(B, "both")
    c = 0.25
    _, grads, mags = SG.plotqa_ref64(inp, R, labels, keep, hc, g_nsp=0.0, g_reg=torch.zeros(B, dtype=torch.float64), Gl=Gl, Gv=Gv, c=c)
    pt, pv, fh = (inp[k].double().requires_grad_(True) for k in ("pt", "pv", "fh"))
    W, bc, w6, b6 = (inp[k].double().requires_grad_(True) for k in ("w_cls", "b_cls", "w6", "b6"))
    logits = (pt * pv) @ W.t() + bc
    needs = R[:, 1] == 1
    value = torch.tanh(fh @ w6 + b6) * R[:, 3].double() * needs
    (c * (Gl.double() * logits).sum() + c * (Gv.double() * value).sum()).backward()
    slope = torch.where(fh.detach() > 0, 1.0, 0.01)
    want = dict(d_pt=pt.grad * (pt.detach() > 0), d_pv=pv.grad * (pv.detach() > 0), d_fh=fh.grad * slope, d_w_cls=W.grad, d_b_cls=bc.grad,
                d_w6=w6.grad, d_b6=b6.grad)
    for k, w in want.items():
        assert torch.allclose(grads[k], w, rtol=1e-12, atol=1e-300), k
    assert float(grads["d_fh"][~needs].abs().max()) == 0.0 and float(mags["d_fh"][~needs].abs().max()) == 0.0
    assert float(grads["d_fh"][needs].abs().min(1).values.min()) > 0.0          # |target| > 1 rows included: the value's upstream flows


def test_inputs_meet_their_conditions():
    B, Hb = 7, 64
    inp = _case(B, Hb)
    hc = H.head_cfg()
    R = SG.targets(inp, hc, seed=B)
    r = H.emu_tanh_r(inp)
    assert abs(np.arctanh(np.float64(r[SG.BIG_ROW])) - SG.BIG_Z) < 0.05 and 1 - float(r[SG.BIG_ROW]) ** 2 < 0.0109
    kinds = inp["kinds"]
    needs = R[:, 1] == 1
    assert not bool(needs[kinds == H._S_NEEDS0].any()) and bool(needs[kinds != H._S_NEEDS0].all())
    assert bool(((R[:, 0] / R[:, 3]).abs()[kinds == H._S_BIG] > 1).all()) and bool((kinds == H._S_BIG).any())
    labels = H.make_labels(B, torch.Generator().manual_seed(B))
    assert bool((labels == -1).any()) and bool((labels != -1).any())
    for Bx in (1, 7, 300):
        Gl, Gv = SG.score_upstream(Bx, "both")
        assert float(Gl.abs().min()) > 0 and float(Gv.abs().min()) > 0
        assert float(Gl.min()) < 0 < float(Gl.max()) and (Bx == 1 or float(Gv.min()) < 0 < float(Gv.max()))
    Gl, Gv = SG.score_upstream(B, "both")
    assert float(Gv[kinds == H._S_NEEDS0].abs().min()) > 0 and float(Gv[kinds == H._S_BIG].abs().min()) > 0
    assert {c[5] for c in SG.COMBOS} == {1.0, 0.25} and {c[4] for c in SG.COMBOS} == {"default", "loss_dev", "nsp_reg_dev"}


# ------------------------------------------------------------------------------------------- the C boundary
def test_new_entry_points_are_exported_and_mirrored_under_abi_7():
    import ctypes as C
    import os
    import re
    from crct import lib as L
    new = ("crct_head_loss_scores", "crct_head_loss_variant_scores", "crct_engine_set_score_grads")
    assert os.path.exists(L.LIB_PATH), "libcrct_hip.so must be built (python -c 'import __graft_entry__ as g; g.build()')"
    raw = C.CDLL(L.LIB_PATH)
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "crct_hip.h")).read()
    for name in new:
        assert hasattr(raw, name), "%s is not exported" % name
        assert name in L.PROTOTYPES and L.PROTOTYPES[name][0] is C.c_int, name
        assert re.search(r"\bint %s\(" % name, text), "%s is not declared in include/crct_hip.h" % name
    assert [len(L.PROTOTYPES[n][1]) for n in new] == [3, 3, 2]
    assert L.load().crct_abi_version() == 7
    assert C.sizeof(L.ScoreGrads) == 16 and [f[0] for f in L.ScoreGrads._fields_] == ["d_logits", "d_value"]
    assert L.ScoreGrads.d_logits.offset == 0 and L.ScoreGrads.d_value.offset == 8
    # no struct of the ABI changed: the two argument structs keep their prototypes
    assert L.PROTOTYPES["crct_head_loss"][1][0]._type_ is L.HeadArgs and L.PROTOTYPES["crct_head_loss_scores"][1][0]._type_ is L.HeadArgs
