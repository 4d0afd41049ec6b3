"""CPU: the masked-region head's reference against torch autograd (hard: CrossEntropyLoss; soft: kl_div(log_softmax(x), t,
reduction='none') summed per row and divided by max(n, 1)), zeros in the soft targets, and what params['img_loss_coeff'] changes in the
layout and at the C boundary -- the ``used`` flags of the six head tensors and nothing else."""
import ctypes as C
import os
import re

import pytest
import torch

import region_head_ref as R
from crct import config as CFG
from crct import lib as L
from crct.layout import frozen_names, is_language_weight, is_unused, parameter_table

HEAD = ("cls.imagePredictions.transform.dense.weight", "cls.imagePredictions.transform.dense.bias",
        "cls.imagePredictions.transform.LayerNorm.weight", "cls.imagePredictions.transform.LayerNorm.bias",
        "cls.imagePredictions.decoder.weight", "cls.imagePredictions.decoder.bias")
NEW = ("crct_region_ce_fwd", "crct_region_ce_bwd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def draw(Cn=17, H=96, N=36, seed=3, std=0.3, soft=False):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    w = dict(D=rn(Cn, H) * std, d=rn(Cn) * std, W=rn(H, H) * std, b=rn(H) * std, gamma=1.0 + rn(H) * std, beta=rn(H) * std)
    seq = rn(N, H)
    label = torch.full((N,), -1, dtype=torch.int64)
    label[::9] = 0                                                     # the <IMG> rows
    rows = torch.randperm(N, generator=g)[:N // 4]
    rows = rows[rows % 9 != 0]
    label[rows] = 1
    if soft:
        t = torch.rand(N, Cn, generator=g, dtype=torch.float64)
        t[torch.rand(N, Cn, generator=g) < 0.3] = 0.0                  # zeros: terms that must vanish
        t = t / t.sum(1, keepdim=True)
        t[rows[0]] *= 0.5                                              # a row that does not sum to 1
        t[rows[1]] = 0.0
        t[rows[1], 3] = 1.0                                            # a one-hot row
        return w, seq, label, t
    ids = torch.randint(0, Cn, (N,), generator=g)
    ids[rows[0]], ids[rows[1]] = 0, Cn - 1
    return w, seq, label, ids


def torch_head(w, seq):
    p = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    x = seq.clone().requires_grad_(True)
    a = torch.nn.functional.gelu(torch.nn.functional.linear(x, p["W"], p["b"]))
    z = torch.nn.functional.layer_norm(a, (a.shape[1],), p["gamma"], p["beta"], eps=1e-12)
    return p, x, torch.nn.functional.linear(z, p["D"], p["d"])


def compare(ref, p, x, loss):
    loss.backward()
    assert float((ref["loss"] - loss.detach()).abs()) <= 1e-12
    for ours, theirs in (("decoder.bias", p["d"]), ("dense.weight", p["W"]), ("dense.bias", p["b"]), ("LayerNorm.weight", p["gamma"]),
                         ("LayerNorm.bias", p["beta"]), ("decoder.weight", p["D"]), ("d_seq", x)):
        err = float((ref[ours] - theirs.grad).abs().max())
        assert err <= 1e-12 * max(1.0, float(theirs.grad.abs().max())), (ours, err)


def test_hard_reference_equals_torch_autograd_of_cross_entropy():
    w, seq, label, ids = draw()
    ref = R.reference(w, seq, label, ids)
    p, x, scores = torch_head(w, seq)
    rows = (label == 1).nonzero().flatten()
    loss = torch.nn.CrossEntropyLoss(reduction="sum")(scores[rows], ids[rows]) / max(int(rows.numel()), 1)
    compare(ref, p, x, loss)
    assert float(ref["d_seq"][label != 1].abs().max()) == 0.0
    ref3 = R.reference(w, seq, label, ids, g=3.0)                      # an upstream scalar scales every gradient and leaves the loss
    assert torch.equal(ref3["loss"], ref["loss"])
    assert float((ref3["decoder.weight"] - 3.0 * ref["decoder.weight"]).abs().max()) <= 1e-12


def test_soft_reference_equals_torch_autograd_of_kl_div():
    w, seq, label, t = draw(soft=True)
    ref = R.reference(w, seq, label, t)
    p, x, scores = torch_head(w, seq)
    rows = (label == 1).nonzero().flatten()
    kl = torch.nn.functional.kl_div(torch.log_softmax(scores[rows], 1), t[rows], reduction="none")
    compare(ref, p, x, kl.sum(1).sum() / max(int(rows.numel()), 1))
    # a one-hot soft target is the hard form
    ids = torch.zeros(seq.shape[0], dtype=torch.int64)
    ids[rows] = torch.arange(rows.numel()) % t.shape[1]
    onehot = torch.zeros_like(t)
    onehot[torch.arange(seq.shape[0]), ids] = 1.0
    a, b = R.reference(w, seq, label, onehot), R.reference(w, seq, label, ids)
    for k in R.OUTPUTS:
        assert float((a[k] - b[k]).abs().max()) <= 1e-12 * max(1.0, float(b[k].abs().max())), k


def test_zeros_in_the_soft_targets_give_zero_terms_and_finite_gradients():
    w, seq, label, t = draw(soft=True)
    rows = (label == 1).nonzero().flatten()
    assert int((t[rows] == 0).sum()) > 0
    ref = R.reference(w, seq, label, t)
    assert all(bool(torch.isfinite(ref[k]).all()) for k in R.OUTPUTS + ("loss_rows",))
    logits = torch.randn(4, 17, dtype=torch.float64)
    tt = torch.zeros(4, 17, dtype=torch.float64)
    tt[0, 2], tt[1, 5], tt[1, 6] = 1.0, 0.25, 0.75                     # rows 2 and 3: all zero
    loss, grad, _ = R.row_losses(logits, tt)
    assert float(loss[2]) == 0.0 and float(loss[3]) == 0.0 and float(grad[2:].abs().max()) == 0.0
    logp = torch.log_softmax(logits, 1)
    assert abs(float(loss[0]) + float(logp[0, 2])) <= 1e-14
    want = 0.25 * (torch.log(torch.tensor(0.25, dtype=torch.float64)) - logp[1, 5]) + 0.75 * (torch.log(torch.tensor(0.75, dtype=torch.float64)) - logp[1, 6])
    assert abs(float(loss[1]) - float(want)) <= 1e-14


@pytest.mark.parametrize("soft", (False, True))
def test_emulation_and_budget_bracket_the_bf16_storage(soft):
    args = draw(soft=soft)
    ref, emu, bud = R.reference(*args), R.emulate(*args), R.budget(*args)
    for k in R.OUTPUTS:
        err = (emu[k] - ref[k]).abs()
        assert bool((err <= bud[k]).all()), (k, float((err / bud[k]).max()))
        assert float(bud[k].max()) <= 0.1 * float(ref[k].abs().max()) + 1e-9, k        # ... and the budget is no blank cheque
    assert float((emu["d_seq"] - ref["d_seq"]).abs().max()) > 0.0


def _table(**extra):
    return parameter_table(CFG.tiny_config(), CFG.default_params(categories=9, **extra))


@pytest.mark.parametrize("lm", (None, 0.5))
def test_option_off_is_todays_table_and_on_moves_only_six_used_flags(lm):
    base = {} if lm is None else dict(lm_loss_coeff=lm)
    t_off, total_off = _table(**base)
    for off_value in (0.0, None):
        assert _table(img_loss_coeff=off_value, **base) == (t_off, total_off)
    assert all(not e.used for e in t_off if e.name.startswith("cls.imagePredictions."))
    t_on, total_on = _table(img_loss_coeff=0.5, **base)
    assert total_on == total_off and len(t_on) == len(t_off)
    assert sorted(a.name for a, b in zip(t_off, t_on) if a != b) == sorted(HEAD)
    for a, b in zip(t_off, t_on):
        assert a._replace(used=True) == b._replace(used=True)        # offsets, shapes, decay and language flags do not move
        assert b.used == (a.used or a.name in HEAD)
    assert all(e.used and not e.language and not is_language_weight(e.name) for e in t_on if e.name in HEAD)      # they train at image_lr
    # the six sit directly behind the masked-LM head's tensors, at the very end of the buffers
    by = {e.name: e for e in t_on}
    lm_end = max(e.offset + e.numel for e in t_on if e.name.startswith("cls.predictions."))
    first = min(by[n].offset for n in HEAD)
    assert lm_end <= first < lm_end + 64 and max(by[n].offset + by[n].numel for n in HEAD) <= total_on < max(by[n].offset + by[n].numel for n in HEAD) + 64
    assert is_unused("cls.imagePredictions.decoder.weight") and is_unused("cls.imagePredictions.decoder.weight", {})
    assert not is_unused("cls.imagePredictions.decoder.weight", dict(img_loss_coeff=1.0)) and is_unused("cls.predictions.bias", dict(img_loss_coeff=1.0))


def test_frozen_names_drops_exactly_the_six():
    cfg = CFG.tiny_config()
    off = frozen_names(cfg, CFG.default_params(categories=9))
    on = frozen_names(cfg, CFG.default_params(categories=9, img_loss_coeff=1.0))
    assert sorted(set(off) - set(on)) == sorted(HEAD) and set(on) <= set(off)


def test_header_declares_the_entry_points_under_abi_7():
    text = open(os.path.join(ROOT, "include", "crct_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, text), "%s is not declared in include/crct_hip.h" % name
        assert name in L.PROTOTYPES and L.PROTOTYPES[name][0] is C.c_int
    assert os.path.exists(L.LIB_PATH), "libcrct_hip.so must be built (python -c 'import __graft_entry__ as g; g.build()')"
    raw = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), "%s is not exported" % name
    assert [len(L.PROTOTYPES[n][1]) for n in NEW] == [12, 15]
    assert L.load().crct_abi_version() == 7
