"""CPU: the masked-LM head's reference against torch autograd, and what params['lm_loss_coeff'] changes in the layout and at the C
boundary -- the ``used`` flags of the five head tensors and nothing else."""
import ctypes as C
import os
import re

import torch

import lm_head_ref as R
from crct import config as CFG
from crct import lib as L
from crct.layout import frozen_names, is_unused, parameter_table

HEAD = ("cls.predictions.bias", "cls.predictions.transform.dense.weight", "cls.predictions.transform.dense.bias",
        "cls.predictions.transform.LayerNorm.weight", "cls.predictions.transform.LayerNorm.bias")
NEW = ("crct_lm_gather_rows", "crct_lm_scatter_rows", "crct_lm_pad_operands", "crct_lm_ce_fwd", "crct_lm_ce_bwd", "crct_lm_add_f32",
       "crct_lm_gelu_bwd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def draw(V=130, H=64, N=48, seed=3, std=0.3):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    w = dict(E=rn(V, H) * std, bias=rn(V) * std, W=rn(H, H) * std, b=rn(H) * std, gamma=1.0 + rn(H) * std, beta=rn(H) * std)
    seq = rn(N, H)
    labels = torch.full((N,), -1, dtype=torch.int64)
    rows = torch.randperm(N, generator=g)[:N // 4]
    labels[rows] = torch.randint(0, V, (rows.numel(),), generator=g)
    labels[rows[0]], labels[rows[1]] = 0, V - 1
    return w, seq, labels


def test_reference_equals_torch_autograd_of_cross_entropy_ignore_index():
    w, seq, labels = draw()
    ref = R.reference(w, seq, labels, g=1.0)
    p = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    x = seq.clone().requires_grad_(True)
    a = torch.nn.functional.gelu(torch.nn.functional.linear(x, p["W"], p["b"]))
    z = torch.nn.functional.layer_norm(a, (a.shape[1],), p["gamma"], p["beta"], eps=1e-12)
    scores = torch.nn.functional.linear(z, p["E"], p["bias"])
    loss = torch.nn.CrossEntropyLoss(ignore_index=-1)(scores.view(-1, scores.shape[-1]), labels.view(-1))
    loss.backward()
    assert float((ref["loss"] - loss.detach()).abs()) <= 1e-12
    for ours, theirs in (("bias", p["bias"]), ("dense.weight", p["W"]), ("dense.bias", p["b"]), ("LayerNorm.weight", p["gamma"]),
                         ("LayerNorm.bias", p["beta"]), ("decoder", p["E"]), ("d_seq", x)):
        err = float((ref[ours] - theirs.grad).abs().max())
        assert err <= 1e-12 * max(1.0, float(theirs.grad.abs().max())), (ours, err)
    # an upstream scalar scales every gradient and leaves the loss
    ref3 = R.reference(w, seq, labels, g=3.0)
    assert torch.equal(ref3["loss"], ref["loss"])
    assert float((ref3["decoder"] - 3.0 * ref["decoder"]).abs().max()) <= 1e-12


def test_emulation_and_budget_bracket_the_bf16_storage():
    w, seq, labels = draw()
    ref, emu, bud = R.reference(w, seq, labels), R.emulate(w, seq, labels), R.budget(w, seq, labels)
    for k in R.OUTPUTS:
        err = (emu[k] - ref[k]).abs()
        assert bool((err <= bud[k]).all()), (k, float((err / bud[k]).max()))
        assert float(bud[k].max()) <= 0.1 * float(ref[k].abs().max()) + 1e-9, k        # ... and the budget is no blank cheque
    assert float((emu["d_seq"] - ref["d_seq"]).abs().max()) > 0.0                       # the roundings are really applied


def _tables(**extra):
    cfg = CFG.tiny_config()
    off = parameter_table(cfg, CFG.default_params(categories=9))
    on = parameter_table(cfg, CFG.default_params(categories=9, **extra))
    return cfg, off, on


def test_option_off_is_todays_table_and_on_moves_only_five_used_flags():
    cfg, (t_off, total_off), (t_zero, total_zero) = _tables(lm_loss_coeff=0.0)
    assert t_off == t_zero and total_off == total_zero
    assert all(not e.used for e in t_off if e.name.startswith("cls.predictions."))
    _, _, (t_on, total_on) = _tables(lm_loss_coeff=0.5)
    assert total_on == total_off and len(t_on) == len(t_off)
    changed = [a.name for a, b in zip(t_off, t_on) if a != b]
    assert sorted(changed) == sorted(HEAD)
    for a, b in zip(t_off, t_on):
        assert a._replace(used=True) == b._replace(used=True)        # offsets, shapes, decay and language flags do not move
        assert b.used == (a.used or a.name in HEAD)
    assert is_unused("cls.predictions.bias") and is_unused("cls.predictions.bias", {}) and is_unused("cls.imagePredictions.decoder.weight", dict(lm_loss_coeff=1.0))


def test_frozen_names_drops_exactly_the_five():
    cfg = CFG.tiny_config()
    off = frozen_names(cfg, CFG.default_params(categories=9))
    on = frozen_names(cfg, CFG.default_params(categories=9, lm_loss_coeff=1.0))
    assert [n for n in off if n not in on] == [n for n in off if n in HEAD] and sorted(set(off) - set(on)) == sorted(HEAD)
    assert set(on) <= set(off)


def test_header_declares_the_entry_points_under_abi_7():
    text = open(os.path.join(ROOT, "include", "crct_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, text), "%s is not declared in include/crct_hip.h" % name
        assert name in L.PROTOTYPES and L.PROTOTYPES[name][0] is C.c_int
    assert os.path.exists(L.LIB_PATH), "libcrct_hip.so must be built (python -c 'import __graft_entry__ as g; g.build()')"
    raw = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), "%s is not exported" % name
    assert [len(L.PROTOTYPES[n][1]) for n in NEW] == [7, 6, 8, 10, 13, 5, 5]
    assert L.load().crct_abi_version() == 7
