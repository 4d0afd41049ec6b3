"""CPU: the reference of the masked-LM head's scores (tests/lm_scores_ref.py) against torch autograd of (scores * G).sum(), its emulation
inside its budget, the top-k order against torch.topk and on the values torch leaves open (ties, signed zeros, NaN), and the two new
entry points at the C boundary."""
import ctypes as C
import os
import re

import numpy as np
import torch

import lm_scores_ref as SR
from crct import lib as L
from test_lm_head_ref_cpu import draw

NEW = ("crct_lm_topk_rows", "crct_lm_scores_grad_pack")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def upstream(R, V, seed=5):
    return torch.randn(R, V, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def torch_head(w, seq, rows, G, c):
    p = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    x = seq.clone().requires_grad_(True)
    a = torch.nn.functional.gelu(torch.nn.functional.linear(x[rows], p["W"], p["b"]))
    z = torch.nn.functional.layer_norm(a, (a.shape[1],), p["gamma"], p["beta"], eps=1e-12)
    scores = torch.nn.functional.linear(z, p["E"], p["bias"])
    (scores * (c * G)).sum().backward()
    return scores.detach(), p, x


def test_reference_equals_torch_autograd_of_a_weighted_sum_of_the_scores():
    w, seq, _ = draw()
    N, V = seq.shape[0], w["E"].shape[0]
    for rows, c in ((None, 1.0), (torch.tensor([3, 7, 8, 40]), 0.5)):
        idx = torch.arange(N) if rows is None else rows
        G = upstream(idx.numel(), V)
        ref = SR.reference(w, seq, G, rows, c)
        scores, p, x = torch_head(w, seq, idx, G, c)
        assert tuple(ref["scores"].shape) == (idx.numel(), V)
        assert float((ref["scores"] - scores).abs().max()) <= 1e-12 * max(1.0, float(scores.abs().max()))
        for ours, theirs in (("bias", p["bias"]), ("dense.weight", p["W"]), ("dense.bias", p["b"]), ("LayerNorm.weight", p["gamma"]),
                             ("LayerNorm.bias", p["beta"]), ("decoder", p["E"]), ("d_seq", x)):
            err = float((ref[ours] - theirs.grad).abs().max())
            assert err <= 1e-12 * max(1.0, float(theirs.grad.abs().max())), (ours, err)
    fwd = SR.reference(w, seq)                                                          # forward only: the scores and nothing else
    assert sorted(fwd) == ["rows", "scores"] and torch.equal(fwd["scores"], SR.reference(w, seq, upstream(N, V))["scores"])


def test_emulation_and_budget_bracket_the_bf16_storage():
    w, seq, _ = draw()
    G = upstream(seq.shape[0], w["E"].shape[0])
    ref, emu, bud = SR.reference(w, seq, G), SR.emulate(w, seq, G), SR.budget(w, seq, G)
    for k in SR.OUTPUTS:
        err = (emu[k] - ref[k]).abs()
        assert bool((err <= bud[k]).all()), (k, float((err / bud[k]).max()))
        assert float(bud[k].max()) <= 0.1 * float(ref[k].abs().max()) + 1e-9, k
    assert float((emu["d_seq"] - ref["d_seq"]).abs().max()) > 0.0 and float((emu["scores"] - ref["scores"]).abs().max()) > 0.0


def test_order_is_torch_topk_on_distinct_values():
    g = torch.Generator().manual_seed(9)
    x = torch.randn(7, 130, generator=g)
    x[0, 3], x[1, 5], x[2, 0], x[3, 129] = float("inf"), float("-inf"), 1e-42, -1e-42     # infinities and subnormals are ordinary values
    assert all(len(set(r.tolist())) == 130 for r in x)
    for k in (1, 5, 8, 130):
        assert np.array_equal(SR.topk_ids(x.numpy(), k), torch.topk(x, k, dim=1).indices.numpy())
    labels = torch.randint(0, 130, (7,), generator=g)
    rank = SR.label_rank(x.numpy(), labels.numpy())
    want = (x > x[torch.arange(7), labels][:, None]).sum(1)
    assert np.array_equal(rank, want.numpy())


def test_order_on_ties_signed_zeros_and_nan():
    nan = float("nan")
    neg_nan = np.array([0xFFC00001], dtype=np.uint32).view(np.float32)[0]
    x = np.array([[1.0, 2.0, 2.0, -0.0, 0.0, 2.0, -np.inf, np.inf, nan, -1.0, neg_nan]], dtype=np.float32)
    # NaN (either sign) first, by column; then +inf; the 2.0s by column; 1.0; +0 above -0; -1; -inf
    assert SR.topk_ids(x, 11)[0].tolist() == [8, 10, 7, 1, 2, 5, 0, 4, 3, 9, 6]
    assert SR.label_rank(x, [8])[0] == 0 and SR.label_rank(x, [10])[0] == 1 and SR.label_rank(x, [7])[0] == 2
    assert [int(SR.label_rank(x, [c])[0]) for c in (1, 2, 5)] == [3, 4, 5]              # first, middle and last column of a tie group
    assert SR.label_rank(x, [6])[0] == 10
    key = SR.order_key(x[0])
    assert key[8] == key[10] == 0xFFFFFFFF and key[4] == key[3] + 1 and key.min() > 0
    flat = np.full((1, 9), 0.25, dtype=np.float32)                                     # an all-equal row: the columns in order
    assert SR.topk_ids(flat, 8)[0].tolist() == list(range(8)) and SR.label_rank(flat, [8])[0] == 8


def test_header_declares_the_two_entry_points_under_abi_7():
    text = open(os.path.join(ROOT, "include", "crct_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, text), "%s is not declared in include/crct_hip.h" % name
        assert name in L.PROTOTYPES and L.PROTOTYPES[name][0] is C.c_int
    assert os.path.exists(L.LIB_PATH), "libcrct_hip.so must be built (python -c 'import __graft_entry__ as g; g.build()')"
    raw = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), "%s is not exported" % name
    assert [len(L.PROTOTYPES[n][1]) for n in NEW] == [12, 10]
    assert L.load().crct_abi_version() == 7
