"""Host-only yardstick for the attention-map kernel (csrc/attention_probs.hip): an fp64 reference with a per-element error budget and
an fp32 emulator of the kernel's documented arithmetic with named mutants.  tests/test_attention_probs_ref_cpu.py proves the yardstick
(the emulator stays inside the budget, every mutant leaves it); tests/test_attention_probs_gpu.py holds the kernel to it.  Inputs are
the families of tests/attention_ref.py.

The operation, on bf16 operands (q [B, Tq, heads d], k [B, Tk, heads d], keymask [B, Tk], keep [B heads, Tq, Tk]):
    x = q k^T scale log2e + (1 - keymask) (-10000 log2e)          scale = 1 / sqrt(d); the kernel works in the exp2 domain
    P = keep / (1 - p) softmax_2(x)                               fp32 [B, heads, Tq, Tk]

The budget is DERIVED from where the kernel rounds, never measured:
    |got - ref| <= P_ij (2^-16 + 2 ln2 ulp32(m_i)) + 2^-60
  * 2^-16 is attention_ref's S32: generous slack for the fp32 accumulation of q . k, v_exp_f32, the fp32 row sum and its reciprocal
    (each a few 2^-24) -- 256 times below one bf16 step, it cannot hide a missing term;
  * x is rounded to fp32 once (the fma into the exp2 domain), and so is the row statistic it is compared with: an error of up to half an
    fp32 spacing at |x| in each, 2^(x - m) turns an absolute error e of the exponent into a relative one of ln2 e.  m_i is the largest
    |x_ij| over the keys that decide row i (the attended ones if there are any, else all), ulp32 the fp32 spacing there.  The term is
    2^-10-sized only in fully masked rows, where |x| ~ 14427: the fp32 add of -10000 loses the score's low bits in the kernel and in the
    original model alike, so -- as in attention_ref.reference -- the reference rounds the x of a masked key to fp32 first;
  * 2^-60 admits the flush of probabilities far below the fp32 normal range.  A dropped element is exactly 0 (its budget is 2^-60).
"""
import math

import numpy as np
import torch

from attention_ref import LOG2E, MASK_OFF32, S32, _heads

MUTANTS = ("pad_masked", "ragged_last_key", "no_dropout_scale", "mask_of_batch0", "swapped_qk_lengths")
LN2 = math.log(2.0)


def ulp32(x):
    """fp32 spacing at |x| (fp64 tensor): 2^(exponent - 23); the smallest normal's below it."""
    return torch.exp2(torch.floor(torch.log2(x.double().abs().clamp_min(2.0 ** -126))) - 23)


def _keepf(keep, B, heads, Tq, Tk):
    if keep is None:
        return torch.ones(B, heads, Tq, Tk, dtype=torch.bool)
    return torch.as_tensor(np.asarray(keep)).reshape(B, heads, Tq, Tk).bool()


def reference(q, k, keymask, heads, d, keep=None, p=0.0):
    """(P, budget): fp64 [B, heads, Tq, Tk] each."""
    B, Tq, _ = q.shape
    Tk = k.shape[1]
    qh, kh = _heads(q, heads, d, torch.float64), _heads(k, heads, d, torch.float64)
    ds = 1.0 / (1.0 - p) if p > 0 else 1.0
    att = torch.as_tensor(keymask).bool()[:, None, None, :]
    x = qh @ kh.transpose(-1, -2) * ((1.0 / math.sqrt(d)) * LOG2E)
    x = torch.where(att, x, (x + MASK_OFF32).to(torch.float32).to(torch.float64))      # the masked key's fp32 add (module docstring)
    e = torch.exp2(x - x.max(-1, keepdim=True).values)
    P = e / e.sum(-1, keepdim=True) * (_keepf(keep, B, heads, Tq, Tk).double() * ds)
    any_att = att.any(-1, keepdim=True)
    mag = torch.where(att | ~any_att, x.abs(), torch.zeros((), dtype=torch.float64))   # attended keys if the row has any, else all
    m = mag.max(-1, keepdim=True).values
    budget = P * (S32 + 2.0 * LN2 * ulp32(m)) + 2.0 ** -60
    return P, budget


def ratio(got, ref, budget):
    return (got.double() - ref).abs() / budget


def assert_within(got, ref, budget, what):
    """Every element within its budget; names the first offender.  Returns the largest ratio."""
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), "%s: non-finite output" % what
    r = ratio(got, ref, budget)
    bad = r > 1.0
    assert not bool(bad.any()), "%s: %d elements beyond the budget, first at %s (got %r, fp64 %r, budget %r; worst ratio %.3g)" % (
        what, int(bad.sum()), tuple(int(i) for i in bad.nonzero()[0]), float(got[bad][0]), float(ref[bad][0]), float(budget[bad][0]),
        float(r.max()))
    return float(r.max())


def emulate(q, k, keymask, heads, d, keep=None, p=0.0, mutate=None):
    """The kernel's arithmetic in fp32 (csrc/attention_probs.hip): scores accumulated in fp32 from exact bf16 products, ONE fma into the exp2
    domain with the fp32 constants, keys padded to a multiple of 32 with ABSENT (-inf) keys, sweep 1 over 32-key tile pairs with a running
    maximum m and a running sum l (l <- l exp2(m_old - m_new) + sum exp2(x - m_new)), w = (1 / l) * (1 / (1 - p)), P = exp2(x - m) w or 0.
    Returns fp32 [B, heads, Tq, Tk].

    mutate (one of MUTANTS): the wrong kernels the budget must catch --
      pad_masked          the padding keys of the last tile pair carry -10000 like masked keys instead of being absent
      ragged_last_key     the last real key (Tk - 1) missing from the row: absent from the sum, its probability 0
      no_dropout_scale    1 / (1 - p) missing from the kept probabilities
      mask_of_batch0      batch 0's key mask used for every batch row
      swapped_qk_lengths  Tq / Tk exchanged in the output's index arithmetic (row stride Tq instead of Tk)
    """
    assert mutate is None or mutate in MUTANTS
    B, Tq, _ = q.shape
    Tk = k.shape[1]
    qh, kh = _heads(q, heads, d, torch.float32), _heads(k, heads, d, torch.float32)
    scale = np.float32(1.0) / np.sqrt(np.float32(d))                    # a.scale = 1.0f / sqrtf(d)
    sc = float(np.float32(scale) * np.float32(1.4426950408889634))
    ds = float(np.float32(1.0 / (1.0 - p))) if (p > 0 and mutate != "no_dropout_scale") else 1.0
    km = torch.as_tensor(keymask).bool()
    if mutate == "mask_of_batch0":
        km = km[:1].expand(B, Tk)
    att = km[:, None, None, :]
    s = qh @ kh.transpose(-1, -2)
    x = (s.double() * sc + torch.where(att, 0.0, MASK_OFF32)).to(torch.float32)
    if mutate == "ragged_last_key":
        x[..., Tk - 1] = float("-inf")
    Tkp = (Tk + 31) // 32 * 32
    pad_x = MASK_OFF32 if mutate == "pad_masked" else float("-inf")
    xp = torch.cat([x, torch.full((B, heads, Tq, Tkp - Tk), pad_x, dtype=torch.float32)], -1)
    m = torch.full((B, heads, Tq), float("-inf"))
    l = torch.zeros(B, heads, Tq)
    for j0 in range(0, Tkp, 32):
        xs = xp[..., j0:j0 + 32]
        mn = torch.maximum(m, xs.max(-1).values)
        alpha = torch.where(torch.isinf(mn), torch.zeros(()), torch.exp2(m - mn))      # (only the mutant that removes a lone key gets here)
        l = l * alpha + torch.where(torch.isinf(xs), torch.zeros(()), torch.exp2(xs - mn[..., None])).sum(-1)
        m = mn
    w = (1.0 / l) * np.float32(ds)
    P = torch.exp2(x - m[..., None]) * w[..., None]
    P = torch.where(torch.isinf(x), torch.zeros(()), P)
    P = torch.where(_keepf(keep, B, heads, Tq, Tk), P, torch.zeros(()))
    if mutate == "swapped_qk_lengths":
        flat = torch.zeros(B, heads, Tq * Tk + Tk)
        for i in range(Tq):
            if i * Tq < Tq * Tk:
                flat[..., i * Tq:i * Tq + Tk] = P[:, :, i, :]
        P = flat[..., :Tq * Tk].reshape(B, heads, Tq, Tk)
    return P
