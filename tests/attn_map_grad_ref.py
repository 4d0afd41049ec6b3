"""Host-only yardstick for the backward of an attention map (csrc/attention_probs_bwd.hip, ops.attention_probs_bwd): an fp64 reference with
a per-element error budget, an fp32 / bf16 emulator of the kernel's documented arithmetic with named mutants, and the inputs the CPU and
GPU tests share (the families of attention_ref.make_inputs plus an upstream gradient and the old dq / dk).
tests/test_attn_map_grad_ref_cpu.py proves the yardstick; tests/test_attn_map_grad_kernels_gpu.py holds the kernel to it.

The operation, on bf16 operands (q [B, Tq, heads d], k [B, Tk, heads d], keymask [B, Tk], keep [B heads, Tq, Tk]), an fp32 upstream
gradient G [B, heads, Tq, Tk] of the map M = keep / (1 - p) o P, a scalar c and the old bf16 dq / dk:
    x    = q k^T scale log2e + (1 - keymask) (-10000 log2e)          scale = 1 / sqrt(d); P = softmax_2(x)
    dP   = c G o keep / (1 - p) ;  delta_i = sum_j P_ij dP_ij ;  dS = P o (dP - delta)
    dq   = bf16(dq_old + scale dS k) ;  dk = bf16(dk_old + scale dS^T q)              (accumulate = 0: dq_old = dk_old = 0)

The budget is DERIVED as tests/attention_ref.py derives its own for the recomputing backward, never measured (u = 2^-8 the bf16 unit
roundoff: dS is rounded to bf16 before dS K and dS^T Q; s32 = 2^-16 generous slack for fp32 accumulation order, v_exp_f32, the online
statistics and the one fp32 rounding of c / (1 - p)):
    e_ij = u |dS_ij| + s32 P_ij (|dP_ij| + |delta_i|)
    dq[i,x]  scale sum_j e_ij |k_jx| ;  dk[j,x]  scale sum_i e_ij |q_ix|
on top of one bf16 step at max(|got|, |ref|) for the stored sum (attention_ref.ratio).  The old dq / dk are exact inputs: fp32 holds
the sum of a bf16 number and the fp32 contribution to 2^-24, far inside that step.  Masked keys: x is rounded to fp32 as in
attention_ref.reference (module docstring there).
"""
import math

import numpy as np
import torch

import attention_ref as AR
from attention_ref import LOG2E, MASK_OFF32, S32, U, _heads, _keep, _rb, _rows, assert_within, bf16, ratio      # noqa: F401

MUTANTS = ("delta_dropped", "keep_ignored_on_g", "dropout_scale_once", "scale_missing", "ragged_last_key", "dk_last_qtile", "pad_masked",
           "overwrite")
# (B, heads, Tq, Tk, d): ragged tiles and an odd tile-pair count, Tk % 4 != 0, the zero-filled contraction tail (d = 24, 48), the workgroup
# split (few pairs, many tiles), head size 128, the length limit
SHAPES = [(2, 2, 5, 7, 32), (1, 3, 17, 33, 48), (2, 1, 44, 124, 64), (2, 1, 124, 44, 64), (1, 2, 130, 130, 64), (1, 1, 200, 37, 24),
          (1, 2, 36, 20, 128), (1, 1, 512, 512, 32)]
C_SCALE = 3.0          # the scalar c of the tests: not 1, so that a kernel ignoring it is out by a factor
OLD_STD = 2.0 ** -5    # standard deviation of the old dq / dk: the size of the contributions, so that neither hides the other


def make_case(family, B, heads, Tq, Tk, d, seed=0, mask_offset=0):
    """(q, k, keymask, G, dq_old, dk_old): q / k / keymask of attention_ref.make_inputs, G fp32 randn [B, heads, Tq, Tk], the old
    gradients bf16 randn * OLD_STD [B, T, heads d]."""
    q, k, _, _, km = AR.make_inputs(family, B, heads, Tq, Tk, d, seed=seed, mask_offset=mask_offset)
    g = torch.Generator().manual_seed(7000 + seed)
    G = torch.randn(B, heads, Tq, Tk, generator=g)
    dq0 = bf16(torch.randn(B, Tq, heads * d, generator=g) * OLD_STD)
    dk0 = bf16(torch.randn(B, Tk, heads * d, generator=g) * OLD_STD)
    return q, k, km, G, dq0, dk0


# ------------------------------------------------------------------------------------------- fp64 reference and budget
def probabilities(q, k, keymask, heads, d):
    """fp64 P [B, heads, Tq, Tk] as attention_ref.reference computes it (the masked key's fp32 add included)."""
    qh, kh = (_heads(t, heads, d, torch.float64) for t in (q, k))
    att = torch.as_tensor(keymask).bool()[:, None, None, :]
    x = qh @ kh.transpose(-1, -2) * (LOG2E / math.sqrt(d))
    x = torch.where(att, x, (x + MASK_OFF32).to(torch.float32).to(torch.float64))
    e = torch.exp2(x - x.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


def reference(q, k, keymask, G, c, heads, d, keep=None, p=0.0, dq_old=None, dk_old=None):
    """fp64 (dq, dk) [B, T, heads d] of the operation above and their per-element budgets (the stored sum's bf16 step excluded), as
    ((dq, dk), (budget_dq, budget_dk)); dq_old / dk_old None = accumulate 0."""
    B, Tq, _ = q.shape
    Tk = k.shape[1]
    qh, kh = (_heads(t, heads, d, torch.float64) for t in (q, k))
    scale = 1.0 / math.sqrt(d)
    ds = 1.0 / (1.0 - p) if p > 0 else 1.0
    keepf = _keep(keep, B, heads, Tq, Tk).double() * ds
    P = probabilities(q, k, keymask, heads, d)
    dP = float(c) * G.double() * keepf
    delta = (P * dP).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    dq, dk = _rows(dS @ kh * scale), _rows(dS.transpose(-1, -2) @ qh * scale)
    if dq_old is not None:
        dq = dq + dq_old.double()
    if dk_old is not None:
        dk = dk + dk_old.double()
    e = U * dS.abs() + S32 * P * (dP.abs() + delta.abs())
    return (dq, dk), (_rows(scale * (e @ kh.abs())), _rows(scale * (e.transpose(-1, -2) @ qh.abs())))


# ------------------------------------------------------------------------------------------- emulator
def emulate(q, k, keymask, G, c, heads, d, keep=None, p=0.0, dq_old=None, dk_old=None, mutate=None):
    """The kernel's documented arithmetic in fp32 with its bf16 roundings; returns (dq, dk) as fp64 tensors holding bf16 values.
    x by one fused multiply-add into the exp2 domain; sweep 1 ONLINE over key-tile pairs (32 keys): running maximum m, running sum l and
    dl = sum_j e_ij dP_ij rescaled by exp2(m_old - m_new); P = exp2(x - m) (1 / l), delta = dl (1 / l); dP = G fp32(c / (1 - p)) where kept;
    dS rounded to bf16 before both products; fp32 accumulation; the product times scale plus the old bf16 value, rounded to bf16.

    mutate (one of MUTANTS): the wrong kernels the budget must catch --
      delta_dropped       dS = P o dP, the row term missing
      keep_ignored_on_g   dP = c G / (1 - p) on dropped elements too
      dropout_scale_once  1 / (1 - p) applied to dP in front of the subtraction only: delta summed over c G keep without it
      scale_missing       dq, dk without the factor scale
      ragged_last_key     the last key (Tk - 1, in a ragged tile) missing from both products
      dk_last_qtile       the rows of the last 16-query tile missing from dk
      pad_masked          the padding keys of the last tile pair carry -10000 like masked keys instead of being absent
      overwrite           the old dq / dk ignored: the contribution is written over them"""
    assert mutate is None or mutate in MUTANTS
    B, Tq, _ = q.shape
    Tk = k.shape[1]
    qh, kh = (_heads(t, heads, d, torch.float32) for t in (q, k))
    scale = float(np.float32(1.0) / np.sqrt(np.float32(d)))
    ds = float(np.float32(1.0 / (1.0 - p))) if p > 0 else 1.0
    cds = float(np.float32(c) * np.float32(ds)) if p > 0 else float(np.float32(c))
    kp = _keep(keep, B, heads, Tq, Tk)
    att = torch.as_tensor(keymask).bool()[:, None, None, :]
    sc = float(np.float32(scale) * np.float32(1.4426950408889634))
    x = ((qh @ kh.transpose(-1, -2)).double() * sc + torch.where(att, 0.0, MASK_OFF32)).to(torch.float32)
    Tkp = (Tk + 31) // 32 * 32
    pad_x = MASK_OFF32 if mutate == "pad_masked" else float("-inf")
    x = torch.cat([x, torch.full((B, heads, Tq, Tkp - Tk), pad_x, dtype=torch.float32)], -1)
    Gp = torch.cat([G.float(), torch.zeros(B, heads, Tq, Tkp - Tk)], -1)
    kpp = torch.cat([kp, torch.ones(B, heads, Tq, Tkp - Tk, dtype=torch.bool)], -1)
    kpad = torch.cat([kh, torch.zeros(B, heads, Tkp - Tk, d)], 2)
    dP = Gp * cds if mutate == "keep_ignored_on_g" else torch.where(kpp, Gp * cds, torch.zeros(()))
    dP_delta = torch.where(kpp, Gp * float(np.float32(c)), torch.zeros(())) if mutate == "dropout_scale_once" else dP
    m = torch.full((B, heads, Tq), float("-inf"))
    l = torch.zeros(B, heads, Tq)
    dl = torch.zeros(B, heads, Tq)
    for j0 in range(0, Tkp, 32):
        xs = x[..., j0:j0 + 32]
        mn = torch.maximum(m, xs.max(-1).values)
        alpha = torch.exp2(m - mn)
        e = torch.exp2(xs - mn[..., None])
        l = l * alpha + e.sum(-1)
        dl = dl * alpha + (e * dP_delta[..., j0:j0 + 32]).sum(-1)
        m = mn
    inv = 1.0 / l
    P = torch.exp2(x - m[..., None]) * inv[..., None]
    delta = torch.zeros(B, heads, Tq, 1) if mutate == "delta_dropped" else (dl * inv)[..., None]
    dS = _rb(P * (dP - delta))
    if mutate == "ragged_last_key":
        dS[..., Tk - 1] = 0.0
    dSk = dS.clone()
    if mutate == "dk_last_qtile":
        dSk[:, :, (Tq - 1) // 16 * 16:, :] = 0.0
    so = 1.0 if mutate == "scale_missing" else scale
    dq = _rows((dS @ kpad) * so)
    dk = _rows((dSk.transpose(-1, -2) @ qh)[:, :, :Tk] * so)
    if mutate != "overwrite":
        if dq_old is not None:
            dq = dq + dq_old.float()
        if dk_old is not None:
            dk = dk + dk_old.float()
    return _rb(dq).double(), _rb(dk).double()
