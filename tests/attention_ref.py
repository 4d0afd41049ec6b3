"""Host-only yardstick for the attention kernels (csrc/attention.hip, attention_mfma.hip, attention_long.hip): an fp64 reference with a
per-element error budget, an fp32 / bf16 emulator of the kernels' documented arithmetic with named mutants, and the input families
the CPU and GPU tests share.  tests/test_attention_ref_cpu.py proves the yardstick (the emulator stays inside the budget, every
mutant leaves it); tests/test_attention_gpu.py holds the kernels to it.

The operation, on bf16 operands (q [B, Tq, heads d], k / v [B, Tk, heads d], keymask [B, Tk], keep [B heads, Tq, Tk]):
    x    = q k^T scale log2e + (1 - keymask) (-10000 log2e)          scale = 1 / sqrt(d); the kernels work in the exp2 domain
    P    = softmax_2(x) ;  Pd = P o keep / (1 - p) ;  ctx = Pd v
    dP   = (dctx v^T) o keep / (1 - p) ;  delta_i = sum_j P_ij dP_ij ;  dS = P o (dP - delta)
    dq   = scale dS k ;  dk = scale dS^T q ;  dv = Pd^T dctx

The budget is DERIVED from where the kernels round, never measured.  u = 2^-8 is the bf16 unit roundoff, s32 = 2^-16 generous
slack for fp32 accumulation order, v_exp_f32 and the fp32 lse (256 times smaller than u: it cannot hide a missing term).  On top of one
bf16 step at max(|got|, |ref|) for the stored output (`step`, added by `ratio` / `assert_within`):
    ctx[i,c]   (u + s32) sum_j Pd_ij |v_jc|                     the probabilities are rounded to bf16 before P V
    dv[j,c]    (u + s32) sum_i Pd_ij |dctx_ic|
    dq[i,c]    scale sum_j e_ij |k_jc| ;  dk[j,c]  scale sum_i e_ij |q_ic|
               e_ij = u |dS_ij| + s32 P_ij (|dP_ij| + |delta_i|)      dS is rounded to bf16 before dS K and dS^T Q
    kept statistics (the backward reads delta_i = dctx_i . ctx_i from the forward's bf16 ctx): e_ij gains
               P_ij u sum_c |dctx_ic| (|ctx_ic| + sum_j Pd_ij |v_jc|)
The fp32 VALU kernels round less and sit further inside the same budget.

Fully masked batch rows: every key carries -10000, and x = s scale log2e - 10000 log2e is rounded to fp32 where the spacing is
2^-10 -- in the kernels and in the original model's fp32 add alike.  That loss belongs to the model, so the reference rounds the x of a
masked key to fp32 (with the kernels' fp32 constant) before it exponentiates.
"""
import math

import numpy as np
import torch

U = 2.0 ** -8
S32 = 2.0 ** -16
LOG2E = math.log2(math.e)
MASK_OFF32 = float(np.float32(-10000.0) * np.float32(1.4426950408889634))      # the kernels' fp32 constant -10000.f * log2e
FAMILIES = ("flat", "peaked", "late_max", "early_max", "masks")
MUTANTS = ("delta_dropped", "no_rescale_last", "dv_no_scale", "ragged_last_key", "dk_last_qtile", "pad_masked")
OUTPUTS = ("ctx", "dq", "dk", "dv")


# ------------------------------------------------------------------------------------------- helpers
def bf16(x):
    return x.to(torch.float32).to(torch.bfloat16)


def _rb(x):
    """fp32 -> bf16 -> fp32: a bf16 rounding inside the fp32 emulation."""
    return x.to(torch.bfloat16).to(torch.float32)


def _heads(t, heads, d, dtype):
    """[B, T, heads d] -> [B, heads, T, d]"""
    B, T, _ = t.shape
    return t.to(dtype).reshape(B, T, heads, d).permute(0, 2, 1, 3).contiguous()


def _rows(t):
    """[B, heads, T, d] -> [B, T, heads d]"""
    B, H, T, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, T, H * d)


def _keep(keep, B, heads, Tq, Tk):
    if keep is None:
        return torch.ones(B, heads, Tq, Tk, dtype=torch.bool)
    return torch.as_tensor(np.asarray(keep)).reshape(B, heads, Tq, Tk).bool()


def bf16_step(x):
    """Spacing of the bf16 numbers at |x| (fp64): 2^(exponent - 7); the smallest normal's below it."""
    return torch.exp2(torch.floor(torch.log2(x.double().abs().clamp_min(2.0 ** -126))) - 7)


def ratio(got, ref, budget):
    """|got - ref| / (one bf16 step at max(|got|, |ref|) + budget), per element (fp64)."""
    got, ref = got.double(), ref.double()
    return (got - ref).abs() / (bf16_step(torch.maximum(got.abs(), ref.abs())) + budget)


def assert_within(got, ref, budget, what):
    """Every element within its budget; names the first offender.  Returns the largest ratio."""
    got, ref = got.double().cpu(), ref.double()
    assert bool(torch.isfinite(got).all()), "%s: non-finite output" % what
    r = ratio(got, ref, budget)
    bad = r > 1.0
    assert not bool(bad.any()), "%s: %d elements beyond the budget, first at %s (got %r, fp64 %r, budget %r + bf16 step; worst ratio %.3f)" % (
        what, int(bad.sum()), tuple(int(i) for i in bad.nonzero()[0]), float(got[bad][0]), float(ref[bad][0]), float(budget[bad][0]),
        float(r.max()))
    return float(r.max())


# ------------------------------------------------------------------------------------------- fp64 reference and budget
def reference(q, k, v, keymask, dctx, heads, d, keep=None, p=0.0, ctx_bf16=None):
    """fp64 ctx, dq, dk, dv ([B, T, heads d]) and lse ([B, heads, Tq], log2 sum_j exp2 x_ij) of the operation above on the given (bf16)
    operands and keep mask, with `budget`: a dict of per-element fp64 budgets (the stored output's bf16 step excluded) -- 'ctx', 'dq',
    'dk', 'dv' for a backward that recomputes its statistics and 'dq_kept', 'dk_kept' for one that reads lse and the forward's bf16
    ctx (ctx_bf16, default: the reference's own ctx)."""
    B, Tq, _ = q.shape
    Tk = k.shape[1]
    qh, kh, vh, gh = (_heads(t, heads, d, torch.float64) for t in (q, k, v, dctx))
    scale = 1.0 / math.sqrt(d)
    ds = 1.0 / (1.0 - p) if p > 0 else 1.0
    keepf = _keep(keep, B, heads, Tq, Tk).double() * ds
    att = torch.as_tensor(keymask).bool()[:, None, None, :]
    x = qh @ kh.transpose(-1, -2) * (scale * LOG2E)
    x = torch.where(att, x, (x + MASK_OFF32).to(torch.float32).to(torch.float64))      # the masked key's fp32 add (module docstring)
    mx = x.max(-1, keepdim=True).values
    e = torch.exp2(x - mx)
    l = e.sum(-1, keepdim=True)
    P = e / l
    lse = (mx + torch.log2(l)).squeeze(-1)
    Pd = P * keepf
    ctx = Pd @ vh
    dP = (gh @ vh.transpose(-1, -2)) * keepf
    delta = (P * dP).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    out = dict(ctx=_rows(ctx), dq=_rows(dS @ kh * scale), dk=_rows(dS.transpose(-1, -2) @ qh * scale), dv=_rows(Pd.transpose(-1, -2) @ gh),
               lse=lse)
    pv = Pd @ vh.abs()                                                                  # sum_j Pd_ij |v_jc|
    e_rec = U * dS.abs() + S32 * P * (dP.abs() + delta.abs())
    cb = ctx.abs() if ctx_bf16 is None else _heads(ctx_bf16, heads, d, torch.float64).abs()
    e_kept = e_rec + P * (U * (gh.abs() * (cb + pv)).sum(-1, keepdim=True))
    out["budget"] = dict(
        ctx=_rows((U + S32) * pv), dv=_rows((U + S32) * (Pd.transpose(-1, -2) @ gh.abs())),
        dq=_rows(scale * (e_rec @ kh.abs())), dk=_rows(scale * (e_rec.transpose(-1, -2) @ qh.abs())),
        dq_kept=_rows(scale * (e_kept @ kh.abs())), dk_kept=_rows(scale * (e_kept.transpose(-1, -2) @ qh.abs())))
    return out


def budget_of(ref, name, kept):
    return ref["budget"][name + "_kept" if kept and name in ("dq", "dk") else name]


# ------------------------------------------------------------------------------------------- emulator
def emulate(q, k, v, keymask, dctx, heads, d, keep=None, p=0.0, path="mfma", kept=False, mutate=None):
    """The same operation as the kernels document it, in fp32 with their bf16 roundings.  Returns ctx, dq, dk, dv (fp64 tensors holding
    bf16 values, [B, T, heads d]) and lse (fp32 [B, heads, Tq]; path 'long' only).

    path 'mfma' (attention_mfma.hip): x, softmax and delta in fp32 over the whole row; Pd and dS rounded to bf16 before P V / Pd^T dO and
         dS K / dS^T Q; fp32 accumulation; bf16 outputs.
    path 'long' (attention_long.hip): forward with the ONLINE softmax over key-tile pairs (32 keys): running maximum m, running sum l, the
         accumulator rescaled by exp2(m_old - m_new), the unnormalised exp2(x - m) rounded to bf16 before P V, one division by l at the
         end, lse = m + log2 l.  Backward: statistics swept online per 16-key tile (m, l, delta like l), P = exp2(x - m) / l; with
         kept=True the lse form instead: P = exp2(x - lse), delta_i = dctx_i . ctx_i from the forward's bf16 ctx.
    path 'valu' (attention.hip): fp32 throughout in the natural-exponent domain (x = s scale - 10000), only the outputs rounded.

    mutate (one of MUTANTS): the wrong kernels the budget must catch --
      delta_dropped    delta_i summed over the dropped, rescaled probabilities Pd instead of P (recomputed statistics only: the kept
                       form has no such sum)
      no_rescale_last  'long' forward: the accumulator is not rescaled when the running maximum rises in the last tile pair
      dv_no_scale      1 / (1 - p) missing from the probabilities that enter dv
      ragged_last_key  the last key (Tk - 1, in a ragged tile) missing from P V
      dk_last_qtile    the rows of the last 16-query tile missing from dk
      pad_masked       the padding keys of the last tile (pair) carry -10000 like masked keys instead of being absent
    """
    assert path in ("mfma", "long", "valu") and (mutate is None or mutate in MUTANTS) and not (kept and path != "long")
    assert not (kept and mutate == "delta_dropped")
    B, Tq, _ = q.shape
    Tk = k.shape[1]
    qh, kh, vh, gh = (_heads(t, heads, d, torch.float32) for t in (q, k, v, dctx))
    scale = float(np.float32(1.0) / np.sqrt(np.float32(d)))                    # a.scale = 1.0f / sqrtf(d)
    ds = float(np.float32(1.0 / (1.0 - p))) if p > 0 else 1.0
    kp = _keep(keep, B, heads, Tq, Tk)
    att = torch.as_tensor(keymask).bool()[:, None, None, :]
    # ---- scores: fp32 accumulation of exact bf16 products, one fused multiply-add into the exponent domain
    s = qh @ kh.transpose(-1, -2)
    if path == "valu":
        x = (s.double() * scale + torch.where(att, 0.0, -10000.0)).to(torch.float32)
        ex = torch.exp
    else:
        sc = float(np.float32(scale) * np.float32(1.4426950408889634))
        x = (s.double() * sc + torch.where(att, 0.0, MASK_OFF32)).to(torch.float32)
        ex = torch.exp2
    # keys up to the next multiple of 32 (the long kernels' tile pair; 16 for the others makes no difference): absent = -inf
    Tkp = (Tk + 31) // 32 * 32
    pad_x = (MASK_OFF32 if path != "valu" else -10000.0) if mutate == "pad_masked" else float("-inf")
    x = torch.cat([x, torch.full((B, heads, Tq, Tkp - Tk), pad_x, dtype=torch.float32)], -1)
    kpp = torch.cat([kp, torch.ones(B, heads, Tq, Tkp - Tk, dtype=torch.bool)], -1)
    vp = torch.cat([vh, torch.zeros(B, heads, Tkp - Tk, d)], 2)
    kpad = torch.cat([kh, torch.zeros(B, heads, Tkp - Tk, d)], 2)
    pv_cols = torch.ones(Tkp)
    if mutate == "ragged_last_key":
        pv_cols[Tk - 1] = 0.0
    lse = None
    # ---- forward
    if path == "long":
        m = torch.full((B, heads, Tq), float("-inf"))
        l = torch.zeros(B, heads, Tq)
        o = torch.zeros(B, heads, Tq, d)
        for j0 in range(0, Tkp, 32):
            xs = x[..., j0:j0 + 32]
            mn = torch.maximum(m, xs.max(-1).values)
            alpha = torch.exp2(m - mn)
            e = torch.exp2(xs - mn[..., None])
            pb = _rb(torch.where(kpp[..., j0:j0 + 32], e * ds, torch.zeros(()))) * pv_cols[j0:j0 + 32]
            l = l * alpha + e.sum(-1)
            oa = o if (mutate == "no_rescale_last" and j0 + 32 >= Tkp) else o * alpha[..., None]
            o = oa + pb @ vp[:, :, j0:j0 + 32]
            m = mn
        ctx = _rb(o * (1.0 / l)[..., None])
        lse = m + torch.log2(l)
    else:
        e = ex(x - x.max(-1, keepdim=True).values)
        P = e * (1.0 / e.sum(-1, keepdim=True))
        Pd = torch.where(kpp, P * ds, torch.zeros(()))
        if path == "mfma":
            Pd = _rb(Pd)
        ctx = _rb((Pd * pv_cols) @ vp)
    # ---- backward: probabilities and delta
    gp = torch.where(kpp, (gh @ vp.transpose(-1, -2)) * ds, torch.zeros(()))           # gradient w.r.t. P, through the dropout
    if path == "long" and kept:
        P = torch.exp2(x - lse[..., None])
        delta = (ctx * gh).sum(-1, keepdim=True)
    else:
        if path == "long":       # sweep 1, online per 16-key tile
            m = torch.full((B, heads, Tq), float("-inf"))
            l = torch.zeros(B, heads, Tq)
            dl = torch.zeros(B, heads, Tq)
            for j0 in range(0, (Tk + 15) // 16 * 16, 16):
                xs = x[..., j0:j0 + 16]
                mn = torch.maximum(m, xs.max(-1).values)
                alpha = torch.exp2(m - mn)
                e = torch.exp2(xs - mn[..., None])
                w = e * ds if mutate == "delta_dropped" else e
                l = l * alpha + e.sum(-1)
                dl = dl * alpha + (w * gp[..., j0:j0 + 16]).sum(-1)
                m = mn
            inv = 1.0 / l
            P = torch.exp2(x - m[..., None]) * inv[..., None]
            delta = (dl * inv)[..., None]
        else:
            delta = (gp * (P * ds if mutate == "delta_dropped" else P)).sum(-1, keepdim=True)
    dS = P * (gp - delta)
    Pdv = torch.where(kpp, P * (1.0 if mutate == "dv_no_scale" else ds), torch.zeros(()))
    if path != "valu":
        dS, Pdv = _rb(dS), _rb(Pdv)
    dSk = dS.clone()
    if mutate == "dk_last_qtile":
        dSk[:, :, (Tq - 1) // 16 * 16:, :] = 0.0
    dq = _rb((dS @ kpad) * scale)
    dk = _rb((dSk.transpose(-1, -2) @ qh)[:, :, :Tk] * scale)
    dv = _rb((Pdv.transpose(-1, -2) @ gh)[:, :, :Tk])
    return dict(ctx=_rows(ctx).double(), dq=_rows(dq).double(), dk=_rows(dk).double(), dv=_rows(dv).double(), lse=lse)


# ------------------------------------------------------------------------------------------- input families
def mask_row(kind, Tk, g):
    """One batch row's key mask (uint8 [Tk]) of the 'masks' family: kind 0 a random 70 % attended, 1 every key masked, 2 only one key
    attended, in the last 16-key tile, 3 an aligned pair of key tiles (32 keys; one tile of 16 where there are fewer than 64 keys, the first half of a single tile) masked in the
    middle."""
    km = np.ones(Tk, dtype=np.uint8)
    kind %= 4
    if kind == 0:
        km = (g.random(Tk) < 0.7).astype(np.uint8)
        km[int(g.integers(Tk))] = 1
    elif kind == 1:
        km[:] = 0
    elif kind == 2:
        km[:] = 0
        last = (Tk - 1) // 16 * 16
        km[last + (Tk - 1 - last) // 2] = 1
    elif Tk <= 16:                     # a single tile: its first half
        km[:Tk // 2] = 0
    else:
        w = 32 if Tk >= 64 else 16
        lo = (Tk // w) // 2 * w
        km[lo:lo + w] = 0
    return km


def make_inputs(family, B, heads, Tq, Tk, d, seed=0, mask_offset=0):
    """(q, k, v, dctx, keymask): bf16 CPU tensors [B, T, heads d] and uint8 [B, Tk].
    flat       unit randn; the last b % 4 keys of batch row b masked
    peaked     q and k at standard deviation 2 (sharply peaked softmax); masks as flat
    late_max   the last ATTENDED key of every row dominates (q carries a common direction w, that key is 8 / sqrt(d) w): the row maximum
               arrives in the last key-tile pair, and an online softmax must rescale a full accumulator
    early_max  the same with key 0
    masks      flat data, batch row b with mask_row kind (b + mask_offset) % 4"""
    assert family in FAMILIES
    g = torch.Generator().manual_seed(1000 * seed + 17)
    ng = np.random.default_rng(seed)
    H = heads * d
    std = 2.0 if family == "peaked" else 1.0
    q = torch.randn(B, Tq, H, generator=g) * std
    k = torch.randn(B, Tk, H, generator=g) * std
    v = torch.randn(B, Tk, H, generator=g)
    dctx = torch.randn(B, Tq, H, generator=g)
    km = np.ones((B, Tk), dtype=np.uint8)
    if family == "masks":
        for b in range(B):
            km[b] = mask_row(b + mask_offset, Tk, ng)
    else:
        for b in range(B):
            if b % 4 and Tk > b % 4:
                km[b, Tk - (b % 4):] = 0
    if family in ("late_max", "early_max"):
        w = torch.where(torch.rand(H, generator=g) < 0.5, -1.0, 1.0)
        q = q + w
        for b in range(B):
            j = 0 if family == "early_max" else int(np.nonzero(km[b])[0][-1])
            k[b, j] = w * (8.0 / math.sqrt(d))
    return bf16(q), bf16(k), bf16(v), bf16(dctx), torch.from_numpy(km)
