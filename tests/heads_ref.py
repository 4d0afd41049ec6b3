"""Host-only yardstick for csrc/heads.hip: fp64 restatements of the four head kinds (PlotQA, DVQA cross-entropy regressor, DVQA
evaluation snap, no regressor) and of the evaluation's answer selection, a budget per output element, an fp32 emulator of each
kernel's arithmetic in the kernel's order with named mutants, and the inputs the CPU and GPU tests share.
tests/test_heads_ref_cpu.py proves the yardstick (emulator inside a quarter of every budget, every mutant caught);
tests/test_heads_gpu.py holds the kernels to it.  Imports nothing of the product but tests/dropout_ref.py.

Budgets.  An fp32 output must satisfy |got - fp64| <= 2^-16 mag with NO absolute floor, mag = the sum of the absolute values of the
terms that reach the element (the pre-filled value of an accumulated gradient included); an element nothing reaches has mag = 0
and must be exactly 0.  A bf16 output gets one bf16 step on top.  Counts, classes, table values and gathered values are exact.
The mags of the CE regressor, for a row with weight w_b = g_reg[b] (0 without `needs` or with a target outside [0, 65)):
    z_k      zmag_k = sum_c |fus_h_c| |W_kc| + |b_k|
    p_k      pmag_k = p_k (1 + zmag_k + sum_j p_j zmag_j)       d p_k = p_k (d z_k - sum_j p_j d z_j), plus p_k's own roundings
    loss     lse(p) + pmag_t + sum_j q_j pmag_j,  q = softmax(p)  the two terms of lse(p) - p_t and the p errors they carry
    dz_k     |w_b| p_k (|dp_k| + sum_j p_j |dp_j|),  dp_j = q_j - [j == t]
    d_w[k,c] sum_b |dz_bk| |fus_h_bc| + |prefill|;   d_b[k]: sum_b |dz_bk| + |prefill|
    d_fus_h  slope_c sum_k dzmag_k |W_kc|                         (dz_k carries an error relative to dzmag_k, not to |dz_k|)
2^-16 is 256 fp32 roundings: the z sums are 256 products (their worst case is ~ 2^-16 zmag only if every rounding errs the same
way), everything after them is a handful of roundings on O(1) quantities.
"""
import os

import numpy as np
import torch

import dropout_ref as DR

BOUND = 2.0 ** -16
CE_CLASSES = 65
DVQA_FLOATS = [-9.0 + i for i in range(51)] + [43.0, 50.0, 60.0, 70.0, 80.0, 90.0, 100.0, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9]
HEAD_SITE = 3                                     # the engine's cls dropout site
HEAD_NSP_COEFF, HEAD_REG_COEFF = 1.0, 0.7        # CrctHeadArgs.nsp_coeff / reg_coeff of every launch of the head tests
DROP_SEEDS = ((1 << 40) + 0x2F1D, (0x3A5 << 52) + 77)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TIE_A, TIE_B = 20, 41                             # the two classes with identical ce_fusion.6 rows (table values 11 and 32)
F32, F64 = np.float32, np.float64

CE_MUTANTS = ("softmax_once", "no_pdp", "argmax_ge", "target_rounded", "no_slope", "no_div_B", "grad_scale_twice", "needs_ignored",
              "target_clamped")
SNAP_MUTANTS = ("snap_le", "snap_unscaled", "snap_no_roundtrip", "snap_old_d5")
SELECT_MUTANTS = ("raw_logit", "last_max", "nan_skipped")


def head_cfg(p=0.0, seed=0, fusion_sum=0, use_l1=False, kind_l1=False, tol=0.01):
    """The scalar settings one head launch and its fp64 restatement share."""
    return dict(p=p, seed=seed, fusion_sum=bool(fusion_sum), use_l1=bool(use_l1), kind_l1=bool(kind_l1), tol=tol)


def bf16_step(x):
    """Spacing of the bf16 numbers at |x| (fp64): 2^(exponent - 7); the smallest normal's below it."""
    a = x.double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


def host_keep(hc, B, Hb):
    return torch.from_numpy(DR.keep_rowmajor(hc["seed"], HEAD_SITE, B, Hb, hc["p"])) if hc["p"] else torch.ones(B, Hb, dtype=torch.bool)


def upstream(kind, B, grad_scale):
    """(g_loss, g_nsp, g_reg device tensors or None; the effective fp64 g_nsp scalar and g_reg [B]) for 'default', 'loss_dev' and
    'nsp_reg_dev' (a ramp that crosses 0), as test_head_loss_against_fp64 feeds them."""
    if kind == "nsp_reg_dev":
        g_reg = torch.linspace(-0.5, 1.5, B)
        return None, torch.tensor([1.3]), g_reg, float(F32(1.3)) * grad_scale, g_reg.double() * grad_scale
    g_loss = torch.tensor([0.37]) if kind == "loss_dev" else None
    gl = (float(F32(0.37)) if g_loss is not None else 1.0) * grad_scale
    return g_loss, None, None, HEAD_NSP_COEFF * gl, torch.full((B,), float(F32(HEAD_REG_COEFF)) * gl / B, dtype=torch.float64)


# ------------------------------------------------------------------------------------------- fp64: the classification half
def cls_half64(inp, labels, keep, hc):
    """BertPreTrainingHeads from the poolers' outputs on (vilbert.py:1048-1062) and CrossEntropyLoss(ignore_index = -1) over the labels
    (0 when every label is ignored): fp64 leaves pt, pv, W, bc and logits, nsp (in the graph), fd, nvalid, logit_mag."""
    pt, pv = (inp[k].double().requires_grad_(True) for k in ("pt", "pv"))
    W, bc = (inp[k].double().requires_grad_(True) for k in ("w_cls", "b_cls"))
    f = pt + pv if hc["fusion_sum"] else pt * pv
    fd = f * keep.double() / (1.0 - hc["p"])
    logits = fd @ W.t() + bc
    nvalid = int((labels != -1).sum()) if labels is not None else 0
    if labels is not None:
        lab = labels.clamp_min(0)
        ce = torch.logsumexp(logits, 1) - logits.gather(1, lab[:, None]).squeeze(1)
        nsp = torch.where(labels != -1, ce, torch.zeros_like(ce)).sum() / max(nvalid, 1)
    else:
        nsp = torch.zeros((), dtype=torch.float64)
    return dict(pt=pt, pv=pv, W=W, bc=bc, fd=fd, logits=logits, nsp=nsp, nvalid=nvalid,
                logit_mag=(fd.abs() @ W.abs().t() + bc.abs()).detach())


def _gr(t):
    return t.grad if t.grad is not None else torch.zeros_like(t)        # no labels: no path to the NSP inputs


def cls_grads(c):
    """The seeds w.r.t. the poolers' pre-activations (relu'(pre) == (post > 0)) and the bi_seq_relationship gradients."""
    pt, pv = c["pt"], c["pv"]
    return dict(d_pt=_gr(pt) * (pt.detach() > 0), d_pv=_gr(pv) * (pv.detach() > 0), d_w_cls=_gr(c["W"]), d_b_cls=_gr(c["bc"]))


def reg_tail64(r_use, R, hc, own=None, r_k=None):
    """vilbert.py:1583-1657 after the prediction r_use (fp64, may carry a graph): SmoothL1 (beta 0.5) / L1, the |target| > 1 rule, the
    needs mask, d5 and the two right-flags.  Rows in `own` take their d5 flag as the kernel decides it, by fp32 division of the fp32
    values r_k."""
    R64 = R.double()
    needs = R64[:, 1] == 1
    target = R64[:, 0] / torch.where(needs, R64[:, 3], torch.ones_like(R64[:, 3]))
    diff = r_use - target
    l1v = diff.abs()
    rl = l1v if hc["use_l1"] else torch.where(l1v < 0.5, diff * diff, l1v - 0.25)
    if not hc["kind_l1"]:
        rl = torch.where(target.abs() > 1, torch.zeros_like(rl), rl)
    rl = torch.where(needs, rl, torch.zeros_like(rl))
    both0 = (r_use == 0) & (target == 0)
    d5 = torch.where(target == 0, torch.ones_like(l1v), l1v.detach() / target.abs())
    d5 = torch.where(both0, torch.zeros_like(d5), d5)
    ok5 = ((d5 <= 0.05) | both0) & needs
    if own is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            t32 = (R[:, 0].numpy() / np.where(needs.numpy(), R[:, 3].numpy(), F32(1))).astype(F32)
            d5_32 = np.abs(r_k.numpy() - t32) / np.abs(t32)
        ok5 = torch.where(own, torch.from_numpy(d5_32 <= F32(0.05)) & needs, ok5)
    okt = (l1v <= hc["tol"]) & needs
    return dict(needs=needs, target=target, l1v=l1v, rl=rl, d5=d5, ok5=ok5, okt=okt, both0=both0)


def head_stats(labels, nsp, rl, d5v, needs_n, n5, nt, nvalid, B):
    nspf = float(nsp)
    reg_mean = float(rl.sum()) / B
    loss = HEAD_NSP_COEFF * nspf + HEAD_REG_COEFF * reg_mean if labels is not None else 0.0
    return torch.tensor([loss, nspf, reg_mean, needs_n, n5, nt, nvalid, 0, loss, 0, nspf,
                         float(rl.sum()) / needs_n if needs_n else 0.0, float(d5v.sum()) / needs_n if needs_n else 0.0, 0,
                         needs_n, n5, nt], dtype=torch.float64)


STAT_COUNTS = [3, 4, 5, 6, 7, 9, 13, 14, 15, 16]
STAT_FLOATS = [0, 1, 2, 8, 10, 11, 12]


def head_ref64(inp, R, labels, keep, hc, *, g_nsp, g_reg, r_k, own):
    """oracle.heads_and_losses from the poolers' outputs on, fp64, cls dropout = the host mask: (outputs, gradients, magnitudes) of the
    PlotQA head.  g_nsp / g_reg: the upstream gradients of the NSP mean and of each row's reg loss; r_k: the kernel's fp32 r, used for
    the rows in `own` (placed on a comparison boundary)."""
    c = cls_half64(inp, labels, keep, hc)
    fh = inp["fh"].double().requires_grad_(True)
    w6, b6 = (inp[k].double().requires_grad_(True) for k in ("w6", "b6"))
    z = fh @ w6 + b6
    r = torch.tanh(z)
    r_use = torch.where(own, r_k.double() + (r - r.detach()), r)       # boundary rows: the kernel's own fp32 r, fp64 r's gradient
    t = reg_tail64(r_use, R, hc, own, r_k)
    needs, rl, l1v, d5 = t["needs"], t["rl"], t["l1v"], t["d5"]
    B = R.shape[0]
    (g_nsp * c["nsp"] + (g_reg * rl).sum()).backward()
    d5v = torch.where(needs, d5, torch.zeros_like(d5)).detach()
    stats = head_stats(labels, c["nsp"].detach(), rl.detach(), d5v, int(needs.sum()), int(t["ok5"].sum()), int(t["okt"].sum()), c["nvalid"], B)
    zero = torch.zeros_like(r)
    R64 = R.double()
    reg = torch.stack([torch.where(needs, r_use * R64[:, 3], zero), rl, torch.where(needs, l1v, zero), r, d5v]).detach()
    zmag = (inp["fh"].double().abs() @ inp["w6"].double().abs() + inp["b6"].double().abs())
    tmag = torch.where(t["target"] != 0, t["target"].abs(), torch.ones_like(t["target"]))
    reg_mag = torch.stack([zmag * R64[:, 3].abs(), zmag * (1 + 2 * l1v.detach()), zmag, zmag, zmag / tmag]).detach()
    out = dict(logits=c["logits"].detach(), reg=reg, stats=stats, r=r.detach(), logit_mag=c["logit_mag"])
    grads = dict(cls_grads(c), d_fh=_gr(fh) * torch.where(fh.detach() > 0, 1.0, 0.01), d_w6=_gr(w6), d_b6=_gr(b6))
    return out, grads, reg_mag


# ------------------------------------------------------------------------------------------- fp64: the CE regressor
def ce_targets(R):
    """(tok, t): target class = trunc(R[:,0]) (the reference's .long()), valid when it lies in [0, 65)."""
    tf = R[:, 0].double()
    tok = (tf > -1) & (tf < CE_CLASSES)                 # NaN: False
    t = torch.where(tok, torch.trunc(torch.nan_to_num(tf)), torch.zeros_like(tf)).long()
    return tok, t


def ce_ref64(inp, R, labels, keep, hc, *, g_nsp, g_reg, values):
    """DVQA_Regressor_v20_CE (regressor.py:72-79) and its bookkeeping (vilbert.py:1603-1615) on top of the classification half.
    Returns (out, grads, mags)."""
    c = cls_half64(inp, labels, keep, hc)
    B = R.shape[0]
    fh = inp["fh"].double().requires_grad_(True)
    W6, b6 = (inp[k].double().requires_grad_(True) for k in ("w6", "b6"))
    vals = torch.tensor(values, dtype=torch.float32)
    z = fh @ W6.t() + b6
    p = torch.softmax(z, 1)
    p.retain_grad()
    needs = R[:, 1] == 1
    tok, t = ce_targets(R)
    w = needs & tok
    lse2 = torch.logsumexp(p, 1)
    loss_b = lse2 - p.gather(1, t[:, None]).squeeze(1)
    gw = torch.where(w, g_reg, torch.zeros_like(g_reg))
    (g_nsp * c["nsp"] + (gw * loss_b).sum()).backward()
    pd = p.detach()
    am = torch.argmax(pd, 1)                             # the first maximum
    nan = torch.full_like(lse2, float("nan"))
    rl = torch.where(needs, torch.where(tok, loss_b.detach(), nan), torch.zeros_like(lse2))
    err = torch.where(w, (vals[am] - vals[t]).abs(), torch.zeros(B)).double()          # fp32 subtraction, as the kernel's
    ok = w & (am == t)
    n_ok, needs_n = int(ok.sum()), int(needs.sum())
    reg = torch.stack([torch.where(needs, vals[am], torch.zeros(B)).double(), rl, err, pd.gather(1, am[:, None]).squeeze(1), err])
    stats = head_stats(labels, c["nsp"].detach(), rl, err, needs_n, n_ok, n_ok, c["nvalid"], B)
    # dL/dz per row (what ce_scratch holds): the softmax Jacobian applied to dL/dp
    q = torch.softmax(pd, 1)
    dp = q.clone()
    dp[torch.arange(B), t] -= 1.0
    dz = gw[:, None] * pd * (dp - (pd * dp).sum(1, keepdim=True))
    fa, Wa = inp["fh"].double().abs(), inp["w6"].double().abs()
    zmag = fa @ Wa.t() + inp["b6"].double().abs()
    pmag = pd * (1 + zmag + (pd * zmag).sum(1, keepdim=True))
    loss_mag = lse2.detach().abs() + pmag.gather(1, t[:, None]).squeeze(1) + (q * pmag).sum(1)
    dzmag = gw.abs()[:, None] * pd * (dp.abs() + (pd * dp.abs()).sum(1, keepdim=True))
    slope = torch.where(inp["fh"].double() > 0, 1.0, 0.01)
    mags = dict(reg1=torch.where(w, loss_mag, torch.zeros_like(loss_mag)), reg3=pmag.gather(1, am[:, None]).squeeze(1), dz=dzmag,
                d_fh=(dzmag @ Wa) * slope, d_w6=dz.abs().t() @ fa, d_b6=dz.abs().sum(0), logit_mag=c["logit_mag"])
    out = dict(logits=c["logits"].detach(), reg=reg, stats=stats, dz=dz, p=pd, am=am, t=t, tok=tok, ok=ok, logit_mag=c["logit_mag"])
    grads = dict(cls_grads(c), d_fh=_gr(fh) * slope, d_w6=_gr(W6), d_b6=_gr(b6))
    return out, grads, mags


# ------------------------------------------------------------------------------------------- fp64: snap and NONE
def snap_nearest(r, R, table, mutate=None):
    """vilbert.py:1619-1625 in the fp32 steps the header states: x = fl(r scale), the nearest table entry by fp32 distance (first in
    table order on a tie), r' = fl(best / scale); rows without `needs` keep r.  r: fp32 [B].  Returns (r' fp32, index or -1)."""
    r = np.asarray(r, dtype=F32)
    Rn = R.numpy()
    tab = np.asarray(table, dtype=F32)
    x = r if mutate == "snap_unscaled" else (r * Rn[:, 3]).astype(F32)
    d = np.abs(tab[None, :] - x[:, None]).astype(F32)
    idx = (d.shape[1] - 1 - np.argmin(d[:, ::-1], 1)) if mutate == "snap_le" else np.argmin(d, 1)      # np.argmin: the first minimum
    best = tab[idx]
    with np.errstate(divide="ignore", invalid="ignore"):
        rp = (best / Rn[:, 3]).astype(F32)
    needs = Rn[:, 1] == 1
    return np.where(needs, rp, r).astype(F32), np.where(needs, idx, -1), best


def snap_ref64(inp, R, labels, keep, hc, *, g_nsp, r, table):
    """The DVQA evaluation snap from a given fp32 r (the kernel's own reg[3]): everything after r' as in the PlotQA head, and no
    regression gradient.  Returns (out, grads, reg_mag); reg_mag holds the magnitudes of the fp32 steps from r' on."""
    c = cls_half64(inp, labels, keep, hc)
    B = R.shape[0]
    rp, idx, best = snap_nearest(r, R, table)
    rp64 = torch.from_numpy(rp.astype(F64))
    t = reg_tail64(rp64, R, hc)
    needs, rl, l1v, d5 = t["needs"], t["rl"], t["l1v"], t["d5"]
    if c["nsp"].requires_grad:
        (g_nsp * c["nsp"]).backward()
    d5v = torch.where(needs, d5, torch.zeros_like(d5))
    stats = head_stats(labels, c["nsp"].detach(), rl, d5v, int(needs.sum()), int(t["ok5"].sum()), int(t["okt"].sum()), c["nvalid"], B)
    zero = torch.zeros(B, dtype=torch.float64)
    reg0 = torch.from_numpy((rp * R.numpy()[:, 3]).astype(F32).astype(F64))       # fl(r' scale): two correctly rounded fp32 steps from the table
    reg = torch.stack([torch.where(needs, reg0, zero), rl, torch.where(needs, l1v, zero), torch.from_numpy(np.asarray(r, F64)), d5v])
    m = rp64.abs() + t["target"].abs()                   # the terms of diff = r' - target
    tmag = torch.where(t["target"] != 0, t["target"].abs(), torch.ones_like(m))
    reg_mag = torch.stack([zero, m * (1 + 2 * l1v) + 0.25, m, zero, m / tmag])          # reg[0] and reg[3] are exact
    out = dict(logits=c["logits"].detach(), reg=reg, stats=stats, idx=idx, best=best, rp=rp, logit_mag=c["logit_mag"], tail=t)
    return out, cls_grads(c), reg_mag


def none_ref64(inp, R, labels, keep, hc, *, g_nsp):
    """No regressor module (vilbert.py:1592-1598): reg rows zero, the count of needs rows in stats[3] and stats[14]."""
    c = cls_half64(inp, labels, keep, hc)
    B = R.shape[0]
    if c["nsp"].requires_grad:
        (g_nsp * c["nsp"]).backward()
    zero = torch.zeros(B, dtype=torch.float64)
    stats = head_stats(labels, c["nsp"].detach(), zero, zero, int((R[:, 1] == 1).sum()), 0, 0, c["nvalid"], B)
    return dict(logits=c["logits"].detach(), reg=torch.zeros(5, B, dtype=torch.float64), stats=stats, logit_mag=c["logit_mag"]), cls_grads(c)


# ------------------------------------------------------------------------------------------- fp64: answer selection
def select_ref64(logits, reg_out, reg_err, reg_terr, num_ans, forced=None, N=None):
    """evaluation.py:249, 281-292: p0 = softmax(logits)[:, 0] in fp64; per question the first maximum over its rows below N (a NaN is
    the maximum, as for torch.argmax), or the forced answer; the three gathered values bit for bit.  Whatever selects no valid row
    gives sel_out 0 and +inf errors.  Returns (answers, out, err, terr, p0)."""
    lg = np.asarray(logits, dtype=F64)
    N = lg.shape[0] if N is None else N
    m = lg.max(1, keepdims=True)
    with np.errstate(invalid="ignore"):
        e = np.exp(lg - m)
        p0 = e[:, 0] / (e[:, 0] + e[:, 1])
    ans, out, err, terr = [], [], [], []
    off = 0
    for q, n in enumerate(np.asarray(num_ans).reshape(-1).tolist()):
        live = max(0, min(n, N - off))
        a = int(forced[q]) if forced is not None else (int(np.argmax(p0[off:off + live])) if live else 0)
        okrow = 0 <= a < n and off + a < N
        ans.append(a)
        out.append(reg_out[off + a] if okrow else F32(0))
        err.append(reg_err[off + a] if okrow else F32(np.inf))
        terr.append(reg_terr[off + a] if okrow else F32(np.inf))
        off += n
    return np.array(ans, dtype=np.int64), np.array(out, F32), np.array(err, F32), np.array(terr, F32), p0


# ------------------------------------------------------------------------------------------- the fp32 emulator
_L = np.arange(64)
_DPP = ((_L ^ 1), (_L ^ 2), (_L & 8) | (7 - (_L & 7)) | (_L & 48), (_L & 48) | (15 - (_L & 15)))


def wave_sum32(v):
    """common.hip.h wave_sum over the last axis (64 lanes): four DPP steps inside each row of 16, then (row0 + row1) + (row2 + row3)."""
    v = v.astype(F32)
    for perm in _DPP:
        v = (v + v[..., perm]).astype(F32)
    return ((v[..., 0] + v[..., 16]).astype(F32) + (v[..., 32] + v[..., 48]).astype(F32)).astype(F32)


def fma32(a, b, c):
    """fl32(a b + c): the compiler contracts the kernels' multiply-adds (a b is exact in fp64; the double rounding is below notice)."""
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def strided_dot32(x, w, width):
    """sum_c x[..., c] w[..., c] as `width` threads take it: thread i walks c = i, i + width, ... with fused multiply-adds.
    Returns the per-thread partial sums [..., width]."""
    n = x.shape[-1]
    acc = np.zeros(np.broadcast_shapes(x.shape, w.shape)[:-1] + (width,), F32)
    for s in range(0, n, width):
        m = min(width, n - s)
        acc[..., :m] = fma32(x[..., s:s + m], w[..., s:s + m], acc[..., :m])
    return acc


def block_sum32(part):
    """block_sum of 256 per-thread values: wave_sum per wave, then red[0] + red[1] + red[2] + red[3]."""
    r = wave_sum32(part.reshape(part.shape[:-1] + (4, 64)))
    return (((r[..., 0] + r[..., 1]).astype(F32) + r[..., 2]).astype(F32) + r[..., 3]).astype(F32)


def _np32(t):
    return t.float().numpy().astype(F32)


def emu_cls(inp, labels, keep, hc, g_nsp32):
    """The classification half as head_rows_kernel / head_ce_rows_kernel compute it: logits, the per-row NSP term and dl0 / dl1."""
    pt, pv, W, bc = _np32(inp["pt"]), _np32(inp["pv"]), _np32(inp["w_cls"]), _np32(inp["b_cls"])
    B = pt.shape[0]
    dsc = F32(1.0 / (1.0 - hc["p"])) if hc["p"] else F32(1)
    f = (pt + pv).astype(F32) if hc["fusion_sum"] else (pt * pv).astype(F32)
    f = np.where(keep.numpy(), (f * dsc).astype(F32), F32(0))
    l0 = (block_sum32(strided_dot32(f, W[0][None], 256)) + bc[0]).astype(F32)
    l1 = (block_sum32(strided_dot32(f, W[1][None], 256)) + bc[1]).astype(F32)
    mx = np.maximum(l0, l1)
    lse = (mx + np.log((np.exp((l0 - mx).astype(F32)) + np.exp((l1 - mx).astype(F32))).astype(F32))).astype(F32)
    nsp_b, dl0, dl1 = np.zeros(B, F32), np.zeros(B, F32), np.zeros(B, F32)
    valid = np.zeros(B, bool)
    if labels is not None:
        lab = labels.numpy()
        valid = lab != -1
        wq = (F32(g_nsp32) / F32(max(int(valid.sum()), 1))).astype(F32)
        nsp_b = np.where(valid, (lse - np.where(lab == 0, l0, l1)).astype(F32), F32(0))
        dl0 = np.where(valid, ((np.exp((l0 - lse).astype(F32)) - (lab == 0).astype(F32)).astype(F32) * wq).astype(F32), F32(0))
        dl1 = np.where(valid, ((np.exp((l1 - lse).astype(F32)) - (lab == 1).astype(F32)).astype(F32) * wq).astype(F32), F32(0))
    return dict(logits=np.stack([l0, l1], 1), nsp_b=nsp_b, dl0=dl0, dl1=dl1, valid=valid)


def to_bf16(x):
    return torch.from_numpy(np.asarray(x, dtype=F32)).to(torch.bfloat16)


def emu_gscale(B, grad_scale, g_loss=None, g_nsp=None, g_reg=None, mutate=None):
    """g_nsp (fp32 scalar) and g_reg (fp32 [B]) as the kernels form them from the three optional device tensors."""
    gs = F32(grad_scale)
    gl = ((F32(g_loss[0]) if g_loss is not None else F32(1)) * gs).astype(F32)
    gn = (F32(g_nsp[0]) * gs).astype(F32) if g_nsp is not None else (F32(HEAD_NSP_COEFF) * gl).astype(F32)
    if g_reg is not None:
        gr = (_np32(g_reg) * gs).astype(F32)
        if mutate == "grad_scale_twice":
            gr = (gr * gs).astype(F32)
    else:
        gr = (F32(HEAD_REG_COEFF) * gl).astype(F32)
        gr = np.full(B, gr if mutate == "no_div_B" else (gr / F32(B)).astype(F32), F32)
    return gn, gr


def emu_ce(inp, R, values, g_reg32, prefill=None, mutate=None):
    """head_ce_rows_kernel's regression part and head_ce_wgrad_kernel in fp32, in their order: z by wave-strided dot products, the
    serial 65-term softmax / argmax / logsumexp / pdp loops, dz, d_fus_h, and the row-ordered weight-gradient sums on top of `prefill`."""
    fh, W6, b6 = _np32(inp["fh"]), _np32(inp["w6"]), _np32(inp["b6"])
    vals = np.asarray(values, F32)
    Rn = R.numpy()
    B, K = fh.shape[0], CE_CLASSES
    z = (wave_sum32(strided_dot32(fh[:, None, :], W6[None], 64)) + b6[None]).astype(F32)
    zm = z[:, 0].copy()
    for k in range(1, K):
        zm = np.maximum(zm, z[:, k])
    ez = np.exp((z - zm[:, None]).astype(F32)).astype(F32)
    se = np.zeros(B, F32)
    for k in range(K):
        se = (se + ez[:, k]).astype(F32)
    p = (ez / se[:, None]).astype(F32)
    if mutate == "softmax_once":
        p = z
    needs = Rn[:, 1] == 1
    tf = Rn[:, 0]
    with np.errstate(invalid="ignore"):
        tok = (tf > -1) & (tf < K)
        tcl = np.where(tok, np.trunc(np.nan_to_num(tf)), 0).astype(np.int64)
        if mutate == "target_rounded":
            tcl = np.where(tok, np.clip(np.rint(np.nan_to_num(tf)), 0, K - 1), 0).astype(np.int64)
        if mutate == "target_clamped":
            tcl = np.clip(np.trunc(np.nan_to_num(tf, nan=0.0, posinf=1e9, neginf=-1e9)), 0, K - 1).astype(np.int64)
            tok = np.ones(B, bool)
    am, pm = np.zeros(B, np.int64), p[:, 0].copy()
    for k in range(1, K):
        up = p[:, k] >= pm if mutate == "argmax_ge" else p[:, k] > pm
        pm, am = np.where(up, p[:, k], pm), np.where(up, k, am)
    e2 = np.exp((p - pm[:, None]).astype(F32)).astype(F32)
    s2 = np.zeros(B, F32)
    for k in range(K):
        s2 = (s2 + e2[:, k]).astype(F32)
    lse2 = (pm + np.log(s2).astype(F32)).astype(F32)
    onehot = (np.arange(K)[None] == tcl[:, None]).astype(F32)
    dp = (np.exp((p - lse2[:, None]).astype(F32)).astype(F32) - onehot).astype(F32)
    pdp = np.zeros(B, F32)
    for k in range(K):
        pdp = fma32(p[:, k], dp[:, k], pdp)
    if mutate == "no_pdp":
        pdp = np.zeros(B, F32)
    live = tok if mutate == "needs_ignored" else (needs & tok)
    w = np.where(live, g_reg32, F32(0)).astype(F32)
    dz = ((w[:, None] * p).astype(F32) * (dp - pdp[:, None]).astype(F32)).astype(F32)
    pt_ = p[np.arange(B), tcl]
    rl = np.where(needs, np.where(tok, (lse2 - pt_).astype(F32), F32(np.nan)), F32(0)).astype(F32)
    err = np.where(needs & tok, np.abs(vals[am] - vals[tcl]).astype(F32), F32(0))
    ok = needs & tok & (am == tcl)
    g = np.zeros((B, 256), F32)
    for k in range(K):
        g = fma32(dz[:, k:k + 1], W6[k][None], g)
    slope = np.where(fh > 0, F32(1), F32(1) if mutate == "no_slope" else F32(0.01))
    d_fh = (g * slope).astype(F32)
    reg = np.stack([np.where(needs, vals[am], F32(0)), rl, err, pm, err]).astype(F32)
    out = dict(z=z, p=p, am=am, reg=reg, dz=dz, d_fh=to_bf16(d_fh), ok=ok, needs=needs)
    if prefill is not None:
        gw, gb = np.zeros((K, 256), F32), np.zeros(K, F32)
        for b in range(B):
            gw = fma32(dz[b][:, None], fh[b][None, :], gw)
            gb = (gb + dz[b]).astype(F32)
        out["d_w6"] = (_np32(prefill["d_w6"]) + gw).astype(F32)
        out["d_b6"] = (_np32(prefill["d_b6"]) + gb).astype(F32)
    return out


def emu_reduce_stats(reg, cls, ok5, okt, needs, with_labels):
    """head_reduce_kernel's stats: one wave walks the rows (b = lane, lane + 64, ...) and wave_sums the records."""
    B = reg.shape[1]

    def rows(v):
        v = np.concatenate([np.asarray(v).astype(F32), np.zeros((-B) % 64, F32)]).reshape(-1, 64)
        acc = np.zeros(64, F32)
        for trip in v:
            acc = (acc + trip).astype(F32)
        return wave_sum32(acc)
    s3, s4, s5, s6, s7 = rows(cls["nsp_b"]), rows(cls["valid"]), rows(ok5), rows(okt), rows(needs)
    rl, d5 = rows(reg[1]), rows(reg[4])
    nsp = (s3 / s4).astype(F32) if s4 > 0 else F32(0)
    reg_mean = (rl / F32(B)).astype(F32)
    loss = fma32(F32(HEAD_REG_COEFF), reg_mean, (F32(HEAD_NSP_COEFF) * nsp).astype(F32)) if with_labels else F32(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.array([loss, nsp, reg_mean, s7, s5, s6, s4, 0, loss, 0, nsp, (rl / s7) if s7 > 0 else 0, (d5 / s7) if s7 > 0 else 0, 0,
                         s7, s5, s6], dtype=F32)


def emu_tanh_r(inp):
    """head_rows_kernel's r = tanhf(z): z = fus_h . w_f6 by one thread per column, block_sum, + b_f6."""
    fh, w6, b6 = _np32(inp["fh"]), _np32(inp["w6"]), _np32(inp["b6"])
    z = (block_sum32((fh * w6[None]).astype(F32)) + b6[0]).astype(F32)
    return np.tanh(z).astype(F32)


def emu_snap(r, R, table, hc, mutate=None):
    """head_rows_kernel<HEAD_SNAP> from r on, fp32: the snap, then the PlotQA tail (losses, d5, flags); reg [5, B] and the flags."""
    Rn = R.numpy()
    r = np.asarray(r, F32)
    needs = Rn[:, 1] == 1
    rp, idx, best = snap_nearest(r, R, table, mutate)
    with np.errstate(divide="ignore", invalid="ignore"):
        target = (Rn[:, 0] / Rn[:, 3]).astype(F32)
        diff = (rp - target).astype(F32)
        l1v = np.abs(diff)
        rl = l1v if hc["use_l1"] else np.where(l1v < F32(0.5), (diff * diff).astype(F32), (l1v - F32(0.25)).astype(F32))
        both0 = (rp == 0) & (target == 0)
        l1_for_d5 = np.abs((r - target).astype(F32)) if mutate == "snap_old_d5" else l1v
        d5 = (l1_for_d5 / np.abs(target)).astype(F32)
        d5 = np.where(target == 0, F32(1), d5)
        d5 = np.where(both0, F32(0), d5)
        ok5 = ((d5 <= F32(0.05)) | both0) & needs
        okt = (l1v <= F32(hc["tol"])) & needs
        if not hc["kind_l1"]:
            rl = np.where(np.abs(target) > 1, F32(0), rl)
        rl = np.where(needs, rl, F32(0))
        reg0 = np.where(needs, best if mutate == "snap_no_roundtrip" else (rp * Rn[:, 3]).astype(F32), F32(0))
    reg = np.stack([reg0, rl, np.where(needs, l1v, F32(0)), r, np.where(needs, d5, F32(0))]).astype(F32)
    return dict(reg=reg, ok5=ok5, okt=okt, needs=needs, idx=idx)


def emu_select(logits, reg_out, reg_err, reg_terr, num_ans, forced=None, N=None, mutate=None):
    """eval_select_kernel: p0 in fp32; lane l of a question's wave walks its rows l, l + 64, ... and keeps its first maximum, the 64
    lanes then keep the largest p0 and, among equals, the smallest row; a NaN beats every number, the first NaN wins."""
    lg = np.asarray(logits, F32)
    N = lg.shape[0] if N is None else N
    m = lg.max(1, keepdims=True)
    with np.errstate(invalid="ignore"):
        e = np.exp((lg - m).astype(F32)).astype(F32)
        p0 = (e[:, 0] / (e[:, 0] + e[:, 1]).astype(F32)).astype(F32)
    score = lg[:, 0] if mutate == "raw_logit" else p0
    ans, out, err, terr = [], [], [], []
    off = 0
    for q, n in enumerate(np.asarray(num_ans).reshape(-1).tolist()):
        lanes = []
        for lane in range(min(64, n)):
            best, bi = F32(-np.inf), None
            for j in range(lane, n, 64):
                p = score[off + j] if off + j < N else F32(0)
                nanp, nanb = np.isnan(p), np.isnan(best)
                if mutate == "nan_skipped":
                    take = p > best
                elif mutate == "last_max":
                    take = (p >= best and not nanb) or (nanp and not nanb)
                else:
                    take = (p > best) or (nanp and not nanb)
                if take:
                    best, bi = p, j
            if bi is not None:
                lanes.append((best, bi))
        a = 0
        if n > 0:
            nans = [bi for best, bi in lanes if np.isnan(best)]
            if nans and mutate != "nan_skipped":
                a = min(nans)
            else:
                nums = [(best, bi) for best, bi in lanes if not np.isnan(best)]
                if not nums:
                    a = 0x7fffffffffffffff
                else:
                    top = max(b for b, _ in nums)
                    cands = [bi for b, bi in nums if b == top]
                    a = max(cands) if mutate == "last_max" else min(cands)
        if forced is not None:
            a = int(forced[q])
        okrow = 0 <= a < n and off + a < N
        ans.append(a)
        out.append(reg_out[off + a] if okrow else F32(0))
        err.append(reg_err[off + a] if okrow else F32(np.inf))
        terr.append(reg_terr[off + a] if okrow else F32(np.inf))
        off += n
    return np.array(ans, dtype=np.int64), np.array(out, F32), np.array(err, F32), np.array(terr, F32), p0


# ------------------------------------------------------------------------------------------- budgets
def ratio(got, ref, mag, bf16=False):
    """|got - ref| / budget per element (fp64 tensors); budget = 2^-16 mag (+ one bf16 step at max(|got|, |ref|)).  An element with
    budget 0 gives 0 when it is exactly right and inf otherwise; NaN in the reference demands NaN."""
    got, ref, mag = (torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).double() for x in (got, ref, mag))
    budget = BOUND * mag
    if bf16:
        budget = budget + bf16_step(torch.maximum(got.abs(), ref.abs()))
    err = (got - ref).abs()
    both_nan = torch.isnan(got) & torch.isnan(ref)
    r = torch.where(err == 0, torch.zeros_like(err), err / budget)
    r = torch.where(both_nan, torch.zeros_like(r), r)
    return torch.nan_to_num(r, nan=float("inf"), posinf=float("inf"))


def assert_within(got, ref, mag, what, bf16=False, worst=None, frac=1.0):
    r = ratio(got, ref, mag, bf16)
    top = float(r.max()) if r.numel() else 0.0
    if worst is not None:
        key = what.split(": ")[-1]
        worst[key] = max(worst.get(key, 0.0), top)
    if not top <= frac:
        i = tuple(int(k) for k in (r == r.max()).nonzero()[0])
        g, f, m = (torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).double() for x in (got, ref, mag))
        raise AssertionError("%s: %d elements beyond %.2f of the budget, worst %.3g at %s (got %r, fp64 %r, sum|terms| %r)" % (
            what, int((r > frac).sum()), frac, top, i, float(g[i]), float(f[i]), float(m[i])))


# ------------------------------------------------------------------------------------------- inputs
HEAD_SHAPES = [(B, Hb) for B in (1, 7, 80, 300) for Hb in (64, 1032)]
# (fusion_sum, p, upstream, grad_scale, labels): the combinations test_head_loss_against_fp64 uses
COMBOS = ((0, 0.0, "default", 1.0, "some"), (1, 0.1, "loss_dev", 2.5, "some"), (0, 0.1, "nsp_reg_dev", 0.5, "some"),
          (1, 0.0, "loss_dev", 1.0, "all_ignored"))
CE_MARGIN = 1e-3
_RIGHT, _WRONG, _NEEDS0, _ZERO_R, _FRAC, _NEG_HALF, _TIE = range(7)


def cls_inputs(B, Hb, g):
    pt = torch.relu(torch.randn(B, Hb, generator=g)).to(torch.bfloat16)
    pv = torch.relu(torch.randn(B, Hb, generator=g)).to(torch.bfloat16)
    return dict(pt=pt, pv=pv, w_cls=torch.randn(2, Hb, generator=g) * 0.05, b_cls=torch.tensor([0.1, -0.1]))


def make_labels(B, g, kind="some"):
    if kind == "all_ignored":
        return torch.full((B,), -1, dtype=torch.long)
    labels = torch.randint(0, 2, (B,), generator=g)
    labels[torch.arange(B) % 5 == 2] = -1
    return labels


def _ce_kinds(B):
    kinds = [(_WRONG if b % 3 == 1 else _RIGHT) for b in range(B)]
    special = {2: _NEEDS0, 3: _ZERO_R, 4: _FRAC, 5: _NEG_HALF, 6: _TIE}
    for base in ((0, 40) if B >= 80 else (0,)):
        for k, v in special.items():
            if base + k < B:
                kinds[base + k] = v
    return kinds


def ce_margin(inp, tie_rows=()):
    """fp64 top-2 margin of p = softmax(z) per row; on a tie row the margin of the tied pair over the third."""
    p = torch.softmax(inp["fh"].double() @ inp["w6"].double().t() + inp["b6"].double(), 1)
    top = torch.sort(p, 1, descending=True).values
    m = top[:, 0] - top[:, 1]
    for b in tie_rows:
        m[b] = top[b, 1] - top[b, 2]
    return m, p


def ce_inputs(B, Hb, seed):
    """Inputs of the CE head: rows right, wrong, needs = 0, R = [0, 0, 0, 0], a fractional target (c + 0.75), target -0.5 (class 0)
    and an exact argmax tie between the classes TIE_A < TIE_B (identical ce_fusion.6 rows, different table values) whose target is
    TIE_B.  At B >= 80 every class is some row's target.  fus_h points at the row's chosen class; the boost is raised per row until the
    fp64 top-2 margin of p is at least CE_MARGIN."""
    g = torch.Generator().manual_seed(seed)
    inp = cls_inputs(B, Hb, g)
    w6 = torch.randn(CE_CLASSES, 256, generator=g) * 0.1
    b6 = torch.randn(CE_CLASSES, generator=g) * 0.1
    w6[TIE_B], b6[TIE_B] = w6[TIE_A], b6[TIE_A]
    kinds = _ce_kinds(B)
    noise = torch.randn(B, 256, generator=g) * 0.3
    chosen, target, needs = [0] * B, [0.0] * B, [1.0] * B
    nxt = 0
    for b, kind in enumerate(kinds):
        if kind in (_RIGHT, _WRONG, _FRAC):
            t, nxt = nxt % CE_CLASSES, nxt + 1
            if kind == _WRONG or t in (TIE_A, TIE_B):
                c = (t + 7) % CE_CLASSES
                c = (t + 9) % CE_CLASSES if c in (TIE_A, TIE_B) else c
                if kind == _FRAC:
                    kinds[b] = _WRONG
            else:
                c = t
            chosen[b], target[b] = c, float(t) + (0.75 if kind == _FRAC else 0.0)
        elif kind == _NEEDS0:
            chosen[b], target[b], needs[b] = 3, 3.0, 0.0
        elif kind == _ZERO_R:
            chosen[b], target[b], needs[b] = 7, 0.0, 0.0
        elif kind == _NEG_HALF:
            chosen[b], target[b] = (0 if b < 40 else 5), -0.5
        else:
            chosen[b], target[b] = TIE_A, float(TIE_B)
    ch = torch.tensor(chosen)
    direction = w6[ch] / w6[ch].norm(dim=1, keepdim=True) ** 2
    boost = torch.full((B,), 2.5)
    tie_rows = [b for b, k in enumerate(kinds) if k == _TIE]
    for _ in range(40):
        fh = torch.nn.functional.leaky_relu(noise + boost[:, None] * direction, 0.01).to(torch.bfloat16)
        inp.update(fh=fh, w6=w6, b6=b6)
        m, _p = ce_margin(inp, tie_rows)
        low = m < CE_MARGIN
        if not bool(low.any()):
            break
        boost = torch.where(low, boost * 1.25, boost)
    R = torch.stack([torch.tensor(target), torch.tensor(needs), torch.full((B,), 0.01), torch.full((B,), 100.0)], 1).float()
    R[[b for b, k in enumerate(kinds) if k == _ZERO_R]] = 0.0
    inp.update(kinds=kinds, chosen=ch, tie_rows=tie_rows, g=g)
    return inp, R


def ce_prefill(B, Hb):
    g = torch.Generator().manual_seed(B + Hb)
    torch.randn(2, Hb, generator=g), torch.randn(2, generator=g)          # the launch helper's d_w_cls / d_b_cls draws come first
    return dict(d_w6=torch.randn(CE_CLASSES, 256, generator=g) * 0.3, d_b6=torch.randn(CE_CLASSES, generator=g) * 0.3)


BAD_TARGETS = (-1.0, 65.0, 1e9, float("nan"))

_S_PLAIN, _S_NEEDS0, _S_SNAP0, _S_BIG = range(4)


def snap_inputs(B, Hb, seed):
    """Inputs of the snap / NONE / shared-half launches: the PlotQA regressor (fusion.6 [256] -> 1).  Row kinds (b % 4): ordinary,
    needs = 0, target 0 with a small r (z = 2^-8: r scale <= 0.4 snaps to a table's 0.0), |target| > 1.  The scales differ by row: 40 divides
    back exactly for every DVQA integer, 47 / 49 / 100 do not (fl(fl(k / s) s) != k for some k)."""
    g = torch.Generator().manual_seed(seed)
    inp = cls_inputs(B, Hb, g)
    fh = torch.nn.functional.leaky_relu(torch.randn(B, 256, generator=g) * 0.7, 0.01)
    w6 = torch.randn(256, generator=g) * 0.08
    w6[0], b6 = 0.5, torch.tensor([0.0625])
    kinds = torch.arange(B) % 4
    small = kinds == _S_SNAP0
    fh[small] = 0.0
    fh[small, 0] = -0.1171875                    # z = 0.0625 - 0.05859375 = 2^-8 exactly
    inp.update(fh=fh.to(torch.bfloat16), w6=w6, b6=b6, kinds=kinds, g=g, scale=torch.tensor([40.0, 47.0, 49.0, 100.0])[(torch.arange(B) // 4) % 4])
    return inp


def snap_targets(inp, rp, hc, seed):
    """R [B, 4] for predictions rp (fp32, already snapped): ordinary targets keep 1e-3 away from every comparison boundary."""
    rng = np.random.default_rng(seed)
    kinds, scale = inp["kinds"].tolist(), inp["scale"].numpy()
    B, tol = len(kinds), hc["tol"]
    R = np.zeros((B, 4), F32)
    for b, kind in enumerate(kinds):
        s, r = F32(scale[b]), float(rp[b])
        if kind == _S_SNAP0:
            R[b] = (0.0, 1.0, tol, s)
            continue
        while True:
            t = float(rng.uniform(1.05, 3.0)) * (1 if b % 8 < 4 else -1) if kind == _S_BIG else r + float(rng.uniform(-1.2, 1.2))
            t32 = float(F32(F32(t * s) / s))
            l1 = abs(r - t32)
            if (abs(abs(t32) - 1) > 1e-3 and abs(t32) > 1e-3 and abs(l1 - 0.5) > 1e-3 and abs(l1 - tol) > 1e-3 * max(tol, 1e-3)
                    and abs(l1 / abs(t32) - 0.05) > 1e-3):
                break
        R[b] = (F32(t * s), 0.0 if kind == _S_NEEDS0 else 1.0, tol, s)
    return torch.from_numpy(R)


def tie_tables(x):
    """Four tables for x = fl(r scale) of one row: entries x - d and x + d (d a power of two, both fp32 distances equal) in either order,
    once at the head of the table and once between far entries.  Returns ((table, index of the entry that must win), ...)."""
    x = F32(x)
    for e in range(-3, -20, -1):
        d = F32(2.0 ** (np.floor(np.log2(abs(float(x)))) + e))
        lo, hi = F32(x - d), F32(x + d)
        if float(lo) == float(x) - float(d) and float(hi) == float(x) + float(d) and np.abs(F32(lo - x)) == np.abs(F32(hi - x)) == d:
            far = [F32(x + 5), F32(x - 7)]
            return (([far[0], lo, hi, far[1]], 1), ([far[0], hi, lo, far[1]], 1), ([lo, hi] + far, 0), ([hi, lo] + far, 0))
    raise AssertionError("no power of two makes an exact tie at x = %r" % float(x))


def snap_tie_row(r, inp):
    """The row the tie tables are built on: the first ordinary row whose product r scale is inexact in fp32, so that a distance taken
    from the unrounded product (a multiply fused into the subtraction) is no tie; row 0 if there is none."""
    r = np.asarray(r, F32)
    s = inp["scale"].numpy()
    for b in np.nonzero((inp["kinds"] == _S_PLAIN).numpy())[0]:
        if float(F32(r[b] * s[b])) != float(r[b]) * float(s[b]):
            return int(b)
    return 0


def check_tie_table(table, x, win):
    """Both entries at the same fp32 distance, smaller than every other entry's; `win` is the first of the two."""
    tab, x = np.asarray(table, F32), F32(x)
    d = np.abs(tab - x).astype(F32)
    order = np.argsort(d, kind="stable")
    assert d[order[0]] == d[order[1]] and d[order[1]] < d[order[2]], d
    assert win == min(order[0], order[1]) and tab[order[0]] != tab[order[1]]


def snap_tables(r, inp):
    """The tables of the snap test from the kernel's r: DVQA, the same shuffled, one entry, three entries, and the four tie tables
    built on the row snap_tie_row names.  Returns (tie row, [(name, table, expected index for the tie row or None)])."""
    rng = np.random.default_rng(11)
    b = snap_tie_row(r, inp)
    x = F32(F32(r[b]) * F32(inp["scale"][b]))
    ties = [(n, [float(v) for v in t], w) for n, (t, w) in zip(("tie_low_first", "tie_high_first", "tie_low_at_head", "tie_high_at_head"),
                                                                 tie_tables(x))]
    return b, [("dvqa", list(DVQA_FLOATS), None), ("shuffled", [DVQA_FLOATS[i] for i in rng.permutation(CE_CLASSES)], None),
               ("one", [5.0], None), ("three", [7.0, 0.0, -3.0], None)] + ties


SELECT_COUNTS = (0, 1, 2, 63, 64, 65, 200)


def select_inputs(Q, seed):
    """Candidate rows for Q questions.  Counts cycle through SELECT_COUNTS; drawn rows have l0 - l1 in [-6, 6] and a per-question fp64
    top-2 margin of p0 of at least 1e-4.  Ties are bit-exact copies of the best row's logits or that row shifted by 8 (exact): the
    copy sits at j + 64 (same lane), j + 1 (next lane) or before j.  One question saturates to p0 = 1 on every row, one to 0.
    The gathered buffers hold distinct integers.  Returns a dict; `special` names the constructed questions."""
    rng = np.random.default_rng(seed)
    if Q == 1:
        counts = [1]
    else:
        counts = [SELECT_COUNTS[i % len(SELECT_COUNTS)] for i in range(Q)]
    special, rows = {}, []
    big = [q for q, n in enumerate(counts) if n == 200]
    plan = {}
    if Q > 1:
        plan = {big[0]: "tie_same_lane", big[1]: "tie_next_lane", big[2]: "tie_before", big[3]: "sat_one", big[4]: "sat_zero",
                big[5]: "tie_shifted_same_lane", big[6]: "tie_shifted_before"}
    for q, n in enumerate(counts):
        diff = np.round(rng.uniform(-6, 6, n) * 64) / 64
        base = np.round(rng.uniform(-3, 3, n) * 64) / 64
        kind = plan.get(q)
        if n >= 2 and kind not in ("sat_one", "sat_zero"):
            j = int(rng.integers(0, n)) if kind is None else {"tie_same_lane": 70, "tie_next_lane": 70, "tie_before": 150,
                                                                "tie_shifted_same_lane": 3, "tie_shifted_before": 199}[kind]
            diff[j] = 6.0
            others = np.arange(n) != j
            diff[others] = np.minimum(diff[others], 5.5)          # p0 margin: sigmoid(6) - sigmoid(5.5) = 1.6e-3
        lg = np.stack([base + diff, base], 1)
        if kind == "sat_one":
            lg = np.stack([base + 40.0, base], 1)
        elif kind == "sat_zero":
            lg = np.stack([base - 120.0, base], 1)
        elif kind is not None:
            shift = {"tie_shifted_same_lane": 8.0, "tie_shifted_before": -8.0}.get(kind, 0.0)     # the later row has the larger raw l0
            k = {"tie_same_lane": j + 64, "tie_next_lane": j + 1, "tie_before": 17, "tie_shifted_same_lane": j + 128,
                 "tie_shifted_before": 4}[kind]
            lg[k] = lg[j] + shift
            special[kind] = (q, min(j, k))
        if kind in ("sat_one", "sat_zero"):
            special[kind] = (q, 0)
        rows.append(lg)
    logits = np.concatenate(rows, 0).astype(F32) if rows else np.zeros((0, 2), F32)
    N = logits.shape[0]
    assert N < 2 ** 20
    ids = rng.permutation(3 * N).astype(F32)
    return dict(logits=logits, num_ans=np.array(counts, np.int64), reg_out=ids[:N] + 1, reg_err=ids[N:2 * N] + 1, reg_terr=ids[2 * N:] + 1,
                special=special, plan=plan)


def select_variants(case):
    """The launches of the GPU selection test: (name, kwargs for select_ref64 / emu_select[, expected answers])."""
    lg, na = case["logits"], case["num_ans"]
    Q = na.shape[0]
    base = dict(logits=lg, reg_out=case["reg_out"], reg_err=case["reg_err"], reg_terr=case["reg_terr"], num_ans=na)
    out = [("plain", dict(base))]
    if Q > 1:
        nan = lg.copy()
        offs = np.concatenate([[0], np.cumsum(na)])
        qs = [q for q in range(Q) if na[q] == 200 and q not in case["plan"]]
        q1, q2, q3 = qs[0], qs[1], qs[2]
        nan[offs[q1] + 130, 0] = np.nan                   # one NaN row (not the numeric best): it must be chosen
        nan[offs[q2]:offs[q2 + 1], 1] = np.nan            # every row NaN: row 0
        nan[offs[q3] + 70, 0] = np.nan                    # two NaN rows, same lane (70, 134) and an earlier lane's later row (5 + 64)
        nan[offs[q3] + 134, 1] = np.nan
        nan[offs[q3] + 69, 0] = np.nan
        out.append(("nan", dict(base, logits=nan), {q1: 130, q2: 0, q3: 69}))
        qs = max(q for q in range(Q) if na[q] == 200)     # it straddles N (70 rows below), the questions after it lie beyond
        cut = int(offs[qs] + 70)
        assert qs < Q - 2 and int(na[qs + 1:].sum()) > 0
        out.append(("short_N", dict(base, N=cut)))
        pad = lambda x, v: np.concatenate([x, np.full((37,) + x.shape[1:], v, x.dtype)])          # noqa: E731
        out.append(("extra_rows", dict(base, logits=pad(lg, 0.5), reg_out=pad(case["reg_out"], -1), reg_err=pad(case["reg_err"], -2),
                                       reg_terr=pad(case["reg_terr"], -3))))          # sum(num_ans) < N: 37 rows no question owns
        forced = np.array([(0, n, -1, n - 1, 7)[q % 5] if n else (0, 3, -1)[q % 3] for q, n in enumerate(na.tolist())], np.int64)
        out.append(("forced", dict(base, forced=forced)))
    return out
